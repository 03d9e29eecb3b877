"""What GeneratorTrainer and PostTuner share (impersonator_amd/models/generator_trainer.py), without a GPU: the device layout
of the parameters as a function of the state_dict's shapes, the parameter store on the CPU, and the one head rectangle."""
import types

import pytest
import torch

from impersonator_amd.models.generator_trainer import HEAD_ROWS, GeneratorParams, head_rect, param_layout
from impersonator_amd.networks.generator import ImpersonatorGenerator

HEADS = ("heads:bg", "heads:src_model", "heads:tsf_model")


@pytest.fixture(scope="module")
def generator():
    torch.manual_seed(1)
    G = ImpersonatorGenerator(bg_dim=4, src_dim=6, tsf_dim=6, repeat_num=1, image_size=64, max_batch=1)
    with torch.no_grad():
        for p in G.parameters():
            p.uniform_(-1, 1)     # no tensor is all zero: a padding entry cannot pass for a copied one
    return G


def test_layout_covers_every_tensor_once_in_contiguous_ranges(generator):
    sd = generator.state_dict()
    spec = param_layout({k: tuple(v.shape) for k, v in sd.items()}, generator.repeat_num)
    placed = [sk for _, _, parts in spec for sk, _, _ in parts]
    assert sorted(placed) == sorted(sd) and len(set(placed)) == len(placed)          # every trainable tensor, exactly once
    shapes = {key: shape for key, shape, _ in spec}
    assert len(shapes) == len(spec)                                                   # device keys are unique
    assert [shapes[k] for k in HEADS] == [(HEAD_ROWS, 64, 7, 7)] * 3 and HEAD_ROWS == 8
    assert sum(k.startswith("heads:") for k in shapes) == 3
    stems = ["bg_model.model.0.weight", "src_model.encoders.0.0.weight", "tsf_model.encoders.0.0.weight"]
    for k in stems:
        assert shapes[k] == (sd[k].shape[0], 8, 7, 7) and sd[k].shape[1] in (4, 6), k
    assert sorted(k for k, s in shapes.items() if len(s) == 4 and s[2] == 7) == sorted(stems + list(HEADS))
    for key, shape, parts in spec:                                                    # everything else keeps its shape
        if key not in stems and not key.startswith("heads:"):
            assert parts == [(key, None, None)] and shape == tuple(sd[key].shape), key

    store = GeneratorParams(generator, device="cpu")
    n = store.flat_p.numel()
    assert [k for k, _, _ in store._ranges] == [k for k, _, _ in spec]
    assert store._ranges[0][1] == 0 and store._ranges[-1][2] == n == sum(torch.Size(s).numel() for s in shapes.values())
    for (k, lo, hi), (_, nxt, _) in zip(store._ranges, store._ranges[1:] + [(None, n, None)]):
        assert hi - lo == torch.Size(shapes[k]).numel() > 0 and hi == nxt, k          # contiguous, and they tile [0, n)
    # what PostTuner._lo rests on: from the first range that is not BGNet's on, the keys are exactly the two streams'
    is_bg = [k.startswith("bg_model.") or k == "heads:bg" for k, _, _ in store._ranges]
    first = is_bg.index(False)
    assert first > 0 and all(is_bg[:first]) and not any(is_bg[first:])
    assert all(k.startswith(("src_model.", "tsf_model.", "heads:src_model", "heads:tsf_model")) for k, _, _ in store._ranges[first:])


def test_store_round_trip_padding_and_first_write(generator):
    sd = generator.state_dict()
    store = GeneratorParams(generator, device="cpu")
    assert all(t.device.type == "cpu" and t.dtype == torch.float32 for t in (store.flat_p, store.flat_g, store.flat_m, store.flat_v))
    out = store.state_dict()
    assert sorted(out) == sorted(sd)
    for k, v in sd.items():
        assert torch.equal(out[k], v), k
    for key, lo, _ in store._ranges:
        p = store.P[key]
        assert p.data_ptr() == store.flat_p[lo:].data_ptr() and store.G[key].data_ptr() == store.flat_g[lo:].data_ptr(), key   # views
        if key.startswith("heads:"):
            rows = 3 if key == "heads:bg" else 4               # colour (+ mask) rows, then zero rows up to HEAD_ROWS
            assert bool((p[:rows] != 0).all()) and not bool(p[rows:].any()), key
        elif p.dim() == 4 and p.shape[2] == 7:
            cin = sd[key].shape[1]                              # 6 (BGNet's stem: 4) input channels, then zero columns up to 8
            assert cin <= 6 and bool((p[:, :cin] != 0).all()) and not bool(p[:, cin:].any()), key
    assert set(store.gradients()) == set(sd) and not any(bool(g.any()) for g in store.gradients().values())

    key = "heads:tsf_model"
    assert store.first_write(key) is None                       # outside a backward pass nothing is handed out
    for _ in range(2):                                          # the second pass: zero_grads hands every slice out again
        store.zero_grads()
        g = store.first_write(key)
        assert g is store.G[key] and g.data_ptr() == store.G[key].data_ptr()
        assert store.first_write(key) is None
        assert store.first_write("src_model.encoders.0.0.weight") is store.G["src_model.encoders.0.0.weight"]
        store.grads_checkpoint()                                # no buckets: nothing to do
        g.fill_(1.0)
    store.zero_grads()
    assert not bool(store.flat_g.any())

    with pytest.raises(ValueError, match="conv_precision"):
        GeneratorParams(generator, conv_precision="fp16", device="cpu")


def test_cal_head_bbox_is_head_rect_of_a_square_image():
    from impersonator_amd.models.impersonator_trainer import BodyRecoveryFlow
    g = torch.Generator().manual_seed(1)
    for scale in (0.3, 0.8, 1.3):          # 1.3: joints outside the image, the clamps at 0 and 1 act
        kps = (torch.rand(5, 19, 2, generator=g) * 2 - 1) * scale
        for size in (64, 200):
            stub = types.SimpleNamespace(_opt=types.SimpleNamespace(image_size=size))
            got = BodyRecoveryFlow.cal_head_bbox(stub, kps)
            assert got.dtype == torch.int64 and torch.equal(got, head_rect(kps, size, size))
            if scale > 1:
                assert bool((got == 0).any()) and bool((got == size).any())
    # the rectangle itself, on joints whose answer can be read off: x, y in [-0.5, 0.5] -> [0.25 - 0.05, 0.75 + 0.05] of the
    # width, [0.25 - 0.05, 0.75] of the height: no margin at the bottom (networks/networks.py:336-364)
    kps = torch.zeros(1, 19, 2)
    kps[0, 12], kps[0, 13] = torch.tensor([-0.5, -0.5]), torch.tensor([0.5, 0.5])
    kps[0, :12] = 5.0                                           # body joints are not read
    assert head_rect(kps, 103, 203).tolist() == [[40, 162, 20, 77]]     # 40.6, 162.4, 20.6, 77.25 truncated
