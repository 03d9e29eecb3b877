"""Checks of the CPU restatement the post-tune GPU tests are held to (tests/post_tune_ref.py), against the reference's own
code where the reference tree is present: the face term carries no gradient, the head rectangle, the sample builder."""
import importlib
import types

import pytest
import torch

from oracle import reference_loader, torch_ref
from tests import helpers
from tests import post_tune_ref as ref

needs_reference = pytest.mark.skipif(not reference_loader.available(), reason="the reference tree is not present")


def _case(size=32):
    gsd = torch_ref.state_dict_from_numpy(helpers.generator_state_dict(seed=2, affine="random"))
    sample = ref.sample_batch(seed=5, n=1, size=size, nf=12)
    bg = torch.rand(1, 3, size, size, generator=torch.Generator().manual_seed(9)) * 2 - 1
    back_head = 1 - ref.TableRender(12, seed=3).encode_front_fim(sample["tsf_fim"], front_fn=False)
    return gsd, sample, bg, back_head


def test_fid_term_carries_no_gradient():
    """FaceLoss.compute_loss detaches its SECOND argument (networks/networks.py:284) and post_personalize passes the generated
    image second (models/imitator.py:445-446): the term is a readout.  Exactly zero for every parameter, not small."""
    gsd, sample, bg, back_head = _case()
    fsd = helpers.sphere20a_state_dict(seed=4)
    params = {k: v.clone().requires_grad_(True) for k, v in gsd.items()}
    _, terms, images = ref.step_loss(params, sample, bg, back_head, fsd=fsd)
    fid = terms["fid"]
    assert float(fid) > 0
    if fid.requires_grad:     # (it does not: nothing with a graph reaches it)
        grads = torch.autograd.grad(fid, list(params.values()), allow_unused=True, retain_graph=True)
        assert all(g is None or not bool(g.any()) for g in grads)
    # the gradient of the total is the same with and without the term, bit for bit
    with_fid = torch.autograd.grad(terms["total"], list(params.values()), allow_unused=True)
    total, _, _ = ref.step_loss(params, sample, bg, back_head)
    without = torch.autograd.grad(total, list(params.values()), allow_unused=True)
    for k, a, b in zip(params, with_fid, without):
        assert (a is None and b is None) or torch.equal(a, b), k
    # ... and it is the argument order that does it: generated image first, and the term has a gradient
    swapped = ref.face_term(fsd, images["cyc_tsf"], sample["images"][:, 0], sample["j2d"][:, 0])
    assert swapped.requires_grad


@needs_reference
def test_head_rect_equals_the_reference():
    from impersonator_amd.models.generator_trainer import head_rect
    live = reference_loader.load().networks.FaceLoss.find_head_rect
    g = torch.Generator().manual_seed(1)
    for scale in (0.3, 0.8, 1.3):          # 1.3: joints outside the image, the clamps act
        kps = (torch.rand(5, 19, 2, generator=g) * 2 - 1) * scale
        for h, w in ((64, 64), (128, 96)):
            want = live(kps, h, w)
            assert torch.equal(ref.find_head_rect(kps, h, w), want)
            assert torch.equal(head_rect(kps, h, w), want)


@needs_reference
def test_sample_builder_equals_the_reference_preprocess():
    """tests/post_tune_ref.py::preprocess against the live PairSampleDataset.preprocess (data/dataset.py:249-324), called
    unbound on a stand-in for the dataset object (its constructor reads asset files)."""
    reference_loader.load()
    try:
        dataset = importlib.import_module("data.dataset")
    except Exception as e:     # a module of the reference that the loader's stubs do not cover
        pytest.skip("data/dataset.py of the reference does not import here (%s); restated lines: data/dataset.py:269-304" % e)
    size = 32
    g = torch.Generator().manual_seed(2)
    images = torch.rand(2, 3, size, size, generator=g) * 2 - 1
    fims = torch.cat([torch.rand(2, 2, size, size, generator=g), (torch.rand(2, 1, size, size, generator=g) > 0.4).float()], dim=1)
    T = torch.rand(size, size, 2, generator=g) * 2.4 - 1.2
    sample = dict(images=images, fims=fims, T=T, j2d=torch.zeros(2, 19, 2), src_fim=torch.zeros(size, size), tsf_fim=torch.zeros(size, size))
    this = types.SimpleNamespace(bg_ks=13, ft_ks=3, bg_kernel=torch.ones(1, 1, 13, 13), ft_kernel=torch.ones(1, 1, 3, 3), is_both=False)
    want = dataset.PairSampleDataset.preprocess(this, dict(sample))
    got = ref.preprocess(images, fims, T, ft_ks=3)
    for k in ("src_inputs", "tsf_inputs", "pseudo_masks"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(want["images"], images) and torch.equal(want["T"], T)
