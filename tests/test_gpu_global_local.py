"""GPU: the body-crop kernel (lwg_crop_resize and its adjoint) against fp64 F.interpolate / autograd on the CPU, and the
GlobalLocalDiscriminator (forward, optimize_D, input_grad) against numbers from the live reference in fp64
(tests/golden/make_global_local_golden.py), in both arithmetic modes of the convolutions.  S = 64, N = 3: the smallest size four
stride-2 layers allow, with a box touching the right and bottom edges, a 2x2 corner and a one-pixel-wide column.
Every test prints the figures it compares before it asserts (run with -s); DESIGN.md section 7 keeps the observed ratios."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers

pytestmark = pytest.mark.gpu

S, N = 64, 3
RECTS = [[10, 50, 4, 64], [0, 2, 0, 2], [31, 32, 5, 60]]
FULL = [0, S, 0, S]
LR = 0.0002


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)


def _crop_ref(x, rects):
    """GlobalLocalDiscriminator.crop_body (networks/discriminator.py:80-96), restated on whatever dtype x has."""
    out = []
    for i, (x0, x1, y0, y1) in enumerate(rects):
        out.append(F.interpolate(x[i:i + 1, :, y0:y1, x0:x1], size=(x.shape[2], x.shape[3]), mode='bilinear', align_corners=True))
    return torch.cat(out, 0)


def _outside(rects, C):
    m = torch.ones(len(rects), C, S, S, dtype=torch.bool)
    for i, (x0, x1, y0, y1) in enumerate(rects):
        m[i, :, y0:y1, x0:x1] = False
    return m


# ---- op level ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[6, 4])
def op(request):
    """Inputs, the device results and the fp64 references of one channel count, computed once."""
    from impersonator_amd import ops
    C, rects = request.param, RECTS + [FULL]
    gen = torch.Generator().manual_seed(20 + C)
    x = torch.rand(len(rects), C, S, S, generator=gen) * 2 - 1
    dy = torch.rand(len(rects), C, S, S, generator=gen) * 2 - 1
    boxes = torch.tensor(rects, dtype=torch.int64).cuda()
    out = ops.crop_resize(x.cuda(), boxes).cpu()
    dx = ops.crop_resize_backward(dy.cuda(), boxes).cpu()
    dx2 = ops.crop_resize_backward(dy.cuda(), boxes).cpu()
    xr = x.double().requires_grad_(True)
    ref = _crop_ref(xr, rects)
    ref_dx, = torch.autograd.grad(ref, xr, dy.double(), retain_graph=True)
    ref_abs, = torch.autograd.grad(ref, xr, dy.double().abs())       # the same adjoint applied to |dy|: the error's yardstick
    return dict(C=C, rects=rects, x=x, dy=dy, out=out, dx=dx, dx2=dx2, ref=ref.detach(), ref_dx=ref_dx, ref_abs=ref_abs)


def test_crop_forward_against_fp64_interpolate(op):
    """Bound (S*2^-21 + 2^-21) * max|x|: src carries at most 2^-23*S absolute error per axis in fp32, a weight error d moves the
    output by at most 2*d*max|x|, two axes; the rest is the rounding of four products and three adds."""
    bound = (S * 2.0 ** -21 + 2.0 ** -21) * float(op["x"].abs().max())
    err = float((op["out"].double() - op["ref"]).abs().max())
    print("crop forward C=%d: max err %.3g, bound %.3g, ratio %.3f" % (op["C"], err, bound, err / bound))
    assert err <= bound


def test_crop_full_box_is_the_identity_bit_for_bit(op):
    assert torch.equal(op["out"][3], op["x"][3])            # scale = 1, lambda = 0


def test_crop_backward_against_fp64_autograd(op):
    """Per element (S*2^-21 + K*2^-24) * A, A the same adjoint applied to |dy| in fp64, K = S^2 the largest number of outputs
    that feed one source pixel (the 2x2 box): the worst-case form tests/test_gpu_hmr.py uses."""
    bound = (S * 2.0 ** -21 + S * S * 2.0 ** -24) * op["ref_abs"]
    err = (op["dx"].double() - op["ref_dx"]).abs()
    inside = op["ref_abs"] > 0
    print("crop backward C=%d: worst err/bound %.3g" % (op["C"], float((err[inside] / bound[inside]).max())))
    assert bool((err <= bound).all())
    assert float(op["dx"][_outside(op["rects"], op["C"])].abs().max()) == 0.0     # exactly 0.0 outside each box
    assert torch.equal(op["dx"], op["dx2"])                                        # bit-reproducible


def test_crop_backward_is_the_adjoint_of_the_forward(op):
    lhs = float((op["out"].double() * op["dy"].double()).sum())
    rhs = float((op["x"].double() * op["dx"].double()).sum())
    print("crop adjoint C=%d: <crop(x),g> %.9g, <x,crop^T(g)> %.9g" % (op["C"], lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_crop_empty_box_gives_zeros_both_ways():
    from impersonator_amd import ops
    boxes = torch.tensor([[5, 5, 0, 10], FULL], dtype=torch.int64).cuda()
    x = (torch.rand(2, 6, S, S, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    out, dx = ops.crop_resize(x, boxes), ops.crop_resize_backward(x, boxes)
    assert float(out[0].abs().max()) == 0.0 and float(dx[0].abs().max()) == 0.0
    assert torch.equal(out[1], x[1]) and torch.equal(dx[1], x[1])


# ---- network level -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = helpers.golden("global_local_golden.npz")
    keys = [str(k) for k in g["keys"]]
    gen = torch.Generator().manual_seed(1)
    xs = [torch.rand(N, c, S, S, generator=gen) * 2 - 1 for c in (4, 6, 4, 6)]   # real_global, real_local, fake_global, fake_local
    sd = {"global_model." + k: v for k, v in helpers.discriminator_state_dict(seed=7, input_nc=4).items()}
    sd.update({"local_model." + k: v for k, v in helpers.discriminator_state_dict(seed=8, input_nc=6).items()})
    assert g["rects"].tolist() == RECTS
    zero = {"%s.model.%d.bias" % (b, i) for b in ("global_model", "local_model") for i in (2, 5, 8, 11)}
    return dict(g=g, keys=keys, strides=dict(zip(keys, g["strides"].tolist())), xs=xs, sd=sd, zero=zero)


def _make(gold, precision, sd=None):
    from impersonator_amd.networks.discriminator import GlobalLocalDiscriminator
    D = GlobalLocalDiscriminator(6, 64, 4, 'instance', False, image_size=S, max_batch=N, conv_precision=precision)
    D.load_state_dict(sd if sd is not None else gold["sd"])
    return D.cuda()


@pytest.fixture(scope="module", params=["fp32", "bf16x3"])
def net(request, gold):
    D = _make(gold, request.param)
    yield D
    D.release()


def test_forward_matches_the_reference(gold, net):
    rg, rl, fg, fl = [x.cuda() for x in gold["xs"]]
    boxes = torch.tensor(RECTS, dtype=torch.int64).cuda()
    for name, out in (("d_real", net(rg, rl, boxes)), ("d_fake", net(fg, fl, RECTS))):       # device boxes; host list
        ref = torch.from_numpy(gold["g"][name])
        assert out.shape == ref.shape == (2 * N, 1, 2, 2)
        print("forward %s %s: rel %.3g (bound 1e-4)" % (net.conv_precision, name, _rel(out.cpu().double(), ref)))
        assert _rel(out.cpu().double(), ref) < 1e-4


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_optimize_D_matches_the_reference(gold, precision):
    D = _make(gold, precision)                      # a fresh model: the update moves the parameters
    g = gold["g"]
    rg, rl, fg, fl = [x.cuda() for x in gold["xs"]]
    loss = D.optimize_D(rg, rl, fg, fl, torch.tensor(RECTS, dtype=torch.int64).cuda(), lr=LR, betas=(0.5, 0.999),
                        all_reduce=False)
    ref_loss = float(g["loss"][0])
    print("optimize_D %s: loss %.9g vs %.9g" % (precision, float(loss), ref_loss))
    assert abs(float(loss) - ref_loss) < 1e-5 * abs(ref_loss)
    mine = D.gradients()
    assert list(mine) == gold["keys"]
    worst = 0.0
    for k in gold["keys"]:
        v, st = mine[k].double(), gold["strides"][k]
        if k in gold["zero"]:
            # InstanceNorm cancels the bias in front of it: the reference's gradient is ~1e-14, ours pure round-off
            assert float(g["gnorm/" + k][2]) < 1e-5 and float(v.abs().max()) < 1e-5, k
            continue
        sample, norms = torch.from_numpy(g["gsample/" + k]), g["gnorm/" + k]
        rel = _rel(v.flatten()[::st], sample)
        worst = max(worst, rel)
        assert rel < 2e-3, (k, rel)
        assert abs(float(v.abs().sum()) - norms[0]) <= 2e-3 * norms[0], k
        assert abs(float((v * v).sum().sqrt()) - norms[1]) <= 2e-3 * norms[1], k
    print("optimize_D %s: worst per-tensor gradient rel %.3g (bound 2e-3)" % (precision, worst))
    D.pull_parameters()
    if precision == "fp32":     # as tests/test_gpu_discriminator.py::test_loss_gradients_and_adam_steps: fp32 only
        sd = D.state_dict()
        for k in gold["keys"]:
            if k in gold["zero"]:
                continue        # Adam normalises round-off gradients to +-lr: not comparable
            st = gold["strides"][k]
            gs = np.abs(g["gsample/" + k])
            big = torch.from_numpy(gs > 1e-2 * g["gnorm/" + k][2])
            diff = (sd[k].cpu().double().flatten()[::st] - torch.from_numpy(g["psample/" + k])).abs()
            if bool(big.any()):
                assert float(diff[big].max()) < 0.2 * LR, k
            assert float(diff.max()) < 2.1 * 2 * LR, k
    D.release()


def test_input_grad_matches_the_reference(gold, net):
    g = gold["g"]
    _, _, fg, fl = [x.cuda() for x in gold["xs"]]
    loss, d_global, d_local = net.input_grad(fg, fl, torch.tensor(RECTS, dtype=torch.int64).cuda(), target=0.0)
    ref_loss = float(g["g_loss"][0])
    assert abs(float(loss) - ref_loss) < 1e-5 * abs(ref_loss)
    assert d_global.shape == fg.shape and d_local.shape == fl.shape
    for name, d in (("d_global", d_global), ("d_local", d_local)):
        rel = _rel(d.cpu().double().flatten()[::13], torch.from_numpy(g["isample/" + name]))
        print("input_grad %s %s: rel %.3g (bound 1e-3)" % (net.conv_precision, name, rel))
        assert rel < 1e-3
        norms = g["inorm/" + name]
        assert abs(float(d.double().abs().sum()) - norms[0]) <= 1e-3 * norms[0]
    assert float(d_local.cpu()[_outside(RECTS, 6)].abs().max()) == 0.0
    # the discriminator's parameters got no gradient from this call: nothing to compare, but the update above must not depend on it


def _ulp(t):
    a = t.abs()
    return torch.nextafter(a, torch.full_like(a, float("inf"))) - a


def test_loss_scale_halves_every_gradient(gold):
    """Both branches on the same 6-channel weights and inputs (the global branch's first layer and input sliced to 4 channels), the
    local branch with a full-image box (the crop is then the identity): each handle's gradient buffer under loss_scale = 0.5 must be
    half of what the unscaled entry point leaves in a plain PatchDiscriminator, within 1 ulp per element."""
    from impersonator_amd.networks.discriminator import PatchDiscriminator
    sd6 = helpers.discriminator_state_dict(seed=8, input_nc=6)
    sd4 = dict(sd6)
    sd4["model.0.weight"] = sd6["model.0.weight"][:, :4].contiguous()
    sd = {"global_model." + k: v for k, v in sd4.items()}
    sd.update({"local_model." + k: v for k, v in sd6.items()})
    real, fake = gold["xs"][1].cuda(), gold["xs"][3].cuda()
    D = _make(gold, "fp32", sd)
    loss = D.optimize_D(real[:, :4].contiguous(), real, fake[:, :4].contiguous(), fake, [FULL] * N, all_reduce=False)
    (_, gg), (_, gl) = D.flat_buffers()
    total = 0.0
    for nc, sdp, mine in ((4, sd4, gg), (6, sd6, gl)):
        P = PatchDiscriminator(nc, 64, 4, 'instance', False, image_size=S, max_batch=N)
        P.load_state_dict(sdp)
        P = P.cuda()
        total += float(P.optimize_D(real[:, :nc].contiguous(), fake[:, :nc].contiguous(), all_reduce=False))
        full = P.flat_buffers()[1]
        assert mine.shape == full.shape and float(full.abs().max()) > 0
        assert bool(((mine - 0.5 * full).abs() <= _ulp(0.5 * full)).all()), nc
        print("loss_scale %d-channel branch: %d of %d entries differ from half" % (nc, int((mine != 0.5 * full).sum()), mine.numel()))
        P.release()
    assert abs(float(loss) - 0.5 * total) <= 1e-6 * abs(total)
    D.release()


def test_graph_replay_reads_the_boxes_on_the_device(gold):
    """forward + input_grad captured once, replayed after the box tensor was overwritten in place: bit for bit the eager result on
    the new boxes.  What a host-side crop (boxes.tolist(), one interpolate per sample) cannot do."""
    D = _make(gold, "fp32")
    _, _, fg, fl = [x.cuda() for x in gold["xs"]]
    boxes = torch.tensor(RECTS, dtype=torch.int64).cuda()
    D(fg, fl, boxes), D.input_grad(fg, fl, boxes)            # warm-up: every lazily allocated buffer exists afterwards
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one stream, no parallel branches
        out = D(fg, fl, boxes)
        loss, d_global, d_local = D.input_grad(fg, fl, boxes)
    rotated = [RECTS[0], RECTS[2], RECTS[1]]
    boxes.copy_(torch.tensor(rotated, dtype=torch.int64))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (out, loss, d_global, d_local)]
    ref = [D(fg, fl, boxes)] + list(D.input_grad(fg, fl, boxes))
    first = [D(fg, fl, RECTS)] + list(D.input_grad(fg, fl, RECTS))
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], first[0]) and not torch.equal(got[3], first[3])     # the new boxes did reach the replay
    del graph
    D.release()
