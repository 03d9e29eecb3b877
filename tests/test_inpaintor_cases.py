"""CPU side of the inpaintor tests: proofs of the attention test cases of tests/helpers.py (what tests/test_gpu_inpaintor.py runs on the kernels): the one-hot case
is exact in fp32, the random cases are peaked, and each of four indexing bugs would move the output by >= 100 x the GPU tolerance."""
import pytest
import torch

from tests import helpers

SIZES = sorted(helpers.ATTN_PRODUCT_CHUNKS)   # 256, 1024, 2304, 4096 tokens
PEAKED = (2.0, 8.0)


@pytest.mark.parametrize("N,winners", [(256, "perm"), (2304, "perm"), (4096, "perm"), (1024, "first"), (1024, "last")])
def test_onehot_case_is_exact_in_fp32(N, winners):
    case = helpers.attention_onehot_case(N, winners)
    logits, v = helpers.attention_parts(case, torch.float32)
    top = logits.topk(2, dim=-1)
    assert torch.equal(top.indices[:, 0], case["perm"])
    assert float(top.values[:, 0].min()) == 768.0 == float(top.values[:, 0].max()) and float(top.values[:, 1].max()) <= 640.0
    p = torch.softmax(logits, -1)
    onehot = torch.zeros_like(p)
    onehot[torch.arange(N), case["perm"]] = 1.0
    assert torch.equal(p, onehot)                                    # every other probability underflows to exactly 0
    assert torch.equal(helpers.attention_reference(case, torch.float32), case["expected"])
    assert torch.equal(helpers.attention_reference(case).float(), case["expected"])
    # the bias add is exercised (no zero bias) and exact: raw + bias gives the +-64 / +-1 / grid targets back
    assert int((case["bias"][:160] != 0).sum()) > 140
    t = case["qkv"] + case["bias"]
    assert set(t[:, :12].abs().unique().tolist()) == {64.0} and set(t[:, 16:28].abs().unique().tolist()) == {1.0}
    if winners == "first":
        assert int(case["perm"].max()) < helpers.ATTN_TILE
    if winners == "last":
        assert int(case["perm"].min()) >= N - helpers.ATTN_TILE


@pytest.mark.parametrize("N", SIZES)
def test_random_cases_are_peaked_and_every_mutation_is_100x_the_tolerance(N):
    """The condition of the peaked cases (median effective key count <= N/8 on the fp64 reference; the flat case keeps > N/2), and the
    sensitivity of the GPU check: each mutant of the fp64 reference moves the output by >= 100 x (ATTN_TOL_FACTOR x yardstick), the
    bound tests/test_gpu_inpaintor.py holds the kernels to.  Measured: moves of 0.37 to 10.3 absolute (4.9e4 to 1e6 x the tolerance)
    against tolerances of 4.3e-6 to 3.0e-5."""
    flat = helpers.attention_checked_case(N, 0.05)
    assert float(helpers.effective_keys(helpers.attention_parts(flat)[0]).median()) > N / 2
    for std in PEAKED:
        case = helpers.attention_checked_case(N, std)
        logits, _ = helpers.attention_parts(case)
        eff = float(helpers.effective_keys(logits).median())
        tol = helpers.ATTN_TOL_FACTOR * case["yardstick"]
        print("N=%d logit std %.2f (asked %.2f): median effective keys %.1f, fp32 yardstick %.3g" %
              (N, float(logits.std()), std, eff, case["yardstick"]))
        assert eff <= N / 8
        assert 0 < tol < 1e-4
        for which in ("pair", "tiles", "chunk", "rescale"):
            moved = float((helpers.attention_mutant(case, which, helpers.ATTN_PRODUCT_CHUNKS[N]) - case["ref"]).abs().max())
            print("    %-8s moves the output by %.3g = %.3g x tolerance" % (which, moved, moved / tol))
            assert moved >= 100 * tol, (N, std, which, moved, tol)


def test_split_bf16_decode_inverts_the_layout():
    g = torch.Generator().manual_seed(3)
    r = torch.randn(64, 128, generator=g)
    hi, lo = helpers.split_bf16_encode(r)
    # the layout of split_bf16_groups (csrc/conv.h): per 32 values, 32 bf16 hi then 32 bf16 lo in the 128 bytes they took as fp32
    buf = torch.stack([hi.view(64, 4, 32), lo.view(64, 4, 32)], dim=2).reshape(64, 256).view(torch.float32)
    assert buf.shape == r.shape
    dhi, dlo = helpers.split_bf16_decode(buf)
    assert torch.equal(dhi, hi) and torch.equal(dlo, lo)
    assert float((hi.float() + lo.float() - r).abs().max()) <= 2.0 ** -16 * float(r.abs().max())


def test_forward_refuses_another_image_size_before_any_launch():
    """A 128 x 128 tensor into a 256 x 256 module used to run: the kernels read past the end of the smaller buffers.  The check comes
    first in forward(): no handle is made and nothing is launched (CPU tensors, no device needed)."""
    from impersonator_amd.networks.inpaintor import InpaintSANet
    net = InpaintSANet(c_dim=4, image_size=256).eval()
    with pytest.raises(ValueError, match="256"):
        net(torch.zeros(1, 3, 128, 128), torch.zeros(1, 1, 128, 128))
    with pytest.raises(ValueError, match="masks"):
        net(torch.zeros(1, 3, 256, 256), torch.zeros(1, 1, 128, 128))
    with pytest.raises(ValueError, match="masks"):
        net(torch.zeros(1, 3, 256, 256), torch.zeros(1, 3, 256, 256))
    with pytest.raises(ValueError):
        net(torch.zeros(2, 3, 256, 256), torch.zeros(2, 1, 256, 256))
    assert net._handle is None
