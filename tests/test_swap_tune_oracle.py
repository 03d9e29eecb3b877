"""CPU checks around the Swapper's fine-tune (impersonator_amd/models/post_tune.py: SwapTuner; the reference's
models/swapper.py:273-476): the learning-rate schedule against the literal transcription of the reference's loop, the
bs == 1 row selection of the helper the GPU tests use (tests/swap_tune_ref.py) against the reference's slicing expressions, and
the argument validation of lwg_adam_update_scheduled, which needs no device."""
import ctypes

import pytest
import torch

from tests import post_tune_ref as ref
from tests import swap_tune_ref as sref


def test_lr_schedule_is_the_reference_loop():
    from impersonator_amd.models.post_tune import SwapTuner
    rates = SwapTuner.lr_schedule()
    assert rates == SwapTuner.lr_schedule(total=50, fix=25, init=2e-4, final=1e-5) == sref.lr_transcription(50, 25, 0.0002, 0.00001)
    assert len(rates) == 50 and all(r == 2e-4 for r in rates[:27])
    assert rates[27] == pytest.approx(1.924e-4, rel=1e-12) and rates[49] == pytest.approx(2.52e-5, rel=1e-12)
    assert len(set(rates)) == 24                                         # the constant stretch + 23 decay steps
    assert all(a > b for a, b in zip(rates[26:], rates[27:]))
    short = SwapTuner.lr_schedule(total=6, fix=2)
    assert short == sref.lr_transcription(6, 2) and short == pytest.approx([2e-4] * 4 + [1.05e-4, 1e-5], rel=1e-12)
    four = SwapTuner.lr_schedule(total=4, fix=1)
    assert four == sref.lr_transcription(4, 1) and four == pytest.approx([2e-4] * 3 + [1e-5], rel=1e-12)


def test_batch_of_one_selection_is_the_reference_slicing():
    """swapper.py:409-421 on the reference's own (flat) tensors against swap_tune_ref.select on the loader's layout."""
    sample = ref.sample_batch(seed=5, n=2, size=16, nf=12)
    init_bg = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1
    # the reference's tensors (set_inputs' return values, :329): images / pseudo_masks flat
    src_imgs = sample["images"][:, 0]
    pseudo_masks = torch.cat([sample["pseudo_masks"][:, 0], sample["pseudo_masks"][:, 1]], dim=0)       # :327
    for step in range(4):
        i = step % 2                                                                                     # :410
        s, bg = sref.select(sample, init_bg, i)
        assert torch.equal(bg, init_bg[i][None])                                                         # :411
        assert torch.equal(s["preds"], sample["preds"][i][None])                                         # :412
        assert torch.equal(s["images"][:, 0], src_imgs[i][None])                                         # :413
        assert torch.equal(s["src_inputs"], sample["src_inputs"][i][None])                               # :414
        assert torch.equal(s["tsf_inputs"], sample["tsf_inputs"][i][None])                               # :415
        assert torch.equal(s["T"], sample["T"][i][None]) and torch.equal(s["T_cycle"], sample["T_cycle"][i][None])   # :416-417
        assert torch.equal(s["src_fim"], sample["src_fim"][i][None]) and torch.equal(s["tsf_fim"], sample["tsf_fim"][i][None])   # :418-419
        # what step_loss makes of the selected masks is the reference's pseudo_masks[i:4:2]
        assert torch.equal(torch.cat([s["pseudo_masks"][:, 0], s["pseudo_masks"][:, 1]], dim=0), pseudo_masks[i:4:2])   # :421
        assert torch.equal(s["j2d"], sample["j2d"][i][None])            # the running sample's own key points (SwapTuner's docstring)


def test_scheduled_adam_argument_validation_without_a_device():
    from impersonator_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    call = lambda a=p, b=p, c=p, d=p, st=p, tab=p, cnt=4: lib.lwg_adam_update_scheduled(a, b, c, d, 16, st, tab, cnt, 0.5, 0.999, 1e-8, None)
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(d=None), dict(st=None), dict(tab=None), dict(cnt=0), dict(cnt=-3)):
        assert call(**kw) == -1, kw
        assert b"adam_update_scheduled" in lib.lwg_last_error()
