"""CPU: the host side of novel views in batches -- run_view.py's parameter parsing and turntable schedule (reference:
run_view.py:15-69), the image-grid layout of torchvision's make_grid (lwg_image_grid_shape needs no device) and the argument
validation of the two new kernels' entry points, which happens before any HIP call."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impersonator_amd import _lib  # noqa: E402


def test_parse_view_params_gives_radians():
    import run_view
    p = run_view.parse_view_params('R=0,90,0/t=0.1,0,0')
    assert p['R'].dtype == np.float32 and p['t'].dtype == np.float32
    assert np.allclose(p['R'], [0.0, np.pi / 2, 0.0], atol=1e-6)
    assert np.array_equal(p['t'], np.array([0.1, 0, 0], np.float32))
    q = run_view.parse_view_params('R=10,-45,180/t=0,0.5,-1')
    assert np.allclose(q['R'], np.radians([10, -45, 180]), atol=1e-6)
    assert np.array_equal(q['t'], np.array([0, 0.5, -1], np.float32))


def test_view_schedule_is_the_reference_turntable():
    import run_view
    params = run_view.parse_view_params('R=0,90,0/t=0.1,0,0')
    rts, ts = run_view.view_schedule(params, 16)
    assert rts.shape == (16, 3) and ts.shape == (16, 3) and rts.dtype == np.float32
    assert np.allclose(rts[:, 0], np.radians(10), atol=1e-6) and np.allclose(rts[:, 2], np.radians(10), atol=1e-6)
    assert np.allclose(rts[:, 1], np.radians(22.5 * np.arange(16)), atol=1e-6)
    assert np.allclose(np.diff(rts[:, 1]), np.radians(22.5), atol=1e-6)
    assert np.array_equal(ts, np.tile(np.array([[0.1, 0, 0]], np.float32), (16, 1)))
    # the same float32s the reference's loop stores into its float32 array
    ref = np.zeros(3, np.float32)
    ref[1] = 360 / 16 * 5 / 180.0 * np.pi
    assert rts[5, 1] == ref[1]
    rts5, ts5 = run_view.view_schedule(params, 5)
    assert rts5.shape == (5, 3) and np.allclose(rts5[:, 1], np.radians(72.0 * np.arange(5)), atol=1e-6)


def test_view_options_carry_the_view_flags():
    from impersonator_amd.options.test_options import TestOptions
    from impersonator_amd.options.view_options import ViewOptions
    opt = ViewOptions().parse([])
    assert opt.view_params == 'R=0,90,0/t=0,0,0' and opt.T_pose is False and opt.num_views == 16
    base = vars(TestOptions().parse([]))
    assert {k: v for k, v in vars(opt).items() if k in base} == base      # every existing option, with its default
    assert sorted(set(vars(opt)) - set(base)) == ['T_pose', 'num_views', 'view_params']
    opt = ViewOptions().parse(['--view_params', 'R=1,2,3/t=4,5,6', '--num_views', '5', '--T_pose'])
    assert opt.view_params == 'R=1,2,3/t=4,5,6' and opt.num_views == 5 and opt.T_pose is True


def _shape(*args):
    gh, gw = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _lib.load().lwg_image_grid_shape(*args, ctypes.byref(gh), ctypes.byref(gw))
    return rc, (gh.value, gw.value)


def test_image_grid_shape_without_a_device():
    assert _shape(16, 256, 256, 8, 2) == (0, (518, 2066))
    assert _shape(1, 5, 7, 8, 2) == (0, (5, 7))              # one image: returned as it is, no padding
    assert _shape(5, 6, 10, 4, 2) == (0, (18, 50))
    assert _shape(3, 4, 4, 8, 0) == (0, (4, 12))
    from impersonator_amd.utils import util
    assert util.image_grid_shape(16, 256, 256) == (518, 2066)
    lib = _lib.load()
    for bad in ((0, 4, 4, 8, 2), (-1, 4, 4, 8, 2), (3, 0, 4, 8, 2), (3, 4, -2, 8, 2), (3, 4, 4, 0, 2), (3, 4, 4, 8, -1)):
        rc, out = _shape(*bad)
        assert rc == -1 and out == (-7, -7), bad
        assert b"image_grid_shape" in lib.lwg_last_error()
    assert lib.lwg_image_grid_shape(3, 4, 4, 8, 2, None, None) == -1
    assert b"NULL" in lib.lwg_last_error()


def test_new_entry_points_validate_before_touching_a_device():
    # the pointers below are never dereferenced: every refusal comes before the first HIP call
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    for args in ((None, 10, p, 2, p), (p, 10, None, 2, p), (p, 10, p, 2, None)):
        assert lib.lwg_rigid_views(*args, None) == -1
        assert b"rigid_views" in lib.lwg_last_error() and b"NULL" in lib.lwg_last_error()
    for nv, n in ((10, 0), (10, -3), (0, 2), (-5, 2)):
        assert lib.lwg_rigid_views(p, nv, p, n, p, None) == -1
        assert b"rigid_views" in lib.lwg_last_error() and b"positive" in lib.lwg_last_error()
    assert lib.lwg_rigid_views(p, 10, p, 1 << 20, p, None) == -2          # more transforms than one launch takes

    grid = lambda x, n, H, W, nrow, pad, out: lib.lwg_image_grid_u8(x, n, H, W, nrow, pad, 0.0, 1, out, None)
    assert grid(None, 2, 4, 4, 8, 2, p) == -1 and b"NULL" in lib.lwg_last_error()
    assert grid(p, 2, 4, 4, 8, 2, None) == -1 and b"NULL" in lib.lwg_last_error()
    for bad in ((0, 4, 4, 8, 2), (-2, 4, 4, 8, 2), (2, 0, 4, 8, 2), (2, 4, 0, 8, 2), (2, 4, 4, 0, 2), (2, 4, 4, 8, -1)):
        assert grid(p, *bad, p) == -1, bad
        assert b"image_grid_u8" in lib.lwg_last_error()
