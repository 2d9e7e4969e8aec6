"""CPU: the numpy restatement of cv::calcOpticalFlowPyrLK (tests/lk_np.py) that the GPU tests compare
the device with, checked against things that are not itself: the pyramid and the Scharr pair against
scipy.ndimage.correlate in integer arithmetic, the level counts, the tracks against the known
motion of a synthetic scene, the flat patch and the points far outside; then the argument checks
of the new entry points that need no device, and that the C++ shim's images path compiles as the
nodes compile it."""
import ctypes
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import lk_np as L
from loam_amd import _core, vo
from vo_frames_util import compile_shim

SIZES = [(16, 17), (17, 16), (31, 33), (48, 64), (65, 97), (2, 9)]  # (height, width)


@pytest.mark.parametrize("h,w", SIZES)
def test_pyr_down_is_the_mirrored_correlation(h, w):
    img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w), dtype=np.uint8)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    full = ndimage.correlate(img.astype(np.int64), np.outer(k, k), mode="mirror")
    ref = ((full[::2, ::2] + 128) >> 8).astype(np.uint8)
    got = L.pyr_down(img)
    assert got.shape == ((h + 1) // 2, (w + 1) // 2) and got.dtype == np.uint8
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("h,w", SIZES)
def test_scharr_is_the_mirrored_correlation(h, w):
    img = np.random.default_rng(h * 100 + w + 1).integers(0, 256, (h, w), dtype=np.uint8)
    kx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]], np.int64)
    dx, dy = L.scharr(img)
    assert dx.dtype == dy.dtype == np.int16
    assert np.array_equal(dx, ndimage.correlate(img.astype(np.int64), kx, mode="mirror"))
    assert np.array_equal(dy, ndimage.correlate(img.astype(np.int64), kx.T, mode="mirror"))


def test_reflect101_is_border_interpolate():
    for n in (1, 2, 5, 16):
        for i in range(-40, 60):
            j = i  # cv::borderInterpolate's loop
            if n == 1:
                j = 0
            while j < 0 or j >= n:
                j = -j if j < 0 else 2 * (n - 1) - j
            assert L.reflect101(i, n) == j, (i, n)


@pytest.mark.parametrize("w,h,levels", [(64, 48, 2), (97, 65, 3), (1241, 376, 3)])
def test_level_counts(w, h, levels):
    pyr = L.build_pyramid(np.zeros((h, w), np.uint8), 15, 2)
    assert len(pyr) == levels
    for k, a in enumerate(pyr):
        assert a.shape == ((h + (1 << k) - 1) >> k, (w + (1 << k) - 1) >> k)


W, H = 128, 96
# The worst |tracked - true| of the status-1 points over the four shifts below, measured with this
# model on these inputs: 0.0324 px (the shift (-3.0, 0.5)).  The uint8 quantisation makes the error
# depend on the input; twice the measured value absorbs a change of seed.
TRACK_BAR = 0.065


def scene_and_points():
    sc = L.Scene(7)
    gx, gy = np.meshgrid(np.arange(14.3, W - 14, 7.9), np.arange(14.6, H - 14, 7.3))
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1)
    x0, y0, x1, y1 = sc.flat
    near = (pts[:, 0] > x0 - 12) & (pts[:, 0] < x1 + 12) & (pts[:, 1] > y0 - 12) & (pts[:, 1] < y1 + 12)
    return sc, pts[~near].astype(np.float32)


@pytest.mark.parametrize("shift", [(0.0, 0.0), (0.25, -0.5), (2.6, 1.3), (-3.0, 0.5)])
def test_tracks_follow_the_known_shift(shift):
    sc, pts = scene_and_points()
    assert len(pts) >= 60
    nxt, status, err = L.track(sc.render(W, H), sc.render(W, H, t=shift), pts)
    ok = status == 1
    assert ok.mean() >= 0.9, ok.mean()
    e = np.abs(nxt.astype(np.float64) - (pts.astype(np.float64) + np.array(shift)))[ok]
    print(f"shift {shift}: {ok.sum()}/{len(pts)} tracked, worst error {e.max():.4f} px")
    assert e.max() <= TRACK_BAR
    if shift == (0.0, 0.0):
        assert np.array_equal(nxt, pts) and not err.any()      # the same image: no step at all


def test_small_affine_motion():
    """a rotation of 1.5 degrees and 2 % of scale about the image centre: the window still locks
    on.  LK answers with a gradient-weighted mean of the displacements inside the window; a pixel
    (dx, dy) from the centre, |dx|, |dy| <= 7, moves differently from the centre by
    (M - I)(dx, dy), at most 7 (|c - 1| + |s|) = 0.33 px per axis: the bar is the shift bar plus that"""
    sc, pts = scene_and_points()
    c, s = np.cos(np.radians(1.5)) * 1.02, np.sin(np.radians(1.5)) * 1.02
    M = np.array([[c, -s], [s, c]])
    ctr = np.array([W / 2, H / 2])
    t = ctr - M @ ctr + (0.8, -0.4)
    nxt, status, _ = L.track(sc.render(W, H), sc.render(W, H, M=M, t=t), pts)
    ok = status == 1
    assert ok.mean() >= 0.9
    e = np.abs(nxt - (pts.astype(np.float64) @ M.T + t))[ok]
    assert e.max() <= TRACK_BAR + 7 * (abs(c - 1) + abs(s)), e.max()


def test_flat_patch_and_outside_points():
    sc, _ = scene_and_points()
    img = sc.render(W, H)
    x0, y0, x1, y1 = sc.flat
    assert (img[int(y0):int(y1) + 1, int(x0):int(x1) + 1] == 128).all()
    flat = np.array([[(x0 + x1) / 2, (y0 + y1) / 2], [x0 + 9.5, y0 + 9.5], [x1 - 9, y1 - 9.25]], np.float32)
    nxt, status, err = L.track(img, sc.render(W, H, t=(1.0, 0.5)), flat)
    assert not status.any() and not err.any()                  # minEig = 0 at level 0
    # floor(p - 7) < -win, or >= the size: more than win outside
    out = np.array([[-8.5, 10], [W + 7, 10], [10, -9.0], [10, H + 7.01], [np.nan, 1], [1e12, 5], [-1e30, -1e30]],
                   np.float32)
    nxt, status, err = L.track(img, img, out)
    assert not status.any() and not err.any()
    just_in = np.array([[-7.99, 40], [W + 6.99, 40]], np.float32)  # floor(p - 7) = -15 / W - 1: inside the check
    assert np.array_equal(L._ifloor(just_in[0, 0] - np.float32(7)), -15)
    L.track(img, img, just_in)                                  # reads reflected pixels, raises nothing


def test_caps_and_oscillation_are_reachable():
    """the scene the GPU test uses for the iteration cap and the oscillation rule takes both branches"""
    sc = L.Scene(8)
    gx, gy = np.meshgrid(np.arange(4, 97 - 3, 6.5), np.arange(4, 65 - 3, 6.5))
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)
    info = {}
    _, status, _ = L.track(sc.render(97, 65), sc.render(97, 65, t=(12.0, 6.0)), pts, info=info)
    assert info["cap"].any() and (info["osc"] & (status == 1)).any()


def test_entry_points_validate_before_any_device_work():
    lib = _core.lib()
    p = vo.lk_params(1241, 376)
    assert (p.max_width, p.max_height, p.win, p.max_level, p.max_count) == (1241, 376, 15, 2, 10)
    assert p.epsilon == 0.03 and p.min_eig_threshold == 1e-4
    d = _core.LKParams()
    lib.loam_lk_params_default(ctypes.byref(d))
    assert (d.max_width, d.max_height, d.win) == (0, 0, 15)
    lib.loam_lk_params_default(None)
    img = np.zeros((8, 8), np.uint8)
    pts = np.zeros((1, 2), np.float32)
    assert lib.loam_vo_frames_enable_images(None, ctypes.byref(p)) == -1
    assert lib.loam_vo_frames_input_images(None, 0, img.ctypes.data, img.ctypes.data, 8, 8, 8, pts.ctypes.data, 1,
                                           0) == -1
    assert lib.loam_vo_frames_tracks_copy(None, 0, None, None, None, None, 0) == -1
    assert lib.loam_vo_frames_pyramid_copy(None, 0, 0, 0, None, 0, None) == -1
    assert "loam_vo_frames" in lib.loam_last_error().decode()


def test_cxx_images_check_compiles(tmp_path):
    """tests/cxx/vo_frames_check.cpp through include/loam_core.hpp with the nodes' compiler and
    warnings; without an input file it only reports the library version"""
    exe = compile_shim(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "version" in r.stdout
