"""CPU: the numpy restatement of cv::goodFeaturesToTrack (tests/gftt_np.py) that the GPU tests compare
the device with, checked against things that are not itself: the Sobel pair and the box sums against
scipy.ndimage.correlate in int64, the eigenvalue against numpy.linalg.eigvalsh in float64, the
selection against its defining properties and against a restatement of OpenCV's cell grid, the
order of planted ties; then the argument checks of the new entry points that need no device, and
that the C++ shim's detection path compiles as the nodes compile it."""
import ctypes
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import gftt_np as G
import lk_np as L
from loam_amd import _core, vo
from vo_frames_util import compile_shim

SIZES = [(16, 17), (31, 33), (65, 97), (2, 9), (9, 1)]  # (height, width)


@pytest.mark.parametrize("h,w", SIZES)
def test_sobel_is_the_mirrored_correlation(h, w):
    img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w), dtype=np.uint8)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int64)
    dx, dy = G.sobel(img)
    assert np.abs(dx).max() <= 1020 and np.abs(dy).max() <= 1020
    assert np.array_equal(dx, ndimage.correlate(img.astype(np.int64), kx, mode="mirror"))
    assert np.array_equal(dy, ndimage.correlate(img.astype(np.int64), kx.T, mode="mirror"))


@pytest.mark.parametrize("block", [2, 3, 5, 15])
@pytest.mark.parametrize("h,w", SIZES[:3])
def test_box_sums_are_the_mirrored_correlation(h, w, block):
    """a box of an even size reaches one further back than forward: for scipy it is an odd kernel
    (centre block // 2) whose last row and column are zero"""
    img = np.random.default_rng(h + w + block).integers(0, 256, (h, w), dtype=np.uint8)
    dx, dy = (p.astype(np.int64) for p in G.sobel(img))
    size = block | 1                                             # odd: its centre is size // 2 = block // 2
    k = np.zeros((size, size), np.int64)
    k[:block, :block] = 1                                        # offsets -(block // 2) .. block - 1 - block // 2
    got = G.cov_sums(img, block)
    for g, plane in zip(got, (dx * dx, dx * dy, dy * dy)):
        assert g.dtype == np.int32
        assert np.array_equal(g, ndimage.correlate(plane, k, mode="mirror"))


@pytest.mark.parametrize("block", [2, 3, 5, 15])
def test_eig_is_the_smaller_eigenvalue(block):
    """|eig - lambda_min| <= 8 * 2^-24 * (a + c): one half-ulp of the (a + c) magnitude for each of
    the ~8 float32 roundings; lambda_min is numpy's in float64 of [[Sxx, Sxy], [Sxy, Syy]] * k,
    whose smaller eigenvalue is (a + c) - sqrt((a - c)^2 + b^2) with a = Sxx k / 2, b = Sxy k,
    c = Syy k / 2"""
    worst = 0.0
    for seed, (h, w) in enumerate([(31, 33), (48, 64)]):
        img = L.Scene(seed + 1).render(w, h) if seed else np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)
        sxx, sxy, syy = (s.astype(np.float64) for s in G.cov_sums(img, block))
        k = float(G.eig_scale(block))
        M = np.stack([np.stack([sxx * k, sxy * k], -1), np.stack([sxy * k, syy * k], -1)], -2)
        lam = np.linalg.eigvalsh(M)[..., 0]
        eig = G.min_eigen(img, block).astype(np.float64)
        a_plus_c = (sxx + syy) * k * 0.5
        bound = 8 * 2.0 ** -24 * a_plus_c
        ratio = (np.abs(eig - lam) / np.maximum(bound, 1e-300)).max()
        worst = max(worst, ratio)
        assert (np.abs(eig - lam) <= bound).all(), ratio
    print(f"block {block}: worst |eig - lambda_min| = {worst:.3f} of the bound")


def inputs():
    yield "scene-128x96", L.Scene(3).render(128, 96)
    yield "scene-97x65", L.Scene(2).render(97, 65)
    yield "noise-128x96", np.random.default_rng(0).integers(0, 256, (96, 128), dtype=np.uint8)


@pytest.mark.parametrize("name,img", list(inputs()), ids=[n for n, _ in inputs()])
@pytest.mark.parametrize("min_distance,max_corners", [(7.5, 1024), (2.5, 1024), (7.5, 20), (1.0, 50)])
def test_selection_properties(name, img, min_distance, max_corners):
    info = {}
    pts = G.good_features_to_track(img, max_corners=max_corners, min_distance=min_distance, info=info)
    h, w = img.shape
    idx, kept = info["idx"], info["kept"]
    assert len(pts) == len(kept) <= max_corners and len(pts) > 0
    assert (np.diff(kept) > 0).all()                             # a subsequence of the order
    assert (np.diff(info["val"].astype(np.float64)) <= 0).all()
    xy = pts.astype(np.float64)
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    d2[np.diag_indices(len(xy))] = np.inf
    assert d2.min() >= min_distance * min_distance               # every kept pair is far enough apart
    # every rejected candidate ranked above the last kept one has an earlier kept corner near it
    cx, cy = (idx % w).astype(np.float64), (idx // w).astype(np.float64)
    is_kept = np.zeros(len(idx), bool)
    is_kept[kept] = True
    for i in np.flatnonzero(~is_kept[:kept[-1]]):
        earlier = kept[kept < i]
        dd = (cx[earlier] - cx[i]) ** 2 + (cy[earlier] - cy[i]) ** 2
        assert len(earlier) and dd.min() < min_distance * min_distance, i
    if len(kept) < max_corners:                                  # not cut: the rest was rejected too
        assert len(G.select(idx, w, len(idx), min_distance)) == len(kept)
    # a prefix: fewer corners asked for are the first of these
    few = G.good_features_to_track(img, max_corners=max(1, len(pts) // 2), min_distance=min_distance)
    assert np.array_equal(few, pts[:len(few)])


def test_no_suppression_below_one():
    img = L.Scene(3).render(128, 96)
    info = {}
    pts = G.good_features_to_track(img, max_corners=70, min_distance=0.0, info=info)
    assert np.array_equal(info["kept"], np.arange(70)) and len(info["idx"]) == 237
    assert np.array_equal(pts, G.good_features_to_track(img, max_corners=70, min_distance=0.99))


@pytest.mark.parametrize("min_distance", [1.0, 1.5, 2.5, 3.0, 3.5, 7.5, 20.0, 500.0])
def test_grid_selection_equals_the_plain_loop(min_distance):
    """OpenCV's own way (cells cvRound(minDistance) wide, 3 x 3 cells) and the O(n^2) loop"""
    assert [G.cv_round(v) for v in (0.5, 1.5, 2.5, 3.5, 7.5)] == [0, 2, 2, 4, 8]   # half to even
    for name, img in inputs():
        h, w = img.shape
        val, idx = G.candidates(G.min_eigen(img), 0.03)
        a = G.select(idx, w, 1024, min_distance)
        b = G.select_grid(idx, w, h, 1024, min_distance)
        assert np.array_equal(a, b), name


def test_planted_tie_comes_out_higher_index_first():
    img = G.tie_image()
    assert np.array_equal(img, img[:, ::-1])
    info = {}
    pts = G.good_features_to_track(img, min_distance=3.0, info=info)
    eig = info["eig"]
    assert np.array_equal(eig.view(np.uint32), eig[:, ::-1].view(np.uint32))   # the plane mirrors exactly
    val, idx = info["val"], info["idx"]
    assert info["ties"] == 27 and len(idx) == 54
    for i in np.flatnonzero(val[1:] == val[:-1]):
        assert idx[i] > idx[i + 1]                               # greaterThanPtr: the higher address first
        assert idx[i] // 64 == idx[i + 1] // 64 and idx[i] % 64 == 63 - idx[i + 1] % 64   # the mirrored pair
    assert val[0] == val[1] and pts[0][0] == idx[0] % 64 > 31.5  # the strongest pair: its right one first


def test_plateau_makes_every_pixel_a_candidate():
    info = {}
    G.good_features_to_track(G.plateau_image(), info=info)
    assert G.adjacent_ties(info, 64) == 1 and len(info["idx"]) == 8


def test_constant_image_has_no_corner():
    img = np.full((48, 64), 77, np.uint8)
    info = {}
    assert len(G.good_features_to_track(img, info=info)) == 0
    assert not info["eig"].any() and len(info["idx"]) == 0


def test_border_pixels_are_no_candidates():
    img = np.random.default_rng(0).integers(0, 256, (96, 128), dtype=np.uint8)
    _, idx = G.candidates(G.min_eigen(img), 0.03)
    x, y = idx % 128, idx // 128
    assert x.min() >= 1 and x.max() <= 126 and y.min() >= 1 and y.max() <= 94
    assert ((x == 1) | (x == 126) | (y == 1) | (y == 94)).any()  # the next ring is allowed, and used


@pytest.mark.parametrize("w,h,seed,n_cand,n_corners,ties", [
    (64, 48, 1, 37, 19, 0), (97, 65, 2, 77, 44, 0), (128, 96, 3, 237, 96, 0), (333, 171, 4, 791, 400, 0),
    (1241, 376, 5, 7802, 1024, 3)])
def test_counts_of_the_gpu_inputs(w, h, seed, n_cand, n_corners, ties):
    info = {}
    pts = G.good_features_to_track(L.Scene(seed).render(w, h), info=info)
    assert (len(info["idx"]), len(pts), info["ties"]) == (n_cand, n_corners, ties)


def test_entry_points_validate_before_any_device_work():
    lib = _core.lib()
    p = vo.gftt_params()
    assert (p.max_corners, p.quality_level, p.min_distance, p.block_size, p.max_candidates) == \
        (1024, 0.03, 7.5, 5, 65536)
    assert vo.gftt_params(block_size=3).block_size == 3
    lib.loam_gftt_params_default(None)
    img = np.zeros((8, 8), np.uint8)
    assert lib.loam_vo_frames_enable_detection(None, ctypes.byref(p)) == -1
    assert lib.loam_vo_frames_input_image_pair(None, 0, img.ctypes.data, img.ctypes.data, 8, 8, 8, 0, 0) == -1
    assert lib.loam_vo_frames_eig_copy(None, 0, None, 0, None) == -1
    assert "loam_vo_frames" in lib.loam_last_error().decode()


def test_cxx_detect_check_compiles(tmp_path):
    """tests/cxx/vo_frames_check.cpp through include/loam_core.hpp with the nodes' compiler and
    warnings; without an input file it only reports the library version"""
    exe = compile_shim(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "version" in r.stdout
