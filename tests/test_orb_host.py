"""CPU: the numpy restatement of ORB's descriptor stage (tests/orb_np.py) that the GPU tests hold the
device to: the pattern's pinned values, the blur's weights and rounding, the rotation's rounding at
exact ties, a descriptor known by hand, the border filter's edge cases, and the argument checks of
the new entry points that need no device."""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest

import orb_np as O
from conftest import ROOT
from loam_amd import _core, vo

F = np.float32
FMA_ANGLES = (291.8060607910156, 81.29690551757812)          # float32 values; see the test below
TEST_ANGLES = (0.0, 30.0, 45.0, 90.0, 137.5, -1.0, 359.0) + FMA_ANGLES   # test_gpu_orb.py's


def test_pattern_pins():
    v = O.PATTERN
    assert v.shape == (256, 4)
    assert v[0].tolist() == [8, -3, 9, 5] and v[1].tolist() == [4, 2, 7, -12] and v[-1].tolist() == [-1, -6, 0, -11]
    flat = v.ravel().astype(np.int64)
    assert int(np.abs(flat).max()) == 13 and int(flat.sum()) == -406
    assert int((flat * (np.arange(1024) + 1)).sum()) == -177504
    r = np.sqrt((v.reshape(-1, 2).astype(np.float64) ** 2).sum(axis=1)).max()
    assert abs(r - 18.3848) < 1e-4


def test_the_header_table_is_the_fixture():
    """csrc/orb_pattern.h and tests/golden/orb_pattern.npz hold the same 1024 values"""
    import re
    text = open(os.path.join(ROOT, "vloam-noted_amd", "csrc", "orb_pattern.h")).read()
    body = text[text.index("#define LOAM_ORB_PATTERN_VALUES"):text.index("constexpr int8_t ORB_PATTERN")]
    vals = [int(t) for t in re.findall(r"-?\d+", body.split("\n", 1)[1])]
    assert vals == O.PATTERN.ravel().tolist()


def test_blur_weights_from_the_gaussian():
    assert O.gaussian_weights().tolist() == [18, 34, 49, 55, 49, 34, 18] == O.WEIGHTS.tolist()
    assert int(O.WEIGHTS.sum()) == 257


def test_blur_of_constants():
    assert (O.blur7(np.full((9, 11), 255, np.uint8)) == 255).all()     # saturates: the weights sum to 257
    assert (100 * 257 * 257 + 32768) >> 16 == 101
    assert (O.blur7(np.full((9, 11), 100, np.uint8)) == 101).all()
    assert (O.blur7(np.zeros((1, 1), np.uint8)) == 0).all()


@pytest.mark.parametrize("pos", [(10, 12), (0, 0), (1, 19), (15, 2)])
def test_blur_impulse_against_direct_2d(pos):
    """an impulse of 200 against the direct 2-D sum over the reflected image"""
    h, w = 16, 20
    img = np.zeros((h, w), np.uint8)
    img[pos] = 200
    got = O.blur7(img)
    W = O.WEIGHTS
    ref = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            s = 0
            for j in range(-3, 4):
                for i in range(-3, 4):
                    yy, xx = y + j, x + i
                    yy = -yy if yy < 0 else 2 * (h - 1) - yy if yy >= h else yy
                    xx = -xx if xx < 0 else 2 * (w - 1) - xx if xx >= w else xx
                    s += int(W[j + 3]) * int(W[i + 3]) * int(img[yy, xx])
            ref[y, x] = min((s + 32768) >> 16, 255)
    assert np.array_equal(got, ref.astype(np.uint8))
    assert got[pos] >= (200 * 55 * 55 + 32768) >> 16                 # (more where the reflection folds it back)


def test_unrotated_patterns_equal_the_table():
    pts = O.PATTERN.reshape(-1, 2)
    assert np.array_equal(O.rotated_pattern(-1.0), pts)               # the reference's angle
    assert np.array_equal(O.rotated_pattern(0.0), pts)


def test_rotation_by_30_degrees_rounds_half_to_even():
    a, b = O.cos_sin(30.0)
    assert b == F(0.5) and a == F(0.8660254)
    pts = O.PATTERN.reshape(-1, 2).astype(np.float64)
    # the float32 products and sums are exact in float64 up to their own rounding: evaluate in float64
    # with the same (a, b), round half to even by hand
    fx = pts[:, 0] * float(a) - pts[:, 1] * float(b)
    fy = pts[:, 0] * float(b) + pts[:, 1] * float(a)

    def half_even(v):
        f = np.floor(v)
        d = v - f
        return np.where(d > 0.5, f + 1, np.where(d < 0.5, f, f + (f % 2))).astype(np.int32)

    ref = np.stack([half_even(fx), half_even(fy)], axis=1)
    got = O.rotated_pattern(30.0)
    assert np.array_equal(got, ref)
    tie_x, tie_y = (fx - np.floor(fx)) == 0.5, (fy - np.floor(fy)) == 0.5
    assert (int(tie_x.sum()), int(tie_y.sum())) == (8, 16)           # x = 0 and y odd; y = 0 and x odd
    away = np.stack([np.where(tie_x, np.sign(fx) * np.ceil(np.abs(fx)), ref[:, 0]),
                     np.where(tie_y, np.sign(fy) * np.ceil(np.abs(fy)), ref[:, 1])], axis=1)
    assert (away != ref).sum() >= 10                                 # half away from zero would show
    assert int((got != O.PATTERN.reshape(-1, 2)).sum()) == 943
    assert int(np.abs(got).max()) <= 19


def test_angles_at_which_a_fused_rotation_moves_a_point():
    """at these two angles an unfused sum lands exactly on k + .5 (and goes to the even side) while
    the exact product is off the tie: each of the four ways to fuse one product of fx = px a - py b,
    fy = px b + py a into the sum changes a rounded coordinate at one of them.  The model is the
    unfused one, checked against a float64 evaluation (exact here: 24-bit by 4-bit products)"""
    pts = O.PATTERN.reshape(-1, 2).astype(np.float64)
    px, py = pts[:, 0], pts[:, 1]
    r32 = lambda v: np.asarray(v, np.float64).astype(F).astype(np.float64)
    moved = {k: 0 for k in O.FUSED_FORMS}
    for deg in FMA_ANGLES:
        assert float(F(deg)) == deg
        a, b = (float(v) for v in O.cos_sin(deg))
        got = O.rotated_pattern(deg)
        fx, fy = r32(r32(px * a) - r32(py * b)), r32(r32(px * b) + r32(py * a))
        assert np.array_equal(got, np.stack([np.rint(fx), np.rint(fy)], axis=1).astype(np.int32))
        assert int(np.abs(got).max()) <= 19
        for k in O.FUSED_FORMS:
            moved[k] += int((O.fused_rotated_pattern(deg, k) != got).sum())
    assert all(n >= 1 for n in moved.values()), moved
    a, b = (float(v) for v in O.cos_sin(FMA_ANGLES[0]))
    i = int(np.flatnonzero((px == 10) & (py == 3))[0])                # the unfused x is exactly 6.5 -> 6; fused: 7
    assert r32(r32(10 * a) - r32(3 * b)) == 6.5 and O.rotated_pattern(FMA_ANGLES[0])[i, 0] == 6
    assert np.rint(r32(10 * a - r32(3 * b))) == 7


def test_the_c_librarys_cosf_and_sinf_are_the_models_at_the_test_angles():
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (m.cosf, m.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    for deg in TEST_ANGLES:
        angle = float(F(deg) * F(np.pi / 180.0))
        assert (F(m.cosf(angle)), F(m.sinf(angle))) == O.cos_sin(deg), deg


def test_every_pattern_stays_within_19_pixels():
    for deg in np.arange(0.0, 360.0, 0.5):
        assert int(np.abs(O.rotated_pattern(deg)).max()) <= 19


def test_descriptor_on_a_step_is_known_by_hand():
    """left of the keypoint's column 50, from it on 200: the blurred plane depends on x alone and
    rises strictly over the offsets -4 .. 3, so test t is clip(x0, -4, 3) < clip(x1, -4, 3)"""
    h, w, cx, cy = 80, 90, 45, 40
    img = np.full((h, w), 50, np.uint8)
    img[:, cx:] = 200
    B = O.blur7(img)
    row = B[cy, cx - 6:cx + 6].astype(int)
    assert (B == B[cy]).all() and (np.diff(row[2:10]) > 0).all() and row[0] == row[2] and row[9] == row[11]
    kept, desc, idx = O.describe(img, [[cx, cy]])
    assert idx.tolist() == [0] and desc.shape == (1, 32)
    P = O.PATTERN
    bits = np.clip(P[:, 0], -4, 3) < np.clip(P[:, 2], -4, 3)
    assert 60 < bits.sum() < 200
    assert np.array_equal(np.unpackbits(desc[0], bitorder="little").astype(bool), bits)
    assert desc[0, 0] & 1 == int(bits[0]) and (desc[0, 31] >> 7) & 1 == int(bits[255])
    # by 90 degrees (x, y) -> (-y, x): the same from the y coordinates of the pattern
    _, d90, _ = O.describe(img, [[cx, cy]], [90.0])
    bits90 = np.clip(-P[:, 1], -4, 3) < np.clip(-P[:, 3], -4, 3)
    assert np.array_equal(np.unpackbits(d90[0], bitorder="little").astype(bool), bits90)


def test_border_filter_edges():
    w, h = 100, 80
    kps = np.array([[30.5, 40], [31, 40], [30.4999, 40], [31.5, 40], [w - 31, 40], [w - 31.5, 40], [w - 32, 40],
                    [w - 31.6, 40], [50, 30.5], [50, 31], [50, h - 31], [50, h - 31.5], [50, h - 32],
                    [np.nan, 40], [50, np.inf], [-np.inf, 40], [50, 40], [1e30, 40], [-5, -5]], F)
    # cvRound: 30.5 -> 30 (even) is out, 31.5 -> 32; w - 31.5 = 68.5 -> 68 is in, 69 is out
    expect = [1, 3, 5, 6, 7, 9, 11, 12, 16]
    assert O.border_filter(kps, w, h).tolist() == expect
    assert O.border_filter(kps, 62, 200).tolist() == [] and O.border_filter(kps, 200, 62).tolist() == []
    assert O.border_filter(np.array([[31, 31]], F), 63, 63).tolist() == [0]
    assert O.border_filter(np.array([[32, 31]], F), 63, 63).tolist() == []
    assert O.border_filter(np.zeros((0, 2), F), w, h).tolist() == []
    assert O.border_filter(kps, w, h, edge=22).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16]


def test_entry_points_validate_before_any_device_work():
    L = _core.lib()
    p = vo.orb_params()
    assert p.edge_threshold == 31
    L.loam_orb_params_default(None)                                   # ignored
    img = np.zeros((64, 64), np.uint8)
    assert L.loam_vo_frames_enable_description(None, ctypes.byref(p)) == -1
    assert L.loam_vo_frames_input_images_keypoints(None, 0, img.ctypes.data, img.ctypes.data, 64, 64, 64, None, None, 0,
                                                   None, None, 0, 0) == -1
    assert L.loam_vo_frames_input_image_pair_match(None, 0, img.ctypes.data, img.ctypes.data, 64, 64, 64, 0) == -1
    assert L.loam_vo_frames_descriptors_copy(None, 0, 0, None, None, 0) == -1
    assert L.loam_vo_frames_blur_copy(None, 0, 0, None, 0, None) == -1
    assert b"bad handle or pair" in L.loam_last_error()
