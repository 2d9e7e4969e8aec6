"""GPU: ORB descriptors on the device in front of the matcher (loam_vo_frames_enable_description /
_input_images_keypoints / _input_image_pair_match / _descriptors_copy / _blur_copy) against the
numpy restatement of cv::ORB::create()->compute on given keypoints (tests/orb_np.py), bit for bit.
 1. the blurred plane, edges and corners included, at sizes no tile divides, on both images of pairs
    of different sizes in one launch;
 2. given keypoints: on and next to the border line on all four sides, non-integer and .5
    coordinates, NaN and inf, with the default angle and with per-keypoint angles (30 degrees has
    exact .5 ties in the rotated pattern, 291.806... and 81.296... degrees have sums that only an
    unfused rotation puts on a tie); 0, 1, 65 and max_keypoints keypoints (more than one chunk
    of the compaction) and an idle pair in one solve; an image too small to keep any;
 3. the reference's default frame from the two images alone: the kept keypoints are the border
    filter of gftt_np's corners, the descriptors orb_np's, and the frame equals the one
    loam_vo_frames_input_descriptors computes from the models' keypoints and descriptors, bit for
    bit, pose included (tests/test_gpu_gftt.py compares device frames exactly; so does this);
 4. the existing modes beside a match pair on a handle that describes equal their own handles;
 5. candidate overflow, state and argument errors, the handle's resources;
 6. the C++ shim reproduces Python.
The counts asserted on the models are the committed models' own on these inputs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gftt_np as G
import lk_np as L
import orb_np as O
import vo_frames_np as N
from conftest import ROOT
from loam_amd import _core, vo
from loam_amd.depth import KITTI_CAM_T_VELO, KITTI_P_RECT0, KITTI_RECT0_T_CAM
from vo_frames_util import X_INIT, counters, give, make_depth, raises, same_bits, same_lm, strided

pytestmark = pytest.mark.gpu
F = np.float32
# the last two: an unfused sum of the rotation lands exactly on k + .5 where the exact product does not,
# so that a fused multiply-add in any of its four forms moves a point (test_orb_host.py shows it)
ANGLES = np.array([0.0, 30.0, 45.0, 90.0, 137.5, -1.0, 359.0, 291.8060607910156, 81.29690551757812], F)


@pytest.fixture(scope="module")
def depth():
    return make_depth()


def noise(w, h, seed):
    """noise with some structure left after the blur: coarse blocks under fine noise"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 200, ((h + 4) // 5, (w + 4) // 5)).repeat(5, axis=0).repeat(5, axis=1)[:h, :w]
    return (coarse + rng.integers(0, 56, (h, w))).astype(np.uint8)


def keypoints(rng, w, h, n):
    """n keypoints in and around the region the border filter keeps: reals, integers, .5 coordinates
    and, from 40 keypoints on, the border line on all four sides and coordinates that are not finite"""
    k = np.stack([rng.uniform(24, w - 24, n), rng.uniform(24, h - 24, n)], axis=1).astype(F)
    k[::5] = np.rint(k[::5])
    k[1::7] = np.floor(k[1::7]) + F(0.5)
    if n >= 40:
        my, mx = F(h // 2), F(w // 2)
        special = [(30.5, my), (31, my), (30.49, my), (31.5, my), (w - 31, my), (w - 31.5, my), (w - 32, my),
                   (w - 31.6, my), (mx, 30.5), (mx, 31), (mx, 31.5), (mx, h - 31), (mx, h - 31.5), (mx, h - 32),
                   (np.nan, my), (mx, np.inf), (-np.inf, my), (1e30, my), (mx + 0.5, my + 0.5), (31, 31),
                   (w - 32, h - 32), (w - 31, h - 32)]
        k[np.arange(len(special)) * (n // len(special))] = np.array(special, F)
    return k


_BLUR = {}


def blur_of(img):
    key = (img.shape, img.tobytes())
    if key not in _BLUR:
        _BLUR[key] = O.blur7(img)
    return _BLUR[key]


def check_described(vf, p, prev, curr, k0, k1, a0=None, a1=None, edge=31):
    """pair p of a solved handle against the models: planes, kept keypoints, descriptors, matches"""
    ref = []
    for image, (img, k, a) in enumerate(((prev, k0, a0), (curr, k1, a1))):
        B = blur_of(img)
        got_b = vf.blur(p, image)
        assert got_b.shape == B.shape and np.array_equal(got_b, B), (p, image, np.argwhere(got_b != B)[:6])
        kept, desc, _ = O.describe(img, k, a, edge=edge, blur=B)
        gk, gd = vf.descriptors(p, image)
        assert gk.shape == kept.shape, (p, image, gk.shape, kept.shape)
        assert same_bits(gk, kept), (p, image)
        bad = np.flatnonzero((gd != desc).any(axis=1))
        assert len(bad) == 0, (p, image, bad[:8], kept[bad[:8]])
        ref.append((kept, desc))
    m = N.match(ref[0][1], ref[1][1])
    assert np.array_equal(vf.matches(p), m), p
    st = vf.result(p)[2]
    assert st.n_knn == (len(ref[0][0]) if len(ref[1][0]) >= 2 else 0) and st.n_matches == len(m)
    return ref, m


# ---------------------------------------------------------------------------------------- 1
def test_blurred_planes_equal_the_model(depth):
    g, _ = depth
    sizes = [(64, 64), (97, 71), (200, 130)]
    imgs = [(noise(w, h, 10 + i), noise(w, h, 20 + i)) for i, (w, h) in enumerate(sizes)]
    imgs[0] = (np.full((64, 64), 255, np.uint8), imgs[0][1])            # saturation: 255 * 257 * 257 >> 16 > 255
    vf = vo.VOFrames(g, len(sizes), max_keypoints=64)
    vf.enable_images(203, 131)                                          # a maximum larger than every image
    vf.enable_description()
    none = np.zeros((0, 2), F)
    for p, (a, b) in enumerate(imgs):
        vf.input_images_keypoints(p, strided(a), strided(b), none, none)
    vf.solve()
    for p, (a, b) in enumerate(imgs):
        for image, img in enumerate((a, b)):
            ref = blur_of(img)
            got = vf.blur(p, image)
            assert got.shape == ref.shape and np.array_equal(got, ref), (p, image, np.argwhere(got != ref)[:6])
        assert vf.result(p)[1].termination == 4 and len(vf.descriptors(p, 0)[0]) == 0
    assert (vf.blur(0, 0) == 255).all()
    vf.close()


# ---------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("own_angles", [False, True], ids=["default-angle", "own-angles"])
@pytest.mark.parametrize("w,h", [(97, 71), (200, 130)])
def test_given_keypoints_are_filtered_and_described(depth, w, h, own_angles):
    g, _ = depth
    rng = np.random.default_rng(w + own_angles)
    prev, curr = noise(w, h, 1), noise(w, h, 2)
    k0, k1 = keypoints(rng, w, h, 300), keypoints(rng, w, h, 280)
    k1[40:200:3] = k0[40:200:3]                                          # some on the same pixels
    a0 = ANGLES[rng.integers(0, len(ANGLES), len(k0))] if own_angles else None
    a1 = ANGLES[np.arange(len(k1)) % len(ANGLES)] if own_angles else None
    vf = vo.VOFrames(g, 1, max_keypoints=512)
    vf.enable_images(w, h)
    vf.enable_description()
    vf.input_images_keypoints(0, prev, curr, k0, k1, a0, a1, 1)
    vf.solve()
    ref, _ = check_described(vf, 0, prev, curr, k0, k1, a0, a1)
    n_in = len(ref[0][0])
    assert 0 < n_in < len(k0) - 10                                       # the filter had something to do
    if own_angles:                                                       # every angle among the kept ones
        assert set(a0[O.border_filter(k0, w, h)].tolist()) == set(ANGLES.tolist())
    vf.close()


@pytest.mark.parametrize("deg,forms", [(291.8060607910156, (0, 3)), (81.29690551757812, (1, 2))], ids=["291.8", "81.3"])
def test_rotation_is_not_fused(depth, deg, forms):
    """every keypoint at an angle where fusing a product of the rotation into its sum moves a pattern
    point: the model says how many descriptors each fused form would change; the device's are the
    unfused model's"""
    g, _ = depth
    w, h = 200, 130
    rng = np.random.default_rng(7)
    prev, curr = noise(w, h, 5), noise(w, h, 6)
    k0, k1 = keypoints(rng, w, h, 250), keypoints(rng, w, h, 250)
    a = np.full(250, deg, F)
    _, ref, _ = O.describe(prev, k0, a)
    for form in (O.FUSED_FORMS[i] for i in forms):
        _, fused, _ = O.describe(prev, k0, a, pattern_of=lambda v, form=form: O.fused_rotated_pattern(v, form))
        changed = int((fused != ref).any(axis=1).sum())
        assert changed >= 10, (form, changed)                            # a fused kernel cannot pass by luck
    vf = vo.VOFrames(g, 1, max_keypoints=256)
    vf.enable_images(w, h)
    vf.enable_description()
    vf.input_images_keypoints(0, prev, curr, k0, k1, a, a)
    vf.solve()
    check_described(vf, 0, prev, curr, k0, k1, a, a)
    vf.close()


def test_mixed_angles_per_image(depth):
    """the previous image's keypoints with angles, the current one's without"""
    g, _ = depth
    w, h = 200, 130
    rng = np.random.default_rng(5)
    prev, curr = noise(w, h, 3), noise(w, h, 4)
    k0, k1 = keypoints(rng, w, h, 120), keypoints(rng, w, h, 90)
    a0 = np.full(len(k0), 30.0, F)
    vf = vo.VOFrames(g, 1, max_keypoints=128)
    vf.enable_images(w, h)
    vf.enable_description()
    vf.input_images_keypoints(0, prev, curr, k0, k1, a0, None)
    vf.solve()
    check_described(vf, 0, prev, curr, k0, k1, a0, None)
    vf.close()


def test_counts_sizes_and_an_idle_pair_in_one_solve(depth):
    g, _ = depth
    K = 1100                                                             # more than one chunk of the compaction
    rng = np.random.default_rng(9)
    big, mid, thin = (200, 130), (97, 71), (62, 80)
    items = []
    for (w, h), n0, n1, own in ((big, 0, 0, False), (mid, 1, 65, True), (big, 65, K, False), (big, K, 1, True),
                                (thin, 50, 50, False), (mid, 0, 33, False)):
        k0, k1 = keypoints(rng, w, h, n0), keypoints(rng, w, h, n1)
        if n0 == 1:
            k0[:] = (40.25, 35.5)
        if n1 == 1:
            k1[:] = (100.5, 64.0)
        a0 = ANGLES[np.arange(n0) % len(ANGLES)] if own else None
        a1 = ANGLES[(np.arange(n1) + 3) % len(ANGLES)] if own else None
        items.append((noise(w, h, 30 + len(items)), noise(w, h, 40 + len(items)), k0, k1, a0, a1))
    vf = vo.VOFrames(g, len(items) + 1, max_keypoints=K)
    vf.enable_images(200, 130)
    vf.enable_description()
    for p, it in enumerate(items):
        vf.input_images_keypoints(p + (p >= 3), *it)                     # pair 3 stays idle
    vf.solve()
    kept = []
    for p, it in enumerate(items):
        ref, _ = check_described(vf, p + (p >= 3), *it)
        kept.append((len(ref[0][0]), len(ref[1][0])))
    assert kept[0] == (0, 0) and kept[1][0] == 1 and kept[3][1] == 1 and kept[4] == (0, 0)   # 62 wide: none stays
    assert kept[2][1] > 700 and kept[3][0] > 700 and kept[2][1] < K
    raises(-4, vf.result, 3)                                             # the idle pair was never solved
    raises(-4, vf.descriptors, 3, 0)
    vf.close()


def test_other_edge_threshold(depth):
    g, _ = depth
    w, h = 97, 71
    rng = np.random.default_rng(2)
    prev, curr = noise(w, h, 5), noise(w, h, 6)
    k0, k1 = keypoints(rng, w, h, 100), keypoints(rng, w, h, 100)
    vf = vo.VOFrames(g, 1, max_keypoints=128)
    vf.enable_images(w, h)
    vf.enable_description(edge_threshold=22)
    vf.input_images_keypoints(0, prev, curr, k0, k1, ANGLES[np.arange(100) % len(ANGLES)], None)
    vf.solve()
    ref, _ = check_described(vf, 0, prev, curr, k0, k1, ANGLES[np.arange(100) % len(ANGLES)], None, edge=22)
    assert len(ref[0][0]) > len(O.border_filter(k0, w, h))
    vf.close()


# ---------------------------------------------------------------------------------------- 3
def assert_same_frame(a, pa, b, pb):
    (xa, la, sa), (xb, lb, sb) = a.result(pa), b.result(pb)
    assert same_bits(xa, xb) and same_lm(la, lb) and counters(sa) == counters(sb)
    (ra, da), (rb, db) = a.records(pa), b.records(pb)
    assert same_bits(ra, rb) and same_bits(da, db)
    assert np.array_equal(a.matches(pa), b.matches(pb))


_SCENES = {}


def scene_models(w, h, seed):
    """(prev, curr, [(corners, eig, kept keypoints, descriptors) per image], matches) of a textured scene
    and its shifted copy, from the two models alone"""
    if (w, h, seed) not in _SCENES:
        sc = L.Scene(seed)
        prev, curr = sc.render(w, h), sc.render(w, h, t=(1.7, -0.6))
        per = []
        for img in (prev, curr):
            info = {}
            c = G.good_features_to_track(img, info=info)
            kept, desc, _ = O.describe(img, c, blur=blur_of(img))
            per.append((c, info["eig"], kept, desc))
        _SCENES[(w, h, seed)] = prev, curr, per, N.match(per[0][3], per[1][3])
    return _SCENES[(w, h, seed)]


@pytest.mark.parametrize("w,h,seed,corners,kept,n_matches", [
    (160, 128, 3, (164, 172), (47, 49), 41), (320, 96, 2, (224, 215), (62, 62), 51),
    (1241, 376, 5, (1024, 1024), (816, 817), 711)], ids=["160x128", "320x96", "kitti"])
def test_default_frame_from_the_two_images(depth, w, h, seed, corners, kept, n_matches):
    g, _ = depth
    prev, curr, per, m = scene_models(w, h, seed)
    assert tuple(len(x[0]) for x in per) == corners and tuple(len(x[2]) for x in per) == kept and len(m) == n_matches
    assert min(kept) >= 40 and all(k < c for k, c in zip(kept, corners)) and n_matches >= 8
    a = vo.VOFrames(g, 1, max_keypoints=1024)
    a.enable_images(w + 5, h + 3)
    a.enable_detection()
    a.enable_description()
    a.input_image_pair_match(0, strided(prev), strided(curr), 1)
    a.set_initial(0, X_INIT)
    a.solve()
    for image in (0, 1):
        gk, gd = a.descriptors(0, image)
        assert same_bits(gk, per[image][2]), image                       # the border filter of gftt_np's corners
        assert np.array_equal(gd, per[image][3]), image
        assert np.array_equal(a.blur(0, image), blur_of((prev, curr)[image]))
    assert same_bits(a.eig(0), per[1][1])                                # the second detection's plane
    det = vo.VOFrames(g, 1, max_keypoints=1024)                          # the detector alone, on either image:
    det.enable_images(w + 5, h + 3)                                      # every corner, before the filter
    det.enable_detection()
    for image in (0, 1):
        det.input_image_pair(0, prev, curr, image, 1)
        det.solve()
        assert same_bits(det.tracks(0)[0], per[image][0]) and det.result(0)[2].n_knn == corners[image], image
    det.close()
    assert np.array_equal(a.matches(0), m)
    b = vo.VOFrames(g, 1, max_keypoints=1024)                            # the models' output through the given path
    b.input_descriptors(0, per[0][2], per[0][3], per[1][2], per[1][3], 1)
    b.set_initial(0, X_INIT)
    b.solve()
    assert_same_frame(a, 0, b, 0)
    s = a.result(0)[2]
    assert s.n_knn == kept[0] and s.n_matches == n_matches and s.n_gated > 0
    print(f"default frame {w}x{h}: kept {kept}, matches {s.n_matches}, gated {s.n_gated}, {s.ms:.3f} ms")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- 4
def test_existing_modes_beside_a_match_pair(depth):
    g, _ = depth
    rng = np.random.default_rng(12)
    prev, curr, per, m = scene_models(160, 128, 3)
    kp = lambda n: np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 374, n)], axis=1).astype(F)
    d0, d1 = rng.integers(0, 256, (300, 32), dtype=np.uint8), rng.integers(0, 256, (280, 32), dtype=np.uint8)
    d1[:200] = d0[:200]
    k0, k1 = kp(300), kp(280)
    k1[:200] = k0[:200] + rng.normal(0, 4, (200, 2)).astype(F)
    pts = kp(150) * F(0.1)
    nxt, st, _ = L.track(prev, curr, pts)
    sc = L.Scene(13)
    other = sc.render(128, 96), sc.render(128, 96, t=(1.0, -0.5))
    items = [("image_pair_match", (prev, curr), 1, X_INIT),
             ("descriptors", (k0, d0, k1, d1), 0, None),
             ("tracks", (pts, nxt, st), 1, 0.5 * X_INIT),
             ("image_pair", (*other, 1), 0, None),
             ("image_pair_match", (*other,), 0, None)]
    batch = vo.VOFrames(g, len(items), max_keypoints=1024)
    batch.enable_images(160, 128)
    batch.enable_detection()
    batch.enable_description()
    for p, item in enumerate(items):
        give(batch, p, item)
    batch.solve()
    for p, item in enumerate(items):
        one = vo.VOFrames(g, 1, max_keypoints=1024)
        if item[0].startswith("image_pair"):
            one.enable_images(*item[1][0].shape[::-1])
            one.enable_detection()
        if item[0] == "image_pair_match":
            one.enable_description()
        give(one, 0, item)
        one.solve()
        assert_same_frame(batch, p, one, 0)
        if item[0] == "image_pair":
            for u, v in zip(batch.tracks(p), one.tracks(0)):
                assert same_bits(u, v), p
            assert same_bits(batch.eig(p), one.eig(0))
            raises(-4, batch.descriptors, p, 0)                          # a detect pair has no description
        if item[0] == "image_pair_match":
            for image in (0, 1):
                for u, v in zip(batch.descriptors(p, image), one.descriptors(0, image)):
                    assert same_bits(u, v), (p, image)
            raises(-4, batch.tracks, p)                                  # and a match pair no tracks
        one.close()
    assert np.array_equal(batch.matches(0), m)
    assert_corners = G.good_features_to_track(other[1])
    assert same_bits(batch.tracks(3)[0], assert_corners) and batch.result(3)[2].n_knn == len(assert_corners)
    batch.close()


# ---------------------------------------------------------------------------------------- 5
def test_candidate_overflow_on_either_image(depth):
    g, _ = depth
    busy = np.random.default_rng(0).integers(0, 256, (96, 128), dtype=np.uint8)
    calm = L.Scene(3).render(128, 96)[:30, :40]
    assert len(G.candidates(G.min_eigen(busy), 0.03)[1]) == 680 and len(G.candidates(G.min_eigen(calm), 0.03)[1]) == 27
    calm_full = np.zeros((96, 128), np.uint8)
    calm_full[:] = 128
    calm_full[33:63, 44:84] = calm                                       # few candidates, away from the border
    vf = vo.VOFrames(g, 3)
    vf.enable_images(128, 96)
    vf.enable_detection(max_candidates=120)
    vf.enable_description()
    n_calm = len(G.candidates(G.min_eigen(calm_full), 0.03)[1])
    assert 0 < n_calm <= 120
    vf.input_image_pair_match(0, busy, calm_full, 0)                     # the previous image overflows
    vf.input_image_pair_match(1, calm_full, busy, 0)                     # the current one
    vf.input_image_pair_match(2, calm_full, calm_full, 0)
    vf.solve()
    for p in (0, 1):
        text = raises(-3, vf.result, p)
        assert "max_candidates" in text and "680" in text and "120" in text
        assert len(vf.matches(p)) == 0
    kept, desc, _ = O.describe(calm_full, G.good_features_to_track(calm_full))
    assert len(kept) >= 2
    for image in (0, 1):
        gk, gd = vf.descriptors(2, image)
        assert same_bits(gk, kept) and np.array_equal(gd, desc)
    assert len(vf.descriptors(0, 0)[0]) == 0 and same_bits(vf.descriptors(0, 1)[0], kept)
    assert vf.result(2)[2].n_matches == len(N.match(desc, desc))
    vf.input_image_pair_match(0, calm_full, calm_full, 0)                # the handle is usable afterwards
    vf.solve()
    assert same_bits(vf.descriptors(0, 0)[0], kept) and vf.result(0)[2].n_knn == len(kept)
    vf.close()


def test_errors_and_resources(depth):
    g, _ = depth
    lib = _core.lib()
    live = (ctypes.c_int64 * 4)()
    lib.loam_debug_live_resources(live)
    start = list(live)
    img = noise(97, 71, 1)
    k = keypoints(np.random.default_rng(1), 97, 71, 50)
    vf = vo.VOFrames(g, 2, max_keypoints=64)
    raises(-4, vf.enable_description)                                    # LOAM_ERR_STATE: before enable_images
    vf.enable_images(97, 71)
    raises(-4, vf.input_images_keypoints, 0, img, img, k, k)             # before enable_description
    for edge in (21, 0, -1, 32768):
        raises(-1, vf.enable_description, edge_threshold=edge)
    vf.enable_description()
    raises(-4, vf.enable_description)                                    # once per handle
    raises(-4, vf.input_image_pair_match, 0, img, img, 0)                # detection is not enabled
    vf.enable_detection(max_corners=64)
    raises(-4, vf.descriptors, 0, 0)                                     # never solved
    raises(-4, vf.blur, 0, 0)
    raises(-1, vf.input_images_keypoints, 2, img, img, k, k)
    raises(-1, vf.input_images_keypoints, 0, img, img, k, k, None, None, 2)
    raises(-3, vf.input_images_keypoints, 0, img, img, np.zeros((65, 2), F), k)       # over max_keypoints
    raises(-3, vf.input_images_keypoints, 0, np.zeros((71, 98), np.uint8), np.zeros((71, 98), np.uint8), k, k)
    raises(-3, vf.input_image_pair_match, 0, np.zeros((72, 97), np.uint8), np.zeros((72, 97), np.uint8), 0)
    raises(-1, vf.input_image_pair_match, 0, img, img, 2)
    with pytest.raises(ValueError):
        vf.input_images_keypoints(0, img, img, k, k, np.zeros(3, F), None)
    assert lib.loam_vo_frames_input_images_keypoints(vf.h, 0, img.ctypes.data, img.ctypes.data, 97, 71, 97, None, None,
                                                     5, k.ctypes.data, None, 5, 0) == -1
    assert lib.loam_vo_frames_input_image_pair_match(vf.h, 0, None, img.ctypes.data, 97, 71, 97, 0) == -1
    vf.input_images_keypoints(0, img, img, k, k)
    vf.solve()
    n = len(O.border_filter(k, 97, 71))
    assert len(vf.descriptors(0, 0)[0]) == n > 0 and vf.blur(0, 1).shape == (71, 97)
    raises(-4, vf.descriptors, 1, 0)                                     # the other pair was never solved
    raises(-1, vf.descriptors, 0, 2)
    raises(-1, vf.blur, 0, -1)
    raises(-4, vf.tracks, 0)
    raises(-4, vf.eig, 0)                                                # given keypoints: no detection
    assert lib.loam_vo_frames_descriptors_copy(vf.h, 0, 0, None, None, 0) == n       # the count only
    assert lib.loam_vo_frames_blur_copy(vf.h, 0, 0, None, 0, None) == 97 * 71
    assert len(vf.matches(0)) == vf.result(0)[2].n_matches               # what only a solve writes stays readable
    vf.input_image_pair_match(0, img, img, 0)                            # a later input replaces the data
    raises(-4, vf.descriptors, 0, 0)
    raises(-4, vf.blur, 0, 0)
    vf.solve()
    assert vf.eig(0).shape == (71, 97) and len(vf.descriptors(0, 1)[0]) > 0
    vf.input_descriptors(0, k, np.zeros((50, 32), np.uint8), k, np.zeros((50, 32), np.uint8), 0)
    raises(-4, vf.descriptors, 0, 1)
    raises(-4, vf.eig, 0)
    vf.close()
    long = vo.VOFrames(g, 1, desc_bytes=64)
    long.enable_images(97, 71)
    raises(-1, long.enable_description)                                  # ORB's descriptors have 32 bytes
    long.close()
    lib.loam_debug_live_resources(live)
    assert list(live) == start


# ---------------------------------------------------------------------------------------- 6
def test_cxx_shim_reproduces_python(depth, tmp_path):
    g, clouds = depth
    prev, curr, per, m = scene_models(320, 96, 2)
    vf = vo.VOFrames(g, 1)
    vf.enable_images(320, 96)
    vf.enable_detection()
    vf.enable_description()
    vf.input_image_pair_match(0, strided(prev, 7), strided(curr, 7), 0)
    vf.set_initial(0, X_INIT)
    vf.solve()
    x, lm, st = vf.result(0)
    lib_dir = os.path.dirname(_core.LIB_PATH)
    exe, path = str(tmp_path / "vo_orb_check"), str(tmp_path / "pair.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "vo_orb_check.cpp"), "-o", exe, "-L", lib_dir,
                    "-lloam_core", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True)
    with open(path, "wb") as f:
        f.write(np.array([len(clouds[0]), 320, 96, 327], np.int32).tobytes())
        for a in (KITTI_CAM_T_VELO, KITTI_RECT0_T_CAM, KITTI_P_RECT0):
            f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(X_INIT.astype(np.float64).tobytes())
        for a in (clouds[0], strided(prev, 7).base, strided(curr, 7).base):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        rows.setdefault(key, []).append(vals)
    assert [float.fromhex(v) for v in rows["x"][0]] == x.tolist()
    assert [int(v) for v in rows["lm"][0][:4]] == [lm.iterations, lm.successful, lm.invalid, lm.termination]
    assert [float.fromhex(v) for v in rows["lm"][0][4:]] == [lm.initial_cost, lm.final_cost]
    assert [int(v) for v in rows["stats"][0]] == counters(st)
    assert np.array_equal(np.array(rows["m"], np.int32), m) and len(m) == 51
    for image in (0, 1):
        got = rows[f"k{image}"]
        xy = np.array([[float.fromhex(v) for v in t[:2]] for t in got], F)
        desc = np.array([list(bytes.fromhex(t[2])) for t in got], np.uint8)
        assert same_bits(xy, per[image][2]) and np.array_equal(desc, per[image][3])
    vf.close()
