"""GPU: Shi-Tomasi corner detection on the device in front of the tracker
(loam_vo_frames_enable_detection / _input_image_pair / _eig_copy) against the numpy restatement of
cv::goodFeaturesToTrack (tests/gftt_np.py), bit for bit.
 1. the eigenvalue plane at sizes no tile divides, under a maximum larger than the image, for
    block 3, 4, 5 and 15;
 2. corners (points, count, order) at small sizes and 333 x 171, on noise cut at 64 corners, with
    other distances and quality levels, on the planted-tie, the plateau and the constant image;
 3. 1241 x 376 on the scene and on noise (more candidates than one sort tile holds);
 4. fused frame: input_image_pair equals input_images fed with the model's corners;
 5. batch: six pairs of all four modes in one handle equal their single-pair calls;
 6. candidate overflow; 7. state and argument errors, the handle's resources;
 8. the C++ shim reproduces Python's corners and pose.
The counts of candidates, corners and ties asserted here are the committed model's own on these
inputs: a drifting input is noticed."""
import ctypes

import numpy as np
import pytest

import gftt_np as G
import lk_np as L
from loam_amd import _core, vo
from vo_frames_util import X_INIT, counters, give, make_depth, raises, run_shim, same_bits, same_lm, strided

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def depth():
    return make_depth()


def noise(w, h):
    return np.random.default_rng(0).integers(0, 256, (h, w), dtype=np.uint8)


_MODEL = {}


def model(key, img, **kw):
    """the model's corners and its info, computed once per input"""
    if key not in _MODEL:
        info = {}
        _MODEL[key] = G.good_features_to_track(img, info=info, **kw), info
    return _MODEL[key]


def detect(g, img, extra_wh=(0, 0), max_keypoints=1024, **kw):
    """(corners, eig plane, frame stats, LM stats) of one detection; the image is tracked onto itself"""
    h, w = img.shape
    vf = vo.VOFrames(g, 1, max_keypoints=max_keypoints)
    vf.enable_images(w + extra_wh[0], h + extra_wh[1])
    vf.enable_detection(**kw)
    vf.input_image_pair(0, strided(img), strided(img), 0, 0)
    vf.solve()
    _, lm, st = vf.result(0)
    out = vf.tracks(0)[0], vf.eig(0), st, lm
    vf.close()
    return out


def assert_corners(got, ref):
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.shape, ref.shape)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert len(bad) == 0, (bad[:8], got[bad[:8]], ref[bad[:8]])


# ---------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("block", [5, 3, 4, 15])
@pytest.mark.parametrize("w,h,seed", [(64, 48, 1), (97, 65, 2), (131, 67, 3)])
def test_eig_plane_is_the_models(depth, w, h, seed, block):
    g, _ = depth
    img = L.Scene(seed).render(w, h)
    ref = G.min_eigen(img, block)
    _, eig, _, _ = detect(g, img, extra_wh=(7, 3), block_size=block)
    bad = np.argwhere(eig.view(np.uint32) != ref.view(np.uint32))
    assert eig.shape == ref.shape and len(bad) == 0, (len(bad), bad[:6])


# ---------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("w,h,seed,n_cand,n_corners", [
    (64, 48, 1, 37, 19), (97, 65, 2, 77, 44), (128, 96, 3, 237, 96), (333, 171, 4, 791, 400)])
def test_corners_equal_the_model(depth, w, h, seed, n_cand, n_corners):
    g, _ = depth
    img = L.Scene(seed).render(w, h)
    ref, info = model(("scene", w, h, seed), img)
    assert (len(info["idx"]), len(ref), info["ties"]) == (n_cand, n_corners, 0)
    got, _, st, _ = detect(g, img)
    assert_corners(got, ref)
    assert st.n_knn == n_corners


def test_noise_is_cut_at_max_corners(depth):
    g, _ = depth
    img = noise(128, 96)
    ref, info = model("noise-64", img, max_corners=64)
    assert len(info["idx"]) == 680 and len(ref) == 64
    assert info["kept"][-1] % 64 not in (0, 63)                  # the cut falls inside a chunk
    got, _, st, _ = detect(g, img, max_corners=64)
    assert_corners(got, ref)
    assert st.n_knn == 64


@pytest.mark.parametrize("kw,n_corners", [
    (dict(min_distance=0.0), 237), (dict(min_distance=3.0), 229), (dict(min_distance=2.5), 231),
    (dict(quality_level=0.5), 2), (dict(min_distance=0.0, max_corners=70), 70),
    (dict(min_distance=1.0), 237), (dict(min_distance=20.0), 22)],
    ids=["d0", "d3", "d2.5", "q0.5", "d0-cut", "d1", "d20"])
def test_other_parameters(depth, kw, n_corners):
    g, _ = depth
    img = L.Scene(3).render(128, 96)
    ref = G.good_features_to_track(img, **kw)
    assert len(ref) == n_corners
    got, _, _, _ = detect(g, img, **kw)
    assert_corners(got, ref)


def test_planted_ties_come_out_higher_index_first(depth):
    g, _ = depth
    img = G.tie_image()
    ref, info = model("tie", img, min_distance=3.0)
    assert (len(info["idx"]), len(ref), info["ties"]) == (54, 51, 27)
    got, _, _, _ = detect(g, img, min_distance=3.0)
    assert_corners(got, ref)
    assert info["val"][0] == info["val"][1] and got[0][0] == info["idx"][0] % 64 > 31.5   # the right one first


def test_plateau_pixels_are_all_candidates(depth):
    g, _ = depth
    img = G.plateau_image()
    ref, info = model("plateau", img)
    assert (len(info["idx"]), len(ref), info["ties"], G.adjacent_ties(info, 64)) == (8, 4, 4, 1)
    got, _, _, _ = detect(g, img)
    assert_corners(got, ref)
    got, _, _, _ = detect(g, img, min_distance=0.0)              # both pixels of the plateau come out
    assert_corners(got, G.good_features_to_track(img, min_distance=0.0))
    assert len(got) == 8


def test_constant_image_has_no_corner(depth):
    g, _ = depth
    img = np.full((48, 64), 77, np.uint8)
    got, eig, st, lm = detect(g, img)
    assert len(got) == 0 and not eig.any() and st.n_knn == 0 and lm.termination == 4


# ---------------------------------------------------------------------------------------- 3
def test_kitti_size_scene(depth):
    g, _ = depth
    img = L.Scene(5).render(1241, 376)
    ref, info = model("kitti-scene", img)
    assert (len(info["idx"]), len(ref), info["ties"]) == (7802, 1024, 3)
    got, eig, st, _ = detect(g, img)
    assert same_bits(eig, info["eig"])
    assert_corners(got, ref)
    assert st.n_knn == 1024


def test_kitti_size_noise(depth):
    g, _ = depth
    img = noise(1241, 376)
    ref, info = model("kitti-noise", img)
    assert (len(info["idx"]), info["ties"]) == (26724, 28) and len(ref) == 1024
    got, _, _, _ = detect(g, img)
    assert_corners(got, ref)
    ref_all = G.good_features_to_track(img, max_corners=8192, min_distance=3.0)
    got, _, _, _ = detect(g, img, max_keypoints=8192, max_corners=8192, min_distance=3.0)
    assert len(ref_all) > 5000                                   # deep into the sorted list
    assert_corners(got, ref_all)


# ---------------------------------------------------------------------------------------- 4
def assert_same_frame(a, pa, b, pb):
    (xa, la, sa), (xb, lb, sb) = a.result(pa), b.result(pb)
    assert same_bits(xa, xb) and same_lm(la, lb) and counters(sa) == counters(sb)
    (ra, da), (rb, db) = a.records(pa), b.records(pb)
    assert same_bits(ra, rb) and same_bits(da, db)
    assert np.array_equal(a.matches(pa), b.matches(pb))
    for u, v in zip(a.tracks(pa), b.tracks(pb)):
        assert same_bits(u, v)


@pytest.fixture(scope="module")
def kitti_pair():
    sc = L.Scene(5)
    return sc.render(1241, 376), sc.render(1241, 376, t=(1.7, -0.6))


@pytest.mark.parametrize("detect_on", [0, 1])
def test_fused_frame_equals_images_of_the_models_corners(depth, kitti_pair, detect_on):
    g, _ = depth
    prev, curr = kitti_pair
    pts, _ = model(("kitti-pair", detect_on), (prev, curr)[detect_on])
    assert len(pts) == 1024
    a = vo.VOFrames(g, 1)
    a.enable_images(1241, 376)
    a.enable_detection()
    a.input_image_pair(0, prev, curr, detect_on, 1)
    a.set_initial(0, X_INIT)
    a.solve()
    b = vo.VOFrames(g, 1)
    b.enable_images(1241, 376)
    b.input_images(0, prev, curr, pts, 1)
    b.set_initial(0, X_INIT)
    b.solve()
    assert_same_frame(a, 0, b, 0)
    assert_corners(a.tracks(0)[0], pts)
    s = a.result(0)[2]
    assert s.n_knn == 1024 and s.n_matches > 700 and s.n_gated > 50
    print(f"fused detect frame (detect_on {detect_on}): tracked {s.n_matches}/1024, gated {s.n_gated}, {s.ms:.3f} ms")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- 5
def test_batch_equals_single_pairs(depth, kitti_pair):
    g, _ = depth
    rng = np.random.default_rng(12)
    sc = L.Scene(13)
    prev, curr = kitti_pair
    img = lambda w, h, t: (sc.render(w, h), sc.render(w, h, t=t))
    kp = lambda n: np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 374, n)], axis=1).astype(np.float32)
    d0, d1 = rng.integers(0, 256, (300, 32), dtype=np.uint8), rng.integers(0, 256, (280, 32), dtype=np.uint8)
    d1[:200] = d0[:200]
    k0, k1 = kp(300), kp(280)
    k1[:200] = k0[:200] + rng.normal(0, 4, (200, 2)).astype(np.float32)
    pts = kp(150)
    nxt, st, _ = L.track(prev, curr, pts)
    items = [("image_pair", (*img(128, 96, (1.0, -0.5)), 0), 0, X_INIT),
             ("descriptors", (k0, d0, k1, d1), 0, None),
             ("image_pair", (*img(200, 61, (2.0, 0.5)), 1), 1, None),
             ("tracks", (pts, nxt, st), 1, 0.5 * X_INIT),
             ("images", (*img(97, 65, (0.5, 0.5)), kp(40) * np.float32(0.07)), 0, None),
             ("image_pair", (prev, curr, 0), 1, None)]
    batch = vo.VOFrames(g, len(items), max_keypoints=1024)
    batch.enable_images(1241, 376)
    batch.enable_detection()
    for p, item in enumerate(items):
        give(batch, p, item)
    batch.solve()
    for p, item in enumerate(items):
        one = vo.VOFrames(g, 1, max_keypoints=1024)
        if item[0] in ("images", "image_pair"):
            one.enable_images(*item[1][0].shape[::-1])           # its own maximum: another layout
        if item[0] == "image_pair":
            one.enable_detection()
        give(one, 0, item)
        one.solve()
        (xa, la, sa), (xb, lb, sb) = batch.result(p), one.result(0)
        assert same_bits(xa, xb) and same_lm(la, lb) and counters(sa) == counters(sb), p
        if item[0] != "descriptors":
            for u, v in zip(batch.tracks(p), one.tracks(0)):
                assert same_bits(u, v), p
        if item[0] == "image_pair":
            assert same_bits(batch.eig(p), one.eig(0)), p
        one.close()
    assert_corners(batch.tracks(5)[0], model(("kitti-pair", 0), prev)[0])
    assert batch.result(0)[2].n_knn > 20 and batch.result(2)[2].n_knn > 20 and batch.result(5)[2].n_gated > 50
    # a second solve of one detect pair only: the others keep their results and their corners
    before = batch.result(5)[0], batch.tracks(5)[0]
    give(batch, 0, items[0])
    batch.solve()
    assert same_bits(batch.result(5)[0], before[0]) and same_bits(batch.tracks(5)[0], before[1])
    batch.close()


# ---------------------------------------------------------------------------------------- 6
def test_candidate_overflow(depth):
    g, _ = depth
    img, ok = noise(128, 96), L.Scene(3).render(128, 96)
    vf = vo.VOFrames(g, 2)
    vf.enable_images(128, 96)
    vf.enable_detection(max_candidates=32)                       # the scene has 237, the noise 680
    vf.input_image_pair(0, img, img, 0, 0)
    vf.input_image_pair(1, ok[:30, :40], ok[:30, :40], 0, 0)     # few enough candidates
    vf.solve()
    text = raises(-3, vf.result, 0)
    assert "max_candidates" in text and "680" in text and "32" in text
    ref = G.good_features_to_track(ok[:30, :40])
    assert len(ref) == 11 and len(G.candidates(G.min_eigen(ok[:30, :40]), 0.03)[1]) == 27
    assert_corners(vf.tracks(1)[0], ref)
    assert vf.result(1)[2].n_knn == len(ref) and len(vf.tracks(0)[0]) == 0
    vf.input_image_pair(0, ok[:30, :40], ok[:30, :40], 0, 0)     # the handle is usable afterwards
    vf.solve()
    assert_corners(vf.tracks(0)[0], ref)
    assert vf.result(0)[2].n_knn == len(ref)
    vf.close()


# ---------------------------------------------------------------------------------------- 7
def test_errors_and_resources(depth):
    g, _ = depth
    lib = _core.lib()
    live = (ctypes.c_int64 * 4)()
    lib.loam_debug_live_resources(live)
    start = list(live)
    img = L.Scene(1).render(64, 48)
    vf = vo.VOFrames(g, 2, max_keypoints=64)
    raises(-4, vf.enable_detection, max_corners=64)              # LOAM_ERR_STATE: before enable_images
    vf.enable_images(64, 48)
    raises(-4, vf.input_image_pair, 0, img, img, 0, 0)           # before enable_detection
    for kw in (dict(max_corners=0), dict(max_corners=65), dict(quality_level=0.0), dict(quality_level=np.nan),
               dict(min_distance=-1.0), dict(min_distance=np.inf), dict(block_size=1), dict(block_size=16),
               dict(max_candidates=0)):
        raises(-1, vf.enable_detection, **{**dict(max_corners=64), **kw})
    vf.enable_detection(max_corners=64)
    raises(-4, vf.enable_detection, max_corners=64)              # once per handle
    raises(-4, vf.eig, 0)                                        # never solved
    raises(-1, vf.input_image_pair, 0, img, img, 2, 0)           # detect_on
    raises(-1, vf.input_image_pair, 2, img, img, 0, 0)
    raises(-1, vf.input_image_pair, 0, img, img, 0, 2)
    raises(-3, vf.input_image_pair, 0, np.zeros((48, 65), np.uint8), np.zeros((48, 65), np.uint8), 0, 0)
    assert lib.loam_vo_frames_input_image_pair(vf.h, 0, None, img.ctypes.data, 64, 48, 64, 0, 0) == -1
    assert lib.loam_vo_frames_input_image_pair(vf.h, 0, img.ctypes.data, img.ctypes.data, 64, 48, 63, 0, 0) == -1
    vf.input_image_pair(0, img, img, 0, 0)
    vf.solve()
    assert len(vf.tracks(0)[0]) == 19 and vf.eig(0).shape == (48, 64)
    raises(-4, vf.eig, 1)                                        # the other pair was never solved
    assert lib.loam_vo_frames_eig_copy(vf.h, 0, None, 0, None) == 64 * 48   # the size only
    vf.input_image_pair(0, img, img, 1, 0)                       # a later input replaces the plane
    raises(-4, vf.eig, 0)
    raises(-4, vf.tracks, 0)
    vf.close()
    big = vo.VOFrames(g, 100, max_keypoints=64)
    big.enable_images(64, 48)
    raises(-3, big.enable_detection, max_corners=64, max_candidates=1 << 22)   # LOAM_ERR_CAPACITY: over 2 GiB
    big.close()
    wide = vo.VOFrames(g, 1, max_keypoints=64)
    wide.enable_images(70000, 16)
    raises(-3, wide.enable_detection, max_corners=64)            # a side over 65535
    wide.close()
    lib.loam_debug_live_resources(live)
    assert list(live) == start


# ---------------------------------------------------------------------------------------- 8
def test_cxx_shim_reproduces_python(depth, kitti_pair, tmp_path):
    g, clouds = depth
    prev, curr = kitti_pair
    vf = vo.VOFrames(g, 1)
    vf.enable_images(1241, 376)
    vf.enable_detection()
    vf.input_image_pair(0, strided(prev, 7), strided(curr, 7), 1, 0)
    vf.set_initial(0, X_INIT)
    vf.solve()
    x, lm, st = vf.result(0)
    tp, tc, ts, te = vf.tracks(0)
    lines, got_t = run_shim(tmp_path, "detect", [len(clouds[0]), 1241, 376, 1248, 1],
                            [clouds[0], strided(prev, 7).base, strided(curr, 7).base])
    assert [float.fromhex(v) for v in lines["x"]] == x.tolist()
    assert [int(v) for v in lines["lm"][:4]] == [lm.iterations, lm.successful, lm.invalid, lm.termination]
    assert [float.fromhex(v) for v in lines["lm"][4:]] == [lm.initial_cost, lm.final_cost]
    assert [int(v) for v in lines["stats"]] == counters(st)
    assert len(got_t) == len(tp) == 1024
    xy = np.array([[float.fromhex(v) for v in t[:4]] for t in got_t], np.float32)
    assert same_bits(xy[:, :2], tp) and same_bits(xy[:, 2:], tc)
    assert [int(t[4]) for t in got_t] == ts.tolist()
    assert same_bits(np.array([float.fromhex(t[5]) for t in got_t], np.float32), te)
    assert st.n_gated > 50
    vf.close()
