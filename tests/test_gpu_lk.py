"""GPU: pyramidal Lucas-Kanade on the device in front of the VO frame
(loam_vo_frames_enable_images / _input_images / _tracks_copy) against the numpy restatement of
cv::calcOpticalFlowPyrLK (tests/lk_np.py), bit for bit.
 1. pyramids: read back through loam_vo_frames_pyramid_copy (a debug copy in the pattern of
    _tracks_copy), byte-identical to the model, from images whose row stride exceeds their width;
 2. tracks: curr_xy, status and err bit-identical to the model for n around the wavefront and over
    several workgroups, with points planted at integer and .5 coordinates, within 8 px of every
    edge (reflected reads), outside the image and in the flat patch, under a shift large enough to
    run into the iteration cap and on a scene where the model stops by the oscillation rule; one
    case at KITTI's 1241 x 376;
 3. other parameters: another window (also one that takes the 16-pass kernel), more levels, one
    iteration, and an image whose level count shrinks;
 4. fused frame: input_images equals input_tracks fed with the model's tracks in result, LM stats,
    counters and records, bit for bit;
 5. batch: five pairs of all three modes in one handle equal their single-pair calls;
 6. errors; 7. the C++ shim reproduces the Python tracks and pose bit for bit."""
import numpy as np
import pytest

import lk_np as L
from loam_amd import _core, vo
from vo_frames_util import X_INIT, counters, give, make_depth, raises, run_shim, same_bits, same_lm, strided

pytestmark = pytest.mark.gpu

W, H = 97, 65
NS = (0, 1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def depth():
    return make_depth()


def planted_points(rng, w, h, flat, n):
    """n points: an interior one first, then integer and .5 coordinates, points within 8 px of
    every edge and in the corners, points outside the image on either side of the bounds check
    (floor(p - 7) = -16 fails, -15 passes and reads reflected pixels), an infinity, points in the flat
    patch, a grid over the whole image, and random ones up to 10 px outside"""
    x0, y0, x1, y1 = flat
    special = [(w - 20.3, 12.4), (20, 10), (20.5, 10.5), (w - 17.0, h - 9.5), (3.2, 30), (w - 3.1, 33), (50.3, 2.1),
               (51, h - 2.3), (1, 1), (w - 1.5, h - 1.5), (0, h - 1), (7.75, 7.25),
               (-9.0, 10), (w + 7.5, 20), (40, -8.01), (40, h + 7), (-7.99, 40), (w + 6.99, 40), (30, -7.5),
               (np.inf, 5), (1e12, 5), (-300, -300),
               ((x0 + x1) / 2, (y0 + y1) / 2), (x0 + 9.5, y0 + 9.5), (x1 - 9, y1 - 9.25)]
    gx, gy = np.meshgrid(np.arange(4, w - 3, 6.5), np.arange(4, h - 3, 6.5))
    pts = np.concatenate([np.array(special), np.stack([gx.ravel(), gy.ravel()], axis=1)])
    more = np.stack([rng.uniform(-10, w + 10, n), rng.uniform(-10, h + 10, n)], axis=1)
    return np.concatenate([pts, more])[:n].astype(np.float32)


def device_tracks(g, prev, curr, pts, stream=0, **lk):
    h, w = prev.shape
    vf = vo.VOFrames(g, 1, max_keypoints=max(len(pts), 1))
    vf.enable_images(w, h, **lk)
    vf.input_images(0, strided(prev), strided(curr), pts, stream)
    vf.solve()
    out = vf.tracks(0), vf.result(0)[2]
    vf.close()
    return out


def assert_tracks(got, pts, ref):
    prev, curr, status, err = got
    nxt, st, er = ref
    assert same_bits(prev, np.asarray(pts, np.float32).reshape(-1, 2))
    assert np.array_equal(status, st), np.nonzero(status != st)[0]
    bad = np.nonzero((curr.view(np.uint32) != nxt.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (bad[:8], curr[bad[:8]], nxt[bad[:8]])
    assert same_bits(err, er), np.nonzero(err != er)[0]


# ---------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("w,h", [(64, 48), (97, 65), (128, 96)])
def test_pyramids_are_the_models(depth, w, h):
    g, _ = depth
    sc = L.Scene(w)
    prev, curr = sc.render(w, h), sc.render(w, h, t=(1.5, -0.75))
    vf = vo.VOFrames(g, 1)
    vf.enable_images(w + 3, h + 5)                               # the maximum is not the image
    vf.input_images(0, strided(prev), strided(curr), np.zeros((0, 2), np.float32), 0)
    vf.solve()
    for image, img in enumerate((prev, curr)):
        ref, got = L.build_pyramid(img), vf.pyramid(0, image)
        assert len(got) == len(ref) == (2 if (w, h) == (64, 48) else 3)
        for a, b in zip(got, ref):
            assert same_bits(a, b)
    assert len(vf.tracks(0)[2]) == 0 and vf.result(0)[1].termination == 4
    vf.close()


# ---------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def small():
    """97 x 65, a shift of (12, 6): 3 px at the top level, several points run into the iteration
    cap and one stops by the oscillation rule (tests/test_lk_host.py checks the same scene)"""
    sc = L.Scene(8)
    prev, curr = sc.render(W, H), sc.render(W, H, t=(12.0, 6.0))
    pts = planted_points(np.random.default_rng(2), W, H, sc.flat, max(NS))
    info = {}
    ref = L.track(prev, curr, pts, info=info)
    return prev, curr, pts, ref, info


def test_planted_cases_are_what_they_claim(small):
    prev, curr, pts, (nxt, st, err), info = small
    assert info["cap"].any() and (info["osc"] & (st == 1)).any()
    assert not st[12:16].any() and not err[12:16].any()           # more than win outside
    assert not st[19:22].any()                                    # infinity, 1e12, far away
    assert not st[22:25].any()                                    # the flat patch
    assert st[:12].sum() >= 6 and 0.3 < st.mean() < 0.95 and err[st == 1].max() > 0


@pytest.mark.parametrize("n", NS)
def test_tracks_equal_the_model(depth, small, n):
    g, _ = depth
    prev, curr, pts, (nxt, st, err), _ = small
    got, stats = device_tracks(g, prev, curr, pts[:n])
    assert_tracks(got, pts[:n], (nxt[:n], st[:n], err[:n]))
    assert stats.n_knn == n and stats.n_matches == int((st[:n] == 1).sum())


def test_tracks_kitti_size(depth):
    g, _ = depth
    w, h = 1241, 376
    sc = L.Scene(3, flat=(600.0, 100.0, 640.0, 140.0))
    prev, curr = sc.render(w, h), sc.render(w, h, t=(-2.3, 0.8))
    rng = np.random.default_rng(9)
    pts = np.concatenate([[[620, 120], [0.5, 0.5], [w - 1, h - 1], [w + 6.5, 200], [1237.25, 3.5]],
                          np.stack([rng.uniform(0, w, 35), rng.uniform(0, h, 35)], axis=1)]).astype(np.float32)
    ref = L.track(prev, curr, pts)
    assert len(L.build_pyramid(prev)) == 3 and ref[1][0] == 0 and ref[1][5:].mean() > 0.8
    got, _ = device_tracks(g, prev, curr, pts, 1)
    assert_tracks(got, pts, ref)


# ---------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("w,h,lk,levels", [
    (128, 96, dict(win=9, max_level=3), 4),
    (128, 96, dict(win=21, max_level=3), 3),                      # win^2 > 256: the 16-pass kernel
    (128, 96, dict(win=31, max_level=1, max_count=30, epsilon=0.01), 2),
    (97, 65, dict(max_count=1), 3),
    (97, 65, dict(max_level=0, min_eig_threshold=1e-2), 1),
    (64, 48, dict(), 2),                                          # the third level would be 16 x 12
], ids=["win9-4levels", "win21", "win31", "one-iteration", "one-level", "64x48"])
def test_other_parameters(depth, w, h, lk, levels):
    g, _ = depth
    sc = L.Scene(11)
    prev, curr = sc.render(w, h), sc.render(w, h, t=(3.4, -1.7))
    pts = planted_points(np.random.default_rng(w), w, h, sc.flat, 90)
    model = dict(win=lk.get("win", 15), max_level=lk.get("max_level", 2), max_count=lk.get("max_count", 10),
                 epsilon=lk.get("epsilon", 0.03), min_eig=lk.get("min_eig_threshold", 1e-4))
    assert len(L.build_pyramid(prev, model["win"], model["max_level"])) == levels
    ref = L.track(prev, curr, pts, **model)
    assert 0.2 < ref[1].mean() < 0.98
    got, _ = device_tracks(g, prev, curr, pts, **lk)
    assert_tracks(got, pts, ref)


# ---------------------------------------------------------------------------------------- 4
@pytest.fixture(scope="module")
def kitti_pair():
    """a 1241 x 376 pair and points over the part of the image the depth scene covers"""
    w, h = 1241, 376
    sc = L.Scene(5, flat=(300.0, 200.0, 340.0, 240.0))
    prev, curr = sc.render(w, h), sc.render(w, h, t=(1.7, -0.6))
    rng = np.random.default_rng(4)
    pts = np.stack([rng.uniform(-5, w + 5, 400), rng.uniform(100, h + 5, 400)], axis=1).astype(np.float32)
    pts[:3] = (320, 220), (310.5, 215.5), (-40, 200)
    return prev, curr, pts, L.track(prev, curr, pts)


def assert_same_frame(a, pa, b, pb):
    (xa, la, sa), (xb, lb, sb) = a.result(pa), b.result(pb)
    assert same_bits(xa, xb) and same_lm(la, lb) and counters(sa) == counters(sb)
    (ra, da), (rb, db) = a.records(pa), b.records(pb)
    assert same_bits(ra, rb) and same_bits(da, db)
    assert np.array_equal(a.matches(pa), b.matches(pb))


@pytest.mark.parametrize("x0", [None, X_INIT], ids=["identity", "prior"])
def test_fused_frame_equals_tracks_of_the_model(depth, kitti_pair, x0):
    g, _ = depth
    prev, curr, pts, (nxt, st, err) = kitti_pair
    a = vo.VOFrames(g, 1)
    a.enable_images(1241, 376)
    a.input_images(0, prev, curr, pts, 1)
    a.set_initial(0, x0)
    a.solve()
    b = vo.VOFrames(g, 1)
    b.input_tracks(0, pts, nxt, st, 1)
    b.set_initial(0, x0)
    b.solve()
    assert_same_frame(a, 0, b, 0)
    assert_tracks(a.tracks(0), pts, (nxt, st, err))
    tb = b.tracks(0)
    assert same_bits(tb[1], nxt) and np.array_equal(tb[2], st) and not tb[3].any()
    s = a.result(0)[2]
    assert s.n_knn == len(pts) and s.n_matches == int(st.sum()) > 250 and s.counter32 > 10 and s.counter22 > 10
    print(f"fused frame: tracked {s.n_matches}/{len(pts)}, gated {s.n_gated}, 32/22 {s.counter32}/{s.counter22}, "
          f"{s.ms:.3f} ms")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- 5
def test_batch_equals_single_pairs(depth, small, kitti_pair):
    g, _ = depth
    rng = np.random.default_rng(12)
    sc = L.Scene(13)
    sizes = [(128, 96, 150), (64, 48, 33), (200, 61, 0)]
    items = []
    for k, (w, h, n) in enumerate(sizes):
        items.append(("images", (sc.render(w, h), sc.render(w, h, t=(1.0 + k, -0.5 * k)),
                                 planted_points(rng, w, h, sc.flat, n)), k % 2, None if k else X_INIT))
    kp = lambda n: np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 374, n)], axis=1).astype(np.float32)
    d0, d1 = rng.integers(0, 256, (300, 32), dtype=np.uint8), rng.integers(0, 256, (280, 32), dtype=np.uint8)
    d1[:200] = d0[:200]
    k0 = kp(300)
    k1 = kp(280)
    k1[:200] = k0[:200] + rng.normal(0, 4, (200, 2)).astype(np.float32)
    items.insert(1, ("descriptors", (k0, d0, k1, d1), 0, None))
    prev, curr, pts, (nxt, st, err) = kitti_pair
    items.insert(3, ("tracks", (pts, nxt, st), 1, 0.5 * X_INIT))
    items.append(("images", (prev, curr, pts[:257]), 1, None))
    batch = vo.VOFrames(g, len(items), max_keypoints=512)
    batch.enable_images(1241, 376)
    for p, item in enumerate(items):
        give(batch, p, item)
    batch.solve()
    for p, item in enumerate(items):
        one = vo.VOFrames(g, 1, max_keypoints=512)
        if item[0] == "images":
            one.enable_images(*item[1][0].shape[::-1])           # its own maximum: another layout
        give(one, 0, item)
        one.solve()
        assert_same_frame(batch, p, one, 0)
        if item[0] != "descriptors":
            for a, b in zip(batch.tracks(p), one.tracks(0)):
                assert same_bits(a, b), p
        if item[0] == "images":
            for image in (0, 1):
                for a, b in zip(batch.pyramid(p, image), one.pyramid(0, image)):
                    assert same_bits(a, b), p
        one.close()
    assert_tracks(batch.tracks(5), pts[:257], (nxt[:257], st[:257], err[:257]))
    assert batch.result(0)[2].n_gated > 20 and batch.result(5)[2].n_gated > 20
    # a second solve of one images pair only: the others keep their results and their tracks
    before = batch.result(5)[0], batch.tracks(5)[1]
    give(batch, 0, items[0])
    batch.solve()
    assert same_bits(batch.result(5)[0], before[0]) and same_bits(batch.tracks(5)[1], before[1])
    batch.close()


# ---------------------------------------------------------------------------------------- 6
def test_errors(depth, small):
    g, _ = depth
    prev, curr, pts, _, _ = small
    vf = vo.VOFrames(g, 2, max_keypoints=64)
    raises(-4, vf.input_images, 0, prev, curr, pts[:10], 0)       # LOAM_ERR_STATE: before enable_images
    for kw in (dict(win=4), dict(win=1), dict(win=33), dict(win=-15), dict(max_level=-1), dict(max_level=8)):
        raises(-1, vf.enable_images, W, H, **kw)                  # LOAM_ERR_ARG
    for w, h in ((0, H), (W, 0), (-1, -1)):
        raises(-1, vf.enable_images, w, h)
    raises(-3, vf.enable_images, 40000, 40000)                    # LOAM_ERR_CAPACITY: over 2 GiB of pyramids
    vf.enable_images(W, H)
    raises(-4, vf.enable_images, W, H)                            # once per handle
    raises(-4, vf.tracks, 0)                                      # never solved
    raises(-3, vf.input_images, 0, np.zeros((H, W + 1), np.uint8), np.zeros((H, W + 1), np.uint8), pts[:10], 0)
    raises(-3, vf.input_images, 0, np.zeros((H + 1, W), np.uint8), np.zeros((H + 1, W), np.uint8), pts[:10], 0)
    raises(-3, vf.input_images, 0, prev, curr, pts[:65], 0)       # n > max_keypoints
    for pair, stream in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        raises(-1, vf.input_images, pair, prev, curr, pts[:10], stream)
    lib = _core.lib()
    assert lib.loam_vo_frames_input_images(vf.h, 0, None, curr.ctypes.data, W, H, W, pts.ctypes.data, 4, 0) == -1
    assert lib.loam_vo_frames_input_images(vf.h, 0, prev.ctypes.data, curr.ctypes.data, W, H, W - 1,
                                           pts.ctypes.data, 4, 0) == -1   # row_stride < width
    vf.input_images(0, prev[:40, :50], curr[:40, :50], pts[:10], 0)      # smaller than the maximum: fine
    vf.solve()
    assert len(vf.tracks(0)[2]) == 10 and len(vf.pyramid(0, 1)) == 2
    raises(-4, vf.tracks, 1)                                      # the other pair was never solved
    raises(-1, lambda: _core.check(lib.loam_vo_frames_pyramid_copy(vf.h, 0, 2, 0, None, 0, None)))
    raises(-1, lambda: _core.check(lib.loam_vo_frames_pyramid_copy(vf.h, 0, 0, 2, None, 0, None)))
    assert lib.loam_vo_frames_tracks_copy(vf.h, 0, None, None, None, None, 5) == 10   # cap too small: the count
    vf.input_images(0, prev, curr, pts[:3], 0)                    # a later input replaces the points
    raises(-4, vf.tracks, 0)
    raises(-4, vf.pyramid, 0, 0)
    rng = np.random.default_rng(1)
    vf.input_descriptors(0, pts[:8], rng.integers(0, 256, (8, 32), dtype=np.uint8), pts[:9],
                         rng.integers(0, 256, (9, 32), dtype=np.uint8), 0)   # replaces the images input
    vf.solve()
    raises(-4, vf.tracks, 0)                                      # solved from descriptors
    vf.close()


# ---------------------------------------------------------------------------------------- 7
def test_cxx_shim_reproduces_python(depth, kitti_pair, tmp_path):
    g, clouds = depth
    prev, curr, pts, _ = kitti_pair
    pts = pts[:200]
    vf = vo.VOFrames(g, 1)
    vf.enable_images(1241, 376)
    vf.input_images(0, strided(prev, 7), strided(curr, 7), pts, 0)
    vf.set_initial(0, X_INIT)
    vf.solve()
    x, lm, st = vf.result(0)
    tp, tc, ts, te = vf.tracks(0)
    lines, got_t = run_shim(tmp_path, "images", [len(clouds[0]), 1241, 376, 1248, len(pts)],
                            [clouds[0], strided(prev, 7).base, strided(curr, 7).base, pts])
    assert [float.fromhex(v) for v in lines["x"]] == x.tolist()
    assert [int(v) for v in lines["lm"][:4]] == [lm.iterations, lm.successful, lm.invalid, lm.termination]
    assert [float.fromhex(v) for v in lines["lm"][4:]] == [lm.initial_cost, lm.final_cost]
    assert [int(v) for v in lines["stats"]] == counters(st)
    assert len(got_t) == len(pts)
    xy = np.array([[float.fromhex(v) for v in t[:4]] for t in got_t], np.float32)
    assert same_bits(xy[:, :2], tp) and same_bits(xy[:, 2:], tc)
    assert [int(t[4]) for t in got_t] == ts.tolist()
    assert same_bits(np.array([float.fromhex(t[5]) for t in got_t], np.float32), te)
    assert st.n_gated > 50
    vf.close()
