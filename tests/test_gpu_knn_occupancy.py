"""The 5-NN search's cell occupancy blocks (cubeindex.h, k_knn's occupied-cell loop).

Every case runs the same inputs through a handle with the blocks and through one created with
LOAM_KNN_OCC=0 (no cube has a block: every cell is probed, the path before the blocks), and asks
for bit-identical neighbours, record types, records, poses and candidate counts.  One stream runs
the cell-split kernel, which does not read the blocks: a handle of at most four streams builds none
(its counters stay 0, and its two runs check that the switch leaves it alone); eight streams run the
one-lane-per-query kernel that reads them.

The neighbours are also checked against brute force:
  * planted maps, first frame: coordinates in eighths of a metre, so the float32 distances are exact
    and the reference is the 5 smallest (d2, submap index) of the window's points, in that order;
  * later frames and the synthetic frame: test_gpu_corr's Ref5 (float64 tree, queries decided
    where float32 rounding cannot change the answer).
"""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from helpers import load_state
from loam_amd.mapping import BatchMapper
from test_gpu_corr import CEN, Planted, Ref5, _cube_of, _planted, frame, submap, window_cubes  # noqa: F401

gpu = pytest.mark.gpu
IN_USE, ALLOC_FAIL, COMPACTIONS = 92, 93, 41  # loam_mapper_debug_counters slots
E = 0.125


def _planted_occ():
    """test_gpu_corr's directed cases (cube faces, the 1 m bound, fewer than 5 in reach, cubes outside
    the window) and the ones the occupied-cell loop adds"""
    P = _planted()
    near4 = [(-2 * E, 0, 0), (2 * E, 0, 0), (0, -2 * E, 0), (0, 2 * E, 0)]
    # sparse: the only occupied cells are the query's own and a few around it; the 5th neighbour lies in
    # a corner cell (dx = dy = dz = +1) of the 3 x 3 x 3
    P.add("5th in a corner cell, corner", 0, (10.875, 10.875, 4.875), [(s * E, s * E, s * E) for s in (-2, -1, 1, 2, 3, 9)])
    P.add("5th in a corner cell, surf", 1, (20.875, -9.125, 6.875),
          [(-E, -E, 0), (0, 0, -2 * E), (-2 * E, -2 * E, E), (-E, -E, -3 * E), (3 * E, 3 * E, 3 * E), (6 * E, 6 * E, 0)])
    # four points in reach, the rest of the 27 cells empty but one far corner cell that holds a point
    # just out of reach
    P.add("four in reach and a far corner", 1, (-20.5, -30.5, 6.5), near4, extra=[(-19.75, -29.75, 7.25)])
    # equal distances: four at 1/4 m in one cell, then two candidates for the 5th at 3/8 m in that cell
    P.add("ties in one cell", 1, (-30.5, 30.5, 2.5), near4 + [(0, 3 * E, 0), (3 * E, 0, 0)])
    # ... and at 5/8 m in the cells on either side (visited in another order than they are filed)
    P.add("ties across cells", 1, (-40.5, 30.5, 2.5), near4 + [(5 * E, 0, 0), (-5 * E, 0, 0)])
    P.add("ties across cells, filed the other way", 1, (-40.5, 20.5, 2.5), near4 + [(-5 * E, 0, 0), (5 * E, 0, 0)])
    P.add("ties across cells y", 1, (-40.5, 10.5, 2.5), near4 + [(0, -5 * E, 0), (0, 5 * E, 0)])
    # a cube corner: x + 25 and y + 25 exact negative multiples of 50 (local coordinate 50 in the cubes
    # below), z + 25 = 50; neighbours in the four cubes around the vertical edge, and along it
    ring0 = [(0, 0, 0), (-2 * E, 0, 0), (3 * E, 0, 0), (0, -4 * E, 0), (0, 5 * E, 0), (-3 * E, -3 * E, 0), (6 * E, 5 * E, 0)]
    P.add("cube corner surf", 1, (-75, -75, 25), ring0)
    P.add("cube corner corner", 0, (-75, -75, 25), [(0, 0, s * E) for s in (0, -3, 3, -5, 6, 9)])
    P.add("cube corner off by a cell", 1, (24.5, -75.5, 24.5), [(-4 * E, 0, 0), (4 * E, 0, 0), (0, -4 * E, 0), (0, 4 * E, 0), (-5 * E, 4 * E, 0), (7 * E, 0, 0)])
    return P


def _cubes(pts, off=(0.0, 0.0, 0.0)):
    out = {}
    for p in pts:
        p = np.asarray(p, np.float64) + np.asarray(off)
        c = [_cube_of(float(p[a]), CEN[a]) for a in range(3)]
        assert all(0 <= c[a] < (21, 21, 11)[a] for a in range(3))
        out.setdefault(c[0] + 21 * c[1] + 441 * c[2], []).append([p[0], p[1], p[2], 0.0])
    return {c: np.array(v, np.float32) for c, v in out.items()}


def _state(P, off=(0.0, 0.0, 0.0), extra=((), ())):
    return dict(cen=np.array(CEN, np.int32), q=np.array([0, 0, 0, 1.0]), t=np.zeros(3),
                corner=_cubes(list(P.pts[0]) + list(extra[0]), off), surf=_cubes(list(P.pts[1]) + list(extra[1]), off))


def _mapper(monkeypatch, n_streams, occ=True, blocks=None, **params):
    monkeypatch.delenv("LOAM_KNN_OCC", raising=False)
    monkeypatch.delenv("LOAM_KNN_OCC_BLOCKS", raising=False)
    if not occ:
        monkeypatch.setenv("LOAM_KNN_OCC", "0")
    if blocks is not None:
        monkeypatch.setenv("LOAM_KNN_OCC_BLOCKS", str(blocks))
    m = BatchMapper(n_streams, **params)  # the switches are read at create
    monkeypatch.delenv("LOAM_KNN_OCC", raising=False)
    monkeypatch.delenv("LOAM_KNN_OCC_BLOCKS", raising=False)
    m.set_profiling(n_streams > 4)  # the correspondence family's bytes carry the candidate counts
    return m


def _frame(m, clouds, q_wodom, t_wodom):
    """one solve of every stream; what the frame left, per stream, and the candidate bytes"""
    m.reset_kernel_times()
    for s in range(m.n_streams):
        m.input(s, clouds[0], clouds[1], q_wodom, t_wodom)
    m.solve()
    out = []
    for s in range(m.n_streams):
        st = m.stats(s)
        out.append(dict(corr=m.corr(s), pose=m.pose(s), center=tuple(st.center), optimized=st.optimized,
                        nums=(list(st.corner_num), list(st.surf_num)), stacks=(st.corner_stack, st.surf_stack),
                        iters=[st.lm[r].iterations for r in range(2)]))
    return out, m.kernel_times()["correspondence"]["bytes"]


def _same(a, b, what):
    (ra, ca), (rb, cb) = a, b
    assert ca == cb, (what, "candidate bytes", ca, cb)
    for s, (x, y) in enumerate(zip(ra, rb)):
        for k in ("center", "optimized", "nums", "stacks", "iters"):
            assert x[k] == y[k], (what, s, k, x[k], y[k])
        for u, v in zip(x["pose"], y["pose"]):
            assert np.array_equal(u, v), (what, s, "pose")
        for u, v, name in zip(x["corr"], y["corr"], ("x0", "type", "records", "neighbours")):
            assert np.array_equal(u, v, equal_nan=True), (what, s, name)


def _exact_brute_force(res, cubes, clouds, t):
    """planted coordinates: the 5 smallest (d2, submap index), float32 distances being exact"""
    x0, typ, recs, nbr = res["corr"]
    nc = res["stacks"][0]
    for w, (lo, hi) in enumerate(((0, nc), (nc, len(typ)))):
        po = recs[lo:hi, 1:4]
        assert np.array_equal(np.sort(po.astype(np.float32).view(np.uint32), axis=0),
                              np.sort(clouds[w][:, :3].view(np.uint32), axis=0))  # the stack left the queries alone
        q = (Rotation.from_quat(x0[:4]).apply(po) + x0[4:]).astype(np.float32)
        assert np.array_equal(q, (po + np.asarray(t)).astype(np.float32)), "the search started off the planted pose"
        sub = submap(cubes[w], res["center"])
        d = sub[None, :, :] - q[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]  # L2_Simple<float>, exact here
        assert np.array_equal(d2 * 64 * 64, np.round(d2 * 64 * 64))
        order = np.lexsort((np.broadcast_to(np.arange(len(sub)), d2.shape), d2), axis=1)[:, :5]
        d5 = np.take_along_axis(d2, order, axis=1)[:, 4]
        ok = d5 < 1.0
        got = nbr[lo:hi]
        assert np.array_equal(np.isnan(got).any(axis=(1, 2)), ~ok), w
        assert np.array_equal(got[ok], sub[order[ok]]), w
        assert ok.sum() >= 5 and (~ok).sum() >= 2, (w, ok.sum())


def _ref5_check(m, s, before, res, what):
    x0, typ, recs, nbr = res["corr"]
    nc = res["stacks"][0]
    for (lo, hi), w in (((0, nc), 0), ((nc, len(typ)), 1)):
        Ref5(submap(before[w], res["center"]), recs[lo:hi, 1:4], x0).check(typ[lo:hi], nbr[lo:hi], f"{what} map {w}")


def _builds(n_streams, occ=True):
    """whether a handle of n_streams builds occupancy blocks"""
    return occ and n_streams > 4


def _nonempty(m):
    return sum(len(m.cubes(s, w)) for s in range(m.n_streams) for w in range(2))


IDENT_Q, ZERO_T = np.array([0, 0, 0, 1.0]), np.zeros(3)


@gpu
@pytest.mark.parametrize("n_streams", [1, 8])
def test_planted_map_sparse_boundaries_ties(n_streams, monkeypatch):
    """sparse map, 5th neighbour in a corner cell, fewer than 5 in reach, cube faces and a cube corner
    (local coordinate 50 in the cube below), equal distances within a cell and across cells"""
    P = _planted_occ()
    clouds, state = [P.cloud(0), P.cloud(1)], _state(P)
    runs = {}
    for occ in (True, False):
        m = _mapper(monkeypatch, n_streams, occ=occ)
        for s in range(n_streams):
            load_state(m, s, state)
        c = m.debug_counters()
        assert c[IN_USE] == ((len(state["corner"]) + len(state["surf"])) * n_streams if _builds(n_streams, occ) else 0) and c[ALLOC_FAIL] == 0
        runs[occ] = _frame(m, clouds, IDENT_Q, ZERO_T)
        for res in runs[occ][0]:
            assert res["optimized"] == 1 and res["center"] == CEN
            _exact_brute_force(res, (state["corner"], state["surf"]), clouds, ZERO_T)
        c = m.debug_counters()
        assert c[IN_USE] == (_nonempty(m) if _builds(n_streams, occ) else 0) and c[ALLOC_FAIL] == 0
        m.close()
    _same(runs[True], runs[False], "blocks on / off")


@gpu
def test_pool_exhaustion_falls_back_and_counts(monkeypatch):
    """a pool of 3 blocks per (stream, map): the other cubes have no block and are probed as before;
    identical results, and the allocation-failure counter says so"""
    P = _planted_occ()
    clouds, state = [P.cloud(0), P.cloud(1)], _state(P)
    assert min(len(state["corner"]), len(state["surf"])) > 3
    runs = {}
    for key, kw in (("small", dict(blocks=3)), ("off", dict(occ=False))):
        m = _mapper(monkeypatch, 8, **kw)
        for s in range(8):
            load_state(m, s, state)
        a = _frame(m, clouds, IDENT_Q, ZERO_T)
        for res in a[0]:
            _exact_brute_force(res, (state["corner"], state["surf"]), clouds, ZERO_T)
        b = _frame(m, clouds, IDENT_Q, ZERO_T)  # over cubes the re-VoxelGrid rebuilt, with and without a block
        runs[key] = (a, b)
        c = m.debug_counters()
        if key == "small":
            assert c[IN_USE] == 3 * 2 * 8 and c[ALLOC_FAIL] > 0, (c[IN_USE], c[ALLOC_FAIL])
        else:
            assert c[IN_USE] == 0 and c[ALLOC_FAIL] == 0
        m.close()
    for k in range(2):
        _same(runs["small"][k], runs["off"][k], f"small pool / off, frame {k}")


@gpu
@pytest.mark.parametrize("n_streams", [1, 8])
def test_window_shift_moves_and_releases_blocks(n_streams, monkeypatch):
    """the planted map 400 m down the x axis: the first frame's pose sits in cube column 2, so the grid
    shifts by one cube (k_shift_cubes) before the search: every cube id moves up by one, the cubes of
    column 20 leave the grid and give their blocks back.  Then the same input again, over the shifted,
    re-filtered map."""
    P = _planted_occ()
    off = (-400.0, 0.0, 0.0)
    gone = ([(500.0 + 3 * i, 0.5 * i, 2.0) for i in range(6)], [(505.0, 3.0 * i, -2.0) for i in range(6)])  # column 20
    state = _state(P, off)
    leaving = _state(P, off, extra=([np.array(p) - off for p in gone[0]], [np.array(p) - off for p in gone[1]]))
    clouds = [P.cloud(0), P.cloud(1)]
    assert sum(len([c for c in leaving[k] if c % 21 == 20]) for k in ("corner", "surf")) >= 2
    assert not [c for k in ("corner", "surf") for c in state[k] if c % 21 == 20]
    shifted = tuple({c + 1: v for c, v in state[k].items()} for k in ("corner", "surf"))
    runs = {}
    for occ in (True, False):
        m = _mapper(monkeypatch, n_streams, occ=occ)
        for s in range(n_streams):
            load_state(m, s, leaving)
        n0 = (len(leaving["corner"]) + len(leaving["surf"])) * n_streams
        assert m.debug_counters()[IN_USE] == (n0 if _builds(n_streams, occ) else 0)
        a = _frame(m, clouds, IDENT_Q, np.array(off))
        for s, res in enumerate(a[0]):
            assert res["optimized"] == 1 and res["center"][0] == 3, res["center"]
            assert m.get_state(s)[0][0] == CEN[0] + 1  # shifted by one cube
            _exact_brute_force(res, shifted, clouds, off)
        now = [(m.cubes(s, 0), m.cubes(s, 1)) for s in range(n_streams)]
        live = sum(len(w) for sw in now for w in sw)
        assert live < n0 + 2 * 27 * n_streams
        c = m.debug_counters()
        assert c[ALLOC_FAIL] == 0 and c[IN_USE] == (live if _builds(n_streams, occ) else 0), (c[IN_USE], live)
        assert not [cb for sw in now for w in sw for cb in w if cb % 21 == 20]  # column 20 was cleared
        b = _frame(m, clouds, IDENT_Q, np.array(off))
        for s in (0, n_streams - 1):
            _ref5_check(m, s, now[s], b[0][s], "after the shift")
        c = m.debug_counters()
        assert c[ALLOC_FAIL] == 0 and c[IN_USE] == (_nonempty(m) if _builds(n_streams, occ) else 0)
        runs[occ] = (a, b)
        m.close()
    for k in range(2):
        _same(runs[True][k], runs[False][k], f"blocks on / off, frame {k}")


@gpu
@pytest.mark.parametrize("n_streams", [1, 8])
def test_compaction_leaves_the_blocks_alone(n_streams, monkeypatch):
    """a small arena compacts mid-sequence (the cubes' content and tables move, the block ids are by
    cube): results identical to a large arena, and to the probe path"""
    P = _planted_occ()
    clouds, state = [P.cloud(0), P.cloud(1)], _state(P)
    small = dict(max_input_points=512, max_submap_points=1024, max_map_points=4096)
    big = dict(max_input_points=512, max_submap_points=1024, max_map_points=65536)
    ms = [_mapper(monkeypatch, n_streams, **small), _mapper(monkeypatch, n_streams, **big),
          _mapper(monkeypatch, n_streams, occ=False, **small)]
    for m in ms:
        for s in range(n_streams):
            load_state(m, s, state)
    frames = 0
    while frames < 60 and ms[0].debug_counters()[COMPACTIONS] < n_streams:
        r = [_frame(m, clouds, IDENT_Q, ZERO_T) for m in ms]
        _same(r[0], r[1], f"small / large arena, frame {frames}")
        _same(r[0], r[2], f"blocks on / off, frame {frames}")
        frames += 1
    assert ms[0].debug_counters()[COMPACTIONS] >= n_streams and ms[1].debug_counters()[COMPACTIONS] == 0
    # one more frame, over the compacted arena
    before = (ms[0].cubes(0, 0), ms[0].cubes(0, 1))
    r = [_frame(m, clouds, IDENT_Q, ZERO_T) for m in ms]
    _same(r[0], r[1], "small / large arena, after the compaction")
    _same(r[0], r[2], "blocks on / off, after the compaction")
    _ref5_check(ms[0], 0, before, r[0][0][0], "after the compaction")
    c = ms[0].debug_counters()
    assert c[ALLOC_FAIL] == 0 and c[IN_USE] == (_nonempty(ms[0]) if _builds(n_streams) else 0)
    for m in ms:
        m.close()


@gpu
@pytest.mark.parametrize("exact", [0, 1])
def test_api_set_content_and_refiltered_cubes(frame, exact, monkeypatch):  # noqa: F811
    """a synthetic frame over content set through the API (k_cube_index builds the blocks), then the
    same input over the cubes the frame re-filtered (k_revox, in PCL's order with exact_voxel_order)"""
    runs = {}
    for occ in (True, False):
        m = _mapper(monkeypatch, 8, occ=occ, exact_voxel_order=exact)
        for s in range(8):
            load_state(m, s, frame["before"])
        clouds = (frame["corner"], frame["surf"])
        a = _frame(m, clouds, frame["q_wodom"], frame["t_wodom"])
        _ref5_check(m, 0, (frame["before"]["corner"], frame["before"]["surf"]), a[0][0], "API-set content")
        before = (m.cubes(7, 0), m.cubes(7, 1))
        b = _frame(m, clouds, frame["q_wodom"], frame["t_wodom"])
        _ref5_check(m, 7, before, b[0][7], "re-filtered content")
        c = m.debug_counters()
        assert c[ALLOC_FAIL] == 0 and c[IN_USE] == (_nonempty(m) if occ else 0)
        runs[occ] = (a, b)
        m.close()
    for k in range(2):
        _same(runs[True][k], runs[False][k], f"blocks on / off, frame {k}")
