"""GPU: what the mapper's correspondence stage produces, checked directly (k_knn<8, true>, k_knn<1>,
k_nn_merge, k_geom of csrc/mapper_corr.h; edge_from_nbrs, plane_from_nbrs, eig3, lsq53 of
csrc/device_math.h).  The other mapper suites compare counts, LM iterations and a pose within
1e-4: a wrong neighbour, a dropped candidate or a flipped line direction passes them.

  a. loam_corr_geometry (the device fits on given neighbour sets) against numpy eigh / lstsq in
     float64 and against the oracle, with the tolerances and knife-edge exclusions of
     tests/test_oracle.py, on random sets and on degenerate ones;
  b. the mapper's 5-NN of every query of a teacher-forced frame (loam_mapper_corr_copy) against
     brute force over the window cubes, for the cell-split kernel (one stream), the one-lane
     kernel (six streams) and the sharded merge (two in-process ranks);
  c. the factor records of that frame against the oracle's factors, one to one;
  d. a planted map whose initial pose is an exact minimiser, for the search's edges: cell and cube
     faces, empty cells, cubes outside the window, the 1 m acceptance, too few points in reach.

A query is *decided* when float32 rounding of the transformed query cannot change which five map
points are nearest, nor whether the 5th lies within 1 m: with delta = 4 ulp of the largest
|coordinate| of the submap, the 5th and 6th squared distances, and the 5th and 1.0, differ by more
than 2 sqrt(d2) delta + delta^2.  (The device rounds each query coordinate once, half an ulp, and
its float32 distance carries a few 2^-24 relative: both far inside delta.)  Only decided queries
are compared; the undecided share is capped at 2 % and checked on the CPU from the oracle's state.
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

import loam_oracle as O
from helpers import load_state, quat_angle, run_sequence
from loam_amd import prims
from loam_amd.mapping import BatchMapper

gpu = pytest.mark.gpu

UNDECIDED_CAP = 0.02


# ------------------------------------------------------------------------------- a. geometry
def _unit(v):
    return v / np.linalg.norm(v)


def _edge_sets():
    """(n, 5, 3) float32 neighbour sets for the line fit and the indices of the degenerate ones"""
    rng = np.random.default_rng(3)
    sets = []
    for far in (False, True):  # as test_edge_pca_matches_eigh; then centres 400 m from the origin
        for _ in range(1000):
            c = 400.0 * _unit(rng.normal(size=3)) if far else rng.uniform(-20, 20, 3)
            d = _unit(rng.normal(size=3))
            spread = rng.uniform(0.02, 0.4)
            sets.append(c + np.outer(rng.uniform(-0.5, 0.5, 5), d) + rng.normal(0, spread, (5, 3)))
    edge = {}
    t = np.array([-0.5, -0.125, 0.0, 0.25, 0.625])
    for name, c, d in (("collinear", (3.0, -7.5, 1.25), (1.0, 2.0, 2.0)), ("collinear axis", (-12.0, 4.0, 0.5), (0.0, 0.0, 1.0)),
                       ("collinear 400 m", (256.0, -256.0, 128.0), (1.0, -1.0, 0.5))):
        edge[name] = len(sets)
        sets.append(np.array(c) + np.outer(t, d))  # exact in float32: dyadic coordinates
    pl = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.75], [-0.25, 0.5]])
    for name, o, u, v in (("coplanar", (2.0, 3.0, -1.5), (1.0, 0.0, 0.5), (0.0, 1.0, 0.25)),
                          ("coplanar 400 m", (-384.0, 96.0, 48.0), (0.5, 0.5, 0.0), (0.0, 0.25, 1.0))):
        edge[name] = len(sets)
        sets.append(np.array(o) + np.outer(pl[:, 0], u) + np.outer(pl[:, 1], v))
    for name, c in (("identical", (1.5, -2.25, 0.75)), ("identical 400 m", (230.5, -230.25, 231.0)), ("identical origin", (0, 0, 0))):
        edge[name] = len(sets)
        sets.append(np.tile(np.array(c, dtype=np.float64), (5, 1)))
    out = np.array(sets, dtype=np.float32)
    for i in edge.values():  # the degenerate sets are exact in float32
        assert np.array_equal(out[i].astype(np.float64), sets[i])
    return out, edge


def _plane_sets():
    """(n, 5, 3) float32 neighbour sets for the plane fit, the indices of the degenerate ones, and
    of those on a plane through the origin (lsq53 rank deficient: no lstsq reference)"""
    rng = np.random.default_rng(4)
    sets = []
    for far in (False, True):  # as test_plane_fit_matches_lstsq; then centres 400 m from the origin
        for _ in range(1000):
            n = _unit(rng.normal(size=3))
            c = 400.0 * _unit(rng.normal(size=3)) if far else rng.uniform(-20, 20, 3)
            u = np.cross(n, rng.normal(size=3))
            v = np.cross(n, u)
            sets.append(c + np.outer(rng.uniform(-1, 1, 5), u) + np.outer(rng.uniform(-1, 1, 5), v)
                        + np.outer(rng.normal(0, rng.choice([0.01, 0.3]), 5), n))
    edge, origin = {}, {}
    pl = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.75], [-0.25, 0.5]])
    for name, o, u, v in (("coplanar", (2.0, 3.0, -1.5), (1.0, 0.0, 0.5), (0.0, 1.0, 0.25)), ("coplanar z", (-6.0, 1.0, 2.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
                          ("coplanar 400 m", (-384.0, 96.0, 48.0), (0.5, 0.5, 0.0), (0.0, 0.25, 1.0))):
        edge[name] = len(sets)
        sets.append(np.array(o) + np.outer(pl[:, 0], u) + np.outer(pl[:, 1], v))
    t = np.array([-0.5, -0.125, 0.0, 0.25, 0.625])
    for name, c, d in (("collinear", (3.0, -7.5, 1.25), (1.0, 2.0, 2.0)), ("collinear 400 m", (256.0, -256.0, 128.0), (1.0, -1.0, 0.5))):
        edge[name] = len(sets)
        sets.append(np.array(c) + np.outer(t, d))
    for name, c in (("identical", (1.5, -2.25, 0.75)), ("identical 400 m", (230.5, -230.25, 231.0))):
        edge[name] = len(sets)
        sets.append(np.tile(np.array(c, dtype=np.float64), (5, 1)))
    # planes through the origin: A n = -1 has no solution in the plane's null direction.  Symmetric
    # about the origin the least-squares solution is 0 (norm 0: n = 0 / 0, d = 1 / 0); otherwise it
    # is whatever the rank-deficient back substitution leaves
    sym = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0]], dtype=np.float64)
    for name, u, v, p2 in (("origin z sym", (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), sym), ("origin tilted sym", (1.0, -1.0, 0.0), (0.5, 0.5, 1.0), sym),
                           ("origin z", (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), pl + 0.125), ("origin tilted", (1.0, -1.0, 0.0), (0.5, 0.5, 1.0), pl + 0.125),
                           ("origin tilted 400 m", (256.0, -256.0, 0.0), (0.5, 0.5, 1.0), pl + 1.0)):
        edge[name] = origin[name] = len(sets)
        sets.append(np.outer(p2[:, 0], u) + np.outer(p2[:, 1], v))
    edge["identical origin"] = origin["identical origin"] = len(sets)
    sets.append(np.zeros((5, 3)))
    out = np.array(sets, dtype=np.float32)
    for i in edge.values():
        assert np.array_equal(out[i].astype(np.float64), sets[i])
    return out, edge, origin


def _nb4(nb):
    p = np.zeros((5, 4), np.float32)
    p[:, :3] = nb
    return p


@gpu
def test_line_fit_matches_eigh_and_oracle():
    """edge_from_nbrs + eig3 on the device: the validity flag, point_a and the unit direction k_geom
    stores, against eigh in float64 on the same float32 inputs (1e-9 on points, 1e-8 on |u.v| - 1,
    test_edge_pca_matches_eigh's) and against the oracle (flag, point_a, sign and norm of b)."""
    sets, edge = _edge_sets()
    ok, a, b = prims.corr_geometry(sets, 0)
    P = sets.astype(np.float64)
    ctr = P.sum(1) / 5.0
    Z = P - ctr[:, None, :]
    w, V = np.linalg.eigh(np.einsum("nki,nkj->nij", Z, Z))
    excluded = np.abs(w[:, 2] - 3 * w[:, 1]) < 1e-9 * w[:, 2]  # knife edge of the line test
    assert excluded.mean() < 0.01 and not excluded[list(edge.values())].any()
    ok_ref = w[:, 2] > 3 * w[:, 1]
    keep = ~excluded
    assert np.array_equal(ok[keep], ok_ref[keep])
    dev_ref = dev_dot = dev_orc = 0.0
    n_ok = 0
    for i in np.nonzero(keep)[0]:
        ok_o, a_o, b_o = O.edge_from_nbrs(_nb4(sets[i]))
        assert ok[i] == ok_o, i
        if not ok[i]:
            assert not a[i].any() and not b[i].any()  # k_geom leaves the record's a, b zero
            continue
        n_ok += 1
        v = V[i][:, 2]
        dev_ref = max(dev_ref, np.abs(a[i] - 0.1 * b[i] - ctr[i]).max())
        dev_dot = max(dev_dot, abs(abs(b[i] @ v) - 1.0))
        u_o = (a_o - b_o) / np.linalg.norm(a_o - b_o)
        dev_orc = max(dev_orc, np.abs(a[i] - a_o).max(), np.abs(b[i] - u_o).max())
    print(f"line fit: {n_ok} valid of {keep.sum()}, excluded {excluded.sum()}; max |a - 0.1 b - centre| {dev_ref:.3e}, "
          f"max ||b.v| - 1| {dev_dot:.3e}; against the oracle max |a|, |b| deviation {dev_orc:.3e}")
    assert n_ok > 200
    assert dev_ref <= 1e-9 and dev_dot < 1e-8
    assert dev_orc <= 1e-9  # same sign, same normalisation as the oracle's (a - b)
    for name in ("collinear", "collinear axis", "collinear 400 m"):
        assert ok[edge[name]], name
    for name in ("identical", "identical 400 m", "identical origin"):  # eigenvalues 0, 0, 0: 0 > 0 fails
        assert not ok[edge[name]], name


@gpu
def test_plane_fit_matches_lstsq_and_oracle():
    """plane_from_nbrs + lsq53 on the device: the flatness flag, unit normal and offset against
    lstsq in float64 (1e-9, test_plane_fit_matches_lstsq's) and against the oracle.  On a plane
    through the origin the system is rank deficient and the norm can be 0: the reference divides
    there too, so the device must give the oracle's values, NaN and inf included."""
    sets, edge, origin = _plane_sets()
    ok, a, b = prims.corr_geometry(sets, 1)
    n = len(sets)
    excluded = np.zeros(n, bool)
    ok_ref = np.zeros(n, bool)
    n_ref = np.zeros((n, 3))
    d_ref = np.zeros(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            A = sets[i].astype(np.float64)
            sol = np.linalg.lstsq(A, -np.ones(5), rcond=None)[0]
            d_ref[i] = 1.0 / np.linalg.norm(sol)
            n_ref[i] = sol * d_ref[i]
            r = np.abs(A @ n_ref[i] + d_ref[i])
            ok_ref[i] = bool(np.all(r <= 0.2))
            excluded[i] = np.min(np.abs(r - 0.2)) < 1e-9  # a point on the flatness limit
    assert excluded.mean() < 0.01 and not excluded[list(edge.values())].any()
    rank_def = np.zeros(n, bool)
    rank_def[list(origin.values())] = True
    # (collinear or identical points leave lstsq's minimum-norm answer and the pivoted QR's apart too)
    for name in ("collinear", "collinear 400 m", "identical", "identical 400 m"):
        rank_def[edge[name]] = True
    dev_ref = dev_orc = 0.0
    n_ok = n_bad = 0
    for i in np.nonzero(~excluded)[0]:
        ok_o, n_o, d_o = O.plane_from_nbrs(_nb4(sets[i]))
        assert ok[i] == ok_o, i
        if rank_def[i]:
            if ok[i]:  # bit for bit what the oracle has, NaN and inf included
                assert np.array_equal(a[i], n_o, equal_nan=True) and np.array_equal(b[i, 0], d_o, equal_nan=True), i
            continue
        assert ok[i] == ok_ref[i], i
        assert b[i, 1] == 0 and b[i, 2] == 0
        if not ok[i]:
            n_bad += 1
            assert not a[i].any() and not b[i].any()
            continue
        n_ok += 1
        dev_ref = max(dev_ref, np.abs(a[i] - n_ref[i]).max(), abs(b[i, 0] - d_ref[i]) / max(1.0, abs(d_ref[i])))
        dev_orc = max(dev_orc, np.abs(a[i] - n_o).max(), abs(b[i, 0] - d_o) / max(1.0, abs(d_o)))
    print(f"plane fit: {n_ok} valid, {n_bad} not flat, excluded {excluded.sum()}; max deviation from lstsq {dev_ref:.3e}, "
          f"from the oracle {dev_orc:.3e}")
    assert n_ok > 200 and n_bad > 200
    assert dev_ref <= 1e-9 and dev_orc <= 1e-9
    for name in ("coplanar", "coplanar z", "coplanar 400 m"):
        assert ok[edge[name]], name
    # all five at the origin: the solution is exactly 0, n = 0 / 0, d = 1 / 0; |NaN| > 0.2 is false, so the
    # fit "passes" and k_geom stores it (as the reference would)
    i = origin["identical origin"]
    assert ok[i] and np.isnan(a[i]).all() and np.isinf(b[i, 0])
    print("planes through the origin (ok, n, d):", {k: (bool(ok[v]), a[v].tolist(), float(b[v, 0])) for k, v in origin.items()})


# --------------------------------------------------------------- the brute-force 5-NN reference
def window_cubes(center):
    """laserCloudValidInd (laser_mapping.cpp:455-472): the 5 x 5 x 3 cubes around the centre cube"""
    ci, cj, ck = (int(c) for c in center)
    return [i + 21 * j + 441 * k for i in range(ci - 2, ci + 3) for j in range(cj - 2, cj + 3) for k in range(ck - 1, ck + 2)
            if 0 <= i < 21 and 0 <= j < 21 and 0 <= k < 11]


def submap(cubes, center):
    """the window cubes' points in window order, (n, 3) float32"""
    parts = [cubes[c][:, :3] for c in window_cubes(center) if c in cubes]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 3), np.float32)


def margin(d2, delta):
    return 2.0 * np.sqrt(d2) * delta + delta * delta


class Ref5:
    """the 6 nearest submap points of every query in float64, and which queries are decided"""

    def __init__(self, sub, po, x0):
        self.sub = sub
        self.q = Rotation.from_quat(x0[:4]).apply(np.asarray(po, np.float64)) + x0[4:]
        self.delta = 4.0 * float(np.spacing(np.float32(np.abs(sub).max()))) if len(sub) else 0.0
        nq = len(self.q)
        self.d2 = np.full((nq, 6), np.inf)
        self.idx = np.full((nq, 6), -1, dtype=np.int64)
        if len(sub) and nq:
            k = min(6, len(sub))
            d, i = cKDTree(sub.astype(np.float64)).query(self.q, k=k)
            d, i = d.reshape(nq, k), i.reshape(nq, k)
            # squared distances recomputed from the points (the tree returns rounded roots)
            diff = sub[i].astype(np.float64) - self.q[:, None, :]
            self.d2[:, :k] = (diff * diff).sum(2)
            self.idx[:, :k] = i
        d5, d6 = self.d2[:, 4], self.d2[:, 5]
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isinf(d6), np.inf, d6 - d5)  # (inf - inf: fewer than 5 points, decided)
            self.decided = (gap > margin(np.where(np.isinf(d6), 0.0, d6), self.delta)) & \
                (np.isinf(d5) | (np.abs(d5 - 1.0) > margin(np.maximum(np.where(np.isinf(d5), 1.0, d5), 1.0), self.delta)))
        self.accept = d5 < 1.0

    def check(self, typ, nbr, what=""):
        """the device's neighbours (nq, 5, 3) float32 and types against the reference"""
        nq = len(self.q)
        assert nbr.shape == (nq, 5, 3) and typ.shape == (nq,)
        none = np.isnan(nbr).any(axis=(1, 2))
        assert np.array_equal(none, np.isnan(nbr).all(axis=(1, 2))), what
        assert not typ[none].any(), what  # no neighbours, no factor
        dec = self.decided
        # NaN neighbours exactly where the reference's 5th is at least 1 m away
        assert np.array_equal(none[dec], ~self.accept[dec]), (what, np.nonzero(dec & (none == self.accept))[0][:10])
        both = dec & self.accept
        want = self.sub[self.idx[both, :5]]

        def rows(p):  # each query's 5 points as bit patterns, sorted lexicographically
            v = np.ascontiguousarray(p, np.float32).view(np.uint32)
            for c in (2, 1, 0):
                o = np.argsort(v[..., c], axis=1, kind="stable")
                v = np.take_along_axis(v, o[..., None], axis=1)
            return v
        got_r, want_r = rows(nbr[both]), rows(want)
        wrong = np.nonzero((got_r != want_r).any(axis=(1, 2)))[0]
        assert len(wrong) == 0, (what, len(wrong), np.nonzero(both)[0][wrong[:10]])
        # nearestKSearch order: ascending wherever float32 rounding cannot swap two neighbours
        have = ~none
        diff = nbr[have].astype(np.float64) - self.q[have][:, None, :]
        dd = (diff * diff).sum(2)
        step = np.diff(dd, axis=1)
        assert np.all(step >= -margin(np.maximum(dd[:, :-1], dd[:, 1:]), self.delta)), what
        return float(1.0 - dec.mean()) if nq else 0.0


# ------------------------------------------------------- b / c. a teacher-forced frame
# the smallest synthetic frame (azimuth steps n_az, frames) whose oracle record has optimized == 1 and,
# in both rounds, at least 200 corner and 500 surf factors: of n_az in steps of 50, 200 gives 394 surf factors,
# and the first frame meets an empty map (test_frame_meets_the_preconditions checks the record)
SEED, N_AZ, N_FRAMES = 11, 250, 2


@pytest.fixture(scope="module")
def frame():
    rec = run_sequence(seed=SEED, n_frames=N_FRAMES, n_az=N_AZ, snapshot_frames=(N_FRAMES - 1,))[-1]
    st = rec["stats"]
    assert st.optimized == 1
    assert min(st.corner_num) >= 200 and min(st.surf_num) >= 500, (list(st.corner_num), list(st.surf_num))
    assert np.array_equal(rec["before"]["cen"], rec["after"]["cen"])  # no recentering: cube ids as loaded
    return rec


def _oracle_refs(rec):
    """the brute-force reference of both maps from the oracle's state alone: its stacks (PCL-order
    VoxelGrid) and the pose its second round started from"""
    x0 = rec["round_pose"][1]
    center = rec["stats"].center
    out = []
    for key, leaf in (("corner", 0.4), ("surf", 0.8)):
        out.append(Ref5(submap(rec["before"][key], center), O.voxel_grid(rec[key], leaf)[:, :3], x0))
    return out


def test_frame_meets_the_preconditions(frame):
    """CPU, before any GPU run: the oracle's record of the frame meets the preconditions (the
    fixture's asserts) and at most 2 % of its queries are undecided"""
    refs = _oracle_refs(frame)
    und = sum(int((~r.decided).sum()) for r in refs)
    nq = sum(len(r.q) for r in refs)
    print(f"oracle state: {nq} queries, {und} undecided ({und / nq:.4%}), delta {refs[0].delta:.3e} / {refs[1].delta:.3e}")
    assert und <= UNDECIDED_CAP * nq
    assert sum(int((r.decided & r.accept).sum()) for r in refs) > 700


def _check_handle(m, stream, rec, what):
    """every query of the last solve against brute force over the loaded window cubes; returns
    (x0, type, records, decided mask)"""
    x0, typ, recs, nbr = m.corr(stream)
    st = m.stats(stream)
    assert st.optimized == 1 and len(typ) == st.corner_stack + st.surf_stack
    assert set(np.unique(typ)) <= {0, 1, 3} and np.array_equal(recs[:, 0], typ.astype(np.float64))
    nc = st.corner_stack
    assert not (typ[:nc] == 3).any() and not (typ[nc:] == 1).any()
    dec = np.zeros(len(typ), bool)
    for (lo, hi), key in (((0, nc), "corner"), ((nc, len(typ)), "surf")):
        ref = Ref5(submap(rec["before"][key], st.center), recs[lo:hi, 1:4], x0)
        ref.check(typ[lo:hi], nbr[lo:hi], f"{what} {key}")
        dec[lo:hi] = ref.decided
    und = float(1.0 - dec.mean())
    print(f"{what}: {len(typ)} queries, undecided {und:.4%}")
    assert und <= UNDECIDED_CAP
    return x0, typ, recs, dec


def _solve(m, streams, rec):
    for s in streams:
        load_state(m, s, rec["before"])
        m.input(s, rec["corner"], rec["surf"], rec["q_wodom"], rec["t_wodom"])
    m.solve()


def _x0_within_bar(x0, rec):
    """the existing teacher-forced bar (1e-4 m / 1e-4 rad), here on the second round's start"""
    xr = rec["round_pose"][1]
    assert np.linalg.norm(x0[4:] - xr[4:]) < 1e-4 and quat_angle(x0[:4], xr[:4]) < 1e-4


def _pair_with_oracle(typ, recs, dec, rec):
    """c. the device records with a factor, in order, against the oracle's second-round factors"""
    F = rec["factors"][1]
    got = recs[typ != 0]
    assert len(got) == len(F)
    assert np.array_equal(got[:, 0], F[:, 0])
    assert np.array_equal(got[:, 1:4].astype(np.float32).view(np.uint32), F[:, 1:4].astype(np.float32).view(np.uint32))
    assert np.array_equal(got[:, 1:4], F[:, 1:4])  # (floats widened: the same doubles)
    d = dec[typ != 0]
    line, plane = d & (F[:, 0] == 1), d & (F[:, 0] == 3)
    assert line.sum() >= 150 and plane.sum() >= 400
    de = F[line, 4:7] - F[line, 7:10]  # (point_a, point_b) -> point + unit direction, as k_geom stores
    u = de / np.linalg.norm(de, axis=1)[:, None]
    dev_a = np.abs(got[line, 4:7] - F[line, 4:7]).max()
    dev_u = np.abs(got[line, 7:10] - u).max()
    dev_dot = np.abs(np.abs((got[line, 7:10] * u).sum(1)) - 1.0).max()
    dev_n = np.abs(got[plane, 4:7] - F[plane, 4:7]).max()
    dev_d = (np.abs(got[plane, 7] - F[plane, 7]) / np.maximum(1.0, np.abs(F[plane, 7]))).max()
    print(f"records against the oracle: {line.sum()} lines |a| {dev_a:.3e} |b| {dev_u:.3e} ||u.v| - 1| {dev_dot:.3e}; "
          f"{plane.sum()} planes |n| {dev_n:.3e} |d| {dev_d:.3e}")
    assert dev_a <= 1e-9 and dev_u <= 1e-9 and dev_dot < 1e-8
    assert dev_n <= 1e-9 and dev_d <= 1e-9
    assert not got[plane, 8:10].any()


@gpu
@pytest.mark.parametrize("exact", [1, 0])
def test_one_stream_5nn(frame, exact):
    """k_knn<8, true> (8 lanes split a query's cells); with exact_voxel_order = 1 the stack is the
    oracle's bit for bit, so the records also pair one to one with the oracle's factors (c)"""
    m = BatchMapper(1, exact_voxel_order=exact)
    _solve(m, [0], frame)
    x0, typ, recs, dec = _check_handle(m, 0, frame, f"one stream, exact_voxel_order {exact}")
    _x0_within_bar(x0, frame)
    if exact:
        _pair_with_oracle(typ, recs, dec, frame)
    m.close()


@gpu
def test_six_streams_5nn(frame):
    """k_knn<1> (one lane per query; handles of more than 4 streams), the same frame in every stream"""
    m = BatchMapper(6)
    _solve(m, range(6), frame)
    first = None
    for s in range(6):
        out = _check_handle(m, s, frame, f"six streams, stream {s}")
        _x0_within_bar(out[0], frame)
        if first is None:
            first = out
        else:  # the streams are independent and hold the same frame
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first[1:3], out[1:3]))
    m.close()


@gpu
def test_two_ranks_5nn(frame):
    """k_nn_merge: each rank searches its own share of the map, the merged five are the exact 5-NN"""
    from test_gpu_shard import _run_ranks

    def body(rank, comm):
        m = BatchMapper(1, comm=comm)
        _solve(m, [0], frame)  # cube_set keeps this rank's blocks
        out = _check_handle(m, 0, frame, f"two ranks, rank {rank}")
        _x0_within_bar(out[0], frame)
        m.close()
        return out

    r0, r1 = _run_ranks(2, body)
    assert np.array_equal(r0[0], r1[0])  # the same start pose, hence the same records, on both ranks
    assert np.array_equal(r0[1], r1[1]) and np.array_equal(r0[2], r1[2], equal_nan=True)


# ------------------------------------------------------------------ d. directed search edges
def _cube_of(v, cen):
    """laser_mapping.cpp:747-756"""
    c = int((v + 25.0) / 50.0) + cen
    return c - 1 if v + 25.0 < 0 else c


CEN = (10, 10, 5)


class Planted:
    """map points and queries in eighths of a metre; a query and the points it may reach share a
    plane z = const (surf) or an axis-parallel line (corner), so the identity pose has zero residuals"""

    def __init__(self):
        self.pts = ([], [])
        self.qs = ([], [])
        self.case = {}

    def add(self, name, which, q, offsets, extra=()):
        """query q; map points q + offsets, and `extra` absolute points"""
        q = np.asarray(q, dtype=np.float64)
        self.case[name] = (which, len(self.qs[which]))
        self.qs[which].append(q)
        for o in offsets:
            self.pts[which].append(q + np.asarray(o, dtype=np.float64))
        for p in extra:
            self.pts[which].append(np.asarray(p, dtype=np.float64))

    def cubes(self, which):
        out = {}
        for p in self.pts[which]:
            assert np.array_equal(p * 8, np.round(p * 8))
            c = [_cube_of(float(p[a]), CEN[a]) for a in range(3)]
            out.setdefault(c[0] + 21 * c[1] + 441 * c[2], []).append([p[0], p[1], p[2], 0.0])
        return {c: np.array(v, np.float32) for c, v in out.items()}

    def cloud(self, which):
        q = np.zeros((len(self.qs[which]), 4), np.float32)
        q[:, :3] = np.array(self.qs[which])
        assert np.array_equal(q[:, :3] * 8, np.round(q[:, :3] * 8))
        return q


def _planted():
    P = Planted()
    e = 0.125
    # five in-plane offsets (not collinear) within 1 m, and a 6th; five on a line, and a 6th
    ring = [(-4 * e, 0, 0), (4 * e, 0, 0), (0, -4 * e, 0), (0, 4 * e, 0), (-2 * e, -2 * e, 0), (6 * e, 5 * e, 0)]

    def along(axis, steps=(-4, 4, -6, 6, -7, 9)):
        return [tuple(s * e if a == axis else 0.0 for a in range(3)) for s in steps]
    # queries on integer coordinates (the floorf cell edge, lx = ly = lz = 0), negative ones included
    P.add("integer negative surf", 1, (-3, -7, -2), ring)
    P.add("integer positive surf", 1, (6, 9, 3), ring)
    P.add("integer negative corner z", 0, (5, -4, -3), along(2))
    P.add("integer negative corner x", 0, (-9, -2, 4), along(0))
    # the query's own 1 m cell is empty: all five neighbours in adjacent cells
    P.add("empty own cell surf", 1, (10.5, 10.5, 4.5), [(-6 * e, 0, 0), (6 * e, 0, 0), (0, -6 * e, 0), (0, 6 * e, 0), (-5 * e, -5 * e, 0), (7 * e, 7 * e, 0)])
    P.add("empty own cell corner", 0, (-20.5, 14.5, 2.5), along(1, (-5, 5, -6, 6, -7, 11)))
    # neighbours on both sides of a cube face (v + 25 a multiple of 50; at a negative multiple the point
    # on the face itself is filed in the cube below, local coordinate 50)
    P.add("cube face x = 25", 1, (25, 3, 6), ring)
    P.add("cube face x = -75", 1, (-75, 5, 6.5), [(0, 0, 0), (-2 * e, 0, 0), (3 * e, 0, 0), (0, -4 * e, 0), (0, 5 * e, 0), (6 * e, 5 * e, 0)])
    P.add("cube face y = -75 on it", 1, (-30, -75, -5.5), [(0, 0, 0), (0, -2 * e, 0), (0, 3 * e, 0), (-4 * e, 0, 0), (5 * e, 0, 0), (6 * e, 5 * e, 0)])
    P.add("cube face z = 25 corner", 0, (12, -12, 25), along(2))
    P.add("cube face y = -75 corner", 0, (33, -75, 1.5), along(1, (0, -4, 4, -6, 6, 9)))
    P.add("cube face z = -25 corner", 0, (-40, 40, -25), along(2, (0, -3, 3, -6, 6, 9)))
    # a populated cube just outside the 5 x 5 x 3 window (x >= 125, z >= 75), closer than the accepted
    # neighbours: not part of the submap (laserCloudValidInd), to be ignored
    P.add("outside window x", 1, (124.5, 0.5, 3.5), [(-4 * e, 0, 0), (-6 * e, 0, 0), (0, -5 * e, 0), (0, 5 * e, 0), (-3 * e, -3 * e, 0)],
          extra=[(125, 0.5, 3.5), (125.125, 0.625, 3.5), (125, 0.25, 3.5)])
    P.add("outside window z corner", 0, (7.5, -30.5, 74.5), along(2, (-2, -3, -5, -6, -7)), extra=[(7.5, -30.5, 75), (7.5, -30.5, 75.25)])
    # the 5th neighbour at squared distance 61 / 64 (accepted) and 65 / 64 (rejected), on a line 49 / 64 and
    # 81 / 64: the closest eighths of a metre allow; the margin is ~1e-4
    near4 = [(-4 * e, 0, 0), (4 * e, 0, 0), (0, -4 * e, 0), (0, 4 * e, 0)]
    P.add("5th just inside 1 m", 1, (40.5, 40.5, 8.5), near4 + [(6 * e, 5 * e, 0), (2, 2, 0)])
    P.add("5th just outside 1 m", 1, (-50.5, 44.5, 8.5), near4 + [(7 * e, 4 * e, 0), (2, 2, 0)])
    P.add("5th just inside 1 m corner", 0, (60.5, -20.5, -8.5), along(0, (-2, 2, -4, 4, 7, 24)))
    P.add("5th just outside 1 m corner", 0, (-60.5, -20.5, -8.5), along(0, (-2, 2, -4, 4, 9, 24)))
    # a map of more than 5 points with fewer than 5 in reach of the query
    P.add("three in reach surf", 1, (-60.5, 60.5, -10.5), ring[:3])
    P.add("none in reach surf", 1, (80.5, -80.5, 20.5), [])
    P.add("four in reach corner", 0, (90.5, 90.5, -30.5), along(0)[:4])
    # filler far from every query: the map stays above the thresholds (> 10 corner, > 50 surf points)
    for i in range(6):
        for j in range(6):
            P.pts[1].append(np.array([-100.0 + 3 * i, -100.0 + 3 * j, -40.0]))
    for i in range(8):
        P.pts[0].append(np.array([100.0, -100.0 + 3 * i, 40.0]))
    return P


def _planted_refs(P, stacks):
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    center = CEN  # the identity pose sits in the grid's centre cube
    return [Ref5(submap(P.cubes(w), center), stacks[w][:, :3], ident) for w in range(2)]


def _planted_expectations(P, refs, stacks):
    """the reference itself shows each case is what its name says"""
    def ref_of(name):
        which, qi = P.case[name]
        row = np.nonzero((stacks[which][:, :3] == P.cloud(which)[qi, :3]).all(1))[0]
        assert len(row) == 1, name
        return refs[which], int(row[0])
    for w in range(2):
        assert refs[w].decided.all()
    for name in P.case:
        r, i = ref_of(name)
        rejected = name.startswith(("5th just outside", "three in", "none in", "four in"))
        assert bool(r.accept[i]) != rejected, name
    r, i = ref_of("5th just inside 1 m")
    assert r.d2[i, 4] == 61 / 64
    r, i = ref_of("5th just outside 1 m")
    assert r.d2[i, 4] == 65 / 64
    for name in ("outside window x", "outside window z corner"):  # the outside points would have been among the five
        which, qi = P.case[name]
        r, i = ref_of(name)
        allp = np.array(P.pts[which])
        d_all = np.sort(((allp - r.q[i]) ** 2).sum(1))
        assert d_all[4] < r.d2[i, 4] < 1.0, name
    for name in ("empty own cell surf", "empty own cell corner"):
        r, i = ref_of(name)
        assert not (np.floor(r.sub[r.idx[i, :5]]) == np.floor(r.q[i])).all(1).any(), name
    for name, axis, face in (("cube face x = 25", 0, 25.0), ("cube face x = -75", 0, -75.0), ("cube face y = -75 on it", 1, -75.0),
                             ("cube face z = 25 corner", 2, 25.0), ("cube face y = -75 corner", 1, -75.0), ("cube face z = -25 corner", 2, -25.0)):
        r, i = ref_of(name)
        v = r.sub[r.idx[i, :5], axis]
        assert (v < face).any() and (v >= face).any(), name


def test_planted_map_is_what_it_claims():
    """CPU: every directed case is decided and is the case its name says; the map is above the
    thresholds; the oracle, from the same state, takes no step in the first round"""
    P = _planted()
    clouds = [P.cloud(0), P.cloud(1)]
    stacks = [O.voxel_grid(clouds[0], 0.4), O.voxel_grid(clouds[1], 0.8)]
    for w in range(2):  # queries more than a leaf apart: the stack VoxelGrid leaves them alone
        assert np.array_equal(np.sort(stacks[w].view(np.uint32), axis=0), np.sort(clouds[w].view(np.uint32), axis=0))
    refs = _planted_refs(P, stacks)
    assert len(refs[0].sub) > 10 and len(refs[1].sub) > 50
    _planted_expectations(P, refs, stacks)
    ref = O.LaserMapping()
    ref.set_state(np.array(CEN, np.int32), [0, 0, 0, 1.0], [0, 0, 0.0])
    for w in range(2):
        for c, pts in P.cubes(w).items():
            ref.set_cube(w, c, pts)
    ref.input(clouds[0], clouds[1], None, [0, 0, 0, 1.0], [0, 0, 0.0])
    ref.solve()
    assert ref.stats().optimized == 1
    assert np.array_equal(ref.round_pose(1), [0, 0, 0, 1.0, 0, 0, 0])


@gpu
@pytest.mark.parametrize("n_streams,ranks", [(1, 1), (6, 1), (1, 2)])
def test_directed_search_edges(n_streams, ranks):
    """the planted map through each search kernel: cell-split (one stream), one lane per query (six
    streams), sharded merge (two ranks)"""
    P = _planted()
    clouds = [P.cloud(0), P.cloud(1)]
    state = dict(cen=np.array(CEN, np.int32), q=np.array([0, 0, 0, 1.0]), t=np.zeros(3), corner=P.cubes(0), surf=P.cubes(1))
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])

    def body(rank, comm):
        m = BatchMapper(n_streams, comm=comm)
        for s in range(n_streams):
            load_state(m, s, state)
            m.input(s, clouds[0], clouds[1], ident[:4], ident[4:])
        m.solve()
        for s in range(n_streams):
            st = m.stats(s)
            assert st.optimized == 1 and tuple(st.center) == CEN
            stacks = [m.stack(s, 0), m.stack(s, 1)]
            for w in range(2):  # the stack VoxelGrid left the queries alone
                assert np.array_equal(np.sort(stacks[w].view(np.uint32), axis=0), np.sort(clouds[w].view(np.uint32), axis=0))
            x0, typ, recs, nbr = m.corr(s)
            # precondition: the initial pose is an exact minimiser, the first round took no step
            assert np.array_equal(x0, ident), x0
            nc = len(stacks[0])
            assert np.array_equal(recs[:nc, 1:4], stacks[0][:, :3]) and np.array_equal(recs[nc:, 1:4], stacks[1][:, :3])
            refs = _planted_refs(P, stacks)
            _planted_expectations(P, refs, stacks)
            assert refs[0].check(typ[:nc], nbr[:nc], "corner") == 0.0
            assert refs[1].check(typ[nc:], nbr[nc:], "surf") == 0.0
            # every accepted query sits on its neighbours' line / plane: a factor with zero residual
            assert np.array_equal(typ[:nc] == 1, refs[0].accept) and np.array_equal(typ[nc:] == 3, refs[1].accept)
        m.close()
        return True

    if ranks == 1:
        body(0, None)
    else:
        from test_gpu_shard import _run_ranks
        assert all(_run_ranks(ranks, body))
