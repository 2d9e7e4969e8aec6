"""The odometry's correspondence search (laser_odometry.cpp:282-485) in plain Python / numpy, written
from the reference text: an independent model for tests/test_odom_corr_host.py and
tests/test_gpu_odometry_corr.py.  Neither the oracle nor the kernel was consulted for it.

Per query (cornerPointsSharp against laserCloudCornerLast, surfPointsFlat against
laserCloudSurfLast, after TransformToStart with s = 1):
  - the 1-NN by brute force, lowest index on ties, accepted when d2 < 25 (:299, :397);
  - the forward loop j = closest + 1 .. n - 1 and the backward loop j = closest - 1 .. 0, literally,
    with their `continue` / `break` tests on int(intensity) and the strict `<` on the running
    minima that carry over from the forward into the backward loop (:309-355, :407-456).

Two modes.
  exact    planted scenes: every coordinate is dyadic and the pose is the identity rotation with a
           dyadic translation, so every float32 difference, product and sum of the distance is exact
           whatever the compiler contracts; the model computes the distances in float32 and in
           float64 and asserts that they agree bit for bit.  Indices must match exactly.
  decided  real frames: distances in float64 from the unrounded transformed query, and a flag per
           query, *decided*: float32 rounding cannot change any comparison that picked the result.
           With delta = 4 ulp of the largest |coordinate| and margin(d2) = 2 sqrt(d2) delta + delta^2
           (tests/test_gpu_corr.py's), these differ by more than the margin: best and runner-up of
           the 1-NN among points with other coordinates; the best 1-NN and 25; winner and runner-up,
           and winner and 25, of the minPointInd2 and of the minPointInd3 search, forward and
           backward candidates combined.  Points with identical coordinates have identical
           distances in every arithmetic: the scan order decides between them.  A query whose 1-NN
           is undecided is undecided as a whole.
"""
import numpy as np
from scipy.spatial.transform import Rotation

THR = 25.0          # DISTANCE_SQ_THRESHOLD (laser_odometry.h:90)
NEARBY_SCAN = 2.5   # laser_odometry.h:90


def margin(d2, delta):
    return 2.0 * np.sqrt(d2) * delta + delta * delta


def ring_ids(cloud):
    """int(intensity) of every point: C++ truncation toward zero"""
    return np.trunc(np.asarray(cloud, np.float32)[:, 3]).astype(np.int64)


def to_start(x0, pts, exact):
    """TransformToStart (:152-173) with s = 1: q_last_curr * p + t_last_curr.  exact: the identity
    rotation and a translation whose sums are float32 numbers; returns float32.  Otherwise float64,
    unrounded."""
    p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    x0 = np.asarray(x0, np.float64)
    if exact:
        assert np.array_equal(x0[:4], [0.0, 0.0, 0.0, 1.0])
        sel = p + x0[4:]
        assert np.array_equal(sel.astype(np.float32).astype(np.float64), sel), "the planted sum is not a float32"
        return sel.astype(np.float32)
    return Rotation.from_quat(x0[:4]).apply(p) + x0[4:]


def _dist(last_xyz, sel, exact):
    """squared distances of one query to every last-cloud point (:319-322), as Python floats"""
    if exact:
        d = last_xyz - sel  # float32
        d32 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        e = last_xyz.astype(np.float64) - sel.astype(np.float64)
        d64 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64), "the planted scene is not exact in float32"
        return d64
    e = last_xyz.astype(np.float64) - sel
    return e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]


def _search(kind, ring, dist):
    """one query: (closestPointInd, minPointInd2, minPointInd3) and, for the decided flags, the
    candidates each running minimum was offered, in scan order.  ring, dist: Python lists."""
    n = len(ring)
    # nearestKSearch(pointSel, 1): the nearest point, the lowest index among equals
    closest, best = -1, float("inf")
    for j in range(n):
        if dist[j] < best:
            best, closest = dist[j], j
    cand2, cand3 = [], []
    if not (closest >= 0 and best < THR):
        return (-1, -1, -1), cand2, cand3
    cid = ring[closest]  # closestPointScanID
    ind2 = ind3 = -1
    min2 = min3 = THR
    if kind == 0:  # :309-355
        for j in range(closest + 1, n):
            if ring[j] <= cid:
                continue
            if ring[j] > cid + NEARBY_SCAN:
                break
            cand2.append(j)
            if dist[j] < min2:
                min2, ind2 = dist[j], j
        for j in range(closest - 1, -1, -1):
            if ring[j] >= cid:
                continue
            if ring[j] < cid - NEARBY_SCAN:
                break
            cand2.append(j)
            if dist[j] < min2:
                min2, ind2 = dist[j], j
    else:  # :407-456
        for j in range(closest + 1, n):
            if ring[j] > cid + NEARBY_SCAN:
                break
            (cand2 if ring[j] <= cid else cand3).append(j)
            if ring[j] <= cid and dist[j] < min2:
                min2, ind2 = dist[j], j
            elif ring[j] > cid and dist[j] < min3:
                min3, ind3 = dist[j], j
        for j in range(closest - 1, -1, -1):
            if ring[j] < cid - NEARBY_SCAN:
                break
            (cand2 if ring[j] >= cid else cand3).append(j)
            if ring[j] >= cid and dist[j] < min2:
                min2, ind2 = dist[j], j
            elif ring[j] < cid and dist[j] < min3:
                min3, ind3 = dist[j], j
    return (closest, ind2, ind3), cand2, cand3


def _decided(cand, win, d, xyz, delta):
    """can float32 rounding change the outcome `win` (-1: none under 25) of a running minimum over
    the candidates `cand`?"""
    if len(cand) == 0:
        return True
    c = np.asarray(cand)
    dc = d[c]
    if win < 0:
        m = float(dc.min())  # every candidate is at least 25 away
        return m - THR > margin(m, delta)
    dw = float(d[win])
    if not abs(dw - THR) > margin(THR, delta):
        return False
    other = c[(xyz[c] != xyz[win]).any(axis=1)]
    if len(other) == 0:
        return True
    r = float(d[other].min())
    return r - dw > margin(r, delta)


def correspond(last, queries, x0, kind, exact):
    """kind 0: corner (sharp against cornerLast), 1: surf (flat against surfLast).  Returns idx (n, 3)
    int32 and decided (n,) bool (all True in exact mode)."""
    last = np.ascontiguousarray(last, np.float32).reshape(-1, 4)
    queries = np.ascontiguousarray(queries, np.float32).reshape(-1, 4)
    nq = len(queries)
    idx = np.full((nq, 3), -1, np.int32)
    decided = np.ones(nq, bool)
    if nq == 0:
        return idx, decided
    sel = to_start(x0, queries, exact)
    xyz = last[:, :3]
    ring = ring_ids(last).tolist()
    if len(last):
        delta = 4.0 * float(np.spacing(np.float32(max(np.abs(xyz).max(), np.abs(sel).max()))))
    for i in range(nq):
        if len(last) == 0:
            continue
        d = _dist(xyz, sel[i], exact)
        res, cand2, cand3 = _search(kind, ring, d.tolist())
        idx[i] = res
        if exact:
            continue
        ok = _decided(np.arange(len(last)), res[0], d, xyz, delta)
        if ok and res[0] >= 0:
            ok = _decided(cand2, res[1], d, xyz, delta) and (kind == 0 or _decided(cand3, res[2], d, xyz, delta))
        decided[i] = ok
    return idx, decided


def corr_model(corner_last, surf_last, sharp, flat, x0, exact):
    """both query sets in the accessor's order (sharp first, then flat): idx (n, 3), decided (n,)"""
    ic, dc = correspond(corner_last, sharp, x0, 0, exact)
    i_s, ds = correspond(surf_last, flat, x0, 1, exact)
    return np.concatenate([ic, i_s]), np.concatenate([dc, ds])


def records_from_idx(corner_last, surf_last, n_sharp, idx):
    """the factor geometry in float64 from the indices: type (n,), a (n, 3), b (n, 3) as the device
    records have them (edge: a = last[closest], b = unit(a - last[ind2]); plane: a = last[closest],
    b = normalised (a - l) x (a - m), 0 when the product is 0), and thin (n,): plane triples whose
    cross product is below 1e-6 of the product of the two edge lengths"""
    n = len(idx)
    typ = np.zeros(n, np.int32)
    a = np.zeros((n, 3))
    b = np.zeros((n, 3))
    thin = np.zeros(n, bool)
    cl = np.asarray(corner_last, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    sl = np.asarray(surf_last, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    for i in range(n):
        c, i2, i3 = (int(v) for v in idx[i])
        if i < n_sharp:
            if c >= 0 and i2 >= 0:
                typ[i] = 1
                a[i] = cl[c]
                e = cl[c] - cl[i2]
                b[i] = e / np.sqrt(e @ e)
        elif c >= 0 and i2 >= 0 and i3 >= 0:
            typ[i] = 2
            a[i] = sl[c]
            u, v = sl[c] - sl[i2], sl[c] - sl[i3]
            w = np.cross(u, v)
            nn = np.sqrt(w @ w)
            b[i] = w / nn if nn > 0 else w
            thin[i] = nn < 1e-6 * np.sqrt(u @ u) * np.sqrt(v @ v)
    return typ, a, b, thin
