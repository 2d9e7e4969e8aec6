"""GPU: what k_od_corr (csrc/odometry.hip) leaves per query, checked directly through
loam_odometry_corr_copy: the 1-NN over the 2 m cell table (od_visit, od_gap2, od_find, the cell lane
loop, ties by index), the second / third point of the ring scans (od_ring_scans, od_merge_lanes) and
the factor records.  tests/test_gpu_odometry.py compares counts, LM iterations and a pose within
1e-6: one wrong neighbour among several hundred Huber-weighted factors passes it.

  A. the accessor's contract;
  B. real frames against tests/odom_corr_np.py (decided queries) and the oracle, records included;
  C. five streams in one handle, a 4100-query stream among them (the query loop's second pass);
  D. planted scenes (tests/odom_corr_scenes.py), exact indices.

References and what decides a query: tests/odom_corr_np.py; that model and oracle agree on all of
this without a device: tests/test_odom_corr_host.py.

Record tolerance (test_odom_corr_host.test_record_tolerance): the oracle's records deviate from
numpy float64 on the same indices by at most 2.220e-16 over all frames of B (0 of 5920 plane triples
thin); 10 x that is below the floor, so the device's b is held to 1e-13.  a is a last-cloud point and
must be bit-equal.
"""
import ctypes

import numpy as np
import pytest

import odom_corr_np as M
import odom_corr_scenes as S
import test_odom_corr_host as H
from loam_amd._core import LoamError, lib, ptr
from loam_amd.odometry import BatchOdometry

pytestmark = pytest.mark.gpu

Z = np.zeros((0, 4), np.float32)


def check_records(what, typ, rec, idx, corner_last, surf_last, sharp, flat):
    """type and records are what the indices say: returns the number of thin plane triples"""
    ns, n = len(sharp), len(sharp) + len(flat)
    assert typ.shape == (n,) and rec.shape == (n, 10) and idx.shape == (n, 3), what
    t_ref, a_ref, b_ref, thin = M.records_from_idx(corner_last, surf_last, ns, idx)
    assert np.array_equal(typ, t_ref), what
    assert np.array_equal(rec[:, 0], typ), what
    assert np.array_equal(rec[:, 1:4], np.concatenate([sharp[:, :3], flat[:, :3]]).astype(np.float64)), what
    assert np.array_equal(rec[:, 4:7], a_ref), what  # a: the last-cloud point, bit for bit
    none = idx[:, 0] < 0
    assert (idx[none] == -1).all() and (idx[:ns, 2] == -1).all(), what
    assert not rec[typ == 0, 4:].any(), what
    dev = np.abs(rec[:, 7:10] - b_ref)[~thin]
    assert dev.size == 0 or dev.max() <= H.REC_TOL, (what, dev.max())
    return int(thin.sum())


# ------------------------------------------------------------------------------ A. contract
def test_accessor_contract():
    frames, priors, recs = H.real_case("VLP-16", True)
    L = lib()
    cpl = BatchOdometry(1, detach_vo_lo=0)
    det = BatchOdometry(1)
    for od in (cpl, det):
        with pytest.raises(LoamError) as e:  # before any solve
            od.corr(0)
        assert e.value.rc == -4
        assert L.loam_odometry_corr_copy(od.h, 1, None, None, None, None, 0) == -1  # no such stream
        c = frames[0]
        od.input(0, c[1], c[2], c[3], c[4])
        od.solve()
        with pytest.raises(LoamError) as e:  # the first frame is not optimised
            od.corr(0)
        assert e.value.rc == -4
    c = frames[1]
    cpl.input(0, c[1], c[2], c[3], c[4])
    cpl.set_prior(0, *priors[1])
    cpl.solve()
    det.input(0, c[1], c[2], c[3], c[4])
    det.solve()
    x0, typ, rec, idx = cpl.corr(0)
    n = len(c[1]) + len(c[3])
    assert len(typ) == n and np.array_equal(x0, np.concatenate(priors[1]))  # coupled: the prior
    # cap too small: the count, nothing written
    t2, r2, i2 = np.full(n, 77, np.int32), np.full((n, 10), 77.0), np.full((n, 3), 77, np.int32)
    assert L.loam_odometry_corr_copy(cpl.h, 0, None, ptr(t2), ptr(r2), ptr(i2), n - 1) == n
    assert (t2 == 77).all() and (r2 == 77.0).all() and (i2 == 77).all()
    assert L.loam_odometry_corr_copy(cpl.h, 0, None, None, None, None, n) == -1  # buffers missing
    # detached: round 1 starts from round 0's result.  A coupled handle given that pose as its prior
    # starts both rounds from it, so its second round must see exactly what the detached one saw
    xd, td, rd, idd = det.corr(0)
    assert not np.array_equal(xd, [0, 0, 0, 1, 0, 0, 0])
    twin = BatchOdometry(1, detach_vo_lo=0)
    twin.input(0, *frames[0][1:])
    twin.solve()
    twin.input(0, c[1], c[2], c[3], c[4])
    twin.set_prior(0, xd[:4], xd[4:])
    twin.solve()
    xt, tt, rt, it = twin.corr(0)
    assert np.array_equal(xt, xd) and np.array_equal(tt, td) and np.array_equal(it, idd)
    assert rt.tobytes() == rd.tobytes()
    # valid until the next solve: a reset forgets it
    det.reset()
    with pytest.raises(LoamError) as e:
        det.corr(0)
    assert e.value.rc == -4
    for od in (cpl, det, twin):
        od.close()


# ---------------------------------------------------------------------------- B. real frames
@pytest.mark.parametrize("cloud,coupled", H.CASES, ids=H.IDS)
def test_real_frames(cloud, coupled):
    frames, priors, recs = H.real_case(cloud, coupled)
    od = BatchOdometry(1, detach_vo_lo=0 if coupled else 1)
    for k, c in enumerate(frames):
        od.input(0, c[1], c[2], c[3], c[4])
        if coupled:
            od.set_prior(0, *priors[k])
        od.solve()
        if k == 0:
            continue
        r = recs[k - 1]
        what = f"{cloud}, frame {k}"
        x0, typ, rec, idx = od.corr(0)
        if coupled:
            assert np.array_equal(x0, r["x0"])
            m_idx, dec = r["idx"], r["decided"]
        else:  # the model at the pose the device used (the oracle's differs in the last digits)
            assert np.abs(x0 - r["x0"]).max() < 1e-6
            m_idx, dec = M.corr_model(r["corner_last"], r["surf_last"], c[1], c[3], x0, exact=False)
        und = 1.0 - dec.mean()
        print(f"{what}: {len(dec)} queries, undecided {und:.4%}")
        assert und <= H.UNDECIDED_CAP
        bad = np.nonzero(dec & (idx != m_idx).any(axis=1))[0]
        assert len(bad) == 0, (what, "model", bad[:10], idx[bad[:10]], m_idx[bad[:10]])
        bad = np.nonzero(dec & (idx != r["oracle_idx"]).any(axis=1))[0]
        assert len(bad) == 0, (what, "oracle", bad[:10], idx[bad[:10]], r["oracle_idx"][bad[:10]])
        n_thin = check_records(what, typ, rec, idx, r["corner_last"], r["surf_last"], c[1], c[3])
        assert n_thin <= H.THIN_CAP * max(1, (typ == 2).sum())
        st = od.stats(0)
        assert (typ == 1).sum() == st.corner_num[1] and (typ == 2).sum() == st.surf_num[1], what
    od.close()


# --------------------------------------------------------------------------------- C. batch
def dyadic_stream(seed=11):
    """4100 queries against last clouds of 40 points, every coordinate a multiple of 1/8 in [0, 8):
    exact in float32, so the model's exact mode applies"""
    rng = np.random.default_rng(seed)

    def pts(n, rings):
        p = np.empty((n, 4), np.float32)
        p[:, :3] = rng.integers(0, 64, (n, 3)) / 8.0
        p[:, 3] = rng.integers(0, rings, n) + 0.25
        return p
    return dict(corner_last=pts(40, 6), surf_last=pts(40, 6), sharp=pts(2000, 1), flat=pts(2100, 1))


def test_batch_streams_equal_their_single_stream_handles():
    fa, pa, _ = H.real_case("64 lines", True)
    fb, pb, _ = H.real_case("VLP-16", True)
    dy = dyadic_stream()
    for c in ("corner_last", "surf_last"):  # no coincident points: an edge through two of them would be NaN
        assert len(np.unique(dy[c][:, :3], axis=0)) == 40
    ident = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    feeds = [  # per stream: (frame 0, frame 1, prior of frame 1)
        (fa[0][1:], fa[1][1:], pa[1]),
        (fb[0][1:], fb[1][1:], pb[1]),
        ((Z, dy["corner_last"], Z, dy["surf_last"]), (dy["sharp"], dy["corner_last"], dy["flat"], dy["surf_last"]), ident),
    ]
    assert len(feeds[2][1][0]) + len(feeds[2][1][2]) == 4100 and len(feeds[0][1][0]) != len(feeds[1][1][0])
    od = BatchOdometry(5, detach_vo_lo=0)
    for s, (f0, _, _) in enumerate(feeds):
        od.input(s, *f0)
    od.solve()
    for s, (_, f1, pr) in enumerate(feeds):
        od.input(s, *f1)
        od.set_prior(s, *pr)
    od.input(4, *fa[0][1:])  # stream 4: its first frame; stream 3: no input at all
    od.solve()
    for s in (3, 4):
        with pytest.raises(LoamError) as e:
            od.corr(s)
        assert e.value.rc == -4, s
    for s, (f0, f1, pr) in enumerate(feeds):
        one = BatchOdometry(1, detach_vo_lo=0)
        one.input(0, *f0)
        one.solve()
        one.input(0, *f1)
        one.set_prior(0, *pr)
        one.solve()
        x1, t1, r1, i1 = one.corr(0)
        xb, tb, rb, ib = od.corr(s)
        assert len(tb) == len(f1[0]) + len(f1[2]) and np.array_equal(xb, x1), s
        assert np.array_equal(tb, t1) and np.array_equal(ib, i1) and rb.tobytes() == r1.tobytes(), s
        one.close()
    # the 4100-query stream against the model: the queries beyond 4096 go through the loop's second pass
    _, tb, rb, ib = od.corr(2)
    m_idx, _ = M.corr_model(dy["corner_last"], dy["surf_last"], dy["sharp"], dy["flat"], np.concatenate(ident), exact=True)
    assert np.array_equal(ib, m_idx), np.nonzero((ib != m_idx).any(axis=1))[0][:10]
    assert (m_idx[4096:, 0] >= 0).any() and (tb > 0).sum() > 1000
    od.close()


# ------------------------------------------------------------------------ D. planted scenes
def device_planted(od, sc):
    od.reset()
    od.input(0, Z, sc["corner_last"], Z, sc["surf_last"])
    od.solve()
    od.input(0, S.fed(sc, 0), sc["corner_last"], S.fed(sc, 1), sc["surf_last"])
    od.set_prior(0, *S.prior(sc))
    od.solve()
    return od.corr(0)


@pytest.mark.parametrize("group", list(S.GROUPS))
def test_planted_scenes(group):
    od = BatchOdometry(1, detach_vo_lo=0)
    for sc in S.GROUPS[group]():
        x0, typ, rec, idx = device_planted(od, sc)
        assert np.array_equal(x0, np.concatenate(S.prior(sc))), sc["name"]
        want = H.model_planted(sc)
        assert np.array_equal(idx, want), (sc["name"], np.nonzero((idx != want).any(axis=1))[0][:10], idx[:8], want[:8])
        H.check_planted(sc, idx, "device")
        check_records(sc["name"], typ, rec, idx, sc["corner_last"], sc["surf_last"], S.fed(sc, 0), S.fed(sc, 1))
        for q, t in sc.get("type", {}).items():
            assert typ[q] == t, sc["name"]
        if sc.get("b_zero"):
            assert typ[0] == 2 and not rec[0, 7:10].any(), sc["name"]
    od.close()


def test_table_overflow_is_reported():
    """16385 distinct 2 m cells in one last cloud: the solve that builds its table says so"""
    od = BatchOdometry(1)
    od.input(0, Z, S.table_overflow_cloud(), Z, Z)
    with pytest.raises(LoamError) as e:
        od.solve()
    assert e.value.rc == -3 and "cell table full" in str(e.value)
    od.close()
