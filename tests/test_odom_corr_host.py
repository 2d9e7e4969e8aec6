"""CPU: the odometry's correspondence search (laser_odometry.cpp:282-485), model against oracle.

tests/odom_corr_np.py restates the search from the reference text; the oracle keeps what its own
search found per round (oracle_odom_corr_idx / _factors / _round_pose).  Here the two meet without a
device, so that tests/test_gpu_odometry_corr.py compares the kernel with references that agree:
  - every planted scene of tests/odom_corr_scenes.py: the scene is what it claims, the model gives
    the indices written into the scene by hand, and the oracle gives the model's;
  - real frames (the oracle's scan registration of synthetic clouds, n_az = 500, 3 frames; 64 lines
    plain, 64 lines column-major with per-laser azimuths, quantised and with boundary points, and
    VLP-16; detached and coupled): decided queries agree on all three indices, at most 2 % of a
    frame's queries are undecided;
  - the record tolerance for the device: the largest deviation of the oracle's factor geometry from
    numpy float64 on the same indices, over all those frames, times 10, at least 1e-13.
"""
import functools

import numpy as np
import pytest

import loam_oracle as O
import odom_corr_np as M
import odom_corr_scenes as S
from loam_amd import synth
from test_gpu_odometry import _relative_priors, features

UNDECIDED_CAP = 0.02
THIN_CAP = 0.01
# the largest |oracle record - numpy float64 on the same indices| over all frames of REAL_CLOUDS,
# as test_record_tolerance measured it, and the tolerance the device records are held to
REC_DEV_MEASURED = 2.3e-16  # measured: 2.220e-16, 0 thin of 5920 plane triples
REC_TOL = max(10.0 * REC_DEV_MEASURED, 1e-13)

REAL_CLOUDS = {
    "64 lines": dict(seed=5, flags=0, n_scans=64),
    "64 lines column-major quantised": dict(seed=7, flags=synth.COLUMN_MAJOR | synth.LASER_AZ | synth.QUANTIZE | synth.BOUNDARY, n_scans=64),
    "VLP-16": dict(seed=6, flags=synth.VLP16, n_scans=16),
}
N_FRAMES = 3


# --------------------------------------------------------------------------- planted scenes
def oracle_planted(sc):
    """frame 0 plants the last clouds, frame 1 carries the queries with the scene's prior"""
    od = O.LaserOdometry()
    z = np.zeros((0, 4), np.float32)
    od.input(z, z, sc["corner_last"], z, sc["surf_last"])
    od.solve()
    od.input(z, S.fed(sc, 0), sc["corner_last"], S.fed(sc, 1), sc["surf_last"])
    od.set_prior(*S.prior(sc))
    od.solve()
    return od


def model_planted(sc):
    x0 = np.concatenate(S.prior(sc))
    return M.corr_model(sc["corner_last"], sc["surf_last"], S.fed(sc, 0), S.fed(sc, 1), x0, exact=True)[0]


def check_planted(sc, idx, what):
    """idx (n, 3) against everything the scene states about its outcome"""
    name = f"{what}: {sc['name']}"
    assert len(idx) == len(sc["sel_sharp"]) + len(sc["sel_flat"]), name
    for q, want in sc["expect"].items():
        assert tuple(int(v) for v in idx[q]) == tuple(want), (name, q, idx[q], want)
    if "closest" in sc:
        assert np.array_equal(idx[:, 0], sc["closest"]), name
    if "win" in sc:
        j, col = sc["win"]
        if len(sc["sel_sharp"]):
            assert idx[0, 1] == j, (name, idx[0])
        assert idx[-1, col] == j, (name, idx[-1])


@pytest.mark.parametrize("group", list(S.GROUPS))
def test_planted_scenes_are_what_they_claim(group):
    n_q = 0
    for sc in S.GROUPS[group]():
        for text, ok in sc["claims"]:
            assert ok, (sc["name"], text)
        idx = model_planted(sc)
        check_planted(sc, idx, "model")
        od = oracle_planted(sc)
        assert np.array_equal(od.round_pose(1), np.concatenate(S.prior(sc)))
        assert np.array_equal(od.corr_idx(1), idx), (sc["name"], od.corr_idx(1), idx)
        n_q += len(idx)
        if "type" in sc or sc.get("b_zero"):  # what becomes of the triple: no factor / a factor with b = 0
            f = od.factors(1)
            want = [t for t in sc["type"].values() if t]
            assert [int(t) for t in f[:, 0]] == want, sc["name"]
            if sc.get("b_zero"):
                assert not f[0, 7:10].any(), sc["name"]
    assert n_q > 0


def test_table_overflow_cloud_has_16385_cells():
    pts = S.table_overflow_cloud()
    assert len({tuple(c) for c in S.cell_of(pts[:, :3])}) == 16385


def test_literal_loops_see_the_break_and_the_strict_less():
    """the model itself on the two rules most easily lost: flipping `<` to `<=` or visiting the
    breaking point changes its answer on the scenes planted for that"""
    sc = next(s for s in S.d5c_equal() if s["name"].startswith("D5c two ahead, corner"))
    idx = model_planted(sc)
    o1, o2 = sc["tie"]
    assert idx[0, 1] == sc["cl"] + o1 != sc["cl"] + o2
    sc = next(s for s in S.d5a_breaks() if s["name"].endswith("forward at offset 64"))
    idx = model_planted(sc)
    last = sc["corner_last"]
    bait = sc["cl"] + 65
    assert idx[0, 1] == sc["cl"] + 63 and S.d2(last[bait], S.Q5) < S.d2(last[idx[0, 1]], S.Q5)


# ------------------------------------------------------------------------------ real frames
@functools.lru_cache(maxsize=None)
def real_case(cloud, coupled):
    """the oracle over N_FRAMES frames of one cloud type; per optimised frame what its second round
    saw and found, and the model's answer at the oracle's round pose"""
    cfg = REAL_CLOUDS[cloud]
    frames, gts = features(cfg["seed"], N_FRAMES, n_az=500, flags=cfg["flags"], with_gt=True, n_scans=cfg["n_scans"])
    priors = _relative_priors(gts) if coupled else None
    od = O.LaserOdometry()
    out = []
    for k, c in enumerate(frames):
        corner_last, surf_last = od.cloud(0), od.cloud(1)
        od.input(*c)
        if coupled:
            od.set_prior(*priors[k])
        od.solve()
        if k == 0:
            continue
        x0 = od.round_pose(1)
        idx, decided = M.corr_model(corner_last, surf_last, c[1], c[3], x0, exact=False)
        for a in (corner_last, surf_last, idx, decided, x0):
            a.setflags(write=False)
        out.append(dict(k=k, corner_last=corner_last, surf_last=surf_last, sharp=c[1], flat=c[3], x0=x0, idx=idx, decided=decided,
                        oracle_idx=od.corr_idx(1), oracle_factors=od.factors(1), corr=list(od.stats()[0])))
    return frames, priors, out


CASES = [(c, m) for c in REAL_CLOUDS for m in (False, True)]
IDS = [f"{c}, {'coupled' if m else 'detached'}" for c, m in CASES]


@pytest.mark.parametrize("cloud,coupled", CASES, ids=IDS)
def test_real_frames_model_and_oracle_agree(cloud, coupled):
    frames, priors, recs = real_case(cloud, coupled)
    assert len(recs) == N_FRAMES - 1
    for r in recs:
        if coupled:
            assert np.array_equal(r["x0"], np.concatenate(priors[r["k"]]))
        dec = r["decided"]
        und = 1.0 - dec.mean()
        n_found = int((r["idx"][:, 0] >= 0).sum())
        print(f"{cloud}, {'coupled' if coupled else 'detached'}, frame {r['k']}: {len(dec)} queries, {n_found} with a 1-NN, undecided {und:.4%}")
        assert len(dec) == len(r["sharp"]) + len(r["flat"]) == len(r["oracle_idx"])
        assert n_found > 0.9 * len(dec)
        assert und <= UNDECIDED_CAP
        bad = np.nonzero(dec & (r["idx"] != r["oracle_idx"]).any(axis=1))[0]
        assert len(bad) == 0, (r["k"], bad[:10], r["idx"][bad[:10]], r["oracle_idx"][bad[:10]])
    if REAL_CLOUDS[cloud]["flags"] & synth.COLUMN_MAJOR:  # the ring ids are not monotone along this last cloud
        assert (np.diff(M.ring_ids(recs[0]["corner_last"])) < 0).sum() > 5


def oracle_records(r):
    """the oracle's compact factor list of a frame spread over its queries, in the device's form:
    type (n,), a (n, 3), b (n, 3) (edge: b = unit(a - point b), from the oracle's two points)"""
    idx, f = r["oracle_idx"], r["oracle_factors"]
    ns = len(r["sharp"])
    has = np.where(np.arange(len(idx)) < ns, (idx[:, 0] >= 0) & (idx[:, 1] >= 0), (idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (idx[:, 2] >= 0))
    assert has.sum() == len(f) and [int(has[:ns].sum()), int(has[ns:].sum())] == r["corr"][2:]
    typ = np.zeros(len(idx), np.int32)
    a = np.zeros((len(idx), 3))
    b = np.zeros((len(idx), 3))
    typ[has] = f[:, 0].astype(np.int32)
    a[has] = f[:, 4:7]
    b[has] = f[:, 7:10]
    edge = typ == 1
    e = a[edge] - b[edge]
    b[edge] = e / np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])[:, None]
    return typ, a, b


def test_record_tolerance():
    """REC_DEV_MEASURED / REC_TOL: the oracle's records against numpy float64 on the oracle's indices"""
    worst, n_thin, n_plane = 0.0, 0, 0
    for cloud, coupled in CASES:
        for r in real_case(cloud, coupled)[2]:
            typ_o, a_o, b_o = oracle_records(r)
            typ, a, b, thin = M.records_from_idx(r["corner_last"], r["surf_last"], len(r["sharp"]), r["oracle_idx"])
            assert np.array_equal(typ, typ_o)
            assert np.array_equal(a, a_o)  # a is a last-cloud point: bit for bit
            n_thin += int(thin.sum())
            n_plane += int((typ == 2).sum())
            assert thin.sum() <= THIN_CAP * max(1, (typ == 2).sum())
            worst = max(worst, float(np.abs(b - b_o)[~thin].max()))
    print(f"oracle records against numpy float64: max |b| deviation {worst:.3e}; {n_thin} thin of {n_plane} plane triples; "
          f"device tolerance max(10 x, 1e-13) = {max(10 * worst, 1e-13):.3e}")
    assert worst <= REC_DEV_MEASURED
