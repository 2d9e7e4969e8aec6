"""Time loam_vo_frames_solve (the fused VO frame) beside the staged sequence the older entry
points allow on the same matches (loam_depth_query -> host vo_factors -> loam_vo_solve), at
--pairs frame pairs of n x n descriptors with ~1400 true matches each (the reference's frame).

    python tools/vo_frames_timing.py --pairs 1 --iters 30
    python tools/vo_frames_timing.py --pairs 64 --iters 10

Prints the handle's own HIP-event time of the launch sequence, the host clock around the call
(it ends in a stream synchronise) and the staged steps' host clocks.  Under
`rocprofv3 --kernel-trace --stats -- python tools/vo_frames_timing.py --fused-only ...` the
kernel statistics give the per-kernel split."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vloam-noted_amd"))

from loam_amd import synth, vo  # noqa: E402
from loam_amd.depth import KITTI_CAM_T_VELO, KITTI_P_RECT0, KITTI_RECT0_T_CAM, BatchDepth  # noqa: E402


def frame_pair(rng, cloud, x_true, n, n_land, nb=32):
    """n keypoints per image: n_land projected landmarks (descriptors a few bits apart between
    the images) and random distractors"""
    w, t = x_true[:3], x_true[3:]
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T = KITTI_RECT0_T_CAM.astype(np.float64) @ KITTI_CAM_T_VELO.astype(np.float64)
    X0 = cloud.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    X0 = X0[X0[:, 2] > 4.0]
    X1 = X0 @ R.T + t
    Kc = KITTI_P_RECT0.astype(np.float64)[:, :3]
    u0, u1 = X0 @ Kc.T, X1 @ Kc.T
    u0, u1 = u0[:, :2] / u0[:, 2:3], u1[:, :2] / u1[:, 2:3]
    inside = X1[:, 2] > 1.0
    for u in (u0, u1):
        inside &= (u[:, 0] > 1) & (u[:, 0] < 1240) & (u[:, 1] > 1) & (u[:, 1] < 373)
    pick = rng.choice(np.nonzero(inside)[0], n_land, replace=False)
    land = rng.integers(0, 256, (n_land, nb), dtype=np.uint8)
    seen = land.copy()
    for row in seen:
        for b in rng.integers(0, nb * 8, rng.integers(0, 7)):
            row[b // 8] ^= np.uint8(1 << (b % 8))
    nd = n - n_land
    rand_kp = lambda: np.stack([rng.uniform(0, 1241, nd), rng.uniform(0, 374, nd)], axis=1)  # noqa: E731
    kp0 = np.concatenate([u0[pick], rand_kp()]).astype(np.float32)
    kp1 = np.concatenate([u1[pick], rand_kp()]).astype(np.float32)
    d0 = np.concatenate([land, rng.integers(0, 256, (nd, nb), dtype=np.uint8)])
    d1 = np.concatenate([seen, rng.integers(0, 256, (nd, nb), dtype=np.uint8)])
    order = rng.permutation(n)
    return kp0, d0, kp1[order], d1[order]


def clock(fn, iters):
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def fmt(v):
    return f"median {np.median(v):8.3f} ms  (min {v.min():8.3f}, max {v.max():8.3f}, n {len(v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--matches", type=int, default=1400)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    cloud = synth.frame(21, 5, 2000)[0]
    g = BatchDepth(1)
    g.input(0, cloud)
    g.process()
    x_true = np.array([0.01, -0.02, 0.005, 0.05, -0.02, -0.9])
    pairs = [frame_pair(rng, cloud, x_true, a.n, a.matches) for _ in range(min(a.pairs, 4))]
    vf = vo.VOFrames(g, a.pairs)

    def give():
        for p in range(a.pairs):
            vf.input_descriptors(p, *pairs[p % len(pairs)], 0)

    dev, wall = [], []
    for it in range(a.warmup + a.iters):
        give()
        t0 = time.perf_counter()
        vf.solve()
        w = (time.perf_counter() - t0) * 1e3
        if it >= a.warmup:
            wall.append(w)
            dev.append(vf.result(0)[2].ms)
    x, lm, st = vf.result(0)
    print(f"pairs {a.pairs}, {a.n} x {a.n} descriptors, pair 0: matches {st.n_matches}, gated {st.n_gated}, "
          f"32/22 {st.counter32}/{st.counter22}, LM iterations {lm.iterations}, "
          f"|x - x_true| {np.abs(x - x_true).max():.2e}")
    print(f"fused  loam_vo_frames_solve   device (HIP events) {fmt(np.array(dev))}")
    print(f"fused  loam_vo_frames_solve   host clock          {fmt(np.array(wall))}")
    if a.fused_only:
        return
    # the staged sequence on the same matches: depth download, host records, upload + solve
    ms = [vf.matches(p) for p in range(a.pairs)]
    prevs = [pairs[p % len(pairs)][0][m[:, 0]].astype(np.int32) for p, m in enumerate(ms)]
    currs = [pairs[p % len(pairs)][2][m[:, 1]].astype(np.int32) for p, m in enumerate(ms)]
    keeps = [((pr - cu).astype(np.int64) ** 2).sum(axis=1) <= 100 * 100 for pr, cu in zip(prevs, currs)]
    prevs = [pr[k] for pr, k in zip(prevs, keeps)]
    currs = [cu[k] for cu, k in zip(currs, keeps)]
    cat = np.concatenate(prevs).astype(np.float32)
    cuts = np.cumsum([len(p) for p in prevs])[:-1]
    state = {}

    def s_query():
        state["d"] = np.split(g.query(0, cat), cuts)

    def s_factors():
        state["F"] = [vo.vo_factors(pr, cu, d, KITTI_P_RECT0) for pr, cu, d in zip(prevs, currs, state["d"])]

    def s_solve():
        state["x"] = vo.solve(state["F"])[0]

    def staged():
        s_query()
        s_factors()
        s_solve()

    clock(staged, a.warmup)
    print(f"staged depth_query + vo_factors + vo_solve  host clock {fmt(clock(staged, a.iters))}")
    for name, fn in (("loam_depth_query", s_query), ("host vo_factors", s_factors), ("loam_vo_solve", s_solve)):
        print(f"staged   {name:18s}                 host clock {fmt(clock(fn, a.iters))}")
    same = all(np.array_equal(state["x"][p], vf.result(p)[0]) for p in range(a.pairs))
    print(f"staged x bit-identical to fused: {same} (records may differ by a float32 ulp, see tests)")


if __name__ == "__main__":
    main()
