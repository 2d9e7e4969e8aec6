"""GPU: every handle releases exactly what it acquired.  loam_debug_live_resources counts the device
buffers, page-locked buffers, streams and events the handles of this process hold; creating a
handle raises the counts by the same amounts every time and destroying it returns all four to where
they were.  The buffers grown on demand (the depth queries, the mapper's publish buffer) are replaced,
never added to, and the results stay those of a fresh handle."""
import ctypes
import gc

import numpy as np
import pytest

from loam_amd import _core, synth, vo
from loam_amd.comm import Comm
from loam_amd.depth import BatchDepth
from loam_amd.mapping import BatchMapper
from loam_amd.odometry import BatchOdometry
from loam_amd.scanreg import ScanRegistration, ScanRegistrationBatch

pytestmark = pytest.mark.gpu

DEVICE, PINNED, STREAM, EVENT = range(4)
# the create functions put no lower bound on the capacities: small, and enough for the growth cases
MAPPER_CAPS = dict(max_input_points=1024, max_submap_points=1024, max_map_points=4096)


def live():
    out = (ctypes.c_int64 * 4)()
    assert _core.lib().loam_debug_live_resources(ctypes.byref(out)) == 0
    return list(out)


def make_depth():
    return BatchDepth(2, max_points=1024)


CASES = {
    "scanreg": lambda: ScanRegistration(max_input_points=1024),
    "scanreg_batch2": lambda: ScanRegistrationBatch(2, max_input_points=1024),
    "odometry2": lambda: BatchOdometry(2, max_input_points=1024),
    "mapper1": lambda: BatchMapper(1, **MAPPER_CAPS),
    "mapper1_exact": lambda: BatchMapper(1, exact_voxel_order=1, **MAPPER_CAPS),
    "mapper5": lambda: BatchMapper(5, **MAPPER_CAPS),
    "mapper5_exact": lambda: BatchMapper(5, exact_voxel_order=1, **MAPPER_CAPS),
    "mapper_sharded": lambda: BatchMapper(1, comm=Comm.single(), **MAPPER_CAPS),
    "depth2": make_depth,
    "vo_frames2": lambda: vo.VOFrames(make_depth(), 2, max_keypoints=64),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_create_destroy_returns_the_counts(case):
    gc.collect()  # handles earlier tests dropped are destroyed now, not between two readings
    held = []
    for _ in range(3):
        before = live()
        h = CASES[case]()
        during = live()
        assert during[DEVICE] > before[DEVICE] and during[STREAM] > before[STREAM]
        held.append([d - b for d, b in zip(during, before)])
        depth, comm = getattr(h, "depth", None), getattr(h, "comm", None)
        h.close()
        if depth is not None:  # the vo_frames case counts its depth handle with it
            depth.close()
        assert live() == before
        if comm is not None:
            comm.close()
    assert held[0] == held[1] == held[2], held


def test_depth_queries_regrow_in_place():
    """8, then 300, then 8 query points on one handle: bit-identical to fresh handles, and after the
    first query the handle holds the same number of buffers throughout"""
    xyz, _ = synth.frame(21, 4, 800)  # the scene of test_gpu_depth.py
    rng = np.random.default_rng(21)
    q = np.stack([rng.uniform(-10, 1252, 300), rng.uniform(-10, 385, 300)], axis=1).astype(np.float32)

    def ready():
        g = BatchDepth(1)
        g.input(0, xyz)
        g.process()
        return g

    g = ready()
    got, counts = [], []
    for n in (8, 300, 8):
        got.append(g.query(0, q[:n]))
        counts.append(live())
    assert counts[0] == counts[1] == counts[2]
    assert np.isfinite(got[1]).any() and (got[1] > 0).any()  # the scene gives depths, not only misses
    for n, res in zip((8, 300, 8), got):
        fresh = ready()
        assert np.array_equal(fresh.query(0, q[:n]), res, equal_nan=True)
        fresh.close()
    g.close()


def cube_points(rng, cube, n):
    """n points inside cube `cube` of a fresh stream (21 x 21 x 11 cubes of 50 m, centre cube (10, 10, 5))"""
    i, j, k = cube % 21, (cube // 21) % 21, cube // 441
    centre = 50.0 * np.array([i - 10, j - 10, k - 5], dtype=np.float32)
    pts = np.zeros((n, 4), dtype=np.float32)
    pts[:, :3] = centre + rng.uniform(-24, 24, (n, 3)).astype(np.float32)
    return pts


def test_map_copy_after_the_map_grew():
    """loam_mapper_map_copy through a publish buffer that has to grow between two calls: the second
    copy is the cubes' content (cube order, corner before surf), bit for bit"""
    rng = np.random.default_rng(7)
    m = BatchMapper(1, **MAPPER_CAPS)
    first = {(0, 2430): 5, (1, 2430): 7}
    for (which, cube), n in first.items():
        m.set_cube(0, which, cube, cube_points(rng, cube, n))
    assert len(m.map_cloud(0)) == 12
    buffers = live()[DEVICE]
    for (which, cube), n in {(0, 200): 300, (1, 2431): 500}.items():
        m.set_cube(0, which, cube, cube_points(rng, cube, n))
    got = m.map_cloud(0)
    assert live()[DEVICE] == buffers  # grown: replaced, not added
    want = np.concatenate([m.cube(0, which, cube) for cube in (200, 2430, 2431) for which in (0, 1)])
    assert len(got) == 812 and np.array_equal(got, want)
    m.close()
