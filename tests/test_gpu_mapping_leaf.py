"""GPU: the mapper at VoxelGrid leaves other than the launch file's 0.4 m / 0.8 m
(mapping_line_resolution / mapping_plane_resolution, include/loam_core.h).

The leaf sets the geometry of most of the mapper's device code: the VoxelGrid keys and their
bounding box, the anchored key box of a cube's merge (W = ceil(50 / leaf) + 3 voxels per axis,
voxel.h vx_merge_fixed_point), which cubes fit the LDS path (density ~ leaf^-3), the hash table
sizes, the shard block size.  Every other test runs 0.4 / 0.8, whose inverses 2.5 and 1.25 are
exact in float; here:
  a. teacher-forced frames over six leaf pairs, each VoxelGrid order against the oracle in that
     order (exact_voxel_order = 1: PCL's; 0: input order), with test_gpu_mapping's assertions;
  b. the same frames as six streams of one handle (the many-stream kernels), both orders;
  c. two voxels of one cube whose anchored keys are equal modulo 2^32 (leaf 0.03: W^3 > 2^32)
     must stay two points;
  d. two sharded ranks against the unsharded handle at leaf 0.3 / 0.7 (shard blocks of 13 and 6
     voxels, not 10 and 5).
The oracle sequences are small (seed 11, 600 azimuths, 8 frames), one per (leaf pair, order),
run when first asked for.  Every case asserts on the oracle's record that it still exercises
what it is here for.
"""
import numpy as np
import pytest

import loam_oracle as O
from helpers import load_state, run_sequence
from loam_amd.mapping import BatchMapper
from test_gpu_mapping import _check_frame, _check_map
from test_gpu_shard import _assert_ranks_match_unsharded, _run_ranks, _sequence_body, _stat_tuple

pytestmark = pytest.mark.gpu

SEED, N_AZ, N_FRAMES = 11, 600, 8
SNAP = (3, 6, 7)
BATCH = (2, 3, 4, 5, 6, 7)
BATCH_LEAF = (0.3, 0.7)
LEAVES = [(0.2, 0.4), (0.3, 0.7), (0.1, 0.1), (0.05, 0.05), (1.6, 3.2), (12.0, 25.0)]
VH_BIG_N = 40000  # voxel_hot.h: the largest cube the exact order filters out of the LDS


def _params(leaf, **kw):
    return dict(mapping_line_resolution=leaf[0], mapping_plane_resolution=leaf[1], **kw)


@pytest.fixture(scope="module")
def oracle_seq():
    """oracle_seq(leaf, order): the oracle sequence with the mapper at leaf = (line, plane) and its
    VoxelGrids in `order` (0 PCL's, 1 input order); run once per (leaf, order)"""
    cache = {}

    def get(leaf, order):
        if (leaf, order) not in cache:
            snap = BATCH if leaf == BATCH_LEAF else SNAP
            cache[leaf, order] = run_sequence(SEED, N_FRAMES, n_az=N_AZ, snapshot_frames=snap, line_res=leaf[0],
                                              plane_res=leaf[1], voxel_order=order)
        return cache[leaf, order]

    return get


def check_preconditions(leaf, seq):
    """what the oracle's record must show for the case at `leaf` to exercise its path"""
    snaps = [seq[f] for f in SNAP]
    opt = [r["stats"].optimized for r in snaps]
    counts = [list(r["stats"].corner_num) + list(r["stats"].surf_num) for r in snaps]
    if leaf == (0.1, 0.1):  # a whole cube past the exact order's LDS path in a real frame
        assert max(len(p) for p in seq[7]["after"]["surf"].values()) > VH_BIG_N
    if leaf == (0.05, 0.05):  # nearly every input point is a voxel of its own
        shrink = [1.0 - r["stats"].surf_stack / len(r["surf"]) for r in snaps]
        shrink += [1.0 - r["stats"].corner_stack / len(r["corner"]) for r in snaps]
        assert min(shrink) < 0.01, shrink
    if leaf == (1.6, 3.2):  # LM rounds without a single factor next to rounds with a few
        assert any(o == 1 and not any(c) for o, c in zip(opt, counts)), (opt, counts)
        assert any(c[0] or c[1] for c in counts), counts
    elif leaf == (12.0, 25.0):  # "map too sparse": no LM, insertion at the predicted pose
        assert opt == [0, 0, 0], opt
        assert all(r["stats"].surf_map <= 50 for r in snaps)
    else:
        assert opt == [1, 1, 1], opt
        assert all(c[0] > 0 and c[2] > 0 for c in counts), counts


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("leaf", LEAVES, ids=lambda l: f"{l[0]}-{l[1]}")
def test_teacher_forced_leaf(oracle_seq, leaf, exact):
    """exact_voxel_order = 1 against the oracle in PCL's order, 0 against the oracle mapper in input
    order: the reference sums every voxel in the device's order, so every integer result is equal"""
    seq = oracle_seq(leaf, 0 if exact else 1)
    check_preconditions(leaf, seq)
    for fi in SNAP:
        rec = seq[fi]
        m = BatchMapper(1, **_params(leaf, exact_voxel_order=exact))
        load_state(m, 0, rec["before"])
        m.input(0, rec["corner"], rec["surf"], rec["q_wodom"], rec["t_wodom"])
        m.solve()
        _check_frame(m, 0, rec)
        _check_map(m, 0, rec["after"])
        m.close()


@pytest.mark.parametrize("exact", [0, 1])
def test_batched_streams_leaf(oracle_seq, exact):
    """six streams of one handle at leaf 0.3 / 0.7, stream s holding the oracle's state before
    frame 2 + s: the many-stream kernels (no per-stream stack split, one lane per 5-NN query)"""
    seq = oracle_seq(BATCH_LEAF, 0 if exact else 1)
    check_preconditions(BATCH_LEAF, seq)
    m = BatchMapper(len(BATCH), **_params(BATCH_LEAF, exact_voxel_order=exact))
    for s, fi in enumerate(BATCH):
        rec = seq[fi]
        load_state(m, s, rec["before"])
        m.input(s, rec["corner"], rec["surf"], rec["q_wodom"], rec["t_wodom"])
    m.solve()
    for s, fi in enumerate(BATCH):
        _check_frame(m, s, seq[fi])
        _check_map(m, s, seq[fi]["after"])
    m.close()


# ---------------------------------------------------------------------------------------
# c. the anchored key box of the merge
# ---------------------------------------------------------------------------------------
A_PT = np.array([-20.0, -20.0, -22.0], np.float32)
CUBE = 10 + 21 * 10 + 21 * 21 * 5  # the cube of corner (-25, -25, -25) with the grid centred
CORNER = np.array([-25.0, -25.0, -25.0], np.float32)
SURF = np.array([[10.0, 5.0, -1.5, 1.0], [-8.0, 12.0, 2.0, 2.0]], np.float32)


def _key_box(leaf):
    """W of vx_merge_fixed_point's anchored key box, in its float arithmetic"""
    inv = np.float32(1.0) / np.float32(leaf)
    return int(np.ceil(np.float32(50.0) * inv)) + 3, inv


def _wrap_offset(W):
    """(dx, dy, dz) voxels inside a W box with dx + dy W + dz W^2 = 2^32, or None"""
    dz, rem = divmod(1 << 32, W * W)
    dy, dx = divmod(rem, W)
    return (dx, dy, dz) if dz < W else None


def _anchored_key(p, W, inv):
    """the voxel of p in the key box of CUBE and its key in 64 bits"""
    minb = np.floor(CORNER * inv).astype(np.int64) - 1
    ijk = (np.floor(p * inv) - minb.astype(np.float32)).astype(np.int64)
    return ijk, int(ijk[0]) + int(ijk[1]) * W + int(ijk[2]) * W * W


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("leaf", [0.03, 0.05])
def test_merge_keeps_voxels_2_32_keys_apart(leaf, exact):
    """frame 1 plants A in an empty cube, frame 2 adds B = A + (dx, dy, dz) voxels into the same
    cube: a fixed-point cube gaining one point, the merge's condition.  At leaf 0.03 the anchored
    keys of A and B are 2^32 apart (W = 1670, W^3 > 2^32): 32-bit keys would average the two into
    one point.  The oracle (PCL: bounding-box keys, 67e6 voxels) keeps both.  Leaf 0.05 (W^3 < 2^32,
    anchored keys apply) is the control with the same two points."""
    W3, inv3 = _key_box(0.03)
    d = _wrap_offset(W3)
    assert (W3, d) == (1670, (1176, 36, 1540))
    b_pt = (A_PT.astype(np.float64) + np.array(d) * 0.03).astype(np.float32)
    W, inv = _key_box(leaf)
    if leaf == 0.03:
        (ia, ka), (ib, kb) = _anchored_key(A_PT, W, inv), _anchored_key(b_pt, W, inv)
        assert all(0 <= v < W for v in list(ia) + list(ib)), (ia, ib)
        assert kb - ka == 1 << 32 and ka != kb
    else:
        assert W ** 3 < 1 << 32 and _wrap_offset(W) is None
    corner = [np.r_[A_PT, 1.0].astype(np.float32)[None], np.r_[b_pt, 2.0].astype(np.float32)[None]]
    ident = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    o = O.LaserMapping(leaf, 0.8)
    m = BatchMapper(1, **_params((leaf, 0.8), exact_voxel_order=exact))
    for f in range(2):
        with O.voxel_order(0 if exact else 1):
            o.input(corner[f], SURF, None, *ident)
            o.solve()
        m.input(0, corner[f], SURF, *ident)
        m.solve()
        assert o.stats().optimized == 0 and m.stats(0).optimized == 0
        q, t = m.pose(0)
        assert np.array_equal(q, ident[0]) and np.array_equal(t, ident[1])
    ref = o.cubes(0)
    assert sorted(ref) == [CUBE] and ref[CUBE].shape == (2, 4)
    assert np.array_equal(ref[CUBE][:, :3], np.stack([A_PT, b_pt]))
    got = m.cubes(0, 0)
    assert sorted(got) == [CUBE]
    assert got[CUBE].shape == (2, 4), got[CUBE]
    assert np.array_equal(got[CUBE], ref[CUBE])
    m.close()


# ---------------------------------------------------------------------------------------
# d. sharding
# ---------------------------------------------------------------------------------------
def _owner_np(p, leaf, bv, nrank):
    """owner rank of point p: the hash of its block of bv voxels per edge"""
    inv = np.float32(1.0) / np.float32(leaf)
    b = [int(np.floor(np.float32(v) * inv)) // bv for v in p]
    h = (b[0] * 73856093 ^ b[1] * 19349663 ^ b[2] * 83492791) & 0xFFFFFFFF
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    h ^= h >> 16
    return h % nrank


def test_two_ranks_match_unsharded_leaf(oracle_seq):
    """test_gpu_shard.test_ranks_match_unsharded at leaf 0.3 / 0.7: the ranks' poses and statistics
    equal the unsharded handle's, the union of their cubes is its map, each rank stores its blocks"""
    from loam_amd.mapping import shard_owner
    leaf = BATCH_LEAF
    # the 4 m shard blocks are 13 and 6 voxels here (10 and 5 at the defaults): the library's owner
    # against the rule (include/loam_core.h) written out with those block sizes
    rng = np.random.default_rng(3)
    for lf, bv in zip(leaf, (13, 6)):
        assert round(4.0 / lf) == bv
        for p in rng.uniform(-60, 60, (64, 3)).astype(np.float32):
            assert shard_owner(p, lf, 2) == _owner_np(p, lf, bv, 2), (p, lf)
    seq = oracle_seq(leaf, 0)
    m = BatchMapper(1, **_params(leaf))
    ref = []
    for rec in seq:
        m.input(0, rec["corner"], rec["surf"], rec["q_wodom"], rec["t_wodom"])
        m.solve()
        ref.append((m.pose(0), _stat_tuple(m.stats(0))))
    ref_maps = [m.cubes(0, 0), m.cubes(0, 1)]
    m.close()
    assert all(st[0] == 1 for _, st in ref[2:])  # the LM (its all-reduced sums) ran
    res = _run_ranks(2, _sequence_body(seq, **_params(leaf)))
    _assert_ranks_match_unsharded(res, ref, ref_maps, 2, leaf)
