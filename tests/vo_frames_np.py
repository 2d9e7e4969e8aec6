"""numpy restatements of the VO frame (loam_vo_frames_*): ImageUtil::matchDescriptors
(image_util.cpp:347-438: BFMatcher(NORM_HAMMING), knnMatch k = 2, ratio test), the integer pixel
coordinates and outlier gate of VisualOdometry::solveNlsAll (visual_odometry.cpp:344-368), and
descriptor sets with the hard cases planted."""
import numpy as np

_POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int32)


def hamming_unpackbits(d0, d1, rows=64):
    """(n0, n1) int32: bits set in d0[i] ^ d1[j], counted with np.unpackbits"""
    d0, d1 = np.asarray(d0, np.uint8), np.asarray(d1, np.uint8)
    out = np.zeros((len(d0), len(d1)), dtype=np.int32)
    for a in range(0, len(d0), rows):
        x = d0[a:a + rows, None, :] ^ d1[None, :, :]
        out[a:a + rows] = np.unpackbits(x, axis=2).sum(axis=2, dtype=np.int32)
    return out


def hamming_lut(d0, d1, rows=256):
    """the same distances through a 256-entry popcount table"""
    d0, d1 = np.asarray(d0, np.uint8), np.asarray(d1, np.uint8)
    out = np.zeros((len(d0), len(d1)), dtype=np.int32)
    for a in range(0, len(d0), rows):
        out[a:a + rows] = _POP8[d0[a:a + rows, None, :] ^ d1[None, :, :]].sum(axis=2, dtype=np.int32)
    return out


def ratio_matches(dist, ratio=0.8):
    """(m, 3) int32 (queryIdx, trainIdx, distance) in query order: the best of the two smallest
    of every row where (double)d0 < ratio * (double)d1; nothing with fewer than 2 train rows"""
    n0, n1 = dist.shape
    if n0 == 0 or n1 < 2:
        return np.zeros((0, 3), dtype=np.int32)
    two = np.partition(dist, 1, axis=1)[:, :2]
    best = np.argmin(dist, axis=1)
    keep = two[:, 0].astype(np.float64) < np.float64(ratio) * two[:, 1].astype(np.float64)
    q = np.nonzero(keep)[0]
    return np.stack([q, best[q], two[q, 0]], axis=1).astype(np.int32)


def match(d0, d1, ratio=0.8, hamming=hamming_unpackbits):
    return ratio_matches(hamming(d0, d1), ratio)


def flip(row, bits):
    """a copy of descriptor `row` with the given bit positions flipped"""
    out = np.array(row, dtype=np.uint8)
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def planted(rng, n0, n1, nb):
    """random descriptors (n0, nb), (n1, nb) with, as far as the sizes allow:
    - near-duplicates (k flipped bits) of random train rows,
    - exact duplicate train rows (a tied best: must be rejected),
    - pairs on the ratio boundary 5 d0 == 4 d1 (4/5 and 40/50: rejected) and next to it
      (4/6, 39/50 accepted; 41/50 rejected),
    - the best and the second best at opposite ends of the train set (first tile / last, partial
      tile, so in different slices), both orders, and both in the last tile.
    Returns d0, d1 and {query: expected to be accepted} for the planted queries."""
    d0 = rng.integers(0, 256, (n0, nb), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, nb), dtype=np.uint8)
    nbits = nb * 8
    expect = {}
    queries = iter(rng.permutation(n0))
    lo, hi = 0, n1 - 1  # train slots handed out from both ends, never reused

    def two_trains(q, ka, kb, a_first):
        """trains at distance ka (slot a) and kb (slot b) of query q on disjoint bits; a is taken
        from the front of the train set and b from the back, or the other way round"""
        nonlocal lo, hi
        bits = rng.permutation(nbits)
        a, b = (lo, hi) if a_first else (hi, lo)
        d1[a] = flip(d0[q], bits[:ka])
        d1[b] = flip(d0[q], bits[ka:ka + kb])
        lo, hi = lo + 1, hi - 1

    if n1 >= 64:
        for ka, kb, a_first, ok in ((2, 2, True, False),      # duplicates -> tie
                                    (4, 5, True, False), (40, 50, False, False),
                                    (4, 6, False, True), (39, 50, True, True), (41, 50, False, False),
                                    (3, 30, False, True), (3, 30, True, True)):
            q = next(queries, None)
            if q is None:
                break
            two_trains(q, ka, kb, a_first)
            expect[int(q)] = ok
        q = next(queries, None)
        if q is not None:  # best and second both in the last tile, adjacent rows
            bits = rng.permutation(nbits)
            d1[hi] = flip(d0[q], bits[:5])
            d1[hi - 1] = flip(d0[q], bits[5:45])
            hi -= 2
            expect[int(q)] = True
    if n1 >= 2:
        mid = np.arange(lo, hi + 1)
        for k in (0, 1, 3, 10, 25):
            q = next(queries, None)
            if q is None or len(mid) == 0:
                break
            d0[q] = flip(d1[rng.choice(mid)], rng.permutation(nbits)[:k])
            if n1 >= 64:  # among random rows the runner-up is far away
                expect[int(q)] = True
    return d0, d1, expect


def gate(kp0, kp1, matches, r):
    """integer pixel coordinates (:344-356) of the matched points and the outlier gate (:363-368):
    prev (m, 2) int32, curr (m, 2) int32, keep (m,) bool"""
    prev = np.asarray(kp0, np.float32)[matches[:, 0]].astype(np.int32)
    curr = np.asarray(kp1, np.float32)[matches[:, 1]].astype(np.int32)
    d = (prev - curr).astype(np.int64)
    keep = np.ones(len(prev), bool) if r <= 0 else ~(d[:, 0] ** 2 + d[:, 1] ** 2 > int(r) * int(r))
    return prev, curr, keep


def ulps32(a, b):
    """distance in float32 units in the last place between float32 arrays (same sign assumed
    where it matters; equal values give 0)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)
