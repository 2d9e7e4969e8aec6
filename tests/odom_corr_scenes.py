"""Planted scenes for the odometry's correspondence search (tests/test_odom_corr_host.py on the CPU,
tests/test_gpu_odometry_corr.py on the device).  Every coordinate and every prior translation is
dyadic, so the float32 distances are exact (tests/odom_corr_np.py, exact mode).

A scene is a dict: name, corner_last / surf_last (n, 4) float32 (frame 0's lessSharp / lessFlat),
sel_sharp / sel_flat (n, 4): the queries as they are after TransformToStart, t (3,) the prior's
translation (rotation: identity), expect: {query number in the accessor's order: (closest, ind2,
ind3)} written by hand, and claims: [(text, bool)] that make the scene what it says it is.
fed() gives the queries as they are fed: sel - t.
"""
import numpy as np

CID = 5  # ring of the planted closest point where the scene does not say otherwise


def P(x, y, z, i):
    return [float(x), float(y), float(z), float(i)]


def cloud(rows):
    a = np.array(rows, dtype=np.float64).reshape(-1, 4)
    out = a.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), a), "a planted coordinate is not a float32"
    return out


def d2(p, q):
    e = np.asarray(p, np.float64)[:3] - np.asarray(q, np.float64)[:3]
    return float(e @ e)


def scene(name, corner_last=(), surf_last=(), sel_sharp=(), sel_flat=(), t=(0.0, 0.0, 0.0), expect=None, claims=()):
    return dict(name=name, corner_last=cloud(corner_last), surf_last=cloud(surf_last), sel_sharp=cloud(sel_sharp),
                sel_flat=cloud(sel_flat), t=np.array(t, np.float64), expect=dict(expect or {}), claims=list(claims))


def fed(sc, which):
    """the queries as fed to input(): TransformToStart with the prior brings them back to sel"""
    sel = sc["sel_sharp" if which == 0 else "sel_flat"]
    out = sel.astype(np.float64)
    out[:, :3] -= sc["t"]
    return cloud(out)


def prior(sc):
    return np.array([0.0, 0.0, 0.0, 1.0]), sc["t"].copy()


# od_key / od_hash of csrc/odometry.hip restated, only to show that the crowded-table scene has
# cells that share a home slot (one of each such pair sits in a probed slot whichever went in first)
def cell_of(v):
    return np.clip(np.floor(np.asarray(v, np.float64) * 0.5).astype(np.int64) + 256, 0, 511)


def home_slot(xyz):
    c = cell_of(xyz)
    k = (c[:, 0] | (c[:, 1] << 9) | (c[:, 2] << 18)).astype(np.uint64)
    h = (k * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    return (h & 16383).astype(np.int64)


# ------------------------------------------------------------------------------- D1 cell faces
def d1_cell_faces():
    """clusters 32 m or more apart; each: the query, its nearest across a boundary of the query's
    2 m cell (ring 1), a decoy inside the query's own cell that is farther (ring 1), and a ring-2
    point 1 m beyond the nearest for the edge's second point"""
    last, sel, expect, claims = [], [], {}, []

    def cluster(base, q, near, decoy, what):
        b = np.array(base, np.float64)
        i0 = len(last)
        qq, nn, dd = b + q, b + near, b + decoy
        second = nn + (nn - qq) / np.abs(nn - qq).max() * 1.0
        last.extend([P(*dd, 1.5), P(*nn, 1.25), P(*second, 2.5)])
        expect[len(sel)] = (i0 + 1, i0 + 2, -1)
        sel.append(P(*qq, 0.0))
        claims.append((f"{what}: the nearest is in another cell than the query", not np.array_equal(cell_of(qq), cell_of(nn))))
        claims.append((f"{what}: the decoy shares the query's cell and is farther", np.array_equal(cell_of(qq), cell_of(dd)) and d2(dd, qq) > d2(nn, qq)))
        return qq, nn

    cluster((0, 0, 0), (0.25, 1, 1), (-0.25, 1, 1), (1.25, 1, 1), "face at 0")
    cluster((-32, -32, 0), (0.25, 0.25, 1), (-0.25, -0.25, 1), (1, 1, 1), "edge, negative coordinates")
    cluster((64, -64, -32), (0.25, 0.25, 0.25), (-0.25, -0.25, -0.25), (1.25, 1.25, 1.25), "corner")
    cluster((-2, 32, -2), (1.75, 1.75, 1.75), (2.25, 1.75, 1.75), (0.75, 1.75, 1.75), "face between cells -1 and 0")
    # three cells away along x.  (24.9375 = 399 / 16 and 399 = 7 mod 8: no three dyadic differences
    # have that sum of squares; 24.96875 = (37^2 + 15^2 + 2^2) / 64 is the nearest below 25 with
    # eighths)
    q, n = np.array([1.875, 96.0625, 1.0]), np.array([6.5, 97.9375, 1.25])
    i0 = len(last)
    last.append(P(*n, 1.25))  # (a second point would have to be farther than this and nearer than 25: none)
    expect[len(sel)] = (i0, -1, -1)
    sel.append(P(*q, 0.0))
    claims.append(("three cells along x at d2 = 24.96875", d2(q, n) == 24.96875 and cell_of(n)[0] - cell_of(q)[0] == 3))
    # exactly 25: no correspondence
    q, n = np.array([1.0, -95.0, 1.0]), np.array([4.0, -91.0, 1.0])
    last.extend([P(*n, 1.25), P(4.0, -91.0, 1.5, 2.5)])
    expect[len(sel)] = (-1, -1, -1)
    sel.append(P(*q, 0.0))
    claims.append(("the only point in reach is at exactly d2 = 25", d2(q, n) == 25.0))
    return scene("D1 cell faces", corner_last=last, sel_sharp=sel, t=(0.5, -0.25, 0.125), expect=expect, claims=claims)


# ------------------------------------------------------------------------------------ D2 ties
def d2_ties():
    last, sel, expect, claims = [], [], {}, []
    # two equidistant points: the lower index in the +x cell, which the shell walk meets after the -x cell
    q = np.array([1.0, 1.0, 1.0])
    last.extend([P(2.5, 1, 1, 1.25), P(-0.5, 1, 1, 1.25), P(1, 1, 3, 2.5)])
    expect[0] = (0, 2, -1)
    sel.append(P(*q, 0.0))
    claims.append(("two equidistant points in different cells", d2(last[0], q) == d2(last[1], q) == 2.25 and cell_of(last[0][:3])[0] > cell_of(last[1][:3])[0]))
    # three: the lowest index in the +z cell (visited last)
    b = np.array([64.0, 0.0, 0.0])
    q = b + 1.0
    i0 = len(last)
    last.extend([P(*(q + [0, 0, 1.5]), 1.25), P(*(q + [0, -1.5, 0]), 1.25), P(*(q + [-1.5, 0, 0]), 1.25), P(*(q + [0, 2.5, 0]), 2.5)])
    expect[1] = (i0, i0 + 3, -1)
    sel.append(P(*q, 0.0))
    claims.append(("three equidistant points in three cells", len({d2(last[i0 + k], q) for k in range(3)}) == 1
                   and len({tuple(cell_of(last[i0 + k][:3])) for k in range(3)}) == 3))
    # a duplicate of the nearest under a higher index on ring 8: the scan ID is the lower index's 3
    b = np.array([-64.0, 32.0, 0.0])
    q = b + 1.0
    i0 = len(last)
    last.extend([P(*(q + [0.5, 0, 0]), 3.5), P(*(q + [0, 2, 0]), 4.5), P(*(q + [0.5, 0, 0]), 8.5), P(*(q + [0, 1, 0]), 9.5)])
    expect[2] = (i0, i0 + 1, -1)
    sel.append(P(*q, 0.0))
    claims.append(("the duplicate has the coordinates of the nearest, a higher index and ring 8", last[i0][:3] == last[i0 + 2][:3] and int(last[i0 + 2][3]) == 8))
    claims.append(("from the duplicate's ring the scan would take the ring-9 point", d2(last[i0 + 3], q) < 25))
    return scene("D2 ties", corner_last=last, sel_sharp=sel, expect=expect, claims=claims)


# ------------------------------------------------------- D3 crowded cell and crowded table
def d3_crowded_cell():
    """200 points in the cell [0, 2)^3 along x, 1/128 apart, indices 0..199; the nearest of the two
    queries are the 65th and the 129th: the second and third 64-lane pass over the cell"""
    last = [P(i / 128.0, 1, 1, 1.25) for i in range(200)] + [P(0.5, 1, 1.5, 2.5), P(1.0, 1, 1.5, 2.5)]
    sel = [P(64 / 128.0, 1.0625, 1, 0.0), P(128 / 128.0, 1.0625, 1, 0.0)]
    claims = [("200 points share one cell", len({tuple(c) for c in cell_of(np.array(last)[:200, :3])}) == 1)]
    return scene("D3 crowded cell", corner_last=last, sel_sharp=sel, expect={0: (64, 200, -1), 1: (128, 201, -1)}, claims=claims)


def lattice(nx, ny, nz, limit=None):
    """one point per 2 m cell, at the cell centres, rings alternating 1 / 2"""
    g = np.array([(i, j, k) for k in range(nz) for j in range(ny) for i in range(nx)], np.float64)
    pts = np.concatenate([2.0 * g + 1.0, (1.25 + (g.sum(1) % 2))[:, None]], axis=1)
    return pts[:limit] if limit else pts


def d3_crowded_table():
    """6000 distinct cells (load 0.37 of the 16384 slots): queries at the cells that share their home
    slot with another occupied cell; whichever of the two was inserted first, the other is found by
    probing"""
    pts = lattice(20, 20, 15)
    slot = home_slot(pts[:, :3])
    order = np.argsort(slot, kind="stable")
    same = np.nonzero(np.diff(slot[order]) == 0)[0]
    pick = np.unique(np.concatenate([order[same], order[same + 1]]))[:64]
    sel = [P(*(pts[i, :3] + [0.25, 0.125, 0.0625]), 0.0) for i in pick]
    claims = [("6000 distinct cells", len({tuple(c) for c in cell_of(pts[:, :3])}) == 6000),
              ("cells that share a home slot exist", len(same) >= 16)]
    sc = scene("D3 crowded table", corner_last=pts, sel_sharp=sel, claims=claims)
    sc["closest"] = pick.astype(np.int32)  # the point of the query's own cell: 0.08 m^2 against 2 m to the next
    return sc


def table_overflow_cloud():
    """16385 distinct cells: one more than the table holds"""
    return cloud(lattice(26, 26, 25, limit=16385))


# -------------------------------------------------------------------------- D4 small clouds
def d4_small_clouds():
    out = [scene("D4 empty last clouds", sel_sharp=[P(1, 1, 1, 0)], sel_flat=[P(1, 1, 1, 0)], expect={0: (-1, -1, -1), 1: (-1, -1, -1)}),
           scene("D4 one point", corner_last=[P(1, 1, 2, 3.5)], surf_last=[P(1, 1, 2, 3.5)], sel_sharp=[P(1, 1, 1, 0)], sel_flat=[P(1, 1, 1, 0)],
                 expect={0: (0, -1, -1), 1: (0, -1, -1)})]
    one_ring = [P(1 + 0.5 * i, 1, 2, 3.25 + i / 64.0) for i in range(6)]
    out.append(scene("D4 one ring", corner_last=one_ring, surf_last=one_ring, sel_sharp=[P(2.0625, 1, 1, 0)], sel_flat=[P(2.0625, 1, 1, 0)],
                     expect={0: (2, -1, -1), 1: (2, 3, -1)},
                     claims=[("all points on ring 3", all(int(p[3]) == 3 for p in one_ring))]))
    for nl in (64, 65, 129):  # a line 0.25 m apart, rings 1, 2, 3 in turn: never a break; cl = 0, the middle, nl - 1
        line = [P(0.25 * i, 1, 2, 1.25 + i % 3) for i in range(nl)]
        at = [0, nl // 2, nl - 1]
        q = [P(0.25 * i + 0.0625, 1, 1, 0) for i in at]
        out.append(scene(f"D4 nl = {nl}", corner_last=line, surf_last=line, sel_sharp=q, sel_flat=q))
        out[-1]["closest"] = np.array(at + at, np.int32)
    return out


# ---------------------------------------------------------------------------- D5 ring scans
Q5 = np.array([1.0, 1.0, 1.0])


def ring_scene(name, items, cid_i=CID + 0.5, fill=True, kinds=(0, 1)):
    """a last cloud around the closest point (offset 0, at Q5 + (0, 0, 0.25), intensity cid_i).
    items: (offset from the closest in index order, xyz relative to Q5, intensity).  Gaps between
    the offsets are filled with valid but far points (d2 >= 16, all distances distinct) of ring
    cid + 1 ahead and cid - 1 behind.  The same cloud and query serve corner and surf."""
    cid = int(cid_i)
    lo = min([0] + [o for o, _, _ in items])
    hi = max([0] + [o for o, _, _ in items])
    rows = {0: P(*(Q5 + [0, 0, 0.25]), cid_i)}
    for o, xyz, inten in items:
        assert o not in rows
        rows[o] = P(*(Q5 + np.array(xyz, np.float64)), inten)
    for o in range(lo, hi + 1):
        if o not in rows:
            assert fill
            rows[o] = P(Q5[0] + 4.0 + (o - lo) / 256.0, Q5[1], Q5[2], cid + 1.25 if o > 0 else cid - 0.75)
    last = [rows[o] for o in range(lo, hi + 1)]
    q = [P(*Q5, 0.0)]
    sc = scene(name, corner_last=last if 0 in kinds else (), surf_last=last if 1 in kinds else (),
               sel_sharp=q if 0 in kinds else (), sel_flat=q if 1 in kinds else ())
    sc["cl"] = -lo
    return sc


def d5a_breaks():
    """the breaking point at offset k from the closest; the nearest visited candidate right before
    it (ring cid +- 2), a nearer point of ring cid +- 1 and one of ring cid right after it"""
    out = []
    for sign, word in ((1, "forward"), (-1, "backward")):
        for k in (1, 63, 64, 65, 128):
            items = [(sign * k, (0.5, 0.5, 0), CID + sign * 3 + 0.25),        # the break, d2 0.5
                     (sign * (k + 1), (0, 0.5, 0), CID + sign * 1 + 0.25),    # bait, d2 0.25
                     (sign * (k + 2), (0.5, 0.25, 0), CID + 0.25)]            # bait on ring cid, d2 0.3125
            if k > 1:
                items.append((sign * (k - 1), (1, 0, 0), CID + sign * 2 + 0.25))  # taken: ring cid +- 2, d2 1
            if k > 2:
                items.append((sign * (k - 2), (0, 1.25, 0), CID + 0.25))          # ring cid: surf's minPointInd2
            sc = ring_scene(f"D5a break {word} at offset {k}", items)
            cl = sc["cl"]
            last = sc["corner_last"]
            brk, bait = last[cl + sign * k], last[cl + sign * (k + 1)]
            sc["claims"] += [("the break is of ring cid +- 3", int(brk[3]) == CID + sign * 3),
                             ("a nearer valid point follows the break", int(bait[3]) == CID + sign and d2(bait, Q5) == 0.25),
                             ("the closest is the nearest of all", d2(last[cl], Q5) == 0.0625 and min(d2(p, Q5) for p in last) == 0.0625)]
            if k > 1:
                sc["expect"][0] = (cl, cl + sign * (k - 1), -1)
                sc["claims"].append(("the taken point is of ring cid +- 2 and farther than the bait", int(last[cl + sign * (k - 1)][3]) == CID + sign * 2))
            else:
                sc["expect"][0] = (cl, -1, -1)
            out.append(sc)
    return out


def d5b_continue():
    """corner only: nearer points of ring <= cid ahead and of ring >= cid behind are skipped"""
    out = []
    for near_fwd in (True, False):
        items = [(-2, (0, 2.0 if near_fwd else 1.0, 0), CID - 0.75),   # valid behind
                 (-1, (0.5, 0, 0), CID + 1.25),                        # ring > cid behind: skipped
                 (1, (0, 0.5, 0), CID + 0.25),                         # ring == cid ahead: skipped
                 (2, (0.25, 0.25, 0), CID - 0.75),                     # ring < cid ahead: skipped
                 (3, (1.0 if near_fwd else 2.0, 0, 0), CID + 1.25)]    # valid ahead
        sc = ring_scene("D5b continue, nearer valid " + ("ahead" if near_fwd else "behind"), items, kinds=(0,))
        sc["expect"][0] = (2, 5 if near_fwd else 0, -1)
        sc["claims"].append(("the skipped points are nearer than the taken one", max(d2(sc["corner_last"][j], Q5) for j in (1, 3, 4)) < 1.0))
        out.append(sc)
    return out


def d5c_equal():
    """equal distances: the scan order decides; a candidate at exactly 25 is rejected"""
    out = []
    A, B = (1.5, 0, 0), (0, 1.5, 0)  # both d2 = 2.25
    # (3 and 67 steps away fall to the same lane of a 64-wide walk, one step apart)
    for o1, o2, word in ((2, 5, "one 64-step"), (60, 70, "two 64-steps"), (3, 67, "64 apart")):
        for r_off, kinds, what in ((1, (0, 1), "corner ind2 / surf ind3"), (0, (1,), "surf ind2")):
            sc = ring_scene(f"D5c two ahead, {what}, {word}", [(o1, A, CID + r_off + 0.25), (o2, B, CID + r_off + 0.25)], kinds=kinds)
            sc["tie"] = (o1, o2)
            sc["win"] = (sc["cl"] + o1, 2 if r_off else 1)  # (index, column of idx for surf)
            out.append(sc)
            sc = ring_scene(f"D5c two behind, {what}, {word}", [(-o1, A, CID - r_off + 0.25), (-o2, B, CID - r_off + 0.25)], kinds=kinds)
            sc["tie"] = (-o1, -o2)
            sc["win"] = (sc["cl"] - o1, 2 if r_off else 1)
            out.append(sc)
    for o, word in ((1, "next to the closest"), (70, "70 steps away")):
        sc = ring_scene(f"D5c ahead against behind, {word}", [(o, A, CID + 1.25), (-o, B, CID - 0.75)])
        sc["tie"] = (o, -o)
        sc["win"] = (sc["cl"] + o, 2)
        out.append(sc)
        # surf ind2: ring cid on both sides
        sc = ring_scene(f"D5c ahead against behind on ring cid, {word}", [(o, A, CID + 0.25), (-o, B, CID + 0.25)], kinds=(1,))
        sc["tie"] = (o, -o)
        sc["win"] = (sc["cl"] + o, 1)
        out.append(sc)
    for sc in out:
        cl, last = sc["cl"], sc["surf_last"]
        a, b = (last[cl + o] for o in sc["tie"])
        sc["claims"].append(("the two tie at d2 = 2.25 with different coordinates", d2(a, Q5) == d2(b, Q5) == 2.25 and not np.array_equal(a[:3], b[:3])))
    sc = ring_scene("D5c a candidate at exactly 25", [(1, (3, 4, 0), CID + 1.25), (-1, (4, 0, 3), CID - 0.75)], fill=False)
    sc["expect"] = {0: (1, -1, -1), 1: (1, -1, -1)}
    sc["claims"].append(("both candidates are at exactly 25", d2(sc["corner_last"][0], Q5) == d2(sc["corner_last"][2], Q5) == 25.0))
    out.append(sc)
    return out


def d5d_intensities():
    out = []
    # cid = 3: int(5.96875) = 5 = cid + 2 is taken, int(6.0) = 6 breaks; the bait after it is nearer
    sc = ring_scene("D5d 5.96875 and 6.0 around cid + 2", [(1, (1, 0, 0), 5.96875), (2, (0.5, 0.5, 0), 6.0), (3, (0, 0.5, 0), 4.25)], cid_i=3.5)
    sc["expect"] = {0: (0, 1, -1), 1: (0, -1, 1)}
    out.append(sc)
    # cid = 2: int(-0.03125) = 0 = cid - 2 (truncation; floor would give -1 and break)
    sc = ring_scene("D5d -0.03125 is ring 0", [(-1, (1, 0, 0), -0.03125), (-2, (0, 1.5, 0), 1.25)], cid_i=2.5)
    sc["expect"] = {0: (2, 1, -1), 1: (2, -1, 1)}
    out.append(sc)
    return out


def d5e_surf_classes():
    out = []
    # ahead: ring <= cid -> ind2, ring > cid -> ind3; behind: ring >= cid -> ind2, ring < cid -> ind3;
    # in each class the nearest of the wrong side's ring is nearer than the winner
    items = [(1, (0, 0.5, 0), CID + 1.25),    # ahead, ring > cid: ind3 candidate, d2 0.25  <- ind3
             (2, (1, 0, 0), CID - 0.75),      # ahead, ring < cid: ind2 candidate, d2 1     <- ind2
             (-1, (0.5, 0.5, 0), CID + 1.25),  # behind, ring > cid: ind2 candidate, d2 0.5 -> nearer: ind2
             (-2, (0, 2, 0), CID - 0.75)]     # behind, ring < cid: ind3 candidate, d2 4
    sc = ring_scene("D5e classes by side", items, kinds=(1,))
    sc["expect"] = {0: (2, 1, 3)}
    out.append(sc)
    # minPointInd2 but no minPointInd3: every point on ring cid -> no factor
    sc = ring_scene("D5e ind2 without ind3", [(1, (1, 0, 0), CID + 0.25), (-1, (0, 1.5, 0), CID + 0.75)], kinds=(1,))
    sc["expect"] = {0: (1, 2, -1)}
    sc["type"] = {0: 0}
    out.append(sc)
    # three collinear points: the cross product is 0, the factor is built with b = 0
    sc = ring_scene("D5e collinear triple", [(1, (0, 0, 1.25), CID + 0.25), (2, (0, 0, 2.25), CID + 1.25)], kinds=(1,))
    sc["expect"] = {0: (0, 1, 2)}
    sc["type"] = {0: 2}
    sc["b_zero"] = True
    out.append(sc)
    return out


# ------------------------------------------------------------------------- D6 beyond 512 m
def d6_beyond_512():
    last = [P(600.5, 1, 1, 1.25), P(600.5, 1, 2, 2.5),
            P(1, -700.5, 1, 1.25), P(1, -700.5, 2, 2.5),
            P(513, 33, 1, 1.25), P(513, 33, 2, 2.5), P(508.5, 33, 1, 1.25)]
    sel = [P(600, 1, 1, 0), P(1, -700, 1, 0), P(511, 33, 1, 0)]
    claims = [("the first two pairs lie beyond 512 m, 0.5 m apart", d2(last[0], sel[0]) == 0.25 and d2(last[2], sel[1]) == 0.25),
              ("the query at 511 m has its nearest at 513 m", d2(last[4], sel[2]) == 4.0 and d2(last[6], sel[2]) == 6.25)]
    return scene("D6 beyond 512 m", corner_last=last, surf_last=last, sel_sharp=sel, sel_flat=sel,
                 expect={0: (0, 1, -1), 1: (2, 3, -1), 2: (4, 5, -1), 3: (0, -1, 1), 4: (2, -1, 3), 5: (4, 6, 5)}, claims=claims)


GROUPS = {
    "D1": lambda: [d1_cell_faces()],
    "D2": lambda: [d2_ties()],
    "D3": lambda: [d3_crowded_cell(), d3_crowded_table()],
    "D4": d4_small_clouds,
    "D5a": d5a_breaks,
    "D5bcde": lambda: d5b_continue() + d5c_equal() + d5d_intensities() + d5e_surf_classes(),
    "D6": lambda: [d6_beyond_512()],
}
