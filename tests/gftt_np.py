"""numpy restatement of OpenCV 4's cv::goodFeaturesToTrack for 8-bit single-channel images without
a mask, gradientSize 3, useHarrisDetector false (the call of ImageUtil::detKeypoints,
image_util.cpp:8-71: 1024 corners, quality 0.03, minDistance 7.5, blockSize 5), which
loam_vo_frames_input_image_pair runs on the device.

The one chosen difference: OpenCV scales inside its float Sobel kernels and adds the float products
of the box in an order its SIMD / IPP dispatch decides; here the three box sums are exact integers
that are converted to float once.  Everything after that is a single float32 operation per step in
calcMinEigenVal's order.  The results differ from an OpenCV build by float noise in the eigenvalue,
visible only at near-ties of the order, at the threshold and at the plateau test."""
import numpy as np

from lk_np import reflect101

F = np.float32


def sobel(img):
    """(dx, dy) int32 of the 3 x 3 Sobel pair, BORDER_REFLECT_101; |d| <= 1020"""
    a = np.asarray(img).astype(np.int32)
    h, w = a.shape
    p = a[reflect101(np.arange(-1, h + 1), h)][:, reflect101(np.arange(-1, w + 1), w)]
    sm = p[:-2, :] + 2 * p[1:-1, :] + p[2:, :]
    dx = sm[:, 2:] - sm[:, :-2]
    sm = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    dy = sm[2:, :] - sm[:-2, :]
    return dx, dy


def box_sum(plane, block_size):
    """the unnormalised block_size^2 box with anchor block_size / 2 (offsets -(b/2) .. b-1-(b/2)),
    BORDER_REFLECT_101 on the plane itself, exact"""
    a = np.asarray(plane).astype(np.int64)
    h, w = a.shape
    lo = block_size // 2
    out = np.zeros((h, w), np.int64)
    ys, xs = np.arange(h), np.arange(w)
    for oy in range(-lo, block_size - lo):
        rows = a[reflect101(ys + oy, h)]
        for ox in range(-lo, block_size - lo):
            out += rows[:, reflect101(xs + ox, w)]
    return out


def cov_sums(img, block_size):
    """(Sxx, Sxy, Syy) int32: 15^2 * 1020^2 < 2^31"""
    dx, dy = sobel(img)
    dx, dy = dx.astype(np.int64), dy.astype(np.int64)
    return tuple(box_sum(p, block_size).astype(np.int32) for p in (dx * dx, dx * dy, dy * dy))


def eig_scale(block_size):
    scale = 1.0 / (4 * block_size * 255)
    return F(scale * scale)


def min_eigen(img, block_size=5):
    """cornerMinEigenVal: float32 plane"""
    sxx, sxy, syy = cov_sums(img, block_size)
    k = eig_scale(block_size)
    a = (sxx.astype(F) * k) * F(0.5)
    b = sxy.astype(F) * k
    c = (syy.astype(F) * k) * F(0.5)
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def threshold(eig, quality_level):
    """(float)((double)max * quality_level)"""
    return F(float(eig.max()) * float(quality_level))


def candidates(eig, quality_level):
    """(values float32, linear indices int64) in the selection order: value descending, equal
    values by linear index descending (greaterThanPtr compares the pointers on a tie)"""
    h, w = eig.shape
    t = np.where(eig > threshold(eig, quality_level), eig, F(0))
    p = np.full((h + 2, w + 2), -np.inf, F)
    p[1:-1, 1:-1] = t
    dil = p[1:-1, 1:-1].copy()
    for oy in range(3):
        for ox in range(3):
            dil = np.maximum(dil, p[oy:oy + h, ox:ox + w])
    ok = (t != 0) & (t == dil)
    ok[0, :] = ok[-1, :] = False
    ok[:, 0] = ok[:, -1] = False
    idx = np.flatnonzero(ok)
    val = t.ravel()[idx]
    order = np.lexsort((-idx, -val.astype(np.float64)))
    return val[order], idx[order]


def select(idx, w, max_corners, min_distance):
    """the sequential greedy over candidates in order: positions (into idx) of the kept ones"""
    xs, ys = idx % w, idx // w
    if not min_distance >= 1:
        return np.arange(min(len(idx), max_corners))
    d2 = float(min_distance) * float(min_distance)
    kept = []
    kx, ky = np.zeros(max_corners, np.int64), np.zeros(max_corners, np.int64)
    for i in range(len(idx)):
        n = len(kept)
        if n == max_corners:
            break
        dx, dy = kx[:n] - xs[i], ky[:n] - ys[i]
        if n and ((dx * dx + dy * dy).astype(np.float64) < d2).any():
            continue
        kx[n], ky[n] = xs[i], ys[i]
        kept.append(i)
    return np.array(kept, np.int64)


def cv_round(v):
    """cvRound: half to even"""
    return int(np.rint(v))


def select_grid(idx, w, h, max_corners, min_distance):
    """the same selection the way OpenCV runs it: a grid of cells cvRound(min_distance) wide, the
    3 x 3 cells around the candidate searched"""
    xs, ys = idx % w, idx // w
    if not min_distance >= 1:
        return np.arange(min(len(idx), max_corners))
    cell = cv_round(min_distance)
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    grid = [[] for _ in range(gw * gh)]
    d2 = float(min_distance) * float(min_distance)
    kept = []
    for i in range(len(idx)):
        if len(kept) == max_corners:
            break
        x, y = int(xs[i]), int(ys[i])
        cx, cy = x // cell, y // cell
        good = True
        for yy in range(max(0, cy - 1), min(gh - 1, cy + 1) + 1):
            for xx in range(max(0, cx - 1), min(gw - 1, cx + 1) + 1):
                for (px, py) in grid[yy * gw + xx]:
                    if float((x - px) * (x - px) + (y - py) * (y - py)) < d2:
                        good = False
        if good:
            grid[cy * gw + cx].append((x, y))
            kept.append(i)
    return np.array(kept, np.int64)


def tie_image(w=64, h=48, seed=6):
    """mirror-symmetric about the vertical axis between the two middle columns: the eigenvalue
    plane is symmetric too (dx changes sign, dx^2, (dx dy)^2 and dy^2 do not; an odd box is
    symmetric), so the candidates come in pairs of equal value"""
    import lk_np
    a = lk_np.Scene(seed, flat=(200.0, 200.0, 201.0, 201.0)).render(w // 2, h)
    return np.ascontiguousarray(np.hstack([a, a[:, ::-1]]))


def plateau_image(w=64, h=48):
    """mirror-symmetric, with a bright bar two pixels wide on the axis: the corner at its end is
    two adjacent pixels of equal eigenvalue, both candidates"""
    img = np.full((h, w), 40, np.uint8)
    img[10:30, w // 2 - 1:w // 2 + 1] = 220
    img[30:40, 20:w - 20] = 140
    n = np.random.default_rng(3).integers(0, 6, (h, w // 2), dtype=np.uint8)
    return img + np.hstack([n, n[:, ::-1]])


def adjacent_ties(info, w):
    """candidates that share their value with the next one in the order and touch it"""
    v, i = info["val"], info["idx"]
    return int(((v[1:] == v[:-1]) & (np.abs(i[1:] - i[:-1]) == 1)).sum())


def good_features_to_track(img, max_corners=1024, quality_level=0.03, min_distance=7.5, block_size=5, info=None):
    """(n, 2) float32 corners (x, y) in selection order.  info (a dict) gets the eigenvalue plane
    ("eig"), the ordered candidates ("val", "idx"), the positions of the kept ones ("kept") and the
    number of candidates that share their value with the next one ("ties")."""
    img = np.asarray(img)
    h, w = img.shape
    eig = min_eigen(img, block_size)
    val, idx = candidates(eig, quality_level)
    kept = select(idx, w, max_corners, min_distance)
    if info is not None:
        info.update(eig=eig, val=val, idx=idx, kept=kept, ties=int((val[1:] == val[:-1]).sum()))
    sel = idx[kept]
    return np.stack([sel % w, sel // w], axis=1).astype(np.float32).reshape(-1, 2)
