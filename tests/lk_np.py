"""numpy restatement of OpenCV 4.2's cv::calcOpticalFlowPyrLK / buildOpticalFlowPyramid for 8-bit
single-channel images with flags 0 (the call of ImageUtil::calculateOpticalFlow,
image_util.cpp:503-570), which loam_vo_frames_input_images runs on the device, and a synthetic
scene that can be rendered under a known motion.

The sums over the window are exact integers (OpenCV adds floats in an order its SIMD width
decides); every float32 operation is a single numpy float32 operation in OpenCV's order.  The
model works on whole precomputed derivative planes with padded borders; the device forms the
derivatives per window from a patch: the two share the definition, not the code path."""
import numpy as np

F = np.float32
W_BITS = 14
INT_MIN = -2 ** 31


def reflect101(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101) for any i (arrays too)"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


_K5 = np.array([1, 4, 6, 4, 1], dtype=np.int64)


def pyr_down(img):
    """cv::pyrDown on CV_8U: [1 4 6 4 1]^2 on the even samples, REFLECT_101, (sum + 128) >> 8"""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    xs = reflect101(2 * np.arange((w + 1) // 2)[:, None] + np.arange(-2, 3)[None, :], w)
    ys = reflect101(2 * np.arange((h + 1) // 2)[:, None] + np.arange(-2, 3)[None, :], h)
    rows = (a[:, xs] * _K5).sum(axis=2)
    out = (rows[ys, :] * _K5[None, :, None]).sum(axis=1)
    return ((out + 128) >> 8).astype(np.uint8)


def scharr(img):
    """(dx, dy) int16 of calcSharrDeriv: the 3-10-3 Scharr pair, REFLECT_101 at the edge"""
    a = np.asarray(img).astype(np.int32)
    h, w = a.shape
    p = a[reflect101(np.arange(-1, h + 1), h)][:, reflect101(np.arange(-1, w + 1), w)]
    t0 = 3 * (p[:-2, :] + p[2:, :]) + 10 * p[1:-1, :]
    dx = t0[:, 2:] - t0[:, :-2]
    t1 = p[2:, :] - p[:-2, :]
    dy = 3 * (t1[:, :-2] + t1[:, 2:]) + 10 * t1[:, 1:-1]
    return dx.astype(np.int16), dy.astype(np.int16)


def build_pyramid(img, win=15, max_level=2):
    """buildOpticalFlowPyramid: stops before a level whose width or height is <= win"""
    levels = [np.ascontiguousarray(img, dtype=np.uint8)]
    while len(levels) <= max_level:
        h, w = levels[-1].shape
        if (w + 1) // 2 <= win or (h + 1) // 2 <= win:
            break
        levels.append(pyr_down(levels[-1]))
    return levels


def _ifloor(v):
    """cvFloor; what no int holds becomes INT_MIN (cvtss2si) and fails every bounds check"""
    if not (v > F(-1.0e9) and v < F(1.0e9)):
        return INT_MIN
    return int(np.floor(v))


def _weights(px, py, ix, iy):
    a, b = px - F(ix), py - F(iy)
    one, s = F(1), F(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _scaled(s):
    return F(int(s)) * F(2.0 ** -20)


class _Level:
    def __init__(self, img, win, with_deriv):
        self.h, self.w = img.shape
        self.pad = pad = win + 2
        ys, xs = reflect101(np.arange(-pad, self.h + pad), self.h), reflect101(np.arange(-pad, self.w + pad), self.w)
        self.img = img.astype(np.int64)[ys][:, xs]
        if with_deriv:
            dx, dy = scharr(img)
            self.dx, self.dy = np.pad(dx.astype(np.int64), pad), np.pad(dy.astype(np.int64), pad)

    def bilinear(self, plane, ix, iy, win, wts, shift):
        y0, x0 = iy + self.pad, ix + self.pad
        a = plane[y0:y0 + win + 1, x0:x0 + win + 1]
        v = a[:-1, :-1] * wts[0] + a[:-1, 1:] * wts[1] + a[1:, :-1] * wts[2] + a[1:, 1:] * wts[3]
        return (v + (1 << (shift - 1))) >> shift

    def outside(self, ix, iy, win):
        return ix < -win or ix >= self.w or iy < -win or iy >= self.h


def track(prev_img, curr_img, pts, win=15, max_level=2, max_count=10, epsilon=0.03, min_eig=1e-4, info=None):
    """(next_xy (n, 2) float32, status (n,) uint8, err (n,) float32).  err is 0 where OpenCV leaves
    it unset.  info (a dict) gets, per point, whether some level ran all max_count iterations
    ("cap") and whether one stopped by the oscillation rule ("osc")."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    n = len(pts)
    max_count = min(max(int(max_count), 0), 100)
    eps = min(max(float(epsilon), 0.0), 10.0)
    eps2 = eps * eps
    P = [_Level(a, win, True) for a in build_pyramid(prev_img, win, max_level)]
    C = [_Level(a, win, False) for a in build_pyramid(curr_img, win, max_level)]
    half = F(win - 1) * F(0.5)
    out, status, err = np.zeros((n, 2), np.float32), np.ones(n, np.uint8), np.zeros(n, np.float32)
    cap, osc = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            nx = ny = F(0)
            for lv in range(len(P) - 1, -1, -1):
                I, J = P[lv], C[lv]
                scale = F(1.0 / (1 << lv))
                px, py = pts[i, 0] * scale, pts[i, 1] * scale
                if lv == len(P) - 1:
                    nx, ny = px, py
                else:
                    nx, ny = nx * F(2), ny * F(2)
                px, py = px - half, py - half
                ipx, ipy = _ifloor(px), _ifloor(py)
                if I.outside(ipx, ipy, win):
                    if lv == 0:
                        status[i], err[i] = 0, 0
                    continue
                wts = _weights(px, py, ipx, ipy)
                Iv = I.bilinear(I.img, ipx, ipy, win, wts, W_BITS - 5)
                Ix = I.bilinear(I.dx, ipx, ipy, win, wts, W_BITS)
                Iy = I.bilinear(I.dy, ipx, ipy, win, wts, W_BITS)
                A11, A12, A22 = _scaled((Ix * Ix).sum()), _scaled((Ix * Iy).sum()), _scaled((Iy * Iy).sum())
                D = A11 * A22 - A12 * A12
                me = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4) * A12 * A12)) / F(2 * win * win)
                if float(me) < min_eig or D < np.finfo(np.float32).eps:
                    if lv == 0:
                        status[i] = 0
                    continue
                D = F(1) / D
                qx, qy = nx - half, ny - half
                pdx = pdy = F(0)
                ended = False
                for j in range(max_count):
                    iqx, iqy = _ifloor(qx), _ifloor(qy)
                    if J.outside(iqx, iqy, win):
                        if lv == 0:
                            status[i] = 0
                        ended = True
                        break
                    diff = J.bilinear(J.img, iqx, iqy, win, _weights(qx, qy, iqx, iqy), W_BITS - 5) - Iv
                    b1, b2 = _scaled((diff * Ix).sum()), _scaled((diff * Iy).sum())
                    dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
                    qx, qy = qx + dx, qy + dy
                    nx, ny = qx + half, qy + half
                    if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                        ended = True
                        break
                    if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                        nx, ny = nx - dx * F(0.5), ny - dy * F(0.5)
                        osc[i] = ended = True
                        break
                    pdx, pdy = dx, dy
                cap[i] |= not ended and max_count > 0
                if lv == 0 and status[i]:
                    ex, ey = nx - half, ny - half
                    iex, iey = _ifloor(ex), _ifloor(ey)
                    if J.outside(iex, iey, win):
                        status[i] = 0
                    else:
                        diff = J.bilinear(J.img, iex, iey, win, _weights(ex, ey, iex, iey), W_BITS - 5) - Iv
                        err[i] = F(int(np.abs(diff).sum())) / F(32 * win * win)
            out[i] = nx, ny
    if info is not None:
        info["cap"], info["osc"] = cap, osc
    return out, status, err


class Scene:
    """A smooth random texture that can be evaluated at real coordinates: a sum of sinusoids of
    random direction, wavelength (7 .. 70 px) and phase plus low-passed noise (random values on a
    coarse grid, joined by a C1 smoothstep), and one flat rectangle `flat` = (x0, y0, x1, y1).
    render() quantises to uint8."""

    def __init__(self, seed, flat=(30.0, 20.0, 62.0, 52.0), waves=28, cell=9.0, contrast=38.0):
        rng = np.random.default_rng(seed)
        lam = rng.uniform(7.0, 70.0, waves)
        ang = rng.uniform(0, 2 * np.pi, waves)
        self.k = (2 * np.pi / lam)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        self.phase = rng.uniform(0, 2 * np.pi, waves)
        self.amp = rng.uniform(0.4, 1.0, waves) * contrast / np.sqrt(waves / 2)
        self.cell = cell
        self.grid = rng.normal(0, 0.6 * contrast, (256, 256))
        self.flat = flat

    def value(self, x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        v = np.full(np.broadcast(x, y).shape, 128.0)
        for (kx, ky), ph, a in zip(self.k, self.phase, self.amp):
            v = v + a * np.sin(kx * x + ky * y + ph)
        gx, gy = x / self.cell + 64.0, y / self.cell + 64.0
        ix, iy = np.floor(gx).astype(int), np.floor(gy).astype(int)
        fx, fy = gx - ix, gy - iy
        fx, fy = fx * fx * (3 - 2 * fx), fy * fy * (3 - 2 * fy)
        g = self.grid
        ix, iy = ix % 255, iy % 255
        v = v + (g[iy, ix] * (1 - fx) + g[iy, ix + 1] * fx) * (1 - fy) + (g[iy + 1, ix] * (1 - fx) + g[iy + 1, ix + 1] * fx) * fy
        x0, y0, x1, y1 = self.flat
        return np.where((x >= x0) & (x <= x1) & (y >= y0) & (y <= y1), 128.0, v)

    def render(self, w, h, M=None, t=(0.0, 0.0)):
        """the scene after the motion x -> M x + t (M: 2 x 2, identity by default)"""
        X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        X, Y = X - t[0], Y - t[1]
        if M is not None:
            Mi = np.linalg.inv(np.asarray(M, np.float64))
            X, Y = Mi[0, 0] * X + Mi[0, 1] * Y, Mi[1, 0] * X + Mi[1, 1] * Y
        return np.clip(np.rint(self.value(X, Y)), 0, 255).astype(np.uint8)
