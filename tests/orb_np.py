"""numpy restatement of cv::ORB::create()->compute on given keypoints (patchSize 31, edgeThreshold 31,
WTA_K 2, 32 bytes; one pyramid level at scale 1; no orientation: a keypoint keeps the angle it comes
with), the call of ImageUtil::descKeypoints (image_util.cpp:280-339), which
loam_vo_frames_input_images_keypoints and loam_vo_frames_input_image_pair_match run on the device.

It was written from the OpenCV 4.2 source as remembered, with no OpenCV build at hand to run beside
it: THIS MODEL IS THE DEFINITION the device is held to.  The points that were chosen:
 1. border_filter: KeyPointsFilter::runByImageBorder(edge): kept iff edge <= cvRound(x) < W - edge and
    edge <= cvRound(y) < H - edge; none if W <= 2 edge or H <= 2 edge; stable.  Chosen difference: a
    coordinate that is not finite is dropped (OpenCV would read out of bounds).
 2. blur7: GaussianBlur 7 x 7, sigma 2, BORDER_REFLECT_101 as the 8-bit fixed-point separable filter
    (the image is a submatrix of the bordered pyramid buffer, so the ufixedpoint16 path is not taken):
    weights cvRound(256 g) with g the float32 normalised Gaussian = 18 34 49 55 49 34 18 (sum 257),
    int32 sums, saturate_u8((sum + 32768) >> 16).  The one point to check again against an OpenCV
    build.  No kept keypoint samples closer than 9 pixels to the edge, so the border mode never
    shows in a descriptor; the plane is REFLECT_101 all the same.
 3. describe: angle = deg * (float)(CV_PI / 180.f), a = cosf(angle), b = sinf(angle) (restated here
    as the float64 cosine and sine rounded to float32; test_orb_host.py checks that the C library's
    cosf / sinf give the same at the angles the tests use); for a pattern point (px, py):
    fx = px a - py b, fy = px b + py a in float32, every product and the sum rounded on its own,
    ix = cvRound(fx), iy = cvRound(fy) (half to even); bit t % 8 of byte t / 8 is
    blur[c + P(2t)] < blur[c + P(2t + 1)], c = (cvRound(x), cvRound(y)).
 4. PATTERN: the first 256 point pairs of OpenCV's bit_pattern_31_ (tests/golden/orb_pattern.npz;
    shape (256, 4), sum -406, sum(v[k] (k + 1)) = -177504, largest radius 18.3848)."""
import math
import os

import numpy as np

from lk_np import reflect101

F = np.float32
PATTERN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orb_pattern.npz"))[
    "pattern"].astype(np.int32)
EDGE = 31


def gaussian_weights(ksize=7, sigma=2.0, bits=8):
    """cvRound(2^bits g): g = cv::getGaussianKernel(ksize, sigma, CV_32F) (formed in double, stored as
    float32)"""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    e = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g = (e / e.sum()).astype(F)
    return np.rint(g.astype(np.float64) * (1 << bits)).astype(np.int64)


WEIGHTS = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)


def blur7(img):
    """(h, w) uint8: the blurred plane ORB samples"""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    p = a[reflect101(np.arange(-3, h + 3), h)][:, reflect101(np.arange(-3, w + 3), w)]
    row = sum(WEIGHTS[k] * p[:, k:k + w] for k in range(7))
    col = sum(WEIGHTS[k] * row[k:k + h, :] for k in range(7))
    return np.minimum((col + 32768) >> 16, 255).astype(np.uint8)


def cv_round(v):
    """cvRound of float32 values (half to even), as float64 so that nothing overflows"""
    return np.rint(np.asarray(v, F).astype(np.float64))


def border_filter(kps, w, h, edge=EDGE):
    """indices of the keypoints (n, 2) that stay, in order"""
    k = np.asarray(kps, F).reshape(-1, 2)
    if w <= 2 * edge or h <= 2 * edge:
        return np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        cx, cy = cv_round(k[:, 0]), cv_round(k[:, 1])
        ok = np.isfinite(k).all(axis=1) & (cx >= edge) & (cx < w - edge) & (cy >= edge) & (cy < h - edge)
    return np.flatnonzero(ok)


def cos_sin(angle_deg):
    angle = F(angle_deg) * F(np.pi / 180.0)
    return F(math.cos(float(angle))), F(math.sin(float(angle)))


def rotated_pattern(angle_deg):
    """(512, 2) int32: the pattern's points (x, y), point 2t and 2t + 1 of test t, rotated and rounded"""
    a, b = cos_sin(angle_deg)
    pts = PATTERN.reshape(-1, 2).astype(F)
    px, py = pts[:, 0], pts[:, 1]
    fx = px * a - py * b
    fy = px * b + py * a
    return np.stack([np.rint(fx), np.rint(fy)], axis=1).astype(np.int32)


FUSED_FORMS = ("x: fma(px, a, -(py b))", "x: fma(-py, b, px a)", "y: fma(px, b, py a)", "y: fma(py, a, px b)")


def fused_rotated_pattern(angle_deg, form):
    """NOT the definition: rotated_pattern with one of the two products of one coordinate fused into
    the sum (a single rounding), the four ways a compiler or a careless kernel could contract it; for
    the tests to show that they would notice"""
    a, b = (float(v) for v in cos_sin(angle_deg))
    pts = PATTERN.reshape(-1, 2).astype(np.float64)   # float64 is exact for these products and sums
    px, py = pts[:, 0], pts[:, 1]
    r = lambda v: np.asarray(v).astype(F).astype(np.float64)
    fx = {0: r(px * a - r(py * b)), 1: r(r(px * a) - py * b)}.get(FUSED_FORMS.index(form), r(r(px * a) - r(py * b)))
    fy = {2: r(px * b + r(py * a)), 3: r(r(px * b) + py * a)}.get(FUSED_FORMS.index(form), r(r(px * b) + r(py * a)))
    return np.stack([np.rint(fx), np.rint(fy)], axis=1).astype(np.int32)


def describe(img, kps, angles=None, edge=EDGE, blur=None, pattern_of=None):
    """(kept keypoints (m, 2) float32 in order, descriptors (m, 32) uint8, their indices into kps);
    angles: degrees per keypoint, None = -1 for all (cv::KeyPoint's default); pattern_of: another
    rotation than rotated_pattern (the tests' fused ones)"""
    img = np.asarray(img)
    h, w = img.shape
    k = np.asarray(kps, F).reshape(-1, 2)
    idx = border_filter(k, w, h, edge)
    kept = k[idx]
    ang = np.full(len(k), -1.0, F) if angles is None else np.asarray(angles, F).reshape(-1)
    ang = ang[idx]
    B = blur7(img) if blur is None else blur
    cx, cy = cv_round(kept[:, 0]).astype(np.int64), cv_round(kept[:, 1]).astype(np.int64)
    bits = np.zeros((len(kept), 256), bool)
    for v in np.unique(ang):
        sel = np.flatnonzero(ang == v)
        P = (pattern_of or rotated_pattern)(v)
        x = cx[sel, None] + P[None, :, 0]
        y = cy[sel, None] + P[None, :, 1]
        s = B[y, x]
        bits[sel] = s[:, 0::2] < s[:, 1::2]
    desc = np.packbits(bits, axis=1, bitorder="little") if len(kept) else np.zeros((0, 32), np.uint8)
    return kept, desc.reshape(-1, 32), idx
