"""Visual-odometry pose solve on MI355X — host side of VisualOdometry::solveNlsAll
(src/visual_odometry/src/visual_odometry.cpp:304-509).

``vo_factors`` builds the residual blocks of one frame pair the way the reference does
(:346-493): a match whose previous point has a depth (``queryDepth`` > 0) becomes a
CostFunctor32 (3D point in rectified camera 0 -> normalised image point), otherwise a
CostFunctor22 (epipolar).  ``solve`` runs any number of such problems on the device (one
workgroup per problem, every Ceres iteration on the GPU): HuberLoss(0.1), TR-LM, DENSE_QR,
max_num_iterations = 100 (:70-74).

``VOFrames`` is the whole frame on the device: descriptors, LK tracks, the two images and the
points to track (pyramidal Lucas-Kanade on the device), or the two images alone (Shi-Tomasi corners
and, in the reference's default configuration, ORB descriptors on the device) in, pose out, with the matcher, the gate,
the depth lookup and the records between them (``vo_factors`` stays the host
definition the device records are checked against).  ``vo_to_velo_prior`` turns its solution into
the prior of the coupled LiDAR odometry.
"""
import ctypes

import numpy as np

from . import _core
from ._core import check, lib, ptr

CF32, CF22 = 4, 5


def vo_factors(prev_xy, curr_xy, depth0, P_rect0):
    """factor records (n, 10) of one frame pair.  prev_xy / curr_xy: matched pixel coordinates
    (the reference stores them in ints, :346); depth0: queryDepth of the previous points.
    The 3x3 solves with P_rect0.leftCols(3) (:421-424, colPivHouseholderQr in float) are done
    in float64 and rounded to float32 here: the records match the reference to float rounding,
    not bit for bit."""
    K = np.asarray(P_rect0, dtype=np.float64)[:, :3]
    prev = np.asarray(prev_xy).astype(np.int32).astype(np.float32)
    curr = np.asarray(curr_xy).astype(np.int32).astype(np.float32)
    d0 = np.asarray(depth0, dtype=np.float32)
    n = len(prev)
    out = np.zeros((n, 10))
    ones = np.ones(n, np.float32)
    p1 = np.linalg.solve(K, np.stack([curr[:, 0], curr[:, 1], ones]).astype(np.float64)).T.astype(np.float32)
    x1 = p1[:, 0].astype(np.float64) / p1[:, 2].astype(np.float64)
    y1 = p1[:, 1].astype(np.float64) / p1[:, 2].astype(np.float64)
    has = d0 > 0
    h0 = np.stack([prev[:, 0] * d0, prev[:, 1] * d0, d0])
    X0 = np.linalg.solve(K, h0.astype(np.float64)).T.astype(np.float32)
    p0 = np.linalg.solve(K, np.stack([prev[:, 0], prev[:, 1], ones]).astype(np.float64)).T.astype(np.float32)
    out[has, 0] = CF32
    out[has, 1:4] = X0[has]
    out[has, 4] = x1[has]
    out[has, 5] = y1[has]
    nh = ~has
    out[nh, 0] = CF22
    out[nh, 4] = p0[nh, 0].astype(np.float64) / p0[nh, 2].astype(np.float64)
    out[nh, 5] = p0[nh, 1].astype(np.float64) / p0[nh, 2].astype(np.float64)
    out[nh, 7] = x1[nh]
    out[nh, 8] = y1[nh]
    return out


def solve(problems, x0=None, max_iterations=100, device=0):
    """problems: list of (n_i, 10) factor arrays; x0: (P, 6) initial angles_0to1, t_0to1 (zeros
    by default, reset_VO_to_identity).  Returns (x (P, 6), [LMStats])."""
    P = len(problems)
    off = np.zeros(P + 1, dtype=np.int32)
    for i, f in enumerate(problems):
        off[i + 1] = off[i] + len(f)
    F = np.ascontiguousarray(np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in problems])
                             if P else np.zeros((0, 10)))
    x = np.zeros((P, 6)) if x0 is None else np.array(x0, dtype=np.float64).reshape(P, 6).copy()
    st = (_core.LMStats * max(P, 1))()
    check(lib().loam_vo_solve(device, P, ptr(off), ptr(F), ptr(x), max_iterations, st))
    return x, [st[i] for i in range(P)]


def vo_frames_params(P_rect0=None, **kw):
    """loam_vo_frames_params: the reference's defaults (remove_vo_outlier 100, match_ratio 0.8,
    ORB's 32-byte descriptors, searching_radius 2, 100 iterations, 8192 keypoints per image)"""
    if P_rect0 is None:
        from .depth import KITTI_P_RECT0 as P_rect0
    p = _core.VOFramesParams()
    lib().loam_vo_frames_params_default(ctypes.byref(p))
    p.P_rect0[:] = [float(v) for v in np.ascontiguousarray(P_rect0, dtype=np.float32).reshape(12)]
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def lk_params(max_width, max_height, **kw):
    """loam_lk_params: the reference's cv::calcOpticalFlowPyrLK call (window 15, maxLevel 2,
    COUNT + EPS (10, 0.03), minEigThreshold 1e-4) for images up to max_width x max_height"""
    p = _core.LKParams()
    lib().loam_lk_params_default(ctypes.byref(p))
    p.max_width, p.max_height = int(max_width), int(max_height)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def gftt_params(**kw):
    """loam_gftt_params: the reference's cv::goodFeaturesToTrack call (1024 corners, quality 0.03,
    minDistance 7.5, blockSize 5), 65536 candidates per image"""
    p = _core.GFTTParams()
    lib().loam_gftt_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def orb_params(**kw):
    """loam_orb_params: cv::ORB::create()'s edgeThreshold 31"""
    p = _core.ORBParams()
    lib().loam_orb_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _image_pair(img_prev, img_curr):
    """(a, b, w, h, row_stride): two (height, width) uint8 images of one size as arrays of one row
    stride with dense rows (copied where they are not)"""
    a, b = np.asarray(img_prev), np.asarray(img_curr)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 2 or a.shape != b.shape:
        raise ValueError("two 8-bit single-channel images of one size")
    if a.size and (a.strides[1] != 1 or b.strides != a.strides):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    h, w = a.shape
    return a, b, w, h, a.strides[0] if a.size else w


class VOFrames:
    """The VO frame on the device (loam_vo_frames_*): ``n_pairs`` independent frame pairs, each
    from its descriptors (or LK tracks) to angles_0to1 / t_0to1 in one launch sequence per
    ``solve``: ImageUtil::matchDescriptors, the outlier gate, queryDepth on ``depth`` (a
    ``BatchDepth`` whose streams hold the previous frames' buckets), the CostFunctor32 / 22
    records and the Ceres solve of VisualOdometry::solveNlsAll."""

    def __init__(self, depth, n_pairs=1, params=None, **kw):
        self.params = params if params is not None else vo_frames_params(
            kw.pop("P_rect0", np.array(depth.params.P_rect0[:], dtype=np.float32)), **kw)
        self.depth = depth  # the depth handle must outlive this one
        self.n_pairs = n_pairs
        h = ctypes.c_void_p()
        check(lib().loam_vo_frames_create(ctypes.byref(self.params), depth.h, n_pairs, ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().loam_vo_frames_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def input_descriptors(self, pair, kp0_xy, desc0, kp1_xy, desc1, depth_stream_prev=0):
        """previous (0) / current (1) image: keypoint pixels (n, 2) and descriptors (n, desc_bytes)"""
        nb = self.params.desc_bytes
        k0 = np.ascontiguousarray(kp0_xy, dtype=np.float32).reshape(-1, 2)
        k1 = np.ascontiguousarray(kp1_xy, dtype=np.float32).reshape(-1, 2)
        d0 = np.ascontiguousarray(desc0, dtype=np.uint8).reshape(-1, nb)
        d1 = np.ascontiguousarray(desc1, dtype=np.uint8).reshape(-1, nb)
        if len(k0) != len(d0) or len(k1) != len(d1):
            raise ValueError("one keypoint per descriptor")
        check(lib().loam_vo_frames_input_descriptors(self.h, pair, ptr(k0), ptr(d0), len(d0), ptr(k1), ptr(d1),
                                                     len(d1), depth_stream_prev))

    def input_tracks(self, pair, prev_xy, curr_xy, status, depth_stream_prev=0):
        """optical_flow_match: paired points and the LK status (kept where 1)"""
        a = np.ascontiguousarray(prev_xy, dtype=np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(curr_xy, dtype=np.float32).reshape(-1, 2)
        s = np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
        if not len(a) == len(b) == len(s):
            raise ValueError("prev_xy, curr_xy and status must have one row per track")
        check(lib().loam_vo_frames_input_tracks(self.h, pair, ptr(a), ptr(b), ptr(s), len(s), depth_stream_prev))

    def enable_images(self, max_width, max_height, **kw):
        """allocate the image pyramids of every pair (once); kw: loam_lk_params fields"""
        self.lk = lk_params(max_width, max_height, **kw)
        check(lib().loam_vo_frames_enable_images(self.h, ctypes.byref(self.lk)))

    def input_images(self, pair, img_prev, img_curr, pts_xy, depth_stream_prev=0):
        """optical_flow_match from the images: two (height, width) uint8 images of one size (rows
        may be strided views) and the (n, 2) points of the previous image to track"""
        a, b, w, h, row_stride = _image_pair(img_prev, img_curr)
        pts = np.ascontiguousarray(pts_xy, dtype=np.float32).reshape(-1, 2)
        check(lib().loam_vo_frames_input_images(self.h, pair, a.ctypes.data, b.ctypes.data, w, h, row_stride,
                                                ptr(pts), len(pts), depth_stream_prev))

    def enable_detection(self, **kw):
        """allocate the corner detector's buffers of every pair (once, after enable_images); kw:
        loam_gftt_params fields"""
        self.gftt = gftt_params(**kw)
        check(lib().loam_vo_frames_enable_detection(self.h, ctypes.byref(self.gftt)))

    def input_image_pair(self, pair, img_prev, img_curr, detect_on=0, depth_stream_prev=0):
        """optical_flow_match from the two images alone: goodFeaturesToTrack on the previous image
        (detect_on 0) or the current one (1, the reference's order) runs on the device, and the
        corners are tracked from img_prev to img_curr"""
        a, b, w, h, row_stride = _image_pair(img_prev, img_curr)
        check(lib().loam_vo_frames_input_image_pair(self.h, pair, a.ctypes.data, b.ctypes.data, w, h, row_stride,
                                                    detect_on, depth_stream_prev))

    def eig(self, pair=0):
        """the (h, w) float32 minimum-eigenvalue plane of the pair's last detection"""
        wh = np.zeros(2, np.int32)
        n = check(lib().loam_vo_frames_eig_copy(self.h, pair, None, 0, ptr(wh)))
        out = np.empty((int(wh[1]), int(wh[0])), np.float32)
        check(lib().loam_vo_frames_eig_copy(self.h, pair, ptr(out), n, None))
        return out

    def enable_description(self, **kw):
        """allocate the blurred planes of every pair (once, after enable_images); kw: loam_orb_params
        fields"""
        self.orb = orb_params(**kw)
        check(lib().loam_vo_frames_enable_description(self.h, ctypes.byref(self.orb)))

    def input_images_keypoints(self, pair, img_prev, img_curr, kp0_xy, kp1_xy, angle0_deg=None, angle1_deg=None,
                               depth_stream_prev=0):
        """optical_flow_match = false from the images and keypoints of one's own: (n, 2) pixel
        coordinates per image and, optionally, their angles in degrees (None: -1 for all, as
        cv::KeyPoint's default); ORB's border filter and descriptors run on the device in front of the
        matcher"""
        a, b, w, h, row_stride = _image_pair(img_prev, img_curr)
        k0 = np.ascontiguousarray(kp0_xy, dtype=np.float32).reshape(-1, 2)
        k1 = np.ascontiguousarray(kp1_xy, dtype=np.float32).reshape(-1, 2)
        a0 = None if angle0_deg is None else np.ascontiguousarray(angle0_deg, dtype=np.float32).reshape(-1)
        a1 = None if angle1_deg is None else np.ascontiguousarray(angle1_deg, dtype=np.float32).reshape(-1)
        if (a0 is not None and len(a0) != len(k0)) or (a1 is not None and len(a1) != len(k1)):
            raise ValueError("one angle per keypoint")
        # (an empty angle array is no array to the C side: -1 for all of no keypoints)
        check(lib().loam_vo_frames_input_images_keypoints(
            self.h, pair, a.ctypes.data, b.ctypes.data, w, h, row_stride, ptr(k0), ptr(a0), len(k0), ptr(k1), ptr(a1),
            len(k1), depth_stream_prev))

    def input_image_pair_match(self, pair, img_prev, img_curr, depth_stream_prev=0):
        """the reference's default frame (optical_flow_match = false) from the two images alone:
        goodFeaturesToTrack on both, ORB descriptors, the ratio-test matcher and the solve"""
        a, b, w, h, row_stride = _image_pair(img_prev, img_curr)
        check(lib().loam_vo_frames_input_image_pair_match(self.h, pair, a.ctypes.data, b.ctypes.data, w, h, row_stride,
                                                          depth_stream_prev))

    def descriptors(self, pair=0, image=0):
        """(keypoints (n, 2) float32, descriptors (n, 32) uint8) image 0 (previous) / 1 (current) kept
        in the pair's last description, in order: what the matches' indices refer to"""
        n = check(lib().loam_vo_frames_descriptors_copy(self.h, pair, image, None, None, 0))
        kp, desc = np.empty((n, 2), np.float32), np.empty((n, 32), np.uint8)
        if n:
            check(lib().loam_vo_frames_descriptors_copy(self.h, pair, image, ptr(kp), ptr(desc), n))
        return kp, desc

    def blur(self, pair=0, image=0):
        """the (h, w) uint8 blurred plane the descriptors of the pair's last description sampled"""
        wh = np.zeros(2, np.int32)
        n = check(lib().loam_vo_frames_blur_copy(self.h, pair, image, None, 0, ptr(wh)))
        out = np.empty((int(wh[1]), int(wh[0])), np.uint8)
        check(lib().loam_vo_frames_blur_copy(self.h, pair, image, ptr(out), n, None))
        return out

    def set_initial(self, pair, x6=None):
        x = None if x6 is None else np.ascontiguousarray(x6, dtype=np.float64).reshape(6)
        check(lib().loam_vo_frames_set_initial(self.h, pair, None if x is None else x.ctypes.data))

    def solve(self):
        check(lib().loam_vo_frames_solve(self.h))

    def result(self, pair=0):
        """(x6 = angles_0to1 ++ t_0to1, LMStats, VOFrameStats)"""
        x = np.empty(6)
        lm, st = _core.LMStats(), _core.VOFrameStats()
        check(lib().loam_vo_frames_result(self.h, pair, x.ctypes.data, ctypes.byref(lm), ctypes.byref(st)))
        return x, lm, st

    def matches(self, pair=0):
        """(n, 3) int32: queryIdx, trainIdx, distance of the accepted matches, in query order"""
        n = check(lib().loam_vo_frames_matches_copy(self.h, pair, None, 0))
        out = np.empty((n, 3), dtype=np.int32)
        if n:
            check(lib().loam_vo_frames_matches_copy(self.h, pair, ptr(out), n))
        return out

    def records(self, pair=0):
        """the residual blocks of the last solve, (n, 10) in ``solve``'s layout, and their depth0"""
        n = check(lib().loam_vo_frames_records_copy(self.h, pair, None, None, 0))
        rec, d0 = np.empty((n, 10)), np.empty(n, dtype=np.float32)
        if n:
            check(lib().loam_vo_frames_records_copy(self.h, pair, ptr(rec), ptr(d0), n))
        return rec, d0


    def tracks(self, pair=0):
        """(prev_xy (n, 2), curr_xy (n, 2), status (n,) uint8, err (n,)) of the pair's last tracks
        or images solve; err is LK's (0 for a tracks pair)"""
        n = check(lib().loam_vo_frames_tracks_copy(self.h, pair, None, None, None, None, 0))
        prev, curr = np.empty((n, 2), np.float32), np.empty((n, 2), np.float32)
        status, err = np.empty(n, np.uint8), np.empty(n, np.float32)
        if n:
            check(lib().loam_vo_frames_tracks_copy(self.h, pair, ptr(prev), ptr(curr), ptr(status), ptr(err), n))
        return prev, curr, status, err

    def pyramid(self, pair=0, image=0):
        """the pyramid levels (list of (h, w) uint8) of the pair's last images solve; image 0 is
        the previous, 1 the current"""
        out = []
        wh = np.zeros(2, np.int32)
        while True:
            n = lib().loam_vo_frames_pyramid_copy(self.h, pair, image, len(out), None, 0, ptr(wh))
            if n == -1 and out:
                return out  # LOAM_ERR_ARG: past the last level
            check(n)
            lvl = np.empty((int(wh[1]), int(wh[0])), np.uint8)
            check(lib().loam_vo_frames_pyramid_copy(self.h, pair, image, len(out), ptr(lvl), n, None))
            out.append(lvl)


def vo_to_velo_prior(x6, velo_T_cam0):
    """velo_last_VOT_velo_curr = velo_T_cam0 . (cam0_curr_T_cam0_last)^-1 . velo_T_cam0^-1
    (vloam_tf.cpp:66-70) of a VO solution x6 = angles_0to1 ++ t_0to1 (the axis-angle form of
    visual_odometry.cpp:485-489), as (q_xyzw, t): the argument of loam_odometry_set_prior.
    None when the angle is 0 (the reference divides by it and guards the NaN, :76-79) or any
    component is NaN."""
    x = np.asarray(x6, dtype=np.float64).reshape(6)
    V = np.asarray(velo_T_cam0, dtype=np.float64).reshape(4, 4)
    w, t = x[:3], x[3:]
    angle = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if np.isnan(x).any() or np.isnan(V).any() or angle == 0.0:
        return None
    u = w / angle
    Kx = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    R = np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)
    Tinv = np.eye(4)
    Tinv[:3, :3] = R.T
    Tinv[:3, 3] = -R.T @ t
    Vinv = np.eye(4)
    Vinv[:3, :3] = V[:3, :3].T
    Vinv[:3, 3] = -V[:3, :3].T @ V[:3, 3]
    M = V @ Tinv @ Vinv
    return _quat_xyzw(M[:3, :3]), M[:3, 3].copy()


def _quat_xyzw(R):
    """unit quaternion (x, y, z, w), w >= 0, of a rotation matrix (largest-component branch)"""
    q = np.empty(4)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q[:] = (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q
