"""CPU: the host side of the VO frame (loam_vo_frames_*): the numpy matcher restatement the GPU
tests compare against agrees with a second formulation on the planted cases, the planted cases
are what they claim, vo_to_velo_prior against a plain 4x4 composition, the argument checks that
need no device, and that the C++ shim's VisualOdometryFrames compiles as the nodes compile it."""
import ctypes
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import vo_frames_np as N
from loam_amd import _core, vo
from vo_frames_util import compile_shim


@pytest.mark.parametrize("n0,n1,nb", [(257, 300, 32), (65, 64, 64), (40, 3, 32), (5, 2, 8), (3, 1, 32), (0, 70, 32),
                                      (300, 1025, 32)])
def test_matcher_restatements_agree(n0, n1, nb):
    rng = np.random.default_rng(n0 * 131 + n1)
    d0, d1, expect = N.planted(rng, n0, n1, nb)
    a, b = N.hamming_unpackbits(d0, d1), N.hamming_lut(d0, d1)
    assert np.array_equal(a, b)
    m = N.ratio_matches(a)
    assert np.array_equal(m, N.match(d0, d1, hamming=N.hamming_lut))
    if n1 < 2:
        assert len(m) == 0
        return
    # a plain loop over the rows: the two smallest by sorting, the same double expression
    slow = []
    for q in range(n0):
        order = np.argsort(a[q], kind="stable")
        e0, e1 = int(a[q, order[0]]), int(a[q, order[1]])
        if float(e0) < 0.8 * float(e1):
            slow.append((q, int(order[0]), e0))
    assert np.array_equal(m, np.array(slow, dtype=np.int32).reshape(-1, 3))
    got = set(m[:, 0].tolist())
    for q, ok in expect.items():
        assert (q in got) == ok, (q, ok, np.sort(a[q])[:3])
    # an accepted match has a strictly unique best
    for q, t, d in m:
        assert (a[q] == d).sum() == 1 and a[q, t] == d


def test_planted_boundaries_are_exact():
    """5 d0 == 4 d1 is rejected by the double expression, one bit either side decides"""
    for e0, e1, ok in ((4, 5, False), (40, 50, False), (4, 6, True), (39, 50, True), (41, 50, False), (8, 10, False)):
        assert (float(e0) < 0.8 * float(e1)) == ok
    rng = np.random.default_rng(4)
    d0, d1, expect = N.planted(rng, 64, 257, 32)
    assert sum(expect.values()) >= 8 and sum(not v for v in expect.values()) >= 4


def test_gate_and_ulps():
    kp0 = np.array([[100.7, 50.2], [100.7, 50.2], [100.9, 50.9]], np.float32)
    kp1 = np.array([[160.9, 130.4], [200.1, 51.99], [200.0, 50.0]], np.float32)
    m = np.array([[0, 0, 0], [1, 1, 0], [2, 2, 0]], np.int32)
    prev, curr, keep = N.gate(kp0, kp1, m, 100)
    assert prev.tolist() == [[100, 50]] * 3 and curr.tolist() == [[160, 130], [200, 51], [200, 50]]
    assert keep.tolist() == [True, False, True]          # 60^2 + 80^2 = r^2, r^2 + 1, r^2
    assert N.gate(kp0, kp1, m, 0)[2].all()
    one = np.float32(1.0)
    assert N.ulps32([one, one, -one], [np.nextafter(one, np.float32(2)), one, -one]).tolist() == [1, 0, 0]


def compose(x6, V):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(x6[:3]).as_matrix()
    T[:3, 3] = x6[3:]
    return V @ np.linalg.inv(T) @ np.linalg.inv(V)


@pytest.mark.parametrize("seed", range(6))
def test_vo_to_velo_prior_is_the_matrix_composition(seed):
    rng = np.random.default_rng(seed)
    V = np.eye(4)
    V[:3, :3] = Rotation.from_rotvec(rng.normal(0, 1.0, 3)).as_matrix()
    V[:3, 3] = rng.normal(0, 0.5, 3)
    scale = (1e-3, 0.02, 0.3, 1.5, 3.0, 1e-7)[seed]
    x6 = np.concatenate([rng.normal(0, scale, 3), rng.normal(0, 1.0, 3)])
    q, t = vo.vo_to_velo_prior(x6, V)
    M = compose(x6, V)
    assert abs(np.linalg.norm(q) - 1.0) < 1e-12
    assert np.abs(Rotation.from_quat(q).as_matrix() - M[:3, :3]).max() < 1e-12
    assert np.abs(t - M[:3, 3]).max() < 1e-12


def test_vo_to_velo_prior_guards():
    V = np.eye(4)
    assert vo.vo_to_velo_prior(np.array([0, 0, 0, 0.1, 0.2, -0.9]), V) is None       # angle 0: 0 / 0
    assert vo.vo_to_velo_prior(np.zeros(6), V) is None
    for k in range(6):
        x = np.array([0.01, -0.02, 0.005, 0.05, -0.02, -0.9])
        x[k] = np.nan
        assert vo.vo_to_velo_prior(x, V) is None
    Vn = np.eye(4)
    Vn[0, 3] = np.nan
    assert vo.vo_to_velo_prior(np.array([0.01, 0, 0, 0, 0, 1.0]), Vn) is None
    assert vo.vo_to_velo_prior(np.array([0.01, 0, 0, 0, 0, 1.0]), V) is not None


def test_entry_points_validate_before_any_device_work():
    L = _core.lib()
    p = vo.vo_frames_params()
    assert (p.remove_vo_outlier, p.desc_bytes, p.depth_radius, p.max_iterations, p.max_keypoints) == \
        (100, 32, 2, 100, 8192)
    assert abs(p.match_ratio - 0.8) < 1e-15
    h = ctypes.c_void_p()
    assert L.loam_vo_frames_create(ctypes.byref(p), None, 1, ctypes.byref(h)) == -1   # no depth handle
    assert L.loam_vo_frames_create(None, None, 1, ctypes.byref(h)) == -1
    assert L.loam_vo_frames_solve(None) == -1
    assert L.loam_vo_frames_destroy(None) == -1
    assert L.loam_vo_frames_set_initial(None, 0, None) == -1
    assert L.loam_vo_frames_result(None, 0, None, None, None) == -1


def test_cxx_shim_check_compiles(tmp_path):
    """tests/cxx/vo_frames_check.cpp through include/loam_core.hpp with the nodes' compiler and
    warnings; without an input file it only reports the library version"""
    exe = compile_shim(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "version" in r.stdout
