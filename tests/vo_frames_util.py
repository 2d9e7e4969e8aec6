"""What the VO-frame suites share (test_gpu_vo_frames.py, test_gpu_lk.py, test_gpu_gftt.py): the depth
streams, small comparisons, and the C++ shim run (tests/cxx/vo_frames_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from loam_amd import _core, synth
from loam_amd.depth import KITTI_CAM_T_VELO, KITTI_P_RECT0, KITTI_RECT0_T_CAM, BatchDepth

X_INIT = np.array([0.008, -0.018, 0.004, 0.04, -0.01, -0.85])


def make_depth():
    """two processed depth streams (consecutive synthetic frames) and their clouds"""
    clouds = [synth.frame(21, 4 + s, 800)[0] for s in range(2)]
    g = BatchDepth(2)
    for s, c in enumerate(clouds):
        g.input(s, c)
    g.process()
    return g, clouds


def strided(img, extra=13):
    """the same image as a view of rows that are `extra` bytes longer"""
    buf = np.full((img.shape[0], img.shape[1] + extra), 0xA5, np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def raises(rc, fn, *a, **kw):
    """fn(*a, **kw) raises LoamError with the code rc; returns its text"""
    with pytest.raises(_core.LoamError) as e:
        fn(*a, **kw)
    assert e.value.rc == rc, (e.value.rc, str(e.value))
    return str(e.value)


def same_lm(a, b):
    return [a.iterations, a.successful, a.invalid, a.termination, a.initial_cost, a.final_cost] == \
        [b.iterations, b.successful, b.invalid, b.termination, b.initial_cost, b.final_cost]


def counters(s):
    return [s.n_knn, s.n_matches, s.n_gated, s.counter32, s.counter22]


def give(vf, pair, item):
    """item: (descriptors / tracks / images / image_pair, that input's arguments, depth stream, x0)"""
    kind, data, stream, x0 = item
    getattr(vf, "input_" + kind)(pair, *data, stream)
    vf.set_initial(pair, x0)


def compile_shim(tmp_path):
    """tests/cxx/vo_frames_check.cpp through include/loam_core.hpp with the nodes' compiler and warnings"""
    lib_dir = os.path.dirname(_core.LIB_PATH)
    exe = str(tmp_path / "vo_frames_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "vo_frames_check.cpp"), "-o", exe, "-L", lib_dir,
                    "-lloam_core", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True)
    return exe


def run_shim(tmp_path, mode, header_ints, arrays):
    """one pair through the C++ shim in `mode` (descriptors, images, detect), from X_INIT with the KITTI
    calibration: writes its input file (the int32 header, the calibration, X_INIT, the arrays: the
    cloud first), compiles and runs it.  Returns (the x / lm / stats lines as {key: [text]}, the m or
    t rows as [[text]])"""
    path = str(tmp_path / "pair.bin")
    with open(path, "wb") as f:
        f.write(np.array(header_ints, np.int32).tobytes())
        for a in (KITTI_CAM_T_VELO, KITTI_RECT0_T_CAM, KITTI_P_RECT0):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(X_INIT.astype(np.float64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([compile_shim(tmp_path), path, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines, rows = {}, []
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        if key in ("m", "t"):
            rows.append(vals)
        else:
            lines[key] = vals
    return lines, rows
