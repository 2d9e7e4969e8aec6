"""CPU: the resource owners of csrc/device_res.h in a stand-alone program (tests/cxx/device_res_check.cpp),
built with plain g++ and linked to the library for the error text and the live counts.  Without a
device every acquire must fail cleanly; with one the program acquires, grows and releases."""
import os
import subprocess

from conftest import ROOT, gpu_available
from loam_amd import _core


def test_owners_fail_cleanly_or_release_everything(tmp_path):
    lib_dir = os.path.dirname(_core.LIB_PATH)
    exe = str(tmp_path / "device_res_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vloam-noted_amd", "csrc"),
                    "-isystem", "/opt/rocm/include", os.path.join(ROOT, "tests", "cxx", "device_res_check.cpp"),
                    "-o", exe, "-L", lib_dir, "-lloam_core", "-L", "/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "1" if gpu_available() else "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout
