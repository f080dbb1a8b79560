"""The host arithmetic of tog_create that decides which kernel code runs (csrc/tog_host_plan.hpp), without a GPU.

``tests/c/host_plan_host.cpp`` is a stand-alone program over that header: the run-time flag -> template constant
dispatcher of the launch table (``pick``), the stage-cost table with its Cholesky factors and the diagonal-cost
class (class 2 lets the kernels use literal zeros off the diagonal, so it must hold for +0.0 only), and the Q.xx
pattern of the packed expansion records. It runs here under AddressSanitizer + UBSan.
"""
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_host_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "host_plan_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "host_plan_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
