"""The host scheduling of a streamed solve (csrc/tog_stream.hpp), without a GPU.

``tests/c/stream_plan_host.cpp`` is a stand-alone program over that header: it drives the planner and the pipelined
driver loop of tog_solve_stream with a scripted device (random finish times, seeds frozen) through J < B, J = B,
J = 3B + 5, J = 0, all slots finishing in one readback, step budgets, and one slot that never finishes until the
budget runs out. It checks that every job is started once and output once, that no active or ungathered slot is
refilled, that the active hint is never below the true active count at a step, and termination. It runs here under
AddressSanitizer + UBSan.
"""
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_stream_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "stream_plan_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "stream_plan_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
