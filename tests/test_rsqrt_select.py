"""tog_rsqrt_select (include/tog_math.h), the straight-line form of tog_rsqrt that wave D of k_bwd_quad calls: the
same result bits as tog_rsqrt for every class of input (0, subnormals, DBL_MIN, 1, DBL_MAX, +Inf, -0.0, negatives,
NaN) and for 2^20 seeded normals across the exponent range, through a stand-alone host program
(tests/c/rsqrt_select_host.cpp) under AddressSanitizer + UBSan. CPU only."""
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "c" / "rsqrt_select_host.cpp"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-ffp-contract=off", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}"]


def test_rsqrt_select_equals_rsqrt_under_sanitizers(tmp_path):  # (host only: sanitizers never run in a gpu test)
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    ref, exe = tmp_path / "rsqrt_reference.o", tmp_path / "rsqrt_select_host"
    # the reference's own unit: tog_rsqrt's signed seed difference overflows at -0.0 (see the program's header)
    r = subprocess.run([cxx, *SAN, "-fno-sanitize=signed-integer-overflow", "-DRSQRT_REFERENCE_UNIT", "-c", str(SRC),
                        "-o", str(ref)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([cxx, *SAN, str(SRC), str(ref), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == "ok", r.stdout + r.stderr
    assert int(lines[-3]) == 14 + (1 << 20)
