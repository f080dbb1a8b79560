"""The convergence tail picks its square-root backward kernel by the launch width (tog_plan::tail_backward,
csrc/tog_host_plan.hpp): k_bwd_quad while the launch fits one resident round of one workgroup per
CU, the one-wave k_bwd_team above that.

* The verdicts at the widths around the one- and two-round boundaries, for two CU counts, through a stand-alone
  host program (tests/c/tail_plan_host.cpp) under AddressSanitizer + UBSan.
* On the device, a config-3 batch just wider than one round (B = CUs + 8) stepped with the default plan (team at
  that width) equals the same steps with TOG_BWD_TAIL=quad bit for bit: the plan changes which kernel runs,
  never what it computes.
"""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

# quad while width <= cus, team above
VERDICTS = {
    256: {1: "quad", 256: "quad", 257: "team", 512: "team", 513: "team", 2048: "team"},
    304: {1: "quad", 304: "quad", 305: "team", 608: "team", 609: "team", 2048: "team"},
}


def test_tail_plan_verdicts_under_sanitizers(tmp_path):  # (host only: sanitizers never run in a gpu test)
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "tail_plan_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "tail_plan_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == "ok", r.stdout + r.stderr
    got = {}
    for ln in lines[:-2]:
        cus, width, verdict = ln.split()
        got.setdefault(int(cus), {})[int(width)] = verdict
    assert got == VERDICTS


def _steps(tog, B, nsteps, env):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        prob, opts = tog.Problems.config_quadrotor(B=B)
        h = tog.AbstractSolverFor(prob, opts).handle
        h.solve_init(tog.abi.MODE_AL)
        for _ in range(nsteps):
            h.solve_step(1)
        A = tog.abi
        return {f: h.get(f, raw=True) for f in (A.FIELD_X, A.FIELD_U, A.FIELD_K, A.FIELD_D, A.FIELD_STATS)}
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
def test_plan_and_forced_quad_agree_past_one_round(tog, gpu, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "cu_count"
    r = subprocess.run([hipcc, str(ROOT / "tests" / "c" / "cu_count.cpp"), "-o", str(exe)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    cus = int(r.stdout)
    B = cus + 8  # a second quad round of 8 workgroups; the default plan takes the team kernel here
    a = _steps(tog, B, 8, {"TOG_BWD_TAIL": None})
    b = _steps(tog, B, 8, {"TOG_BWD_TAIL": "quad"})
    assert a[tog.abi.FIELD_STATS][:, tog.abi.STAT_TOTAL_STEPS].min() >= 1  # the steps really iterated
    for f in a:
        assert np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64)), f
