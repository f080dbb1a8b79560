"""Which rollout kernel a line-search launch takes (tog_plan::spec_kernel, spec_tail2_lds, spec_tail_lds in
csrc/tog_host_plan.hpp; DESIGN.md §5 "tail"): the three-wave k_ls_spec_tail2 for a whole round of at most 32 trials
of a tail launch whose image fits 64 KB, the one-wave k_ls_spec_tail up to 64 trials, the bulk k_ls_spec /
k_ls_spec_w1 otherwise (more than 16 rows per knot, a dense cost, per-trajectory cost data, a listed round, no tail
flag, no candidate slots).

Through a stand-alone host program (tests/c/rollout_plan_host.cpp) under AddressSanitizer + UBSan: the plan of every
case of tests/test_tail_line_search.py, and the boundaries below with their LDS sizes worked out by hand
(8 bytes x (2 images of TC x (mn + 2m + n + 2p) + 2p doubles, a ring of 2 x 4 x (n + m) x 32, 16 + 32)).
"""
import pathlib
import shutil
import subprocess

import test_tail_line_search as tls  # (its CASES table only: shapes, row counts and the kernel each case means)

ROOT = pathlib.Path(__file__).resolve().parent.parent

# (tail, cand, cost_diag, tv, listed, cnt, n, m, pmax) -> (tail2_lds, tail_lds, kernel)
QUAD3 = 8 * (2 * (16 * (52 + 8 + 13 + 32) + 32) + 2 * 4 * 17 * 32 + 48)  # 62,592
QUAD1 = 8 * (16 * (52 + 8 + 13 + 32) + 32)
BOUNDARIES = {
    (1, 1, 2, 0, 0, 21, 13, 4, 16): (QUAD3, QUAD1, "tail3"),  # pmax 16 | 17
    (1, 1, 2, 0, 0, 21, 13, 4, 17): (0, 0, "bulk"),
    (1, 1, 2, 0, 0, 32, 13, 4, 16): (QUAD3, QUAD1, "tail3"),  # cnt 32 | 33, 64
    (1, 1, 2, 0, 0, 33, 13, 4, 16): (QUAD3, QUAD1, "tail1"),
    (1, 1, 2, 0, 0, 64, 13, 4, 16): (QUAD3, QUAD1, "tail1"),
    # n = 14, m = 8 (TC = 8): 8 x (7,952 + 36 p) bytes, 65,344 at p = 6 and 65,632 at p = 7, around 65,536
    (1, 1, 2, 0, 0, 21, 14, 8, 6): (65344, 8 * (8 * 154 + 12), "tail3"),
    (1, 1, 2, 0, 0, 21, 14, 8, 7): (0, 8 * (8 * 156 + 14), "tail1"),
    # the infeasible quadrotor (m = 17): 96 KB for three waves at any pmax
    (1, 1, 2, 0, 0, 21, 13, 17, 13): (0, 8 * (8 * (221 + 34 + 13 + 26) + 26), "tail1"),
    (1, 1, 2, 0, 0, 21, 13, 17, 21): (0, 0, "bulk_w1"),
    (1, 1, 0, 0, 0, 21, 13, 4, 16): (QUAD3, QUAD1, "bulk"),  # a dense cost
    (1, 1, 1, 0, 0, 21, 13, 4, 16): (QUAD3, QUAD1, "tail3"),  # diagonal, off-diagonals not +0.0
    (1, 1, 2, 1, 0, 21, 13, 4, 16): (QUAD3, QUAD1, "tail3"),  # a time-varying shared Objective
    (1, 1, 2, 2, 0, 21, 13, 4, 16): (QUAD3, QUAD1, "bulk"),  # per-trajectory cost data
    (1, 1, 2, 3, 0, 21, 13, 4, 16): (QUAD3, QUAD1, "bulk"),
    (1, 1, 2, 0, 1, 13, 13, 4, 16): (QUAD3, QUAD1, "bulk"),  # a listed round
    (1, 1, 2, 0, 1, 13, 14, 7, 14): (8 * (2 * (8 * (98 + 14 + 14 + 28) + 28) + 2 * 4 * 21 * 32 + 48),
                                     8 * (8 * (98 + 14 + 14 + 28) + 28), "bulk_w1"),
    (0, 1, 2, 0, 0, 8, 13, 4, 16): (QUAD3, QUAD1, "bulk"),  # no tail flag
    (1, 0, 2, 0, 0, 21, 13, 4, 16): (QUAD3, QUAD1, "bulk"),  # no candidate slots (the replaying line search)
}
DIMS = {("quad", False): (13, 4), ("quad", True): (13, 17), ("cartpole", False): (4, 1), ("kuka", False): (14, 7)}


def test_rollout_plan_under_sanitizers(tmp_path):  # (host only: sanitizers never run in a gpu test)
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "rollout_plan_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "rollout_plan_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    queries, want = [], []
    for q, w in BOUNDARIES.items():
        queries.append(q)
        want.append(w)
    for name, case in tls.CASES.items():  # a tail launch of every trial, shared diagonal cost, candidate slots
        n, m = DIMS[(case["model"], case["mode"] == "inf")]
        queries.append((1, 1, 2, 0, 0, case["nc"], n, m, case["pmax"]))
        want.append(case["kernel"].lower())
    r = subprocess.run([str(exe)] + [",".join(map(str, q)) for q in queries], capture_output=True, text=True,
                       timeout=120)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == "ok", r.stdout + r.stderr
    assert len(lines) == len(queries) + 2
    for q, w, ln in zip(queries, want, lines):
        l2, l1, kern = ln.split()
        got = (int(l2), int(l1), kern)
        assert (got if isinstance(w, tuple) else kern) == w, (q, got, w)
