"""When a tail step's Jacobians and cost expansion go out as one launch, and how that launch's grid is cut
(tog_plan::tail_prepare, prepare_role in csrc/tog_host_plan.hpp; DESIGN.md §5 "One preparation launch"): fused only
under the tail flag, with the team backward path, a model on the plain k_jacobian branch and no TOG_TAIL_PREPARE=split;
the grid is three contiguous ranges of 256-thread blocks, [Jacobian | 4-lane expansion teams | TEAM-lane expansion
teams], of ceil(width (N-1) NCH / 256), ceil(width (N-1) / 64) (0 when every knot is on the wide teams, mode 0) and
ceil(teams / (256 / TEAM)) blocks with teams = width N (modes 0, 1) or width (mode 2); LDS is the wide teams' image,
8 x (256 / TEAM) x stride bytes.

Through a stand-alone host program (tests/c/prepare_plan_host.cpp) under AddressSanitizer + UBSan: the verdicts and
ranges below, worked out by hand at each boundary (a total that is a multiple of the block's share, one less and one
more), and the program's own sweep over small shapes and every flag combination.
"""
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent

QUAD_LDS = 8 * 16 * 182  # quadrotor, 13 rows per knot: stride 48 + 9 x 13 + 17 = 182 doubles, 16 teams per block
# (tail, team, plain, split, width, N, nch, lanes, mode, stride) -> (verdict, jac, quad, team, lds)
CASES = {
    # config 3 at one active trajectory: 500 Jacobian threads, 100 quads, the terminal knot's team
    (1, 1, 1, 0, 1, 101, 5, 16, 2, 182): ("fused", 2, 2, 1, QUAD_LDS),
    # each condition alone answers split
    (0, 1, 1, 0, 1, 101, 5, 16, 2, 182): ("split", 0, 0, 0, 0),
    (1, 0, 1, 0, 1, 101, 5, 16, 2, 182): ("split", 0, 0, 0, 0),
    (1, 1, 0, 0, 1, 101, 5, 16, 2, 182): ("split", 0, 0, 0, 0),
    (1, 1, 1, 1, 1, 101, 5, 16, 2, 182): ("split", 0, 0, 0, 0),
    # Jacobian range: 255 | 256 | 257 threads (nch = 1); every knot on the wide teams (mode 0): 256, 257, 258 teams
    (1, 1, 1, 0, 1, 256, 1, 16, 0, 182): ("fused", 1, 0, 16, QUAD_LDS),
    (1, 1, 1, 0, 1, 257, 1, 16, 0, 182): ("fused", 1, 0, 17, QUAD_LDS),
    (1, 1, 1, 0, 1, 258, 1, 16, 0, 182): ("fused", 2, 0, 17, QUAD_LDS),
    (1, 1, 1, 0, 1, 255, 1, 16, 0, 182): ("fused", 1, 0, 16, QUAD_LDS),  # 255 teams
    # quad range: 63 | 64 | 65 quads (mode 1: the wide teams still cover width N slots)
    (1, 1, 1, 0, 1, 64, 5, 16, 1, 182): ("fused", 2, 1, 4, QUAD_LDS),
    (1, 1, 1, 0, 1, 65, 5, 16, 1, 182): ("fused", 2, 1, 5, QUAD_LDS),
    (1, 1, 1, 0, 1, 66, 5, 16, 1, 182): ("fused", 2, 2, 5, QUAD_LDS),
    # team range in mode 2 (one team per trajectory): 15 | 16 | 17 trajectories of 2 knots
    (1, 1, 1, 0, 15, 2, 5, 16, 2, 182): ("fused", 1, 1, 1, QUAD_LDS),
    (1, 1, 1, 0, 16, 2, 5, 16, 2, 182): ("fused", 1, 1, 1, QUAD_LDS),
    (1, 1, 1, 0, 17, 2, 5, 16, 2, 182): ("fused", 1, 1, 2, QUAD_LDS),
    # 8-lane teams (the cartpole: n + m = 5 partials in one chunk), 32 per block: 32 | 33 knots
    (1, 1, 1, 0, 1, 32, 1, 8, 0, 54): ("fused", 1, 0, 1, 8 * 32 * 54),
    (1, 1, 1, 0, 1, 33, 1, 8, 0, 54): ("fused", 1, 0, 2, 8 * 32 * 54),
    # the test shapes of tests/test_tail_prepare.py: B = 5, N - 1 = 17
    (1, 1, 1, 0, 5, 18, 5, 16, 2, 182): ("fused", 2, 2, 1, QUAD_LDS),  # 425 threads, 85 quads, 5 teams
    (1, 1, 1, 0, 5, 18, 5, 16, 0, 182): ("fused", 2, 0, 6, QUAD_LDS),  # 90 teams
    # the team image above 64 KB
    (1, 1, 1, 0, 1, 101, 5, 16, 2, 513): ("split", 0, 0, 0, 0),
}


def test_prepare_plan_under_sanitizers(tmp_path):  # (host only: sanitizers never run in a gpu test)
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "prepare_plan_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "prepare_plan_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    queries = list(CASES)
    r = subprocess.run([str(exe)] + [",".join(map(str, q)) for q in queries], capture_output=True, text=True,
                       timeout=120)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == "ok", r.stdout + r.stderr
    assert len(lines) == len(queries) + 2
    for q, ln in zip(queries, lines):
        f = ln.split()
        assert (f[0],) + tuple(int(v) for v in f[1:]) == CASES[q], (q, ln)
