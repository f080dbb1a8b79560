"""Kuka iiwa 7-DoF (BASELINE config 5; examples/kuka_iiwa/Kuka iiwa.ipynb, src/model.jl:394-447).

RigidBodyDynamics v2.1.0 (the reference's dependency, Manifest.toml:467-472) is not available here,
so the oracle restates its algorithms (RNEA bias, CRBA mass matrix, Cholesky solve; oracle/tog_oracle.c
f_kuka). SURVEY §8(c) expected this to stay unpinned; it is pinned by:
* physics: an independent numpy formulation below (world-frame geometric Jacobians: M = Σ m JvᵀJv
  + JωᵀRIRᵀJω, gravity = Σ m Jvᵀ(-g), Coriolis from Christoffel symbols of a finite-differenced M);
* the reference's own logged output: the notebook's whole AL-iLQR solve log (cell 16), 23 iterates
  whose costs the oracle reproduces to ~11 digits (test_notebook_solve_log), and its initial AL
  cost 2479.763, which depends on the hold torques (dynamics_bias);
* the HIP model, host-compiled, equal to the oracle bit for bit (tools/kuka_host_check.cpp), and on
  the GPU the jacobian / backward / solve parity tests at the end (marked gpu).
"""
import ctypes as C
import math
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
TABLES = ROOT / "include" / "tog_kuka.h"


def _tables():
    """Parse include/tog_kuka.h (the data the oracle and the kernels compile in)."""
    txt = TABLES.read_text()
    out = {}
    for key in ("R0", "P", "MASS", "COM", "IC"):
        line = next(l for l in txt.splitlines() if l.startswith(f"#define TOG_KUKA_{key} "))
        body = line.split(" ", 2)[2].replace("{", "[").replace("}", "]")
        out[key] = np.array(eval(body), dtype=float)  # numeric literals only
    return out


T = _tables()
G = np.array([0.0, 0.0, -9.81])


def _rz(q):
    c, s = math.cos(q), math.sin(q)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _fk(q):
    """World pose (R_j, o_j) of every body frame."""
    R, o = np.eye(3), np.zeros(3)
    poses = []
    for j in range(7):
        o = o + R @ T["P"][j]
        R = R @ T["R0"][j].reshape(3, 3) @ _rz(q[j])
        poses.append((R.copy(), o.copy()))
    return poses


def np_mass_gravity(q):
    poses = _fk(q)
    M = np.zeros((7, 7))
    g = np.zeros(7)
    for j in range(7):
        Rj, oj = poses[j]
        pc = oj + Rj @ T["COM"][j]
        Jv = np.zeros((3, 7))
        Jw = np.zeros((3, 7))
        for i in range(j + 1):
            Ri, oi = poses[i]
            z = Ri[:, 2]
            Jv[:, i] = np.cross(z, pc - oi)
            Jw[:, i] = z
        ixx, ixy, ixz, iyy, iyz, izz = T["IC"][j]
        Ic = np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]])
        m = T["MASS"][j]
        M += m * Jv.T @ Jv + Jw.T @ Rj @ Ic @ Rj.T @ Jw
        g += m * Jv.T @ (-G)
    return M, g


def np_coriolis(q, v, h=1e-6):
    """C(q,v)v = Σ_jk Γ_ijk v_j v_k with Christoffel symbols from central differences of M."""
    dM = np.zeros((7, 7, 7))  # dM[:, :, k] = ∂M/∂q_k
    for k in range(7):
        e = np.zeros(7)
        e[k] = h
        dM[:, :, k] = (np_mass_gravity(q + e)[0] - np_mass_gravity(q - e)[0]) / (2 * h)
    c = np.zeros(7)
    for i in range(7):
        for j in range(7):
            for k in range(7):
                c[i] += 0.5 * (dM[i, j, k] + dM[i, k, j] - dM[j, k, i]) * v[j] * v[k]
    return c


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def olib(oracle):
    return oracle.lib()


def oracle_mass(olib, q):
    M = np.zeros((7, 7), order="F")
    olib.oc_kuka_mass(_dp(M), _dp(np.ascontiguousarray(q, float)))
    return M


def oracle_bias(olib, q, v):
    tau = np.zeros(7)
    olib.oc_kuka_bias(_dp(tau), _dp(np.ascontiguousarray(q, float)), _dp(np.ascontiguousarray(v, float)))
    return tau


def test_mass_matrix_crba_matches_energy_form(olib):
    rng = np.random.default_rng(0)
    for _ in range(10):
        q = rng.uniform(-math.pi, math.pi, 7)
        M_ref, _ = np_mass_gravity(q)
        M = oracle_mass(olib, q)
        assert np.allclose(M, M_ref, rtol=1e-12, atol=1e-13)
        assert np.all(np.linalg.eigvalsh(M) > 0)


def test_bias_gravity_and_coriolis(olib):
    rng = np.random.default_rng(1)
    for _ in range(4):
        q = rng.uniform(-math.pi, math.pi, 7)
        v = rng.uniform(-2, 2, 7)
        _, g = np_mass_gravity(q)
        assert np.allclose(oracle_bias(olib, q, np.zeros(7)), g, rtol=1e-12, atol=1e-12)
        cor = oracle_bias(olib, q, v) - oracle_bias(olib, q, np.zeros(7))
        assert np.allclose(cor, np_coriolis(q, v), rtol=1e-6, atol=1e-7)


def test_dynamics_is_mass_inverse(oracle, olib):
    """ẋ = [v; M⁻¹(u − c)] (RBD dynamics!, src/model.jl:410-414)."""
    rng = np.random.default_rng(2)
    q, v, u = rng.uniform(-1, 1, 7), rng.uniform(-1, 1, 7), rng.uniform(-5, 5, 7)
    xd = oracle.continuous_f(5, np.r_[q, v], u)
    M = oracle_mass(olib, q)
    assert np.array_equal(xd[:7], v)
    assert np.allclose(xd[7:], np.linalg.solve(M, u - oracle_bias(olib, q, v)), rtol=1e-11, atol=1e-12)


def test_jacobian_matches_central_differences(oracle):
    """ForwardDiff Jacobian of the rk3 step (src/model.jl:491-522) vs central differences."""
    rng = np.random.default_rng(3)
    x, u, dt = rng.uniform(-1, 1, 14), rng.uniform(-3, 3, 7), 0.1
    S = oracle.discrete_jacobian(5, 0, x, u, dt)
    z = np.r_[x, u]
    h = 1e-6
    for c in range(21):
        e = np.zeros(21)
        e[c] = h
        fp = oracle.discrete_f(5, 0, (z + e)[:14], (z + e)[14:], dt)
        fm = oracle.discrete_f(5, 0, (z - e)[:14], (z - e)[14:], dt)
        assert np.allclose(S[:, c], (fp - fm) / (2 * h), rtol=1e-6, atol=1e-7), c


def test_hold_trajectory_and_notebook_initial_cost(tog, oracle, olib):
    """Kuka iiwa.ipynb cells 15-16: x0 = 0, U0 = hold_trajectory -> initial AL cost 2479.763."""
    x0 = np.zeros(14)
    tau = tog.Problems.dynamics_bias(tog.Dynamics.kuka, x0)  # libtog host evaluation
    assert np.array_equal(tau, oracle_bias(olib, np.zeros(7), np.zeros(7)))  # bit for bit
    prob = tog.Problems.kuka()
    assert np.array_equal(prob._U[0, 0], tau)
    opts = tog.Problems.kuka_options()
    o = oracle.OracleSolver(prob, opts, b=0)
    o.rollout_open_loop()
    assert np.array_equal(o.get("X")[-1], x0)  # the hold torques hold the arm exactly
    o.update_constraints()
    assert round(o.cost(True), 3) == 2479.763


def test_notebook_solve_log(tog, oracle):
    """The whole AL-iLQR solve of the notebook (cell 16): every logged inner iterate's cost (printed
    to ~11 digits), line-search α and z, and each outer iteration's total/c_max, reproduced by the
    oracle from the same problem (tests/golden/kuka_notebook_log.json, extracted by
    make_kuka_notebook_log.py). This pins the RBD restatement to the reference's own output."""
    import json
    log = json.loads((ROOT / "tests" / "golden" / "kuka_notebook_log.json").read_text())
    prob, opts = tog.Problems.kuka(), tog.Problems.kuka_options()
    o = oracle.OracleSolver(prob, opts, b=0)
    steps = o.solve()
    tr = o.trace()
    assert steps == len(log["inner"]) == 23
    for row, ref in zip(tr, log["inner"]):
        assert abs(row[0] - ref["cost"]) <= 1e-9 * ref["cost"] + 5e-9, (row[0], ref["cost"])
        assert row[1] == ref["alpha"]
        assert abs(row[5] - ref["z"]) < 5e-6, (row[5], ref["z"])
    assert abs(o.max_violation() - log["outer"][-1]["c_max"]) < 1e-8


def test_host_model_bitwise_equal_to_oracle(oracle, tmp_path):
    """The HIP model code (csrc/tog_device.hpp Kuka), compiled for the host, reproduces the
    oracle's f, rk3 step and dual Jacobian columns bit for bit."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not pathlib.Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = next(ROOT.glob("*_amd")) / "csrc"
    exe = tmp_path / "tog_kuka_host_check"
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "-x", "hip", "--offload-arch=gfx950",
                        "--cuda-host-only", f"-I{csrc}", str(ROOT / "tools" / "kuka_host_check.cpp"), "-o",
                        str(exe), "-ldl"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), str(ROOT / "oracle" / "liboracle.so")], capture_output=True, text=True)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr


# --------------------------------------------------------------------------- GPU parity (config 5)
TOL_STEP = 1e-13
TOL_SOLVE = 1e-6


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))


@pytest.mark.gpu
def test_kuka_jacobian_parity(tog, oracle, gpu):
    prob, _ = tog.Problems.config_kuka(B=3)
    rng = np.random.default_rng(4)
    prob._X[...] = rng.uniform(-1, 1, prob._X.shape)
    solver = tog.iLQRSolver(prob, tog.iLQRSolverOptions())
    tog.jacobian_b(prob, solver)
    A = solver.handle.get(tog.abi.FIELD_A)
    Bm = solver.handle.get(tog.abi.FIELD_B)
    for b in range(prob.B):
        for k in range(prob.N - 1):
            S = oracle.discrete_jacobian(5, 0, prob._X[b, k], prob._U[b, k], prob.dt)
            assert rel(A[b, k], S[:, :14]) < TOL_STEP, (b, k)
            assert rel(Bm[b, k], S[:, 14:21]) < TOL_STEP, (b, k)


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
def test_kuka_backward_pass_parity(tog, oracle, gpu, sqrt):
    prob, opts_al = tog.Problems.config_kuka(B=3)
    opts_al.opts_uncon.square_root = sqrt
    solver = tog.AbstractSolverFor(prob, opts_al)
    h = solver.handle
    h.rollout_open_loop()
    h.jacobians()
    dV = h.backward_pass(sqrt=sqrt, al=True, store_S=True)
    K, d = h.get(tog.abi.FIELD_K), h.get(tog.abi.FIELD_D)
    for b in range(prob.B):
        o = oracle.OracleSolver(prob, opts_al, b=b)
        o.rollout_open_loop()
        o.update_constraints()
        o.jacobians()
        assert o.cost_expansion(sqrt, True) == 0
        dV_ref, _ = o.backward(sqrt)
        assert rel(dV[b], dV_ref) < TOL_STEP
        assert rel(K[b], o.get("K")) < TOL_STEP
        assert rel(d[b], o.get("d")) < TOL_STEP


@pytest.mark.gpu
def test_kuka_solve_al(tog, oracle, gpu):
    """Config 5 (AL-iLQR, terminal goal, notebook options) on a small batch: X, U and iteration
    counts equal to the oracle's, and the goal reached to the constraint tolerance."""
    prob, opts = tog.Problems.config_kuka(B=2)
    gp = prob.copy()
    solver = tog.solve_b(gp, opts)
    for b in range(prob.B):
        o = oracle.OracleSolver(prob, opts, b=b)
        steps = o.solve()
        assert rel(gp._X[b], o.get("X")) < TOL_SOLVE
        assert rel(gp._U[b], o.get("U")) < TOL_SOLVE
        assert steps == solver.stats["iterations_total"][b]
    assert np.all(solver.stats["c_max"] < opts.constraint_tolerance)


@pytest.mark.gpu
def test_kuka_notebook_solve_on_gpu(tog, oracle, gpu):
    """The notebook problem (x0 = 0, hold-torque U0) solved by the HIP path: 23 iterations, the
    oracle's X/U, and the logged final c_max."""
    import json
    log = json.loads((ROOT / "tests" / "golden" / "kuka_notebook_log.json").read_text())
    prob, opts = tog.Problems.kuka(), tog.Problems.kuka_options()
    gp = prob.copy()
    solver = tog.solve_b(gp, opts)
    o = oracle.OracleSolver(prob, opts, b=0)
    o.solve()
    assert int(solver.stats["iterations_total"][0]) == len(log["inner"])
    assert rel(gp._X[0], o.get("X")) < TOL_SOLVE and rel(gp._U[0], o.get("U")) < TOL_SOLVE
    assert abs(solver.stats["c_max"][0] - log["outer"][-1]["c_max"]) < 1e-8
