"""The fused finish of the candidate-copy line search (k_ls_finish): in the convergence tail one
workgroup per trajectory runs the acceptance loop, the copy of the accepted rollout, the out-of-trials fallback,
the bookkeeping and the AL outer update in one launch. It calls the same per-trajectory functions as the five
kernels it replaces (TOG_LS_FINISH=split keeps those), so a solve with either path gives the same bits: X, U and
every per-trajectory statistic.

The config-3 batch starts at offset 86 (seeds 2086-2109): on the CPU oracle trajectory 18 of it (seed 2104) has a
line search that runs out of trials (step counts 23 to 235), and every trajectory takes two or more AL outer
updates. The step-level pass checks on the device that both paths really ran.
"""
import os

import numpy as np
import pytest

OFFSET = 86


def _env(env):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return old


def _solve(tog, make, env):
    old = _env(env)
    try:
        prob, opts = make()
        gpu = prob.copy()
        solver = tog.solve_b(gpu, opts)
        return gpu._X.copy(), gpu._U.copy(), solver.handle.get(tog.abi.FIELD_STATS)
    finally:
        _env(old)


def _steps(tog, make, mode, nsteps, env):
    old = _env(env)
    try:
        prob, opts = make()
        h = tog.AbstractSolverFor(prob, opts).handle
        h.solve_init(mode)
        h.solve_step(nsteps)
        return h.get(tog.abi.FIELD_X), h.get(tog.abi.FIELD_U), h.get(tog.abi.FIELD_STATS)
    finally:
        _env(old)


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_fused_finish_equals_split_config3(tog, gpu):
    A = tog.abi

    def make():
        return tog.Problems.config_quadrotor(B=24, offset=OFFSET)

    a = _solve(tog, make, {"TOG_LS_FINISH": None})
    b = _solve(tog, make, {"TOG_LS_FINISH": "split"})
    _same(a, b)
    assert not (a[2][:, A.STAT_FLAGS].astype(np.int64) & A.TRAJ_ACTIVE).any()  # solved to the end

    # the same solve step by step on the fused path: an out-of-trials line search (forward_pass.jl:22-37 leaves
    # α = 0 and z = 0) and an AL outer update must both happen
    prob, opts = make()
    h = tog.AbstractSolverFor(prob, opts).handle
    h.solve_init(A.MODE_AL)
    prev = h.get(A.FIELD_STATS)
    ran_out = outer = 0
    for _ in range(400):
        h.solve_step(1)
        S = h.get(A.FIELD_STATS)
        stepped = S[:, A.STAT_TOTAL_STEPS] > prev[:, A.STAT_TOTAL_STEPS]
        ran_out += int(np.sum(stepped & (S[:, A.STAT_ALPHA] == 0.0) & (S[:, A.STAT_Z] == 0.0)))
        outer += int(np.sum(S[:, A.STAT_AL_ITER] > prev[:, A.STAT_AL_ITER]))
        prev = S
        if h.batch_stats()[0] == 0:
            break
    assert ran_out >= 1
    assert outer >= 1
    assert np.array_equal(prev, a[2])  # the step-level pass is the same solve


@pytest.mark.gpu
def test_fused_finish_equals_split_cartpole_ilqr(tog, gpu):
    """iLQR mode: no outer update and no constraint rows."""

    def make():
        return tog.Problems.config_cartpole(B=8)

    a = _solve(tog, make, {"TOG_LS_FINISH": None})
    b = _solve(tog, make, {"TOG_LS_FINISH": "split"})
    _same(a, b)
    assert a[2][:, tog.abi.STAT_TOTAL_STEPS].min() >= 1


@pytest.mark.gpu
def test_fused_finish_equals_split_linf_gradient(tog, gpu):
    """A gradient type other than todorov takes traj_gradient in the bookkeeping: 12 steps of config 3."""

    def make():
        prob, opts = tog.Problems.config_quadrotor(B=8)
        opts.opts_uncon.gradient_type = "ℓinf"
        return prob, opts

    a = _steps(tog, make, tog.abi.MODE_AL, 12, {"TOG_LS_FINISH": None})
    b = _steps(tog, make, tog.abi.MODE_AL, 12, {"TOG_LS_FINISH": "split"})
    _same(a, b)
    assert a[2][:, tog.abi.STAT_TOTAL_STEPS].min() == 12
