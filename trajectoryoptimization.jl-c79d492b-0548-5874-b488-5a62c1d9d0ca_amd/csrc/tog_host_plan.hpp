// Host arithmetic that decides which kernel code a handle runs (tog_create): the run-time flag -> template
// constant dispatcher of the launch table (tog_launch.hpp), the stage-cost table with its Cholesky factors and
// diagonal-cost class, the Q.xx pattern of the packed expansion records, the grid of a tail step's fused preparation
// launch, and the line search's rollout-kernel choice with the LDS layout arithmetic of the tail rollouts. Plain C++
// with no device runtime in it, so that a stand-alone program can run it under the host sanitizers
// (tests/c/host_plan_host.cpp, rollout_plan_host.cpp, prepare_plan_host.cpp). tog_kernels.hpp
// includes it too: the spec_tail* constants and constexpr size functions below are the kernels' own LDS layout
// (used in device code), so the plan and the kernels cannot disagree about it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

namespace tog_plan {

// a run-time value -> the compile-time constant among Vs it equals: f(std::integral_constant<int, v>{})
// (f runs once when v is in Vs and never otherwise)
template <int... Vs, class F>
inline void pick(int v, F&& f) {
  (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// The square-root backward kernel of a convergence-tail launch over `width` trajectories on a device of `cus`
// compute units. The quad kernel (k_bwd_quad: a 256-thread workgroup per trajectory under a one-wave-per-SIMD
// register budget, so one workgroup is resident per CU) takes ceil(width / cus) rounds of its single-trajectory
// latency. The one-wave team kernel (k_bwd_team at one wave per SIMD, four trajectories per wave) takes one
// round of about twice that latency for any tail width. Quad while the launch fits TAIL_QUAD_ROUNDS resident
// rounds, team above (DESIGN.md §5 has the measured times on either side of the boundary).
enum TailBackward { TAIL_BWD_TEAM = 0, TAIL_BWD_QUAD = 1 };
constexpr long long TAIL_QUAD_ROUNDS = 1;
inline TailBackward tail_backward(long long width, int cus) {
  return (cus > 0 && width <= TAIL_QUAD_ROUNDS * (long long)cus) ? TAIL_BWD_QUAD : TAIL_BWD_TEAM;
}

// The preparation of a tail step: the Jacobians (k_jacobian) and the cost expansion (k_expand_u on 4-lane teams,
// k_expand_team on TEAM-lane teams) read X, U, λ and μ only and none reads another's output, so in the convergence
// tail, where each is a handful of waves waiting on its own loads, they go out as one launch, k_tail_prepare. Its
// grid is three contiguous ranges of PREP_THREADS-thread blocks, [Jacobian | 4-lane teams | TEAM-lane teams]; a
// block takes its role from its index (prepare_role: uniform over the block, so every wave runs one role and the
// team code's DPP broadcasts stay within whole teams) and runs the separate kernel's body on the separate kernel's
// work item: thread t of the Jacobian range is (slot, knot, chunk) t; 4-lane team i of the second range is (slot,
// knot) i over the N - 1 stage knots; TEAM-lane team i of the third is (slot, knot) i over all N knots, or slot i's
// terminal knot in mode 2.
constexpr int PREP_THREADS = 256;
constexpr int PREP_QUADS = PREP_THREADS / 4;  // 4-lane teams of a block
enum PrepareRole { PREP_JAC = 0, PREP_QUAD = 1, PREP_TEAM = 2 };
// the role of block `blk` of a grid whose first `jac` blocks are the Jacobian's and next `quad` the 4-lane teams',
// and the block's index within its role's range
constexpr int prepare_role(unsigned blk, unsigned jac, unsigned quad) {
  return blk < jac ? PREP_JAC : (blk - jac < quad ? PREP_QUAD : PREP_TEAM);
}
constexpr unsigned prepare_block(unsigned blk, unsigned jac, unsigned quad) {
  return blk < jac ? blk : (blk - jac < quad ? blk - jac : blk - jac - quad);
}
struct TailPrepare {
  bool fused = false;                    // one k_tail_prepare launch (else the separate kernels, as in the bulk)
  unsigned jac = 0, quad = 0, team = 0;  // blocks of each range
  unsigned lds = 0;                      // dynamic LDS bytes: the TEAM-lane teams' images
  unsigned blocks() const { return jac + quad + team; }
};
// tail, bwd_team: DevBuffers::tail and the handle's team backward path; plain_jac: the model's Jacobians are one
// k_jacobian launch (not the minimum-time kernel, not the Kuka's stage chain); split: TOG_TAIL_PREPARE=split.
// width: slots of the launch; nch: Jacobian chunks per knot; team_lanes: lanes of a wide team; mode: 0 every knot on
// the wide teams (no 4-lane range), 1 the 4-lane teams and the dense knots among all N on the wide ones, 2 the
// 4-lane teams and the terminal knot alone on the wide ones (k_expand_team's mode); team_stride: doubles of one
// wide team's LDS image (expand_team_stride). A launch whose image is above SPEC_LDS_MAX, or whose grid does not
// fit 31 bits, stays split.
inline TailPrepare tail_prepare(int tail, int bwd_team, bool plain_jac, bool split, long long width, int N, int nch,
                                int team_lanes, int mode, int team_stride) {
  TailPrepare p;
  if (!tail || !bwd_team || !plain_jac || split || width <= 0 || N < 2) return p;
  const long long tpb = PREP_THREADS / team_lanes;
  const long long jt = width * (long long)(N - 1) * nch, qt = mode ? width * (long long)(N - 1) : 0;
  const long long tt = mode == 2 ? width : width * (long long)N;
  const long long jb = (jt + PREP_THREADS - 1) / PREP_THREADS, qb = (qt + PREP_QUADS - 1) / PREP_QUADS;
  const long long tb = (tt + tpb - 1) / tpb;
  const long long lds = (long long)sizeof(double) * tpb * team_stride;
  if (lds > 64 * 1024 || jb + qb + tb > 0x7fffffffLL) return p;
  p.fused = true;
  p.jac = (unsigned)jb;
  p.quad = (unsigned)qb;
  p.team = (unsigned)tb;
  p.lds = (unsigned)lds;
  return p;
}

// The speculative rollout kernels of the line search (tog_kernels.hpp) and which of them a launch takes.
// The tail kernels stage a trajectory's per-knot inputs through LDS, a chunk of spec_tail_tc knots at a time;
// one chunk image is (doubles, field-major) [K: TC·mn | ū: TC·m | d: TC·m | x: TC·n | λ: TC·p | μ: TC·p].
constexpr int SPEC_WAVE = 64;       // lanes of a wave: the trials of one k_ls_spec_tail workgroup
constexpr int SPEC_TAIL_PMAX = 16;  // larger row counts per knot take k_ls_spec
constexpr int SPEC_RQ = 4;          // k_ls_spec_tail2: steps per ring slot (and per barrier)
constexpr int SPEC_LANES = 32;      // k_ls_spec_tail2: trials per workgroup
constexpr int SPEC_LDS_MAX = 64 * 1024;  // dynamic LDS of a launch that raises no limit
constexpr int spec_tail_tc(int n, int m) { return (m * n <= 64) ? 16 : 8; }
constexpr int spec_tail_rec(int n, int m, int pmax) { return m * n + 2 * m + n + 2 * pmax; }
// k_ls_spec_tail2's layout: two staging images (each with the terminal λ, μ after it), the ring, then SPEC_LANES
// ints of wave A's verdicts (live_out), rounded up to whole doubles, then SPEC_LANES doubles of wave C's sums
constexpr int spec_tail2_ring_off(int n, int m, int pmax) {
  return 2 * (spec_tail_tc(n, m) * spec_tail_rec(n, m, pmax) + 2 * pmax);
}
constexpr int spec_tail2_doubles(int n, int m, int pmax) {
  return spec_tail2_ring_off(n, m, pmax) + 2 * SPEC_RQ * (n + m) * SPEC_LANES +
         (SPEC_LANES * (int)sizeof(int) + (int)sizeof(double) - 1) / (int)sizeof(double) + SPEC_LANES;
}
// LDS bytes of a tail kernel's launch for a problem of at most pmax rows per knot, 0 where the kernel is not
// admissible: the three-wave k_ls_spec_tail2 (DevBuffers::spec_tail2_shmem) up to SPEC_TAIL_PMAX rows and within
// SPEC_LDS_MAX, the one-wave k_ls_spec_tail (DevBuffers::spec_tail_shmem: one image) up to SPEC_TAIL_PMAX rows
inline int spec_tail2_lds(int n, int m, int pmax) {
  const size_t b = sizeof(double) * (size_t)spec_tail2_doubles(n, m, pmax);
  return (pmax <= SPEC_TAIL_PMAX && b <= (size_t)SPEC_LDS_MAX) ? (int)b : 0;
}
inline int spec_tail_lds(int n, int m, int pmax) {
  return pmax <= SPEC_TAIL_PMAX ? (int)(sizeof(double) * (spec_tail_tc(n, m) * spec_tail_rec(n, m, pmax) + 2 * pmax)) : 0;
}
// The rollout kernels that inline the diagonal cost are the shared objective's: per-trajectory costs or goals
// (tv bit 1) ride the run-time-structure variants, and so does a dense cost (its run-time indexing of x, u would
// put the tail kernels in scratch).
inline bool spec_inline_diag(int cost_diag, int tv) { return cost_diag && !(tv & 2); }
// The bulk kernel of a model with a gain block of mn entries: above 64, 64-lane workgroups at one wave per SIMD
// (k_ls_spec_w1), which spread the waves over every CU and hold the rigid-body models' live arrays in registers
constexpr bool spec_bulk_w1(int mn) { return mn > 64; }
enum SpecKernel { SPEC_TAIL3 = 0, SPEC_TAIL1 = 1, SPEC_BULK = 2, SPEC_BULK_W1 = 3 };
// The kernel of one launch of trials [lo, lo + cnt): tail, cand, cost_diag, tv as in DevBuffers; listed: a second
// round over a device list of trajectories; tail2_lds, tail_lds: spec_tail2_lds, spec_tail_lds of the problem.
// The tail kernels run whole rounds of the candidate-copy line search in the convergence tail: three waves up to
// SPEC_LANES trials, one wave up to SPEC_WAVE. Everything else is the bulk kernel's.
inline SpecKernel spec_kernel(int tail, int cand, int cost_diag, int tv, bool listed, int cnt, int tail2_lds,
                              int tail_lds, int mn) {
  const bool staged = tail && cand && spec_inline_diag(cost_diag, tv) && !listed;
  if (staged && tail2_lds > 0 && cnt <= SPEC_LANES) return SPEC_TAIL3;
  if (staged && tail_lds > 0 && cnt <= SPEC_WAVE) return SPEC_TAIL1;
  return spec_bulk_w1(mn) ? SPEC_BULK_W1 : SPEC_BULK;
}

// upper Cholesky (dpotrf 'U') of a symmetric matrix; returns false if not PD
inline bool chol_upper(const double* A, int n, double* U) {
  for (int i = 0; i < n * n; i++) U[i] = 0.0;
  for (int j = 0; j < n; j++) {
    double s = A[j + n * j];
    for (int k = 0; k < j; k++) s -= U[k + n * j] * U[k + n * j];
    if (!(s > 0.0)) return false;
    const double ujj = std::sqrt(s);
    U[j + n * j] = ujj;
    for (int c = j + 1; c < n; c++) {
      double t = A[j + n * c];
      for (int k = 0; k < j; k++) t -= U[k + n * j] * U[k + n * c];
      U[j + n * c] = t / ujj;
    }
  }
  return true;
}

// The stage cost(s) of a problem: one for every knot, or a time-varying Objective's table (rows
// [Q; R; H; q; r; c], nc_in doubles each). The device table (DevProblem::kc) adds each knot's square-root
// factors: row k is [Q; R; H; q; r; c; cQ; cR] with cQ = chol(Q dt), cR = chol(R dt), kst doubles.
struct CostPlan {
  int nc_in = 0, kst = 0, nk = 0;  // nk rows: N - 1 with a table, else 1
  int n = 0, m = 0;
  std::vector<double> kc;   // (kst, nk)
  std::vector<double> cQf;  // chol(Qf), (n, n)
  bool sqrt_ok = false;     // every Hessian is PD
  // 0 dense; 1 diagonal Q/R/Qf, H = 0; 2 = 1 with every off-diagonal entry (and H, and the factors'
  // off-diagonals) +0.0 and dt > 0, so the kernels may use literal zeros for them and stay bit-identical
  int diag_cost = 0;
  const double* Q(int k) const { return kc.data() + (size_t)k * kst; }
  const double* R(int k) const { return Q(k) + n * n; }
  const double* H(int k) const { return R(k) + m * m; }
  const double* q(int k) const { return H(k) + m * n; }
  const double* r(int k) const { return q(k) + n; }
  double c(int k) const { return Q(k)[nc_in - 1]; }
  const double* cQ(int k) const { return Q(k) + nc_in; }
  const double* cR(int k) const { return cQ(k) + n * n; }
};

// The square-root expansion's factors of one stage cost (src/objective.jl:70-94): cQ = chol(Q dt), cR = chol(R dt),
// upper. 0 when both exist, else which of them is not positive definite: 1 Q dt (cR is then left as it was: R is not
// factored after a failed Q), 2 R dt.
inline int factor_stage(int n, int m, double dt, const double* Q, const double* R, double* cQ, double* cR) {
  std::vector<double> Qdt((size_t)n * n), Rdt((size_t)m * m);
  for (int i = 0; i < n * n; i++) Qdt[i] = Q[i] * dt;
  for (int i = 0; i < m * m; i++) Rdt[i] = R[i] * dt;
  if (!chol_upper(Qdt.data(), n, cQ)) return 1;
  return chol_upper(Rdt.data(), m, cR) ? 0 : 2;
}
// The diagonal-cost class of one stage cost beside the terminal cost (CostPlan::diag_cost; a table's class, and a
// batch of per-trajectory Hessians', is the minimum over its members): 0 dense; 1 diagonal Q, R, Qf and H = 0; 2 = 1
// with every off-diagonal entry, H and (ok: when every factor exists) the factors' off-diagonals +0.0, and dt > 0.
inline int cost_class(int n, int m, double dt, const double* Q, const double* R, const double* H, const double* Qf,
                      const double* cQ, const double* cR, const double* cQf, bool ok) {
  bool diag = true;
  for (int j = 0; j < n; j++)
    for (int i = 0; i < n; i++)
      if (i != j && (Qf[i + n * j] != 0.0 || Q[i + n * j] != 0.0)) diag = false;
  for (int j = 0; j < m; j++)
    for (int i = 0; i < m; i++)
      if (i != j && R[i + m * j] != 0.0) diag = false;
  for (int i = 0; i < m * n; i++)
    if (H[i] != 0.0) diag = false;
  if (!diag) return 0;
  auto offdiag_pz = [](const double* A, int kk) {
    for (int j = 0; j < kk; j++)
      for (int i = 0; i < kk; i++)
        if (i != j && (A[i + kk * j] != 0.0 || std::signbit(A[i + kk * j]))) return false;
    return true;
  };
  bool pz = dt > 0.0 && offdiag_pz(Qf, n) && (!ok || offdiag_pz(cQf, n)) && offdiag_pz(Q, n) && offdiag_pz(R, m);
  if (pz && ok) pz = offdiag_pz(cQ, n) && offdiag_pz(cR, m);
  for (int i = 0; pz && i < m * n; i++)
    if (std::signbit(H[i])) pz = false;
  return pz ? 2 : 1;
}

// stage_costs: the (nc_in, N - 1) table, or null for the shared Q, R, H, q, r, c
inline CostPlan plan_costs(int n, int m, int N, double dt, const double* Q, const double* R, const double* H,
                           const double* q, const double* r, double c, const double* stage_costs,
                           const double* Qf) {
  CostPlan p;
  p.n = n;
  p.m = m;
  p.nc_in = n * n + m * m + m * n + n + m + 1;
  p.kst = 2 * n * n + 2 * m * m + m * n + n + m + 1;
  p.nk = stage_costs ? N - 1 : 1;
  const int nc_in = p.nc_in, nk = p.nk;
  p.kc.assign((size_t)nk * p.kst, 0.0);
  for (int k = 0; k < nk; k++) {
    double* o = p.kc.data() + (size_t)k * p.kst;
    if (stage_costs) {
      memcpy(o, stage_costs + (size_t)k * nc_in, sizeof(double) * nc_in);
    } else {
      memcpy(o, Q, sizeof(double) * n * n);
      memcpy(o + n * n, R, sizeof(double) * m * m);
      memcpy(o + n * n + m * m, H, sizeof(double) * m * n);
      memcpy(o + n * n + m * m + m * n, q, sizeof(double) * n);
      memcpy(o + n * n + m * m + m * n + n, r, sizeof(double) * m);
      o[nc_in - 1] = c;
    }
  }
  auto kcQ = [&](int k) { return p.kc.data() + (size_t)k * p.kst + nc_in; };
  auto kcR = [&](int k) { return kcQ(k) + n * n; };
  p.cQf.assign((size_t)n * n, 0.0);
  bool ok = chol_upper(Qf, n, p.cQf.data());
  for (int k = 0; k < nk; k++) ok = factor_stage(n, m, dt, p.Q(k), p.R(k), kcQ(k), kcR(k)) == 0 && ok;
  p.sqrt_ok = ok;
  p.diag_cost = 2;
  for (int k = 0; k < nk; k++)
    p.diag_cost = std::min(p.diag_cost, cost_class(n, m, dt, p.Q(k), p.R(k), p.H(k), Qf, p.cQ(k), p.cR(k),
                                                   p.cQf.data(), ok));
  return p;
}

// Packed std AL expansion records: the Q.xx entries a constraint row can change. masks: one per row, a bit per
// state index with a non-zero gradient entry. qpat[c]: a bit per row i of column c (the union over the rows of
// (state indices)^2), qoff[c] its running count, qpat_n the total, qpat_max the most entries in one column.
struct QPattern {
  std::vector<unsigned int> qpat;
  std::vector<int> qoff;
  int qpat_n = 0, qpat_max = 0;
};
inline QPattern plan_qpattern(int n, const unsigned int* masks, size_t nmasks) {
  QPattern p;
  p.qpat.assign((size_t)n, 0u);
  p.qoff.assign((size_t)n, 0);
  for (size_t r = 0; r < nmasks; r++)
    for (int c = 0; c < n; c++)
      if (masks[r] >> c & 1u) p.qpat[(size_t)c] |= masks[r];
  int off = 0;
  for (int c = 0; c < n; c++) {
    p.qoff[(size_t)c] = off;
    off += __builtin_popcount(p.qpat[(size_t)c]);
    p.qpat_max = std::max(p.qpat_max, __builtin_popcount(p.qpat[(size_t)c]));
  }
  p.qpat_n = off;
  return p;
}

}  // namespace tog_plan
