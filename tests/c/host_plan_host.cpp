// Stand-alone host check of csrc/tog_host_plan.hpp (the host arithmetic of tog_create that decides which kernel
// code runs): the run-time flag -> template constant dispatcher, the stage-cost table with its Cholesky factors
// and diagonal-cost class (class 2 promises the kernels +0.0 everywhere off the diagonal, a signed-zero rule), and
// the Q.xx pattern of the packed expansion records. Built with -fsanitize=address,undefined by
// tests/test_host_plan.py; it has no device code and needs no GPU. Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tog_host_plan.hpp"

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                               \
    }                                                        \
  } while (0)

using namespace tog_plan;

// the shared-cost problem of the diagonal cases: n = 2, m = 1, dt = 0.1, Q = diag(1, 2), R = [0.5], H = 0,
// Qf = diag(3, 4)
struct Shared {
  int n = 2, m = 1, N = 4;
  double dt = 0.1;
  std::vector<double> Q = {1.0, 0.0, 0.0, 2.0}, R = {0.5}, H = {0.0, 0.0}, q = {0.1, 0.2}, r = {0.3};
  std::vector<double> Qf = {3.0, 0.0, 0.0, 4.0};
  double c = 0.7;
  CostPlan plan() const {
    return plan_costs(n, m, N, dt, Q.data(), R.data(), H.data(), q.data(), r.data(), c, nullptr, Qf.data());
  }
};

static bool bits_pz(double v) { return v == 0.0 && !std::signbit(v); }

int main() {
  // pick: f runs once with the constant v equals, never for a value outside Vs
  for (int v = -1; v <= 4; v++) {
    int calls = 0, got = -100;
    pick<0, 1, 2, 3>(v, [&](auto c) {
      calls++;
      got = decltype(c)::value;
    });
    if (v >= 0 && v <= 3)
      CHECK(calls == 1 && got == v);
    else
      CHECK(calls == 0);
  }

  // Cholesky: U'U = A for a PD matrix (column-major, upper), false for an indefinite one
  {
    const double A[4] = {4.0, 2.0, 2.0, 3.0};
    double U[4];
    CHECK(chol_upper(A, 2, U));
    CHECK(U[0] == 2.0 && U[1] == 0.0 && U[2] == 1.0 && U[3] == std::sqrt(2.0));
    const double Bm[4] = {1.0, 2.0, 2.0, 1.0};
    CHECK(!chol_upper(Bm, 2, U));
  }

  // diagonal cost, class 2: the factors are diagonal, the square roots of the dt-scaled entries
  {
    const Shared s;
    const CostPlan p = s.plan();
    CHECK(p.nk == 1 && p.nc_in == 4 + 1 + 2 + 2 + 1 + 1 && p.kst == p.nc_in + 4 + 1);
    CHECK(p.kc.size() == (size_t)p.kst);
    CHECK(p.sqrt_ok && p.diag_cost == 2);
    CHECK(p.Q(0)[0] == 1.0 && p.Q(0)[3] == 2.0 && p.R(0)[0] == 0.5 && p.q(0)[1] == 0.2 && p.r(0)[0] == 0.3);
    CHECK(p.c(0) == 0.7);
    CHECK(p.cQ(0)[0] == std::sqrt(1.0 * s.dt) && p.cQ(0)[3] == std::sqrt(2.0 * s.dt));
    CHECK(bits_pz(p.cQ(0)[1]) && bits_pz(p.cQ(0)[2]));
    CHECK(p.cR(0)[0] == std::sqrt(0.5 * s.dt));
    CHECK(p.cQf[0] == std::sqrt(3.0) && p.cQf[3] == std::sqrt(4.0) && bits_pz(p.cQf[1]) && bits_pz(p.cQf[2]));
  }
  // signed zeros: a -0.0 off the diagonal of Q, or in H, is diagonal but not class 2; a non-zero H is dense
  {
    Shared s;
    s.Q[1] = s.Q[2] = -0.0;
    CostPlan p = s.plan();
    CHECK(p.sqrt_ok && p.diag_cost == 1);
    s = Shared();
    s.H[0] = -0.0;
    p = s.plan();
    CHECK(p.sqrt_ok && p.diag_cost == 1);
    s.H[0] = 0.25;
    p = s.plan();
    CHECK(p.diag_cost == 0);
  }
  // not positive definite
  {
    Shared s;
    s.Qf = {1.0, 2.0, 2.0, 1.0};
    CHECK(!s.plan().sqrt_ok);
  }

  // time-varying table: N = 4, three rows [Q; R; H; q; r; c] with n = 2, m = 2; row k's factors from row k
  {
    const int n = 2, m = 2, N = 4, nc_in = 4 + 4 + 4 + 2 + 2 + 1;
    const double dt = 0.5;
    std::vector<double> t((size_t)nc_in * (N - 1), 0.0);
    for (int k = 0; k < N - 1; k++) {
      double* o = t.data() + (size_t)k * nc_in;
      o[0] = 1.0 + k;  // Q = diag(1 + k, 2 + k)
      o[3] = 2.0 + k;
      o[4] = 3.0 + k;  // R = diag(3 + k, 4 + k)
      o[7] = 4.0 + k;
      o[nc_in - 1] = 10.0 + k;
    }
    const double Qf[4] = {1.0, 0.0, 0.0, 1.0};
    CostPlan p = plan_costs(n, m, N, dt, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, t.data(), Qf);
    CHECK(p.nk == N - 1 && p.kc.size() == (size_t)p.kst * (N - 1) && p.nc_in == nc_in);
    CHECK(p.sqrt_ok && p.diag_cost == 2);
    for (int k = 0; k < N - 1; k++) {
      CHECK(p.Q(k)[0] == 1.0 + k && p.R(k)[3] == 4.0 + k && p.c(k) == 10.0 + k);
      CHECK(p.cQ(k)[0] == std::sqrt((1.0 + k) * dt) && p.cQ(k)[3] == std::sqrt((2.0 + k) * dt));
      CHECK(p.cR(k)[0] == std::sqrt((3.0 + k) * dt) && p.cR(k)[3] == std::sqrt((4.0 + k) * dt));
      CHECK(bits_pz(p.cQ(k)[2]) && bits_pz(p.cR(k)[2]));
    }
    // a single off-diagonal entry in knot 2's R alone: dense
    t[(size_t)2 * nc_in + 4 + 2] = 0.5;
    CHECK(plan_costs(n, m, N, dt, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, t.data(), Qf).diag_cost == 0);
    // ... and with its mirror entry: still dense, and only row 2's factor changes
    t[(size_t)2 * nc_in + 4 + 1] = 0.5;
    const CostPlan p2 = plan_costs(n, m, N, dt, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, t.data(), Qf);
    CHECK(p2.sqrt_ok && p2.diag_cost == 0);
    CHECK(p2.cR(2)[2] == (0.5 * dt) / std::sqrt(5.0 * dt) && p2.cR(1)[2] == 0.0);
    for (int i = 0; i < 4; i++) CHECK(p2.cR(0)[i] == p.cR(0)[i] && p2.cR(1)[i] == p.cR(1)[i] && p2.cQ(2)[i] == p.cQ(2)[i]);
  }

  // Q.xx pattern: n = 4, a row on state 2 and a row on states {0, 1}
  {
    const unsigned int masks[3] = {1u << 2, 0b11u, 0b1111u};
    QPattern p = plan_qpattern(4, masks, 2);
    CHECK(p.qpat.size() == 4 && p.qpat[0] == 3u && p.qpat[1] == 3u && p.qpat[2] == 4u && p.qpat[3] == 0u);
    CHECK(p.qoff.size() == 4 && p.qoff[0] == 0 && p.qoff[1] == 2 && p.qoff[2] == 4 && p.qoff[3] == 5);
    CHECK(p.qpat_n == 5 && p.qpat_max == 2);
    p = plan_qpattern(4, masks, 3);  // a dense row added
    CHECK(p.qpat_max == 4 && p.qpat_n == 16);
    p = plan_qpattern(4, nullptr, 0);  // no rows
    CHECK(p.qpat_n == 0 && p.qpat_max == 0 && p.qpat[3] == 0u);
  }

  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
