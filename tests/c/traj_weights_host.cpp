// Stand-alone host check of the weight part of csrc/tog_traj_tables.hpp (the host side of
// tog_set_trajectory_weights): the widths, the device image [Q; R; H; cQ; cR; Qf; cQf] of every trajectory against a
// direct tog_plan::plan_costs of that member alone, the batch's sqrt_ok (the AND) and diagonal-cost class (the
// minimum, the mixed batch included), the argument checks and the plan's positive-definiteness finding with their
// texts, the slices a multi-device handle hands to its parts, and replace_buffer under an injected allocation failure. Built with -fsanitize=address,undefined by
// tests/test_trajectory_weights.py; it has no device code and needs no GPU. Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "tog_traj_tables.hpp"

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                               \
    }                                                        \
  } while (0)

static const int n = 3, m = 2;
static const double dt = 0.1;

// one trajectory's block [Q; R; H; Qf]: dense = 0 a positive diagonal with +0.0 elsewhere, 1 symmetric positive
// definite with off-diagonals and H != 0, 2 a diagonal whose Q has a -0.0 off-diagonal entry (class 1, not 2)
static std::vector<double> member(int seed, int dense) {
  std::vector<double> w(tog_traj::weights_width(n, m), 0.0);
  double* Q = w.data();
  double* R = Q + n * n;
  double* H = R + m * m;
  double* Qf = H + m * n;
  for (int i = 0; i < n; i++) {
    Q[i + n * i] = 1.0 + 0.25 * i + 0.01 * seed;
    Qf[i + n * i] = 50.0 + i + seed;
  }
  for (int i = 0; i < m; i++) R[i + m * i] = 0.5 + 0.125 * i + 0.02 * seed;
  if (dense == 1) {
    Q[0 + n * 1] = Q[1 + n * 0] = 0.125;
    Qf[1 + n * 2] = Qf[2 + n * 1] = -2.0;
    R[0 + m * 1] = R[1 + m * 0] = 0.0625;
    for (int i = 0; i < m * n; i++) H[i] = 0.01 * (i + 1);
  }
  if (dense == 2) Q[0 + n * 2] = Q[2 + n * 0] = -0.0;
  return w;
}

static std::vector<double> batch(const std::vector<std::vector<double>>& ms) {
  std::vector<double> W;
  for (const auto& w : ms) W.insert(W.end(), w.begin(), w.end());
  return W;
}

// the image of trajectory b against plan_costs run on that member alone, bit for bit
static void check_member(const tog_traj::WeightPlan& p, long long b, const std::vector<double>& w) {
  const tog_traj::HessLayout L(n, m);
  const double* Q = w.data();
  const double* R = Q + n * n;
  const double* H = R + m * m;
  const double* Qf = H + m * n;
  const double zq[n] = {0, 0, 0}, zr[m] = {0, 0};
  const tog_plan::CostPlan cp = tog_plan::plan_costs(n, m, 5, dt, Q, R, H, zq, zr, 0.0, nullptr, Qf);
  const double* o = p.image.data() + (size_t)b * L.nh;
  CHECK(!memcmp(o, cp.Q(0), sizeof(double) * n * n));
  CHECK(!memcmp(o + L.R, cp.R(0), sizeof(double) * m * m));
  CHECK(!memcmp(o + L.H, cp.H(0), sizeof(double) * m * n));
  CHECK(!memcmp(o + L.cQ, cp.cQ(0), sizeof(double) * n * n));
  CHECK(!memcmp(o + L.cR, cp.cR(0), sizeof(double) * m * m));
  CHECK(!memcmp(o + L.Qf, Qf, sizeof(double) * n * n));
  CHECK(!memcmp(o + L.cQf, cp.cQf.data(), sizeof(double) * n * n));
}

static int class_of(const std::vector<double>& w) {
  const double* Q = w.data();
  const double* R = Q + n * n;
  const double* H = R + m * m;
  const double* Qf = H + m * n;
  const double zq[n] = {0, 0, 0}, zr[m] = {0, 0};
  return tog_plan::plan_costs(n, m, 5, dt, Q, R, H, zq, zr, 0.0, nullptr, Qf).diag_cost;
}

// the setter's checks in its order: finite and symmetric, then (a square-root handle) the plan's factors
static std::string check(const double* W, long long B, bool need_pd) {
  std::string e = tog_traj::weight_table_check(W, n, m, B);
  if (e.empty() && need_pd) e = tog_traj::weight_pd_text(tog_traj::weight_plan(W, n, m, dt, B));
  return e;
}

int main() {
  using namespace tog_traj;
  const size_t nw = weights_width(n, m), nh = hess_width(n, m);
  CHECK(nw == 2 * 9 + 4 + 6 && nh == 4 * 9 + 2 * 4 + 6);
  {
    const HessLayout L(n, m);
    CHECK(L.R == 9 && L.H == 13 && L.cQ == 19 && L.cR == 28 && L.Qf == 32 && L.cQf == 41 && L.nh == (int)nh);
    CHECK(weights_width(13, 4) == 2 * 169 + 16 + 52 && hess_width(13, 4) == 4 * 169 + 32 + 52);
  }
  // the classes of the three kinds of member, by plan_costs' own rule
  CHECK(class_of(member(0, 0)) == 2 && class_of(member(0, 1)) == 0 && class_of(member(0, 2)) == 1);

  // the image: every member against plan_costs of that member alone; the class is the minimum, sqrt_ok the AND
  {
    const std::vector<std::vector<double>> ms = {member(0, 0), member(1, 0), member(2, 0), member(3, 0), member(4, 0)};
    const std::vector<double> W = batch(ms);
    CHECK(check(W.data(), 5, true).empty());
    const WeightPlan p = weight_plan(W.data(), n, m, dt, 5);
    CHECK(p.image.size() == nh * 5 && p.sqrt_ok && p.diag_cost == 2);
    for (long long b = 0; b < 5; b++) check_member(p, b, ms[(size_t)b]);
  }
  {  // the mixed batch: trajectory 0 diagonal, trajectory 1 dense: the batch is dense
    const std::vector<std::vector<double>> ms = {member(0, 0), member(1, 1)};
    const std::vector<double> W = batch(ms);
    CHECK(check(W.data(), 2, true).empty());
    const WeightPlan p = weight_plan(W.data(), n, m, dt, 2);
    CHECK(p.diag_cost == 0 && p.sqrt_ok);
    check_member(p, 0, ms[0]);
    check_member(p, 1, ms[1]);
    // and the other way round, and a -0.0 member among literal-zero ones: class 1
    const std::vector<double> W2 = batch({member(1, 1), member(0, 0)});
    CHECK(weight_plan(W2.data(), n, m, dt, 2).diag_cost == 0);
    const std::vector<double> W3 = batch({member(0, 0), member(1, 0), member(2, 2)});
    CHECK(weight_plan(W3.data(), n, m, dt, 3).diag_cost == 1);
    const std::vector<double> W4 = batch({member(0, 2), member(1, 1)});
    CHECK(weight_plan(W4.data(), n, m, dt, 2).diag_cost == 0);
  }
  {  // dt = 0: class 1 at the most (plan_costs' rule), and the factors of Q dt fail
    const std::vector<double> W = batch({member(0, 0)});
    const WeightPlan p = weight_plan(W.data(), n, m, 0.0, 1);
    CHECK(p.diag_cost == 1 && !p.sqrt_ok);
  }

  // the argument checks: the trajectory and the matrix are named; a refused table is told apart from a good one
  {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<std::vector<double>> ms = {member(0, 1), member(1, 1), member(2, 1)};
    std::vector<double> W = batch(ms);
    CHECK(check(W.data(), 3, false).empty());
    W[2 * nw + 9 + 1] = std::nan("");  // R of trajectory 2
    std::string e = check(W.data(), 3, false);
    CHECK(e == "tog_set_trajectory_weights: trajectory 2: R has a NaN or an infinite entry");
    W = batch(ms);
    W[1 * nw + 13 + 5] = -inf;  // the last entry of H of trajectory 1
    e = check(W.data(), 3, false);
    CHECK(e == "tog_set_trajectory_weights: trajectory 1: H has a NaN or an infinite entry");
    W = batch(ms);
    W[3 * nw - 1] = inf;  // the very last entry: Qf of trajectory 2
    CHECK(check(W.data(), 3, false).find("trajectory 2: Qf has a NaN") != std::string::npos);
    W = batch(ms);
    W[0] = std::nan("");
    CHECK(check(W.data(), 3, false).find("trajectory 0: Q has a NaN") != std::string::npos);
    // symmetry of Q, R, Qf (H is m x n: any values)
    W = batch(ms);
    W[1 * nw + 0 + 3 * 1] += 1e-9;  // Q(0, 1) of trajectory 1
    CHECK(check(W.data(), 3, false) == "tog_set_trajectory_weights: trajectory 1: Q is not symmetric");
    W = batch(ms);
    W[2 * nw + 9 + 2] = 0.5;  // R(0, 1) of trajectory 2
    CHECK(check(W.data(), 3, false) == "tog_set_trajectory_weights: trajectory 2: R is not symmetric");
    W = batch(ms);
    W[0 * nw + 19 + 2 + 3 * 0] = 7.0;  // Qf(2, 0) of trajectory 0
    CHECK(check(W.data(), 3, false) == "tog_set_trajectory_weights: trajectory 0: Qf is not symmetric");
    // positive definiteness, asked of a square-root handle only
    W = batch(ms);
    W[1 * nw + 0] = -1.0;  // Q(0, 0) of trajectory 1
    CHECK(check(W.data(), 3, false).empty());
    e = check(W.data(), 3, true);
    CHECK(e.find("trajectory 1: Q is not positive definite") != std::string::npos);
    CHECK(!weight_plan(W.data(), n, m, dt, 3).sqrt_ok);
    W = batch(ms);
    W[2 * nw + 9 + 3] = 0.0;  // R(1, 1) of trajectory 2: semi-definite
    CHECK(check(W.data(), 3, true).find("trajectory 2: R is not positive definite") != std::string::npos);
    W = batch(ms);
    W[0 * nw + 19 + 8] = -3.0;  // Qf(2, 2) of trajectory 0
    CHECK(check(W.data(), 3, true).find("trajectory 0: Qf is not positive definite") != std::string::npos);

    // multi-device split: B = 3 over parts of 2 and 1, each slice read to its end
    W = batch(ms);
    const double* s1 = part_slice(W.data(), 2, nw);
    CHECK(s1 == W.data() + 2 * nw && part_slice(nullptr, 2, nw) == nullptr);
    CHECK(check(part_slice(W.data(), 0, nw), 2, true).empty());
    CHECK(check(s1, 1, true).empty());
    const WeightPlan whole = weight_plan(W.data(), n, m, dt, 3), tail = weight_plan(s1, n, m, dt, 1);
    CHECK(!memcmp(whole.image.data() + 2 * nh, tail.image.data(), sizeof(double) * nh));
    W[2 * nw + 4] = std::nan("");  // seen by the second part as its trajectory 0
    CHECK(check(s1, 1, false).find("trajectory 0: Q has a NaN") != std::string::npos);
    CHECK(check(W.data(), 3, false).find("trajectory 2: Q has a NaN") != std::string::npos);
  }

  // the refusal texts
  CHECK(weights_varying_text().find("time-varying stage_costs table") != std::string::npos);
  {
    const std::string s = weights_set_text("tog_refill_tables");
    CHECK(s.rfind("tog_refill_tables: per-trajectory cost weights are set", 0) == 0);
    CHECK(s.find("tog_set_trajectory_weights(h, NULL)") != std::string::npos);
  }

  // replace_buffer with the image: an allocation failure, and a failed upload, leave the table in place
  {
    const std::vector<double> W = batch({member(0, 0), member(1, 1)});
    const WeightPlan p = weight_plan(W.data(), n, m, dt, 2);
    int live = 0;
    bool fail_alloc = false, fail_upload = false;
    auto alloc = [&](size_t c) -> double* {
      if (fail_alloc) return nullptr;
      live++;
      return static_cast<double*>(std::malloc(sizeof(double) * c));
    };
    auto upload = [&](double* dst, const double* src, size_t c) {
      if (fail_upload) return false;
      std::memcpy(dst, src, sizeof(double) * c);
      return true;
    };
    auto release = [&](double* q) {
      live--;
      std::free(q);
    };
    double* slot = nullptr;
    CHECK(replace_buffer(&slot, p.image.data(), p.image.size(), alloc, upload, release) && slot && live == 1);
    CHECK(!memcmp(slot, p.image.data(), sizeof(double) * p.image.size()));
    double* before = slot;
    fail_alloc = true;
    CHECK(!replace_buffer(&slot, p.image.data(), p.image.size(), alloc, upload, release) && slot == before && live == 1);
    fail_alloc = false;
    fail_upload = true;
    CHECK(!replace_buffer(&slot, p.image.data(), p.image.size(), alloc, upload, release) && slot == before && live == 1);
    fail_upload = false;
    CHECK(replace_buffer(&slot, p.image.data(), p.image.size(), alloc, upload, release) && slot && live == 1);
    drop_buffer(&slot, release);
    CHECK(slot == nullptr && live == 0);
  }

  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
