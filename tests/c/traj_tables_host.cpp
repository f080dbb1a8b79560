// Stand-alone host check of csrc/tog_traj_tables.hpp (the host side of tog_set_trajectory_costs / _goals): the
// slices a multi-device handle hands to its parts, the goal table's expansion, the per-knot replication, the
// terminal goal row scan and the replace order of a device buffer, alone and as tog_history_enable's pair (new
// before old), with heap buffers in the place of device memory. Built with -fsanitize=address,undefined by tests/test_trajectory_goals.py; it has no
// device code and needs no GPU. Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
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

int main() {
  using namespace tog_traj;
  const int n = 4, m = 1, N = 6;
  // widths
  CHECK(lin_width(n, m, N, 0) == 6 && lin_width(n, m, N, 1) == 30 && term_width(n) == 5);

  // multi-device split: B = 5 over parts of 3 and 2, every element of every slice read to its end
  {
    const long long B = 5, off[3] = {0, 3, 5};
    for (int per_knot = 0; per_knot < 2; per_knot++) {
      const size_t w = lin_width(n, m, N, per_knot);
      std::vector<double> lin(w * B);
      for (size_t i = 0; i < lin.size(); i++) lin[i] = (double)i;
      for (int p = 0; p < 2; p++) {
        const double* s = part_slice(lin.data(), (size_t)off[p], w);
        const size_t cnt = (size_t)(off[p + 1] - off[p]) * w;
        double sum = 0.0;
        for (size_t i = 0; i < cnt; i++) sum += s[i];
        CHECK(s[0] == (double)(off[p] * w) && s[cnt - 1] == (double)(off[p + 1] * w - 1));
        CHECK(sum > 0.0);
      }
    }
    CHECK(part_slice(nullptr, 3, 7) == nullptr);
  }

  // terminal goal rows: bounds at the stage knots, goal rows on states 0, 1, 3 at the terminal knot
  {
    const int GOAL = 4;
    std::vector<int> types, idx, koff(N), kcnt(N);
    for (int k = 0; k < N - 1; k++) {
      koff[k] = (int)types.size();
      kcnt[k] = 2;
      types.push_back(1);
      idx.push_back(0);
      types.push_back(3);
      idx.push_back(0);
    }
    koff[N - 1] = (int)types.size();
    kcnt[N - 1] = 3;
    for (int i : {0, 1, 3}) {
      types.push_back(GOAL);
      idx.push_back(i);
    }
    std::vector<int> gi;
    CHECK(terminal_goal_rows(types.data(), idx.data(), koff.data(), kcnt.data(), N, n, GOAL, gi).empty());
    CHECK(gi.size() == 3 && gi[0] == 0 && gi[1] == 1 && gi[2] == 3);
    // (ng, B) -> (n, B)
    const long long B = 3;
    std::vector<double> xf(3 * B);
    for (size_t i = 0; i < xf.size(); i++) xf[i] = 10.0 + (double)i;
    const std::vector<double> t = goal_table(xf.data(), gi, n, B);
    CHECK(t.size() == (size_t)n * B);
    for (long long b = 0; b < B; b++) {
      CHECK(t[b * n + 0] == xf[b * 3 + 0] && t[b * n + 1] == xf[b * 3 + 1] && t[b * n + 3] == xf[b * 3 + 2]);
      CHECK(t[b * n + 2] == 0.0);
    }
    // no goal rows: empty list, no error
    std::vector<int> none;
    CHECK(terminal_goal_rows(types.data(), idx.data(), koff.data(), kcnt.data(), N - 1, n, GOAL, none).empty());
    CHECK(none.empty());
    // refusals: a goal row at a stage knot; two goal rows on one state; an index out of range
    types[0] = GOAL;
    CHECK(!terminal_goal_rows(types.data(), idx.data(), koff.data(), kcnt.data(), N, n, GOAL, none).empty());
    types[0] = 1;
    idx[koff[N - 1] + 1] = 0;
    CHECK(!terminal_goal_rows(types.data(), idx.data(), koff.data(), kcnt.data(), N, n, GOAL, none).empty());
    idx[koff[N - 1] + 1] = n;
    CHECK(!terminal_goal_rows(types.data(), idx.data(), koff.data(), kcnt.data(), N, n, GOAL, none).empty());
  }

  // per-knot replication of one cost row
  {
    std::vector<double> row = {1.0, 2.0, 3.0};
    const std::vector<double> t = replicate_row(row, N - 1);
    CHECK(t.size() == 3u * (N - 1));
    for (int k = 0; k < N - 1; k++) CHECK(t[3 * k] == 1.0 && t[3 * k + 2] == 3.0);
  }

  // replace order: grow, shrink, failures and drop, with the heap as the device. The old buffer is alive while
  // the new one is allocated and filled (the sanitizer sees a use after free or a leak otherwise).
  {
    int live = 0;
    double* cur_old = nullptr;
    bool old_alive_at_alloc = true;
    auto alloc = [&](size_t c) {
      if (cur_old) old_alive_at_alloc = old_alive_at_alloc && (cur_old[0] == cur_old[0]);  // reads the old buffer
      live++;
      return (double*)std::malloc(sizeof(double) * (c ? c : 1));
    };
    auto upload = [&](double* dst, const double* src, size_t c) {
      for (size_t i = 0; i < c; i++) dst[i] = src[i];
      return true;
    };
    auto release = [&](double* p) {
      live--;
      std::free(p);
    };
    double* slot = nullptr;
    std::vector<double> a(8, 1.0), b(64, 2.0), c(3, 3.0);
    CHECK(replace_buffer(&slot, a.data(), a.size(), alloc, upload, release) && slot && slot[7] == 1.0 && live == 1);
    cur_old = slot;
    CHECK(replace_buffer(&slot, b.data(), b.size(), alloc, upload, release) && slot[63] == 2.0 && live == 1);  // grow
    cur_old = slot;
    CHECK(replace_buffer(&slot, c.data(), c.size(), alloc, upload, release) && slot[2] == 3.0 && live == 1);  // shrink
    CHECK(old_alive_at_alloc);
    // a failed allocation or upload leaves the old table in place and leaks nothing
    double* keep = slot;
    cur_old = nullptr;
    CHECK(!replace_buffer(&slot, a.data(), a.size(), [&](size_t) { return (double*)nullptr; }, upload, release));
    CHECK(slot == keep && live == 1 && slot[2] == 3.0);
    CHECK(!replace_buffer(&slot, a.data(), a.size(), alloc, [&](double*, const double*, size_t) { return false; }, release));
    CHECK(slot == keep && live == 1 && slot[2] == 3.0);
    drop_buffer(&slot, release);
    CHECK(slot == nullptr && live == 0);
    drop_buffer(&slot, release);  // (null: nothing)
    CHECK(live == 0);
  }

  // a pair replaced together (tog_history_enable's grow): both new buffers before the old ones go; an allocator
  // that fails on its first call, and one that fails on its second, leave the slots and the old buffers alone and
  // leak nothing (the leak check sees a fresh buffer that was not released)
  {
    int live = 0, calls = 0, fail_at = 0;  // fail_at: the call of alloc that returns null (0: none)
    double *old_a = nullptr, *old_b = nullptr;
    bool old_alive_at_alloc = true;
    auto alloc = [&](size_t c) -> double* {
      if (old_a) old_alive_at_alloc = old_alive_at_alloc && old_a[0] == 1.0 && old_b[0] == 2.0;  // reads the old ones
      if (++calls == fail_at) return nullptr;
      live++;
      return (double*)std::malloc(sizeof(double) * (c ? c : 1));
    };
    auto release = [&](double* p) {
      live--;
      std::free(p);
    };
    double *a = nullptr, *b = nullptr;
    CHECK(replace_buffer_pair(&a, 6, &b, 8, alloc, release) && a && b && a != b && live == 2);  // first enable
    a[0] = a[5] = 1.0;
    b[0] = b[7] = 2.0;
    old_a = a;
    old_b = b;
    for (fail_at = 1; fail_at <= 2; fail_at++) {
      calls = 0;
      CHECK(!replace_buffer_pair(&a, 60, &b, 80, alloc, release));
      CHECK(a == old_a && b == old_b && live == 2 && calls == fail_at);
      CHECK(a[5] == 1.0 && b[7] == 2.0);  // the old buffers were not released
    }
    fail_at = 0;
    CHECK(replace_buffer_pair(&a, 60, &b, 80, alloc, release) && a != old_a && b != old_b && live == 2);  // grow
    CHECK(old_alive_at_alloc);
    a[59] = b[79] = 3.0;  // the new sizes
    release(a);
    release(b);
    CHECK(live == 0);
  }

  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
