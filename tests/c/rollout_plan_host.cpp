// Stand-alone host check of the line-search rollout plan (csrc/tog_host_plan.hpp): tog_plan::spec_tail2_lds /
// spec_tail_lds (LDS admissibility of the tail kernels) and tog_plan::spec_kernel (the kernel one launch takes).
// Every argument is one query "tail,cand,cost_diag,tv,listed,cnt,n,m,pmax"; per query it prints
// "<tail2_lds> <tail_lds> tail3|tail1|bulk|bulk_w1" for tests/test_rollout_plan.py to compare with the documented
// verdicts. It then checks the plan's shape itself over every small (n, m, pmax, cnt) and flag combination: a tail
// kernel only in a whole round of a tail launch with candidate slots and the shared diagonal cost, within its lanes
// and with an admissible image; the three-wave image within 64 KB. Built with -fsanitize=address,undefined; no
// device code.
#include <cstdio>
#include <cstdlib>

#include "tog_host_plan.hpp"

using namespace tog_plan;

static const char* name(SpecKernel k) {
  return k == SPEC_TAIL3 ? "tail3" : k == SPEC_TAIL1 ? "tail1" : k == SPEC_BULK ? "bulk" : "bulk_w1";
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    int tail, cand, diag, tv, listed, cnt, n, m, pmax;
    if (std::sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d", &tail, &cand, &diag, &tv, &listed, &cnt, &n, &m, &pmax) != 9) {
      std::printf("bad query %s\n", argv[a]);
      return 2;
    }
    const int l2 = spec_tail2_lds(n, m, pmax), l1 = spec_tail_lds(n, m, pmax);
    std::printf("%d %d %s\n", l2, l1, name(spec_kernel(tail, cand, diag, tv, listed != 0, cnt, l2, l1, n * m)));
  }
  long fails = 0;
  for (int n = 1; n <= 16; n++)
    for (int m = 1; m <= 24; m++)
      for (int pmax = 0; pmax <= 20; pmax++) {
        const int l2 = spec_tail2_lds(n, m, pmax), l1 = spec_tail_lds(n, m, pmax);
        // the images, written out: TC knots of [K | ū | d | x | λ | μ] and the terminal λ, μ; for three waves two
        // of them, a ring of 2 x 4 steps of (x, u) for 32 lanes, 32 ints and 32 doubles
        const int tc = m * n <= 64 ? 16 : 8;
        const long img = (long)tc * (m * n + 2 * m + n + 2 * pmax) + 2 * pmax;
        const long b2 = 8 * (2 * img + 2L * 4 * (n + m) * 32 + 16 + 32);
        if (l1 != (pmax <= 16 ? 8 * img : 0)) fails++;
        if (l2 != ((pmax <= 16 && b2 <= 65536) ? b2 : 0)) fails++;
        if (l2 < 0 || l2 > 65536 || (l2 > 0 && l1 <= 0)) fails++;
        for (int flags = 0; flags < 64; flags++) {
          const int tail = flags & 1, cand = flags >> 1 & 1, diag = flags >> 2 & 1, listed = flags >> 3 & 1;
          const int tv = flags >> 4;  // 0..3
          const bool staged = tail && cand && diag && !(tv & 2) && !listed;
          for (int cnt = 1; cnt <= 64; cnt++) {
            const SpecKernel k = spec_kernel(tail, cand, diag, tv, listed != 0, cnt, l2, l1, n * m);
            const SpecKernel want = (staged && l2 > 0 && cnt <= 32)   ? SPEC_TAIL3
                                    : (staged && l1 > 0 && cnt <= 64) ? SPEC_TAIL1
                                    : (n * m > 64)                    ? SPEC_BULK_W1
                                                                      : SPEC_BULK;
            if (k != want) fails++;
          }
        }
      }
  if (fails)
    std::printf("FAIL %ld\n", fails);
  else
    std::printf("ok\n");
  return fails ? 1 : 0;
}
