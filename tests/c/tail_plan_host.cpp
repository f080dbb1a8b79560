// Stand-alone host check of tog_plan::tail_backward (csrc/tog_host_plan.hpp): which square-root backward kernel a
// convergence-tail launch of a given width takes on a device of a given CU count. Prints one line
// "<cus> <width> quad|team" per case for tests/test_tail_plan.py to compare with the documented verdicts, and
// checks the function's shape itself: one switch from quad to team as the width grows, team for a device
// without a CU count, no overflow at the largest widths. Built with -fsanitize=address,undefined; no device code.
#include <climits>
#include <cstdio>

#include "tog_host_plan.hpp"

using namespace tog_plan;

int main() {
  int fails = 0;
  for (int cus : {256, 304}) {
    const long long widths[] = {1, cus, cus + 1, 2LL * cus, 2LL * cus + 1, 2048};
    for (long long w : widths) std::printf("%d %lld %s\n", cus, w, tail_backward(w, cus) == TAIL_BWD_QUAD ? "quad" : "team");
    int switches = 0;
    for (long long w = 1; w < 4096; w++) switches += tail_backward(w, cus) != tail_backward(w + 1, cus);
    if (switches != 1 || tail_backward(1, cus) != TAIL_BWD_QUAD || tail_backward(4096, cus) != TAIL_BWD_TEAM) fails++;
  }
  if (tail_backward(1, 0) != TAIL_BWD_TEAM) fails++;
  if (tail_backward(LLONG_MAX, INT_MAX) != TAIL_BWD_TEAM) fails++;
  if (tail_backward(INT_MAX, INT_MAX) != TAIL_BWD_QUAD) fails++;
  std::printf(fails ? "FAIL\n" : "ok\n");
  return fails ? 1 : 0;
}
