// Stand-alone host check of the tail step's fused preparation launch (csrc/tog_host_plan.hpp): tog_plan::tail_prepare
// (whether a step's Jacobians and cost expansion go out as one k_tail_prepare launch, and the three contiguous block
// ranges of its grid) and tog_plan::prepare_role (the role a block takes from its index, the kernel's own arithmetic).
// Every argument is one query "tail,team,plain,split,width,N,nch,lanes,mode,stride"; per query it prints
// "fused|split <jac> <quad> <team> <lds>" for tests/test_prepare_plan.py to compare with verdicts worked out by hand.
// It then checks the plan's shape itself over small widths, horizons and every flag combination: each role's range
// covers its work items with less than one block to spare, the ranges tile the grid in order, and prepare_role puts
// every block of the grid in the range the plan gave it. Built with -fsanitize=address,undefined; no device code.
#include <cstdio>
#include <cstdlib>

#include "tog_host_plan.hpp"

using namespace tog_plan;

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    int tail, team, plain, split, N, nch, lanes, mode, stride;
    long long width;
    if (std::sscanf(argv[a], "%d,%d,%d,%d,%lld,%d,%d,%d,%d,%d", &tail, &team, &plain, &split, &width, &N, &nch, &lanes,
                    &mode, &stride) != 10) {
      std::printf("bad query %s\n", argv[a]);
      return 2;
    }
    const TailPrepare p = tail_prepare(tail, team, plain != 0, split != 0, width, N, nch, lanes, mode, stride);
    std::printf("%s %u %u %u %u\n", p.fused ? "fused" : "split", p.jac, p.quad, p.team, p.lds);
  }
  long fails = 0;
  for (long long width = 1; width <= 70; width++)
    for (int N = 2; N <= 19; N++)
      for (int nch = 1; nch <= 5; nch += 2)
        for (int lanes = 8; lanes <= 16; lanes += 8)
          for (int mode = 0; mode <= 2; mode++)
            for (int flags = 0; flags < 16; flags++) {
              const int tail = flags & 1, team = flags >> 1 & 1, plain = flags >> 2 & 1, split = flags >> 3 & 1;
              const int stride = 210;
              const TailPrepare p = tail_prepare(tail, team, plain != 0, split != 0, width, N, nch, lanes, mode, stride);
              if (p.fused != (tail && team && plain && !split)) fails++;
              if (!p.fused) {
                if (p.jac || p.quad || p.team || p.lds) fails++;
                continue;
              }
              const long long jt = width * (N - 1) * nch, qt = mode ? width * (N - 1) : 0;
              const long long tt = mode == 2 ? width : width * N, tpb = PREP_THREADS / lanes;
              if ((long long)p.jac * PREP_THREADS < jt || ((long long)p.jac - 1) * PREP_THREADS >= jt) fails++;
              if ((long long)p.quad * PREP_QUADS < qt || (qt > 0 && ((long long)p.quad - 1) * PREP_QUADS >= qt)) fails++;
              if (qt == 0 && p.quad != 0) fails++;
              if ((long long)p.team * tpb < tt || ((long long)p.team - 1) * tpb >= tt) fails++;
              if (p.lds != 8u * (unsigned)(tpb * stride)) fails++;
              if (p.blocks() != p.jac + p.quad + p.team) fails++;
              for (unsigned blk = 0; blk < p.blocks(); blk++) {
                const int role = prepare_role(blk, p.jac, p.quad);
                const int want = blk < p.jac ? PREP_JAC : blk < p.jac + p.quad ? PREP_QUAD : PREP_TEAM;
                if (role != want) fails++;
                const unsigned first = role == PREP_JAC ? 0u : role == PREP_QUAD ? p.jac : p.jac + p.quad;
                if (prepare_block(blk, p.jac, p.quad) != blk - first) fails++;
              }
            }
  // a team image above the launch's LDS limit, and a grid beyond 2^31 - 1 blocks: split
  if (tail_prepare(1, 1, true, false, 4, 11, 5, 16, 2, 600).fused) fails++;  // 16 x 600 x 8 = 76,800 bytes
  if (!tail_prepare(1, 1, true, false, 4, 11, 5, 16, 2, 512).fused) fails++;  // 65,536 bytes: the limit itself
  if (tail_prepare(1, 1, true, false, 1LL << 40, 101, 5, 16, 2, 210).fused) fails++;
  if (fails)
    std::printf("FAIL %ld\n", fails);
  else
    std::printf("ok\n");
  return fails ? 1 : 0;
}
