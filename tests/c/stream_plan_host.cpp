// Stand-alone host check of csrc/tog_stream.hpp (the scheduling of a streamed solve: job queue, slot <-> job map,
// harvests and refills after a readback, the active-count hint, termination, and the pipelined driver loop). The
// device is scripted: a job started in a slot stays active for a random number of steps (seeds frozen), the
// readback lists the slots that hold a finished job once, exactly as k_list_finished does. Built with
// -fsanitize=address,undefined by tests/test_stream_plan.py; it has no device code and needs no GPU. Exit status 0
// and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tog_stream.hpp"

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                               \
    }                                                        \
  } while (0)

using namespace tog_stream;

// xorshift64*: the same sequence everywhere
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
  int range(int lo, int hi) { return lo + (int)(next() % (uint64_t)(hi - lo + 1)); }
};

// The scripted device. Slot state mirrors the handle's: `left` steps until the trajectory finishes (0: inactive),
// `holds` the job whose end has not been listed (-1: empty or listed), as d_slot_job.
struct ScriptDev {
  int B;
  long long J;
  Rng rng;
  int min_len, max_len;
  long long never = -1;  // this job never finishes
  std::vector<long long> left, holds, job;  // per slot
  std::vector<int> started, outputs, out_finished;  // per job
  std::vector<int> listed;  // the readback in flight
  bool rb_open = false;
  long long steps = 0, step_calls = 0, max_width = 0;
  bool hint_ok = true, refill_ok = true, gather_ok = true;

  ScriptDev(int B_, long long J_, uint64_t seed, int lo, int hi)
      : B(B_), J(J_), rng(seed), min_len(lo), max_len(hi), left((size_t)B_, 0), holds((size_t)B_, -1),
        job((size_t)B_, -1), started((size_t)J_, 0), outputs((size_t)J_, 0), out_finished((size_t)J_, 0) {}

  int active() const {
    int a = 0;
    for (long long l : left) a += l > 0;
    return a;
  }
  int refill(const std::vector<SlotJob>& r) {
    std::vector<char> seen((size_t)B, 0);
    for (const SlotJob& p : r) {
      if (p.slot < 0 || p.slot >= B || p.job < 0 || p.job >= J) {
        refill_ok = false;
        continue;
      }
      if (left[(size_t)p.slot] > 0) refill_ok = false;    // never an active slot
      if (holds[(size_t)p.slot] >= 0) refill_ok = false;  // nor one whose result was not gathered
      if (job[(size_t)p.slot] >= 0) refill_ok = false;    // (gather empties the slot)
      if (seen[(size_t)p.slot]) refill_ok = false;
      seen[(size_t)p.slot] = 1;
      started[(size_t)p.job]++;
      job[(size_t)p.slot] = holds[(size_t)p.slot] = p.job;
      left[(size_t)p.slot] = p.job == never ? (1LL << 40) : rng.range(min_len, max_len);
    }
    return 0;
  }
  int step(int n, double hint) {
    step_calls++;
    // rule 1: the hint bounds the active count, and the compacted launch (ceil(hint) slots) covers the list
    if (hint < (double)active() || hint > (double)B) hint_ok = false;
    if ((long long)hint > max_width) max_width = (long long)hint;
    for (long long& l : left)
      if (l > 0) l = l > n ? l - n : 0;
    steps += n;
    return 0;
  }
  int begin_readback() {
    CHECK(!rb_open);
    rb_open = true;
    listed.clear();
    for (int s = B - 1; s >= 0; s--)  // (any order: the device list's depends on timing)
      if (holds[(size_t)s] >= 0 && left[(size_t)s] == 0) {
        listed.push_back(s);
        holds[(size_t)s] = -1;
      }
    return 0;
  }
  int end_readback(std::vector<int>& l) {
    CHECK(rb_open);
    rb_open = false;
    l = listed;
    return 0;
  }
  int gather(const std::vector<SlotJob>& g, bool finished) {
    for (const SlotJob& p : g) {
      if (p.slot < 0 || p.slot >= B || job[(size_t)p.slot] != p.job) {
        gather_ok = false;
        continue;
      }
      if (finished != (left[(size_t)p.slot] == 0)) gather_ok = false;
      outputs[(size_t)p.job]++;
      out_finished[(size_t)p.job] += finished ? 1 : 0;
      job[(size_t)p.slot] = -1;
      if (!finished) holds[(size_t)p.slot] = -1;
    }
    return 0;
  }
  int flush() { return 0; }
};

// one scripted stream; returns the device for case-specific checks
static ScriptDev run_case(int B, long long J, uint64_t seed, int lo, int hi, long long max_steps, long long never = -1) {
  Planner p(J, B);
  ScriptDev dev(B, J, seed, lo, hi);
  dev.never = never;
  const int rc = run(p, dev, 4, max_steps);
  CHECK(rc == 0);
  CHECK(dev.hint_ok);
  CHECK(dev.refill_ok);
  CHECK(dev.gather_ok);
  CHECK(!dev.rb_open);  // no readback is left in flight
  CHECK(p.running() == 0);
  CHECK(p.output() == p.started());
  long long nstarted = 0, nfin = 0;
  for (long long j = 0; j < J; j++) {
    CHECK(dev.started[(size_t)j] <= 1);
    CHECK(dev.outputs[(size_t)j] == dev.started[(size_t)j]);  // output exactly once, never without a start
    nstarted += dev.started[(size_t)j];
    nfin += dev.out_finished[(size_t)j];
    if (j > 0) CHECK(dev.started[(size_t)j] <= dev.started[(size_t)j - 1]);  // the queue is served in order
  }
  CHECK(nstarted == p.started());
  CHECK(nfin == p.finished());
  if (max_steps <= 0) {  // termination: every job done
    CHECK(nstarted == J);
    CHECK(p.finished() == J);
    CHECK(p.done());
  } else {
    CHECK(dev.steps <= max_steps);
  }
  return dev;
}

int main() {
  // J < B, J = B, J = 3B + 5, J = 0, over several frozen seeds and spreads of finish times
  for (uint64_t seed = 1; seed <= 12; seed++) {
    run_case(8, 5, seed, 1, 40, 0);
    run_case(8, 8, seed, 1, 40, 0);
    run_case(8, 3 * 8 + 5, seed, 1, 40, 0);
    run_case(4, 13, seed, 3, 90, 0);
    run_case(64, 3 * 64 + 5, seed, 1, 200, 0);
    run_case(1, 7, seed, 1, 9, 0);
  }
  {
    ScriptDev d = run_case(8, 0, 1, 1, 40, 0);
    CHECK(d.step_calls == 0);
  }
  {  // J < B: the launch hint never exceeds the jobs there are
    ScriptDev d = run_case(8, 5, 3, 1, 40, 0);
    CHECK(d.max_width <= 5);
  }
  // every slot finishes within one readback (all jobs last one step)
  run_case(8, 29, 5, 1, 1, 0);
  run_case(8, 8, 5, 1, 1, 0);
  // a budget: steps never exceed it, the unfinished are output as they stand, the rest never start
  for (uint64_t seed = 1; seed <= 6; seed++) {
    ScriptDev d = run_case(8, 29, seed, 5, 60, 8);
    CHECK(d.steps == 8);
    run_case(8, 29, seed, 5, 60, 3);
    run_case(8, 29, seed, 5, 60, 13);
  }
  {  // one slot never finishes until max_steps: the other jobs all stream past it
    const long long J = 29;
    ScriptDev d = run_case(8, J, 7, 1, 6, 400, /*never=*/2);
    CHECK(d.steps == 400);
    for (long long j = 0; j < J; j++) {
      CHECK(d.outputs[(size_t)j] == 1);
      CHECK(d.out_finished[(size_t)j] == (j == 2 ? 0 : 1));
    }
  }
  {  // the planner refuses a readback it cannot have: a slot out of range, an empty slot, a slot listed twice
    Planner p(10, 4);
    std::vector<SlotJob> out;
    const std::vector<SlotJob> r = p.refill();
    CHECK(r.size() == 4 && p.running() == 4 && p.active_hint() == 4.0);
    int bad1[] = {4};
    CHECK(!p.harvest(bad1, 1, out) && !p.error().empty());
    int twice[] = {1, 1};
    CHECK(!p.harvest(twice, 2, out));
    int again[] = {1};
    CHECK(!p.harvest(again, 1, out));  // slot 1 was emptied by the call above
    int ok[] = {0, 3};
    CHECK(p.harvest(ok, 2, out) && out.size() == 2 && out[0].job == 0 && out[1].job == 3);
    CHECK(p.running() == 1 && p.active_hint() == 1.0);
    const std::vector<SlotJob> r2 = p.refill();  // slots 0, 1, 3 are empty: jobs 4, 5, 6
    CHECK(r2.size() == 3 && r2[0].slot == 0 && r2[0].job == 4 && r2[2].slot == 3 && r2[2].job == 6);
    CHECK(p.active_hint() == 4.0 && !p.done());
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
