// Host scheduling of a streamed solve (tog_solve_stream, include/tog.h): J jobs through the B trajectory slots of
// one handle. A slot whose trajectory finished is harvested (its result gathered) and given the next queued job
// while the other slots keep iterating. Here live the job queue, the slot <-> job map, which slots a readback
// harvests and refills, the active-count hint of the next solve step and termination; `run` is the pipelined
// driver loop over an abstract device. Plain C++ with no device runtime in it, so that a stand-alone program can
// drive it with a scripted device under the host sanitizers (tests/c/stream_plan_host.cpp).
//
// Two rules:
//   1. The hint handed to a solve step is never below the number of trajectories active at that step: it is the
//      number of slots that hold a job the host has not seen finished. A refill raises it by the slots refilled
//      (the step's compacted launch covers ceil(hint) slots of a list that is rebuilt per step call), so refills
//      happen only between step calls.
//   2. A slot is refilled only after its result has been gathered (harvest empties it, refill takes empty slots
//      only), and every job is output exactly once.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

namespace tog_stream {

struct SlotJob {
  int slot;
  long long job;
};

class Planner {
 public:
  Planner(long long njobs, int nslots)
      : J_(njobs > 0 ? njobs : 0), job_of_((size_t)(nslots > 0 ? nslots : 0), -1LL) {}

  int slots() const { return (int)job_of_.size(); }
  long long jobs() const { return J_; }
  long long started() const { return next_; }    // jobs handed to a slot so far
  long long finished() const { return fin_; }    // jobs harvested after they finished
  long long output() const { return out_; }      // jobs harvested at all (finished, or drained as they stand)
  int running() const { return running_; }       // slots holding a job that is not harvested
  long long job_of(int slot) const { return job_of_[(size_t)slot]; }
  const std::string& error() const { return err_; }

  // rule 1: an upper bound of the trajectories active at the next step
  double active_hint() const { return (double)running_; }
  // nothing runs and nothing is queued
  bool done() const { return running_ == 0 && next_ >= J_; }

  // The finished slots a readback listed -> the (slot, job) pairs to gather; the slots are empty afterwards.
  // False (with error()) when a listed slot is out of range, holds no job, or is listed twice.
  bool harvest(const int* list, int count, std::vector<SlotJob>& out) {
    out.clear();
    if (count < 0 || count > slots()) return fail("readback lists " + std::to_string(count) + " slots of " + std::to_string(slots()));
    for (int i = 0; i < count; i++) {
      const int s = list[i];
      if (s < 0 || s >= slots()) return fail("readback lists slot " + std::to_string(s) + " out of range");
      if (job_of_[(size_t)s] < 0) return fail("readback lists slot " + std::to_string(s) + ", which holds no job (or twice)");
      out.push_back({s, job_of_[(size_t)s]});
      job_of_[(size_t)s] = -1;
      running_--;
      fin_++;
      out_++;
    }
    return true;
  }

  // rule 2: the queue's next jobs for the empty slots, lowest slot first (the first call fills slots 0 .. min(J, B))
  std::vector<SlotJob> refill() {
    std::vector<SlotJob> r;
    for (int s = 0; s < slots() && next_ < J_; s++) {
      if (job_of_[(size_t)s] >= 0) continue;
      job_of_[(size_t)s] = next_;
      r.push_back({s, next_});
      next_++;
      running_++;
    }
    return r;
  }

  // the step budget ran out: the jobs still in their slots, to be output as they stand
  std::vector<SlotJob> drain() {
    std::vector<SlotJob> r;
    for (int s = 0; s < slots(); s++) {
      if (job_of_[(size_t)s] < 0) continue;
      r.push_back({s, job_of_[(size_t)s]});
      job_of_[(size_t)s] = -1;
      running_--;
      out_++;
    }
    return r;
  }

 private:
  bool fail(const std::string& m) {
    err_ = m;
    return false;
  }
  long long J_, next_ = 0, fin_ = 0, out_ = 0;
  int running_ = 0;
  std::vector<long long> job_of_;  // slot -> job, -1 = empty
  std::string err_;
};

// The driver loop. Dev is the device (every call returns 0 or an error code, which ends the run):
//   refill(pairs)           start the jobs in their slots (stream-ordered after everything before it)
//   step(nsteps, hint)      nsteps solve steps of the active trajectories; hint as above
//   begin_readback()        enqueue the list of the slots that finished and were not listed before
//   end_readback(list)      wait for that list only
//   gather(pairs, finished) enqueue the gather of the slots' results, to be output under their jobs
//   flush()                 wait until every gathered result is output
// The stopping check is pipelined as in tog_solve: the next chunk of steps is enqueued before the host waits for
// the previous chunk's readback, so the device does not idle on the host. A finished slot stays finished, so a
// slot that finishes during a chunk is listed by that chunk's readback and refilled after the chunk that follows.
// max_steps <= 0: no bound. Returns 0, the device's error code, or -1 for a readback the planner refuses
// (Planner::error()).
template <class Dev>
int run(Planner& p, Dev& dev, int chunk, long long max_steps) {
  int rc;
  std::vector<int> fin;
  std::vector<SlotJob> out;
  const std::vector<SlotJob> first = p.refill();
  if (first.empty()) return 0;  // no job
  if ((rc = dev.refill(first))) return rc;
  long long steps = 0;
  auto take = [&]() { return max_steps > 0 ? std::min<long long>(chunk, max_steps - steps) : (long long)chunk; };
  long long n = take();
  if ((rc = dev.step((int)n, p.active_hint()))) return rc;
  steps += n;
  if ((rc = dev.begin_readback())) return rc;
  while (true) {
    const long long next = take();
    if (next > 0) {
      if ((rc = dev.step((int)next, p.active_hint()))) return rc;
      steps += next;
    }
    if ((rc = dev.end_readback(fin))) return rc;  // the chunk before `next`
    if (!p.harvest(fin.data(), (int)fin.size(), out)) return -1;
    if (!out.empty() && (rc = dev.gather(out, true))) return rc;
    if (next == 0) break;  // the budget is spent
    const std::vector<SlotJob> r = p.refill();
    if (!r.empty() && (rc = dev.refill(r))) return rc;
    if (p.done()) break;
    if ((rc = dev.begin_readback())) return rc;
  }
  if (p.running() > 0) {  // out of budget: the unfinished jobs as they stand
    out = p.drain();
    if ((rc = dev.gather(out, false))) return rc;
  }
  return dev.flush();
}

}  // namespace tog_stream
