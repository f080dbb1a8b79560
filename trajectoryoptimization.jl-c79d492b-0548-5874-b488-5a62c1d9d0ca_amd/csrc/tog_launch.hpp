// tog_launch.hpp — host launch table over the kernels of tog_kernels.hpp: ModelOps (one table of function
// pointers per model variant, what the runtime and the plugins share) and ModelLaunch<M>, which turns run-time
// problem flags into the kernel instantiations of model M and launches them.
#pragma once

#include "tog_kernels.hpp"
#include "tog_host_plan.hpp"

namespace tog {

using tog_plan::pick;

// The kernels' ALI template argument from the run-time flags: bit 0 the augmented-Lagrangian terms (al), bit 1
// a variant that reads cost data from tables (DevBuffers::tv). The two kernel families key bit 1 differently.
// The team and quad backward kernels read the shared Hessians from DevProblem unless bit 1 is set, so they need
// it whenever there is a per-knot table (tv bit 0: a time-varying Objective, or per-trajectory cost data beside
// the replicated shared cost). They read no constraint row: a handle whose only table is the obstacles' (tv = 2)
// keeps the shared-cost variants.
inline int ali_backward(int al, int tv) { return (al ? 1 : 0) | ((tv & 1) ? 2 : 0); }
// The expansion kernels look for the per-knot table at run time in every variant (cost_at), so their extra
// variants are only the per-trajectory ones (tv bit 1: DevProblem::lin, term, goal, obs).
inline int ali_expand(int al, int tv) { return (al ? 1 : 0) | ((tv & 2) ? 2 : 0); }

// a second stream on the handle's device and the fork/join events that overlap work on it
struct StreamPair {
  hipStream_t st2;
  hipEvent_t fork, join;
};

struct ModelOps {
  int n, m;
  int slack;  // n for an infeasible model (add_slack_controls), else 0
  int pcap;   // max constraint rows per knot of the backward kernels' LDS layout
  int has_con;  // the model defines user constraint functions (ROW_USER_*)
  int min_time; // minimum-time model (MinTime<M>): std backward pass on the LDS kernel only
  long long jws_per_lane;  // sizes DevBuffers::jws: doubles per (knot, partial of [x; u]) (0: no workspace)
  void (*slack_controls)(const DevProblem*, const DevBuffers&, long long B, int integ, hipStream_t);
  void (*cost_expansion)(const DevProblem*, const DevBuffers&, long long B, int N, int sqrt, int al, int* fail,
                         hipStream_t);
  void (*init)(const DevProblem*, const DevBuffers&, long long B, int integ, int mode, hipStream_t);
  // k_refill: init for the `count` slots of a device list, from staged x0, U and X (X null: the initial rollout)
  void (*refill)(const DevProblem*, const DevBuffers&, int count, int N, int integ, int mode, const int* list,
                 const double* x0, const double* U, const double* X, hipStream_t);
  void (*rollout_open)(const DevProblem*, const DevBuffers&, long long B, int integ, hipStream_t);
  void (*jacobian)(const DevProblem*, const DevBuffers&, long long B, int N, int integ, hipStream_t);
  void (*backward)(const DevProblem*, const DevBuffers&, long long B, int sqrt, int al, int flags, int team,
                   hipStream_t);
  // k_expand_team: the cost expansion records the team backward kernel reads (tog_bwd_team.hpp)
  void (*expand)(const DevProblem*, const DevBuffers&, long long B, int N, int pmax, int sqrt, int al, hipStream_t);
  // k_tail_prepare: jacobian and expand as one launch in the convergence tail (1), or nothing launched (0: the caller
  // launches the two); team: the handle's team backward path
  int (*tail_prepare)(const DevProblem*, const DevBuffers&, long long B, int N, int pmax, int integ, int sqrt, int al,
                      int team, hipStream_t);
  void (*forward)(const DevProblem*, const DevBuffers&, long long B, int integ, int mode, int bookkeeping,
                  const double* Jprev, double* Jout, hipStream_t, const StreamPair* sp);
  void (*cost)(const DevProblem*, const DevBuffers&, long long B, int al, int use_bar, double* J, hipStream_t);
  void (*rollout)(const DevProblem*, const DevBuffers&, long long B, int integ, double alpha, int* ok, hipStream_t);
  void (*update_constraints)(const DevProblem*, const DevBuffers&, long long B, hipStream_t);
  // projected Newton (tog_pn.hpp): phase 0 = k_pn_begin, 1 = k_pn_project, 2 = k_pn_finish, :optimal's
  // 3 = k_pn_kkt, 4 = k_pn_ls_begin, 5 = k_pn_ls_proj, 6 = k_pn_ls_end; null for
  // the infeasible (slack) models. pn_wide: the same phases with the wide kernels (blocks of 65-128 rows), a
  // workgroup per slot of W. Both return the hipError_t of raising a kernel's LDS limit (hipSuccess otherwise).
  int (*pn)(const DevProblem*, const DevBuffers&, const PNBuffers&, long long B, int integ, int phase, hipStream_t);
  int (*pn_wide)(const DevProblem*, const DevBuffers&, const PNWideBuffers&, long long slots, int integ, int phase,
                 hipStream_t);
  bool implicit;                   // TOG_RK3_IMPLICIT / TOG_MIDPOINT_IMPLICIT instantiated
  int bwd_lds_bytes;
  int team_tpw;                    // trajectories per wave of k_bwd_team
  int (*team_stride)(int pmax, int sqrt);  // per-team LDS stride of k_bwd_team (doubles)
};

template <class M>
struct ModelLaunch {
  // dual partials per thread: all of them for small models, chunks of 4 otherwise (512-register
  // budget with no scratch for the quadrotor RK4 step)
#ifndef TOG_JW
#define TOG_JW 4
#endif
  // (the Kuka RBD step keeps per-joint force and mass-matrix arrays live: one partial per thread
  // holds its scratch to ~4 KB/lane against ~12 KB with 4)
  using Mb = typename ModelTraits<M>::Base;  // the differentiated model (infeasible: without slacks)
  static constexpr int JW = (Mb::n + Mb::m) <= 6 ? (Mb::n + Mb::m + (ModelTraits<M>::min_time ? 1 : 0))
                                                 : (Mb::id == TOG_MODEL_KUKA ? 1 : TOG_JW);
  static unsigned grid(long long total, int blk) { return (unsigned)((total + blk - 1) / blk); }
  // runtime integrator -> compile-time INTEG (the implicit schemes only where instantiated; tog_create
  // rejects them elsewhere)
  template <class F>
  static void with_integ(int integ, F&& f) {
    if constexpr (!ModelTraits<M>::explicit_ok) {  // KukaImplicit: the implicit schemes only
      if (integ == TOG_RK3_IMPLICIT)
        f(std::integral_constant<int, TOG_RK3_IMPLICIT>{});
      else
        f(std::integral_constant<int, TOG_MIDPOINT_IMPLICIT>{});
      return;
    }
    if (integ == TOG_RK4) {
      f(std::integral_constant<int, TOG_RK4>{});
    } else if (integ == TOG_MIDPOINT) {
      f(std::integral_constant<int, TOG_MIDPOINT>{});
    } else if (integ == TOG_RK3_IMPLICIT || integ == TOG_MIDPOINT_IMPLICIT) {
      if constexpr (ModelTraits<M>::implicit_ok) {
        if (integ == TOG_RK3_IMPLICIT)
          f(std::integral_constant<int, TOG_RK3_IMPLICIT>{});
        else
          f(std::integral_constant<int, TOG_MIDPOINT_IMPLICIT>{});
      }
    } else {
      f(std::integral_constant<int, TOG_RK3>{});
    }
  }
  static void init(const DevProblem* P, const DevBuffers& Bf, long long B, int integ, int mode, hipStream_t st) {
    with_integ(integ, [&](auto ic) {
      constexpr int I = decltype(ic)::value;
      hipLaunchKernelGGL((k_init<M, I>), dim3(grid(B, 64)), dim3(64), 0, st, P, Bf, mode);
    });
  }
  static void refill(const DevProblem* P, const DevBuffers& Bf, int count, int N, int integ, int mode, const int* list,
                     const double* x0, const double* U, const double* X, hipStream_t st) {
    if (count <= 0) return;
    const unsigned sm = (unsigned)(N * (2 * sizeof(double) + sizeof(int)));
    with_integ(integ, [&](auto ic) {
      constexpr int I = decltype(ic)::value;
      hipLaunchKernelGGL((k_refill<M, I>), dim3((unsigned)count), dim3(64), sm, st, P, Bf, mode, list, count, x0, U, X);
    });
  }
  static void rollout_open(const DevProblem* P, const DevBuffers& Bf, long long B, int integ, hipStream_t st) {
    with_integ(integ, [&](auto ic) {
      constexpr int I = decltype(ic)::value;
      hipLaunchKernelGGL((k_rollout_open<M, I>), dim3(grid(B, 64)), dim3(64), 0, st, P, Bf);
    });
  }
  static void jacobian(const DevProblem* P, const DevBuffers& Bf, long long B, int N, int integ, hipStream_t st) {
    if constexpr (ModelTraits<M>::min_time) {
      using Mc = typename ModelTraits<M>::Core;
      constexpr int NCHT = (Mc::n + Mc::m + 1 + JW - 1) / JW;
      const long long total = B * (long long)(N - 1) * NCHT;
      with_integ(integ, [&](auto ic) {
        constexpr int I = decltype(ic)::value;
        hipLaunchKernelGGL((k_jacobian_mt<M, I, JW>), dim3(grid(total, 256)), dim3(256), 0, st, P, Bf, total);
      });
    } else if (Mb::id == TOG_MODEL_KUKA && integ == TOG_RK3 && Bf.jws) {
      if constexpr (Mb::id == TOG_MODEL_KUKA && ModelTraits<M>::explicit_ok) {  // stage-chain form (tog_kuka_jac.hpp)
        const long long total = B * (long long)(N - 1);
        hipLaunchKernelGGL((k_kuka_points<M>), dim3(grid(total, 64)), dim3(64), 0, st, P, Bf, total);
        hipLaunchKernelGGL((k_kuka_sjac<M, 0>), dim3(grid(total * 21, 256)), dim3(256), 0, st, P, Bf, total);
        hipLaunchKernelGGL((k_kuka_sjac<M, 1>), dim3(grid(total * 21, 256)), dim3(256), 0, st, P, Bf, total);
        hipLaunchKernelGGL((k_kuka_chain<M>), dim3((unsigned)total), dim3(64), 0, st, P, Bf, total);
      }
    } else {
      constexpr int NCH = (Mb::n + Mb::m + JW - 1) / JW;
      const long long total = B * (long long)(N - 1) * NCH;
      with_integ(integ, [&](auto ic) {
        constexpr int I = decltype(ic)::value;
        hipLaunchKernelGGL((k_jacobian<M, I, JW>), dim3(grid(total, 256)), dim3(256), 0, st, P, Bf, total);
      });
    }
  }
  static void backward(const DevProblem* P, const DevBuffers& Bf, long long B, int sq, int al, int flags, int team,
                       hipStream_t st) {
    if constexpr (M::m <= M::n && M::n + 1 <= 16 && !ModelTraits<M>::min_time) {
    if (team) {  // column-per-lane teams, TPW trajectories per wave (tog_bwd_team.hpp)
      constexpr int TPW = TeamCfg<M>::TPW;
      const dim3 g((unsigned)((B + TPW - 1) / TPW)), blk(64);
      DevBuffers Bl = Bf;  // layout of this variant (the S-region differs between std and sqrt)
      Bl.bwd_stride = Bf.bwd_stride2[sq ? 1 : 0];
      Bl.bwd_shmem = Bf.bwd_shmem2[sq ? 1 : 0];
      const unsigned sm = (unsigned)Bl.bwd_shmem;
      const int ali = ali_backward(al, Bf.tv);
      auto launch = [&](auto wpe_c) {
        pick<0, 1>(sq ? 1 : 0, [&](auto sq_c) {
          pick<0, 1, 2, 3>(ali, [&](auto ali_c) {
            hipLaunchKernelGGL((k_bwd_team<M, decltype(sq_c)::value, decltype(ali_c)::value, decltype(wpe_c)::value>),
                               g, blk, sm, st, P, Bl, flags);
          });
        });
      };
      // quad or the one-wave team kernel by the launch width (tog_plan::tail_backward); TOG_BWD_TAIL = "quad" or
      // "team" forces either, for A/B checks (read per launch: tests switch it within one process)
      const char* tk = getenv("TOG_BWD_TAIL");
      const bool quad = (tk && !strcmp(tk, "team"))   ? false
                        : (tk && !strcmp(tk, "quad")) ? true
                                                      : tog_plan::tail_backward(B, Bf.simds / 4) == tog_plan::TAIL_BWD_QUAD;
      if (Bf.tail && sq && TeamCfg<M>::TEAM == 16 && quad) {
        // convergence tail, square-root pass, one trajectory per workgroup: the QRs, the side work, tmp1
        // and the downdate on four waves (tog_bwd_quad.hpp)
        if constexpr (TeamCfg<M>::TEAM == 16) {
          pick<0, 1, 2, 3>(ali, [&](auto ali_c) {
            hipLaunchKernelGGL((k_bwd_quad<M, decltype(ali_c)::value>), dim3((unsigned)B), dim3(256), 0, st, P, Bf,
                               flags);
          });
        }
      } else if (Bf.tail || (B + TPW - 1) / TPW <= Bf.simds) {
        // (a batch that gives at most one wave per SIMD, e.g. config 5's 4,096 Kuka trajectories in 1,024
        // waves, gains nothing from the 2-wave register budget and would spill under it)
        launch(std::integral_constant<int, 1>{});
      } else {
        launch(std::integral_constant<int, TOG_BWD_WAVES>{});
      }
      return;
    }
    }
    // one wave per trajectory, LDS (reads a per-knot table at run time: AL is its only ALI bit)
    pick<0, 1>(sq ? 1 : 0, [&](auto sq_c) {
      pick<0, 1>(al ? 1 : 0, [&](auto al_c) {
        hipLaunchKernelGGL((k_backward<M, decltype(sq_c)::value, decltype(al_c)::value>), dim3((unsigned)B), dim3(64),
                           0, st, P, Bf, flags);
      });
    });
  }
  // Which knots k_expand_team takes (its mode argument). Square root, at most 4 controls, 16-lane teams: the knots
  // with a constant Q.xx on 4-lane teams (k_expand_u), the dense ones on k_expand_team (mode 1; only the terminal
  // knot when no stage knot has a state row, mode 2); otherwise, and with TOG_EXPAND_QUAD=0 (A/B checks), every
  // knot on k_expand_team (mode 0).
  static int expand_mode(const DevBuffers& Bf, int sq, int al) {
    if constexpr (M::m <= 4 && TeamCfg<M>::TEAM == 16) {
      const char* eq = getenv("TOG_EXPAND_QUAD");
      if (sq && !(eq && eq[0] == '0')) return (al && Bf.dense_stage_knots) ? 1 : 2;
    }
    return 0;
  }
  static void expand(const DevProblem* P, const DevBuffers& Bf, long long B, int N, int pmax, int sq, int al,
                     hipStream_t st) {
    if constexpr (M::m <= M::n && M::n + 1 <= 16 && !ModelTraits<M>::min_time) {
      constexpr int TPW = TeamCfg<M>::TPW;
      const unsigned sm = (unsigned)(sizeof(double) * TPW * expand_team_stride<M>(pmax));
      const int mode = expand_mode(Bf, sq, al);
      const int ali = ali_expand(al, Bf.tv);
      if constexpr (M::m <= 4 && TeamCfg<M>::TEAM == 16) {
        if (mode) {
          const long long qteams = B * (long long)(N - 1);
          pick<0, 1, 2, 3>(ali, [&](auto ali_c) {
            hipLaunchKernelGGL((k_expand_u<M, decltype(ali_c)::value>), dim3((unsigned)((qteams + 15) / 16)), dim3(64),
                               0, st, P, Bf);
          });
        }
      }
      const long long teams = (mode == 2) ? B : B * (long long)N;
      const dim3 g((unsigned)((teams + TPW - 1) / TPW)), blk(64);
      pick<0, 1>(sq ? 1 : 0, [&](auto sq_c) {
        pick<0, 1, 2, 3>(ali, [&](auto ali_c) {
          hipLaunchKernelGGL((k_expand_team<M, decltype(sq_c)::value, decltype(ali_c)::value>), g, blk, sm, st, P, Bf,
                             mode);
        });
      });
    }
  }
  // The Jacobians and the expansion of a tail step as one k_tail_prepare launch where tog_plan::tail_prepare says so;
  // returns 1 when it launched, 0 when the step takes jacobian() and expand(). Instantiated for the models whose
  // Jacobians are one k_jacobian launch under an explicit integrator (the Kuka's kernels, stage chain or not, live
  // on scratch that the other two roles would inherit). TOG_TAIL_PREPARE=split keeps the separate launches, for A/B
  // checks (read per launch: tests switch it within one process).
  static int tail_prepare(const DevProblem* P, const DevBuffers& Bf, long long B, int N, int pmax, int integ, int sq,
                          int al, int team, hipStream_t st) {
    if constexpr (M::m <= M::n && M::n + 1 <= 16 && !ModelTraits<M>::min_time && Mb::id != TOG_MODEL_KUKA &&
                  ModelTraits<M>::explicit_ok) {
      constexpr int NCH = (Mb::n + Mb::m + JW - 1) / JW;
      const bool plain = integ == TOG_RK3 || integ == TOG_RK4 || integ == TOG_MIDPOINT;
      const char* tp = getenv("TOG_TAIL_PREPARE");
      const int mode = expand_mode(Bf, sq, al);
      const tog_plan::TailPrepare pl = tog_plan::tail_prepare(Bf.tail, team, plain, tp && !strcmp(tp, "split"), B, N, NCH,
                                                              TeamCfg<M>::TEAM, mode, expand_team_stride<M>(pmax));
      if (!pl.fused) return 0;
      const long long jtotal = B * (long long)(N - 1) * NCH;
      const int ali = ali_expand(al, Bf.tv);
      pick<TOG_RK3, TOG_RK4, TOG_MIDPOINT>(integ, [&](auto ic) {
        pick<0, 1>(sq ? 1 : 0, [&](auto sq_c) {
          pick<0, 1, 2, 3>(ali, [&](auto ali_c) {
            hipLaunchKernelGGL(
                (k_tail_prepare<M, decltype(ic)::value, decltype(sq_c)::value, decltype(ali_c)::value, JW>),
                dim3(pl.blocks()), dim3(tog_plan::PREP_THREADS), pl.lds, st, P, Bf, jtotal, pl.jac, pl.quad, mode);
          });
        });
      });
      return 1;
    }
    return 0;
  }
  template <int INTEG>
  static void spec(const DevProblem* P, const DevBuffers& Bf, long long B, int mode, int lo, int cnt, const int* list,
                   const int* count, hipStream_t st) {
    // which kernel: tog_plan::spec_kernel (the tail kernels inline the diagonal cost only, DC = 1; dense costs and
    // per-trajectory cost data take k_ls_spec's run-time-structure variants, DC = 0)
    const bool diag = tog_plan::spec_inline_diag(Bf.cost_diag, Bf.tv);
    const tog_plan::SpecKernel kern =
        tog_plan::spec_kernel(Bf.tail, Bf.cand ? 1 : 0, Bf.cost_diag, Bf.tv, list != nullptr, cnt,
                              Bf.spec_tail2_shmem, Bf.spec_tail_shmem, M::n * M::m);
    if (kern == tog_plan::SPEC_TAIL3) {
      hipLaunchKernelGGL((k_ls_spec_tail2<M, INTEG, 1>), dim3((unsigned)B), dim3(3 * WAVE),
                         (unsigned)Bf.spec_tail2_shmem, st, P, Bf, mode, lo, cnt);
      return;
    }
    if (kern == tog_plan::SPEC_TAIL1) {
      hipLaunchKernelGGL((k_ls_spec_tail<M, INTEG, 1>), dim3((unsigned)B), dim3(WAVE), (unsigned)Bf.spec_tail_shmem, st,
                         P, Bf, mode, lo, cnt);
      return;
    }
    const unsigned gs = grid(B * (long long)cnt, 256);  // one lane per (trajectory, trial); list rounds exit early
    const unsigned rb = (mode == TOG_MODE_AL) ? (unsigned)Bf.rows_lds : 0u;
    pick<0, 1>(Bf.cand ? 1 : 0, [&](auto cand_c) {
      pick<0, 1>(rb ? 1 : 0, [&](auto lrt_c) {
        pick<0, 1>(diag ? 1 : 0, [&](auto diag_c) {
          constexpr bool CAND = decltype(cand_c)::value != 0, LRT = decltype(lrt_c)::value != 0;
          // (the candidate-copy line search is the default path: only its kernels know the diagonal cost)
          constexpr int DC = CAND ? decltype(diag_c)::value : 0;
          // SPEC_BULK_W1 (64-lane workgroups spread the waves over every CU: 5% on the Kuka's) or SPEC_BULK
          if constexpr (tog_plan::spec_bulk_w1(M::n * M::m))
            hipLaunchKernelGGL((k_ls_spec_w1<M, INTEG, CAND, LRT, DC>), dim3(grid(B * (long long)cnt, 64)), dim3(64),
                               LRT ? rb : 0u, st, P, Bf, mode, lo, cnt, list, count);
          else
            hipLaunchKernelGGL((k_ls_spec<M, INTEG, CAND, LRT, DC>), dim3(gs), dim3(256), LRT ? rb : 0u, st, P, Bf,
                               mode, lo, cnt, list, count);
        });
      });
    });
  }
  // candidate-copy line search: one or two speculative rounds, each followed by its decisions, then the
  // copy of the accepted rollouts and the bookkeeping (no replay rollout on the critical path)
  template <int INTEG>
  static void forward_cand(const DevProblem* P, const DevBuffers& Bf, long long B, int mode, int bk, const double* Jp,
                           double* Jo, hipStream_t st) {
    const int F = Bf.ls_first;
    const unsigned knots_lds = (unsigned)(Bf.nknots * (2 * sizeof(double) + sizeof(int)));
    if (F >= Bf.nc && bk && Bf.tail) {
      // TOG_LS_FINISH=split keeps the five launches below, for A/B checks (read per launch: tests switch it
      // within one process)
      const char* lf = getenv("TOG_LS_FINISH");
      if (!(lf && !strcmp(lf, "split"))) {
        spec<INTEG>(P, Bf, B, mode, 0, Bf.nc, nullptr, nullptr, st);
        const unsigned rows = (mode == TOG_MODE_AL) ? (unsigned)Bf.rows_lds : 0u;
        hipLaunchKernelGGL((k_ls_finish<M, INTEG>), dim3((unsigned)B), dim3(LS_FINISH_THREADS),
                           knots_lds > rows ? knots_lds : rows, st, P, Bf, mode, Jp, Jo);
        return;
      }
    }
    (void)hipMemsetAsync(Bf.ls_count, 0, sizeof(int) * LS_COUNT_SLOTS, st);
    if (F >= Bf.nc) {
      spec<INTEG>(P, Bf, B, mode, 0, Bf.nc, nullptr, nullptr, st);
      hipLaunchKernelGGL((k_ls_decide<M>), dim3(grid(B, 256)), dim3(256), 0, st, P, Bf, Bf.nc, bk, Jp, nullptr,
                         nullptr, nullptr, nullptr, 0);
    } else if (bk && Bf.ls_pend_ok) {
      // pending mode: one round per batch step; a trajectory the round leaves undecided continues its
      // line search in the next step's round, so no step waits on a second serial rollout chain
      spec<INTEG>(P, Bf, B, mode, 0, F, nullptr, nullptr, st);
      hipLaunchKernelGGL((k_ls_decide<M>), dim3(grid(B, 256)), dim3(256), 0, st, P, Bf, F, bk, Jp, nullptr, nullptr,
                         nullptr, nullptr, 1);
    } else {
      spec<INTEG>(P, Bf, B, mode, 0, F, nullptr, nullptr, st);
      hipLaunchKernelGGL((k_ls_decide<M>), dim3(grid(B, 256)), dim3(256), 0, st, P, Bf, F, bk, Jp, nullptr, nullptr,
                         Bf.ls_list, Bf.ls_count, 0);
      spec<INTEG>(P, Bf, B, mode, F, Bf.nc - F, Bf.ls_list, Bf.ls_count, st);
      hipLaunchKernelGGL((k_ls_decide<M>), dim3(grid(B, 256)), dim3(256), 0, st, P, Bf, Bf.nc, bk, Jp, Bf.ls_list,
                         Bf.ls_count, nullptr, nullptr, 0);
    }
    const long long tot = B * (long long)Bf.nknots * cand_q<M>();
    hipLaunchKernelGGL((k_ls_apply<M>), dim3(grid(tot, 256)), dim3(256), 0, st, P, Bf, bk);
    hipLaunchKernelGGL((k_ls_fallback<M>), dim3((unsigned)B), dim3(64),
                       (unsigned)(Bf.nknots * (2 * sizeof(double) + sizeof(int))), st, P, Bf,
                       (int)(mode == TOG_MODE_AL), Bf.ls_fb, Bf.ls_count + 2);
    hipLaunchKernelGGL((k_ls_book<M, INTEG>), dim3(grid(B, 64)), dim3(64), (unsigned)Bf.rows_lds, st, P, Bf, mode,
                       bk, Jp, Jo);
    if (bk && mode == TOG_MODE_AL) {
      const unsigned sm = (unsigned)(Bf.nknots * (2 * sizeof(double) + sizeof(int)));
      hipLaunchKernelGGL((k_al_outer<M>), dim3((unsigned)B), dim3(64), sm, st, P, Bf, mode, Bf.ls_done,
                         Bf.ls_count + 1);
    }
  }
  template <int INTEG>
  static void commit(const DevProblem* P, const DevBuffers& Bf, long long B, int mode, int bk, const double* Jp,
                     double* Jo, int phase, int hi, const int* list, const int* count, hipStream_t st) {
    hipLaunchKernelGGL((k_ls_commit<M, INTEG>), dim3(grid(B, 64)), dim3(64), (unsigned)Bf.rows_lds, st, P, Bf, mode,
                       bk, Jp, Jo, phase, hi, list, count);
  }
  template <int INTEG>
  static void forward_i(const DevProblem* P, const DevBuffers& Bf, long long B, int mode, int bk, const double* Jp,
                        double* Jo, hipStream_t st, const StreamPair* sp) {
    if (Bf.cand) {
      forward_cand<INTEG>(P, Bf, B, mode, bk, Jp, Jo, st);
      return;
    }
    // speculative line search in two rounds: trials [0, 8) for every trajectory (settles ~98% of them
    // on configs 2, 3 and 5), then [8, nc) only for the trajectories the first round left undecided
    // (k_ls_compact lists them, so the second round's waves are dense). Narrower first rounds were
    // measured slower: 8 lanes sharing one trajectory's K/X/U per load is what keeps the rollouts
    // coalesced, and the Kuka's heavy lanes need the width to fill the SIMDs.
    (void)hipMemsetAsync(Bf.ls_count, 0, sizeof(int) * LS_COUNT_SLOTS, st);
    if (sp && LS_MAX_ROUNDS == 2 && Bf.nc > LS_FIRST) {
      // the decided trajectories' commit (phase 1) overlaps the second round on a second stream;
      // both kernels are latency bound at low occupancy
      spec<INTEG>(P, Bf, B, mode, 0, LS_FIRST, nullptr, nullptr, st);
      int* list = Bf.ls_list + (size_t)B;
      int* count = Bf.ls_count + 1;
      hipLaunchKernelGGL((k_ls_compact<M>), dim3(grid(B, 256)), dim3(256), 0, st, P, Bf, LS_FIRST, bk, Jp, nullptr,
                         nullptr, list, count);
      (void)hipEventRecord(sp->fork, st);
      (void)hipStreamWaitEvent(sp->st2, sp->fork, 0);
      commit<INTEG>(P, Bf, B, mode, bk, Jp, Jo, 1, LS_FIRST, nullptr, nullptr, sp->st2);
      spec<INTEG>(P, Bf, B, mode, LS_FIRST, Bf.nc - LS_FIRST, list, count, st);
      commit<INTEG>(P, Bf, B, mode, bk, Jp, Jo, 2, LS_FIRST, list, count, st);
      (void)hipEventRecord(sp->join, sp->st2);
      (void)hipStreamWaitEvent(st, sp->join, 0);
      return;
    }
    int lo = 0, round = 0;
    const int* list = nullptr;
    const int* count = nullptr;
    while (lo < Bf.nc) {
      const int hi = (round + 1 < LS_MAX_ROUNDS) ? (lo == 0 ? LS_FIRST : 2 * lo) : Bf.nc;
      const int cnt = (hi < Bf.nc ? hi : Bf.nc) - lo;
      if (round > 0) {  // list the trajectories trials [0, lo) did not settle
        int* out = Bf.ls_list + (size_t)(round & 1) * B;
        hipLaunchKernelGGL((k_ls_compact<M>), dim3(grid(B, 256)), dim3(256), 0, st, P, Bf, lo, bk, Jp,
                           list, count, out, Bf.ls_count + round);
        list = out;
        count = Bf.ls_count + round;
      }
      spec<INTEG>(P, Bf, B, mode, lo, cnt, list, count, st);
      lo += cnt;
      round++;
    }
    commit<INTEG>(P, Bf, B, mode, bk, Jp, Jo, 0, 0, nullptr, nullptr, st);
  }
  static void forward(const DevProblem* P, const DevBuffers& Bf, long long B, int integ, int mode, int bk,
                      const double* Jp, double* Jo, hipStream_t st, const StreamPair* sp) {
    with_integ(integ, [&](auto ic) { forward_i<decltype(ic)::value>(P, Bf, B, mode, bk, Jp, Jo, st, sp); });
  }
  static void cost(const DevProblem* P, const DevBuffers& Bf, long long B, int al, int bar, double* J,
                   hipStream_t st) {
    hipLaunchKernelGGL((k_cost<M>), dim3(grid(B, 64)), dim3(64), 0, st, P, Bf, al, bar, J);
  }
  static void rollout(const DevProblem* P, const DevBuffers& Bf, long long B, int integ, double alpha, int* ok,
                      hipStream_t st) {
    with_integ(integ, [&](auto ic) {
      constexpr int I = decltype(ic)::value;
      hipLaunchKernelGGL((k_rollout<M, I>), dim3(grid(B, 64)), dim3(64), 0, st, P, Bf, alpha, ok);
    });
  }
  static void slack_controls(const DevProblem* P, const DevBuffers& Bf, long long B, int integ, hipStream_t st) {
    // (an infeasible minimum-time model takes its slacks from the infeasible problem: tog_slack_controls refuses)
    if constexpr (ModelTraits<M>::slack > 0 && !ModelTraits<M>::min_time) {
      with_integ(integ, [&](auto ic) {
        constexpr int I = decltype(ic)::value;
        hipLaunchKernelGGL((k_slack_controls<M, I>), dim3(grid(B, 64)), dim3(64), 0, st, P, Bf);
      });
    }
  }
  static void cost_expansion(const DevProblem* P, const DevBuffers& Bf, long long B, int N, int sq, int al,
                             int* fail, hipStream_t st) {
    hipLaunchKernelGGL((k_cost_expansion<M>), dim3(grid(B * (long long)N, 64)), dim3(64), 0, st, P, Bf, sq, al,
                       fail);
  }
  static void update_constraints(const DevProblem* P, const DevBuffers& Bf, long long B, hipStream_t st) {
    hipLaunchKernelGGL((k_update_constraints<M>), dim3(grid(B, 64)), dim3(64), 0, st, P, Bf);
  }
  // T = WAVE: the narrow kernels over the batch; T = PN_WIDE_THREADS: the wide ones over W's slots
  template <int INTEG, int T>
  static hipError_t pn_phase(const DevProblem* P, const DevBuffers& Bf, const PNArg<T>& W, long long B, int phase,
                             hipStream_t st) {
    // the factoring kernels' LDS is sized by the block stride (pn_lds_bytes; up to 113 KB at SM = 64; the wide
    // path's pn_lds_bytes_wide, 130 KB at SM = 128)
    const size_t lds = T == WAVE ? pn_lds_bytes(W.SM, M::n + M::m) : pn_lds_bytes_wide(W.SM);
    hipError_t rc = hipSuccess;
    auto big = [&](auto kern) {  // allow dynamic LDS above 64 KB (gfx950: 160 KB per workgroup)
      if (lds > 65536) {
        rc = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rc != hipSuccess) return;  // reported by the caller; an earlier launch's error stays where it is
      }
      hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(T), lds, st, P, Bf, W);
    };
    if (phase == 0)
      hipLaunchKernelGGL((k_pn_begin<M, INTEG, T>), dim3((unsigned)B), dim3(T), 0, st, P, Bf, W);
    else if (phase == 1)
      big(k_pn_project<M, INTEG, T>);
    else if (phase == 2)
      hipLaunchKernelGGL((k_pn_finish<M, INTEG, T>), dim3((unsigned)B), dim3(T), 0, st, P, Bf, W);
    else {  // solve_type :optimal
      if (phase == 3)
        big(k_pn_kkt<M, INTEG, T>);
      else if (phase == 4)
        big(k_pn_ls_begin<M, INTEG, T>);
      else if (phase == 5)
        big(k_pn_ls_proj<M, INTEG, T>);
      else
        big(k_pn_ls_end<M, INTEG, T>);
    }
    return rc;
  }
  static int pn(const DevProblem* P, const DevBuffers& Bf, const PNBuffers& W, long long B, int integ, int phase,
                hipStream_t st) {
    hipError_t rc = hipSuccess;
    with_integ(integ, [&](auto ic) { rc = pn_phase<decltype(ic)::value, WAVE>(P, Bf, W, B, phase, st); });
    return (int)rc;
  }
  static int pn_wide(const DevProblem* P, const DevBuffers& Bf, const PNWideBuffers& W, long long slots, int integ,
                     int phase, hipStream_t st) {
    hipError_t rc = hipSuccess;
    with_integ(integ, [&](auto ic) { rc = pn_phase<decltype(ic)::value, PN_WIDE_THREADS>(P, Bf, W, slots, phase, st); });
    return (int)rc;
  }
  static ModelOps ops() {
    ModelOps o;
    o.n = M::n;
    o.m = M::m;
    o.slack = ModelTraits<M>::slack;
    o.pcap = pcap_of<M>();
    o.has_con = HasCon<M>::value ? 1 : 0;
    o.min_time = ModelTraits<M>::min_time ? 1 : 0;
    o.jws_per_lane = (Mb::id == TOG_MODEL_KUKA && !ModelTraits<M>::min_time) ? 2LL * M::n * 2 : 0;
    o.implicit = ModelTraits<M>::implicit_ok;
    o.slack_controls = slack_controls;
    o.cost_expansion = cost_expansion;
    o.init = init;
    o.refill = refill;
    o.rollout_open = rollout_open;
    o.jacobian = jacobian;
    o.backward = backward;
    o.expand = expand;
    o.tail_prepare = tail_prepare;
    o.forward = forward;
    o.cost = cost;
    o.rollout = rollout;
    o.update_constraints = update_constraints;
    // projected Newton: every model whose [x; u] fits a wave (a lane per variable of a knot)
    if constexpr (M::n + M::m <= PN_SM_MAX) {
      o.pn = pn;
      o.pn_wide = pn_wide;
    } else {
      o.pn = nullptr;
      o.pn_wide = nullptr;
    }
    o.bwd_lds_bytes = (int)sizeof(BwdLds<M, true>);
    o.team_tpw = TeamCfg<M>::TPW;
    o.team_stride = bwd_team_stride<M>;
    return o;
  }
};

}  // namespace tog
