// stmpc_host.hpp -- what the three host units share: the error string and the status macros, device buffers and staging, the argument checks,
// struct stmpc_ctx, and the few functions one unit calls in another (the sections "defined in <unit>" at the end).  The units:
//   stmpc.hip          the context and the host helpers; the controllers on top of the solver (finer fit, st_control, no-jerk grid, combined
//                      controller, policy features and actor, first-step shield); the episode world, the vector env, the flight recorder
//   stmpc_solver.hip   the batched ST solver
//   stmpc_learner.hip  the DDPG learner, its population, and the actor population
// Internal to the library: everything declared here has hidden visibility, so none of it joins the C-ABI of include/stmpc.h.
//
// The kernel headers below are here for the structs the context holds.  Their non-template kernels are compiled only where the unit that launches them
// has defined its STMPC_UNIT_* macro before this include; a template kernel is compiled where it is instantiated.
#pragma once
#include "stmpc_kernels.hpp"
#include "stmpc_cc_kernels.hpp"
#include "stmpc_actor_kernels.hpp"
#include "stmpc_env_kernels.hpp"
#include "stmpc_env_groups_kernels.hpp"
#include "stmpc_shield_env_kernels.hpp"
#include "stmpc_cshield_env_kernels.hpp"
#include "stmpc_qshield_env_kernels.hpp"
#include "stmpc_traffic_mix_kernels.hpp"
#include "stmpc_shield_groups_kernels.hpp"
#include "stmpc_solve_plan.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "stmpc.h"

using namespace stmpc;

// The one kernel a unit names without compiling it: stmpc_learner.hip compiles and launches it (stmpc_actor_pop_kernels.hpp), actor_raise_lds in stmpc.hip
// raises its dynamic LDS.  (Before the visibility push: a kernel keeps the visibility its header gives it.)
namespace stmpc {
__global__ void k_actor_eval_pop(FeatCfg f, const ActorDev *members, int n_per_member, int Kmax, const double *ego4, const int *k_count, const double *ox,
                                 const double *ov, const double *oa, const int *live, int *evals, float *feat_out, int feat_stride, double *jerk_out);
}

#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;       // one object for the whole library (stmpc.hip): stmpc_last_error reads it

inline int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(_e == hipErrorOutOfMemory ? STMPC_ENOMEM : STMPC_EHIP,                     \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                        \
    } while (0)

// returns the status of an entry's step when it is not STMPC_OK
#define TRY(expr)                                                                                  \
    do {                                                                                           \
        if (const int _rc = (expr)) return _rc;                                                    \
    } while (0)

// A device allocation that only grows; freed on destruction (on the current device: the destroy entries select the owner's first).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return STMPC_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return fail(STMPC_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
        cap = want;
        return STMPC_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

// host -> device staging: the buffer grows to count elements, then the copy
template <class T> int upload(DevBuf &b, const T *host, size_t count) {
    TRY(b.ensure(count * sizeof(T)));
    HIPCHK(hipMemcpy(b.p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return STMPC_OK;
}
// device -> host; a NULL host pointer is an output the caller did not ask for
template <class T> int download(T *host, const DevBuf &b, size_t count) {
    if (host) HIPCHK(hipMemcpy(host, b.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

// the kernels' vehicle capacity (template argument KMAX): f(std::integral_constant<int, 8, 16 or 32>), the smallest that holds Kalloc
template <class F> void with_kmax(int Kalloc, F &&f) {
    if (Kalloc <= 8) f(std::integral_constant<int, 8>{});
    else if (Kalloc <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 32>{});
}

// argument checks of the host batch entries: the batch's shape, then each state's vehicle count
inline int check_batch(int N, int Kmax) { return N < 0 || Kmax < 0 || Kmax > STMPC_KMAX_LIMIT ? fail(STMPC_EINVAL, "N or Kmax out of range") : STMPC_OK; }
inline int check_counts(int N, int Kmax, const int32_t *k) {
    for (int i = 0; i < N; ++i) if (k[i] < 0 || k[i] > Kmax) return fail(STMPC_EINVAL, "k_count[i] outside [0, Kmax]");
    return STMPC_OK;
}

// the count checks every group entry starts with; `range` is the whole first message (it names the limit), `letter` and `per` the two arguments
inline int check_group_counts(int count, int n_per_group, int max, const char *range, const char *letter = "G", const char *per = "n_per_group") {
    if (count < 1 || count > max) return fail(STMPC_EINVAL, range);
    if (n_per_group < 1) return fail(STMPC_EINVAL, std::string(per) + " must be positive");
    if ((int64_t)count * n_per_group > INT32_MAX) return fail(STMPC_EINVAL, std::string(letter) + " * " + per + " out of range");
    return STMPC_OK;
}
// "`what` must share `field` (it differs in `unit` i)`tail`": SHARED(field) compares that field of `a` (unit 0's struct) and `b` (unit i's), with a
// `const Share share` in scope
struct Share {
    const char *what, *unit;
    int i;
    const char *tail;
    std::string differs(const char *field) const { return std::string(what) + " must share " + field + " (it differs in " + unit + " " + std::to_string(i) + ")" + tail; }
};
#define SHARED(field) if (!(a.field == b.field)) return fail(STMPC_EINVAL, share.differs(#field))
// two host arrays hold the same n bytes: one array, or equal contents
inline bool same_bytes(const void *p, const void *q, size_t n) { return p == q || memcmp(p, q, n) == 0; }

struct stmpc_ctx {
    int device = 0;
    int num_cu = 256;
    int lds_per_block = 65536;
    // staging for the host-pointer API
    struct Staging {
        DevBuf ego, k, ox, ov, path, bt, cost, pd, crash, misc0, misc1, misc2, misc3;
        DevBuf f_seq, f_len, f_v0, f_a0, f_bac, f_out, f_olen, f_iters, f_speed;   // finer_fit / st_control
        // a host batch's states: ego [N][ego_w] (a buffer of [N][5]), k [N], other vehicles [N][Kmax] (buffers for at least one)
        int states(int N, int Kmax, const double *ego_h, int ego_w, const int32_t *k_h, const double *ox_h, const double *ov_h) {
            const size_t n = (size_t)N, Kalloc = Kmax > 0 ? Kmax : 1;
            TRY(ego.ensure(n * 5 * 8)); TRY(k.ensure(n * 4)); TRY(ox.ensure(n * Kalloc * 8)); TRY(ov.ensure(n * Kalloc * 8));
            TRY(upload(ego, ego_h, n * ego_w));
            TRY(upload(k, k_h, n));
            if (Kmax > 0) { TRY(upload(ox, ox_h, n * Kmax)); TRY(upload(ov, ov_h, n * Kmax)); }
            return STMPC_OK;
        }
    } s;
    // What a shield controller keeps of "st.do_st_control of the start states" (shield_control): the controller's outputs for its N rows, with the probe's
    // verdicts, and for the sparse solve the compact batch of the rows that need the controller.  One per controller: each is read back after its call.
    struct ShieldBufs {
        DevBuf path, bt, cost, pcrash, speed, fine, fine_len,
            sel_idx, sel_count, c_ego, c_k, c_ox, c_ov, c_speed, c_fine, c_fine_len;
        int *host_count = nullptr;  // pinned host word for the number of selected rows
        ~ShieldBufs() { if (host_count) (void)hipHostFree(host_count); }      // (on the current device, as DevBuf)
        int ensure(int N, int H) {
            const size_t n = (size_t)N;
            TRY(path.ensure(n * H * 4)); TRY(bt.ensure(n * 4)); TRY(cost.ensure(n * 8)); TRY(pcrash.ensure(n * 4));
            TRY(speed.ensure(n * 8)); TRY(fine.ensure(n * STMPC_QP_NMAX * 8)); TRY(fine_len.ensure(n * 4));
            return STMPC_OK;
        }
        // the selection and the compact batch, sized once for all rows: no allocation between the launches of a tick
        int ensure_compact(int N, int Kalloc) {
            const size_t n = (size_t)N;
            TRY(sel_idx.ensure(n * 4)); TRY(sel_count.ensure(4));
            TRY(c_ego.ensure(n * 5 * 8)); TRY(c_k.ensure(n * 4)); TRY(c_ox.ensure(n * Kalloc * 8)); TRY(c_ov.ensure(n * Kalloc * 8));
            TRY(c_speed.ensure(n * 8)); TRY(c_fine.ensure(n * STMPC_QP_NMAX * 8)); TRY(c_fine_len.ensure(n * 4));
            return STMPC_OK;
        }
    };
    // combined controller (stmpc_rollout_step_device / stmpc_combined_decide_device): rollout bookkeeping, the probe's states, the controller's outputs
    struct Combined {
        DevBuf live, hist_len, crash_pred, have_test, sel, rollout_s, test_ego, test_ox, test_ov, probe_ego, probe_ox, probe_ov;
        ShieldBufs sh;
        int N = 0, K = 0, R = 0;
        // controller groups (stmpc_combined_groups_set): `groups` holds C CCfg; C = 0: no table.  `grouped`: the rollout in the context was begun by
        // stmpc_rollout_step_groups_device (R is then the largest group's rollout_length, the row stride of rollout_s less one)
        DevBuf groups, ask, test_idx, c_pcrash;
        std::vector<CCfg> table;
        int C = 0, n_per_group = 0, Rmax = 0, n_test = 0, any_strict = 0, sparse = 0;
        double tick = 0;
        bool grouped = false;
        int64_t ticks = 0, control_solves = 0;      // decisions taken / controller solves run for them (stmpc_combined_counts)
        int ensure(int n_, int k_, int r_) {        // the rollout's bookkeeping (step 1)
            const size_t n = (size_t)n_;
            TRY(live.ensure(n * 4)); TRY(hist_len.ensure(n * 4)); TRY(crash_pred.ensure(n * 4)); TRY(have_test.ensure(n * 4)); TRY(sel.ensure(n * 8));
            TRY(rollout_s.ensure(n * (r_ + 1) * 8)); TRY(test_ego.ensure(n * 4 * 8)); TRY(test_ox.ensure(n * k_ * 8)); TRY(test_ov.ensure(n * k_ * 8));
            N = n_; K = k_; R = r_;
            return STMPC_OK;
        }
        CCState state() const {
            return CCState{live.as<int>(), hist_len.as<int>(), crash_pred.as<int>(), have_test.as<int>(), sel.as<double>(), rollout_s.as<double>(),
                           test_ego.as<double>(), test_ox.as<double>(), test_ov.as<double>()};
        }
        void drop_grouped() { if (grouped) { grouped = false; N = 0; } }       // (a grouped rollout of a former table cannot be continued or decided)
    } cc;
    // first-step shield controller (stmpc_first_step_device): the predicted states, the probe's and the controller's outputs
    struct FirstStep {
        DevBuf next_ego, next_ox, next_ov, crashed, takeovers;
        ShieldBufs sh;
        int N = 0, K = 0;           // shape of the last call (stmpc_first_step reads the predicted states back)
        int64_t decisions = 0, control_solves = 0;      // stmpc_first_step_counts (the takeovers are counted on the device: `takeovers`, one 64-bit word)
    } fs;
    // batched episode simulator (stmpc_sim_*)
    struct Sim {
        DevBuf ego, nveh, vx, vv, va, vc, delay, status, ticks, rng, acc, route, groups;
        int N = 0, route_n = 0;
        int G = 0, n_per_group = 0;   // traffic groups (stmpc_sim_init_groups_device): `groups` holds G sim::Cfg; 0, 0 = an ungrouped world
        int64_t generation = 0;    // stmpc_sim_init_device calls so far (a recorder bound to an earlier world refuses to go on)
        int ensure(int n_) {
            const size_t n = (size_t)n_, KS = sim::KS;
            TRY(ego.ensure(n * 4 * 8)); TRY(nveh.ensure(n * 4)); TRY(vx.ensure(n * KS * 8)); TRY(vv.ensure(n * KS * 8)); TRY(va.ensure(n * KS * 8));
            TRY(vc.ensure(n * KS * 8)); TRY(delay.ensure(n * 8)); TRY(status.ensure(n * 4)); TRY(ticks.ensure(n * 4)); TRY(rng.ensure(n * 4));
            TRY(acc.ensure(n * sim::NACC * 8));
            return STMPC_OK;
        }
        sim::State state() const {
            return sim::State{ego.as<double>(), nveh.as<int>(), vx.as<double>(), vv.as<double>(), va.as<double>(), vc.as<double>(), delay.as<double>(),
                              status.as<int>(), ticks.as<int>(), rng.as<unsigned>(), acc.as<double>()};
        }
    } sim;
    // vector environment on the simulator (stmpc_env_*)
    struct Env {
        DevBuf ep, prev_a, pjerk, inv, ret, cmd, live, vx, vv, va, k, log, log_n, actions, rtab, mix_rows, mix_cum, mix_type;
        int N = 0, n_actions = 0, log_cap = 0, mode = -1;    // (N = 0: no environment; a plain stmpc_sim_init_device invalidates it)
        int R = 0, n_per_rg = 0;      // reward groups (stmpc_reward_groups_env_reset_device): `rtab` holds R env::RewardRow; 0, 0 = one reward for all
        sim::Cfg rg_sc{};             // the ungrouped world of an env with reward groups (its step entry takes no sim cfg)
        env::RewardTab reward_tab() const { return env::RewardTab{rtab.as<env::RewardRow>(), n_per_rg}; }
        // traffic mix (stmpc_traffic_mix_env_reset_device): `mix_rows` / `mix_cum` hold T env::TrafficRow / cumulative weights, `mix_type` the type of
        // each environment's current episode; T = 0: no mix.  `mix_sc`: what the types share (the mix step takes no sim cfg)
        int T = 0;
        unsigned long long mix_seed = 0;
        sim::Cfg mix_sc{};
        env::TrafficMix traffic_mix() const { return env::TrafficMix{mix_rows.as<env::TrafficRow>(), mix_cum.as<double>(), mix_type.as<int>(), T, mix_seed}; }
        int ensure(int n_, int cap) {
            const size_t n = (size_t)n_, KS = sim::KS;
            TRY(ep.ensure(n * 4)); TRY(prev_a.ensure(n * 8)); TRY(pjerk.ensure(n * 8)); TRY(inv.ensure(n * 8)); TRY(ret.ensure(n * 8)); TRY(cmd.ensure(n * 8));
            TRY(live.ensure(n * 4)); TRY(vx.ensure(n * KS * 8)); TRY(vv.ensure(n * KS * 8)); TRY(va.ensure(n * KS * 8)); TRY(k.ensure(n * 4)); TRY(log_n.ensure(4));
            TRY(log.ensure((size_t)cap * env::NLOG * 8));
            log_cap = cap;
            return STMPC_OK;
        }
        env::EState state(unsigned *err) const {
            return env::EState{ep.as<int>(), prev_a.as<double>(), pjerk.as<double>(), inv.as<double>(), ret.as<double>(), cmd.as<double>(), live.as<int>(),
                               vx.as<double>(), vv.as<double>(), va.as<double>(), k.as<int>(), log.as<double>(), log_n.as<unsigned>(), err};
        }
    } env;
    // shielded vector environment (stmpc_shield_env_*): the planner's view and the proposal handed to the first-step shield, its decision, and the
    // takeovers of each environment's current episode with the episode they were counted in.  Valid while `generation` is the world's.
    // `penalty`: the takeover penalties of a shielded env with groups or a traffic mix (stmpc_shield_traffic_groups_env_reset_device and its kin), P values for
    // n_per_penalty consecutive environments each; P = 0: the lone shielded env, whose step takes its penalty by value
    struct ShieldEnv {
        DevBuf ego5, k, ox, ov, proposal, speed, takeover, reason, count, tag, penalty;
        int N = 0, kmax = 0, P = 0, n_per_penalty = 0;
        int64_t generation = -1;
        env::PenaltyTab penalty_tab() const { return env::PenaltyTab{penalty.as<double>(), n_per_penalty}; }
        int ensure(int n_, int kmax_) {
            const size_t n = (size_t)n_;
            TRY(ego5.ensure(n * 5 * 8)); TRY(k.ensure(n * 4)); TRY(ox.ensure(n * kmax_ * 8)); TRY(ov.ensure(n * kmax_ * 8)); TRY(proposal.ensure(n * 8));
            TRY(speed.ensure(n * 8)); TRY(takeover.ensure(n * 4)); TRY(reason.ensure(n * 4)); TRY(count.ensure(n * 4)); TRY(tag.ensure(n * 4));
            return STMPC_OK;
        }
        env::ShieldView view() const { return env::ShieldView{ego5.as<double>(), k.as<int>(), ox.as<double>(), ov.as<double>(), proposal.as<double>()}; }
    } shield;
    // vector environment behind the combined controller (stmpc_cshield_env_*): the start and current rows of the rollout, the first action, the rollout
    // actor's time counter with the episode it was counted in, the decision, and the takeovers of each environment's current episode with theirs.  Valid
    // while `generation` is the world's; kmax, rollout_time and L (the rollout length) are the reset's.  The discrete env behind a Q-network
    // (stmpc_qshield_env_*) keeps the same rows here -- a context holds one env -- without the time counter: `qpolicy` is then the reset's stmpc_qactor
    // or stmpc_qactor_pop (NULL: the continuous env behind an actor), n_per_member the population's rows per member (0: a lone Q-actor)
    struct CShieldEnv {
        DevBuf ego5, k, ox, ov, cur_ego4, cur_ox, cur_ov, cur_oa, first_action, jerk, evals, evals_tag, speed, takeover, reason, count, tag;
        int N = 0, kmax = 0, rollout_time = 0, L = 0;
        const void *qpolicy = nullptr;
        int n_per_member = 0;
        int64_t generation = -1;
        int ensure(int n_, int kmax_) {
            const size_t n = (size_t)n_, row = n * kmax_ * 8;
            TRY(ego5.ensure(n * 5 * 8)); TRY(k.ensure(n * 4)); TRY(ox.ensure(row)); TRY(ov.ensure(row)); TRY(cur_ego4.ensure(n * 4 * 8)); TRY(cur_ox.ensure(row));
            TRY(cur_ov.ensure(row)); TRY(cur_oa.ensure(row)); TRY(first_action.ensure(n * 8)); TRY(jerk.ensure(n * 8)); TRY(evals.ensure(n * 4));
            TRY(evals_tag.ensure(n * 4)); TRY(speed.ensure(n * 8)); TRY(takeover.ensure(n * 4)); TRY(reason.ensure(n * 4)); TRY(count.ensure(n * 4));
            TRY(tag.ensure(n * 4));
            return STMPC_OK;
        }
        env::CShieldView view() const {
            return env::CShieldView{ego5.as<double>(), k.as<int>(), ox.as<double>(), ov.as<double>(), cur_ego4.as<double>(), cur_ox.as<double>(), cur_ov.as<double>(),
                                    cur_oa.as<double>(), first_action.as<double>(), evals.as<int>(), evals_tag.as<int>()};
        }
    } cshield;
    // the batched ST solver (solve_device and the entries on top of it)
    struct Solver {
        plan::SolveKnobs knobs;        // the STMPC_* settings (stmpc_create)
        DevBuf tab_edge, tab_win, tab_nact, tab_nums, counters, lists, ubound, proxy, order, gscratch, bp_tier[STMPC_MAX_TIERS], resume_t, phase_prof, prio_key, cu_tab;   // scratch
        // checkpoint pool, and what the quarter-of-free-memory rule remembers
        DevBuf ckpt, pool_bp;
        unsigned resume_refused_calls = 0;
        bool last_resume_refused = false;   // the last batch wanted checkpoint / resume and did not get it (stmpc_stats::resume_refused)
        size_t resume_refused_for = 0; // back-pointer bytes of the last request the quarter-of-free-memory rule turned down (not asked again until the request changes)
        // guide tables, one per parameter set (dynamics + cost weights), least recently used replaced: a caller that alternates parameter sets
        // (two controllers on one context) neither rebuilds nor waits
        struct GuideSlot { double key[12] = {0}; bool valid = false, ok = false; int imax = 0, D = 0; std::vector<unsigned char> host; DevBuf dev; uint64_t last_use = 0; };
        GuideSlot guides[4]; uint64_t guide_clock = 0;
        DevBuf guide_cells;
        // solver groups: the device copy of the last grouped call's table (kept while the next call's table is equal), its guide tables, one after another,
        // and the groups' crash_min_s for the grouped world step
        struct SolverGroupsDev {
            DevBuf table, guide, crash_min_s;
            std::vector<GroupP> host;          // what `table` holds
            std::vector<double> host_cms;      // what `crash_min_s` holds
            bool want_guide = false, guide_ok = false; int guide_imax = 0, guide_D = 0;
        } sg;
        double fd2_dt = 0, fd2_dt2 = 0, fd2_dt3 = 0, fd2_zl[3] = {0, 0, 0}; bool fd2_ok = false;      // fastdiv2_ok results for the current dt
        // the side stream and the CU-masked pair of STMPC_CU_RESERVE, with the events that fork from and join the caller's stream
        hipStream_t aux_stream = nullptr, main_masked = nullptr, aux_reserved = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join0 = nullptr, ev_join_r = nullptr;
        int *h_overflow = nullptr, *d_overflow = nullptr;   // mapped pinned words the batch's last launch stores (plan::SolveHistory::overflow)
        int last_nt = 0;
        bool last_has_hbm = true;
        int64_t last_hbm_tier_count = 0;    // episodes the last batch whose statistics were read sent to the clean-up tier
        hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
        // profiling pool: one (begin, dp-begin, dp-end, end) event quad per launch while enabled
        bool profiling = false;
        std::vector<hipEvent_t> pool;
        size_t pool_used = 0;          // events used (multiple of 4)
        double acc_solve_ms = 0, acc_dp_ms = 0;
        int64_t acc_launches = 0, acc_fallback = 0, acc_episodes = 0;
    } solver;
    stmpc_stats stats{};
    bool stats_pending = false;
    DevBuf sticky;                 // [3] error flags that outlive a call: [0] solver internal error, [1] QP re-sampling refused a path, [2] a discrete env action out of range
                                   // (read and cleared by stmpc_check_error)
};

// ---- defined in stmpc.hip
extern double (*volatile host_pow)(double, double);
// the policy network (stmpc_actor_create, or a view of a learner's weights: stmpc_actor_view_ddpg in stmpc_learner.hip)
struct stmpc_actor {
    int device = 0;
    DevBuf p0, b0, p1, b1, w2, b2;      // empty for a view (stmpc_actor_view_ddpg): dev then points into the learner's arrays
    ActorDev dev{};
    size_t lds = 0;
};
// for stmpc_learner.hip: the lone actor's argument checks (the actor population makes them too), the rows of a rollout that are still live, an actor's
// dynamic LDS and the kernel attribute that allows it
int actor_eval_checks(const stmpc_ctx *c, int device, int n_in, const stmpc_policy_features_cfg *f, int N, int Kmax, int step, const double *d_cur_ego4,
                      const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const int32_t *d_evals, const float *d_feat, int feat_stride,
                      const double *d_jerk, FeatCfg *fc);
int rollout_live(const stmpc_ctx *c, int N, int step, const int **live);
size_t actor_lds_bytes(int h1p, int h2p);
int actor_raise_lds(int which, int device, size_t lds);
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel, not to the actor or learner that launches it: it is only ever raised, so that
// a narrower network created later does not take the dynamic LDS away from a wider one that is still in use.  One ceiling per kernel (and device),
// kept by the caller; the current device is `device`.
struct LdsCeiling { size_t max[16] = {0}; };
int raise_dynamic_lds(const void *fn, const char *kernel, LdsCeiling &ceiling, int device, size_t lds);

// ---- defined in stmpc_learner.hip
// stmpc_qactor_eval_device / stmpc_pop_qactor_eval_device after their argument checks (N >= 1): the entries' bodies, shared with stmpc_qshield_env_step_device
int qactor_eval_run(stmpc_ctx *c, const stmpc_qactor *q, const FeatCfg &fc, int N, int Kmax, int step, const double *d_cur_ego4, const int32_t *d_k,
                    const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, float *d_feat, int feat_stride, int32_t *d_action, float *d_q,
                    double *d_jerk, void *stream);
int qactor_pop_eval_run(stmpc_ctx *c, const stmpc_qactor_pop *p, const FeatCfg &fc, int n_per_member, int Kmax, int step, const double *d_cur_ego4,
                        const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, float *d_feat, int feat_stride,
                        int32_t *d_action, float *d_q, double *d_jerk, void *stream);
// what stmpc_qshield_env_* requires of its rollout policy -- exactly one of q (a lone Q-actor on all N rows) and pop (P members, P * n_per_member == N):
// the context's device, n_actions == n_values, the env's action mode, a table byte-identical to `values` and, in acceleration mode, the env's tick and
// jerk limits.  *n_in receives the policy's input width.
int qshield_policy_check(const stmpc_ctx *c, const stmpc_qactor *q, const stmpc_qactor_pop *pop, int n_per_member, int N, bool acceleration,
                         const double *values, int n_values, double tick, double jerk_min, double jerk_max, int *n_in);

// ---- defined in stmpc_solver.hip
void host_t_values(const stmpc_params *p, int H, double *t);
bool bad_layers(int H);
int num_layers(const stmpc_params *p, int *H);
int host_batch_begin(stmpc_ctx *c, int N, int Kmax, const double *ego, const int32_t *k, const double *ox, const double *ov, bool outs);
int make_devp(const stmpc_params *p, DevP *d);
int check_solver_groups(const stmpc_params *groups, int G, int n_per_group, std::vector<GroupP> *out);
// the groups of a grouped solve: the table as check_solver_groups made it (band, band2_mult and guide_off are filled in by solve_device)
struct SolverGroupsHost { std::vector<GroupP> table; int n_per_group = 0; };
int solver_groups_of(const stmpc_params *groups, int G, int n_per_group, int N, SolverGroupsHost *sg);
int solve_device(stmpc_ctx *c, const stmpc_params *p, SolverGroupsHost *sg, int N, int Kmax, const double *d_ego,
                 const int32_t *d_k, const double *d_ox, const double *d_ov, int32_t *d_path,
                 int32_t *d_bt, double *d_cost, double *d_pd, int32_t *d_crash, double *d_action_cost, void *stream);

#pragma GCC visibility pop
