// stmpc.hip -- the core of the C-ABI (include/stmpc.h): the context and the host helpers, the controllers on top of the solver (stmpc_solver.hip),
// the episode world, the vector env and the flight recorder.  The learners are stmpc_learner.hip; what they call here is declared in stmpc_host.hpp.
// Host side: context, device buffers, launch sequencing on the caller's HIP stream.
// No CPU fallback: every compute entry needs a HIP device.
// (The world and the env stay in this unit with the controllers: their observation kernels are optimised together with k_policy_features and k_actor_eval,
// whose feature code they share, and come out different in a module without them.)
#define STMPC_UNIT_CONTROL      // (this unit launches the kernels of the controllers and of the episode world)
#define STMPC_UNIT_ENV
#include "stmpc_host.hpp"      // (the context, the shared helpers, the kernel headers the context needs)
#include "stmpc_ff_kernels.hpp"
#include "stmpc_nj_kernels.hpp"
#include "stmpc_rec_kernels.hpp"
#include "stmpc_sim_groups_kernels.hpp"
#include "stmpc_cc_groups_kernels.hpp"
#include "stmpc_fs_kernels.hpp"
#include "stmpc_solver_groups_kernels.hpp"

thread_local std::string g_err;

// libm pow through a volatile pointer so clang cannot fold pow(x,2.0)/pow(x,3.0): the reference's
// Python evaluates float**int with libm pow (control.py:38) and Cython's dt**3 likewise (st_cy.pyx:49).
double (*volatile host_pow)(double, double) = pow;

namespace {
std::string g_info;
}  // namespace

extern "C" {

const char *stmpc_last_error(void) { return g_err.c_str(); }

#ifndef STMPC_SRC_HASH
#define STMPC_SRC_HASH "unknown"      /* build.py passes sha256[:16] of csrc/ + include/stmpc.h */
#endif
const char *stmpc_backend_info(void) {
    if (!g_info.empty()) return g_info.c_str();
    int n = 0;
    char buf[512];
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        g_info = "stmpc 0.1 hip (no device) src=" STMPC_SRC_HASH;
        return g_info.c_str();
    }
    hipDeviceProp_t pr;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) { g_info = "stmpc 0.1 hip (device query failed) src=" STMPC_SRC_HASH; return g_info.c_str(); }
    snprintf(buf, sizeof buf, "stmpc 0.1 hip %s %s cu=%d lds=%zu devices=%d src=%s", pr.gcnArchName, pr.name,
             pr.multiProcessorCount, (size_t)pr.sharedMemPerBlock, n, STMPC_SRC_HASH);
    g_info = buf;
    return g_info.c_str();
}

int stmpc_create(stmpc_ctx **out, int device) {
    if (!out) return fail(STMPC_EINVAL, "stmpc_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(STMPC_ENODEV, "no HIP device available (stmpc has no CPU fallback)");
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return fail(STMPC_ENODEV, "hipGetDevice failed"); }
    if (device >= n) return fail(STMPC_EINVAL, "device index out of range");
    HIPCHK(hipSetDevice(device));
    stmpc_ctx *c = new stmpc_ctx();
    c->device = device;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) == hipSuccess) {
        c->num_cu = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
        c->lds_per_block = (int)pr.sharedMemPerBlock;
    }
    stmpc_ctx::Solver &sv = c->solver;
    if (hipEventCreate(&sv.ev0) != hipSuccess || hipEventCreate(&sv.ev1) != hipSuccess ||
        hipEventCreate(&sv.ev2) != hipSuccess || hipEventCreate(&sv.ev3) != hipSuccess) {
        delete c;
        return fail(STMPC_EHIP, "hipEventCreate failed");
    }
    sv.knobs = plan::SolveKnobs::from_env();
    // the side stream gets the highest priority: priority levels have their own hardware queues, so its launch
    // cannot end up queued behind the main stream's in a process that owns many streams (torch + RCCL)
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&sv.aux_stream, hipStreamNonBlocking, prio_greatest) != hipSuccess) {
        (void)hipGetLastError();
        sv.aux_stream = nullptr;
        if (hipStreamCreateWithFlags(&sv.aux_stream, hipStreamNonBlocking) != hipSuccess) sv.aux_stream = nullptr;
    }
    if (!sv.aux_stream) sv.knobs.overlap = 0;          // no side stream: the tiers simply run one after the other
    if (c->sticky.ensure(3 * sizeof(unsigned)) || hipMemset(c->sticky.p, 0, 3 * sizeof(unsigned)) != hipSuccess) { stmpc_destroy(c); return fail(STMPC_ENOMEM, "device allocation failed"); }
    if (const int v = sv.knobs.cu_reserve) {
        // Reserved compute units: bit 32a + a + 8j (a = 0..7, j < n/8) of the CU mask.  Whether the driver numbers the mask bits
        // XCD by XCD or round-robin over the XCDs, every XCD gives up n/8 units and keeps the rest (a queue whose mask leaves an XCD
        // without units would never get the workgroups the dispatcher assigns to that XCD).
        sv.knobs.cu_reserve = 0;
        if (sv.aux_stream && c->num_cu == 256) {
            uint32_t res[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rest[8];
            for (int a = 0; a < 8; ++a) for (int j = 0; j < v / 8; ++j) { const int bit = 32 * a + ((a + 8 * j) & 31); res[bit >> 5] |= 1u << (bit & 31); }
            for (int i = 0; i < 8; ++i) rest[i] = ~res[i];
            if (hipExtStreamCreateWithCUMask(&sv.main_masked, 8, rest) == hipSuccess && hipExtStreamCreateWithCUMask(&sv.aux_reserved, 8, res) == hipSuccess &&
                hipEventCreateWithFlags(&sv.ev_join0, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&sv.ev_join_r, hipEventDisableTiming) == hipSuccess)
                sv.knobs.cu_reserve = v;
            else (void)hipGetLastError();
        }
    }
    if (hipEventCreateWithFlags(&sv.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sv.ev_join, hipEventDisableTiming) != hipSuccess) {
        stmpc_destroy(c);
        return fail(STMPC_EHIP, "stream/event creation failed");
    }
    *out = c;
    return STMPC_OK;
}

void stmpc_destroy(stmpc_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);       // (the device buffers are freed by their destructors, on this device)
    stmpc_ctx::Solver &sv = c->solver;
    if (sv.h_overflow) (void)hipHostFree(sv.h_overflow);
    if (sv.main_masked) (void)hipStreamDestroy(sv.main_masked);
    if (sv.aux_reserved) (void)hipStreamDestroy(sv.aux_reserved);
    if (sv.ev_join0) (void)hipEventDestroy(sv.ev_join0);
    if (sv.ev_join_r) (void)hipEventDestroy(sv.ev_join_r);
    if (sv.ev_fork) (void)hipEventDestroy(sv.ev_fork);
    if (sv.ev_join) (void)hipEventDestroy(sv.ev_join);
    if (sv.aux_stream) (void)hipStreamDestroy(sv.aux_stream);
    if (sv.ev0) (void)hipEventDestroy(sv.ev0);
    if (sv.ev1) (void)hipEventDestroy(sv.ev1);
    if (sv.ev2) (void)hipEventDestroy(sv.ev2);
    if (sv.ev3) (void)hipEventDestroy(sv.ev3);
    for (hipEvent_t ev : sv.pool) (void)hipEventDestroy(ev);
    delete c;
}

// ---- host helpers ------------------------------------------------------------------------
double stmpc_ego_s(double x, double y) {
    // control.py:366-380 with control.distance (control.py:37-38): math.sqrt(dx**2 + dy**2)
    const double mpx = -50.9, mpy = 1.72, mp2x = 1.5, mp3x = -51.0;
    const double common_s = mp2x - mp3x;
    if (x < mpx) return -sqrt(host_pow(x - mpx, 2.0) + host_pow(y - mpy, 2.0));
    else if (x < mp2x) return sqrt(host_pow(x - mpx, 2.0) + host_pow(y - mpy, 2.0));
    else return x - mp2x + common_s;
}

int stmpc_num_s(const stmpc_params *p, double start_s) {
    if (!p) return STMPC_EINVAL;
    double stop = start_s + p->future_s + p->ds;
    return (int)ceil((stop - start_s) / p->ds);
}

int stmpc_num_t(const stmpc_params *p) {
    if (!p) return STMPC_EINVAL;
    double stop = p->future_t + p->dt;
    return (int)ceil((stop - 0.0) / p->dt);
}

double stmpc_path_mean_abs_jerk(const double *s, int n, double v0, double a0, double dt) {
    // st.py:274-288
    double prev_a = a0, prev_v = v0, acc = 0.0;
    for (int i = 1; i < n; ++i) {
        double v = (s[i] - s[i - 1]) / dt;
        double a = (v - prev_v) / dt;
        double j = (a - prev_a) / dt;
        prev_v = v; prev_a = a;
        acc += fabs(j);
    }
    return acc / (double)(n - 1);
}

int stmpc_abi_version(void) { return STMPC_ABI_VERSION; }

int stmpc_check_error(stmpc_ctx *c) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned flags[3] = {0, 0, 0}, cur = 0;
    HIPCHK(hipMemcpy(flags, c->sticky.p, sizeof flags, hipMemcpyDeviceToHost));
    if (c->solver.counters.p) HIPCHK(hipMemcpy(&cur, (const unsigned *)c->solver.counters.p + STMPC_CNT_ERR, sizeof cur, hipMemcpyDeviceToHost));
    if (flags[0] || flags[1] || flags[2] || cur) {
        HIPCHK(hipMemset(c->sticky.p, 0, sizeof flags));
        if (cur) HIPCHK(hipMemset((unsigned *)c->solver.counters.p + STMPC_CNT_ERR, 0, sizeof cur));
    }
    if (flags[0] || cur) return fail(STMPC_EINTERNAL, "solver error flag set on device (an episode of an earlier batch may not have been solved)");
    if (flags[1]) return fail(STMPC_EINVAL, "finer_fit: a fine grid longer than STMPC_QP_NMAX samples is not supported (the commanded speed of that state is not valid)");
    if (flags[2]) return fail(STMPC_EINVAL, "stmpc_env_step_device: a discrete action index out of range (that environment kept its speed for the tick)");
    return STMPC_OK;
}
}  // extern "C"

namespace {
int make_ffconst(const stmpc_params *p, double dt, double cdt, int maxiters, FFConst *k) {
    if (!p) return fail(STMPC_EINVAL, "params is NULL");
    if (!(dt > 0) || !(cdt > 0)) return fail(STMPC_EINVAL, "delta_t and coarse_delta_t must be positive");
    if (maxiters < 0) return fail(STMPC_EINVAL, "maxiters must be >= 0");
    memset(k, 0, sizeof *k);
    const double dt2 = host_pow(dt, 2.0), dt3 = host_pow(dt, 3.0);   // delta_t ** 2, delta_t ** 3 (st.py:626,644)
    k->dt = dt; k->cdt = cdt; k->dt2 = dt2;
    k->cv = 1.0 / dt;                                                // st.py:613
    k->ca1 = 1.0 / dt2; k->ca2 = 2.0 / dt2;                          // st.py:629-633
    k->cj1 = 1.0 / dt3; k->cj2 = 2.0 / dt3; k->cj3 = 3.0 / dt3;      // st.py:646-658
    k->v_max = p->v_max; k->a_max = p->a_max; k->a_min = p->a_min; k->j_max = p->j_max; k->j_min = p->j_min;
    k->car_length = p->car_length;
    k->maxiters = maxiters;
    return STMPC_OK;
}

// Lanes per problem: the smallest of 16/32/64 that holds the longest fine grid a path of Hs samples can produce
// (st.py:590-595); a wavefront then carries 64/GW problems.  The result bits do not depend on the choice.
int ff_group_width(int Hs, double dt, double cdt) {
    const double t_last = (double)(Hs - 1) * cdt;
    int n = (int)rint(t_last / dt + 1.0);
    if ((double)(n - 1) * dt > t_last) n -= 1;
    if (Hs > 32 || n > 32) return 64;       // the coarse path itself is held one sample per lane
    if (Hs > 16 || n > 16) return 32;
    return 16;
}

void launch_finer_fit(const FFArgs &a, bool bounds, int gw, hipStream_t st) {
    const dim3 block(64), grid((a.N + (64 / gw) - 1) / (64 / gw));
#define STMPC_FF(NF_, GW_) hipLaunchKernelGGL((k_finer_fit<NF_, GW_>), grid, block, 0, st, a)
    if (bounds) { if (gw == 16) STMPC_FF(8, 16); else if (gw == 32) STMPC_FF(8, 32); else STMPC_FF(8, 64); }
    else { if (gw == 16) STMPC_FF(6, 16); else if (gw == 32) STMPC_FF(6, 32); else STMPC_FF(6, 64); }
#undef STMPC_FF
}
}  // namespace

extern "C" {

int stmpc_finer_fit_batch(stmpc_ctx *c, const stmpc_params *p, double dt, double cdt, int maxiters, int N, int Hs,
                          const double *s_seq, const int32_t *len, const double *v0, const double *a0, const double *bac,
                          int n_max, double *out, int32_t *out_len, int32_t *iters) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N < 0 || Hs < 1 || Hs > 64 || n_max < 1) return fail(STMPC_EINVAL, "N, Hs (1..64) or n_max out of range");
    if (N == 0) return STMPC_OK;
    if (!s_seq || !len || !v0 || !a0 || !out || !out_len) return fail(STMPC_EINVAL, "NULL host pointer");
    for (int i = 0; i < N; ++i) if (len[i] < 1 || len[i] > Hs) return fail(STMPC_EINVAL, "len[i] outside [1, Hs]");
    FFArgs a;
    memset(&a, 0, sizeof a);
    TRY(make_ffconst(p, dt, cdt, maxiters, &a.k));
    HIPCHK(hipSetDevice(c->device));
    auto &s = c->s;
    const size_t n = (size_t)N;
    TRY(s.f_out.ensure(n * n_max * 8)); TRY(s.f_olen.ensure(n * 4)); TRY(s.f_iters.ensure(n * 4));
    TRY(upload(s.f_seq, s_seq, n * Hs)); TRY(upload(s.f_len, len, n)); TRY(upload(s.f_v0, v0, n)); TRY(upload(s.f_a0, a0, n));
    if (bac) TRY(upload(s.f_bac, bac, n * 4));
    HIPCHK(hipMemset(s.f_out.p, 0, n * n_max * 8));
    a.N = N; a.Hs = Hs; a.n_max = n_max; a.use_qp = 1;
    a.s_seq = s.f_seq.as<double>(); a.len = s.f_len.as<int>(); a.v0 = s.f_v0.as<double>(); a.a0 = s.f_a0.as<double>();
    a.bac = bac ? s.f_bac.as<double>() : nullptr;
    a.out = s.f_out.as<double>(); a.out_len = s.f_olen.as<int>(); a.iters = s.f_iters.as<int>();
    launch_finer_fit(a, bac != nullptr, ff_group_width(Hs, dt, cdt), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    TRY(download(out, s.f_out, n * n_max)); TRY(download(out_len, s.f_olen, n)); TRY(download(iters, s.f_iters, n));
    return STMPC_OK;
}

// st.do_st_control on device buffers.  `refused`: the word a path that cannot be re-sampled raises (the public entry: the context's sticky flag,
// so that stmpc_check_error reports STMPC_EINVAL; the combined controller: null -- there k_cc_decide raises it only when that speed is used).
static int st_control_device(stmpc_ctx *c, const stmpc_params *p, double tick, int N, int Kmax, const double *d_ego,
                             const int32_t *d_k, const double *d_ox, const double *d_ov, int32_t *d_path,
                             int32_t *d_bt, double *d_cost, double *d_speed, double *d_fine, int32_t *d_fine_len,
                             void *stream, unsigned *refused, SolverGroupsHost *sg = nullptr) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N == 0) return STMPC_OK;
    if (!d_speed) return fail(STMPC_EINVAL, "NULL device pointer (speed)");
    // (with solver groups: the re-sampling below reads none of the fields the groups may differ in -- FFConst holds limits, tick and car length only)
    TRY(solve_device(c, p, sg, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, nullptr, nullptr, nullptr, stream));
    FFArgs a;
    memset(&a, 0, sizeof a);
    const int H = stmpc_num_t(p);
    double tv[STMPC_MAXH];
    host_t_values(p, H, tv);
    // finer_fit is called with (TICK_LENGTH, T_DISCRETIZATION) = the settings, not the arange spacing (st.py:771-772)
    TRY(make_ffconst(p, tick, p->dt, c->solver.knobs.qp_maxiters, &a.k));
    a.N = N; a.Hs = H; a.n_max = STMPC_QP_NMAX; a.use_qp = (tick < p->dt) ? 1 : 0;
    a.path_idx = d_path; a.best_t = d_bt; a.ego = d_ego; a.ds = p->ds;
    a.out = d_fine; a.out_len = d_fine_len; a.speed = d_speed;
    a.refused = refused;
    launch_finer_fit(a, false, a.use_qp ? ff_group_width(H, tick, p->dt) : 64, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_st_control_batch_device(stmpc_ctx *c, const stmpc_params *p, double tick, int N, int Kmax, const double *d_ego,
                                  const int32_t *d_k, const double *d_ox, const double *d_ov, int32_t *d_path,
                                  int32_t *d_bt, double *d_cost, double *d_speed, double *d_fine, int32_t *d_fine_len,
                                  void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    // a path that cannot be re-sampled (its speed is NaN): stmpc_check_error returns STMPC_EINVAL
    return st_control_device(c, p, tick, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_speed, d_fine, d_fine_len, stream, c->sticky.as<unsigned>() + 1);
}

int stmpc_st_control_batch(stmpc_ctx *c, const stmpc_params *p, double tick, int N, int Kmax, const double *ego,
                           const int32_t *k, const double *ox, const double *ov, double *speed, int32_t *bt,
                           int32_t *path, double *cost, double *fine, int32_t *fine_len) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(host_batch_begin(c, N, Kmax, ego, k, ox, ov, speed && bt));
    if (N == 0) return STMPC_OK;
    int H;
    TRY(num_layers(p, &H));
    auto &s = c->s;
    const size_t n = (size_t)N;
    TRY(s.path.ensure(n * H * 4)); TRY(s.bt.ensure(n * 4)); TRY(s.cost.ensure(n * 8));
    TRY(s.f_speed.ensure(n * 8)); TRY(s.f_out.ensure(n * STMPC_QP_NMAX * 8)); TRY(s.f_olen.ensure(n * 4));
    TRY(s.states(N, Kmax, ego, 5, k, ox, ov));
    if (fine) HIPCHK(hipMemset(s.f_out.p, 0, n * STMPC_QP_NMAX * 8));
    TRY(stmpc_st_control_batch_device(c, p, tick, N, Kmax, s.ego.as<double>(), s.k.as<int32_t>(), s.ox.as<double>(), s.ov.as<double>(), s.path.as<int32_t>(),
                                      s.bt.as<int32_t>(), s.cost.as<double>(), s.f_speed.as<double>(), s.f_out.as<double>(), s.f_olen.as<int>(), nullptr));
    HIPCHK(hipDeviceSynchronize());
    TRY(download(speed, s.f_speed, n)); TRY(download(bt, s.bt, n)); TRY(download(path, s.path, n * H)); TRY(download(cost, s.cost, n));
    TRY(download(fine, s.f_out, n * STMPC_QP_NMAX)); TRY(download(fine_len, s.f_olen, n));
    stmpc_stats st;
    TRY(stmpc_get_stats(c, &st));
    // (this entry is synchronous: a refused re-sampling is its own error, not left for a later stmpc_check_error)
    unsigned refused = 0;
    HIPCHK(hipMemcpy(&refused, c->sticky.as<unsigned>() + 1, sizeof refused, hipMemcpyDeviceToHost));
    if (refused) {
        HIPCHK(hipMemset(c->sticky.as<unsigned>() + 1, 0, sizeof refused));
        return fail(STMPC_EINVAL, "finer_fit: a fine grid longer than STMPC_QP_NMAX samples is not supported (speed = NaN, fine_len = -1 for those states)");
    }
    return STMPC_OK;
}

int stmpc_st_control_groups_device(stmpc_ctx *c, const stmpc_params *groups, int G, int n_per_group, double tick, int N, int Kmax, const double *d_ego,
                                   const int32_t *d_k, const double *d_ox, const double *d_ov, int32_t *d_path, int32_t *d_bt, double *d_cost,
                                   double *d_speed, double *d_fine, int32_t *d_fine_len, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    SolverGroupsHost sg;
    TRY(solver_groups_of(groups, G, n_per_group, N, &sg));
    return st_control_device(c, &groups[0], tick, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_speed, d_fine, d_fine_len, stream,
                             c->sticky.as<unsigned>() + 1, &sg);
}

}  // extern "C"

namespace {
int make_ccfg(const stmpc_params *p, const stmpc_combined_cfg *g, CCfg *c) {
    if (!p || !g) return fail(STMPC_EINVAL, "params / combined cfg is NULL");
    if (!(g->tick_length > 0)) return fail(STMPC_EINVAL, "tick_length must be positive");
    memset(c, 0, sizeof *c);
    c->tick = g->tick_length; c->comb_min_dist = p->comb_min_dist; c->stop_x = g->stop_x;
    c->a_max = p->a_max; c->a_min = p->a_min; c->v_max = p->v_max; c->desired_speed = p->v_des;
    c->rollout_length = g->rollout_length > 1 ? g->rollout_length : 1;            // max(ROLLOUT_LENGTH, 1), dqn.py:129
    c->st_test_rollouts = g->st_test_rollouts; c->check_rollout_crash = g->check_rollout_crash; c->limit_speed = g->limit_dqn_speed;
    c->test_rollout_state = g->test_rollout_state; c->strictly_better = g->test_st_strictly_better; c->remember_last = g->remember_last_choice;
    if (c->rollout_length > STMPC_ROLLOUT_LIMIT) return fail(STMPC_EINVAL, "rollout_length above STMPC_ROLLOUT_LIMIT");
    return STMPC_OK;
}
// the policy's state vector: checked and converted (stmpc_policy_features_device, stmpc_actor_eval_device, the environment's observation)
int make_featcfg(const stmpc_policy_features_cfg *f, FeatCfg *fc) {
    if (f->cars_ahead < 0 || f->cars_behind < 0 || f->cars_ahead > STMPC_KMAX_LIMIT || f->cars_behind > STMPC_KMAX_LIMIT) return fail(STMPC_EINVAL, "cars_ahead / cars_behind out of range");
    if (f->normalize && (!(f->max_speed > 0) || !(f->sensor_radius > 0))) return fail(STMPC_EINVAL, "max_speed and sensor_radius must be positive");
    memset(fc, 0, sizeof *fc);
    fc->max_speed = f->max_speed; fc->sensor_radius = f->sensor_radius; fc->time_scale = (float)f->time_scale;
    fc->cars_ahead = f->cars_ahead; fc->cars_behind = f->cars_behind; fc->use_accel = f->use_acceleration != 0; fc->use_speed_diff = f->use_speed_difference != 0;
    fc->normalize = f->normalize != 0; fc->time_feature = f->time_feature != 0;
    return STMPC_OK;
}
}  // namespace

// (declared in stmpc_host.hpp: the actor population of stmpc_learner.hip asks too)
// later rollout steps: only states whose rollout is still going on are evaluated by the reference (dqn.py:129-133); *live = NULL at step 1
int rollout_live(const stmpc_ctx *c, int N, int step, const int **live) {
    *live = nullptr;
    if (step > 1) {
        if (c->cc.N != N) return fail(STMPC_EINVAL, "step > 1 without a rollout of this size in the context (stmpc_rollout_step_device)");
        *live = c->cc.grouped ? c->cc.ask.as<int>() : c->cc.live.as<int>();      // (a grouped rollout: not past the row's own group's last step either)
    }
    return STMPC_OK;
}

namespace {
// pointer checks of the two rollout step entries
int rollout_step_ptrs(int Kmax, const double *d_ego5_start, const double *d_cur_ego4, const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov,
                      const double *d_action) {
    if (!d_ego5_start || !d_cur_ego4 || !d_k || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    if (Kmax > 0 && (!d_cur_ox || !d_cur_ov)) return fail(STMPC_EINVAL, "NULL device pointer (vehicles)");
    return STMPC_OK;
}

// The shield controllers' step "st.do_st_control of the start states": the commands into b.speed / b.fine / b.fine_len (paths into b.path, b.bt, b.cost).
// Dense: every row, fully asynchronous.  Sparse: the reference solves the start state only where control is handed over (dqn.py:144-155, st.py:808: a few
// per cent of the ticks), so `select(sel_idx, sel_count)` launches the caller's ordered compaction of those rows, ONE host round trip fetches their number M,
// the controller runs on the compact batch and the commands are scattered back; a row that keeps its proposal has speed NaN and fine_len 0.  b.fine is
// the caller's to zero if its decide kernel reads it; `solves` is its control_solves counter, `who` its name in the error text.
template <class Select>
int shield_control(stmpc_ctx *c, const stmpc_params *p, double tick, int N, int Kmax, const double *d_ego5, const int32_t *d_k, const double *d_ox,
                   const double *d_ov, stmpc_ctx::ShieldBufs &b, hipStream_t st_, bool sparse, Select &&select, int64_t &solves, const char *who) {
    if (!sparse) {
        solves += N;
        return st_control_device(c, p, tick, N, Kmax, d_ego5, d_k, d_ox, d_ov, b.path.as<int32_t>(), b.bt.as<int32_t>(), b.cost.as<double>(), b.speed.as<double>(),
                                 b.fine.as<double>(), b.fine_len.as<int32_t>(), st_, nullptr);
    }
    const size_t n = (size_t)N;
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    if (!b.host_count) HIPCHK(hipHostMalloc((void **)&b.host_count, 4, hipHostMallocDefault));
    HIPCHK(hipMemsetAsync(b.speed.p, 0xFF, n * 8, st_));            // NaN: no controller command exists for a row that keeps its proposal
    HIPCHK(hipMemsetAsync(b.fine_len.p, 0, n * 4, st_));
    select(b.sel_idx.as<int>(), b.sel_count.as<int>());
    HIPCHK(hipMemcpyAsync(b.host_count, b.sel_count.p, 4, hipMemcpyDeviceToHost, st_));
    HIPCHK(hipStreamSynchronize(st_));
    const int M = *b.host_count;
    if (M < 0 || M > N) return fail(STMPC_EINTERNAL, std::string(who) + ": selection count out of range");
    solves += M;
    if (M == 0) return STMPC_OK;
    const int mb = (M + 63) / 64;
    hipLaunchKernelGGL(k_cc_gather, dim3(mb), dim3(64), 0, st_, M, Kalloc, Kmax, (const int *)b.sel_idx.as<int>(), d_ego5, d_k, d_ox, d_ov, b.c_ego.as<double>(),
                       b.c_k.as<int>(), b.c_ox.as<double>(), b.c_ov.as<double>());
    HIPCHK(hipMemsetAsync(b.c_fine.p, 0, (size_t)M * STMPC_QP_NMAX * 8, st_));
    TRY(st_control_device(c, p, tick, M, Kalloc, b.c_ego.as<double>(), b.c_k.as<int32_t>(), b.c_ox.as<double>(), b.c_ov.as<double>(), b.path.as<int32_t>(),
                          b.bt.as<int32_t>(), b.cost.as<double>(), b.c_speed.as<double>(), b.c_fine.as<double>(), b.c_fine_len.as<int32_t>(), st_, nullptr));
    hipLaunchKernelGGL(k_cc_scatter, dim3(mb), dim3(64), 0, st_, M, (const int *)b.sel_idx.as<int>(), (const double *)b.c_speed.as<double>(),
                       (const double *)b.c_fine.as<double>(), (const int *)b.c_fine_len.as<int>(), STMPC_QP_NMAX, b.speed.as<double>(), b.fine.as<double>(),
                       b.fine_len.as<int>());
    return STMPC_OK;
}

// the decision's buffers for N states of Kalloc vehicle slots and H layers (grow-only: a no-op once they hold the shape)
int combined_ensure(stmpc_ctx *c, int N, int Kalloc, int H, bool sparse) {
    const size_t n = (size_t)N;
    auto &b = c->cc;
    TRY(b.probe_ego.ensure(n * 5 * 8)); TRY(b.probe_ox.ensure(n * Kalloc * 8)); TRY(b.probe_ov.ensure(n * Kalloc * 8));
    TRY(b.sh.ensure(N, H));
    if (sparse) TRY(b.sh.ensure_compact(N, Kalloc));
    return STMPC_OK;
}

// A tick of the combined controller once the entry has checked its arguments and the rollout in the context: probe, controller, decision.  `n_test`: the
// rows that probe their rolled-out state -- none, all, or those of the context's static list test_idx (controller groups).  `select` is shield_control's,
// `decide()` launches the entry's decide kernel on what the two steps left in c->cc.sh.
template <class Select, class Decide>
int combined_decide(stmpc_ctx *c, const stmpc_params *p, int H, double tick, bool sparse, int n_test, int N, int Kmax, const double *d_ego5_start,
                    const int32_t *d_k, const double *d_ox_start, const double *d_ov_start, const double *d_cur_ego4, const double *d_cur_ox,
                    const double *d_cur_ov, hipStream_t st_, Select &&select, Decide &&decide) {
    auto &b = c->cc;
    auto &o = b.sh;
    const size_t n = (size_t)N;
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    TRY(combined_ensure(c, N, Kalloc, H, sparse));
    HIPCHK(hipMemsetAsync(o.pcrash.p, 0, n * 4, st_));
    // 1. feasibility probe of the rolled-out state (st.test_guaranteed_crash_from_state, dqn.py:152): one batched solve, of the rows that test only (a lone
    //    run of a group that does not test never calls the solver for them)
    if (n_test > 0) {
        hipLaunchKernelGGL(k_cc_probe_state, dim3((N + 63) / 64), dim3(64), 0, st_, N, Kalloc, Kmax, d_k, d_cur_ego4, d_cur_ox, d_cur_ov, b.state(),
                           b.probe_ego.as<double>(), b.probe_ox.as<double>(), b.probe_ov.as<double>());
        if (n_test == N) {
            TRY(stmpc_solve_batch_device(c, p, N, Kmax, b.probe_ego.as<double>(), d_k, b.probe_ox.as<double>(), b.probe_ov.as<double>(), o.path.as<int32_t>(),
                                         o.bt.as<int32_t>(), o.cost.as<double>(), nullptr, o.pcrash.as<int32_t>(), st_));
        } else {
            const int M = n_test, mb = (M + 63) / 64;
            hipLaunchKernelGGL(k_cc_gather, dim3(mb), dim3(64), 0, st_, M, Kalloc, Kalloc, (const int *)b.test_idx.as<int>(), (const double *)b.probe_ego.as<double>(), d_k,
                               (const double *)b.probe_ox.as<double>(), (const double *)b.probe_ov.as<double>(), o.c_ego.as<double>(), o.c_k.as<int>(),
                               o.c_ox.as<double>(), o.c_ov.as<double>());
            TRY(stmpc_solve_batch_device(c, p, M, Kalloc, o.c_ego.as<double>(), o.c_k.as<int32_t>(), o.c_ox.as<double>(), o.c_ov.as<double>(), o.path.as<int32_t>(),
                                         o.bt.as<int32_t>(), o.cost.as<double>(), nullptr, b.c_pcrash.as<int32_t>(), st_));
            hipLaunchKernelGGL(k_cc_scatter_flag, dim3(mb), dim3(64), 0, st_, M, (const int *)b.test_idx.as<int>(), (const int *)b.c_pcrash.as<int>(), o.pcrash.as<int>());
        }
    }
    // 2. the controller on the start state (st.do_st_control; also the path of the strictly-better comparison, dqn.py:157-164, which needs every row's)
    HIPCHK(hipMemsetAsync(o.fine.p, 0, n * STMPC_QP_NMAX * 8, st_));          // (k_cc_decide* read the fine path)
    b.ticks += N;
    TRY(shield_control(c, p, tick, N, Kmax, d_ego5_start, d_k, d_ox_start, d_ov_start, o, st_, sparse, select, b.control_solves, "combined controller"));
    // 3. the decision
    decide();
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

// stmpc_rollout_step_device after its argument checks (N >= 1): the entry's body, shared with stmpc_cshield_env_step_device
int rollout_step_run(stmpc_ctx *c, const stmpc_params *p, const stmpc_combined_cfg *g, int N, int Kmax, int step, const double *d_ego5_start, double *d_cur_ego4,
                     const int32_t *d_k, double *d_cur_ox, double *d_cur_ov, double *d_cur_oa, const double *d_action, void *stream) {
    HIPCHK(hipSetDevice(c->device));
    DevP dp; CCfg cc;
    TRY(make_devp(p, &dp));
    TRY(make_ccfg(p, g, &cc));
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    if (step == 1) { TRY(c->cc.ensure(N, Kalloc, cc.rollout_length)); c->cc.grouped = false; }
    else if (c->cc.grouped || c->cc.N != N || c->cc.K != Kalloc || c->cc.R != cc.rollout_length) return fail(STMPC_EINVAL, "rollout step > 1 does not continue the rollout begun with step 1");
    CCState st = c->cc.state();
    with_kmax(Kalloc, [&](auto km) {
        hipLaunchKernelGGL(k_rollout_step<decltype(km)::value>, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, dp, cc, N, Kalloc, step, d_ego5_start, d_cur_ego4,
                           d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_action, st);
    });
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

// stmpc_combined_decide_device after its argument checks (N >= 1): the entry's body, shared with stmpc_cshield_env_step_device
int combined_decide_run(stmpc_ctx *c, const stmpc_params *p, const stmpc_combined_cfg *g, int N, int Kmax, const double *d_ego5_start, const int32_t *d_k,
                        const double *d_ox_start, const double *d_ov_start, const double *d_cur_ego4, const double *d_cur_ox, const double *d_cur_ov,
                        const double *d_first_action, const int32_t *d_last_choice_rl, int32_t *d_takeover, int32_t *d_reason, double *d_speed, void *stream) {
    HIPCHK(hipSetDevice(c->device));
    CCfg cc;
    TRY(make_ccfg(p, g, &cc));
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    auto &b = c->cc;
    if (b.grouped || b.N != N || b.K != Kalloc || b.R != cc.rollout_length) return fail(STMPC_EINVAL, "no rollout of this shape in the context (call stmpc_rollout_step_device first)");
    int H;
    TRY(num_layers(p, &H));
    hipStream_t st_ = (hipStream_t)stream;
    const CCState st = b.state();
    const auto &o = b.sh;
    // (sparse: not with the strictly-better comparison, which needs every row's path)
    return combined_decide(
        c, p, H, g->tick_length, g->sparse_control && !cc.strictly_better, cc.test_rollout_state ? N : 0, N, Kmax, d_ego5_start, d_k, d_ox_start, d_ov_start,
        d_cur_ego4, d_cur_ox, d_cur_ov, st_,
        [&](int *sel_idx, int *sel_count) {
            hipLaunchKernelGGL(k_cc_select, dim3(1), dim3(1024), 0, st_, cc, N, st, (const int *)o.pcrash.as<int>(), sel_idx, sel_count);
        },
        [&] {
            hipLaunchKernelGGL(k_cc_decide, dim3((N + 63) / 64), dim3(64), 0, st_, cc, N, d_ego5_start, d_first_action, d_last_choice_rl, st,
                               (const int *)o.pcrash.as<int>(), (const double *)o.speed.as<double>(), (const double *)o.fine.as<double>(),
                               (const int *)o.fine_len.as<int>(), STMPC_QP_NMAX, d_takeover, d_reason, d_speed, c->sticky.as<unsigned>() + 1);
        });
}
}  // namespace

extern "C" {

int stmpc_rollout_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_combined_cfg *g, int N, int Kmax, int step,
                              const double *d_ego5_start, double *d_cur_ego4, const int32_t *d_k, double *d_cur_ox, double *d_cur_ov,
                              double *d_cur_oa, const double *d_action, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N < 0 || Kmax < 0 || Kmax > STMPC_KMAX_LIMIT || step < 1) return fail(STMPC_EINVAL, "N, Kmax or step out of range");
    if (N == 0) return STMPC_OK;
    TRY(rollout_step_ptrs(Kmax, d_ego5_start, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_action));
    return rollout_step_run(c, p, g, N, Kmax, step, d_ego5_start, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_action, stream);
}

int stmpc_policy_features_device(stmpc_ctx *c, const stmpc_policy_features_cfg *f, int N, int Kmax, int step, const double *d_cur_ego4, const int32_t *d_k,
                                 const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, int32_t *d_evals, float *d_feat, int feat_stride, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!f) return fail(STMPC_EINVAL, "features cfg is NULL");
    if (N < 0 || Kmax < 0 || Kmax > STMPC_KMAX_LIMIT || step < 1) return fail(STMPC_EINVAL, "N, Kmax or step out of range");
    FeatCfg fc;
    TRY(make_featcfg(f, &fc));
    if (feat_stride < stmpc_policy_features_len(f)) return fail(STMPC_EINVAL, "feat_stride is shorter than the feature vector");
    if (N == 0) return STMPC_OK;
    if (!d_cur_ego4 || !d_k || !d_feat) return fail(STMPC_EINVAL, "NULL device pointer");
    if (Kmax > 0 && (!d_cur_ox || !d_cur_ov)) return fail(STMPC_EINVAL, "NULL device pointer (vehicles)");
    if (f->time_feature && !d_evals) return fail(STMPC_EINVAL, "time_feature needs the evaluation counters");
    const int *live;
    TRY(rollout_live(c, N, step, &live));
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_policy_features, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, fc, N, Kmax, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, live,
                       d_evals, d_feat, feat_stride);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_policy_features_len(const stmpc_policy_features_cfg *f) {
    if (!f) return 0;
    return (f->cars_ahead + f->cars_behind) * (f->use_acceleration ? 4 : 3) + 4 + (f->time_feature ? 1 : 0);
}

}  // extern "C"

// ---- the policy network itself (optional: the caller may keep it in its own framework and only use stmpc_policy_features_device) ----
// (struct stmpc_actor: stmpc_host.hpp, with the declarations of what stmpc_learner.hip calls of this section)
namespace {
// [column tile][k block][lane = j + 16 kk][4]: W[n0 + j][k0 + 4 kk + s], zero outside [rows) x [cols)
std::vector<float> pack_layer(const float *W, int rows, int cols, int rows_p, int cols_p) {
    std::vector<float> out((size_t)rows_p * cols_p, 0.f);
    const int kblocks = cols_p / 16;
    for (int nt = 0; nt < rows_p / 16; ++nt)
        for (int kb = 0; kb < kblocks; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int q = 0; q < 4; ++q) {
                    const int n = nt * 16 + (lane & 15), k = kb * 16 + 4 * (lane >> 4) + q;
                    if (n < rows && k < cols) out[(((size_t)nt * kblocks + kb) * 64 + lane) * 4 + q] = W[(size_t)n * cols + k];
                }
    return out;
}
int upload(DevBuf &b, const std::vector<float> &v) { return upload(b, v.data(), v.size()); }
}  // namespace

size_t actor_lds_bytes(int h1p, int h2p) { return ((size_t)AT_TM * AT_KIN + (size_t)AT_TM * (h1p + 4) + (size_t)AT_TM * (h2p + 4)) * sizeof(float); }
// (stmpc_host.hpp: the attribute is only ever raised)
int raise_dynamic_lds(const void *fn, const char *kernel, LdsCeiling &ceiling, int device, size_t lds) {
    size_t &lds_max = ceiling.max[(unsigned)device & 15u];
    if (lds > 48 * 1024 && lds > lds_max) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return fail(STMPC_EHIP, std::string("hipFuncSetAttribute(") + kernel + ", dynamic LDS) failed");
        }
        lds_max = lds;
    }
    return STMPC_OK;
}
// dynamic LDS of k_actor_eval (which = 0) / k_actor_eval_pop (1)
int actor_raise_lds(int which, int device, size_t lds) {
    static LdsCeiling ceiling[2];
    return which ? raise_dynamic_lds((const void *)k_actor_eval_pop, "k_actor_eval_pop", ceiling[1], device, lds)
                 : raise_dynamic_lds((const void *)k_actor_eval, "k_actor_eval", ceiling[0], device, lds);
}
// the argument checks stmpc_actor_eval_device and stmpc_actor_pop_eval_device share; N: all rows of the call
int actor_eval_checks(const stmpc_ctx *c, int device, int n_in, const stmpc_policy_features_cfg *f, int N, int Kmax, int step, const double *d_cur_ego4,
                      const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const int32_t *d_evals, const float *d_feat, int feat_stride,
                      const double *d_jerk, FeatCfg *fc) {
    if (device != c->device) return fail(STMPC_EINVAL, "actor and context are on different devices");
    if (N < 0 || Kmax < 0 || Kmax > STMPC_KMAX_LIMIT || step < 1) return fail(STMPC_EINVAL, "N, Kmax or step out of range");
    TRY(make_featcfg(f, fc));
    if (stmpc_policy_features_len(f) != n_in) return fail(STMPC_EINVAL, "the actor's input width is not the length of this state vector");
    if (d_feat && feat_stride < n_in) return fail(STMPC_EINVAL, "feat_stride is shorter than the feature vector");
    if (N == 0) return STMPC_OK;
    if (!d_cur_ego4 || !d_k || !d_jerk) return fail(STMPC_EINVAL, "NULL device pointer");
    if (Kmax > 0 && (!d_cur_ox || !d_cur_ov)) return fail(STMPC_EINVAL, "NULL device pointer (vehicles)");
    if (f->time_feature && !d_evals) return fail(STMPC_EINVAL, "time_feature needs the evaluation counters");
    return STMPC_OK;
}

namespace {
// stmpc_actor_eval_device after its argument checks (N >= 1): the entry's body, shared with stmpc_cshield_env_step_device
int actor_eval_run(stmpc_ctx *c, const stmpc_actor *a, const FeatCfg &fc, int N, int Kmax, int step, const double *d_cur_ego4, const int32_t *d_k,
                   const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, int32_t *d_evals, float *d_feat, int feat_stride, double *d_jerk,
                   void *stream) {
    const int *live;
    TRY(rollout_live(c, N, step, &live));
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_actor_eval, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), a->lds, (hipStream_t)stream, fc, a->dev, N, Kmax, d_cur_ego4, d_k, d_cur_ox, d_cur_ov,
                       d_cur_oa, live, d_evals, d_feat, feat_stride, d_jerk);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
}  // namespace

extern "C" {

int stmpc_actor_create(stmpc_ctx *c, int n_in, int h1, int h2, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                       const float *b2, double tanh_scale, double tanh_mean, stmpc_actor **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (!w0 || !b0 || !w1 || !b1 || !w2 || !b2) return fail(STMPC_EINVAL, "NULL weight pointer");
    if (n_in < 1 || n_in > AT_KIN || h1 < 1 || h1 > 1024 || h2 < 1 || h2 > 1024) return fail(STMPC_EINVAL, "actor shape out of range (n_in <= 32, hidden widths <= 1024)");
    HIPCHK(hipSetDevice(c->device));
    const int h1p = (h1 + 15) & ~15, h2p = (h2 + 15) & ~15;
    const size_t lds = actor_lds_bytes(h1p, h2p);
    if (lds + 1024 > (size_t)c->lds_per_block) return fail(STMPC_EINVAL, "actor too wide for one workgroup's LDS");
    stmpc_actor *a = new stmpc_actor();
    a->device = c->device; a->lds = lds;
    std::vector<float> vb0(h1p, 0.f), vb1(h2p, 0.f), vw2(h2p, 0.f), vb2(1, b2[0]);
    for (int i = 0; i < h1; ++i) vb0[i] = b0[i];
    for (int i = 0; i < h2; ++i) { vb1[i] = b1[i]; vw2[i] = w2[i]; }
    int rc;
    if ((rc = upload(a->p0, pack_layer(w0, h1, n_in, h1p, AT_KIN))) || (rc = upload(a->b0, vb0)) || (rc = upload(a->p1, pack_layer(w1, h2, h1, h2p, h1p))) ||
        (rc = upload(a->b1, vb1)) || (rc = upload(a->w2, vw2)) || (rc = upload(a->b2, vb2))) { stmpc_actor_destroy(a); return rc; }
    a->dev.p0 = a->p0.as<float>(); a->dev.b0 = a->b0.as<float>(); a->dev.p1 = a->p1.as<float>(); a->dev.b1 = a->b1.as<float>(); a->dev.w2 = a->w2.as<float>();
    a->dev.b2p = a->b2.as<float>(); a->dev.scale = (float)tanh_scale; a->dev.mean = (float)tanh_mean; a->dev.n_in = n_in; a->dev.h1p = h1p; a->dev.h2p = h2p;
    if ((rc = actor_raise_lds(0, c->device, lds))) { stmpc_actor_destroy(a); return rc; }
    *out = a;
    return STMPC_OK;
}

void stmpc_actor_destroy(stmpc_actor *a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    delete a;
}

int stmpc_actor_eval_device(stmpc_ctx *c, const stmpc_actor *a, const stmpc_policy_features_cfg *f, int N, int Kmax, int step, const double *d_cur_ego4,
                            const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, int32_t *d_evals, float *d_feat,
                            int feat_stride, double *d_jerk, void *stream) {
    if (!c || !a || !f) return fail(STMPC_EINVAL, "NULL argument");
    FeatCfg fc;
    TRY(actor_eval_checks(c, a->device, a->dev.n_in, f, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_evals, d_feat, feat_stride, d_jerk, &fc));
    if (N == 0) return STMPC_OK;
    return actor_eval_run(c, a, fc, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_evals, d_feat, feat_stride, d_jerk, stream);
}

int stmpc_combined_counts(stmpc_ctx *c, int64_t *decisions, int64_t *control_solves, int reset) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (decisions) *decisions = c->cc.ticks;
    if (control_solves) *control_solves = c->cc.control_solves;
    if (reset) { c->cc.ticks = 0; c->cc.control_solves = 0; }
    return STMPC_OK;
}

int stmpc_combined_decide_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_combined_cfg *g, int N, int Kmax,
                                 const double *d_ego5_start, const int32_t *d_k, const double *d_ox_start, const double *d_ov_start,
                                 const double *d_cur_ego4, const double *d_cur_ox, const double *d_cur_ov, const double *d_first_action,
                                 const int32_t *d_last_choice_rl, int32_t *d_takeover, int32_t *d_reason, double *d_speed, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!p || !g) return fail(STMPC_EINVAL, "NULL parameter struct");
    TRY(check_batch(N, Kmax));
    if (N == 0) return STMPC_OK;
    if (!d_ego5_start || !d_k || !d_cur_ego4 || !d_first_action || !d_takeover || !d_reason || !d_speed) return fail(STMPC_EINVAL, "NULL device pointer");
    if (Kmax > 0 && (!d_ox_start || !d_ov_start || !d_cur_ox || !d_cur_ov)) return fail(STMPC_EINVAL, "NULL device pointer (vehicles)");
    return combined_decide_run(c, p, g, N, Kmax, d_ego5_start, d_k, d_ox_start, d_ov_start, d_cur_ego4, d_cur_ox, d_cur_ov, d_first_action, d_last_choice_rl,
                               d_takeover, d_reason, d_speed, stream);
}

// ---- controller groups (stmpc_cc_groups_kernels.hpp) ----
int stmpc_combined_groups_set(stmpc_ctx *c, const stmpc_params *p, const stmpc_combined_cfg *cfgs, int C, int n_per_group) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!p || !cfgs) return fail(STMPC_EINVAL, "params / combined cfgs is NULL");
    TRY(check_group_counts(C, n_per_group, STMPC_SIM_GROUPS_MAX, "C must be 1 ... STMPC_SIM_GROUPS_MAX (64) controller groups", "C"));
    std::vector<CCfg> table((size_t)C);
    for (int g = 0; g < C; ++g) TRY(make_ccfg(p, &cfgs[g], &table[g]));
    for (int g = 1; g < C; ++g) {
        const stmpc_combined_cfg &a = cfgs[0], &b = cfgs[g];
        const Share share{"controller groups", "group", g, ""};
        SHARED(tick_length); SHARED(stop_x); SHARED(sparse_control);
    }
    // the rows of the groups that probe their rolled-out state: a static list, so a tick needs no round trip to gather them
    std::vector<int> test_rows;
    int Rmax = 1, any_strict = 0;
    for (int g = 0; g < C; ++g) {
        Rmax = table[g].rollout_length > Rmax ? table[g].rollout_length : Rmax;
        any_strict |= table[g].strictly_better != 0;
        if (table[g].test_rollout_state) for (int e = 0; e < n_per_group; ++e) test_rows.push_back(g * n_per_group + e);
    }
    HIPCHK(hipSetDevice(c->device));
    auto &b = c->cc;
    TRY(b.groups.ensure(table.size() * sizeof(CCfg)));
    TRY(b.test_idx.ensure((test_rows.size() + 1) * 4));
    b.drop_grouped();
    b.C = 0;
    HIPCHK(hipMemcpy(b.groups.p, table.data(), table.size() * sizeof(CCfg), hipMemcpyHostToDevice));      // (synchronous: table and test_rows are locals)
    if (!test_rows.empty()) HIPCHK(hipMemcpy(b.test_idx.p, test_rows.data(), test_rows.size() * 4, hipMemcpyHostToDevice));
    b.table = std::move(table);
    b.C = C; b.n_per_group = n_per_group; b.Rmax = Rmax; b.n_test = (int)test_rows.size(); b.any_strict = any_strict;
    b.sparse = cfgs[0].sparse_control != 0; b.tick = cfgs[0].tick_length;
    return STMPC_OK;
}

int stmpc_combined_groups_clear(stmpc_ctx *c) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    auto &b = c->cc;
    b.drop_grouped();
    b.C = 0; b.n_per_group = 0; b.Rmax = 0; b.n_test = 0; b.any_strict = 0; b.table.clear();
    return STMPC_OK;
}

int stmpc_rollout_step_groups_device(stmpc_ctx *c, const stmpc_params *p, int N, int Kmax, int step, const double *d_ego5_start, double *d_cur_ego4,
                                     const int32_t *d_k, double *d_cur_ox, double *d_cur_ov, double *d_cur_oa, const double *d_action, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N < 0 || Kmax < 0 || Kmax > STMPC_KMAX_LIMIT || step < 1) return fail(STMPC_EINVAL, "N, Kmax or step out of range");
    auto &b = c->cc;
    if (b.C < 1) return fail(STMPC_EINVAL, "the context has no controller groups (stmpc_combined_groups_set): use the plain rollout entry");
    if ((int64_t)N != (int64_t)b.C * b.n_per_group) return fail(STMPC_EINVAL, "N does not match stmpc_combined_groups_set (C * n_per_group)");
    TRY(rollout_step_ptrs(Kmax, d_ego5_start, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_action));
    DevP dp;
    TRY(make_devp(p, &dp));
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    if (step > 1 && (!b.grouped || b.N != N || b.K != Kalloc || b.R != b.Rmax)) return fail(STMPC_EINVAL, "rollout step > 1 does not continue the grouped rollout begun with step 1");
    HIPCHK(hipSetDevice(c->device));
    if (step == 1) {
        TRY(b.ask.ensure((size_t)N * 4));
        TRY(b.ensure(N, Kalloc, b.Rmax));
        b.grouped = true;
    }
    CCState st = b.state();
    with_kmax(Kalloc, [&](auto km) {
        hipLaunchKernelGGL(k_rollout_step_groups<decltype(km)::value>, dim3((b.n_per_group + 63) / 64, b.C), dim3(64), 0, (hipStream_t)stream, dp,
                           (const CCfg *)b.groups.as<CCfg>(), b.n_per_group, Kalloc, step, b.Rmax + 1, d_ego5_start, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_action,
                           st, b.ask.as<int>());
    });
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_combined_decide_groups_device(stmpc_ctx *c, const stmpc_params *p, int N, int Kmax, const double *d_ego5_start, const int32_t *d_k,
                                        const double *d_ox_start, const double *d_ov_start, const double *d_cur_ego4, const double *d_cur_ox,
                                        const double *d_cur_ov, const double *d_first_action, const int32_t *d_last_choice_rl, int32_t *d_takeover,
                                        int32_t *d_reason, double *d_speed, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!p) return fail(STMPC_EINVAL, "NULL parameter struct");
    TRY(check_batch(N, Kmax));
    auto &b = c->cc;
    if (b.C < 1) return fail(STMPC_EINVAL, "the context has no controller groups (stmpc_combined_groups_set): use the plain decide entry");
    if ((int64_t)N != (int64_t)b.C * b.n_per_group) return fail(STMPC_EINVAL, "N does not match stmpc_combined_groups_set (C * n_per_group)");
    if (!d_ego5_start || !d_k || !d_cur_ego4 || !d_first_action || !d_takeover || !d_reason || !d_speed) return fail(STMPC_EINVAL, "NULL device pointer");
    if (Kmax > 0 && (!d_ox_start || !d_ov_start || !d_cur_ox || !d_cur_ov)) return fail(STMPC_EINVAL, "NULL device pointer (vehicles)");
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    if (!b.grouped || b.N != N || b.K != Kalloc || b.R != b.Rmax) return fail(STMPC_EINVAL, "no grouped rollout of this shape in the context (call stmpc_rollout_step_groups_device first)");
    int H;
    TRY(num_layers(p, &H));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st_ = (hipStream_t)stream;
    auto &o = b.sh;
    // (the compact batch serves the probe's gather too, so it exists in a dense run as well)
    TRY(o.ensure_compact(N, Kalloc)); TRY(b.c_pcrash.ensure((size_t)N * 4));
    const CCState st = b.state();
    const CCfg *groups = b.groups.as<CCfg>();
    const int npg = b.n_per_group;
    // (sparse as the plain entry unless a group compares paths: then every row's path is needed and the run is dense)
    return combined_decide(
        c, p, H, b.tick, b.sparse && !b.any_strict, b.n_test, N, Kmax, d_ego5_start, d_k, d_ox_start, d_ov_start, d_cur_ego4, d_cur_ox, d_cur_ov, st_,
        [&](int *sel_idx, int *sel_count) {
            hipLaunchKernelGGL(k_cc_select_groups, dim3(1), dim3(1024), 0, st_, groups, npg, N, st, (const int *)o.pcrash.as<int>(), sel_idx, sel_count);
        },
        [&] {
            hipLaunchKernelGGL(k_cc_decide_groups, dim3((npg + 63) / 64, b.C), dim3(64), 0, st_, groups, npg, b.Rmax + 1, d_ego5_start, d_first_action,
                               d_last_choice_rl, st, (const int *)o.pcrash.as<int>(), (const double *)o.speed.as<double>(), (const double *)o.fine.as<double>(),
                               (const int *)o.fine_len.as<int>(), STMPC_QP_NMAX, d_takeover, d_reason, d_speed, c->sticky.as<unsigned>() + 1);
        });
}

int stmpc_combined_read_state(stmpc_ctx *c, int N, int32_t *live, int32_t *hist_len, int32_t *crash_pred, double *sel_speed, double *rollout_s,
                              int32_t *have_test, double *test_ego4, double *test_ox, double *test_ov, int32_t *probe_crash, double *st_speed,
                              double *fine, int32_t *fine_len) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    const auto &b = c->cc;
    if (N != b.N) return fail(STMPC_EINVAL, "no rollout of this size in the context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t n = (size_t)N, K = b.K, R1 = b.R + 1;
    TRY(download(live, b.live, n)); TRY(download(hist_len, b.hist_len, n)); TRY(download(crash_pred, b.crash_pred, n)); TRY(download(sel_speed, b.sel, n));
    TRY(download(rollout_s, b.rollout_s, n * R1)); TRY(download(have_test, b.have_test, n)); TRY(download(test_ego4, b.test_ego, n * 4));
    TRY(download(test_ox, b.test_ox, n * K)); TRY(download(test_ov, b.test_ov, n * K));
    // (the decision's buffers exist once stmpc_combined_decide_device has run)
    if (b.sh.pcrash.p) TRY(download(probe_crash, b.sh.pcrash, n));
    if (b.sh.speed.p) TRY(download(st_speed, b.sh.speed, n));
    if (b.sh.fine.p) TRY(download(fine, b.sh.fine, n * STMPC_QP_NMAX));
    if (b.sh.fine_len.p) TRY(download(fine_len, b.sh.fine_len, n));
    return stmpc_check_error(c);         // (device already synchronised: just the flags)
}

int stmpc_solve_grid_no_jerk(stmpc_ctx *c, int variant, const uint8_t *obstacles, const double *s_values, int S, const double *t_values,
                             int H, double ego_start_speed, const double *distances, double *s_sequence_out) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (variant != 0 && variant != 1) return fail(STMPC_EINVAL, "variant must be 0 (no_jerk_fast) or 1 (no_jerk_djikstra)");
    if (!obstacles || !s_values || !t_values || !distances || !s_sequence_out) return fail(STMPC_EINVAL, "NULL host pointer");
    if (bad_layers(H)) return fail(STMPC_EINVAL, "num_t must be in [2, 64]");
    if (S < 2 || S > STMPC_S_LIMIT) return fail(STMPC_EINVAL, "num_s must be in [2, 65000]");
    if (variant == 1 && (size_t)H * S * S > ((size_t)1 << 28)) return fail(STMPC_EINVAL, "no_jerk_djikstra keeps H*S*S node flags: lattice too large (H*S*S > 2^28)");
    if (t_values[1] - t_values[0] == 0.0) return fail(STMPC_EINVAL, "float division by zero (delta_t == 0)");
    if (s_values[1] - s_values[0] == 0.0) return fail(STMPC_EINVAL, "float division by zero (delta_s == 0)");
    HIPCHK(hipSetDevice(c->device));
    auto &s = c->s;
    const size_t cells = (size_t)H * S, states = variant ? cells * S : cells;
    size_t cap = states * 8;
    if (cap < ((size_t)1 << 20)) cap = (size_t)1 << 20;
    if (cap > ((size_t)1 << 25)) cap = (size_t)1 << 25;               // 32 M entries = 768 MB at most
    TRY(s.misc3.ensure((size_t)H * 8 + 16)); TRY(s.pd.ensure(states)); TRY(s.path.ensure(states * 4)); TRY(c->solver.gscratch.ensure(cap * sizeof(NjItem)));
    TRY(upload(s.misc0, obstacles, cells)); TRY(upload(s.misc1, distances, cells)); TRY(upload(s.misc2, s_values, (size_t)S));
    HIPCHK(hipMemset(s.pd.p, 0, states));
    HIPCHK(hipMemset(s.path.p, 0, states * 4));
    NjArgs a;
    memset(&a, 0, sizeof a);
    a.triple = variant; a.S = S; a.H = H; a.v0 = ego_start_speed;
    a.obstacles = s.misc0.as<uint8_t>(); a.distances = s.misc1.as<double>(); a.s_values = s.misc2.as<double>();
    a.dt = t_values[1] - t_values[0];
    a.enc = s.pd.as<uint8_t>(); a.prev = s.path.as<int>(); a.heap = c->solver.gscratch.as<NjItem>(); a.cap = cap;
    a.s_sequence = s.misc3.as<double>(); a.status = (int *)(s.misc3.as<double>() + H);
    hipLaunchKernelGGL(k_nojerk, dim3(1), dim3(64), 0, nullptr, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    int status = 0;
    TRY(download(s_sequence_out, s.misc3, (size_t)H));
    HIPCHK(hipMemcpy(&status, (char *)s.misc3.p + (size_t)H * 8, 4, hipMemcpyDeviceToHost));
    if (status == 1) return fail(STMPC_ENOMEM, "no-jerk solver: heap capacity exceeded");
    if (status == 2) return fail(STMPC_EINVAL, "index out of bounds: the first layer's reachable cells leave the grid (IndexError in the reference)");
    return STMPC_OK;
}

}  // extern "C"

// ---- first-step shield controller (stmpc_fs_kernels.hpp): st.do_conditional_st_based_on_first_step, st.py:805-814 ----
namespace {
// the checks of stmpc_first_step_device's cfg and batch shape (the shielded env's entries make them too, before anything changes)
int first_step_check(const stmpc_params *p, const stmpc_first_step_cfg *g, int N, int Kmax) {
    if (!p || !g) return fail(STMPC_EINVAL, "NULL parameter struct");
    if (!(g->tick_length > 0)) return fail(STMPC_EINVAL, "tick_length must be positive");
    if (!(g->min_crash_distance >= 0)) return fail(STMPC_EINVAL, "min_crash_distance must not be negative");
    return check_batch(N, Kmax);
}
// the controller's buffers for N states of Kalloc vehicle slots and H layers (grow-only: a no-op once they hold the shape)
int first_step_ensure(stmpc_ctx *c, int N, int Kalloc, int H, bool sparse) {
    const size_t n = (size_t)N;
    auto &b = c->fs;
    TRY(b.next_ego.ensure(n * 5 * 8)); TRY(b.next_ox.ensure(n * Kalloc * 8)); TRY(b.next_ov.ensure(n * Kalloc * 8)); TRY(b.crashed.ensure(n * 4));
    TRY(b.sh.ensure(N, H));
    if (sparse) TRY(b.sh.ensure_compact(N, Kalloc));
    if (!b.takeovers.p) { TRY(b.takeovers.ensure(8)); HIPCHK(hipMemset(b.takeovers.p, 0, 8)); }
    return STMPC_OK;
}
// stmpc_first_step_device after its argument checks (N >= 1): the entry's body, shared with stmpc_shield_env_step_device
int first_step_run(stmpc_ctx *c, const stmpc_params *p, const stmpc_first_step_cfg *g, int N, int Kmax, const double *d_ego5, const int32_t *d_k,
                   const double *d_ox, const double *d_ov, const double *d_start_speed, double *d_cmd_speed, int32_t *d_takeover, int32_t *d_reason,
                   void *stream) {
    HIPCHK(hipSetDevice(c->device));
    DevP dp;
    TRY(make_devp(p, &dp));
    const int H = dp.H;
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    hipStream_t st_ = (hipStream_t)stream;
    const size_t n = (size_t)N;
    auto &b = c->fs;
    auto &o = b.sh;
    TRY(first_step_ensure(c, N, Kalloc, H, g->sparse_control != 0));
    b.N = N; b.K = Kalloc;
    const int blocks = (N + 63) / 64;
    // 1. one predictor step with the proposed speed, laid out as the probe's state (st.py:806)
    with_kmax(Kalloc, [&](auto km) {
        hipLaunchKernelGGL(k_fs_step<decltype(km)::value>, dim3(blocks), dim3(64), 0, st_, dp, g->tick_length, g->min_crash_distance, N, Kmax, d_ego5, d_k, d_ox, d_ov,
                           d_start_speed, b.crashed.as<int>(), b.next_ego.as<double>(), b.next_ox.as<double>(), b.next_ov.as<double>());
    });
    HIPCHK(hipGetLastError());
    // 2. st.test_guaranteed_crash_from_state(next_state), st.py:807: one batched solve (the reference asks before it looks at `crashed`, so every state is solved)
    TRY(stmpc_solve_batch_device(c, p, N, Kmax, b.next_ego.as<double>(), d_k, b.next_ox.as<double>(), b.next_ov.as<double>(), o.path.as<int32_t>(),
                                 o.bt.as<int32_t>(), o.cost.as<double>(), nullptr, o.pcrash.as<int32_t>(), stream));
    // 3. st.do_st_control(state) of the START state, st.py:811; sparse: only for the states st.py:808 hands over.  k_fs_decide reads no fine path, so only
    //    the dense run, which fills every row's, clears them first
    b.decisions += N;
    if (!g->sparse_control) HIPCHK(hipMemsetAsync(o.fine.p, 0, n * STMPC_QP_NMAX * 8, st_));
    TRY(shield_control(
        c, p, g->tick_length, N, Kmax, d_ego5, d_k, d_ox, d_ov, o, st_, g->sparse_control != 0,
        [&](int *sel_idx, int *sel_count) {
            hipLaunchKernelGGL(k_fs_select, dim3(1), dim3(1024), 0, st_, N, (const int *)b.crashed.as<int>(), (const int *)o.pcrash.as<int>(), sel_idx, sel_count);
        },
        b.control_solves, "first-step controller"));
    // 4. the choice, st.py:808-814
    hipLaunchKernelGGL(k_fs_decide, dim3(blocks), dim3(64), 0, st_, N, d_start_speed, (const int *)b.crashed.as<int>(), (const int *)o.pcrash.as<int>(),
                       (const double *)o.speed.as<double>(), (const int *)o.fine_len.as<int>(), d_cmd_speed, d_takeover, d_reason,
                       b.takeovers.as<unsigned long long>(), c->sticky.as<unsigned>() + 1);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
}  // namespace

extern "C" {

int stmpc_first_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_first_step_cfg *g, int N, int Kmax, const double *d_ego5, const int32_t *d_k,
                            const double *d_ox, const double *d_ov, const double *d_oa, const double *d_start_speed, double *d_cmd_speed, int32_t *d_takeover,
                            int32_t *d_reason, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(first_step_check(p, g, N, Kmax));
    if (N == 0) return STMPC_OK;
    if (!d_ego5 || !d_k || !d_start_speed || !d_cmd_speed || !d_takeover || !d_reason) return fail(STMPC_EINVAL, "NULL device pointer");
    if (Kmax > 0 && (!d_ox || !d_ov)) return fail(STMPC_EINVAL, "NULL device pointer (vehicles)");
    (void)d_oa;                          // (prediction.py:75-97 reads no accelerations: the argument completes the planner's view, nothing more)
    return first_step_run(c, p, g, N, Kmax, d_ego5, d_k, d_ox, d_ov, d_start_speed, d_cmd_speed, d_takeover, d_reason, stream);
}

int stmpc_first_step(stmpc_ctx *c, const stmpc_params *p, const stmpc_first_step_cfg *g, int N, int Kmax, const double *ego, const int32_t *k, const double *ox,
                     const double *ov, const double *start_speed, double *cmd_speed, int32_t *takeover, int32_t *reason, int32_t *crashed,
                     int32_t *crash_guaranteed, double *next_ego, double *next_ox, double *next_ov) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(host_batch_begin(c, N, Kmax, ego, k, ox, ov, start_speed && cmd_speed && takeover && reason));
    if (N == 0) return STMPC_OK;
    auto &s = c->s;
    const size_t n = (size_t)N;
    TRY(s.states(N, Kmax, ego, 5, k, ox, ov));
    TRY(upload(s.misc0, start_speed, n));
    TRY(s.misc1.ensure(n * 8)); TRY(s.misc2.ensure(n * 4)); TRY(s.misc3.ensure(n * 4));
    TRY(stmpc_first_step_device(c, p, g, N, Kmax, s.ego.as<double>(), s.k.as<int32_t>(), s.ox.as<double>(), s.ov.as<double>(), nullptr, s.misc0.as<double>(),
                                s.misc1.as<double>(), s.misc2.as<int32_t>(), s.misc3.as<int32_t>(), nullptr));
    HIPCHK(hipDeviceSynchronize());
    const auto &b = c->fs;
    TRY(download(cmd_speed, s.misc1, n)); TRY(download(takeover, s.misc2, n)); TRY(download(reason, s.misc3, n));
    TRY(download(crashed, b.crashed, n)); TRY(download(crash_guaranteed, b.sh.pcrash, n)); TRY(download(next_ego, b.next_ego, n * 5));
    if (Kmax > 0) { TRY(download(next_ox, b.next_ox, n * Kmax)); TRY(download(next_ov, b.next_ov, n * Kmax)); }
    return stmpc_check_error(c);         // (this entry is synchronous: what its kernels flagged is its own error)
}

int stmpc_first_step_counts(stmpc_ctx *c, int64_t *decisions, int64_t *takeovers, int64_t *control_solves, int reset) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    auto &b = c->fs;
    unsigned long long t = 0;
    if (b.takeovers.p) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(&t, b.takeovers.p, sizeof t, hipMemcpyDeviceToHost));
        if (reset) HIPCHK(hipMemset(b.takeovers.p, 0, sizeof t));
    }
    if (decisions) *decisions = b.decisions;
    if (takeovers) *takeovers = (int64_t)t;
    if (control_solves) *control_solves = b.control_solves;
    if (reset) { b.decisions = 0; b.control_solves = 0; }
    return STMPC_OK;
}

int stmpc_speed_from_jerk_device(stmpc_ctx *c, const stmpc_params *p, double tick_length, int N, const double *d_ego5, const double *d_jerk, double *d_speed,
                                 void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!p) return fail(STMPC_EINVAL, "params is NULL");
    if (!(tick_length > 0)) return fail(STMPC_EINVAL, "tick_length must be positive");
    if (N < 0) return fail(STMPC_EINVAL, "N out of range");
    if (N == 0) return STMPC_OK;
    if (!d_ego5 || !d_jerk || !d_speed) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(c->device));
    CCfg cc;
    memset(&cc, 0, sizeof cc);
    cc.tick = tick_length; cc.a_max = p->a_max; cc.a_min = p->a_min; cc.v_max = p->v_max;
    hipLaunchKernelGGL(k_fs_speed_from_jerk, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, cc, N, d_ego5, d_jerk, d_speed);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

}  // extern "C"

namespace {
int make_simcfg(const stmpc_sim_cfg *g, sim::Cfg *c) {
    if (!g) return fail(STMPC_EINVAL, "sim cfg is NULL");
    if (!(g->tick_length > 0) || !(g->other_car_speed > 0) || !(g->base_traffic_interval > 0)) return fail(STMPC_EINVAL, "tick_length, other_car_speed and base_traffic_interval must be positive");
    memset(c, 0, sizeof *c);
    c->tick = g->tick_length; c->other_speed = g->other_car_speed; c->base_interval = g->base_traffic_interval;
    c->spawn_x = g->spawn_x; c->despawn_x = g->despawn_x; c->ego_start_x = g->ego_start_x; c->ego_start_y = g->ego_start_y; c->arrive_x = g->arrive_x;
    c->sensor_radius = g->sensor_radius; c->start_speed = g->start_speed; c->start_speed_std = g->start_speed_std;
    c->min_start_speed = g->min_start_speed; c->max_start_speed = g->max_start_speed;
    if (!(g->veh_accel > 0) || !(g->veh_decel > 0) || !(g->veh_tau >= 0) || !(g->veh_length > 0) || !(g->veh_emergency_decel >= g->veh_decel) || g->veh_min_gap < 0 || g->speed_dev < 0)
        return fail(STMPC_EINVAL, "vehicle type parameters (accel, decel, tau, length, emergency decel, minGap, speed_dev) out of range");
    c->veh_accel = g->veh_accel; c->veh_decel = g->veh_decel; c->veh_min_gap = g->veh_min_gap; c->veh_tau = g->veh_tau; c->veh_emergency_decel = g->veh_emergency_decel;
    c->veh_length = g->veh_length; c->veh_width = g->veh_width; c->speed_dev = g->speed_dev;
    c->vary_interval = g->vary_traffic_start_times; c->randomize_start_speed = g->randomize_start_speed; c->max_ticks = g->max_ticks; c->seed = g->seed;
    if (g->yield_overlap != 2) return fail(STMPC_EINVAL, "stmpc_sim_cfg.yield_overlap must be 2 (the one junction rule since ABI v6)");
    c->route = nullptr; c->route_n = 0;          // (the device copy of the route belongs to the context: sim_route_of)
    c->disruption_min_s = g->disruption_min_s;
    return STMPC_OK;
}
void sim_route_of(stmpc_ctx *c, sim::Cfg *sc) {
    if (c->sim.route_n >= 2) { sc->route = c->sim.route.as<double>(); sc->route_n = c->sim.route_n; }
}
// g's route, if it has one: at most 4096 points, x strictly increasing.  Changes nothing
int route_check(const stmpc_sim_cfg *g) {
    if (!g->ego_route_xy || g->ego_route_n < 2) return STMPC_OK;
    if (g->ego_route_n > 4096) return fail(STMPC_EINVAL, "ego_route_n out of range (at most 4096 points)");
    for (int i = 1; i < g->ego_route_n; ++i)
        if (!(g->ego_route_xy[2 * i] > g->ego_route_xy[2 * i - 2])) return fail(STMPC_EINVAL, "ego_route_xy: x must be strictly increasing");
    return STMPC_OK;
}
// the context's device copy of g's route (x then y), or none; the route has passed route_check
int sim_route_upload(stmpc_ctx *c, const stmpc_sim_cfg *g, void *stream) {
    c->sim.route_n = 0;
    if (g->ego_route_xy && g->ego_route_n >= 2) {
        const int n = g->ego_route_n;
        std::vector<double> xy((size_t)2 * n);
        for (int i = 0; i < n; ++i) { xy[i] = g->ego_route_xy[2 * i]; xy[n + i] = g->ego_route_xy[2 * i + 1]; }
        TRY(c->sim.route.ensure(xy.size() * 8));
        HIPCHK(hipMemcpyAsync(c->sim.route.p, xy.data(), xy.size() * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));       // (xy is a local)
        c->sim.route_n = n;
    }
    return STMPC_OK;
}
// A new world of N environments takes the context over (the init entries, after their checks): its buffers and g's route.  The vector environment's
// bookkeeping, its reward groups and the table of traffic groups no longer describe this world (the entries that made them set them again), and what
// is bound to the former world's generation (a recorder, a shielded env) is outdated.
int sim_world_begin(stmpc_ctx *c, const stmpc_sim_cfg *g, int N, void *stream) {
    TRY(c->sim.ensure(N));
    c->sim.N = N;
    ++c->sim.generation;
    c->env.N = 0; c->env.R = 0; c->env.n_per_rg = 0; c->env.T = 0;
    c->sim.G = 0; c->sim.n_per_group = 0;
    return sim_route_upload(c, g, stream);
}
// Traffic groups: every cfg valid, and equal in what the shared kernels (k_sim_view, k_env_act), the one route and the one vehicle type read.
// Changes nothing; `out` receives the G kernel cfgs without their route.
int check_groups(const stmpc_sim_cfg *cfgs, int G, int n_per_group, std::vector<sim::Cfg> *out, int G_max = STMPC_SIM_GROUPS_MAX) {
    if (!cfgs) return fail(STMPC_EINVAL, "sim cfgs is NULL");
    TRY(check_group_counts(G, n_per_group, G_max,
                           G_max == STMPC_SIM_GROUPS_MAX ? "G must be 1 ... STMPC_SIM_GROUPS_MAX (64) traffic groups" : "G must be 1 ... STMPC_SOLVER_GROUPS_MAX (512) cells"));
    out->resize((size_t)G);
    for (int g = 0; g < G; ++g) TRY(make_simcfg(&cfgs[g], &(*out)[g]));
    const stmpc_sim_cfg &a = cfgs[0];
    TRY(route_check(&a));
    const int route_a = a.ego_route_xy && a.ego_route_n >= 2 ? a.ego_route_n : 0;
    for (int g = 1; g < G; ++g) {
        const stmpc_sim_cfg &b = cfgs[g];
        const Share share{"traffic groups", "group", g, ""};
        SHARED(tick_length); SHARED(spawn_x); SHARED(despawn_x); SHARED(ego_start_x); SHARED(ego_start_y); SHARED(arrive_x); SHARED(sensor_radius);
        SHARED(veh_accel); SHARED(veh_decel); SHARED(veh_min_gap); SHARED(veh_tau); SHARED(veh_emergency_decel); SHARED(veh_length); SHARED(veh_width);
        SHARED(disruption_min_s); SHARED(yield_overlap);
        const int route_b = b.ego_route_xy && b.ego_route_n >= 2 ? b.ego_route_n : 0;
        if (route_a != route_b || (route_a && !same_bytes(a.ego_route_xy, b.ego_route_xy, (size_t)route_a * 16)))
            return fail(STMPC_EINVAL, "traffic groups must share ego_route_xy (it differs in group " + std::to_string(g) + ": equal points, or NULL alike)");
    }
    return STMPC_OK;
}
const char *const UNGROUPED_WORLD = "the world has no traffic groups (stmpc_sim_init_groups_device): use the plain step entry";
// the checks every grouped world step entry starts with
int check_grouped_world(stmpc_ctx *c, int N) {
    if (c->sim.G < 1) return fail(STMPC_EINVAL, UNGROUPED_WORLD);
    if (N != c->sim.N) return fail(STMPC_EINVAL, "N does not match stmpc_sim_init_groups_device (G * n_per_group)");
    return STMPC_OK;
}
int sim_init_groups(stmpc_ctx *c, const stmpc_sim_cfg *cfgs, int G, int n_per_group, void *stream, int G_max) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    std::vector<sim::Cfg> table;
    TRY(check_groups(cfgs, G, n_per_group, &table, G_max));
    const int N = G * n_per_group;
    HIPCHK(hipSetDevice(c->device));
    TRY(c->sim.groups.ensure(table.size() * sizeof(sim::Cfg)));
    TRY(sim_world_begin(c, &cfgs[0], N, stream));
    for (auto &sc : table) sim_route_of(c, &sc);
    HIPCHK(hipMemcpyAsync(c->sim.groups.p, table.data(), table.size() * sizeof(sim::Cfg), hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));           // (table is a local; the step entries read the device copy and take no cfgs)
    c->sim.G = G; c->sim.n_per_group = n_per_group;
    hipLaunchKernelGGL(sim::k_sim_init_groups, dim3((n_per_group + 63) / 64, G), dim3(64), 0, (hipStream_t)stream, c->sim.groups.as<sim::Cfg>(), n_per_group, c->sim.state());
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
const char *const GROUPED_WORLD = "the world has traffic groups (stmpc_sim_init_groups_device): one cfg would step every group; use the grouped step entry";
const char *const MIXED_ENV = "the env has a traffic mix (stmpc_traffic_mix_env_reset_device): one cfg would step every type; use stmpc_traffic_mix_env_step_device";
const char *const CSHIELD_ENV = "the env runs behind the combined controller (stmpc_cshield_env_reset_device): this entry would execute the proposal unprotected; use stmpc_cshield_env_step_device";
const char *const SHIELDED_ENV = "the env runs behind the first-step shield (a stmpc_shield_*_reset_device entry): this entry would execute the proposal unprotected; use the shielded step entry of the env's groups";
const char *const QSHIELD_ENV = "the env runs behind the combined controller with a Q-network (stmpc_qshield_env_reset_device): this entry would execute the proposal unprotected; use stmpc_qshield_env_step_device";
// (one set of rows serves both envs behind the combined controller: `qpolicy` tells whose they are)
bool has_combined_env(const stmpc_ctx *c) { return c->env.N >= 1 && c->cshield.N == c->env.N && c->cshield.generation == c->sim.generation; }
bool has_cshield_env(const stmpc_ctx *c) { return has_combined_env(c) && !c->cshield.qpolicy; }
bool has_qshield_env(const stmpc_ctx *c) { return has_combined_env(c) && c->cshield.qpolicy; }
const char *const REWARD_GROUPED_ENV = "the env has reward groups (stmpc_reward_groups_env_reset_device): one cfg would reward every group; use stmpc_reward_groups_env_step_device";
}  // namespace

extern "C" {

int stmpc_sim_init_device(stmpc_ctx *c, const stmpc_sim_cfg *g, int N, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N < 1) return fail(STMPC_EINVAL, "N must be positive");
    sim::Cfg sc;
    TRY(make_simcfg(g, &sc));
    TRY(route_check(g));
    HIPCHK(hipSetDevice(c->device));
    TRY(sim_world_begin(c, g, N, stream));
    sim_route_of(c, &sc);
    hipLaunchKernelGGL(sim::k_sim_init, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, sc, N, c->sim.state());
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_sim_view_device(stmpc_ctx *c, const stmpc_sim_cfg *g, int N, int Kmax, double *d_ego5, int32_t *d_k, double *d_ox, double *d_ov, double *d_oa, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    // (up to the world's vehicle slots: rows wider than STMPC_KMAX_LIMIT show the whole world to a test; the solver's entries take at most that limit)
    if (N != c->sim.N || Kmax < 1 || Kmax > sim::KS) return fail(STMPC_EINVAL, "N does not match stmpc_sim_init_device, or Kmax out of range");
    if (!d_ego5 || !d_k || !d_ox || !d_ov) return fail(STMPC_EINVAL, "NULL device pointer");
    sim::Cfg sc;
    TRY(make_simcfg(g, &sc));
    sim_route_of(c, &sc);
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(sim::k_sim_view, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, sc, N, Kmax, c->sim.state(), d_ego5, d_k, d_ox, d_ov, d_oa);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_sim_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, int N, const double *d_cmd_speed, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N != c->sim.N || !d_cmd_speed) return fail(STMPC_EINVAL, "N does not match stmpc_sim_init_device, or NULL device pointer");
    if (c->sim.G) return fail(STMPC_EINVAL, GROUPED_WORLD);
    if (c->env.N >= 1 && c->env.T >= 1) return fail(STMPC_EINVAL, MIXED_ENV);
    if (has_cshield_env(c)) return fail(STMPC_EINVAL, CSHIELD_ENV);
    if (has_qshield_env(c)) return fail(STMPC_EINVAL, QSHIELD_ENV);
    sim::Cfg sc;
    DevP dp;
    TRY(make_simcfg(g, &sc));
    sim_route_of(c, &sc);
    TRY(make_devp(p, &dp));
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(sim::k_sim_step, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, dp, sc, N, c->sim.state(), d_cmd_speed, p->crash_min_s);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_sim_init_groups_device(stmpc_ctx *c, const stmpc_sim_cfg *cfgs, int G, int n_per_group, void *stream) {
    return sim_init_groups(c, cfgs, G, n_per_group, stream, STMPC_SIM_GROUPS_MAX);
}

// (the world of a solver-groups run: one traffic group per cell of the grid, so the table may hold as many groups as the solver's)
int stmpc_solver_groups_sim_init_device(stmpc_ctx *c, const stmpc_sim_cfg *cfgs, int G, int n_per_group, void *stream) {
    return sim_init_groups(c, cfgs, G, n_per_group, stream, STMPC_SOLVER_GROUPS_MAX);
}

int stmpc_sim_step_groups_device(stmpc_ctx *c, const stmpc_params *p, int N, const double *d_cmd_speed, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(check_grouped_world(c, N));
    if (!d_cmd_speed) return fail(STMPC_EINVAL, "NULL device pointer");
    DevP dp;
    TRY(make_devp(p, &dp));
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(sim::k_sim_step_groups, dim3((c->sim.n_per_group + 63) / 64, c->sim.G), dim3(64), 0, (hipStream_t)stream, dp, c->sim.groups.as<sim::Cfg>(),
                       c->sim.n_per_group, c->sim.state(), d_cmd_speed, p->crash_min_s);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_solver_groups_sim_step_device(stmpc_ctx *c, const stmpc_params *groups, int G, int n_per_group, int N, const double *d_cmd_speed, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(check_solver_groups(groups, G, n_per_group, nullptr));
    TRY(check_grouped_world(c, N));
    if (G != c->sim.G || n_per_group != c->sim.n_per_group)
        return fail(STMPC_EINVAL, "the solver groups must coincide with the world's traffic groups (cell c pairs traffic c with solver c): G and n_per_group differ");
    if (!d_cmd_speed) return fail(STMPC_EINVAL, "NULL device pointer");
    DevP dp;
    TRY(make_devp(&groups[0], &dp));          // (the step reads the limits only: shared fields)
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> cms((size_t)G);
    for (int g = 0; g < G; ++g) cms[g] = groups[g].crash_min_s;
    if (cms != c->solver.sg.host_cms) {                  // (once per runner: the table is kept while the next step brings equal values)
        HIPCHK(hipDeviceSynchronize());
        c->solver.sg.host_cms.clear();
        TRY(upload(c->solver.sg.crash_min_s, cms.data(), cms.size()));
        c->solver.sg.host_cms = cms;
    }
    hipLaunchKernelGGL(sim::k_sim_step_solver_groups, dim3((n_per_group + 63) / 64, G), dim3(64), 0, (hipStream_t)stream, dp, c->sim.groups.as<sim::Cfg>(), n_per_group,
                       c->sim.state(), d_cmd_speed, c->solver.sg.crash_min_s.as<double>());
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_sim_groups(stmpc_ctx *c, int *G, int *n_per_group) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (G) *G = c->sim.G;
    if (n_per_group) *n_per_group = c->sim.n_per_group;
    return STMPC_OK;
}

int stmpc_sim_status_device(stmpc_ctx *c, int N, int32_t *d_status, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N != c->sim.N || !d_status) return fail(STMPC_EINVAL, "N does not match stmpc_sim_init_device, or NULL pointer");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(d_status, c->sim.status.p, (size_t)N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return STMPC_OK;
}

int stmpc_sim_read(stmpc_ctx *c, int N, int32_t *status, int32_t *ticks, double *acc, double *ego4) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N != c->sim.N) return fail(STMPC_EINVAL, "N does not match stmpc_sim_init_device");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t n = (size_t)N;
    TRY(download(status, c->sim.status, n)); TRY(download(ticks, c->sim.ticks, n)); TRY(download(acc, c->sim.acc, n * sim::NACC));
    TRY(download(ego4, c->sim.ego, n * 4));
    return STMPC_OK;
}

}  // extern "C"

// ---- vector environment on the simulator (stmpc_env_*): the reference's gym environments, merge_gym.py ----
namespace {
int make_envcfg(const stmpc_env_cfg *g, env::ECfg *c) {
    if (!g) return fail(STMPC_EINVAL, "env cfg is NULL");
    if (!g->features) return fail(STMPC_EINVAL, "env cfg: features is NULL");
    const stmpc_policy_features_cfg *f = g->features;
    if (f->time_feature) return fail(STMPC_EINVAL, "env cfg: the observation has no time feature (TimeFeature wraps the agent, not the env)");
    FeatCfg fc;
    TRY(make_featcfg(f, &fc));
    if (g->action_mode < STMPC_ENV_CONTINUOUS_JERK || g->action_mode > STMPC_ENV_ACCELERATION) return fail(STMPC_EINVAL, "env cfg: unknown action_mode");
    if (g->reward_function < STMPC_REWARD_CONTINUOUS || g->reward_function > STMPC_REWARD_ST) return fail(STMPC_EINVAL, "env cfg: unknown reward_function");
    if (!(g->tick_length > 0)) return fail(STMPC_EINVAL, "env cfg: tick_length must be positive");
    memset(c, 0, sizeof *c);
    c->tick = g->tick_length; c->crash_r = g->crash_reward; c->success_r = g->success_reward; c->time_r = g->time_reward;
    c->wt_smooth = g->wt_smooth; c->wt_safe = g->wt_safe; c->wt_eff = g->wt_efficient;
    c->alt_v = g->alt_v_weight; c->alt_a = g->alt_a_weight; c->alt_j = g->alt_j_weight; c->alt_d = g->alt_d_weight;
    c->min_follow = g->min_follow_distance; c->desired_speed = g->desired_speed; c->car_length = g->car_length;
    c->penalty = g->invalid_action_penalty; c->j_min = g->minimum_negative_jerk; c->j_max = g->maximum_positive_jerk;
    c->a_min = g->max_negative_acceleration; c->a_max = g->max_positive_acceleration; c->v_max = g->max_speed;
    c->mode = g->action_mode; c->reward = g->reward_function; c->autoreset = g->autoreset != 0;
    c->f = fc;                                   // (time_feature = 0: refused above)
    c->obs_len = stmpc_policy_features_len(f);
    return STMPC_OK;
}
env::EState env_state(stmpc_ctx *c) { return c->env.state(c->sticky.as<unsigned>() + 2); }
// argument checks of the reset entries (nothing changes before they pass)
int env_reset_check(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, const float *d_obs, int obs_stride, env::ECfg *e) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!p) return fail(STMPC_EINVAL, "params is NULL");
    TRY(make_envcfg(ec, e));
    if (d_obs && obs_stride < e->obs_len) return fail(STMPC_EINVAL, "obs_stride is shorter than the observation");
    if (ec->action_mode != STMPC_ENV_CONTINUOUS_JERK && (!ec->action_values || ec->n_action_values < 1 || ec->n_action_values > STMPC_ENV_MAX_ACTIONS))
        return fail(STMPC_EINVAL, "a discrete env needs 1..STMPC_ENV_MAX_ACTIONS action_values");
    if (ec->log_capacity < 0) return fail(STMPC_EINVAL, "log_capacity must not be negative");
    return STMPC_OK;
}
// the environment's bookkeeping for the world of N environments just initialised: buffers, the action table, an empty log
int env_reset_begin(stmpc_ctx *c, const stmpc_env_cfg *ec, int N, env::ECfg *e, void *stream) {
    auto &v = c->env;
    const int cap = ec->log_capacity ? ec->log_capacity : 16 * N;
    TRY(v.ensure(N, cap));
    v.n_actions = 0;
    if (ec->action_mode != STMPC_ENV_CONTINUOUS_JERK) {
        TRY(v.actions.ensure((size_t)ec->n_action_values * 8));
        HIPCHK(hipMemcpyAsync(v.actions.p, ec->action_values, (size_t)ec->n_action_values * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));       // (the table is the caller's host memory)
        v.n_actions = ec->n_action_values;
    }
    HIPCHK(hipMemsetAsync(v.log_n.p, 0, 4, (hipStream_t)stream));
    v.N = N;
    v.mode = ec->action_mode;
    e->log_cap = cap; e->n_actions = v.n_actions; e->actions = v.actions.as<double>();
    return STMPC_OK;
}
// the env cfg of a step against the environment in the context (`reset_entry` made it), which then completes the ECfg (but for the seed)
int env_step_begin(const stmpc_ctx *c, const stmpc_env_cfg *ec, int obs_stride, const char *reset_entry, env::ECfg *e) {
    TRY(make_envcfg(ec, e));
    if (obs_stride < e->obs_len) return fail(STMPC_EINVAL, "obs_stride is shorter than the observation");
    if (e->mode != c->env.mode) return fail(STMPC_EINVAL, std::string("env_cfg.action_mode differs from the one the context was reset with (") + reset_entry + ")");
    e->log_cap = c->env.log_cap; e->n_actions = c->env.n_actions; e->actions = c->env.actions.as<double>();
    return STMPC_OK;
}

// Every cfg valid, and equal in what the shared ECfg, the one action table, the one log and the one observation hold.  Changes nothing; `rows` receives
// the R table rows.
int check_reward_groups(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *cfgs, int R, int n_per_group, const float *d_obs, int obs_stride,
                        std::vector<env::RewardRow> *rows, env::ECfg *shared) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!cfgs) return fail(STMPC_EINVAL, "env cfgs is NULL");
    TRY(check_group_counts(R, n_per_group, STMPC_ENV_REWARD_GROUPS_MAX, "R must be 1 ... STMPC_ENV_REWARD_GROUPS_MAX (64) reward groups", "R", "n_per_reward_group"));
    rows->resize((size_t)R);
    for (int r = 0; r < R; ++r) {
        env::ECfg e;
        TRY(env_reset_check(c, p, &cfgs[r], d_obs, obs_stride, &e));
        if (r == 0) *shared = e;
        (*rows)[r] = env::RewardRow{e.crash_r, e.success_r, e.time_r, e.wt_smooth, e.wt_safe, e.wt_eff, e.alt_v, e.alt_a, e.alt_j, e.alt_d, e.min_follow,
                                    e.desired_speed, e.penalty, e.reward, 0};
    }
    const stmpc_env_cfg &a = cfgs[0];
    for (int r = 1; r < R; ++r) {
        const stmpc_env_cfg &b = cfgs[r];
        const Share share{"reward groups", "group", r, ""};
        SHARED(action_mode); SHARED(n_action_values); SHARED(tick_length); SHARED(minimum_negative_jerk); SHARED(maximum_positive_jerk); SHARED(max_negative_acceleration);
        SHARED(max_positive_acceleration); SHARED(max_speed); SHARED(car_length); SHARED(autoreset); SHARED(log_capacity);
        if (a.action_mode != STMPC_ENV_CONTINUOUS_JERK && !same_bytes(a.action_values, b.action_values, (size_t)a.n_action_values * 8))
            return fail(STMPC_EINVAL, "reward groups must share action_values (they differ in group " + std::to_string(r) + ")");
        if (!same_bytes(a.features, b.features, sizeof *a.features))
            return fail(STMPC_EINVAL, "reward groups must share features (they differ in group " + std::to_string(r) + ")");
    }
    return STMPC_OK;
}
struct MixReset {                            // what stmpc_traffic_mix_env_reset_device adds to a reset
    std::vector<env::TrafficRow> rows;       // one per type
    std::vector<double> cum;                 // the cumulative normalised weights
    unsigned long long seed;
    int32_t *d_type;                         // may be NULL
};
// The traffic mix: every cfg valid and equal in everything but the three traffic fields, the weights finite, not negative and of positive sum.  Changes
// nothing; `out` receives the table rows and the cumulative weights (the rule of include/stmpc.h: left to right in fp64, 1.0 from the last positive weight on).
int check_traffic_mix(const stmpc_sim_cfg *cfgs, int T, const double *weights, int N, MixReset *out) {
    if (!cfgs) return fail(STMPC_EINVAL, "sim cfgs is NULL");
    if (!weights) return fail(STMPC_EINVAL, "weights is NULL");
    if (T < 1 || T > STMPC_TRAFFIC_MIX_MAX) return fail(STMPC_EINVAL, "T must be 1 ... STMPC_TRAFFIC_MIX_MAX (64) traffic types");
    if (N < 1) return fail(STMPC_EINVAL, "N must be positive");
    std::vector<sim::Cfg> table;
    TRY(check_groups(cfgs, T, 1, &table));                   // (every cfg valid; the fields traffic groups must share, and the route)
    const stmpc_sim_cfg &a = cfgs[0];
    for (int t = 1; t < T; ++t) {
        const stmpc_sim_cfg &b = cfgs[t];
        const Share share{"traffic types", "type", t, ""};
        SHARED(seed); SHARED(start_speed); SHARED(start_speed_std); SHARED(min_start_speed); SHARED(max_start_speed); SHARED(speed_dev); SHARED(randomize_start_speed); SHARED(max_ticks);
    }
    double sum = 0.0;
    int last = -1;
    for (int t = 0; t < T; ++t) {
        if (!(weights[t] >= 0.0) || !(weights[t] <= 1.7976931348623157e308)) return fail(STMPC_EINVAL, "weights must be finite and not negative (type " + std::to_string(t) + ")");
        sum += weights[t];
        if (weights[t] > 0.0) last = t;
    }
    if (!(sum > 0.0) || !(sum <= 1.7976931348623157e308)) return fail(STMPC_EINVAL, "weights must have a positive, finite sum");
    out->rows.resize((size_t)T); out->cum.resize((size_t)T);
    double run = 0.0;
    for (int t = 0; t < T; ++t) {
        run += weights[t] / sum;
        out->cum[t] = t >= last ? 1.0 : run;
        out->rows[t] = env::TrafficRow{table[t].base_interval, table[t].other_speed, table[t].vary_interval, 0};
    }
    return STMPC_OK;
}
// the shielded env's cfg (its reset and its step)
int shield_cfg_check(const stmpc_params *p, const stmpc_shield_env_cfg *sh, int N) {
    if (!sh) return fail(STMPC_EINVAL, "shield cfg is NULL");
    if (sh->kmax < 1 || sh->kmax > STMPC_KMAX_LIMIT) return fail(STMPC_EINVAL, "shield cfg: kmax must be 1 ... STMPC_KMAX_LIMIT (32), the solver's vehicles per state");
    if (!(sh->takeover_penalty >= 0) || !(sh->takeover_penalty <= 1.7976931348623157e308)) return fail(STMPC_EINVAL, "shield cfg: takeover_penalty must be finite and not negative");
    return first_step_check(p, &sh->fs, N, sh->kmax);
}
// The checks of a shielded reset (nothing changes).  `count`: 0 for the lone shielded env, whose step takes sh->takeover_penalty by value (no table); else the
// env's groups (1 for the traffic mix), and `table` receives the takeover penalties the step reads: the P = 1 or P = count values of
// `penalties`, or (P = 0) the one sh->takeover_penalty.
struct ShieldReset {
    std::vector<double> table;
    int N = 0, H = 0;
};
int shield_reset_check(stmpc_ctx *c, const stmpc_params *p, const stmpc_shield_env_cfg *sh, int N, const double *penalties, int P, int count, ShieldReset *r) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(shield_cfg_check(p, sh, N));
    if (N < 1) return fail(STMPC_EINVAL, "N must be positive");
    DevP dp;
    TRY(make_devp(p, &dp));
    r->N = N; r->H = dp.H;
    if (!count) return STMPC_OK;
    if (P < 0 || (P > 0 && !penalties) || (P != 0 && P != 1 && P != count))
        return fail(STMPC_EINVAL, "takeover_penalties: P must be 0 (shield_cfg's takeover_penalty for every group), 1 or the number of groups (" + std::to_string(count) + ")");
    r->table.assign(penalties, penalties + P);
    if (!P) r->table.push_back(sh->takeover_penalty);
    for (size_t i = 0; i < r->table.size(); ++i)
        if (!(r->table[i] >= 0) || !(r->table[i] <= 1.7976931348623157e308))
            return fail(STMPC_EINVAL, "takeover_penalties must be finite and not negative (group " + std::to_string(i) + ")");
    return STMPC_OK;
}
// ... and what follows the env's reset: the shield's buffers (view, proposal, decision, counters, zeroed), the first-step controller's, the penalty table
int shield_reset_finish(stmpc_ctx *c, const stmpc_shield_env_cfg *sh, const ShieldReset &r, void *stream) {
    auto &v = c->shield;                         // (the world initialised by the env's reset has outdated an earlier shielded env by its generation)
    const int N = r.N;
    TRY(v.ensure(N, sh->kmax));
    TRY(first_step_ensure(c, N, sh->kmax, r.H, true));        // (the sparse solve's compact batch too: a step may set fs.sparse_control either way)
    HIPCHK(hipMemsetAsync(v.count.p, 0, (size_t)N * 4, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(v.tag.p, 0, (size_t)N * 4, (hipStream_t)stream));
    v.P = 0; v.n_per_penalty = 0;
    if (!r.table.empty()) {
        TRY(v.penalty.ensure((size_t)STMPC_SIM_GROUPS_MAX * 8));      // (its full size once: never reallocated under a running kernel)
        HIPCHK(hipMemcpyAsync(v.penalty.p, r.table.data(), r.table.size() * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));       // (the table is the caller's local; the step reads the device copy)
        v.P = (int)r.table.size(); v.n_per_penalty = N / v.P;
    }
    v.N = N; v.kmax = sh->kmax; v.generation = c->sim.generation;
    return STMPC_OK;
}
// the checks of a reward-groups reset (nothing changes): the table rows, the shared cfg, N = R * n_per_reward_group
struct RewardGroupsReset {
    std::vector<env::RewardRow> rows;
    env::ECfg e;
    int N = 0;
};
int reward_groups_reset_check(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int G, int n_per_traffic_group, const stmpc_env_cfg *env_cfgs,
                              int R, int n_per_reward_group, const float *d_obs, int obs_stride, RewardGroupsReset *rg) {
    std::vector<sim::Cfg> world;
    TRY(check_reward_groups(c, p, env_cfgs, R, n_per_reward_group, d_obs, obs_stride, &rg->rows, &rg->e));
    rg->N = R * n_per_reward_group;
    if (G < 0) return fail(STMPC_EINVAL, "G must not be negative (0: an ungrouped world from sim_cfgs[0])");
    TRY(check_groups(sim_cfgs, G ? G : 1, G ? n_per_traffic_group : rg->N, &world));       // (G = 0: the one cfg and its route, as a table of one)
    if (G && (G != R || n_per_traffic_group != n_per_reward_group))
        return fail(STMPC_EINVAL, "the reward groups must coincide with the world's traffic groups (cell c pairs traffic c with reward c): R must equal G and "
                                  "n_per_reward_group n_per_traffic_group");
    return STMPC_OK;
}

// The env behind the combined controller, whichever policy proposes in its rollout: what its reset and its step take of the entry's cfg
// (stmpc_cshield_env_cfg, stmpc_qshield_env_cfg) and the policy.  `cc` is NULL where the entry's cfg was.
struct CombinedShield {
    const stmpc_combined_cfg *cc;
    const stmpc_policy_features_cfg *features;
    double takeover_penalty;
    int kmax, rollout_time;                  // (rollout_time: 0 for the Q env, which has no time counter)
    bool qnet;                               // the Q env (stmpc_qshield_env_*): the policy is q or pop, else actor
    const stmpc_actor *actor;
    const stmpc_qactor *q;                   // exactly one of q and pop (qshield_policy_check)
    const stmpc_qactor_pop *pop;
    int n_per_member;
    const void *qpolicy() const { return q ? (const void *)q : (const void *)pop; }
};
CombinedShield combined_shield_of(const stmpc_cshield_env_cfg *sh, const stmpc_actor *a) {
    if (!sh) return CombinedShield{nullptr, nullptr, 0, 0, 0, false, a, nullptr, nullptr, 0};
    return CombinedShield{&sh->cc, &sh->features, sh->takeover_penalty, sh->kmax, sh->rollout_time, false, a, nullptr, nullptr, 0};
}
CombinedShield combined_shield_of(const stmpc_qshield_env_cfg *sh, const stmpc_qactor *q, const stmpc_qactor_pop *pop, int n_per_member) {
    if (!sh) return CombinedShield{nullptr, nullptr, 0, 0, 0, true, nullptr, q, pop, n_per_member};
    return CombinedShield{&sh->cc, &sh->features, sh->takeover_penalty, sh->kmax, 0, true, nullptr, q, pop, n_per_member};
}
// the Q env's own checks: a discrete env cfg, no time feature, the policy (*n_in receives its input width)
int qshield_checks(const stmpc_ctx *c, const stmpc_env_cfg *ec, const CombinedShield &d, int N, int *n_in) {
    if (N < 1) return fail(STMPC_EINVAL, "N must be positive");
    if (ec->action_mode == STMPC_ENV_CONTINUOUS_JERK)
        return fail(STMPC_EINVAL, "stmpc_qshield_env_* serves STMPC_ENV_JERK and STMPC_ENV_ACCELERATION (the rollout policy is a Q-network): the continuous env "
                                  "behind the combined controller is stmpc_cshield_env_reset_device / stmpc_cshield_env_step_device");
    if (ec->action_mode != STMPC_ENV_JERK && ec->action_mode != STMPC_ENV_ACCELERATION) return fail(STMPC_EINVAL, "env cfg: unknown action_mode");
    if (!ec->action_values || ec->n_action_values < 1 || ec->n_action_values > STMPC_ENV_MAX_ACTIONS)
        return fail(STMPC_EINVAL, "a discrete env needs 1..STMPC_ENV_MAX_ACTIONS action_values");
    if (d.features->time_feature) return fail(STMPC_EINVAL, "a Q-network has no time feature: the features cfg must have time_feature = 0");
    return qshield_policy_check(c, d.q, d.pop, d.n_per_member, N, ec->action_mode == STMPC_ENV_ACCELERATION, ec->action_values, ec->n_action_values,
                                ec->tick_length, ec->minimum_negative_jerk, ec->maximum_positive_jerk, n_in);
}
// its cfg, and with a Q-network its env cfg, and its policy (the reset and the step): `cc`, `fc` receive the kernels' forms.  Changes nothing.
int combined_shield_check(const stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, const CombinedShield &d, int N, CCfg *cc, FeatCfg *fc) {
    const std::string cfg = d.qnet ? "combined shield (Q) cfg" : "combined shield cfg";
    if (!d.cc) return fail(STMPC_EINVAL, cfg + " is NULL");
    if (d.qnet && !ec) return fail(STMPC_EINVAL, "env cfg is NULL");
    if (!d.qnet && !d.actor) return fail(STMPC_EINVAL, "combined shield: actor is NULL");
    if (d.kmax < 1 || d.kmax > STMPC_KMAX_LIMIT) return fail(STMPC_EINVAL, cfg + ": kmax must be 1 ... STMPC_KMAX_LIMIT (32), the solver's vehicles per state");
    if (!(d.takeover_penalty >= 0) || !(d.takeover_penalty <= 1.7976931348623157e308)) return fail(STMPC_EINVAL, cfg + ": takeover_penalty must be finite and not negative");
    if (d.rollout_time != env::ROLLOUT_TIME_ENV && d.rollout_time != env::ROLLOUT_TIME_DEPLOYED)
        return fail(STMPC_EINVAL, "combined shield cfg: rollout_time must be 0 (env) or 1 (deployed)");
    TRY(make_ccfg(p, d.cc, cc));
    if (cc->remember_last) return fail(STMPC_EINVAL, cfg + ": remember_last_choice must be 0 (the env keeps no takeover history per episode)");
    TRY(check_batch(N, d.kmax));
    int device = c->device, n_in = 0;
    if (d.qnet) { TRY(qshield_checks(c, ec, d, N, &n_in)); }
    else { device = d.actor->device; n_in = d.actor->dev.n_in; }
    // (the eval entries' checks of an empty batch: the device, the features, the policy's input width; the rows are the context's own)
    return actor_eval_checks(c, device, n_in, d.features, 0, d.kmax, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, fc);
}
// the rollout's "propose step `step`" on the current rows: the bodies of stmpc_actor_eval_device, stmpc_qactor_eval_device or stmpc_pop_qactor_eval_device
int combined_shield_propose(stmpc_ctx *c, const CombinedShield &d, const FeatCfg &fc, int N, int step, const env::CShieldView &w, double *jerk, void *stream) {
    if (d.actor) return actor_eval_run(c, d.actor, fc, N, d.kmax, step, w.cur_ego4, w.k, w.cur_ox, w.cur_ov, w.cur_oa, w.evals, nullptr, 0, jerk, stream);
    if (d.q) return qactor_eval_run(c, d.q, fc, N, d.kmax, step, w.cur_ego4, w.k, w.cur_ox, w.cur_ov, w.cur_oa, nullptr, 0, nullptr, nullptr, jerk, stream);
    return qactor_pop_eval_run(c, d.pop, fc, d.n_per_member, d.kmax, step, w.cur_ego4, w.k, w.cur_ox, w.cur_ov, w.cur_oa, nullptr, 0, nullptr, nullptr, jerk, stream);
}

// ---- one reset, one step and one reward body behind the plain, traffic-groups, reward-groups and shielded entries ----
// Which env shapes an entry serves: a shape the context has and the entry refuses, or lacks and the entry requires, is STMPC_EINVAL.
enum Need { REFUSED, EITHER, REQUIRED };
struct EnvEntry {
    const char *reset_entry;                 // the reset entry that makes this entry's env (for messages)
    Need traffic_groups, reward_groups, shield, traffic_mix, cshield, qshield = REFUSED;
};
const EnvEntry PLAIN_ENV{"stmpc_env_reset_device", REFUSED, REFUSED, EITHER, REFUSED, REFUSED};       // (on a shield-reset context: the unshielded step)
// (the unshielded grouped entries refuse a shielded env: only the lone shielded env, whose world takes one cfg, has an unshielded step)
const EnvEntry TRAFFIC_GROUPS_ENV{"stmpc_env_reset_groups_device", REQUIRED, REFUSED, REFUSED, REFUSED, REFUSED};
const EnvEntry REWARD_GROUPS_ENV{"stmpc_reward_groups_env_reset_device", EITHER, REQUIRED, REFUSED, REFUSED, REFUSED};
const EnvEntry SHIELD_ENV{"stmpc_shield_env_reset_device", REFUSED, REFUSED, REQUIRED, REFUSED, REFUSED};
const EnvEntry TRAFFIC_MIX_ENV{"stmpc_traffic_mix_env_reset_device", REFUSED, REFUSED, REFUSED, REQUIRED, REFUSED};
const EnvEntry CSHIELD_ENV_ENTRY{"stmpc_cshield_env_reset_device", REFUSED, REFUSED, REFUSED, REFUSED, REQUIRED};
const EnvEntry QSHIELD_ENV_ENTRY{"stmpc_qshield_env_reset_device", REFUSED, REFUSED, REFUSED, REFUSED, REFUSED, REQUIRED};
const EnvEntry SHIELD_TRAFFIC_GROUPS_ENV{"stmpc_shield_traffic_groups_env_reset_device", REQUIRED, REFUSED, REQUIRED, REFUSED, REFUSED};
const EnvEntry SHIELD_REWARD_GROUPS_ENV{"stmpc_shield_reward_groups_env_reset_device", EITHER, REQUIRED, REQUIRED, REFUSED, REFUSED};
const EnvEntry SHIELD_TRAFFIC_MIX_ENV{"stmpc_shield_traffic_mix_env_reset_device", REFUSED, REFUSED, REQUIRED, REQUIRED, REFUSED};

int env_shape_check(const stmpc_ctx *c, const EnvEntry &who) {
    const auto &v = c->shield;
    const struct { bool has; Need need; const char *refused, *missing; } shapes[] = {
        {c->sim.G > 0, who.traffic_groups, GROUPED_WORLD, UNGROUPED_WORLD},
        {c->env.N >= 1 && c->env.R >= 1, who.reward_groups, REWARD_GROUPED_ENV,
         "the env has no reward groups (stmpc_reward_groups_env_reset_device): use the plain or the traffic-groups step entry"},
        {c->env.N >= 1 && v.N == c->env.N && v.generation == c->sim.generation, who.shield, SHIELDED_ENV,
         "the environment in this context was not reset through stmpc_shield_env_reset_device or a shielded reset entry of its groups"},
        {c->env.N >= 1 && c->env.T >= 1, who.traffic_mix, MIXED_ENV, "the environment in this context was not reset through stmpc_traffic_mix_env_reset_device"},
        {has_cshield_env(c), who.cshield, CSHIELD_ENV, "the environment in this context was not reset through stmpc_cshield_env_reset_device"},
        {has_qshield_env(c), who.qshield, QSHIELD_ENV, "the environment in this context was not reset through stmpc_qshield_env_reset_device"},
    };
    for (const auto &sh : shapes) {
        if (sh.has && sh.need == REFUSED) return fail(STMPC_EINVAL, sh.refused);
        if (!sh.has && sh.need == REQUIRED) return fail(STMPC_EINVAL, sh.missing);
    }
    return STMPC_OK;
}

// Reset.  The world is the lone sim_cfgs[0] with N environments (G = 0) or G traffic groups; the reward is the lone env_cfgs[0] (R = 0) or R reward groups
// (`rows`: their table, checked by the caller with `e`, the shared cfg).  The caller has made every check of the env's arguments; the world inits make
// theirs before they change anything.
// `mix`: NULL, or the traffic mix of an ungrouped world under one reward (checked by the caller; sim_cfgs[0] then carries what the types share).
int env_reset(stmpc_ctx *c, const stmpc_sim_cfg *sim_cfgs, int G, int n_per_group, int N, const stmpc_env_cfg *env_cfgs, int R, int n_per_rg,
              const std::vector<env::RewardRow> &rows, env::ECfg e, float *d_obs, int obs_stride, void *stream, const MixReset *mix = nullptr) {
    if (G) { TRY(sim_init_groups(c, sim_cfgs, G, n_per_group, stream, STMPC_SIM_GROUPS_MAX)); }
    else if (mix) { TRY(sim_world_begin(c, sim_cfgs, N, stream)); }          // (no k_sim_init: k_env_reset_mix starts each environment under its own type)
    else { TRY(stmpc_sim_init_device(c, sim_cfgs, N, stream)); }
    N = c->sim.N;
    TRY(env_reset_begin(c, env_cfgs, N, &e, stream));
    if (mix) {
        auto &v = c->env;
        HIPCHK(hipMemcpyAsync(v.mix_rows.p, mix->rows.data(), mix->rows.size() * sizeof(env::TrafficRow), hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(hipMemcpyAsync(v.mix_cum.p, mix->cum.data(), mix->cum.size() * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));       // (the caller's locals; the step entry reads the device copies)
        sim::Cfg sc;
        TRY(make_simcfg(sim_cfgs, &sc));
        sim_route_of(c, &sc);
        v.T = (int)mix->rows.size(); v.mix_seed = mix->seed; v.mix_sc = sc;
        e.seed = sc.seed;
        hipLaunchKernelGGL(env::k_env_reset_mix, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, e, sc, v.traffic_mix(), N, c->sim.state(), env_state(c), d_obs,
                           obs_stride, mix->d_type);
        HIPCHK(hipGetLastError());
        return STMPC_OK;
    }
    if (R) {
        HIPCHK(hipMemcpyAsync(c->env.rtab.p, rows.data(), rows.size() * sizeof(env::RewardRow), hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));       // (rows is the caller's local; the step entries read the device copy)
        c->env.R = R; c->env.n_per_rg = n_per_rg;
    }
    if (G) {
        e.seed = 0;                              // (unused: a group's environments take their seed from the group's cfg)
        hipLaunchKernelGGL(env::k_env_reset_groups, dim3((n_per_group + 63) / 64, G), dim3(64), 0, (hipStream_t)stream, e, c->sim.groups.as<sim::Cfg>(), n_per_group,
                           c->sim.state(), env_state(c), d_obs, obs_stride);
    } else {
        sim::Cfg sc;
        TRY(make_simcfg(sim_cfgs, &sc));
        sim_route_of(c, &sc);
        if (R) c->env.rg_sc = sc;                // (the reward-groups step takes no sim cfg)
        e.seed = sc.seed;
        hipLaunchKernelGGL(env::k_env_reset, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, e, sc, N, c->sim.state(), env_state(c), d_obs, obs_stride);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

struct StepOut {                             // the tail every step entry takes
    const void *action;
    float *obs;
    int obs_stride;
    double *reward;
    uint8_t *terminated, *truncated;
    float *final_obs;
    double *final_stats;
    void *stream;
};
struct MixStep {                             // what the traffic-mix step takes on top
    int32_t *traffic_type, *final_traffic_type;
};
struct ShieldOut {                           // what a step behind either shield writes on top (executed_action may be NULL)
    uint8_t *takeover;
    int32_t *reason;
    double *executed_jerk, *executed_action;
    int32_t *takeover_ticks;
};
struct StepExtra {                           // what an entry has besides the plain step's arguments: it names those it has
    const stmpc_shield_env_cfg *shield = nullptr;    // behind the first-step shield ...
    const CombinedShield *combined = nullptr;        // ... or the combined controller: either writes `out`
    ShieldOut out{};
    const MixStep *mix = nullptr;
};

// the world step and the env's reward / observation / autoreset: `lone` is the cfg of an ungrouped world, NULL for the context's traffic groups
// (`mix`: the world is the context's traffic mix, `lone` what its types share)
void env_world_step(stmpc_ctx *c, const DevP &dp, double crash_min_s, const env::ECfg &e, const sim::Cfg *lone, bool reward_groups, const StepOut &o,
                    const MixStep *mix = nullptr) {
    const int N = c->sim.N, npg = c->sim.n_per_group;
    const dim3 grid = lone ? dim3((N + 63) / 64) : dim3((npg + 63) / 64, c->sim.G), block(64);
    hipStream_t st_ = (hipStream_t)o.stream;
    const sim::State s = c->sim.state();
    const env::EState es = env_state(c);
    const env::RewardTab tab = c->env.reward_tab();
    const sim::Cfg *groups = c->sim.groups.as<sim::Cfg>();
    if (mix) {
        const env::TrafficMix m = c->env.traffic_mix();
        hipLaunchKernelGGL(env::k_sim_step_mix, grid, block, 0, st_, dp, *lone, m, N, s, (const double *)es.cmd, crash_min_s);
        hipLaunchKernelGGL(env::k_env_post_mix, grid, block, 0, st_, e, *lone, m, N, s, es, o.obs, o.obs_stride, o.reward, o.terminated, o.truncated, o.final_obs,
                           o.final_stats, mix->traffic_type, mix->final_traffic_type);
        return;
    }
    if (lone) hipLaunchKernelGGL(sim::k_sim_step, grid, block, 0, st_, dp, *lone, N, s, (const double *)es.cmd, crash_min_s);
    else hipLaunchKernelGGL(sim::k_sim_step_groups, grid, block, 0, st_, dp, groups, npg, s, (const double *)es.cmd, crash_min_s);
#define POST(kernel, ...) hipLaunchKernelGGL(env::kernel, grid, block, 0, st_, e, __VA_ARGS__, s, es, o.obs, o.obs_stride, o.reward, o.terminated, o.truncated, o.final_obs, o.final_stats)
    if (lone && reward_groups) POST(k_env_post_rg, tab, *lone, N);
    else if (lone) POST(k_env_post, *lone, N);
    else if (reward_groups) POST(k_env_post_rg_groups, tab, groups, npg);
    else POST(k_env_post_groups, groups, npg);
#undef POST
}

// Step.  `g`: the cfg of a lone world (NULL: the entry takes none); `x`: what the entry has on top of the plain step.
int env_step(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, int N, const EnvEntry &who, const StepOut &o,
             const StepExtra &x = {}) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(env_shape_check(c, who));
    if (N != c->env.N || N != c->sim.N || N < 1) return fail(STMPC_EINVAL, std::string("N does not match ") + who.reset_entry);
    const stmpc_shield_env_cfg *sh = x.shield;
    const CombinedShield *cs = x.combined;
    const MixStep *mix = x.mix;
    const ShieldOut &out = x.out;
    const auto &v = c->shield;
    const auto &u = c->cshield;
    CCfg cs_cc;
    FeatCfg cs_fc;
    if (cs) {
        TRY(combined_shield_check(c, p, ec, *cs, N, &cs_cc, &cs_fc));
        const bool as_reset = cs->kmax == u.kmax && cs_cc.rollout_length == u.L &&
                              (cs->qnet ? cs->qpolicy() == u.qpolicy && cs->n_per_member == u.n_per_member && ec->n_action_values == c->env.n_actions
                                        : cs->rollout_time == u.rollout_time);
        if (!as_reset)
            return fail(STMPC_EINVAL, cs->qnet ? "combined shield (Q): kmax, the rollout length, the policy, n_per_member or n_action_values differs from the one the context was reset with (stmpc_qshield_env_reset_device)"
                                               : "combined shield cfg: kmax, rollout_time or the rollout length differs from the one the context was reset with (stmpc_cshield_env_reset_device)");
    } else if (sh) {
        TRY(shield_cfg_check(p, sh, N));
        if (sh->kmax != v.kmax) return fail(STMPC_EINVAL, std::string("shield cfg: kmax differs from the one the context was reset with (") + who.reset_entry + ")");
    }
    if (!o.action || !o.obs || !o.reward || !o.terminated || !o.truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    if ((sh || cs) && (!out.takeover || !out.reason || !out.executed_jerk || !out.takeover_ticks)) return fail(STMPC_EINVAL, "NULL device pointer (shield outputs)");
    if (mix && (!mix->traffic_type || !mix->final_traffic_type)) return fail(STMPC_EINVAL, "NULL device pointer (traffic type outputs)");
    env::ECfg e;
    sim::Cfg sc;
    DevP dp;
    TRY(env_step_begin(c, ec, o.obs_stride, who.reset_entry, &e));
    if (out.executed_action && e.mode != env::ACT_CONTINUOUS_JERK)
        return fail(STMPC_EINVAL, "d_executed_action is the continuous env's (a discrete index is not rewritten): pass NULL");
    if (cs && !cs->qnet && e.mode != env::ACT_CONTINUOUS_JERK) return fail(STMPC_EINVAL, "the combined shield serves STMPC_ENV_CONTINUOUS_JERK only (the rollout policy is a continuous actor)");
    // the world: one cfg -- the caller's, or the one an ungrouped reward-groups reset kept -- or the context's table of traffic groups
    const bool grouped = c->sim.G > 0, reward_groups = who.reward_groups == REQUIRED;
    if (sh && (grouped || reward_groups || mix) && (v.P < 1 || (int64_t)v.P * v.n_per_penalty != N))         // (what k_shield_env_apply_groups indexes)
        return fail(STMPC_EINVAL, std::string("the context holds no takeover penalty table for this env (") + who.reset_entry + ")");
    if (!grouped && reward_groups) sc = c->env.rg_sc;
    else if (mix) sc = c->env.mix_sc;
    else if (!grouped) { TRY(make_simcfg(g, &sc)); sim_route_of(c, &sc); }
    TRY(make_devp(p, &dp));
    e.seed = grouped ? 0 : sc.seed;
    HIPCHK(hipSetDevice(c->device));
    const dim3 grid((N + 63) / 64), block(64);
    hipStream_t st_ = (hipStream_t)o.stream;
    const sim::State s = c->sim.state();
    const env::EState es = env_state(c);
    // the action stage: the command of every live environment
    if (cs) {
        const env::CShieldView w = u.view();
        // 1. action handling, the planner's view into the start and the current rows, the first action and, in front of an actor, the rollout's time
        //    counter (a Q-network has no time feature)
        if (cs->qnet) hipLaunchKernelGGL(env::k_qshield_env_pre, grid, block, 0, st_, e, sc, N, u.kmax, s, es, o.action, w);
        else hipLaunchKernelGGL(env::k_cshield_env_pre, grid, block, 0, st_, e, sc, N, u.kmax, u.rollout_time, s, es, o.action, w);
        HIPCHK(hipGetLastError());
        // 2. dqn.RLAgent.do_combined_control on that view: the policy's eval body (steps 2 ... L), stmpc_rollout_step_device's and
        //    stmpc_combined_decide_device's
        for (int step = 1; step <= cs_cc.rollout_length; ++step) {
            if (step > 1) TRY(combined_shield_propose(c, *cs, cs_fc, N, step, w, u.jerk.as<double>(), o.stream));
            TRY(rollout_step_run(c, p, cs->cc, N, u.kmax, step, w.ego5, w.cur_ego4, w.k, w.cur_ox, w.cur_ov, w.cur_oa, step > 1 ? u.jerk.as<double>() : w.first_action,
                                 o.stream));
        }
        TRY(combined_decide_run(c, p, cs->cc, N, u.kmax, w.ego5, w.k, w.ox, w.ov, w.cur_ego4, w.cur_ox, w.cur_ov, w.first_action, nullptr, u.takeover.as<int32_t>(),
                                u.reason.as<int32_t>(), u.speed.as<double>(), o.stream));
        // 3. what is executed, and what the learner is told: the first-step shield's rule, unchanged (the Q env's executed_action is NULL: the index is
        //    not rewritten)
        hipLaunchKernelGGL(env::k_shield_env_apply, grid, block, 0, st_, e, cs->takeover_penalty, N, s, es, o.action, (const double *)u.speed.as<double>(),
                           (const int *)u.takeover.as<int>(), (const int *)u.reason.as<int>(), u.count.as<int>(), u.tag.as<int>(), out.takeover, out.reason,
                           out.executed_jerk, out.executed_action, out.takeover_ticks);
    } else if (sh) {
        const env::ShieldView w = v.view();
        const bool lone = !grouped && !reward_groups && !mix;
        const sim::Cfg *groups = c->sim.groups.as<sim::Cfg>();
        // 1. action handling, the planner's view, the proposal: the lone kernel, or the form of the env's groups (one launch either way)
        if (lone) hipLaunchKernelGGL(env::k_shield_env_pre, grid, block, 0, st_, e, sc, N, v.kmax, s, es, o.action, w);
        else if (mix) hipLaunchKernelGGL(env::k_shield_env_pre_mix, grid, block, 0, st_, e, sc, c->env.traffic_mix(), N, v.kmax, s, es, o.action, w);
        else if (grouped && reward_groups)
            hipLaunchKernelGGL(env::k_shield_env_pre_rg_groups, grid, block, 0, st_, e, c->env.reward_tab(), groups, N, v.kmax, s, es, o.action, w);
        else if (grouped) hipLaunchKernelGGL(env::k_shield_env_pre_groups, grid, block, 0, st_, e, groups, c->sim.n_per_group, N, v.kmax, s, es, o.action, w);
        else hipLaunchKernelGGL(env::k_shield_env_pre_rg, grid, block, 0, st_, e, c->env.reward_tab(), sc, N, v.kmax, s, es, o.action, w);
        HIPCHK(hipGetLastError());
        // 2. st.do_conditional_st_based_on_first_step on that view and proposal: stmpc_first_step_device's body, on all N rows whatever their group
        TRY(first_step_run(c, p, &sh->fs, N, v.kmax, w.ego5, w.k, w.ox, w.ov, w.proposal, v.speed.as<double>(), v.takeover.as<int32_t>(), v.reason.as<int32_t>(),
                           o.stream));
        // 3. what is executed, and what the learner is told (with groups: under the penalty of the environment's row of the reset's table)
        if (lone)
            hipLaunchKernelGGL(env::k_shield_env_apply, grid, block, 0, st_, e, sh->takeover_penalty, N, s, es, o.action, (const double *)v.speed.as<double>(),
                               (const int *)v.takeover.as<int>(), (const int *)v.reason.as<int>(), v.count.as<int>(), v.tag.as<int>(), out.takeover, out.reason,
                               out.executed_jerk, out.executed_action, out.takeover_ticks);
        else
            hipLaunchKernelGGL(env::k_shield_env_apply_groups, grid, block, 0, st_, e, v.penalty_tab(), N, s, es, o.action, (const double *)v.speed.as<double>(),
                               (const int *)v.takeover.as<int>(), (const int *)v.reason.as<int>(), v.count.as<int>(), v.tag.as<int>(), out.takeover, out.reason,
                               out.executed_jerk, out.executed_action, out.takeover_ticks);
    } else if (reward_groups) {
        hipLaunchKernelGGL(env::k_env_act_rg, grid, block, 0, st_, e, c->env.reward_tab(), N, s, es, o.action);
    } else {
        hipLaunchKernelGGL(env::k_env_act, grid, block, 0, st_, e, N, s, es, o.action);
    }
    env_world_step(c, dp, p->crash_min_s, e, grouped ? nullptr : &sc, reward_groups, o, mix);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

// The reset behind both combined-shield reset entries: the plain reset, then every buffer of the step and zeroed counters.
int combined_shield_reset(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, const CombinedShield &d, int N, float *d_obs,
                          int obs_stride, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    CCfg cc;
    FeatCfg fc;
    TRY(combined_shield_check(c, p, ec, d, N, &cc, &fc));
    if (!d.qnet) {                               // (the Q env's checks have looked at N and the env cfg)
        if (N < 1) return fail(STMPC_EINVAL, "N must be positive");
        if (!ec) return fail(STMPC_EINVAL, "env cfg is NULL");
        if (ec->action_mode != STMPC_ENV_CONTINUOUS_JERK)
            return fail(STMPC_EINVAL, "the combined shield serves STMPC_ENV_CONTINUOUS_JERK only (the rollout policy is a continuous actor)");
    }
    DevP dp;
    TRY(make_devp(p, &dp));
    HIPCHK(hipSetDevice(c->device));
    auto &u = c->cshield;                        // (a world initialised below outdates an earlier combined-shield env by its generation)
    TRY(stmpc_env_reset_device(c, p, g, ec, N, d_obs, obs_stride, stream));
    TRY(u.ensure(N, d.kmax));
    TRY(c->cc.ensure(N, d.kmax, cc.rollout_length));
    TRY(combined_ensure(c, N, d.kmax, dp.H, true));           // (the sparse solve's compact batch too: a step may set cc.sparse_control either way)
    DevBuf *const zeroed[] = {&u.evals, &u.evals_tag, &u.count, &u.tag};      // (the Q env has no time counter: the takeover counters only)
    for (int i = d.qnet ? 2 : 0; i < 4; ++i) HIPCHK(hipMemsetAsync(zeroed[i]->p, 0, (size_t)N * 4, (hipStream_t)stream));
    u.N = N; u.kmax = d.kmax; u.rollout_time = d.rollout_time; u.L = cc.rollout_length; u.generation = c->sim.generation;
    u.qpolicy = d.qnet ? d.qpolicy() : nullptr; u.n_per_member = d.n_per_member;
    return STMPC_OK;
}

// Reward of arbitrary batched states: under the one cfg, or (`reward_groups`) state e under reward group e / n_per_reward_group of the context's env.
int env_reward(stmpc_ctx *c, bool reward_groups, const stmpc_env_cfg *ec, int N, int Kmax, const double *d_ego4, const int32_t *d_k, const double *d_ox,
               const double *d_jerk, const int32_t *d_crashed, const int32_t *d_arrived, double *d_reward, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (reward_groups) TRY(env_shape_check(c, REWARD_GROUPS_ENV));
    env::ECfg e;
    TRY(make_envcfg(ec, &e));
    if (N < 0 || (reward_groups && N > c->env.N) || Kmax < 0 || Kmax > sim::KS)
        return fail(STMPC_EINVAL, "N or Kmax out of range (Kmax <= 64; with reward groups N <= R * n_per_reward_group)");
    if (N == 0) return STMPC_OK;
    if (!d_ego4 || !d_k || !d_jerk || !d_reward || (Kmax > 0 && !d_ox)) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(c->device));
    const dim3 grid((N + 63) / 64), block(64);
    if (reward_groups)
        hipLaunchKernelGGL(env::k_env_reward_rg, grid, block, 0, (hipStream_t)stream, e, c->env.reward_tab(), N, Kmax, d_ego4, d_k, d_ox, d_jerk, d_crashed, d_arrived,
                           d_reward);
    else hipLaunchKernelGGL(env::k_env_reward, grid, block, 0, (hipStream_t)stream, e, N, Kmax, d_ego4, d_k, d_ox, d_jerk, d_crashed, d_arrived, d_reward);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
}  // namespace

extern "C" {

uint64_t stmpc_env_episode_seed(uint64_t seed, uint32_t episode) { return env::episode_seed(seed, episode); }

int stmpc_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, int N, float *d_obs, int obs_stride, void *stream) {
    env::ECfg e;
    TRY(env_reset_check(c, p, ec, d_obs, obs_stride, &e));
    return env_reset(c, g, 0, 0, N, ec, 0, 0, {}, e, d_obs, obs_stride, stream);
}

int stmpc_env_reset_groups_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *cfgs, int G, int n_per_group, const stmpc_env_cfg *ec, float *d_obs,
                                  int obs_stride, void *stream) {
    env::ECfg e;
    TRY(env_reset_check(c, p, ec, d_obs, obs_stride, &e));
    std::vector<sim::Cfg> world;
    TRY(check_groups(cfgs, G, n_per_group, &world));
    return env_reset(c, cfgs, G, n_per_group, 0, ec, 0, 0, {}, e, d_obs, obs_stride, stream);
}

// The reference's per-run reward settings (dqn.py:449-563, rl.py:168-174, merge_gym.py:25,83-140) as a group axis of one vector environment.
int stmpc_reward_groups_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int G, int n_per_traffic_group,
                                         const stmpc_env_cfg *env_cfgs, int R, int n_per_reward_group, float *d_obs, int obs_stride, void *stream) {
    RewardGroupsReset rg;
    TRY(reward_groups_reset_check(c, p, sim_cfgs, G, n_per_traffic_group, env_cfgs, R, n_per_reward_group, d_obs, obs_stride, &rg));
    HIPCHK(hipSetDevice(c->device));
    TRY(c->env.rtab.ensure((size_t)STMPC_ENV_REWARD_GROUPS_MAX * sizeof(env::RewardRow)));   // (its full size once: never reallocated under a running kernel)
    return env_reset(c, sim_cfgs, G, n_per_traffic_group, rg.N, env_cfgs, R, n_per_reward_group, rg.rows, rg.e, d_obs, obs_stride, stream);
}

// The env behind st.do_conditional_st_based_on_first_step (st.py:805-814): the plain reset, then the shield's buffers and zeroed counters.
int stmpc_shield_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, const stmpc_shield_env_cfg *sh, int N,
                                  float *d_obs, int obs_stride, void *stream) {
    ShieldReset r;
    TRY(shield_reset_check(c, p, sh, N, nullptr, 0, 0, &r));
    HIPCHK(hipSetDevice(c->device));
    TRY(stmpc_env_reset_device(c, p, g, ec, N, d_obs, obs_stride, stream));
    return shield_reset_finish(c, sh, r, stream);
}

// st.do_conditional_st_based_on_first_step (st.py:805-814) in front of the traffic-type axis of the reference's experiments (configs/train_*_*.json,
// control.py:215-226): the traffic-groups reset, then the shield's buffers, zeroed counters and the groups' takeover penalties.
int stmpc_shield_traffic_groups_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *cfgs, int G, int n_per_group, const stmpc_env_cfg *ec,
                                         const stmpc_shield_env_cfg *sh, const double *takeover_penalties, int P, float *d_obs, int obs_stride, void *stream) {
    env::ECfg e;
    TRY(env_reset_check(c, p, ec, d_obs, obs_stride, &e));
    std::vector<sim::Cfg> world;
    TRY(check_groups(cfgs, G, n_per_group, &world));
    ShieldReset r;
    TRY(shield_reset_check(c, p, sh, G * n_per_group, takeover_penalties, P, G, &r));
    HIPCHK(hipSetDevice(c->device));
    TRY(env_reset(c, cfgs, G, n_per_group, 0, ec, 0, 0, {}, e, d_obs, obs_stride, stream));
    return shield_reset_finish(c, sh, r, stream);
}

// ... in front of the reference's per-run reward settings (dqn.py:449-563, rl.py:168-174, merge_gym.py:25,83-140): the reward-groups reset (an ungrouped
// world, G = 0, or traffic groups that coincide with the reward groups), then the shield's part.
int stmpc_shield_reward_groups_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int G, int n_per_traffic_group,
                                                const stmpc_env_cfg *env_cfgs, int R, int n_per_reward_group, const stmpc_shield_env_cfg *sh,
                                                const double *takeover_penalties, int P, float *d_obs, int obs_stride, void *stream) {
    RewardGroupsReset rg;
    TRY(reward_groups_reset_check(c, p, sim_cfgs, G, n_per_traffic_group, env_cfgs, R, n_per_reward_group, d_obs, obs_stride, &rg));
    ShieldReset r;
    TRY(shield_reset_check(c, p, sh, rg.N, takeover_penalties, P, R, &r));
    HIPCHK(hipSetDevice(c->device));
    TRY(c->env.rtab.ensure((size_t)STMPC_ENV_REWARD_GROUPS_MAX * sizeof(env::RewardRow)));
    TRY(env_reset(c, sim_cfgs, G, n_per_traffic_group, rg.N, env_cfgs, R, n_per_reward_group, rg.rows, rg.e, d_obs, obs_stride, stream));
    return shield_reset_finish(c, sh, r, stream);
}

int stmpc_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, int N, const void *d_action, float *d_obs, int obs_stride,
                          double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats, void *stream) {
    return env_step(c, p, g, ec, N, PLAIN_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream});
}

int stmpc_env_step_groups_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, int N, const void *d_action, float *d_obs, int obs_stride,
                                 double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats, void *stream) {
    return env_step(c, p, nullptr, ec, N, TRAFFIC_GROUPS_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream});
}

int stmpc_reward_groups_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, int N, const void *d_action, float *d_obs, int obs_stride,
                                        double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats, void *stream) {
    return env_step(c, p, nullptr, ec, N, REWARD_GROUPS_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream});
}

int stmpc_shield_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, const stmpc_shield_env_cfg *sh, int N,
                                 const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                                 float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk,
                                 double *d_executed_action, int32_t *d_takeover_ticks, void *stream) {
    StepExtra x;
    x.shield = sh; x.out = {d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks};
    return env_step(c, p, g, ec, N, SHIELD_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream}, x);
}

// The env behind dqn.RLAgent.do_combined_control (dqn.py:117-200): the plain reset, then every buffer of the step and zeroed counters.
int stmpc_cshield_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, const stmpc_cshield_env_cfg *sh,
                                   const stmpc_actor *actor, int N, float *d_obs, int obs_stride, void *stream) {
    return combined_shield_reset(c, p, g, ec, combined_shield_of(sh, actor), N, d_obs, obs_stride, stream);
}

int stmpc_cshield_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, const stmpc_cshield_env_cfg *sh,
                                  const stmpc_actor *actor, int N, const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated,
                                  uint8_t *d_truncated, float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason,
                                  double *d_executed_jerk, double *d_executed_action, int32_t *d_takeover_ticks, void *stream) {
    const CombinedShield cs = combined_shield_of(sh, actor);
    StepExtra x;
    x.combined = &cs; x.out = {d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks};
    return env_step(c, p, g, ec, N, CSHIELD_ENV_ENTRY, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream}, x);
}

// The discrete envs behind dqn.RLAgent.do_combined_control (dqn.py:117-200) with DQNAgent.get_control (dqn.py:375-380) in the rollout: the same reset
// (no time counter to zero) and the same step (the action index is not rewritten: no d_executed_action).
int stmpc_qshield_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, const stmpc_qshield_env_cfg *sh,
                                   const stmpc_qactor *qactor, const stmpc_qactor_pop *qactor_pop, int n_per_member, int N, float *d_obs, int obs_stride,
                                   void *stream) {
    return combined_shield_reset(c, p, g, ec, combined_shield_of(sh, qactor, qactor_pop, n_per_member), N, d_obs, obs_stride, stream);
}

int stmpc_qshield_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *g, const stmpc_env_cfg *ec, const stmpc_qshield_env_cfg *sh,
                                  const stmpc_qactor *qactor, const stmpc_qactor_pop *qactor_pop, int n_per_member, int N, const void *d_action, float *d_obs,
                                  int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats,
                                  uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk, int32_t *d_takeover_ticks, void *stream) {
    const CombinedShield cs = combined_shield_of(sh, qactor, qactor_pop, n_per_member);
    StepExtra x;
    x.combined = &cs; x.out = {d_takeover, d_reason, d_executed_jerk, nullptr, d_takeover_ticks};
    return env_step(c, p, g, ec, N, QSHIELD_ENV_ENTRY, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream}, x);
}

int stmpc_cshield_env_evals_device(stmpc_ctx *c, int N, int32_t *d_evals, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(env_shape_check(c, CSHIELD_ENV_ENTRY));
    if (N != c->env.N || !d_evals) return fail(STMPC_EINVAL, "N does not match stmpc_cshield_env_reset_device, or NULL device pointer");
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(env::k_cshield_env_evals, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, N, c->cshield.rollout_time, c->sim.state(), env_state(c),
                       c->cshield.view(), d_evals);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

// Domain randomisation over the reference's traffic types (configs/train_*_*.json, control.py:215-226) at the episode boundary.
int stmpc_traffic_mix_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int T, const double *weights, uint64_t mix_seed,
                                       const stmpc_env_cfg *ec, int N, float *d_obs, int obs_stride, int32_t *d_traffic_type, void *stream) {
    env::ECfg e;
    TRY(env_reset_check(c, p, ec, d_obs, obs_stride, &e));
    MixReset mix;
    TRY(check_traffic_mix(sim_cfgs, T, weights, N, &mix));
    mix.seed = mix_seed; mix.d_type = d_traffic_type;
    HIPCHK(hipSetDevice(c->device));
    auto &v = c->env;                            // (their full size once: never reallocated under a running kernel while N does not grow)
    TRY(v.mix_rows.ensure((size_t)STMPC_TRAFFIC_MIX_MAX * sizeof(env::TrafficRow)));
    TRY(v.mix_cum.ensure((size_t)STMPC_TRAFFIC_MIX_MAX * 8));
    TRY(v.mix_type.ensure((size_t)N * 4));
    return env_reset(c, sim_cfgs, 0, 0, N, ec, 0, 0, {}, e, d_obs, obs_stride, stream, &mix);
}

int stmpc_traffic_mix_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, int N, const void *d_action, float *d_obs, int obs_stride,
                                      double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats,
                                      int32_t *d_traffic_type, int32_t *d_final_traffic_type, void *stream) {
    const MixStep mix{d_traffic_type, d_final_traffic_type};
    StepExtra x;
    x.mix = &mix;
    return env_step(c, p, nullptr, ec, N, TRAFFIC_MIX_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream}, x);
}

// ... in front of the traffic mix (one policy across the types of configs/train_*_*.json): the mix's reset, then the shield's part; one takeover penalty,
// shield_cfg's, for every row.
int stmpc_shield_traffic_mix_env_reset_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int T, const double *weights, uint64_t mix_seed,
                                              const stmpc_env_cfg *ec, const stmpc_shield_env_cfg *sh, int N, float *d_obs, int obs_stride, int32_t *d_traffic_type,
                                              void *stream) {
    env::ECfg e;
    TRY(env_reset_check(c, p, ec, d_obs, obs_stride, &e));
    MixReset mix;
    TRY(check_traffic_mix(sim_cfgs, T, weights, N, &mix));
    mix.seed = mix_seed; mix.d_type = d_traffic_type;
    ShieldReset r;
    TRY(shield_reset_check(c, p, sh, N, nullptr, 0, 1, &r));
    HIPCHK(hipSetDevice(c->device));
    auto &v = c->env;
    TRY(v.mix_rows.ensure((size_t)STMPC_TRAFFIC_MIX_MAX * sizeof(env::TrafficRow)));
    TRY(v.mix_cum.ensure((size_t)STMPC_TRAFFIC_MIX_MAX * 8));
    TRY(v.mix_type.ensure((size_t)N * 4));
    TRY(env_reset(c, sim_cfgs, 0, 0, N, ec, 0, 0, {}, e, d_obs, obs_stride, stream, &mix));
    return shield_reset_finish(c, sh, r, stream);
}

// The shielded step (st.py:805-814 in front of merge_gym.py:83-140) of an env with traffic groups, reward groups or a traffic mix: thin entries over env_step.
int stmpc_shield_traffic_groups_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, const stmpc_shield_env_cfg *sh, int N, const void *d_action,
                                        float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs,
                                        double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk, double *d_executed_action,
                                        int32_t *d_takeover_ticks, void *stream) {
    StepExtra x;
    x.shield = sh; x.out = {d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks};
    return env_step(c, p, nullptr, ec, N, SHIELD_TRAFFIC_GROUPS_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream},
                    x);
}

int stmpc_shield_reward_groups_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, const stmpc_shield_env_cfg *sh, int N,
                                               const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                                               float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk,
                                               double *d_executed_action, int32_t *d_takeover_ticks, void *stream) {
    StepExtra x;
    x.shield = sh; x.out = {d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks};
    return env_step(c, p, nullptr, ec, N, SHIELD_REWARD_GROUPS_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream},
                    x);
}

int stmpc_shield_traffic_mix_env_step_device(stmpc_ctx *c, const stmpc_params *p, const stmpc_env_cfg *ec, const stmpc_shield_env_cfg *sh, int N,
                                             const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                                             float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk,
                                             double *d_executed_action, int32_t *d_takeover_ticks, int32_t *d_traffic_type, int32_t *d_final_traffic_type,
                                             void *stream) {
    StepExtra x;
    x.shield = sh; x.out = {d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks};
    const MixStep mix{d_traffic_type, d_final_traffic_type};
    x.mix = &mix;
    return env_step(c, p, nullptr, ec, N, SHIELD_TRAFFIC_MIX_ENV, {d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream},
                    x);
}

int stmpc_traffic_mix_draw(uint64_t mix_seed, int env_index, uint32_t episode, const double *cum, int T) {
    if (!cum || T < 1 || T > STMPC_TRAFFIC_MIX_MAX) return -1;
    return env::mix_draw(mix_seed, env_index, episode, cum, T);
}

int stmpc_env_reward_device(stmpc_ctx *c, const stmpc_env_cfg *ec, int N, int Kmax, const double *d_ego4, const int32_t *d_k, const double *d_ox, const double *d_ov,
                            const double *d_oa, const double *d_jerk, const int32_t *d_crashed, const int32_t *d_arrived, double *d_reward, void *stream) {
    (void)d_ov; (void)d_oa;        // (no reward function reads the other vehicles' speeds or accelerations)
    return env_reward(c, false, ec, N, Kmax, d_ego4, d_k, d_ox, d_jerk, d_crashed, d_arrived, d_reward, stream);
}

int stmpc_reward_groups_env_reward_device(stmpc_ctx *c, const stmpc_env_cfg *ec, int N, int Kmax, const double *d_ego4, const int32_t *d_k, const double *d_ox,
                                          const double *d_ov, const double *d_oa, const double *d_jerk, const int32_t *d_crashed, const int32_t *d_arrived,
                                          double *d_reward, void *stream) {
    (void)d_ov; (void)d_oa;
    return env_reward(c, true, ec, N, Kmax, d_ego4, d_k, d_ox, d_jerk, d_crashed, d_arrived, d_reward, stream);
}

int stmpc_env_drain(stmpc_ctx *c, int max_rows, double *rows, int64_t *n_rows, int64_t *n_dropped) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!n_rows || (max_rows > 0 && !rows)) return fail(STMPC_EINVAL, "NULL host pointer");
    if (c->env.N < 1) return fail(STMPC_EINVAL, "no environment in this context (stmpc_env_reset_device)");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned cnt = 0;
    TRY(download(&cnt, c->env.log_n, 1));
    const int64_t kept = cnt < (unsigned)c->env.log_cap ? (int64_t)cnt : (int64_t)c->env.log_cap;
    const int64_t take = kept < (int64_t)(max_rows > 0 ? max_rows : 0) ? kept : (int64_t)(max_rows > 0 ? max_rows : 0);
    if (take) TRY(download(rows, c->env.log, (size_t)take * env::NLOG));
    HIPCHK(hipMemset(c->env.log_n.p, 0, 4));
    *n_rows = take;
    if (n_dropped) *n_dropped = (int64_t)cnt - take;
    return STMPC_OK;
}

int stmpc_env_episode_ticks_device(stmpc_ctx *c, int N, int32_t *d_ticks, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N != c->env.N || N < 1 || !d_ticks) return fail(STMPC_EINVAL, "N does not match stmpc_env_reset_device, or NULL pointer");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(d_ticks, c->sim.ticks.p, (size_t)N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return STMPC_OK;
}

int stmpc_reward_groups_split(stmpc_ctx *c, int *R, int *n_per_group) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    const bool on = c->env.N >= 1;
    if (R) *R = on ? c->env.R : 0;
    if (n_per_group) *n_per_group = on ? c->env.n_per_rg : 0;
    return STMPC_OK;
}

}  // extern "C"

// ---- episode flight recorder (stmpc_rec_*): per-tick rings and position-binned accumulators; kernels in stmpc_rec_kernels.hpp ----------------------
struct stmpc_rec {
    stmpc_ctx *ctx = nullptr;
    int device = 0;
    rec::Cfg cfg{};
    DevBuf ring, nrec, last_tick, prev_a, acc, red;
    int64_t generation = -1;       // the world (stmpc_ctx::Sim::generation) the recorder follows; -1: none yet (stmpc_rec_reset)
    rec::State state() const { return rec::State{ring.as<double>(), nrec.as<int>(), last_tick.as<int>(), prev_a.as<double>(), acc.as<double>(), red.as<double>()}; }
    size_t ring_len() const { return (size_t)cfg.N * cfg.T * rec::row_width(cfg.Kmax); }
    size_t acc_len() const { return (size_t)rec::acc_rows(cfg.n_edges) * cfg.N; }
};

namespace {
// the recorder follows the world it was reset on: same context, same N, no stmpc_sim_init_device since
int rec_bound(const stmpc_rec *r) {
    if (!r) return fail(STMPC_EINVAL, "recorder is NULL");
    if (r->cfg.N != r->ctx->sim.N || r->generation != r->ctx->sim.generation)
        return fail(STMPC_EINVAL, "the recorder's world was re-initialised (or has another N) since stmpc_rec_reset");
    return STMPC_OK;
}
void rec_launch_reduce(const stmpc_rec *r, hipStream_t st) {
    hipLaunchKernelGGL(rec::k_rec_reduce, dim3(rec::acc_rows(r->cfg.n_edges)), dim3(rec::THREADS), 0, st, r->cfg.N, (const double *)r->acc.p, r->red.as<double>());
}
}  // namespace

extern "C" {

int stmpc_rec_create(stmpc_ctx *c, int N, int Kmax, int depth, double tick_length, const double *edges, int n_edges, stmpc_rec **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (N < 1 || Kmax < 1 || Kmax > STMPC_KMAX_LIMIT) return fail(STMPC_EINVAL, "recorder: N or Kmax out of range");
    if (depth < 1 || depth > STMPC_REC_MAX_DEPTH) return fail(STMPC_EINVAL, "recorder: the ring depth must be in 1 ... STMPC_REC_MAX_DEPTH");
    if (!edges || n_edges < 2 || n_edges > STMPC_REC_MAX_EDGES) return fail(STMPC_EINVAL, "recorder: 2 ... STMPC_REC_MAX_EDGES bin edges");
    if (!(tick_length > 0)) return fail(STMPC_EINVAL, "recorder: tick_length must be positive");
    for (int i = 0; i < n_edges; ++i)
        if (!(fabs(edges[i]) < 1e300) || (i && !(edges[i] > edges[i - 1]))) return fail(STMPC_EINVAL, "recorder: bin edges must be finite and strictly increasing");
    HIPCHK(hipSetDevice(c->device));
    stmpc_rec *r = new stmpc_rec();
    r->ctx = c; r->device = c->device;
    r->cfg.N = N; r->cfg.Kmax = Kmax; r->cfg.T = depth; r->cfg.n_edges = n_edges; r->cfg.tick = tick_length;
    for (int i = 0; i < n_edges; ++i) r->cfg.edges[i] = edges[i];
    const size_t n = (size_t)N;
    int rc = r->ring.ensure(r->ring_len() * 8);
    if (!rc) rc = r->nrec.ensure(n * 4);
    if (!rc) rc = r->last_tick.ensure(n * 4);
    if (!rc) rc = r->prev_a.ensure(n * 8);
    if (!rc) rc = r->acc.ensure(r->acc_len() * 8);
    if (!rc) rc = r->red.ensure((size_t)rec::acc_rows(n_edges) * 8);
    if (!rc && c->sim.N == N) rc = stmpc_rec_reset(r, nullptr);      // (a world of this size exists: follow it from here)
    if (rc) { delete r; return rc; }
    *out = r;
    return STMPC_OK;
}

void stmpc_rec_destroy(stmpc_rec *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}

int stmpc_rec_reset(stmpc_rec *r, void *stream) {
    if (!r) return fail(STMPC_EINVAL, "recorder is NULL");
    if (r->cfg.N != r->ctx->sim.N) return fail(STMPC_EINVAL, "recorder: N does not match stmpc_sim_init_device");
    HIPCHK(hipSetDevice(r->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)r->cfg.N;
    HIPCHK(hipMemsetAsync(r->ring.p, 0, r->ring_len() * 8, st));
    HIPCHK(hipMemsetAsync(r->nrec.p, 0, n * 4, st));
    HIPCHK(hipMemsetAsync(r->last_tick.p, 0, n * 4, st));
    HIPCHK(hipMemsetAsync(r->prev_a.p, 0, n * 8, st));
    HIPCHK(hipMemsetAsync(r->acc.p, 0, r->acc_len() * 8, st));
    HIPCHK(hipMemsetAsync(r->red.p, 0, (size_t)rec::acc_rows(r->cfg.n_edges) * 8, st));
    r->generation = r->ctx->sim.generation;
    return STMPC_OK;
}

int stmpc_rec_tick_device(stmpc_rec *r, int N, int Kmax, const double *d_ego5, const int32_t *d_k, const double *d_ox, const double *d_ov, const double *d_oa,
                          const double *d_cmd_speed, const int32_t *d_takeover, void *stream) {
    TRY(rec_bound(r));
    if (N != r->cfg.N || Kmax != r->cfg.Kmax) return fail(STMPC_EINVAL, "recorder: N or Kmax differ from stmpc_rec_create's");
    if (!d_ego5 || !d_k || !d_ox || !d_ov || !d_cmd_speed) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(r->ctx->device));
    const sim::State s = r->ctx->sim.state();
    hipLaunchKernelGGL(rec::k_rec_tick, dim3((N + rec::G - 1) / rec::G), dim3(rec::THREADS), 0, (hipStream_t)stream, r->cfg, r->state(), (const int *)s.status,
                       (const int *)s.ticks, d_ego5, d_k, d_ox, d_ov, d_oa, d_cmd_speed, d_takeover);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_rec_reduce_device(stmpc_rec *r, double *d_out, void *stream) {
    TRY(rec_bound(r));
    HIPCHK(hipSetDevice(r->ctx->device));
    rec_launch_reduce(r, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    if (d_out) HIPCHK(hipMemcpyAsync(d_out, r->red.p, (size_t)rec::acc_rows(r->cfg.n_edges) * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return STMPC_OK;
}

int stmpc_rec_read(stmpc_rec *r, double *ring, int32_t *length, double *acc_env, double *acc_reduced, int32_t *status) {
    TRY(rec_bound(r));
    HIPCHK(hipSetDevice(r->ctx->device));
    HIPCHK(hipDeviceSynchronize());
    const int N = r->cfg.N, T = r->cfg.T, W = rec::row_width(r->cfg.Kmax);
    const size_t n = (size_t)N;
    if (ring || length) {
        std::vector<int32_t> nrec(n), last(n);
        TRY(download(nrec.data(), r->nrec, n)); TRY(download(last.data(), r->last_tick, n));
        std::vector<double> raw;
        if (ring) { raw.resize(r->ring_len()); TRY(download(raw.data(), r->ring, raw.size())); }
        for (int e = 0; e < N; ++e) {
            const int len = nrec[e] < T ? nrec[e] : T;
            if (length) length[e] = len;
            if (!ring) continue;
            double *dst = ring + (size_t)e * T * W;
            // chronological order: the newest record sits in slot last % T, the ones before it in the slots before that (the world's tick counts up by one per record)
            for (int i = 0; i < len; ++i) {
                const int slot = ((last[e] - (len - 1 - i)) % T + T) % T;
                memcpy(dst + (size_t)i * W, raw.data() + ((size_t)e * T + slot) * W, (size_t)W * 8);
            }
            if (len < T) memset(dst + (size_t)len * W, 0, (size_t)(T - len) * W * 8);
        }
    }
    TRY(download(acc_env, r->acc, r->acc_len()));
    if (acc_reduced) {
        rec_launch_reduce(r, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        TRY(download(acc_reduced, r->red, (size_t)rec::acc_rows(r->cfg.n_edges)));
    }
    TRY(download(status, r->ctx->sim.status, n));
    return STMPC_OK;
}

}  // extern "C"
