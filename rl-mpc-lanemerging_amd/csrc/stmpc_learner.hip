// stmpc_learner.hip -- the DDPG learner and its population (stmpc_ddpg_*, stmpc_ddpg_pop_*), the TD3 learner on top of it and its population (stmpc_td3_*, stmpc_pop_td3_*), prioritised replay for the two lone learners (stmpc_per_*) and for the two populations (stmpc_pop_per_*), actors that view a learner's networks
// (stmpc_actor_view_ddpg), the population of actors (stmpc_actor_pop_*) and the DQN learner for the discrete envs (stmpc_dqn_*).  struct stmpc_actor and the actor's checks are stmpc.hip's (stmpc_host.hpp).
#include "stmpc_host.hpp"      // (the context, the shared helpers, the kernel headers the context needs)
#include "stmpc_ddpg_kernels.hpp"
#include "stmpc_per_kernels.hpp"
#include "stmpc_ddpg_pop_kernels.hpp"
#include "stmpc_td3_kernels.hpp"
#include "stmpc_td3_pop_kernels.hpp"
#include "stmpc_per_pop_kernels.hpp"
#include "stmpc_actor_pop_kernels.hpp"

// ---- DDPG learner (stmpc_ddpg_*): replay ring, fused update, acting; kernels in stmpc_ddpg_kernels.hpp -------------------------------------------
struct stmpc_ddpg {
    int device = 0;
    stmpc_ddpg_cfg cfg{};
    DdpgDev dev{};
    DevBuf netbuf[2][13], ring, cnt, tick, ws[7];
    int h1p = 0, h2p = 0, np = 0, Bp = 0;
    size_t lds = 0;
    bool td3_base = false;          // lent by a stmpc_td3 (stmpc_td3_base): an update or gradients of this handle alone would leave critic 2 behind
    struct stmpc_td3 *td3_owner = nullptr;  // that stmpc_td3: it holds copies of dev (its two views), which stmpc_per_enable has to follow
    bool pop_member = false;        // owned by a population, whose device table holds a copy of dev
    bool per = false;               // prioritised replay (stmpc_per_enable, stmpc_pop_per_enable_*): dev.tree ... dev.per_L are set
    DevBuf per_tree, per_idx, per_aw, per_atd, per_atd2;    // (per_atd2: critic 2's Q - y, when td3_owner)
    int n_in(int which) const { return cfg.n_obs + 1 + which; }
    int64_t slot_len(int which) const { const int64_t n = n_in(which); return (int64_t)cfg.h1 * n + cfg.h1 + (int64_t)cfg.h2 * cfg.h1 + cfg.h2 + cfg.h2 + 1; }
};

namespace {
int ddpg_zero(DevBuf &b, size_t bytes) {
    TRY(b.ensure(bytes));
    HIPCHK(hipMemset(b.p, 0, bytes));
    return STMPC_OK;
}
float *ddpg_slot_ptr(stmpc_ddpg *l, int slot) {
    const DdpgNet &n = slot >= 4 ? l->dev.q : l->dev.pi;
    switch (slot & 3) { case 0: return n.w; case 1: return n.wt; case 2: return n.m; default: return n.v; }
}
// slot layout (unpadded) <-> padded layout, on the host
void ddpg_pad(const stmpc_ddpg *l, int n_in, const float *flat, std::vector<float> &pad, bool to_pad, float *flat_out) {
    const int h1 = l->cfg.h1, h2 = l->cfg.h2, h1p = l->h1p, h2p = l->h2p;
    size_t i = 0;
    auto item = [&](size_t p) { if (to_pad) pad[p] = flat[i]; else flat_out[i] = pad[p]; ++i; };
    for (int n = 0; n < h1; ++n) for (int k = 0; k < n_in; ++k) item((size_t)n * AT_KIN + k);
    for (int n = 0; n < h1; ++n) item((size_t)dg_o_b0(h1p) + n);
    for (int n = 0; n < h2; ++n) for (int k = 0; k < h1; ++k) item((size_t)dg_o_w1(h1p) + (size_t)n * h1p + k);
    for (int n = 0; n < h2; ++n) item((size_t)dg_o_b1(h1p, h2p) + n);
    for (int n = 0; n < h2; ++n) item((size_t)dg_o_w2(h1p, h2p) + n);
    item((size_t)dg_o_b2(h1p, h2p));
}
// dynamic LDS of the three per-tile kernels of a learner (pop = false) or of a population (true): raised, never lowered (raise_dynamic_lds)
int ddpg_raise_lds(bool pop, int device, size_t lds) {
    static LdsCeiling ceiling[2][3];
    static const void *const fn[2][3] = {{(const void *)k_ddpg_critic_fwd, (const void *)k_ddpg_actor_fwd, (const void *)k_ddpg_act},
                                         {(const void *)k_ddpg_critic_fwd_pop, (const void *)k_ddpg_actor_fwd_pop, (const void *)k_ddpg_act_pop}};
    static const char *const name[2][3] = {{"k_ddpg_critic_fwd", "k_ddpg_actor_fwd", "k_ddpg_act"}, {"k_ddpg_critic_fwd_pop", "k_ddpg_actor_fwd_pop", "k_ddpg_act_pop"}};
    for (int i = 0; i < 3; ++i) TRY(raise_dynamic_lds(fn[pop][i], name[pop][i], ceiling[pop][i], device, lds));
    return STMPC_OK;
}
// the host twin of dg_gauss: the standard normal of one hash in fp64, and its two draws
double ddpg_gauss_host(unsigned long long h, uint32_t *draw1, uint32_t *draw2) {
    const uint32_t u1 = (uint32_t)(h >> 40), u2 = (uint32_t)((h >> 8) & 0xFFFFFFull);
    if (draw1) *draw1 = u1;
    if (draw2) *draw2 = u2;
    const double f1 = ((double)u1 + 1.0) * 5.9604644775390625e-8;
    const volatile float theta = 6.2831855f * ((float)u2 * 5.9604644775390625e-8f);      // the float32 product the kernel forms
    return sqrt(-2.0 * log(f1)) * cos((double)theta);
}
// prioritised replay: the sampling step in front of a pass that gathers (nothing on a learner that samples uniformly)
void per_launch_sample(const stmpc_ddpg *l, int gate, hipStream_t st) {
    if (l->per) hipLaunchKernelGGL(k_per_sample, dim3(1), dim3(PER_THREADS), 0, st, l->dev, l->cfg.batch, l->Bp, gate);
}
// ... and the priority update behind the critic pass
void per_launch_update(const stmpc_ddpg *l, hipStream_t st) {
    if (l->per) hipLaunchKernelGGL(k_per_update, dim3(1), dim3(PER_THREADS), 0, st, l->dev, (const float *)l->per_atd2.as<float>(), l->cfg.batch, 1);
}
void ddpg_launch_grads(stmpc_ddpg *l, int which, int gate, hipStream_t st) {
    const int tiles = l->Bp / AT_TM, t1 = l->h2p / 16, t0 = l->h1p / 16;
    if (which) hipLaunchKernelGGL(k_ddpg_critic_fwd, dim3(tiles), dim3(AT_THREADS), l->lds, st, l->dev, l->cfg.batch, gate);
    else hipLaunchKernelGGL(k_ddpg_actor_fwd, dim3(tiles), dim3(AT_THREADS), l->lds, st, l->dev, l->cfg.batch, gate);
    hipLaunchKernelGGL(k_ddpg_wgrad, dim3(t1 * t0 + 2 * t0 + t1 + t0 + t1 + 1), dim3(64 * DG_WG_WAVES), 0, st, l->dev, which, l->Bp, gate);
}
void ddpg_launch_adam(stmpc_ddpg *l, int which, float lr, int mode, int bump, hipStream_t st) {
    hipLaunchKernelGGL(k_ddpg_adam, dim3((l->np + 255) / 256), dim3(256), 0, st, l->dev, which, lr, mode, bump, 1);
}
}  // namespace

extern "C" {

int stmpc_ddpg_create(stmpc_ctx *c, const stmpc_ddpg_cfg *g, stmpc_ddpg **out) {
    if (!c || !g || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (g->n_obs < 1 || g->n_obs > AT_KIN - 2 || g->h1 < 1 || g->h1 > 1024 || g->h2 < 1 || g->h2 > 1024) return fail(STMPC_EINVAL, "DDPG network shape out of range (n_obs <= 30, hidden widths <= 1024)");
    if (g->batch < 16 || g->batch > 8192) return fail(STMPC_EINVAL, "batch must be in 16 ... 8192");
    if (g->capacity < 1 || g->replay_start < 0 || g->replay_start >= g->capacity) return fail(STMPC_EINVAL, "capacity must be positive and replay_start below it");
    if (!(g->gamma >= 0) || !(g->tau >= 0 && g->tau <= 1) || !(g->beta1 >= 0 && g->beta1 < 1) || !(g->beta2 >= 0 && g->beta2 < 1) || !(g->eps > 0) ||
        !(g->noise_std >= 0) || !(g->action_low <= g->action_high)) return fail(STMPC_EINVAL, "DDPG constants out of range");
    HIPCHK(hipSetDevice(c->device));
    stmpc_ddpg *l = new stmpc_ddpg();
    l->device = c->device; l->cfg = *g;
    const int h1p = l->h1p = (g->h1 + 15) & ~15, h2p = l->h2p = (g->h2 + 15) & ~15;
    const int np = l->np = dg_nparam(h1p, h2p), Bp = l->Bp = (g->batch + 15) & ~15;
    l->lds = ddpg_tile_bytes(h1p, h2p);
    if (l->lds + 1024 > (size_t)c->lds_per_block) { delete l; return fail(STMPC_EINVAL, "DDPG networks too wide for one workgroup's LDS"); }
    DdpgDev &d = l->dev;
    int rc = 0;
    for (int w = 0; w < 2 && !rc; ++w) {
        DdpgNet &n = w ? d.q : d.pi;
        float **ptr[13] = {&n.w, &n.wt, &n.m, &n.v, &n.g, &n.p0, &n.p1, &n.p1t, &n.t0, &n.t1, &n.bpow, nullptr, nullptr};
        const size_t len[11] = {(size_t)np, (size_t)np, (size_t)np, (size_t)np, (size_t)np, (size_t)h1p * AT_KIN, (size_t)h2p * h1p, (size_t)h2p * h1p,
                                (size_t)h1p * AT_KIN, (size_t)h2p * h1p, 4};
        for (int i = 0; i < 11 && !rc; ++i) { rc = ddpg_zero(l->netbuf[w][i], len[i] * sizeof(float)); *ptr[i] = l->netbuf[w][i].as<float>(); }
        n.n_in = l->n_in(w);
    }
    const size_t wlen[7] = {(size_t)Bp * AT_KIN, (size_t)Bp * h1p, (size_t)Bp * h2p, (size_t)Bp * h2p, (size_t)Bp * h1p, (size_t)Bp, (size_t)Bp * 2};
    float **wptr[7] = {&d.aX, &d.aH1, &d.aH2, &d.aD2, &d.aD1, &d.adz, &d.arow};
    for (int i = 0; i < 7 && !rc; ++i) { rc = ddpg_zero(l->ws[i], wlen[i] * sizeof(float)); *wptr[i] = l->ws[i].as<float>(); }
    if (!rc) rc = ddpg_zero(l->ring, (size_t)g->capacity * DG_ROW * sizeof(float));
    if (!rc) rc = ddpg_zero(l->cnt, DG_NCNT * sizeof(long long));
    if (!rc) rc = ddpg_zero(l->tick, DG_NTICK * sizeof(unsigned int));
    if (!rc) rc = ddpg_raise_lds(false, l->device, l->lds);
    if (rc) { stmpc_ddpg_destroy(l); return rc; }
    d.ring = l->ring.as<float>(); d.cnt = l->cnt.as<long long>(); d.tick = l->tick.as<unsigned int>();
    d.n_obs = g->n_obs; d.h1 = g->h1; d.h2 = g->h2; d.h1p = h1p; d.h2p = h2p; d.capacity = g->capacity; d.replay_start = g->replay_start; d.seed = g->seed;
    d.gamma = (float)g->gamma; d.tau = (float)g->tau; d.beta1 = (float)g->beta1; d.beta2 = (float)g->beta2;
    d.omb1 = 1.0f - d.beta1; d.omb2 = 1.0f - d.beta2; d.omtau = 1.0f - d.tau; d.eps = (float)g->eps; d.time_scale = (float)g->time_scale;
    d.scale = (float)g->tanh_scale; d.mean = (float)g->tanh_mean; d.noise_std = (float)g->noise_std; d.a_low = (float)g->action_low; d.a_high = (float)g->action_high;
    const float one[4] = {1.f, 1.f, 0.f, 0.f};                       // beta^0
    HIPCHK(hipMemcpy(d.pi.bpow, one, sizeof one, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.q.bpow, one, sizeof one, hipMemcpyHostToDevice));
    *out = l;
    return STMPC_OK;
}

void stmpc_ddpg_destroy(stmpc_ddpg *l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    delete l;
}

int stmpc_ddpg_set_params(stmpc_ddpg *l, int slot, const float *values, int64_t count) {
    if (!l || !values || slot < 0 || slot > 7) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    const int which = slot >= 4;
    if (count != l->slot_len(which)) return fail(STMPC_EINVAL, "count is not the length of this slot");
    HIPCHK(hipSetDevice(l->device));
    std::vector<float> pad((size_t)l->np, 0.f);
    ddpg_pad(l, l->n_in(which), values, pad, true, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(ddpg_slot_ptr(l, slot), pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
    if ((slot & 3) < 2) {                                            // the packed copies follow the parameters
        ddpg_launch_adam(l, which, 0.f, 1, 0, (hipStream_t)0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    }
    return STMPC_OK;
}

int stmpc_ddpg_get_params(stmpc_ddpg *l, int slot, float *values, int64_t count) {
    if (!l || !values || slot < 0 || slot > 7) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    const int which = slot >= 4;
    if (count != l->slot_len(which)) return fail(STMPC_EINVAL, "count is not the length of this slot");
    HIPCHK(hipSetDevice(l->device));
    std::vector<float> pad((size_t)l->np, 0.f);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pad.data(), ddpg_slot_ptr(l, slot), pad.size() * sizeof(float), hipMemcpyDeviceToHost));
    ddpg_pad(l, l->n_in(which), nullptr, pad, false, values);
    return STMPC_OK;
}

int stmpc_ddpg_set_state(stmpc_ddpg *l, const int64_t *counters, const float *beta_pow) {
    if (!l || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    if (counters[DG_CURSOR] < 0 || counters[DG_CURSOR] >= l->cfg.capacity || counters[DG_FILL] < 0 || counters[DG_FILL] > l->cfg.capacity || counters[DG_UPDATES] < 0 ||
        counters[DG_ACTS] < 0 || counters[DG_FRAMES] < 0) return fail(STMPC_EINVAL, "counters out of range");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipDeviceSynchronize());
    long long cn[DG_NCNT];
    if (l->per) {                                                    // the tree's leaves follow the ring's cursor and fill
        HIPCHK(hipMemcpy(cn, l->dev.cnt, sizeof cn, hipMemcpyDeviceToHost));
        if (cn[DG_CURSOR] != counters[DG_CURSOR] || cn[DG_FILL] != counters[DG_FILL])
            return fail(STMPC_EINVAL, "prioritised replay is enabled: the ring's cursor and fill cannot be set (the priorities belong to the rows pushed)");
    }
    for (int i = 0; i < DG_NCNT; ++i) cn[i] = i <= DG_FRAMES ? counters[i] : 0;
    HIPCHK(hipMemcpy(l->dev.cnt, cn, sizeof cn, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(l->dev.pi.bpow, beta_pow, 2 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(l->dev.q.bpow, beta_pow + 2, 2 * sizeof(float), hipMemcpyHostToDevice));
    return STMPC_OK;
}

int stmpc_ddpg_get_state(stmpc_ddpg *l, int64_t *counters, float *beta_pow) {
    if (!l || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipDeviceSynchronize());
    long long cn[DG_NCNT];
    HIPCHK(hipMemcpy(cn, l->dev.cnt, sizeof cn, hipMemcpyDeviceToHost));
    for (int i = 0; i < DG_NCNT; ++i) counters[i] = cn[i];
    HIPCHK(hipMemcpy(beta_pow, l->dev.pi.bpow, 2 * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(beta_pow + 2, l->dev.q.bpow, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

int stmpc_ddpg_push_device(stmpc_ddpg *l, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_ticks,
                           const int32_t *d_next_ticks, const double *d_action, const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated,
                           void *stream) {
    if (!l) return fail(STMPC_EINVAL, "learner is NULL");
    if (N < 0 || N > l->cfg.capacity || obs_stride < l->cfg.n_obs) return fail(STMPC_EINVAL, "N exceeds the replay capacity, or obs_stride is shorter than the observation");
    if (N == 0) return STMPC_OK;
    if (!d_obs || !d_next_obs || !d_ticks || !d_action || !d_reward || !d_terminated || !d_truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(l->device));
    const long long items = (long long)N * DG_ROW;
    const int blocks = (int)((items + 255) / 256 < 1024 ? (items + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_replay_push, dim3(blocks), dim3(256), 0, (hipStream_t)stream, l->dev, N, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks,
                       d_action, d_reward, d_terminated, d_truncated);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_act_device(stmpc_ddpg *l, int N, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise, double *d_action, uint32_t *d_debug,
                          void *stream) {
    if (!l) return fail(STMPC_EINVAL, "learner is NULL");
    if (N < 0 || obs_stride < l->cfg.n_obs) return fail(STMPC_EINVAL, "N negative, or obs_stride shorter than the observation");
    if (N == 0) return STMPC_OK;
    if (!d_obs || !d_ticks || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(l->device));
    hipLaunchKernelGGL(k_ddpg_act, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), l->lds, (hipStream_t)stream, l->dev, N, d_obs, obs_stride, d_ticks, noise != 0,
                       d_action, d_debug);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_update_device(stmpc_ddpg *l, int n_updates, double lr_q, double lr_pi, void *stream) {
    if (!l) return fail(STMPC_EINVAL, "learner is NULL");
    if (l->td3_base) return fail(STMPC_EINVAL, "this learner is the base of a TD3 learner: update it with stmpc_td3_update_device");
    if (n_updates < 0 || !(lr_q >= 0) || !(lr_pi >= 0)) return fail(STMPC_EINVAL, "n_updates or a learning rate is negative");
    HIPCHK(hipSetDevice(l->device));
    for (int u = 0; u < n_updates; ++u) {
        per_launch_sample(l, 1, (hipStream_t)stream);
        ddpg_launch_grads(l, 1, 1, (hipStream_t)stream);
        per_launch_update(l, (hipStream_t)stream);
        ddpg_launch_adam(l, 1, (float)lr_q, 0, 0, (hipStream_t)stream);
        ddpg_launch_grads(l, 0, 1, (hipStream_t)stream);
        ddpg_launch_adam(l, 0, (float)lr_pi, 0, 1, (hipStream_t)stream);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_grads_device(stmpc_ddpg *l, float *d_grad_actor, float *d_grad_critic, void *stream) {
    if (!l || !d_grad_actor || !d_grad_critic) return fail(STMPC_EINVAL, "NULL argument");
    if (l->td3_base) return fail(STMPC_EINVAL, "this learner is the base of a TD3 learner: take its gradients with stmpc_td3_grads_device");
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = (hipStream_t)stream;
    per_launch_sample(l, 0, st);
    ddpg_launch_grads(l, 1, 0, st);
    hipLaunchKernelGGL(k_ddpg_unpad, dim3(128), dim3(256), 0, st, l->dev, l->n_in(1), (const float *)l->dev.q.g, d_grad_critic);
    ddpg_launch_grads(l, 0, 0, st);
    hipLaunchKernelGGL(k_ddpg_unpad, dim3(128), dim3(256), 0, st, l->dev, l->n_in(0), (const float *)l->dev.pi.g, d_grad_actor);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_stats_device(stmpc_ddpg *l, double *d_out, void *stream) {
    if (!l || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(l->device));
    hipLaunchKernelGGL(k_ddpg_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, l->dev, l->cfg.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_replay_read(stmpc_ddpg *l, int64_t first, int64_t count, float *rows) {
    if (!l || !rows) return fail(STMPC_EINVAL, "NULL argument");
    if (first < 0 || count < 0 || first + count > l->cfg.capacity) return fail(STMPC_EINVAL, "rows outside the ring");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipDeviceSynchronize());
    if (count) HIPCHK(hipMemcpy(rows, l->dev.ring + (size_t)first * DG_ROW, (size_t)count * DG_ROW * sizeof(float), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

int stmpc_ddpg_gather_device(stmpc_ddpg *l, float *d_rows, void *stream) {
    if (!l || !d_rows) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(l->device));
    per_launch_sample(l, 0, (hipStream_t)stream);
    hipLaunchKernelGGL(k_replay_gather, dim3((l->cfg.batch * DG_ROW + 255) / 256), dim3(256), 0, (hipStream_t)stream, l->dev, l->cfg.batch, d_rows);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

uint64_t stmpc_ddpg_sample_index(uint64_t seed, uint64_t update, uint32_t row, uint64_t fill) {
    return fill ? (uint64_t)(dg_hash(seed, update, row) % fill) : 0;
}

double stmpc_ddpg_noise(uint64_t seed, uint64_t call, uint32_t row, uint32_t *draw1, uint32_t *draw2) {
    return ddpg_gauss_host(dg_hash(seed ^ DG_NOISE_STREAM, call, row), draw1, draw2);
}

}  // extern "C"

// ---- DDPG population (stmpc_ddpg_pop_*): P learners of the section above, one launch per kernel; kernels in stmpc_ddpg_pop_kernels.hpp ------------
struct stmpc_ddpg_pop {
    int device = 0;
    std::vector<stmpc_ddpg *> members;      // owned; made by stmpc_ddpg_create, so every single-learner entry works on a borrowed member
    DevBuf table;                           // DdpgDev [P]: the members' structs (their pointers and constants change once at most: stmpc_pop_per_enable_ddpg)
    bool per_called = false, per_any = false;   // stmpc_pop_per_enable_ddpg was called; at least one member has a tree
    int P() const { return (int)members.size(); }
    const DdpgDev *dev() const { return table.as<DdpgDev>(); }
};

static_assert(DG_POP_MAX == STMPC_DDPG_POP_MAX, "DdpgLr holds one learning rate per possible member");

namespace {
int ddpg_pop_lrs(int P, const double *lr, DdpgLr &out) {
    for (int m = 0; m < P; ++m) {
        if (!(lr[m] >= 0)) return fail(STMPC_EINVAL, "a member's learning rate is negative");
        out.lr[m] = (float)lr[m];
    }
    return STMPC_OK;
}
// acting and pushing of P members whose DdpgDev are table[0 ... P): the DDPG population's own, and a TD3 population's on its members' bases
int ddpg_pop_act(int device, const DdpgDev *table, int P, const stmpc_ddpg *l0, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise,
                 double *d_action, uint32_t *d_debug, void *stream) {
    if (n_per_member < 1 || n_per_member > l0->cfg.capacity || obs_stride < l0->cfg.n_obs)
        return fail(STMPC_EINVAL, "n_per_member must be in 1 ... capacity, and obs_stride at least the observation's width");
    if (!d_obs || !d_ticks || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(k_ddpg_act_pop, dim3((n_per_member + AT_TM - 1) / AT_TM, P), dim3(AT_THREADS), l0->lds, (hipStream_t)stream, table, n_per_member, d_obs,
                       obs_stride, d_ticks, noise != 0, d_action, d_debug);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
int ddpg_pop_push(int device, const DdpgDev *table, int P, const stmpc_ddpg *l0, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs,
                  int obs_stride, const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward, const uint8_t *d_terminated,
                  const uint8_t *d_truncated, void *stream) {
    if (n_per_member < 1 || n_per_member > l0->cfg.capacity || obs_stride < l0->cfg.n_obs)
        return fail(STMPC_EINVAL, "n_per_member must be in 1 ... capacity, and obs_stride at least the observation's width");
    if (!d_obs || !d_next_obs || !d_ticks || !d_action || !d_reward || !d_terminated || !d_truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(device));
    const long long items = (long long)n_per_member * DG_ROW;       // per member: stmpc_ddpg_push_device's block count
    const int blocks = (int)((items + 255) / 256 < 1024 ? (items + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_replay_push_pop, dim3(blocks, P), dim3(256), 0, (hipStream_t)stream, table, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride,
                       d_ticks, d_next_ticks, d_action, d_reward, d_terminated, d_truncated);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
}  // namespace

extern "C" {

int stmpc_ddpg_pop_create(stmpc_ctx *c, const stmpc_ddpg_cfg *cfgs, int P, stmpc_ddpg_pop **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (P < 1 || P > DG_POP_MAX) return fail(STMPC_EINVAL, "a population has 1 ... 64 members, not " + std::to_string(P));
    if (!cfgs) return fail(STMPC_EINVAL, "NULL argument");
    for (int m = 1; m < P; ++m)
        if (cfgs[m].n_obs != cfgs[0].n_obs || cfgs[m].h1 != cfgs[0].h1 || cfgs[m].h2 != cfgs[0].h2 || cfgs[m].batch != cfgs[0].batch || cfgs[m].capacity != cfgs[0].capacity)
            return fail(STMPC_EINVAL, "the members of a population share n_obs, h1, h2, batch and capacity (member " + std::to_string(m) + " differs from member 0)");
    HIPCHK(hipSetDevice(c->device));
    stmpc_ddpg_pop *p = new stmpc_ddpg_pop();
    p->device = c->device;
    int rc = STMPC_OK;
    std::vector<DdpgDev> host;
    for (int m = 0; m < P && !rc; ++m) {
        stmpc_ddpg *l = nullptr;
        rc = stmpc_ddpg_create(c, cfgs + m, &l);
        if (!rc) { l->pop_member = true; p->members.push_back(l); host.push_back(l->dev); }
    }
    if (!rc) rc = p->table.ensure(host.size() * sizeof(DdpgDev));
    if (!rc && hipMemcpy(p->table.p, host.data(), host.size() * sizeof(DdpgDev), hipMemcpyHostToDevice) != hipSuccess) rc = fail(STMPC_EHIP, "hipMemcpy of the member table failed");
    if (!rc) rc = ddpg_raise_lds(true, p->device, p->members[0]->lds);
    if (rc) { stmpc_ddpg_pop_destroy(p); return rc; }
    *out = p;
    return STMPC_OK;
}

void stmpc_ddpg_pop_destroy(stmpc_ddpg_pop *p) {
    if (!p) return;
    for (stmpc_ddpg *l : p->members) stmpc_ddpg_destroy(l);
    (void)hipSetDevice(p->device);
    delete p;
}

int stmpc_ddpg_pop_size(const stmpc_ddpg_pop *p) { return p ? p->P() : 0; }

stmpc_ddpg *stmpc_ddpg_pop_member(stmpc_ddpg_pop *p, int m) {
    if (!p || m < 0 || m >= p->P()) { (void)fail(STMPC_EINVAL, "population is NULL, or no such member"); return nullptr; }
    return p->members[m];
}

int stmpc_ddpg_pop_act_device(stmpc_ddpg_pop *p, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise, double *d_action,
                              uint32_t *d_debug, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return ddpg_pop_act(p->device, p->dev(), p->P(), p->members[0], n_per_member, d_obs, obs_stride, d_ticks, noise, d_action, d_debug, stream);
}

int stmpc_ddpg_pop_push_device(stmpc_ddpg_pop *p, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                               const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward, const uint8_t *d_terminated,
                               const uint8_t *d_truncated, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return ddpg_pop_push(p->device, p->dev(), p->P(), p->members[0], n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks, d_action, d_reward,
                         d_terminated, d_truncated, stream);
}

int stmpc_ddpg_pop_update_device(stmpc_ddpg_pop *p, int n_updates, const double *lr_q, const double *lr_pi, int n_lr, void *stream) {
    if (!p || !lr_q || !lr_pi) return fail(STMPC_EINVAL, "NULL argument");
    if (n_lr != p->P()) return fail(STMPC_EINVAL, "the learning-rate arrays have " + std::to_string(n_lr) + " entries, the population " + std::to_string(p->P()) + " members");
    if (n_updates < 0) return fail(STMPC_EINVAL, "n_updates is negative");
    DdpgLr lq{}, lp{};
    TRY(ddpg_pop_lrs(p->P(), lr_q, lq));
    TRY(ddpg_pop_lrs(p->P(), lr_pi, lp));
    HIPCHK(hipSetDevice(p->device));
    const stmpc_ddpg *l = p->members[0];
    const int P = p->P(), tiles = l->Bp / AT_TM, t1 = l->h2p / 16, t0 = l->h1p / 16, jobs = t1 * t0 + 2 * t0 + t1 + t0 + t1 + 1, ablocks = (l->np + 255) / 256;
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // stmpc_ddpg_update_device's six launches (eight with prioritised members), each over the members
        if (p->per_any) hipLaunchKernelGGL(k_per_sample_pop, dim3(1, P), dim3(PER_THREADS), 0, st, p->dev(), l->cfg.batch, l->Bp, 1);
        hipLaunchKernelGGL(k_ddpg_critic_fwd_pop, dim3(tiles, P), dim3(AT_THREADS), l->lds, st, p->dev(), l->cfg.batch, 1);
        hipLaunchKernelGGL(k_ddpg_wgrad_pop, dim3(jobs, P), dim3(64 * DG_WG_WAVES), 0, st, p->dev(), 1, l->Bp, 1);
        if (p->per_any) hipLaunchKernelGGL(k_per_update_pop, dim3(1, P), dim3(PER_THREADS), 0, st, p->dev(), l->cfg.batch, 1);
        hipLaunchKernelGGL(k_ddpg_adam_pop, dim3(ablocks, P), dim3(256), 0, st, p->dev(), 1, lq, 0, 0, 1);
        hipLaunchKernelGGL(k_ddpg_actor_fwd_pop, dim3(tiles, P), dim3(AT_THREADS), l->lds, st, p->dev(), l->cfg.batch, 1);
        hipLaunchKernelGGL(k_ddpg_wgrad_pop, dim3(jobs, P), dim3(64 * DG_WG_WAVES), 0, st, p->dev(), 0, l->Bp, 1);
        hipLaunchKernelGGL(k_ddpg_adam_pop, dim3(ablocks, P), dim3(256), 0, st, p->dev(), 0, lp, 0, 1, 1);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_pop_stats_device(stmpc_ddpg_pop *p, double *d_out, void *stream) {
    if (!p || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->device));
    hipLaunchKernelGGL(k_ddpg_stats_pop, dim3(1, p->P()), dim3(64), 0, (hipStream_t)stream, p->dev(), p->members[0]->cfg.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

}  // extern "C"

// ---- TD3 learner (stmpc_td3_*): a DDPG learner as base (actor, critic 1, ring, counters) plus critic 2; kernels in stmpc_td3_kernels.hpp -----------
struct stmpc_td3 {
    stmpc_ddpg *base = nullptr;             // owned; lent out by stmpc_td3_base
    stmpc_td3_cfg cfg{};
    Td3Dev dev{};
    DevBuf net2[11], ws2[7], tick;          // critic 2, its workspace; tickets: [0 ... DG_NTICK) view 1's, [DG_NTICK] k_td3_adam_finish's
    float *slot_ptr(int slot) { const DdpgNet &n = dev.v[1].q; float *const p[4] = {n.w, n.wt, n.m, n.v}; return p[slot]; }
};

namespace {
int td3_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling[2];
    TRY(raise_dynamic_lds((const void *)k_td3_critic_fwd, "k_td3_critic_fwd", ceiling[0], device, lds));
    return raise_dynamic_lds((const void *)k_td3_actor_fwd, "k_td3_actor_fwd", ceiling[1], device, lds);
}
struct Td3Grid { int tiles, jobs, ablocks; };
Td3Grid td3_grid(const stmpc_ddpg *l) {
    const int t1 = l->h2p / 16, t0 = l->h1p / 16;
    return {l->Bp / AT_TM, t1 * t0 + 2 * t0 + t1 + t0 + t1 + 1, (l->np + 255) / 256};
}
// critic pass and weight gradients of both critics, then (if due, or gate = 0) of the actor against critic 1 as it then is
void td3_launch_critic_grads(stmpc_td3 *t, int gate, hipStream_t st) {
    const stmpc_ddpg *l = t->base;
    const Td3Grid g = td3_grid(l);
    hipLaunchKernelGGL(k_td3_critic_fwd, dim3(g.tiles, 2), dim3(AT_THREADS), l->lds, st, t->dev, l->cfg.batch, gate, (float *)nullptr);
    hipLaunchKernelGGL(k_td3_wgrad, dim3(g.jobs, 2), dim3(64 * DG_WG_WAVES), 0, st, t->dev, 1, l->Bp, gate);
}
void td3_launch_actor_grads(stmpc_td3 *t, int gate, hipStream_t st) {
    const stmpc_ddpg *l = t->base;
    const Td3Grid g = td3_grid(l);
    hipLaunchKernelGGL(k_td3_actor_fwd, dim3(g.tiles), dim3(AT_THREADS), l->lds, st, t->dev, l->cfg.batch, gate);
    hipLaunchKernelGGL(k_td3_wgrad, dim3(g.jobs, 1), dim3(64 * DG_WG_WAVES), 0, st, t->dev, 0, l->Bp, gate);
}
}  // namespace

extern "C" {

int stmpc_td3_create(stmpc_ctx *c, const stmpc_td3_cfg *g, stmpc_td3 **out) {
    if (!c || !g || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (g->policy_delay < 1) return fail(STMPC_EINVAL, "policy_delay must be at least 1");
    if (!(g->target_noise_std >= 0) || !std::isfinite(g->target_noise_std) || !(g->noise_clip >= 0) || !std::isfinite(g->noise_clip))
        return fail(STMPC_EINVAL, "target_noise_std and noise_clip must be finite and not negative");
    stmpc_td3 *t = new stmpc_td3();
    t->cfg = *g;
    int rc = stmpc_ddpg_create(c, &g->base, &t->base);
    if (rc) { delete t; return rc; }
    stmpc_ddpg *l = t->base;
    l->td3_base = true;
    l->td3_owner = t;
    DdpgDev v1 = l->dev;
    DdpgNet &n = v1.q;
    const size_t np = (size_t)l->np, h1p = (size_t)l->h1p, h2p = (size_t)l->h2p, Bp = (size_t)l->Bp;
    float **ptr[11] = {&n.w, &n.wt, &n.m, &n.v, &n.g, &n.p0, &n.p1, &n.p1t, &n.t0, &n.t1, &n.bpow};
    const size_t len[11] = {np, np, np, np, np, h1p * AT_KIN, h2p * h1p, h2p * h1p, h1p * AT_KIN, h2p * h1p, 4};
    for (int i = 0; i < 11 && !rc; ++i) { rc = ddpg_zero(t->net2[i], len[i] * sizeof(float)); *ptr[i] = t->net2[i].as<float>(); }
    const size_t wlen[7] = {Bp * AT_KIN, Bp * h1p, Bp * h2p, Bp * h2p, Bp * h1p, Bp, Bp * 2};
    float **wptr[7] = {&v1.aX, &v1.aH1, &v1.aH2, &v1.aD2, &v1.aD1, &v1.adz, &v1.arow};
    for (int i = 0; i < 7 && !rc; ++i) { rc = ddpg_zero(t->ws2[i], wlen[i] * sizeof(float)); *wptr[i] = t->ws2[i].as<float>(); }
    if (!rc) rc = ddpg_zero(t->tick, (DG_NTICK + 1) * sizeof(unsigned int));
    if (!rc) rc = td3_raise_lds(l->device, l->lds);
    const float one[4] = {1.f, 1.f, 0.f, 0.f};                       // beta^0
    if (!rc && hipMemcpy(n.bpow, one, sizeof one, hipMemcpyHostToDevice) != hipSuccess) rc = fail(STMPC_EHIP, "hipMemcpy of critic 2's beta powers failed");
    if (rc) { stmpc_td3_destroy(t); return rc; }
    v1.tick = t->tick.as<unsigned int>();
    t->dev.v[0] = l->dev; t->dev.v[1] = v1;
    t->dev.tick = v1.tick + DG_NTICK;
    t->dev.sigma = (float)g->target_noise_std; t->dev.clip = (float)g->noise_clip; t->dev.delay = g->policy_delay;
    *out = t;
    return STMPC_OK;
}

void stmpc_td3_destroy(stmpc_td3 *t) {
    if (!t) return;
    stmpc_ddpg_destroy(t->base);            // (sets the device)
    delete t;
}

stmpc_ddpg *stmpc_td3_base(stmpc_td3 *t) {
    if (!t) { (void)fail(STMPC_EINVAL, "learner is NULL"); return nullptr; }
    return t->base;
}

int stmpc_td3_set_params(stmpc_td3 *t, int slot, const float *values, int64_t count) {
    if (!t || !values || slot < 0 || slot > 3) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    stmpc_ddpg *l = t->base;
    if (count != l->slot_len(1)) return fail(STMPC_EINVAL, "count is not the length of this slot");
    HIPCHK(hipSetDevice(l->device));
    std::vector<float> pad((size_t)l->np, 0.f);
    ddpg_pad(l, l->n_in(1), values, pad, true, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(t->slot_ptr(slot), pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
    if (slot < 2) {                                                  // the packed copies follow the parameters
        hipLaunchKernelGGL(k_ddpg_adam, dim3((l->np + 255) / 256), dim3(256), 0, (hipStream_t)0, t->dev.v[1], 1, 0.f, 1, 0, 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    }
    return STMPC_OK;
}

int stmpc_td3_get_params(stmpc_td3 *t, int slot, float *values, int64_t count) {
    if (!t || !values || slot < 0 || slot > 3) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    stmpc_ddpg *l = t->base;
    if (count != l->slot_len(1)) return fail(STMPC_EINVAL, "count is not the length of this slot");
    HIPCHK(hipSetDevice(l->device));
    std::vector<float> pad((size_t)l->np, 0.f);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pad.data(), t->slot_ptr(slot), pad.size() * sizeof(float), hipMemcpyDeviceToHost));
    ddpg_pad(l, l->n_in(1), nullptr, pad, false, values);
    return STMPC_OK;
}

int stmpc_td3_set_state(stmpc_td3 *t, const float *beta_pow2) {
    if (!t || !beta_pow2) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(t->dev.v[1].q.bpow, beta_pow2, 2 * sizeof(float), hipMemcpyHostToDevice));
    return STMPC_OK;
}

int stmpc_td3_get_state(stmpc_td3 *t, float *beta_pow2) {
    if (!t || !beta_pow2) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(beta_pow2, t->dev.v[1].q.bpow, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

int stmpc_td3_update_device(stmpc_td3 *t, int n_updates, double lr_q, double lr_pi, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (n_updates < 0 || !(lr_q >= 0) || !(lr_pi >= 0)) return fail(STMPC_EINVAL, "n_updates or a learning rate is negative");
    HIPCHK(hipSetDevice(t->base->device));
    const Td3Grid g = td3_grid(t->base);
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // the same six launches whatever the counters say
        per_launch_sample(t->base, 1, st);
        td3_launch_critic_grads(t, 1, st);
        per_launch_update(t->base, st);
        hipLaunchKernelGGL(k_td3_adam_critics, dim3(g.ablocks, 2), dim3(256), 0, st, t->dev, (float)lr_q, 1);
        td3_launch_actor_grads(t, 1, st);
        hipLaunchKernelGGL(k_td3_adam_finish, dim3(g.ablocks, 3), dim3(256), 0, st, t->dev, (float)lr_pi, 1);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_td3_grads_device(stmpc_td3 *t, float *d_grad_actor, float *d_grad_critic1, float *d_grad_critic2, void *stream) {
    if (!t || !d_grad_actor || !d_grad_critic1 || !d_grad_critic2) return fail(STMPC_EINVAL, "NULL argument");
    stmpc_ddpg *l = t->base;
    HIPCHK(hipSetDevice(l->device));
    hipStream_t st = (hipStream_t)stream;
    per_launch_sample(l, 0, st);
    td3_launch_critic_grads(t, 0, st);
    hipLaunchKernelGGL(k_ddpg_unpad, dim3(128), dim3(256), 0, st, l->dev, l->n_in(1), (const float *)t->dev.v[0].q.g, d_grad_critic1);
    hipLaunchKernelGGL(k_ddpg_unpad, dim3(128), dim3(256), 0, st, l->dev, l->n_in(1), (const float *)t->dev.v[1].q.g, d_grad_critic2);
    td3_launch_actor_grads(t, 0, st);
    hipLaunchKernelGGL(k_ddpg_unpad, dim3(128), dim3(256), 0, st, l->dev, l->n_in(0), (const float *)l->dev.pi.g, d_grad_actor);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_td3_targets_device(stmpc_td3 *t, float *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    const stmpc_ddpg *l = t->base;
    HIPCHK(hipSetDevice(l->device));
    per_launch_sample(l, 0, (hipStream_t)stream);
    hipLaunchKernelGGL(k_td3_critic_fwd, dim3(l->Bp / AT_TM, 1), dim3(AT_THREADS), l->lds, (hipStream_t)stream, t->dev, l->cfg.batch, 0, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_td3_stats_device(stmpc_td3 *t, double *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base->device));
    hipLaunchKernelGGL(k_td3_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, t->dev, t->base->cfg.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

double stmpc_td3_noise(uint64_t seed, uint64_t update, uint32_t row, uint32_t *draw1, uint32_t *draw2) {
    return ddpg_gauss_host(dg_hash(seed ^ TD3_STREAM, update, row), draw1, draw2);
}

}  // extern "C"

// ---- prioritised replay (stmpc_per_*) for a lone DDPG learner or a lone TD3 learner's base; kernels in stmpc_per_kernels.hpp ----------------------
namespace {
int per_check_cfg(const stmpc_per_cfg *g) {
    if (!(g->min_priority > 0) || !(g->max_priority >= g->min_priority) || !std::isfinite(g->max_priority) || !(g->alpha >= 0) || !std::isfinite(g->alpha) ||
        !(g->beta >= 0) || !std::isfinite(g->beta))
        return fail(STMPC_EINVAL, "prioritised replay needs min_priority > 0, max_priority >= min_priority, alpha >= 0 and beta >= 0, all finite");
    return STMPC_OK;
}
// not enabled yet, and the ring empty (synchronises)
int per_check_ring(stmpc_ddpg *l) {
    if (l->per) return fail(STMPC_EINVAL, "prioritised replay is already enabled on this learner");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipDeviceSynchronize());
    long long cn[DG_NCNT];
    HIPCHK(hipMemcpy(cn, l->dev.cnt, sizeof cn, hipMemcpyDeviceToHost));
    if (cn[DG_FILL] != 0 || cn[DG_CURSOR] != 0) return fail(STMPC_EINVAL, "prioritised replay can be enabled on an empty ring only (fill is " + std::to_string(cn[DG_FILL]) + ")");
    return STMPC_OK;
}
// the tree, idx, weights and td buffers of a learner that passed both checks, and the fields of its host structs (a TD3 learner's base: of both views too)
int per_attach(stmpc_ddpg *l, const stmpc_per_cfg *g) {
    long long leaves = 1;
    while (leaves < l->cfg.capacity) leaves <<= 1;
    const size_t Bp = (size_t)l->Bp;
    TRY(ddpg_zero(l->per_tree, (size_t)(2 * leaves - 1) * sizeof(double)));
    TRY(ddpg_zero(l->per_idx, Bp * sizeof(long long)));
    TRY(ddpg_zero(l->per_aw, Bp * sizeof(float)));
    TRY(ddpg_zero(l->per_atd, Bp * sizeof(float)));
    if (l->td3_owner) { TRY(ddpg_zero(l->per_atd2, Bp * sizeof(float))); }
    auto set = [&](DdpgDev &d, DevBuf &atd) {
        d.tree = l->per_tree.as<double>(); d.idx = l->per_idx.as<long long>(); d.aw = l->per_aw.as<float>(); d.atd = atd.as<float>();
        d.per_alpha = g->alpha; d.per_beta = g->beta; d.per_min = g->min_priority; d.per_max = g->max_priority; d.per_L = leaves;
    };
    set(l->dev, l->per_atd);
    if (l->td3_owner) {                                             // both views share the tree, idx and the weights; each critic leaves its own Q - y
        set(l->td3_owner->dev.v[0], l->per_atd);
        set(l->td3_owner->dev.v[1], l->per_atd2);
    }
    l->per = true;
    return STMPC_OK;
}
}  // namespace

extern "C" {

int stmpc_per_enable(stmpc_ddpg *l, const stmpc_per_cfg *g) {
    if (!l || !g) return fail(STMPC_EINVAL, "NULL argument");
    TRY(per_check_cfg(g));
    if (l->pop_member) return fail(STMPC_EINVAL, "this learner is a member of a population: prioritised replay is enabled on the population (stmpc_pop_per_enable_ddpg / _td3)");
    TRY(per_check_ring(l));
    return per_attach(l, g);
}

int stmpc_per_tree_read(stmpc_ddpg *l, int64_t first, int64_t count, double *nodes) {
    if (!l || !nodes) return fail(STMPC_EINVAL, "NULL argument");
    if (!l->per) return fail(STMPC_EINVAL, "prioritised replay is not enabled on this learner");
    if (first < 0 || count < 0 || first + count > 2 * l->dev.per_L - 1) return fail(STMPC_EINVAL, "nodes outside the tree");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipDeviceSynchronize());
    if (count) HIPCHK(hipMemcpy(nodes, l->dev.tree + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

int stmpc_per_last_device(stmpc_ddpg *l, int64_t *d_idx, float *d_td, float *d_weight, void *stream) {
    if (!l || !d_idx || !d_td || !d_weight) return fail(STMPC_EINVAL, "NULL argument");
    if (!l->per) return fail(STMPC_EINVAL, "prioritised replay is not enabled on this learner");
    HIPCHK(hipSetDevice(l->device));
    hipLaunchKernelGGL(k_per_last, dim3((l->cfg.batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, l->dev, (const float *)l->per_atd2.as<float>(), l->cfg.batch,
                       (long long *)d_idx, d_td, d_weight);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int64_t stmpc_per_sample_index(const double *tree, int64_t leaves, int64_t fill, uint64_t seed, uint64_t update, uint32_t row) {
    if (!tree || leaves < 1 || (leaves & (leaves - 1)) || fill < 1 || fill > leaves) return -1;
    return per_sample_index(tree, leaves, fill, seed, update, row);
}

}  // extern "C"

// ---- TD3 population (stmpc_pop_td3_*): P learners of the section above, one launch per kernel; kernels in stmpc_td3_pop_kernels.hpp ---------------
struct stmpc_td3_pop {
    int device = 0;
    std::vector<stmpc_td3 *> members;       // owned; made by stmpc_td3_create, so every single-learner entry works on a borrowed member (and on its base)
    DevBuf table, bases;                    // Td3Dev [P]: the members' structs; DdpgDev [P]: their bases' (v[0]), for k_ddpg_act_pop / k_replay_push_pop
    bool per_called = false, per_any = false;   // stmpc_pop_per_enable_td3 was called; at least one member has a tree
    int P() const { return (int)members.size(); }
    const Td3Dev *dev() const { return table.as<Td3Dev>(); }
    const DdpgDev *base_dev() const { return bases.as<DdpgDev>(); }
};

static_assert(STMPC_TD3_POP_MAX == DG_POP_MAX && STMPC_TD3_POP_MAX == STMPC_DDPG_POP_MAX, "DdpgLr holds one learning rate per possible member");

namespace {
int td3_pop_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling[2];
    TRY(raise_dynamic_lds((const void *)k_td3_critic_fwd_pop, "k_td3_critic_fwd_pop", ceiling[0], device, lds));
    TRY(raise_dynamic_lds((const void *)k_td3_actor_fwd_pop, "k_td3_actor_fwd_pop", ceiling[1], device, lds));
    return ddpg_raise_lds(true, device, lds);                       // (k_ddpg_act_pop)
}
}  // namespace

extern "C" {

int stmpc_pop_td3_create(stmpc_ctx *c, const stmpc_td3_cfg *cfgs, int P, stmpc_td3_pop **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (P < 1 || P > STMPC_TD3_POP_MAX) return fail(STMPC_EINVAL, "a population has 1 ... 64 members, not " + std::to_string(P));
    if (!cfgs) return fail(STMPC_EINVAL, "NULL argument");
    for (int m = 1; m < P; ++m) {
        const stmpc_ddpg_cfg &a = cfgs[m].base, &b = cfgs[0].base;
        if (a.n_obs != b.n_obs || a.h1 != b.h1 || a.h2 != b.h2 || a.batch != b.batch || a.capacity != b.capacity)
            return fail(STMPC_EINVAL, "the members of a population share n_obs, h1, h2, batch and capacity (member " + std::to_string(m) + " differs from member 0)");
    }
    HIPCHK(hipSetDevice(c->device));
    stmpc_td3_pop *p = new stmpc_td3_pop();
    p->device = c->device;
    int rc = STMPC_OK;
    std::vector<Td3Dev> host;
    std::vector<DdpgDev> base;
    for (int m = 0; m < P && !rc; ++m) {
        stmpc_td3 *t = nullptr;
        rc = stmpc_td3_create(c, cfgs + m, &t);
        if (!rc) { t->base->pop_member = true; p->members.push_back(t); host.push_back(t->dev); base.push_back(t->dev.v[0]); }
    }
    if (!rc) rc = p->table.ensure(host.size() * sizeof(Td3Dev));
    if (!rc) rc = p->bases.ensure(base.size() * sizeof(DdpgDev));
    if (!rc && (hipMemcpy(p->table.p, host.data(), host.size() * sizeof(Td3Dev), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(p->bases.p, base.data(), base.size() * sizeof(DdpgDev), hipMemcpyHostToDevice) != hipSuccess))
        rc = fail(STMPC_EHIP, "hipMemcpy of the member tables failed");
    if (!rc) rc = td3_pop_raise_lds(p->device, p->members[0]->base->lds);
    if (rc) { stmpc_pop_td3_destroy(p); return rc; }
    *out = p;
    return STMPC_OK;
}

void stmpc_pop_td3_destroy(stmpc_td3_pop *p) {
    if (!p) return;
    for (stmpc_td3 *t : p->members) stmpc_td3_destroy(t);
    (void)hipSetDevice(p->device);
    delete p;
}

int stmpc_pop_td3_size(const stmpc_td3_pop *p) { return p ? p->P() : 0; }

stmpc_td3 *stmpc_pop_td3_member(stmpc_td3_pop *p, int m) {
    if (!p || m < 0 || m >= p->P()) { (void)fail(STMPC_EINVAL, "population is NULL, or no such member"); return nullptr; }
    return p->members[m];
}

int stmpc_pop_td3_act_device(stmpc_td3_pop *p, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise, double *d_action,
                             uint32_t *d_debug, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return ddpg_pop_act(p->device, p->base_dev(), p->P(), p->members[0]->base, n_per_member, d_obs, obs_stride, d_ticks, noise, d_action, d_debug, stream);
}

int stmpc_pop_td3_push_device(stmpc_td3_pop *p, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                              const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward, const uint8_t *d_terminated,
                              const uint8_t *d_truncated, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return ddpg_pop_push(p->device, p->base_dev(), p->P(), p->members[0]->base, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks, d_action,
                         d_reward, d_terminated, d_truncated, stream);
}

int stmpc_pop_td3_update_device(stmpc_td3_pop *p, int n_updates, const double *lr_q, const double *lr_pi, int n_lr, void *stream) {
    if (!p || !lr_q || !lr_pi) return fail(STMPC_EINVAL, "NULL argument");
    if (n_lr != p->P()) return fail(STMPC_EINVAL, "the learning-rate arrays have " + std::to_string(n_lr) + " entries, the population " + std::to_string(p->P()) + " members");
    if (n_updates < 0) return fail(STMPC_EINVAL, "n_updates is negative");
    DdpgLr lq{}, lp{};
    TRY(ddpg_pop_lrs(p->P(), lr_q, lq));
    TRY(ddpg_pop_lrs(p->P(), lr_pi, lp));
    HIPCHK(hipSetDevice(p->device));
    const stmpc_ddpg *l = p->members[0]->base;
    const Td3Grid g = td3_grid(l);
    const int P = p->P();
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // stmpc_td3_update_device's six launches (eight with prioritised members), each over the members in gridDim.z
        if (p->per_any) hipLaunchKernelGGL(k_per_sample_td3_pop, dim3(1, 1, P), dim3(PER_THREADS), 0, st, p->dev(), l->cfg.batch, l->Bp, 1);
        hipLaunchKernelGGL(k_td3_critic_fwd_pop, dim3(g.tiles, 2, P), dim3(AT_THREADS), l->lds, st, p->dev(), l->cfg.batch, 1);
        hipLaunchKernelGGL(k_td3_wgrad_pop, dim3(g.jobs, 2, P), dim3(64 * DG_WG_WAVES), 0, st, p->dev(), 1, l->Bp, 1);
        if (p->per_any) hipLaunchKernelGGL(k_per_update_td3_pop, dim3(1, 1, P), dim3(PER_THREADS), 0, st, p->dev(), l->cfg.batch, 1);
        hipLaunchKernelGGL(k_td3_adam_critics_pop, dim3(g.ablocks, 2, P), dim3(256), 0, st, p->dev(), lq, 1);
        hipLaunchKernelGGL(k_td3_actor_fwd_pop, dim3(g.tiles, 1, P), dim3(AT_THREADS), l->lds, st, p->dev(), l->cfg.batch, 1);
        hipLaunchKernelGGL(k_td3_wgrad_pop, dim3(g.jobs, 1, P), dim3(64 * DG_WG_WAVES), 0, st, p->dev(), 0, l->Bp, 1);
        hipLaunchKernelGGL(k_td3_adam_finish_pop, dim3(g.ablocks, 3, P), dim3(256), 0, st, p->dev(), lp, 1);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_pop_td3_stats_device(stmpc_td3_pop *p, double *d_out, void *stream) {
    if (!p || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->device));
    hipLaunchKernelGGL(k_td3_stats_pop, dim3(1, 1, p->P()), dim3(64), 0, (hipStream_t)stream, p->dev(), p->members[0]->base->cfg.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

}  // extern "C"

// ---- prioritised replay for the populations (stmpc_pop_per_*): stmpc_per_enable's work per member, then the device tables anew; kernels in
// stmpc_per_pop_kernels.hpp -----------------------------------------------------------------------------------------------------------------------
namespace {
// the checks both entries share (bases[m]: member m's stmpc_ddpg): stmpc_per_enable's, on every enabled member, before anything is attached
int pop_per_check(const std::vector<stmpc_ddpg *> &bases, bool called, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) {
    if (!cfgs || !enabled) return fail(STMPC_EINVAL, "NULL argument");
    if (P != (int)bases.size()) return fail(STMPC_EINVAL, "cfgs and enabled have " + std::to_string(P) + " entries, the population " + std::to_string(bases.size()) + " members");
    if (called) return fail(STMPC_EINVAL, "prioritised replay was already set up on this population (one call, on empty rings)");
    for (int m = 0; m < P; ++m)
        if (enabled[m]) { TRY(per_check_cfg(cfgs + m)); TRY(per_check_ring(bases[m])); }
    return STMPC_OK;
}
// per_attach on every enabled member; an allocation that fails leaves the members before it prioritised, which the tables then say too
int pop_per_attach(const std::vector<stmpc_ddpg *> &bases, const stmpc_per_cfg *cfgs, const uint8_t *enabled, bool &any) {
    int rc = STMPC_OK;
    for (size_t m = 0; m < bases.size() && !rc; ++m)
        if (enabled[m]) { rc = per_attach(bases[m], cfgs + m); any = any || !rc; }
    return rc;
}
}  // namespace

extern "C" {

int stmpc_pop_per_enable_ddpg(stmpc_ddpg_pop *p, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    TRY(pop_per_check(p->members, p->per_called, cfgs, enabled, P));
    p->per_called = true;
    const int rc = pop_per_attach(p->members, cfgs, enabled, p->per_any);
    if (!p->per_any) return rc;                                     // (no member enabled: the table stands)
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<DdpgDev> host;
    for (const stmpc_ddpg *l : p->members) host.push_back(l->dev);
    HIPCHK(hipMemcpy(p->table.p, host.data(), host.size() * sizeof(DdpgDev), hipMemcpyHostToDevice));
    return rc;
}

int stmpc_pop_per_enable_td3(stmpc_td3_pop *p, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    std::vector<stmpc_ddpg *> bases_of;
    for (const stmpc_td3 *t : p->members) bases_of.push_back(t->base);
    TRY(pop_per_check(bases_of, p->per_called, cfgs, enabled, P));
    p->per_called = true;
    const int rc = pop_per_attach(bases_of, cfgs, enabled, p->per_any);
    if (!p->per_any) return rc;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<Td3Dev> host;
    std::vector<DdpgDev> base;
    for (const stmpc_td3 *t : p->members) { host.push_back(t->dev); base.push_back(t->dev.v[0]); }
    HIPCHK(hipMemcpy(p->table.p, host.data(), host.size() * sizeof(Td3Dev), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->bases.p, base.data(), base.size() * sizeof(DdpgDev), hipMemcpyHostToDevice));
    return rc;
}

}  // extern "C"

// ---- actors from learners, and a population of actors (stmpc_actor_view_ddpg, stmpc_actor_pop_*); kernel in stmpc_actor_pop_kernels.hpp -----------
struct stmpc_actor_pop {
    int device = 0;
    DevBuf table;                           // ActorDev [P]: the members' structs (a view's pointers are fixed for its learner's lifetime)
    int P = 0, n_in = 0;
    size_t lds = 0;
    const ActorDev *dev() const { return table.as<ActorDev>(); }
};

extern "C" {

int stmpc_actor_view_ddpg(stmpc_ddpg *l, int target, stmpc_actor **out) {
    if (!l || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (target != 0 && target != 1) return fail(STMPC_EINVAL, "target must be 0 (online actor) or 1 (target actor)");
    // k_ddpg_adam keeps both actors packed in actor_layer's lane order; biases and the last layer are read in place in the padded parameter array
    const DdpgNet &pi = l->dev.pi;
    const float *w = target ? pi.wt : pi.w;
    HIPCHK(hipSetDevice(l->device));
    stmpc_actor *a = new stmpc_actor();     // owns no buffer: destroying it frees nothing of the learner's
    a->device = l->device; a->lds = actor_lds_bytes(l->h1p, l->h2p);
    a->dev.p0 = target ? pi.t0 : pi.p0; a->dev.b0 = w + dg_o_b0(l->h1p);
    a->dev.p1 = target ? pi.t1 : pi.p1; a->dev.b1 = w + dg_o_b1(l->h1p, l->h2p);
    a->dev.w2 = w + dg_o_w2(l->h1p, l->h2p); a->dev.b2p = w + dg_o_b2(l->h1p, l->h2p);
    a->dev.scale = l->dev.scale; a->dev.mean = l->dev.mean; a->dev.n_in = pi.n_in; a->dev.h1p = l->h1p; a->dev.h2p = l->h2p;
    const int rc = actor_raise_lds(0, l->device, a->lds);
    if (rc) { stmpc_actor_destroy(a); return rc; }
    *out = a;
    return STMPC_OK;
}

int stmpc_actor_pop_create(stmpc_ctx *c, const stmpc_actor *const *actors, int P, stmpc_actor_pop **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (P < 1 || P > STMPC_DDPG_POP_MAX) return fail(STMPC_EINVAL, "a population has 1 ... 64 members, not " + std::to_string(P));
    if (!actors) return fail(STMPC_EINVAL, "NULL argument");
    std::vector<ActorDev> host;
    for (int m = 0; m < P; ++m) {
        const stmpc_actor *a = actors[m];
        if (!a) return fail(STMPC_EINVAL, "member " + std::to_string(m) + " is NULL");
        if (a->device != c->device) return fail(STMPC_EINVAL, "member " + std::to_string(m) + " and the context are on different devices");
        if (a->dev.n_in != actors[0]->dev.n_in || a->dev.h1p != actors[0]->dev.h1p || a->dev.h2p != actors[0]->dev.h2p)
            return fail(STMPC_EINVAL, "the members of a population share n_in and the padded hidden widths (member " + std::to_string(m) + " differs from member 0)");
        host.push_back(a->dev);
    }
    HIPCHK(hipSetDevice(c->device));
    stmpc_actor_pop *p = new stmpc_actor_pop();
    p->device = c->device; p->P = P; p->n_in = host[0].n_in; p->lds = actors[0]->lds;
    int rc = p->table.ensure(host.size() * sizeof(ActorDev));
    if (!rc && hipMemcpy(p->table.p, host.data(), host.size() * sizeof(ActorDev), hipMemcpyHostToDevice) != hipSuccess) rc = fail(STMPC_EHIP, "hipMemcpy of the member table failed");
    if (!rc) rc = actor_raise_lds(1, c->device, p->lds);
    if (rc) { stmpc_actor_pop_destroy(p); return rc; }
    *out = p;
    return STMPC_OK;
}

void stmpc_actor_pop_destroy(stmpc_actor_pop *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

int stmpc_actor_pop_size(const stmpc_actor_pop *p) { return p ? p->P : 0; }

int stmpc_actor_pop_eval_device(stmpc_ctx *c, const stmpc_actor_pop *p, const stmpc_policy_features_cfg *f, int n_per_member, int Kmax, int step,
                                const double *d_cur_ego4, const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa,
                                int32_t *d_evals, float *d_feat, int feat_stride, double *d_jerk, void *stream) {
    if (!c || !p || !f) return fail(STMPC_EINVAL, "NULL argument");
    if (n_per_member < 0 || (long long)n_per_member * p->P > 0x7fffffffLL) return fail(STMPC_EINVAL, "n_per_member out of range");
    const int N = n_per_member * p->P;
    FeatCfg fc;
    TRY(actor_eval_checks(c, p->device, p->n_in, f, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_evals, d_feat, feat_stride, d_jerk, &fc));
    if (N == 0) return STMPC_OK;
    const int *live;
    TRY(rollout_live(c, N, step, &live));
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_actor_eval_pop, dim3((n_per_member + AT_TM - 1) / AT_TM, p->P), dim3(AT_THREADS), p->lds, (hipStream_t)stream, fc, p->dev(), n_per_member, Kmax,
                       d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, live, d_evals, d_feat, feat_stride, d_jerk);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

}  // extern "C"

// ---- DQN learner (stmpc_dqn_*): the discrete agent on the DDPG learner's ring, counters and tree; kernels in stmpc_dqn_kernels.hpp -----------------
#include "stmpc_dqn_kernels.hpp"

struct stmpc_dqn {
    stmpc_ddpg base;                        // NOT made by stmpc_ddpg_create and never handed out: its buffers, its dev (ring, counters, tickets, workspace, base.dev.q = the
                                            // Q-network, h2p = Ap) and the fields the per_ helpers above read (device, cfg.batch, cfg.capacity, Bp, per ...)
    stmpc_dqn_cfg cfg{};
    DqnDev dev{};                           // dev.base is a copy of base.dev: made anew after stmpc_dqn_per_enable
    int Ap = 0, tiles = 0, jobs = 0, ablocks = 0;
    int64_t slot_len() const { return (int64_t)cfg.h1 * cfg.n_obs + cfg.h1 + (int64_t)cfg.n_actions * cfg.h1 + cfg.n_actions; }
};

namespace {
int dqn_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling[2];
    TRY(raise_dynamic_lds((const void *)k_dqn_fwd, "k_dqn_fwd", ceiling[0], device, lds));
    return raise_dynamic_lds((const void *)k_dqn_act, "k_dqn_act", ceiling[1], device, lds);
}
float *dqn_slot_ptr(stmpc_dqn *t, int slot) {
    const DdpgNet &n = t->dev.base.q;
    float *const p[4] = {n.w, n.wt, n.m, n.v};
    return p[slot];
}
// slot layout (unpadded) <-> padded layout, on the host
void dqn_pad(const stmpc_dqn *t, const float *flat, std::vector<float> &pad, bool to_pad, float *flat_out) {
    const int h1 = t->cfg.h1, A = t->cfg.n_actions, n_obs = t->cfg.n_obs, h1p = t->base.h1p, Ap = t->Ap;
    size_t i = 0;
    auto item = [&](size_t p) { if (to_pad) pad[p] = flat[i]; else flat_out[i] = pad[p]; ++i; };
    for (int n = 0; n < h1; ++n) for (int k = 0; k < n_obs; ++k) item((size_t)n * AT_KIN + k);
    for (int n = 0; n < h1; ++n) item((size_t)dg_o_b0(h1p) + n);
    for (int n = 0; n < A; ++n) for (int k = 0; k < h1; ++k) item((size_t)dg_o_w1(h1p) + (size_t)n * h1p + k);
    for (int n = 0; n < A; ++n) item((size_t)dg_o_b1(h1p, Ap) + n);
}
// the pass and the weight gradients; dbg: stmpc_dqn_targets_device's output
void dqn_launch_grads(stmpc_dqn *t, int gate, float *dbg, hipStream_t st) {
    hipLaunchKernelGGL(k_dqn_fwd, dim3(t->tiles), dim3(AT_THREADS), t->base.lds, st, t->dev, t->cfg.batch, gate, dbg);
    hipLaunchKernelGGL(k_dqn_wgrad, dim3(t->jobs), dim3(64 * DG_WG_WAVES), 0, st, t->dev, t->base.Bp, gate);
}
}  // namespace

extern "C" {

int stmpc_dqn_create(stmpc_ctx *c, const stmpc_dqn_cfg *g, stmpc_dqn **out) {
    if (!c || !g || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (g->n_actions < 1 || g->n_actions > STMPC_ENV_MAX_ACTIONS) return fail(STMPC_EINVAL, "n_actions must be in 1 ... " + std::to_string(STMPC_ENV_MAX_ACTIONS));
    if (g->n_obs < 1 || g->n_obs > AT_KIN - 1 || g->h1 < 1 || g->h1 > 1024) return fail(STMPC_EINVAL, "DQN network shape out of range (n_obs <= 31, hidden width <= 1024)");
    if (g->batch < 1 || g->batch > PER_MAX_B) return fail(STMPC_EINVAL, "batch must be in 1 ... 8192");
    if (g->target_period < 1) return fail(STMPC_EINVAL, "target_period must be at least 1");
    if (g->capacity < 1 || g->replay_start < 0 || g->replay_start >= g->capacity) return fail(STMPC_EINVAL, "capacity must be positive and replay_start below it");
    if (!(g->gamma >= 0) || !std::isfinite(g->gamma) || !(g->beta1 >= 0 && g->beta1 < 1) || !(g->beta2 >= 0 && g->beta2 < 1) || !(g->eps > 0) ||
        (g->clip_targets && !(g->clip_min <= g->clip_max))) return fail(STMPC_EINVAL, "DQN constants out of range");
    HIPCHK(hipSetDevice(c->device));
    stmpc_dqn *t = new stmpc_dqn();
    stmpc_ddpg *l = &t->base;
    t->cfg = *g;
    l->device = c->device;
    l->cfg.n_obs = g->n_obs; l->cfg.h1 = g->h1; l->cfg.h2 = g->n_actions; l->cfg.batch = g->batch; l->cfg.capacity = g->capacity;
    l->cfg.replay_start = g->replay_start; l->cfg.seed = g->seed;
    const int h1p = l->h1p = (g->h1 + 15) & ~15, Ap = l->h2p = t->Ap = (g->n_actions + 15) & ~15;
    const int np = l->np = dg_nparam(h1p, Ap), Bp = l->Bp = (g->batch + 15) & ~15;
    l->lds = ddpg_tile_bytes(h1p, Ap);
    if (l->lds + 1024 > (size_t)c->lds_per_block) { delete t; return fail(STMPC_EINVAL, "DQN network too wide for one workgroup's LDS"); }
    t->tiles = Bp / AT_TM;
    t->jobs = (Ap / 16) * (h1p / 16) + 2 * (h1p / 16) + Ap / 16 + h1p / 16;      // k_ddpg_wgrad's dW1, dW0, db1, db0
    t->ablocks = (dq_nparam(h1p, Ap) + 255) / 256;
    DdpgDev &d = l->dev;
    int rc = 0;
    {
        DdpgNet &n = d.q;
        float **ptr[11] = {&n.w, &n.wt, &n.m, &n.v, &n.g, &n.p0, &n.p1, &n.p1t, &n.t0, &n.t1, &n.bpow};
        const size_t len[11] = {(size_t)np, (size_t)np, (size_t)np, (size_t)np, (size_t)np, (size_t)h1p * AT_KIN, (size_t)Ap * h1p, (size_t)Ap * h1p,
                                (size_t)h1p * AT_KIN, (size_t)Ap * h1p, 4};
        for (int i = 0; i < 11 && !rc; ++i) { rc = ddpg_zero(l->netbuf[1][i], len[i] * sizeof(float)); *ptr[i] = l->netbuf[1][i].as<float>(); }
        n.n_in = g->n_obs;
    }
    const size_t wlen[7] = {(size_t)Bp * AT_KIN, (size_t)Bp * h1p, (size_t)Bp * Ap, (size_t)Bp * Ap, (size_t)Bp * h1p, (size_t)Bp, (size_t)Bp * 2};
    float **wptr[7] = {&d.aX, &d.aH1, &d.aH2, &d.aD2, &d.aD1, &d.adz, &d.arow};
    for (int i = 0; i < 7 && !rc; ++i) { rc = ddpg_zero(l->ws[i], wlen[i] * sizeof(float)); *wptr[i] = l->ws[i].as<float>(); }
    if (!rc) rc = ddpg_zero(l->ring, (size_t)g->capacity * DG_ROW * sizeof(float));
    if (!rc) rc = ddpg_zero(l->cnt, DG_NCNT * sizeof(long long));
    if (!rc) rc = ddpg_zero(l->tick, DG_NTICK * sizeof(unsigned int));
    if (!rc) rc = dqn_raise_lds(l->device, l->lds);
    if (rc) { stmpc_dqn_destroy(t); return rc; }
    d.ring = l->ring.as<float>(); d.cnt = l->cnt.as<long long>(); d.tick = l->tick.as<unsigned int>();
    d.n_obs = g->n_obs; d.h1 = g->h1; d.h2 = g->n_actions; d.h1p = h1p; d.h2p = Ap; d.capacity = g->capacity; d.replay_start = g->replay_start; d.seed = g->seed;
    d.gamma = (float)g->gamma; d.beta1 = (float)g->beta1; d.beta2 = (float)g->beta2;
    d.omb1 = 1.0f - d.beta1; d.omb2 = 1.0f - d.beta2; d.eps = (float)g->eps;       // (tau, the time feature, the squash and the noise: unused, 0)
    const float one[4] = {1.f, 1.f, 0.f, 0.f};                       // beta^0
    if (hipMemcpy(d.q.bpow, one, sizeof one, hipMemcpyHostToDevice) != hipSuccess) { stmpc_dqn_destroy(t); return fail(STMPC_EHIP, "hipMemcpy of the beta powers failed"); }
    t->dev.base = d;
    t->dev.A = g->n_actions; t->dev.Ap = Ap; t->dev.dbl = g->double_dqn != 0; t->dev.clip = g->clip_targets != 0; t->dev.target_period = g->target_period;
    t->dev.clip_min = (float)g->clip_min; t->dev.clip_max = (float)g->clip_max;
    *out = t;
    return STMPC_OK;
}

void stmpc_dqn_destroy(stmpc_dqn *t) {
    if (!t) return;
    (void)hipSetDevice(t->base.device);
    delete t;
}

int stmpc_dqn_set_params(stmpc_dqn *t, int slot, const float *values, int64_t count) {
    if (!t || !values || slot < 0 || slot > 3) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    if (count != t->slot_len()) return fail(STMPC_EINVAL, "count is not the length of this slot");
    HIPCHK(hipSetDevice(t->base.device));
    std::vector<float> pad((size_t)t->base.np, 0.f);
    dqn_pad(t, values, pad, true, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dqn_slot_ptr(t, slot), pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
    if (slot < 2) {                                                  // the packed copies follow the parameters
        hipLaunchKernelGGL(k_dqn_adam, dim3(t->ablocks), dim3(256), 0, (hipStream_t)0, t->dev, 0.f, 1, 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    }
    return STMPC_OK;
}

int stmpc_dqn_get_params(stmpc_dqn *t, int slot, float *values, int64_t count) {
    if (!t || !values || slot < 0 || slot > 3) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    if (count != t->slot_len()) return fail(STMPC_EINVAL, "count is not the length of this slot");
    HIPCHK(hipSetDevice(t->base.device));
    std::vector<float> pad((size_t)t->base.np, 0.f);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pad.data(), dqn_slot_ptr(t, slot), pad.size() * sizeof(float), hipMemcpyDeviceToHost));
    dqn_pad(t, nullptr, pad, false, values);
    return STMPC_OK;
}

int stmpc_dqn_set_state(stmpc_dqn *t, const int64_t *counters, const float *beta_pow) {
    if (!t || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    const stmpc_ddpg *l = &t->base;
    if (counters[DG_CURSOR] < 0 || counters[DG_CURSOR] >= l->cfg.capacity || counters[DG_FILL] < 0 || counters[DG_FILL] > l->cfg.capacity || counters[DG_UPDATES] < 0 ||
        counters[DG_ACTS] < 0 || counters[DG_FRAMES] < 0) return fail(STMPC_EINVAL, "counters out of range");
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipDeviceSynchronize());
    long long cn[DG_NCNT];
    if (l->per) {                                                    // the tree's leaves follow the ring's cursor and fill
        HIPCHK(hipMemcpy(cn, l->dev.cnt, sizeof cn, hipMemcpyDeviceToHost));
        if (cn[DG_CURSOR] != counters[DG_CURSOR] || cn[DG_FILL] != counters[DG_FILL])
            return fail(STMPC_EINVAL, "prioritised replay is enabled: the ring's cursor and fill cannot be set (the priorities belong to the rows pushed)");
    }
    for (int i = 0; i < DG_NCNT; ++i) cn[i] = i <= DG_FRAMES ? counters[i] : 0;
    HIPCHK(hipMemcpy(l->dev.cnt, cn, sizeof cn, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(l->dev.q.bpow, beta_pow, 2 * sizeof(float), hipMemcpyHostToDevice));
    return STMPC_OK;
}

int stmpc_dqn_get_state(stmpc_dqn *t, int64_t *counters, float *beta_pow) {
    if (!t || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    const stmpc_ddpg *l = &t->base;
    HIPCHK(hipSetDevice(l->device));
    HIPCHK(hipDeviceSynchronize());
    long long cn[DG_NCNT];
    HIPCHK(hipMemcpy(cn, l->dev.cnt, sizeof cn, hipMemcpyDeviceToHost));
    for (int i = 0; i < DG_NCNT; ++i) counters[i] = cn[i];
    HIPCHK(hipMemcpy(beta_pow, l->dev.q.bpow, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

int stmpc_dqn_push_device(stmpc_dqn *t, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_action,
                          const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (N < 0 || N > t->cfg.capacity || obs_stride < t->cfg.n_obs) return fail(STMPC_EINVAL, "N exceeds the replay capacity, or obs_stride is shorter than the observation");
    if (N == 0) return STMPC_OK;
    if (!d_obs || !d_next_obs || !d_action || !d_reward || !d_terminated || !d_truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(t->base.device));
    const long long items = (long long)N * DG_ROW;
    const int blocks = (int)((items + 255) / 256 < 1024 ? (items + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_dqn_push, dim3(blocks), dim3(256), 0, (hipStream_t)stream, t->dev, N, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward,
                       d_terminated, d_truncated);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_dqn_act_device(stmpc_dqn *t, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (N < 0 || obs_stride < t->cfg.n_obs) return fail(STMPC_EINVAL, "N negative, or obs_stride shorter than the observation");
    if (!(eps >= 0 && eps <= 1)) return fail(STMPC_EINVAL, "eps must be in 0 ... 1");
    if (N == 0) return STMPC_OK;
    if (!d_obs || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(t->base.device));
    hipLaunchKernelGGL(k_dqn_act, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), t->base.lds, (hipStream_t)stream, t->dev, N, d_obs, obs_stride, (float)eps,
                       eps > 0 ? 1 : 0, d_action, d_debug_q);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_dqn_update_device(stmpc_dqn *t, int n_updates, double lr, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (n_updates < 0 || !(lr >= 0)) return fail(STMPC_EINVAL, "n_updates or the learning rate is negative");
    HIPCHK(hipSetDevice(t->base.device));
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // three launches, five with prioritised replay, whatever the counters say
        per_launch_sample(&t->base, 1, st);
        dqn_launch_grads(t, 1, nullptr, st);
        per_launch_update(&t->base, st);
        hipLaunchKernelGGL(k_dqn_adam, dim3(t->ablocks), dim3(256), 0, st, t->dev, (float)lr, 0, 1);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_dqn_grads_device(stmpc_dqn *t, float *d_grad, void *stream) {
    if (!t || !d_grad) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base.device));
    hipStream_t st = (hipStream_t)stream;
    per_launch_sample(&t->base, 0, st);
    dqn_launch_grads(t, 0, nullptr, st);
    hipLaunchKernelGGL(k_dqn_unpad, dim3(128), dim3(256), 0, st, t->dev, (const float *)t->dev.base.q.g, d_grad);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_dqn_targets_device(stmpc_dqn *t, float *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base.device));
    per_launch_sample(&t->base, 0, (hipStream_t)stream);
    hipLaunchKernelGGL(k_dqn_fwd, dim3(t->tiles), dim3(AT_THREADS), t->base.lds, (hipStream_t)stream, t->dev, t->cfg.batch, 0, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_dqn_gather_device(stmpc_dqn *t, float *d_rows, void *stream) {
    if (!t || !d_rows) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base.device));
    per_launch_sample(&t->base, 0, (hipStream_t)stream);
    hipLaunchKernelGGL(k_replay_gather, dim3((t->cfg.batch * DG_ROW + 255) / 256), dim3(256), 0, (hipStream_t)stream, t->dev.base, t->cfg.batch, d_rows);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_dqn_stats_device(stmpc_dqn *t, double *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base.device));
    hipLaunchKernelGGL(k_dqn_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, t->dev, t->cfg.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_dqn_per_enable(stmpc_dqn *t, const stmpc_per_cfg *g) {
    if (!t || !g) return fail(STMPC_EINVAL, "NULL argument");
    TRY(per_check_cfg(g));
    TRY(per_check_ring(&t->base));
    TRY(per_attach(&t->base, g));
    t->dev.base = t->base.dev;                                       // (the tree, idx, aw, atd and the constants)
    return STMPC_OK;
}

int stmpc_dqn_per_tree_read(stmpc_dqn *t, int64_t first, int64_t count, double *nodes) {
    if (!t) return fail(STMPC_EINVAL, "NULL argument");
    return stmpc_per_tree_read(&t->base, first, count, nodes);
}

int stmpc_dqn_per_last_device(stmpc_dqn *t, int64_t *d_idx, float *d_td, float *d_weight, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "NULL argument");
    return stmpc_per_last_device(&t->base, d_idx, d_td, d_weight, stream);
}

int stmpc_dqn_padded_read(stmpc_dqn *t, int slot, float *values, int64_t count) {
    if (!t || !values || slot < 0 || slot > STMPC_DQN_GRAD) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    if (count != dq_nparam(t->base.h1p, t->Ap)) return fail(STMPC_EINVAL, "count is not the length of a padded slot");
    HIPCHK(hipSetDevice(t->base.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(values, slot == STMPC_DQN_GRAD ? t->dev.base.q.g : dqn_slot_ptr(t, slot), (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

}  // extern "C"
