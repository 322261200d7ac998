// stmpc_learner.hip -- the learners' host code.  What they are made of comes first: a replay store (struct Replay: ring, counters, tickets, sum tree),
// a network's and a workspace's buffers (net_build, ws_build), the slot layout as a list of segments (slot_layout, slot_set, slot_get) and the launch
// geometry (struct Grid).  Then the handles, each with ONE function that derives its device structs from what it owns: the DDPG learner (stmpc_ddpg_*,
// ddpg_refresh), the TD3 learner on a DDPG learner as base plus critic 2 (stmpc_td3_*, td3_refresh), prioritised replay for the two (stmpc_per_*), their
// populations on one skeleton (struct PopCore over struct PopSlot; stmpc_ddpg_pop_*, stmpc_pop_td3_*, stmpc_pop_per_*; pop_upload, td3_pop_upload), actors that view a
// learner's networks and their population (stmpc_actor_view_ddpg, stmpc_actor_pop_*), and the learners for the discrete envs, DQN and categorical
// (stmpc_dqn_*, stmpc_c51_*): one struct (QLearner) that holds a replay store, one network and one workspace of its own, and one set of entries (q_*)
// for both, with what differs in a Head (DqnHead, C51Head); their populations likewise on the same skeleton (QPop; stmpc_pop_dqn_*, stmpc_pop_c51_*;
// q_pop_upload), and the Q-network as a policy behind it (stmpc_qactor_*), lone and as a population (stmpc_pop_qactor_*).  struct stmpc_actor and the
// actor's checks are stmpc.hip's (stmpc_host.hpp).
#include "stmpc_host.hpp"      // (the context, the shared helpers, the kernel headers the context needs)
#include "stmpc_ddpg_kernels.hpp"
#include "stmpc_per_kernels.hpp"
#include "stmpc_ddpg_pop_kernels.hpp"
#include "stmpc_td3_kernels.hpp"
#include "stmpc_td3_pop_kernels.hpp"
#include "stmpc_per_pop_kernels.hpp"
#include "stmpc_actor_pop_kernels.hpp"
#include "stmpc_dqn_kernels.hpp"
#include "stmpc_dqn_pop_kernels.hpp"
#include "stmpc_c51_kernels.hpp"
#include "stmpc_c51_pop_kernels.hpp"
#include "stmpc_c51_noisy_kernels.hpp"
#include "stmpc_qactor_kernels.hpp"
#include "stmpc_c51actor_kernels.hpp"
#include "stmpc_qactor_pop_kernels.hpp"
#include "stmpc_c51actor_pop_kernels.hpp"
#include <initializer_list>
#include <utility>

// ---- the parts every learner is made of ---------------------------------------------------------------------------------------------------------
namespace {
int ddpg_zero(DevBuf &b, size_t bytes) {
    TRY(b.ensure(bytes));
    HIPCHK(hipMemset(b.p, 0, bytes));
    return STMPC_OK;
}
// device -> host behind everything queued on the device (synchronises)
int read_back(int device, void *host, const void *dev, size_t bytes) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    if (bytes) HIPCHK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return STMPC_OK;
}
int per_check_cfg(const stmpc_per_cfg *g) {
    if (!(g->min_priority > 0) || !(g->max_priority >= g->min_priority) || !std::isfinite(g->max_priority) || !(g->alpha >= 0) || !std::isfinite(g->alpha) ||
        !(g->beta >= 0) || !std::isfinite(g->beta))
        return fail(STMPC_EINVAL, "prioritised replay needs min_priority > 0, max_priority >= min_priority, alpha >= 0 and beta >= 0, all finite");
    return STMPC_OK;
}

// The replay store of one learner: the ring, the counters, the tickets, and -- once attach() ran -- prioritised replay's tree, idx, weights and td.
struct Replay {
    int device = 0, batch = 0, Bp = 0, capacity = 0;
    bool per = false;               // prioritised replay (stmpc_per_enable, stmpc_pop_per_enable_*, stmpc_dqn_per_enable)
    DevBuf ring, cnt, tick, tree, idx, aw, atd, atd2;       // (atd2: critic 2's Q - y, on a TD3 learner's base)
    stmpc_per_cfg pcfg{};
    long long leaves = 0;

    int create(int dev, int B, int cap) {
        device = dev; batch = B; Bp = (B + 15) & ~15; capacity = cap;
        TRY(ddpg_zero(ring, (size_t)cap * DG_ROW * sizeof(float)));
        TRY(ddpg_zero(cnt, DG_NCNT * sizeof(long long)));
        return ddpg_zero(tick, DG_NTICK * sizeof(unsigned int));
    }
    // its pointers and constants into a learner's device struct
    void wire(DdpgDev &d) const {
        d.ring = ring.as<float>(); d.cnt = cnt.as<long long>(); d.tick = tick.as<unsigned int>(); d.capacity = capacity;
        if (!per) return;
        d.tree = tree.as<double>(); d.idx = idx.as<long long>(); d.aw = aw.as<float>(); d.atd = atd.as<float>();
        d.per_alpha = pcfg.alpha; d.per_beta = pcfg.beta; d.per_min = pcfg.min_priority; d.per_max = pcfg.max_priority; d.per_L = leaves;
    }
    int get_counters(int64_t *counters) const {
        long long cn[DG_NCNT];
        TRY(read_back(device, cn, cnt.p, sizeof cn));
        for (int i = 0; i < DG_NCNT; ++i) counters[i] = cn[i];
        return STMPC_OK;
    }
    // (synchronises; the caller's copies of the beta powers follow on the selected device)
    int set_counters(const int64_t *counters) {
        if (counters[DG_CURSOR] < 0 || counters[DG_CURSOR] >= capacity || counters[DG_FILL] < 0 || counters[DG_FILL] > capacity || counters[DG_UPDATES] < 0 ||
            counters[DG_ACTS] < 0 || counters[DG_FRAMES] < 0) return fail(STMPC_EINVAL, "counters out of range");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipDeviceSynchronize());
        long long cn[DG_NCNT];
        if (per) {                                                   // the tree's leaves follow the ring's cursor and fill
            HIPCHK(hipMemcpy(cn, cnt.p, sizeof cn, hipMemcpyDeviceToHost));
            if (cn[DG_CURSOR] != counters[DG_CURSOR] || cn[DG_FILL] != counters[DG_FILL])
                return fail(STMPC_EINVAL, "prioritised replay is enabled: the ring's cursor and fill cannot be set (the priorities belong to the rows pushed)");
        }
        for (int i = 0; i < DG_NCNT; ++i) cn[i] = i <= DG_FRAMES ? counters[i] : 0;
        HIPCHK(hipMemcpy(cnt.p, cn, sizeof cn, hipMemcpyHostToDevice));
        return STMPC_OK;
    }
    int read_rows(int64_t first, int64_t count, float *rows) const {
        if (!rows) return fail(STMPC_EINVAL, "NULL argument");
        if (first < 0 || count < 0 || first + count > capacity) return fail(STMPC_EINVAL, "rows outside the ring");
        return read_back(device, rows, ring.as<float>() + (size_t)first * DG_ROW, (size_t)count * DG_ROW * sizeof(float));
    }
    int read_tree(int64_t first, int64_t count, double *nodes) const {
        if (!nodes) return fail(STMPC_EINVAL, "NULL argument");
        if (!per) return fail(STMPC_EINVAL, "prioritised replay is not enabled on this learner");
        if (first < 0 || count < 0 || first + count > 2 * leaves - 1) return fail(STMPC_EINVAL, "nodes outside the tree");
        return read_back(device, nodes, tree.as<double>() + first, (size_t)count * sizeof(double));
    }
    // prioritised replay's two checks on the store: not enabled yet, and the ring empty (synchronises)
    int check_empty() const {
        if (per) return fail(STMPC_EINVAL, "prioritised replay is already enabled on this learner");
        long long cn[DG_NCNT];
        TRY(read_back(device, cn, cnt.p, sizeof cn));
        if (cn[DG_FILL] != 0 || cn[DG_CURSOR] != 0) return fail(STMPC_EINVAL, "prioritised replay can be enabled on an empty ring only (fill is " + std::to_string(cn[DG_FILL]) + ")");
        return STMPC_OK;
    }
    // the tree, idx, weights and td buffers of a store that passed both checks (second_td: atd2 too); the owner then wires its device structs anew
    int attach(const stmpc_per_cfg *g, bool second_td) {
        long long L = 1;
        while (L < capacity) L <<= 1;
        TRY(ddpg_zero(tree, (size_t)(2 * L - 1) * sizeof(double)));
        TRY(ddpg_zero(idx, (size_t)Bp * sizeof(long long)));
        TRY(ddpg_zero(aw, (size_t)Bp * sizeof(float)));
        TRY(ddpg_zero(atd, (size_t)Bp * sizeof(float)));
        if (second_td) TRY(ddpg_zero(atd2, (size_t)Bp * sizeof(float)));
        pcfg = *g; leaves = L; per = true;
        return STMPC_OK;
    }
};

// multi-step returns: the checks of a stmpc_nstep_cfg against the store it goes onto (an empty ring; synchronises), then the two fields into dev
int nstep_attach(const Replay &rp, DdpgDev &dev, const stmpc_nstep_cfg *g) {
    if (g->n_step < 1 || g->n_step > STMPC_NSTEP_MAX) return fail(STMPC_EINVAL, "n_step must be in 1 ... " + std::to_string(STMPC_NSTEP_MAX));
    if (g->n_step > 1 && (g->rows_per_push < 1 || (long long)g->n_step * g->rows_per_push > rp.capacity))
        return fail(STMPC_EINVAL, "n_step > 1 needs rows_per_push >= 1 and n_step * rows_per_push <= capacity (" + std::to_string(g->n_step) + " * " +
                                      std::to_string(g->rows_per_push) + " against " + std::to_string(rp.capacity) + ")");
    long long cn[DG_NCNT];
    TRY(read_back(rp.device, cn, rp.cnt.p, sizeof cn));
    if (cn[DG_FILL] != 0 || cn[DG_CURSOR] != 0) return fail(STMPC_EINVAL, "n_step can be set on an empty ring only (fill is " + std::to_string(cn[DG_FILL]) + ")");
    dev.n_step = g->n_step; dev.rows_push = g->n_step > 1 ? g->rows_per_push : 0;
    return STMPC_OK;
}
// a push of N rows onto a learner with n_step > 1: the ring's successor rule (stmpc_nstep_kernels.hpp) needs every push to have rows_push rows
int nstep_check_push(const DdpgDev &dev, int N) {
    if (dev.n_step > 1 && N != dev.rows_push)
        return fail(STMPC_EINVAL, "this learner forms " + std::to_string(dev.n_step) + "-step returns from pushes of " + std::to_string(dev.rows_push) + " rows: a push of " +
                                      std::to_string(N) + " rows is refused");
    return STMPC_OK;
}
// the windows of n_idx ring rows of a store (HOST idx, HOST out [n_idx][4]); synchronises
int nstep_window_read(const Replay &rp, const DdpgDev &dev, const int64_t *idx, int n_idx, double *out) {
    if (!idx || !out || n_idx < 0) return fail(STMPC_EINVAL, "NULL argument or n_idx negative");
    long long cn[DG_NCNT];
    TRY(read_back(rp.device, cn, rp.cnt.p, sizeof cn));
    for (int i = 0; i < n_idx; ++i)
        if (idx[i] < 0 || idx[i] >= cn[DG_FILL]) return fail(STMPC_EINVAL, "index " + std::to_string(i) + " is not a filled ring row (fill is " + std::to_string(cn[DG_FILL]) + ")");
    if (n_idx == 0) return STMPC_OK;
    static_assert(sizeof(long long) == sizeof(int64_t), "ring indices travel as int64");
    DevBuf d_idx, d_out;
    TRY(upload(d_idx, (const long long *)idx, (size_t)n_idx));
    TRY(d_out.ensure((size_t)n_idx * 4 * sizeof(double)));
    const int blocks = (n_idx + 7) / 8 < 256 ? (n_idx + 7) / 8 : 256;      // (two rows per wave, four waves per block)
    hipLaunchKernelGGL(k_nstep_window, dim3(blocks), dim3(256), 0, (hipStream_t)0, dev, (const long long *)d_idx.as<long long>(), n_idx, d_out.as<double>());
    HIPCHK(hipGetLastError());
    return read_back(rp.device, out, d_out.p, (size_t)n_idx * 4 * sizeof(double));
}

// prioritised replay: the sampling step in front of a pass that gathers (nothing on a store that samples uniformly); d: the device struct wired to rp
void per_launch_sample(const Replay &rp, const DdpgDev &d, int gate, hipStream_t st) {
    if (rp.per) hipLaunchKernelGGL(k_per_sample, dim3(1), dim3(PER_THREADS), 0, st, d, rp.batch, rp.Bp, gate);
}
// ... and the priority update behind the critic pass
void per_launch_update(const Replay &rp, const DdpgDev &d, hipStream_t st) {
    if (rp.per) hipLaunchKernelGGL(k_per_update, dim3(1), dim3(PER_THREADS), 0, st, d, (const float *)rp.atd2.as<float>(), rp.batch, 1);
}
int per_last(const Replay &rp, const DdpgDev &d, int64_t *d_idx, float *d_td, float *d_weight, void *stream) {
    if (!d_idx || !d_td || !d_weight) return fail(STMPC_EINVAL, "NULL argument");
    if (!rp.per) return fail(STMPC_EINVAL, "prioritised replay is not enabled on this learner");
    HIPCHK(hipSetDevice(rp.device));
    hipLaunchKernelGGL(k_per_last, dim3((rp.batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, (const float *)rp.atd2.as<float>(), rp.batch, (long long *)d_idx,
                       d_td, d_weight);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
int replay_gather(const Replay &rp, const DdpgDev &d, float *d_rows, void *stream) {
    HIPCHK(hipSetDevice(rp.device));
    per_launch_sample(rp, d, 0, (hipStream_t)stream);
    hipLaunchKernelGGL(k_replay_gather, dim3((rp.batch * DG_ROW + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, rp.batch, d_rows);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

// One network's eleven buffers for the padded widths (h1p, h2p): net_wire points a DdpgNet at them, net_build allocates them first and starts Adam's
// beta powers at beta^0.
void net_wire(DdpgNet &n, const DevBuf (&buf)[11], int n_in) {
    float **ptr[11] = {&n.w, &n.wt, &n.m, &n.v, &n.g, &n.p0, &n.p1, &n.p1t, &n.t0, &n.t1, &n.bpow};
    for (int i = 0; i < 11; ++i) *ptr[i] = buf[i].as<float>();
    n.n_in = n_in;
}
int net_build(DevBuf (&buf)[11], DdpgNet &n, int n_in, int h1p, int h2p) {
    const size_t np = (size_t)dg_nparam(h1p, h2p), l0 = (size_t)h1p * AT_KIN, l1 = (size_t)h2p * h1p;
    const size_t len[11] = {np, np, np, np, np, l0, l1, l1, l0, l1, 4};
    for (int i = 0; i < 11; ++i) TRY(ddpg_zero(buf[i], len[i] * sizeof(float)));
    net_wire(n, buf, n_in);
    const float one[4] = {1.f, 1.f, 0.f, 0.f};                       // beta^0
    if (hipMemcpy(n.bpow, one, sizeof one, hipMemcpyHostToDevice) != hipSuccess) return fail(STMPC_EHIP, "hipMemcpy of the beta powers failed");
    return STMPC_OK;
}
// ... and one minibatch's seven workspace buffers
void ws_wire(DdpgDev &d, const DevBuf (&buf)[7]) {
    float **ptr[7] = {&d.aX, &d.aH1, &d.aH2, &d.aD2, &d.aD1, &d.adz, &d.arow};
    for (int i = 0; i < 7; ++i) *ptr[i] = buf[i].as<float>();
}
int ws_build(DevBuf (&buf)[7], DdpgDev &d, int Bp, int h1p, int h2p) {
    const size_t B = (size_t)Bp, len[7] = {B * AT_KIN, B * h1p, B * h2p, B * h2p, B * h1p, B, B * 2};
    for (int i = 0; i < 7; ++i) TRY(ddpg_zero(buf[i], len[i] * sizeof(float)));
    ws_wire(d, buf);
    return STMPC_OK;
}

// The slot layout (unpadded, what the C-ABI hands over) against the padded one as data: rows x cols values, row r at pad[off + r * stride].
struct Seg { int rows, cols; size_t off, stride; };
// W0, b0, W1, b1 and -- with a third layer (the DDPG nets; not the Q-network) -- W2, b2
std::vector<Seg> slot_layout(int n_in, int h1, int h2, int h1p, int h2p, bool third) {
    std::vector<Seg> lay = {{h1, n_in, 0, AT_KIN}, {1, h1, (size_t)dg_o_b0(h1p), 0}, {h2, h1, (size_t)dg_o_w1(h1p), (size_t)h1p}, {1, h2, (size_t)dg_o_b1(h1p, h2p), 0}};
    if (third) { lay.push_back({1, h2, (size_t)dg_o_w2(h1p, h2p), 0}); lay.push_back({1, 1, (size_t)dg_o_b2(h1p, h2p), 0}); }
    return lay;
}
int64_t slot_len(const std::vector<Seg> &lay) {
    int64_t n = 0;
    for (const Seg &s : lay) n += (int64_t)s.rows * s.cols;
    return n;
}
// one slot between the two layouts, on the host, either way
void slot_move(const std::vector<Seg> &lay, float *flat, float *pad, bool to_pad) {
    for (const Seg &s : lay)
        for (int r = 0; r < s.rows; ++r, flat += s.cols) {
            float *p = pad + s.off + (size_t)r * s.stride;
            if (to_pad) memcpy(p, flat, s.cols * sizeof(float)); else memcpy(flat, p, s.cols * sizeof(float));
        }
}
int slot_args(const void *handle, const void *values, int slot, int n_slots) {
    return !handle || !values || slot < 0 || slot >= n_slots ? fail(STMPC_EINVAL, "NULL argument or slot out of range") : STMPC_OK;
}
float *net_slot(const DdpgNet &n, int i) { float *const p[4] = {n.w, n.wt, n.m, n.v}; return p[i]; }
// a *_set_params entry behind slot_args: d_slot is the slot's padded array of np floats; repack() launches the kernel that makes the packed copies
// follow the parameters, which slots 0 and 1 of a net (online, target) have
template <class F> int slot_set(int device, const std::vector<Seg> &lay, size_t np, float *d_slot, const float *values, int64_t count, bool packed, F repack) {
    if (count != slot_len(lay)) return fail(STMPC_EINVAL, "count is not the length of this slot");
    HIPCHK(hipSetDevice(device));
    std::vector<float> pad(np, 0.f);
    slot_move(lay, const_cast<float *>(values), pad.data(), true);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(d_slot, pad.data(), np * sizeof(float), hipMemcpyHostToDevice));
    if (packed) {
        repack();
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    }
    return STMPC_OK;
}
int slot_get(int device, const std::vector<Seg> &lay, size_t np, const float *d_slot, float *values, int64_t count) {
    if (count != slot_len(lay)) return fail(STMPC_EINVAL, "count is not the length of this slot");
    std::vector<float> pad(np, 0.f);
    TRY(read_back(device, pad.data(), d_slot, np * sizeof(float)));
    slot_move(lay, values, pad.data(), false);
    return STMPC_OK;
}

// The launch geometry of a learner: minibatch tiles, weight-gradient jobs (dW1, dW0, db1, db0 and, with a third layer, dW2, db2) and Adam's blocks.
struct Grid { int tiles, jobs, ablocks; };
Grid make_grid(int Bp, int h1p, int h2p, bool third) {
    const int t1 = h2p / 16, t0 = h1p / 16;
    return {Bp / AT_TM, t1 * t0 + 2 * t0 + t1 + t0 + (third ? t1 + 1 : 0), ((third ? dg_nparam(h1p, h2p) : dq_nparam(h1p, h2p)) + 255) / 256};
}
// blocks of a push of `rows` rows (of one member)
int push_blocks(int rows) {
    const long long blocks = ((long long)rows * DG_ROW + 255) / 256;
    return (int)(blocks < 1024 ? blocks : 1024);
}
}  // namespace

// ---- DDPG learner (stmpc_ddpg_*): replay ring, fused update, acting; kernels in stmpc_ddpg_kernels.hpp -------------------------------------------
struct stmpc_ddpg {
    stmpc_ddpg_cfg cfg{};
    DdpgDev dev{};                  // the constants (stmpc_ddpg_create), the nets and the workspace; the replay's part is ddpg_refresh's
    Replay rp;
    DevBuf net[2][11], ws[7];       // actor, critic; workspace
    std::vector<Seg> lay[2];        // the actor's and the critic's slot layout
    int h1p = 0, h2p = 0, np = 0;
    size_t lds = 0;
    Grid grid{};
    bool td3_base = false;          // lent by a stmpc_td3 (stmpc_td3_base): an update or gradients of this handle alone would leave critic 2 behind
    struct stmpc_td3 *td3_owner = nullptr;  // that stmpc_td3: its two views derive from dev (td3_refresh)
    bool pop_member = false;        // owned by a population, whose device table holds a copy of dev
};

namespace {
void td3_refresh(struct stmpc_td3 *t);
// dev's replay part from rp, and what derives from dev
void ddpg_refresh(stmpc_ddpg *l) {
    l->rp.wire(l->dev);
    if (l->td3_owner) td3_refresh(l->td3_owner);
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
void ddpg_launch_grads(stmpc_ddpg *l, int which, int gate, hipStream_t st) {
    if (which) hipLaunchKernelGGL(k_ddpg_critic_fwd, dim3(l->grid.tiles), dim3(AT_THREADS), l->lds, st, l->dev, l->cfg.batch, gate);
    else hipLaunchKernelGGL(k_ddpg_actor_fwd, dim3(l->grid.tiles), dim3(AT_THREADS), l->lds, st, l->dev, l->cfg.batch, gate);
    hipLaunchKernelGGL(k_ddpg_wgrad, dim3(l->grid.jobs), dim3(64 * DG_WG_WAVES), 0, st, l->dev, which, l->rp.Bp, gate);
}
// k_ddpg_adam on net `which` of the device struct d of a learner with l's shape (l->dev, or a TD3 learner's second view)
void ddpg_launch_adam(const stmpc_ddpg *l, const DdpgDev &d, int which, float lr, int mode, int bump, hipStream_t st) {
    hipLaunchKernelGGL(k_ddpg_adam, dim3(l->grid.ablocks), dim3(256), 0, st, d, which, lr, mode, bump, 1);
}
void ddpg_launch_unpad(const stmpc_ddpg *l, int which, const float *d_grad, float *d_out, hipStream_t st) {
    hipLaunchKernelGGL(k_ddpg_unpad, dim3(128), dim3(256), 0, st, l->dev, (which ? l->dev.q : l->dev.pi).n_in, d_grad, d_out);
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
    const int h1p = (g->h1 + 15) & ~15, h2p = (g->h2 + 15) & ~15;
    const size_t lds = ddpg_tile_bytes(h1p, h2p);
    if (lds + 1024 > (size_t)c->lds_per_block) return fail(STMPC_EINVAL, "DDPG networks too wide for one workgroup's LDS");
    stmpc_ddpg *l = new stmpc_ddpg();
    l->cfg = *g; l->h1p = h1p; l->h2p = h2p; l->np = dg_nparam(h1p, h2p); l->lds = lds;
    l->rp.device = c->device;                                        // (what destroy selects, should an allocation fail)
    DdpgDev &d = l->dev;
    int rc = 0;
    for (int w = 0; w < 2 && !rc; ++w) {
        l->lay[w] = slot_layout(g->n_obs + 1 + w, g->h1, g->h2, h1p, h2p, true);
        rc = net_build(l->net[w], w ? d.q : d.pi, g->n_obs + 1 + w, h1p, h2p);
    }
    if (!rc) rc = ws_build(l->ws, d, (g->batch + 15) & ~15, h1p, h2p);
    if (!rc) rc = l->rp.create(c->device, g->batch, g->capacity);     // (the ring behind the nets and the workspace: the order the buffers always had)
    if (!rc) rc = ddpg_raise_lds(false, c->device, lds);
    if (rc) { stmpc_ddpg_destroy(l); return rc; }
    l->grid = make_grid(l->rp.Bp, h1p, h2p, true);
    d.n_obs = g->n_obs; d.h1 = g->h1; d.h2 = g->h2; d.h1p = h1p; d.h2p = h2p; d.replay_start = g->replay_start; d.seed = g->seed;
    d.gamma = (float)g->gamma; d.tau = (float)g->tau; d.beta1 = (float)g->beta1; d.beta2 = (float)g->beta2;
    d.omb1 = 1.0f - d.beta1; d.omb2 = 1.0f - d.beta2; d.omtau = 1.0f - d.tau; d.eps = (float)g->eps; d.time_scale = (float)g->time_scale;
    d.scale = (float)g->tanh_scale; d.mean = (float)g->tanh_mean; d.noise_std = (float)g->noise_std; d.a_low = (float)g->action_low; d.a_high = (float)g->action_high;
    ddpg_refresh(l);
    *out = l;
    return STMPC_OK;
}

void stmpc_ddpg_destroy(stmpc_ddpg *l) {
    if (!l) return;
    (void)hipSetDevice(l->rp.device);
    delete l;
}

int stmpc_ddpg_set_params(stmpc_ddpg *l, int slot, const float *values, int64_t count) {
    TRY(slot_args(l, values, slot, 8));
    const int which = slot >= 4;
    return slot_set(l->rp.device, l->lay[which], l->np, net_slot(which ? l->dev.q : l->dev.pi, slot & 3), values, count, (slot & 3) < 2,
                    [&] { ddpg_launch_adam(l, l->dev, which, 0.f, 1, 0, (hipStream_t)0); });
}

int stmpc_ddpg_get_params(stmpc_ddpg *l, int slot, float *values, int64_t count) {
    TRY(slot_args(l, values, slot, 8));
    const int which = slot >= 4;
    return slot_get(l->rp.device, l->lay[which], l->np, net_slot(which ? l->dev.q : l->dev.pi, slot & 3), values, count);
}

int stmpc_ddpg_set_state(stmpc_ddpg *l, const int64_t *counters, const float *beta_pow) {
    if (!l || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    TRY(l->rp.set_counters(counters));
    HIPCHK(hipMemcpy(l->dev.pi.bpow, beta_pow, 2 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(l->dev.q.bpow, beta_pow + 2, 2 * sizeof(float), hipMemcpyHostToDevice));
    return STMPC_OK;
}

int stmpc_ddpg_get_state(stmpc_ddpg *l, int64_t *counters, float *beta_pow) {
    if (!l || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    TRY(l->rp.get_counters(counters));
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
    TRY(nstep_check_push(l->dev, N));
    if (!d_obs || !d_next_obs || !d_ticks || !d_action || !d_reward || !d_terminated || !d_truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(l->rp.device));
    hipLaunchKernelGGL(k_replay_push, dim3(push_blocks(N)), dim3(256), 0, (hipStream_t)stream, l->dev, N, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks,
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
    HIPCHK(hipSetDevice(l->rp.device));
    hipLaunchKernelGGL(k_ddpg_act, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), l->lds, (hipStream_t)stream, l->dev, N, d_obs, obs_stride, d_ticks, noise != 0,
                       d_action, d_debug);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_update_device(stmpc_ddpg *l, int n_updates, double lr_q, double lr_pi, void *stream) {
    if (!l) return fail(STMPC_EINVAL, "learner is NULL");
    if (l->td3_base) return fail(STMPC_EINVAL, "this learner is the base of a TD3 learner: update it with stmpc_td3_update_device");
    if (n_updates < 0 || !(lr_q >= 0) || !(lr_pi >= 0)) return fail(STMPC_EINVAL, "n_updates or a learning rate is negative");
    HIPCHK(hipSetDevice(l->rp.device));
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {
        per_launch_sample(l->rp, l->dev, 1, st);
        ddpg_launch_grads(l, 1, 1, st);
        per_launch_update(l->rp, l->dev, st);
        ddpg_launch_adam(l, l->dev, 1, (float)lr_q, 0, 0, st);
        ddpg_launch_grads(l, 0, 1, st);
        ddpg_launch_adam(l, l->dev, 0, (float)lr_pi, 0, 1, st);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_grads_device(stmpc_ddpg *l, float *d_grad_actor, float *d_grad_critic, void *stream) {
    if (!l || !d_grad_actor || !d_grad_critic) return fail(STMPC_EINVAL, "NULL argument");
    if (l->td3_base) return fail(STMPC_EINVAL, "this learner is the base of a TD3 learner: take its gradients with stmpc_td3_grads_device");
    HIPCHK(hipSetDevice(l->rp.device));
    hipStream_t st = (hipStream_t)stream;
    per_launch_sample(l->rp, l->dev, 0, st);
    ddpg_launch_grads(l, 1, 0, st);
    ddpg_launch_unpad(l, 1, l->dev.q.g, d_grad_critic, st);
    ddpg_launch_grads(l, 0, 0, st);
    ddpg_launch_unpad(l, 0, l->dev.pi.g, d_grad_actor, st);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_stats_device(stmpc_ddpg *l, double *d_out, void *stream) {
    if (!l || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(l->rp.device));
    hipLaunchKernelGGL(k_ddpg_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, l->dev, l->cfg.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_replay_read(stmpc_ddpg *l, int64_t first, int64_t count, float *rows) {
    if (!l) return fail(STMPC_EINVAL, "NULL argument");
    return l->rp.read_rows(first, count, rows);
}

int stmpc_ddpg_gather_device(stmpc_ddpg *l, float *d_rows, void *stream) {
    if (!l || !d_rows) return fail(STMPC_EINVAL, "NULL argument");
    return replay_gather(l->rp, l->dev, d_rows, stream);
}

uint64_t stmpc_ddpg_sample_index(uint64_t seed, uint64_t update, uint32_t row, uint64_t fill) {
    return fill ? (uint64_t)(dg_hash(seed, update, row) % fill) : 0;
}

double stmpc_ddpg_noise(uint64_t seed, uint64_t call, uint32_t row, uint32_t *draw1, uint32_t *draw2) {
    return ddpg_gauss_host(dg_hash(seed ^ DG_NOISE_STREAM, call, row), draw1, draw2);
}

}  // extern "C"

// ---- TD3 learner (stmpc_td3_*): a DDPG learner as base (actor, critic 1, ring, counters) plus critic 2; kernels in stmpc_td3_kernels.hpp -----------
struct stmpc_td3 {
    stmpc_ddpg *base = nullptr;             // owned; lent out by stmpc_td3_base
    stmpc_td3_cfg cfg{};
    Td3Dev dev{};                           // sigma, clip, delay, tick (stmpc_td3_create); the two views are td3_refresh's
    DevBuf net2[11], ws2[7], tick;          // critic 2, its workspace; tickets: [0 ... DG_NTICK) view 1's, [DG_NTICK] k_td3_adam_finish's
};

namespace {
// the two views from the base's dev and critic 2: both share the ring, the counters, the tree, idx and the weights; view 1 has critic 2 in the critic's
// place, a workspace and tickets of its own, and leaves its own Q - y
void td3_refresh(stmpc_td3 *t) {
    const stmpc_ddpg *l = t->base;
    DdpgDev &v1 = t->dev.v[1];
    t->dev.v[0] = v1 = l->dev;
    net_wire(v1.q, t->net2, l->dev.q.n_in);
    ws_wire(v1, t->ws2);
    v1.tick = t->tick.as<unsigned int>();
    if (l->rp.per) v1.atd = l->rp.atd2.as<float>();
}
int td3_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling[2];
    TRY(raise_dynamic_lds((const void *)k_td3_critic_fwd, "k_td3_critic_fwd", ceiling[0], device, lds));
    return raise_dynamic_lds((const void *)k_td3_actor_fwd, "k_td3_actor_fwd", ceiling[1], device, lds);
}
// critic pass and weight gradients of both critics, then (if due, or gate = 0) of the actor against critic 1 as it then is
void td3_launch_critic_grads(stmpc_td3 *t, int gate, hipStream_t st) {
    const stmpc_ddpg *l = t->base;
    hipLaunchKernelGGL(k_td3_critic_fwd, dim3(l->grid.tiles, 2), dim3(AT_THREADS), l->lds, st, t->dev, l->cfg.batch, gate, (float *)nullptr);
    hipLaunchKernelGGL(k_td3_wgrad, dim3(l->grid.jobs, 2), dim3(64 * DG_WG_WAVES), 0, st, t->dev, 1, l->rp.Bp, gate);
}
void td3_launch_actor_grads(stmpc_td3 *t, int gate, hipStream_t st) {
    const stmpc_ddpg *l = t->base;
    hipLaunchKernelGGL(k_td3_actor_fwd, dim3(l->grid.tiles), dim3(AT_THREADS), l->lds, st, t->dev, l->cfg.batch, gate);
    hipLaunchKernelGGL(k_td3_wgrad, dim3(l->grid.jobs, 1), dim3(64 * DG_WG_WAVES), 0, st, t->dev, 0, l->rp.Bp, gate);
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
    rc = net_build(t->net2, t->dev.v[1].q, l->dev.q.n_in, l->h1p, l->h2p);
    if (!rc) rc = ws_build(t->ws2, t->dev.v[1], l->rp.Bp, l->h1p, l->h2p);
    if (!rc) rc = ddpg_zero(t->tick, (DG_NTICK + 1) * sizeof(unsigned int));
    if (!rc) rc = td3_raise_lds(l->rp.device, l->lds);
    if (rc) { stmpc_td3_destroy(t); return rc; }
    t->dev.tick = t->tick.as<unsigned int>() + DG_NTICK;
    t->dev.sigma = (float)g->target_noise_std; t->dev.clip = (float)g->noise_clip; t->dev.delay = g->policy_delay;
    td3_refresh(t);
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
    TRY(slot_args(t, values, slot, 4));
    const stmpc_ddpg *l = t->base;
    return slot_set(l->rp.device, l->lay[1], l->np, net_slot(t->dev.v[1].q, slot), values, count, slot < 2,
                    [&] { ddpg_launch_adam(l, t->dev.v[1], 1, 0.f, 1, 0, (hipStream_t)0); });
}

int stmpc_td3_get_params(stmpc_td3 *t, int slot, float *values, int64_t count) {
    TRY(slot_args(t, values, slot, 4));
    const stmpc_ddpg *l = t->base;
    return slot_get(l->rp.device, l->lay[1], l->np, net_slot(t->dev.v[1].q, slot), values, count);
}

int stmpc_td3_set_state(stmpc_td3 *t, const float *beta_pow2) {
    if (!t || !beta_pow2) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base->rp.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(t->dev.v[1].q.bpow, beta_pow2, 2 * sizeof(float), hipMemcpyHostToDevice));
    return STMPC_OK;
}

int stmpc_td3_get_state(stmpc_td3 *t, float *beta_pow2) {
    if (!t || !beta_pow2) return fail(STMPC_EINVAL, "NULL argument");
    return read_back(t->base->rp.device, beta_pow2, t->dev.v[1].q.bpow, 2 * sizeof(float));
}

int stmpc_td3_update_device(stmpc_td3 *t, int n_updates, double lr_q, double lr_pi, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (n_updates < 0 || !(lr_q >= 0) || !(lr_pi >= 0)) return fail(STMPC_EINVAL, "n_updates or a learning rate is negative");
    const stmpc_ddpg *l = t->base;
    HIPCHK(hipSetDevice(l->rp.device));
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // the same six launches whatever the counters say
        per_launch_sample(l->rp, l->dev, 1, st);
        td3_launch_critic_grads(t, 1, st);
        per_launch_update(l->rp, l->dev, st);
        hipLaunchKernelGGL(k_td3_adam_critics, dim3(l->grid.ablocks, 2), dim3(256), 0, st, t->dev, (float)lr_q, 1);
        td3_launch_actor_grads(t, 1, st);
        hipLaunchKernelGGL(k_td3_adam_finish, dim3(l->grid.ablocks, 3), dim3(256), 0, st, t->dev, (float)lr_pi, 1);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_td3_grads_device(stmpc_td3 *t, float *d_grad_actor, float *d_grad_critic1, float *d_grad_critic2, void *stream) {
    if (!t || !d_grad_actor || !d_grad_critic1 || !d_grad_critic2) return fail(STMPC_EINVAL, "NULL argument");
    stmpc_ddpg *l = t->base;
    HIPCHK(hipSetDevice(l->rp.device));
    hipStream_t st = (hipStream_t)stream;
    per_launch_sample(l->rp, l->dev, 0, st);
    td3_launch_critic_grads(t, 0, st);
    ddpg_launch_unpad(l, 1, t->dev.v[0].q.g, d_grad_critic1, st);
    ddpg_launch_unpad(l, 1, t->dev.v[1].q.g, d_grad_critic2, st);
    td3_launch_actor_grads(t, 0, st);
    ddpg_launch_unpad(l, 0, l->dev.pi.g, d_grad_actor, st);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_td3_targets_device(stmpc_td3 *t, float *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    const stmpc_ddpg *l = t->base;
    HIPCHK(hipSetDevice(l->rp.device));
    per_launch_sample(l->rp, l->dev, 0, (hipStream_t)stream);
    hipLaunchKernelGGL(k_td3_critic_fwd, dim3(l->grid.tiles, 1), dim3(AT_THREADS), l->lds, (hipStream_t)stream, t->dev, l->cfg.batch, 0, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_td3_stats_device(stmpc_td3 *t, double *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->base->rp.device));
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
// the store's buffers on a learner of any type that passed the checks, and the device struct the store is wired into (a TD3 learner's base: both
// views too) anew
int per_attach(Replay &rp, DdpgDev &dev, stmpc_td3 *td3_owner, const stmpc_per_cfg *g) {
    TRY(rp.attach(g, td3_owner != nullptr));
    rp.wire(dev);
    if (td3_owner) td3_refresh(td3_owner);
    return STMPC_OK;
}
}  // namespace

extern "C" {

int stmpc_per_enable(stmpc_ddpg *l, const stmpc_per_cfg *g) {
    if (!l || !g) return fail(STMPC_EINVAL, "NULL argument");
    TRY(per_check_cfg(g));
    if (l->pop_member) return fail(STMPC_EINVAL, "this learner is a member of a population: prioritised replay is enabled on the population (stmpc_pop_per_enable_ddpg / _td3)");
    TRY(l->rp.check_empty());
    return per_attach(l->rp, l->dev, l->td3_owner, g);
}

int stmpc_nstep_enable_ddpg(stmpc_ddpg *l, const stmpc_nstep_cfg *g) {
    if (!l || !g) return fail(STMPC_EINVAL, "NULL argument");
    if (l->pop_member) return fail(STMPC_EINVAL, "this learner is a member of a population: n_step is set on the population (stmpc_pop_nstep_enable_ddpg / _td3)");
    TRY(nstep_attach(l->rp, l->dev, g));
    ddpg_refresh(l);
    return STMPC_OK;
}

int stmpc_nstep_window_ddpg(stmpc_ddpg *l, const int64_t *idx, int n_idx, double *out) {
    if (!l) return fail(STMPC_EINVAL, "NULL argument");
    return nstep_window_read(l->rp, l->dev, idx, n_idx, out);
}

int stmpc_per_tree_read(stmpc_ddpg *l, int64_t first, int64_t count, double *nodes) {
    if (!l) return fail(STMPC_EINVAL, "NULL argument");
    return l->rp.read_tree(first, count, nodes);
}

int stmpc_per_last_device(stmpc_ddpg *l, int64_t *d_idx, float *d_td, float *d_weight, void *stream) {
    if (!l) return fail(STMPC_EINVAL, "NULL argument");
    return per_last(l->rp, l->dev, d_idx, d_td, d_weight, stream);
}

int64_t stmpc_per_sample_index(const double *tree, int64_t leaves, int64_t fill, uint64_t seed, uint64_t update, uint32_t row) {
    if (!tree || leaves < 1 || (leaves & (leaves - 1)) || fill < 1 || fill > leaves) return -1;
    return per_sample_index(tree, leaves, fill, seed, update, row);
}

}  // extern "C"

// ---- the populations (stmpc_ddpg_pop_*, stmpc_pop_td3_*, stmpc_pop_per_*): P learners of the sections above, one launch per kernel; kernels in
// stmpc_ddpg_pop_kernels.hpp, stmpc_td3_pop_kernels.hpp and stmpc_per_pop_kernels.hpp -------------------------------------------------------------
// What a population's shared code uses of a member, whatever its type: the replay store, the DdpgDev that store is wired into (a DDPG learner's
// dev, a TD3 member's base's, a DQN member's dev.base) and -- a TD3 member's base alone -- the stmpc_td3 whose views derive from it.
struct PopSlot {
    Replay *rp = nullptr;
    DdpgDev *dev = nullptr;
    stmpc_td3 *td3_owner = nullptr;
};
// What every population type holds: its members' slots, the shape they share and the device table of their DdpgDev.
struct PopCore {
    int device = 0, n_obs = 0, capacity = 0, batch = 0;
    size_t lds = 0;
    std::vector<PopSlot> slots;
    DevBuf table;                               // DdpgDev [P]: the slots' dev (pop_upload), for the DDPG kernels, k_ddpg_act_pop, k_replay_push_pop,
                                                // k_per_sample_pop, k_per_update_pop and k_ddpg_stats_pop
    bool per_called = false, per_any = false;   // stmpc_pop_per_enable_* / stmpc_pop_dqn_per_enable was called; at least one member has a tree
    int P() const { return (int)slots.size(); }
    const DdpgDev *dev() const { return table.as<DdpgDev>(); }
    void add(stmpc_ddpg *l) {
        l->pop_member = true;
        slots.push_back({&l->rp, &l->dev, l->td3_owner});
        n_obs = l->cfg.n_obs; capacity = l->cfg.capacity; batch = l->cfg.batch; lds = l->lds;
    }
};
struct stmpc_ddpg_pop {
    PopCore core;
    std::vector<stmpc_ddpg *> bases;        // the members, owned; made by stmpc_ddpg_create, so every single-learner entry works on a borrowed member
};
struct stmpc_td3_pop {
    PopCore core;
    std::vector<stmpc_td3 *> members;       // owned; made by stmpc_td3_create, so every single-learner entry works on a borrowed member (and on its base)
    DevBuf table;                           // Td3Dev [P]: the members' structs (td3_pop_upload)
    const Td3Dev *dev() const { return table.as<Td3Dev>(); }
};

static_assert(DG_POP_MAX == STMPC_DDPG_POP_MAX && STMPC_TD3_POP_MAX == DG_POP_MAX, "DdpgLr holds one learning rate per possible member");

namespace {
// the device tables from the members as they are now: at create, and again once prioritised replay gave members a tree
int pop_upload(PopCore &c) {
    std::vector<DdpgDev> host;
    for (const PopSlot &s : c.slots) host.push_back(*s.dev);
    return upload(c.table, host.data(), host.size());
}
int td3_pop_upload(stmpc_td3_pop *p) {
    std::vector<Td3Dev> host;
    for (const stmpc_td3 *t : p->members) host.push_back(t->dev);
    TRY(upload(p->table, host.data(), host.size()));
    return pop_upload(p->core);
}
int td3_pop_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling[2];
    TRY(raise_dynamic_lds((const void *)k_td3_critic_fwd_pop, "k_td3_critic_fwd_pop", ceiling[0], device, lds));
    TRY(raise_dynamic_lds((const void *)k_td3_actor_fwd_pop, "k_td3_actor_fwd_pop", ceiling[1], device, lds));
    return ddpg_raise_lds(true, device, lds);                       // (k_ddpg_act_pop)
}
// a create entry's checks; same(a, b): two members' cfgs agree in the fields `shared` names
template <class Cfg, class Pop, class F> int pop_check_create(const stmpc_ctx *c, const Cfg *cfgs, int P, Pop **out, const char *shared, F same) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (P < 1 || P > DG_POP_MAX) return fail(STMPC_EINVAL, "a population has 1 ... 64 members, not " + std::to_string(P));
    if (!cfgs) return fail(STMPC_EINVAL, "NULL argument");
    for (int m = 1; m < P; ++m)
        if (!same(cfgs[m], cfgs[0]))
            return fail(STMPC_EINVAL, std::string("the members of a population share ") + shared + " (member " + std::to_string(m) + " differs from member 0)");
    return STMPC_OK;
}
const char *const DDPG_SHARED = "n_obs, h1, h2, batch and capacity";
bool ddpg_same_shape(const stmpc_ddpg_cfg &a, const stmpc_ddpg_cfg &b) {
    return a.n_obs == b.n_obs && a.h1 == b.h1 && a.h2 == b.h2 && a.batch == b.batch && a.capacity == b.capacity;
}
// an update entry's checks behind the population's own, and the learning rates as the kernels take them
// (rates: each HOST array of n_lr learning rates with the struct it goes into -- two of DDPG and TD3, one of DQN)
int pop_check_update(const PopCore &c, int n_updates, int n_lr, std::initializer_list<std::pair<const double *, DdpgLr *>> rates) {
    for (const auto &r : rates)
        if (!r.first) return fail(STMPC_EINVAL, "NULL argument");
    if (n_lr != c.P()) return fail(STMPC_EINVAL, "the learning-rate arrays have " + std::to_string(n_lr) + " entries, the population " + std::to_string(c.P()) + " members");
    if (n_updates < 0) return fail(STMPC_EINVAL, "n_updates is negative");
    for (const auto &r : rates)
        for (int m = 0; m < c.P(); ++m) {
            if (!(r.first[m] >= 0)) return fail(STMPC_EINVAL, "a member's learning rate is negative");
            r.second->lr[m] = (float)r.first[m];
        }
    return STMPC_OK;
}
// what an acting or pushing entry of any population checks of its row count and stride
int pop_check_rows(const PopCore &c, int n_per_member, int obs_stride) {
    if (n_per_member < 1 || n_per_member > c.capacity || obs_stride < c.n_obs)
        return fail(STMPC_EINVAL, "n_per_member must be in 1 ... capacity, and obs_stride at least the observation's width");
    return STMPC_OK;
}
// ... and a pushing entry of the members' n-step windows
int pop_check_push(const PopCore &c, int n_per_member) {
    for (const PopSlot &s : c.slots) TRY(nstep_check_push(*s.dev, n_per_member));
    return STMPC_OK;
}
// stmpc_nstep_enable_* per member -- every check before any member changes --, then the device tables anew (upload_tables)
template <class F> int pop_nstep_enable(PopCore &c, const stmpc_nstep_cfg *cfgs, int P, F upload_tables) {
    if (!cfgs) return fail(STMPC_EINVAL, "NULL argument");
    if (P != c.P()) return fail(STMPC_EINVAL, "cfgs has " + std::to_string(P) + " entries, the population " + std::to_string(c.P()) + " members");
    std::vector<DdpgDev> probe;
    for (int m = 0; m < P; ++m) { probe.push_back(*c.slots[m].dev); TRY(nstep_attach(*c.slots[m].rp, probe[m], cfgs + m)); }
    for (int m = 0; m < P; ++m) {
        c.slots[m].dev->n_step = probe[m].n_step; c.slots[m].dev->rows_push = probe[m].rows_push;
        if (c.slots[m].td3_owner) td3_refresh(c.slots[m].td3_owner);
    }
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(hipDeviceSynchronize());
    return upload_tables();
}
// acting and pushing of the members: the DDPG population's own, and a TD3 population's on its members' bases
int pop_act(const PopCore &c, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise, double *d_action, uint32_t *d_debug, void *stream) {
    TRY(pop_check_rows(c, n_per_member, obs_stride));
    if (!d_obs || !d_ticks || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(c.device));
    hipLaunchKernelGGL(k_ddpg_act_pop, dim3((n_per_member + AT_TM - 1) / AT_TM, c.P()), dim3(AT_THREADS), c.lds, (hipStream_t)stream, c.dev(), n_per_member, d_obs,
                       obs_stride, d_ticks, noise != 0, d_action, d_debug);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
int pop_push(const PopCore &c, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_ticks,
             const int32_t *d_next_ticks, const double *d_action, const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    TRY(pop_check_rows(c, n_per_member, obs_stride));
    TRY(pop_check_push(c, n_per_member));
    if (!d_obs || !d_next_obs || !d_ticks || !d_action || !d_reward || !d_terminated || !d_truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(c.device));
    hipLaunchKernelGGL(k_replay_push_pop, dim3(push_blocks(n_per_member), c.P()), dim3(256), 0, (hipStream_t)stream, c.dev(), n_per_member, d_obs, d_next_obs, d_final_obs,
                       obs_stride, d_ticks, d_next_ticks, d_action, d_reward, d_terminated, d_truncated);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}
// stmpc_per_enable's work per enabled member -- every check before anything is attached --, then the device tables anew (upload_tables).  An
// allocation that fails leaves the members before it prioritised, which the tables then say too.
template <class F> int pop_per_enable(PopCore &c, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P, F upload_tables) {
    if (!cfgs || !enabled) return fail(STMPC_EINVAL, "NULL argument");
    if (P != c.P()) return fail(STMPC_EINVAL, "cfgs and enabled have " + std::to_string(P) + " entries, the population " + std::to_string(c.P()) + " members");
    if (c.per_called) return fail(STMPC_EINVAL, "prioritised replay was already set up on this population (one call, on empty rings)");
    for (int m = 0; m < P; ++m)
        if (enabled[m]) { TRY(per_check_cfg(cfgs + m)); TRY(c.slots[m].rp->check_empty()); }
    c.per_called = true;
    int rc = STMPC_OK;
    for (int m = 0; m < P && !rc; ++m)
        if (enabled[m]) { rc = per_attach(*c.slots[m].rp, *c.slots[m].dev, c.slots[m].td3_owner, cfgs + m); c.per_any = c.per_any || !rc; }
    if (!c.per_any) return rc;                                      // (no member enabled: the tables stand)
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(hipDeviceSynchronize());
    TRY(upload_tables());
    return rc;
}
}  // namespace

extern "C" {

int stmpc_ddpg_pop_create(stmpc_ctx *c, const stmpc_ddpg_cfg *cfgs, int P, stmpc_ddpg_pop **out) {
    TRY(pop_check_create(c, cfgs, P, out, DDPG_SHARED, ddpg_same_shape));
    HIPCHK(hipSetDevice(c->device));
    stmpc_ddpg_pop *p = new stmpc_ddpg_pop();
    p->core.device = c->device;
    int rc = STMPC_OK;
    for (int m = 0; m < P && !rc; ++m) {
        stmpc_ddpg *l = nullptr;
        rc = stmpc_ddpg_create(c, cfgs + m, &l);
        if (!rc) { p->bases.push_back(l); p->core.add(l); }
    }
    if (!rc) rc = pop_upload(p->core);
    if (!rc) rc = ddpg_raise_lds(true, c->device, p->core.lds);
    if (rc) { stmpc_ddpg_pop_destroy(p); return rc; }
    *out = p;
    return STMPC_OK;
}

void stmpc_ddpg_pop_destroy(stmpc_ddpg_pop *p) {
    if (!p) return;
    for (stmpc_ddpg *l : p->bases) stmpc_ddpg_destroy(l);
    (void)hipSetDevice(p->core.device);
    delete p;
}

int stmpc_ddpg_pop_size(const stmpc_ddpg_pop *p) { return p ? p->core.P() : 0; }

stmpc_ddpg *stmpc_ddpg_pop_member(stmpc_ddpg_pop *p, int m) {
    if (!p || m < 0 || m >= p->core.P()) { (void)fail(STMPC_EINVAL, "population is NULL, or no such member"); return nullptr; }
    return p->bases[m];
}

int stmpc_ddpg_pop_act_device(stmpc_ddpg_pop *p, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise, double *d_action,
                              uint32_t *d_debug, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_act(p->core, n_per_member, d_obs, obs_stride, d_ticks, noise, d_action, d_debug, stream);
}

int stmpc_ddpg_pop_push_device(stmpc_ddpg_pop *p, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                               const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward, const uint8_t *d_terminated,
                               const uint8_t *d_truncated, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_push(p->core, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks, d_action, d_reward, d_terminated, d_truncated, stream);
}

int stmpc_ddpg_pop_update_device(stmpc_ddpg_pop *p, int n_updates, const double *lr_q, const double *lr_pi, int n_lr, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "NULL argument");
    DdpgLr lq{}, lp{};
    TRY(pop_check_update(p->core, n_updates, n_lr, {{lr_q, &lq}, {lr_pi, &lp}}));
    HIPCHK(hipSetDevice(p->core.device));
    const stmpc_ddpg *l = p->bases[0];
    const DdpgDev *tab = p->core.dev();
    const Grid g = l->grid;
    const int P = p->core.P(), B = l->cfg.batch, Bp = l->rp.Bp;
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // stmpc_ddpg_update_device's six launches (eight with prioritised members), each over the members
        if (p->core.per_any) hipLaunchKernelGGL(k_per_sample_pop, dim3(1, P), dim3(PER_THREADS), 0, st, tab, B, Bp, 1);
        hipLaunchKernelGGL(k_ddpg_critic_fwd_pop, dim3(g.tiles, P), dim3(AT_THREADS), l->lds, st, tab, B, 1);
        hipLaunchKernelGGL(k_ddpg_wgrad_pop, dim3(g.jobs, P), dim3(64 * DG_WG_WAVES), 0, st, tab, 1, Bp, 1);
        if (p->core.per_any) hipLaunchKernelGGL(k_per_update_pop, dim3(1, P), dim3(PER_THREADS), 0, st, tab, B, 1);
        hipLaunchKernelGGL(k_ddpg_adam_pop, dim3(g.ablocks, P), dim3(256), 0, st, tab, 1, lq, 0, 0, 1);
        hipLaunchKernelGGL(k_ddpg_actor_fwd_pop, dim3(g.tiles, P), dim3(AT_THREADS), l->lds, st, tab, B, 1);
        hipLaunchKernelGGL(k_ddpg_wgrad_pop, dim3(g.jobs, P), dim3(64 * DG_WG_WAVES), 0, st, tab, 0, Bp, 1);
        hipLaunchKernelGGL(k_ddpg_adam_pop, dim3(g.ablocks, P), dim3(256), 0, st, tab, 0, lp, 0, 1, 1);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_ddpg_pop_stats_device(stmpc_ddpg_pop *p, double *d_out, void *stream) {
    if (!p || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->core.device));
    hipLaunchKernelGGL(k_ddpg_stats_pop, dim3(1, p->core.P()), dim3(64), 0, (hipStream_t)stream, p->core.dev(), p->core.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_pop_nstep_enable_ddpg(stmpc_ddpg_pop *p, const stmpc_nstep_cfg *cfgs, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_nstep_enable(p->core, cfgs, P, [&] { return pop_upload(p->core); });
}

int stmpc_pop_per_enable_ddpg(stmpc_ddpg_pop *p, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_per_enable(p->core, cfgs, enabled, P, [&] { return pop_upload(p->core); });
}

int stmpc_pop_td3_create(stmpc_ctx *c, const stmpc_td3_cfg *cfgs, int P, stmpc_td3_pop **out) {
    TRY(pop_check_create(c, cfgs, P, out, DDPG_SHARED, [](const stmpc_td3_cfg &a, const stmpc_td3_cfg &b) { return ddpg_same_shape(a.base, b.base); }));
    HIPCHK(hipSetDevice(c->device));
    stmpc_td3_pop *p = new stmpc_td3_pop();
    p->core.device = c->device;
    int rc = STMPC_OK;
    for (int m = 0; m < P && !rc; ++m) {
        stmpc_td3 *t = nullptr;
        rc = stmpc_td3_create(c, cfgs + m, &t);
        if (!rc) { p->members.push_back(t); p->core.add(t->base); }
    }
    if (!rc) rc = td3_pop_upload(p);
    if (!rc) rc = td3_pop_raise_lds(c->device, p->core.lds);
    if (rc) { stmpc_pop_td3_destroy(p); return rc; }
    *out = p;
    return STMPC_OK;
}

void stmpc_pop_td3_destroy(stmpc_td3_pop *p) {
    if (!p) return;
    for (stmpc_td3 *t : p->members) stmpc_td3_destroy(t);
    (void)hipSetDevice(p->core.device);
    delete p;
}

int stmpc_pop_td3_size(const stmpc_td3_pop *p) { return p ? p->core.P() : 0; }

stmpc_td3 *stmpc_pop_td3_member(stmpc_td3_pop *p, int m) {
    if (!p || m < 0 || m >= p->core.P()) { (void)fail(STMPC_EINVAL, "population is NULL, or no such member"); return nullptr; }
    return p->members[m];
}

int stmpc_pop_td3_act_device(stmpc_td3_pop *p, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise, double *d_action,
                             uint32_t *d_debug, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_act(p->core, n_per_member, d_obs, obs_stride, d_ticks, noise, d_action, d_debug, stream);
}

int stmpc_pop_td3_push_device(stmpc_td3_pop *p, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                              const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward, const uint8_t *d_terminated,
                              const uint8_t *d_truncated, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_push(p->core, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks, d_action, d_reward, d_terminated, d_truncated, stream);
}

int stmpc_pop_td3_update_device(stmpc_td3_pop *p, int n_updates, const double *lr_q, const double *lr_pi, int n_lr, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "NULL argument");
    DdpgLr lq{}, lp{};
    TRY(pop_check_update(p->core, n_updates, n_lr, {{lr_q, &lq}, {lr_pi, &lp}}));
    HIPCHK(hipSetDevice(p->core.device));
    const stmpc_ddpg *l = p->members[0]->base;
    const Grid g = l->grid;
    const int P = p->core.P(), B = l->cfg.batch, Bp = l->rp.Bp;
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // stmpc_td3_update_device's six launches (eight with prioritised members), each over the members in gridDim.z
        if (p->core.per_any) hipLaunchKernelGGL(k_per_sample_td3_pop, dim3(1, 1, P), dim3(PER_THREADS), 0, st, p->dev(), B, Bp, 1);
        hipLaunchKernelGGL(k_td3_critic_fwd_pop, dim3(g.tiles, 2, P), dim3(AT_THREADS), l->lds, st, p->dev(), B, 1);
        hipLaunchKernelGGL(k_td3_wgrad_pop, dim3(g.jobs, 2, P), dim3(64 * DG_WG_WAVES), 0, st, p->dev(), 1, Bp, 1);
        if (p->core.per_any) hipLaunchKernelGGL(k_per_update_td3_pop, dim3(1, 1, P), dim3(PER_THREADS), 0, st, p->dev(), B, 1);
        hipLaunchKernelGGL(k_td3_adam_critics_pop, dim3(g.ablocks, 2, P), dim3(256), 0, st, p->dev(), lq, 1);
        hipLaunchKernelGGL(k_td3_actor_fwd_pop, dim3(g.tiles, 1, P), dim3(AT_THREADS), l->lds, st, p->dev(), B, 1);
        hipLaunchKernelGGL(k_td3_wgrad_pop, dim3(g.jobs, 1, P), dim3(64 * DG_WG_WAVES), 0, st, p->dev(), 0, Bp, 1);
        hipLaunchKernelGGL(k_td3_adam_finish_pop, dim3(g.ablocks, 3, P), dim3(256), 0, st, p->dev(), lp, 1);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_pop_td3_stats_device(stmpc_td3_pop *p, double *d_out, void *stream) {
    if (!p || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->core.device));
    hipLaunchKernelGGL(k_td3_stats_pop, dim3(1, 1, p->core.P()), dim3(64), 0, (hipStream_t)stream, p->dev(), p->core.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_pop_nstep_enable_td3(stmpc_td3_pop *p, const stmpc_nstep_cfg *cfgs, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_nstep_enable(p->core, cfgs, P, [&] { return td3_pop_upload(p); });
}

int stmpc_pop_per_enable_td3(stmpc_td3_pop *p, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_per_enable(p->core, cfgs, enabled, P, [&] { return td3_pop_upload(p); });
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
    HIPCHK(hipSetDevice(l->rp.device));
    stmpc_actor *a = new stmpc_actor();     // owns no buffer: destroying it frees nothing of the learner's
    a->device = l->rp.device; a->lds = actor_lds_bytes(l->h1p, l->h2p);
    a->dev.p0 = target ? pi.t0 : pi.p0; a->dev.b0 = w + dg_o_b0(l->h1p);
    a->dev.p1 = target ? pi.t1 : pi.p1; a->dev.b1 = w + dg_o_b1(l->h1p, l->h2p);
    a->dev.w2 = w + dg_o_w2(l->h1p, l->h2p); a->dev.b2p = w + dg_o_b2(l->h1p, l->h2p);
    a->dev.scale = l->dev.scale; a->dev.mean = l->dev.mean; a->dev.n_in = pi.n_in; a->dev.h1p = l->h1p; a->dev.h2p = l->h2p;
    const int rc = actor_raise_lds(0, l->rp.device, a->lds);
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

// ---- the discrete learners (stmpc_dqn_*, stmpc_c51_*): a discrete agent on a replay store, one network and one workspace of its own, written once
// for both heads; kernels in stmpc_dqn_kernels.hpp and stmpc_c51_kernels.hpp ----------------------------------------------------------------------
// What the DQN learner and the categorical one differ in is their Head (DqnHead, C51Head below): the cfg and device structs, the network's output
// width, the LDS size, the head's own cfg checks and device fields, and the kernels.  A C51 learner is not a DQN learner: its device struct is a
// C51Dev and its network's output width is n_actions * n_atoms, or (n_actions + 1) * n_atoms with a dueling head (cfg.dueling).
template <class H> struct QLearner {
    using Head = H;
    typename H::Cfg cfg{};
    typename H::Dev dev{};                  // base(): the constants (q_create), base().q the network (base().h2: its output width, base().h2p = Ap;
                                            // base().pi stays null), the workspace, and the replay's part, which rp.wire writes at create and again
                                            // in q_per_enable
    Replay rp;
    DevBuf net[11], ws[7];
    std::vector<Seg> lay;
    int h1p = 0, Ap = 0, np = 0;
    size_t lds = 0;
    Grid grid{};
    bool pop_member = false;                // owned by a population (QPop), whose device tables hold copies of dev and base()
    typename H::Extra ex;                   // what one head has on top (C51Head: the noisy output layer's buffers; stmpc_noisy_c51_enable)
    DdpgDev &base() { return H::base(dev); }        // dev.base of a DqnDev, dev.dq.base of a C51Dev
};

struct DqnHead {
    using Cfg = stmpc_dqn_cfg;
    using Dev = DqnDev;
    using L = QLearner<DqnHead>;
    struct Extra {};
    static constexpr const char *name = "DQN", *shared = "n_obs, h1, n_actions, batch and capacity";
    static bool noisy(const L &) { return false; }
    static void noisy_update(const L &, float, hipStream_t) {}
    static void noisy_grads(const L &, hipStream_t) {}
    static constexpr const char *pop_per_enable = "stmpc_pop_dqn_per_enable", *pop_nstep_enable = "stmpc_pop_nstep_enable_dqn";      // (what a member's refusals name)
    static DdpgDev &base(Dev &d) { return d.base; }
    static DqnDev &dq(Dev &d) { return d; }
    static int n_out(const Cfg &g) { return g.n_actions; }
    static size_t tile_bytes(const Cfg &, int h1p, int Ap) { return ddpg_tile_bytes(h1p, Ap); }
    static int check(const Cfg &) { return STMPC_OK; }
    static bool constants_ok(const Cfg &g) { return !g.clip_targets || g.clip_min <= g.clip_max; }
    static bool same_shape(const Cfg &a, const Cfg &b) { return a.n_obs == b.n_obs && a.h1 == b.h1 && a.n_actions == b.n_actions && a.batch == b.batch && a.capacity == b.capacity; }
    static void wire(Dev &d, const Cfg &g) { d.clip = g.clip_targets != 0; d.clip_min = (float)g.clip_min; d.clip_max = (float)g.clip_max; }
    static int raise_lds(bool pop, int device, size_t lds) {
        static LdsCeiling ceiling[2][2];
        static const void *const fn[2][2] = {{(const void *)k_dqn_fwd, (const void *)k_dqn_act}, {(const void *)k_dqn_fwd_pop, (const void *)k_dqn_act_pop}};
        static const char *const kernel[2][2] = {{"k_dqn_fwd", "k_dqn_act"}, {"k_dqn_fwd_pop", "k_dqn_act_pop"}};
        TRY(raise_dynamic_lds(fn[pop][0], kernel[pop][0], ceiling[pop][0], device, lds));
        return raise_dynamic_lds(fn[pop][1], kernel[pop][1], ceiling[pop][1], device, lds);
    }
    // the launches of a lone learner ...
    static void fwd(const L &t, int gate, hipStream_t st) { hipLaunchKernelGGL(k_dqn_fwd, dim3(t.grid.tiles), dim3(AT_THREADS), t.lds, st, t.dev, t.cfg.batch, gate, (float *)nullptr); }
    static void wgrad(const L &t, int gate, hipStream_t st) { hipLaunchKernelGGL(k_dqn_wgrad, dim3(t.grid.jobs), dim3(64 * DG_WG_WAVES), 0, st, t.dev, t.rp.Bp, gate); }
    static void adam(const L &t, float lr, int mode, hipStream_t st) { hipLaunchKernelGGL(k_dqn_adam, dim3(t.grid.ablocks), dim3(256), 0, st, t.dev, lr, mode, 1); }
    static void unpad(const L &t, float *d_grad, hipStream_t st) { hipLaunchKernelGGL(k_dqn_unpad, dim3(128), dim3(256), 0, st, t.dev, (const float *)t.dev.base.q.g, d_grad); }
    static void stats(const L &t, double *d_out, hipStream_t st) { hipLaunchKernelGGL(k_dqn_stats, dim3(1), dim3(64), 0, st, t.dev, t.cfg.batch, d_out); }
    static void act(const L &t, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, hipStream_t st) {
        hipLaunchKernelGGL(k_dqn_act, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), t.lds, st, t.dev, N, d_obs, obs_stride, (float)eps, eps > 0 ? 1 : 0, d_action, d_debug_q);
    }
    // ... and of a population of P, on its table of device structs
    static void fwd_pop(const L &, const Dev *tab, const Grid &g, int P, size_t lds, int B, hipStream_t st) { hipLaunchKernelGGL(k_dqn_fwd_pop, dim3(g.tiles, P), dim3(AT_THREADS), lds, st, tab, B, 1); }
    static void wgrad_pop(const Dev *tab, const Grid &g, int P, int Bp, hipStream_t st) { hipLaunchKernelGGL(k_dqn_wgrad_pop, dim3(g.jobs, P), dim3(64 * DG_WG_WAVES), 0, st, tab, Bp, 1); }
    static void adam_pop(const Dev *tab, const Grid &g, int P, const DdpgLr &lrs, hipStream_t st) { hipLaunchKernelGGL(k_dqn_adam_pop, dim3(g.ablocks, P), dim3(256), 0, st, tab, lrs, 1); }
    static void act_pop(const Dev *tab, int P, size_t lds, int n, const float *d_obs, int obs_stride, const DqnEps &e, int32_t *d_action, float *d_debug_q, hipStream_t st) {
        hipLaunchKernelGGL(k_dqn_act_pop, dim3((n + AT_TM - 1) / AT_TM, P), dim3(AT_THREADS), lds, st, tab, n, d_obs, obs_stride, e, d_action, d_debug_q);
    }
    static void push_pop(const Dev *tab, int P, int n, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_action,
                         const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, hipStream_t st) {
        hipLaunchKernelGGL(k_dqn_push_pop, dim3(push_blocks(n), P), dim3(256), 0, st, tab, n, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated,
                           d_truncated);
    }
};

// the widest layer: n_actions * n_atoms logits, (n_actions + 1) * n_atoms with a dueling head's value block (stmpc_c51_create and the actors' creates)
static int c51_check_width(int n_actions, int n_atoms, int dueling) {
    const long long W = (long long)(n_actions + (dueling ? 1 : 0)) * n_atoms;
    if (W <= STMPC_C51_MAX_LOGITS) return STMPC_OK;
    if (dueling) return fail(STMPC_EINVAL, "(n_actions + 1) * n_atoms = " + std::to_string(W) + " (a dueling head) exceeds " + std::to_string(STMPC_C51_MAX_LOGITS));
    return fail(STMPC_EINVAL, "n_actions * n_atoms = " + std::to_string(W) + " exceeds " + std::to_string(STMPC_C51_MAX_LOGITS));
}

// The noisy output layer of a C51 learner (stmpc_noisy_c51_enable; kernels in stmpc_c51_noisy_kernels.hpp): sigma, its target and Adam moments, the f
// vectors, and per draw (online, target, acting) the effective parameter array and its packed W1, which a shadow of the learner's struct points at.
struct C51Noisy {
    bool on = false;
    double sigma0 = 0;
    DevBuf sig, sigt, sm, sv, f, we[C51_NZ_SETS], pe[C51_NZ_SETS];
    C51NoisyDev dev{};
    // the learner's struct as it is now with the network's effective copies in the online (and target) network's place
    C51Dev shadow(const C51Dev &own, bool acting) const {
        C51Dev s = own;
        DdpgNet &n = s.dq.base.q;
        if (acting) { n.w = dev.we2; n.p1 = dev.pe2; }
        else { n.w = dev.we0; n.p1 = dev.pe0; n.wt = dev.we1; n.t1 = dev.pe1; }
        return s;
    }
};

struct C51Head {
    using Cfg = stmpc_c51_cfg;
    using Dev = C51Dev;
    using L = QLearner<C51Head>;
    using Extra = C51Noisy;
    static constexpr const char *name = "C51", *shared = "n_obs, h1, n_actions, n_atoms, batch and capacity";      // (and the head: dueling or not)
    static constexpr const char *pop_per_enable = "stmpc_pop_c51_per_enable", *pop_nstep_enable = "stmpc_pop_c51_multi_step_enable";
    static DdpgDev &base(Dev &d) { return d.dq.base; }
    static DqnDev &dq(Dev &d) { return d.dq; }
    static int n_out(const Cfg &g) { return (g.n_actions + (g.dueling ? 1 : 0)) * g.n_atoms; }       // (a dueling head: the value block behind the advantage blocks)
    static size_t tile_bytes(const Cfg &g, int h1p, int Ap) { return c51_tile_bytes(h1p, Ap, g.n_atoms); }
    static int check(const Cfg &g) {
        if (g.n_atoms < 2) return fail(STMPC_EINVAL, "n_atoms must be at least 2");
        if (g.dueling != 0 && g.dueling != 1) return fail(STMPC_EINVAL, "dueling must be 0 or 1, not " + std::to_string(g.dueling));
        TRY(c51_check_width(g.n_actions, g.n_atoms, g.dueling));
        if (!std::isfinite(g.v_min) || !std::isfinite(g.v_max) || !(g.v_max > g.v_min)) return fail(STMPC_EINVAL, "the support needs finite v_min < v_max");
        return STMPC_OK;
    }
    static bool constants_ok(const Cfg &) { return true; }          // (clip_targets is not read: the support's clamp is the clip)
    static bool same_shape(const Cfg &a, const Cfg &b) {
        return a.n_obs == b.n_obs && a.h1 == b.h1 && a.n_actions == b.n_actions && a.n_atoms == b.n_atoms && a.dueling == b.dueling && a.batch == b.batch &&
               a.capacity == b.capacity;
    }
    static void wire(Dev &d, const Cfg &g) { d.dq.clip = 0; d.K = g.n_atoms; d.dueling = g.dueling; d.v_min = g.v_min; d.v_max = g.v_max; d.dz = (g.v_max - g.v_min) / (double)(g.n_atoms - 1); }
    static int raise_lds(bool pop, int device, size_t lds) {
        static LdsCeiling ceiling[2][3];
        static const void *const fn[2][3] = {{(const void *)k_c51_fwd, (const void *)k_c51_act, (const void *)k_c51_fwd_duel},
                                             {(const void *)k_c51_fwd_pop, (const void *)k_c51_act_pop, (const void *)k_c51_fwd_duel_pop}};
        static const char *const kernel[2][3] = {{"k_c51_fwd", "k_c51_act", "k_c51_fwd_duel"}, {"k_c51_fwd_pop", "k_c51_act_pop", "k_c51_fwd_duel_pop"}};
        for (int k = 0; k < 3; ++k) TRY(raise_dynamic_lds(fn[pop][k], kernel[pop][k], ceiling[pop][k], device, lds));      // (both heads' passes: the LDS size is one)
        return STMPC_OK;
    }
    // the forward / backward pass has a kernel per head (d_out, d_dist: the debug outputs of stmpc_c51_dist_device, null in an update)
    // (a noisy learner's pass runs on the shadow struct behind the draw's compose: noisy_fwd)
    static void fwd_on(const Dev &dev, const L &t, int gate, float *d_out, float *d_dist, hipStream_t st) {
        if (dev.dueling) hipLaunchKernelGGL(k_c51_fwd_duel, dim3(t.grid.tiles), dim3(AT_THREADS), t.lds, st, dev, t.cfg.batch, gate, d_out, d_dist);
        else hipLaunchKernelGGL(k_c51_fwd, dim3(t.grid.tiles), dim3(AT_THREADS), t.lds, st, dev, t.cfg.batch, gate, d_out, d_dist);
    }
    static void fwd_launch(const L &t, int gate, float *d_out, float *d_dist, hipStream_t st) {
        if (t.ex.on) noisy_fwd(t, gate, d_out, d_dist, st);
        else fwd_on(t.dev, t, gate, d_out, d_dist, st);
    }
    // the noisy learner's launches: the learning draw of the current update index, the pass and the weight gradients on the shadow struct ...
    static bool noisy(const L &t) { return t.ex.on; }
    static int compose_blocks(const L &t) { return (t.h1p + (t.h1p + 1) * t.Ap + 255) / 256; }
    static void noisy_fwd(const L &t, int gate, float *d_out, float *d_dist, hipStream_t st) {
        hipLaunchKernelGGL(k_c51_noisy_compose, dim3(compose_blocks(t)), dim3(256), 0, st, t.dev, t.ex.dev, 0, gate);
        fwd_on(t.ex.shadow(t.dev, false), t, gate, d_out, d_dist, st);
    }
    static void noisy_grads(const L &t, hipStream_t st) {
        noisy_fwd(t, 0, nullptr, nullptr, st);
        hipLaunchKernelGGL(k_c51_wgrad, dim3(t.grid.jobs), dim3(64 * DG_WG_WAVES), 0, st, t.ex.shadow(t.dev, false), t.rp.Bp, 0);
    }
    // ... and one update behind the sampling step: compose, fwd, wgrad, (the priority update,) sigma's and mu's Adam
    static void noisy_update(const L &t, float lr, hipStream_t st) {
        noisy_fwd(t, 1, nullptr, nullptr, st);
        hipLaunchKernelGGL(k_c51_wgrad, dim3(t.grid.jobs), dim3(64 * DG_WG_WAVES), 0, st, t.ex.shadow(t.dev, false), t.rp.Bp, 1);
        per_launch_update(t.rp, t.dev.dq.base, st);
        hipLaunchKernelGGL(k_c51_noisy_adam, dim3(t.grid.ablocks), dim3(256), 0, st, t.dev, t.ex.dev, lr, 1);
    }
    static void fwd(const L &t, int gate, hipStream_t st) { fwd_launch(t, gate, nullptr, nullptr, st); }
    static void wgrad(const L &t, int gate, hipStream_t st) { hipLaunchKernelGGL(k_c51_wgrad, dim3(t.grid.jobs), dim3(64 * DG_WG_WAVES), 0, st, t.dev, t.rp.Bp, gate); }
    static void adam(const L &t, float lr, int mode, hipStream_t st) { hipLaunchKernelGGL(k_c51_adam, dim3(t.grid.ablocks), dim3(256), 0, st, t.dev, lr, mode, 1); }
    static void unpad(const L &t, float *d_grad, hipStream_t st) { hipLaunchKernelGGL(k_c51_unpad, dim3(128), dim3(256), 0, st, t.dev, (const float *)t.dev.dq.base.q.g, d_grad); }
    static void stats(const L &t, double *d_out, hipStream_t st) { hipLaunchKernelGGL(k_c51_stats, dim3(1), dim3(64), 0, st, t.dev, t.cfg.batch, d_out); }
    static void act(const L &t, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, hipStream_t st) {
        hipLaunchKernelGGL(k_c51_act, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), t.lds, st, t.dev, N, d_obs, obs_stride, (float)eps, eps > 0 ? 1 : 0, d_action, d_debug_q);
    }
    static void fwd_pop(const L &t0, const Dev *tab, const Grid &g, int P, size_t lds, int B, hipStream_t st) {      // (t0: member 0; the members share the head)
        if (t0.dev.dueling) hipLaunchKernelGGL(k_c51_fwd_duel_pop, dim3(g.tiles, P), dim3(AT_THREADS), lds, st, tab, B, 1);
        else hipLaunchKernelGGL(k_c51_fwd_pop, dim3(g.tiles, P), dim3(AT_THREADS), lds, st, tab, B, 1);
    }
    static void wgrad_pop(const Dev *tab, const Grid &g, int P, int Bp, hipStream_t st) { hipLaunchKernelGGL(k_c51_wgrad_pop, dim3(g.jobs, P), dim3(64 * DG_WG_WAVES), 0, st, tab, Bp, 1); }
    static void adam_pop(const Dev *tab, const Grid &g, int P, const DdpgLr &lrs, hipStream_t st) { hipLaunchKernelGGL(k_c51_adam_pop, dim3(g.ablocks, P), dim3(256), 0, st, tab, lrs, 1); }
    static void act_pop(const Dev *tab, int P, size_t lds, int n, const float *d_obs, int obs_stride, const DqnEps &e, int32_t *d_action, float *d_debug_q, hipStream_t st) {
        hipLaunchKernelGGL(k_c51_act_pop, dim3((n + AT_TM - 1) / AT_TM, P), dim3(AT_THREADS), lds, st, tab, n, d_obs, obs_stride, e, d_action, d_debug_q);
    }
    static void push_pop(const Dev *tab, int P, int n, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_action,
                         const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, hipStream_t st) {
        hipLaunchKernelGGL(k_c51_push_pop, dim3(push_blocks(n), P), dim3(256), 0, st, tab, n, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated,
                           d_truncated);
    }
};

struct stmpc_dqn : QLearner<DqnHead> {};
struct stmpc_c51 : QLearner<C51Head> {};
static_assert(STMPC_DQN_GRAD == STMPC_C51_GRAD, "q_padded_read takes either head's gradient slot");

namespace {
// the entries both heads have, each behind a one-line extern "C" forward; L: stmpc_dqn or stmpc_c51
template <class L> void q_destroy(L *t) {
    if (!t) return;
    (void)hipSetDevice(t->rp.device);
    delete t;
}

template <class L> int q_create(stmpc_ctx *c, const typename L::Head::Cfg *g, L **out) {
    using H = typename L::Head;
    if (!c || !g || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (g->n_actions < 1 || g->n_actions > STMPC_ENV_MAX_ACTIONS) return fail(STMPC_EINVAL, "n_actions must be in 1 ... " + std::to_string(STMPC_ENV_MAX_ACTIONS));
    TRY(H::check(*g));
    if (g->n_obs < 1 || g->n_obs > AT_KIN - 1 || g->h1 < 1 || g->h1 > 1024)
        return fail(STMPC_EINVAL, std::string(H::name) + " network shape out of range (n_obs <= 31, hidden width <= 1024)");
    if (g->batch < 1 || g->batch > PER_MAX_B) return fail(STMPC_EINVAL, "batch must be in 1 ... 8192");
    if (g->target_period < 1) return fail(STMPC_EINVAL, "target_period must be at least 1");
    if (g->capacity < 1 || g->replay_start < 0 || g->replay_start >= g->capacity) return fail(STMPC_EINVAL, "capacity must be positive and replay_start below it");
    if (!(g->gamma >= 0) || !std::isfinite(g->gamma) || !(g->beta1 >= 0 && g->beta1 < 1) || !(g->beta2 >= 0 && g->beta2 < 1) || !(g->eps > 0) || !H::constants_ok(*g))
        return fail(STMPC_EINVAL, std::string(H::name) + " constants out of range");
    HIPCHK(hipSetDevice(c->device));
    const int W = H::n_out(*g), h1p = (g->h1 + 15) & ~15, Ap = (W + 15) & ~15;
    const size_t lds = H::tile_bytes(*g, h1p, Ap);
    if (lds + 1024 > (size_t)c->lds_per_block) return fail(STMPC_EINVAL, std::string(H::name) + " network too wide for one workgroup's LDS");
    L *t = new L();
    t->cfg = *g; t->h1p = h1p; t->Ap = Ap; t->np = dg_nparam(h1p, Ap); t->lds = lds;
    t->lay = slot_layout(g->n_obs, g->h1, W, h1p, Ap, false);
    t->rp.device = c->device;                                        // (what destroy selects, should an allocation fail)
    DdpgDev &d = t->base();
    int rc = net_build(t->net, d.q, g->n_obs, h1p, Ap);
    if (!rc) rc = ws_build(t->ws, d, (g->batch + 15) & ~15, h1p, Ap);
    if (!rc) rc = t->rp.create(c->device, g->batch, g->capacity);     // (the ring behind the net and the workspace: the order the buffers always had)
    if (!rc) rc = H::raise_lds(false, c->device, lds);
    if (rc) { q_destroy(t); return rc; }
    t->grid = make_grid(t->rp.Bp, h1p, Ap, false);
    d.n_obs = g->n_obs; d.h1 = g->h1; d.h2 = W; d.h1p = h1p; d.h2p = Ap; d.replay_start = g->replay_start; d.seed = g->seed;
    d.gamma = (float)g->gamma; d.beta1 = (float)g->beta1; d.beta2 = (float)g->beta2;
    d.omb1 = 1.0f - d.beta1; d.omb2 = 1.0f - d.beta2; d.eps = (float)g->eps;       // (tau, the time feature, the squash and the noise: unused, 0)
    t->rp.wire(d);
    DqnDev &q = H::dq(t->dev);
    q.A = g->n_actions; q.Ap = Ap; q.dbl = g->double_dqn != 0; q.target_period = g->target_period;
    H::wire(t->dev, *g);                                             // (the clip range, or the support)
    *out = t;
    return STMPC_OK;
}

template <class L> int q_set_params(L *t, int slot, const float *values, int64_t count) {
    TRY(slot_args(t, values, slot, 4));
    return slot_set(t->rp.device, t->lay, t->np, net_slot(t->base().q, slot), values, count, slot < 2, [&] { L::Head::adam(*t, 0.f, 1, (hipStream_t)0); });
}

template <class L> int q_get_params(L *t, int slot, float *values, int64_t count) {
    TRY(slot_args(t, values, slot, 4));
    return slot_get(t->rp.device, t->lay, t->np, net_slot(t->base().q, slot), values, count);
}

template <class L> int q_set_state(L *t, const int64_t *counters, const float *beta_pow) {
    if (!t || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    TRY(t->rp.set_counters(counters));
    HIPCHK(hipMemcpy(t->base().q.bpow, beta_pow, 2 * sizeof(float), hipMemcpyHostToDevice));
    return STMPC_OK;
}

template <class L> int q_get_state(L *t, int64_t *counters, float *beta_pow) {
    if (!t || !counters || !beta_pow) return fail(STMPC_EINVAL, "NULL argument");
    TRY(t->rp.get_counters(counters));
    HIPCHK(hipMemcpy(beta_pow, t->base().q.bpow, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return STMPC_OK;
}

// (both heads push with the DQN learner's own kernel on the embedded DqnDev: the row has the same columns)
template <class L> int q_push(L *t, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_action,
                              const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (N < 0 || N > t->cfg.capacity || obs_stride < t->cfg.n_obs) return fail(STMPC_EINVAL, "N exceeds the replay capacity, or obs_stride is shorter than the observation");
    if (N == 0) return STMPC_OK;
    TRY(nstep_check_push(t->base(), N));
    if (!d_obs || !d_next_obs || !d_action || !d_reward || !d_terminated || !d_truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(t->rp.device));
    hipLaunchKernelGGL(k_dqn_push, dim3(push_blocks(N)), dim3(256), 0, (hipStream_t)stream, L::Head::dq(t->dev), N, d_obs, d_next_obs, d_final_obs, obs_stride, d_action,
                       d_reward, d_terminated, d_truncated);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class L> int q_act(L *t, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (N < 0 || obs_stride < t->cfg.n_obs) return fail(STMPC_EINVAL, "N negative, or obs_stride shorter than the observation");
    if (!(eps >= 0 && eps <= 1)) return fail(STMPC_EINVAL, "eps must be in 0 ... 1");
    if (N == 0) return STMPC_OK;
    if (!d_obs || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(t->rp.device));
    L::Head::act(*t, N, d_obs, obs_stride, eps, d_action, d_debug_q, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class L> int q_update(L *t, int n_updates, double lr, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (n_updates < 0 || !(lr >= 0)) return fail(STMPC_EINVAL, "n_updates or the learning rate is negative");
    HIPCHK(hipSetDevice(t->rp.device));
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // three launches, five with prioritised replay, whatever the counters say
        per_launch_sample(t->rp, t->base(), 1, st);
        if (L::Head::noisy(*t)) { L::Head::noisy_update(*t, (float)lr, st); continue; }      // (four launches, six with prioritised replay)
        L::Head::fwd(*t, 1, st);
        L::Head::wgrad(*t, 1, st);
        per_launch_update(t->rp, t->base(), st);
        L::Head::adam(*t, (float)lr, 0, st);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class L> int q_grads(L *t, float *d_grad, void *stream) {
    if (!t || !d_grad) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->rp.device));
    hipStream_t st = (hipStream_t)stream;
    per_launch_sample(t->rp, t->base(), 0, st);
    if (L::Head::noisy(*t)) L::Head::noisy_grads(*t, st);            // (the gradient with respect to the effective parameters: mu's)
    else {
        L::Head::fwd(*t, 0, st);
        L::Head::wgrad(*t, 0, st);
    }
    L::Head::unpad(*t, d_grad, st);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class L> int q_gather(L *t, float *d_rows, void *stream) {
    if (!t || !d_rows) return fail(STMPC_EINVAL, "NULL argument");
    return replay_gather(t->rp, t->base(), d_rows, stream);
}

template <class L> int q_stats(L *t, double *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->rp.device));
    L::Head::stats(*t, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class L> int q_per_enable(L *t, const stmpc_per_cfg *g) {
    if (!t || !g) return fail(STMPC_EINVAL, "NULL argument");
    TRY(per_check_cfg(g));
    if (t->pop_member)
        return fail(STMPC_EINVAL, std::string("this learner is a member of a population: prioritised replay is enabled on the population (") + L::Head::pop_per_enable + ")");
    TRY(t->rp.check_empty());
    return per_attach(t->rp, t->base(), nullptr, g);                 // (the tree, idx, aw, atd and the constants into base())
}

template <class L> int q_nstep_enable(L *t, const stmpc_nstep_cfg *g) {
    if (!t || !g) return fail(STMPC_EINVAL, "NULL argument");
    if (t->pop_member) return fail(STMPC_EINVAL, std::string("this learner is a member of a population: n_step is set on the population (") + L::Head::pop_nstep_enable + ")");
    return nstep_attach(t->rp, t->base(), g);
}

// (a lone learner's ring, or a borrowed member's)
template <class L> int q_nstep_window(L *t, const int64_t *idx, int n_idx, double *out) {
    if (!t) return fail(STMPC_EINVAL, "NULL argument");
    return nstep_window_read(t->rp, t->base(), idx, n_idx, out);
}

template <class L> int q_replay_read(L *t, int64_t first, int64_t count, float *rows) {
    if (!t) return fail(STMPC_EINVAL, "NULL argument");
    return t->rp.read_rows(first, count, rows);
}

template <class L> int q_per_tree_read(L *t, int64_t first, int64_t count, double *nodes) {
    if (!t) return fail(STMPC_EINVAL, "NULL argument");
    return t->rp.read_tree(first, count, nodes);
}

template <class L> int q_per_last(L *t, int64_t *d_idx, float *d_td, float *d_weight, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "NULL argument");
    return per_last(t->rp, t->base(), d_idx, d_td, d_weight, stream);
}

template <class L> int q_padded_read(L *t, int slot, float *values, int64_t count) {
    if (!t || !values || slot < 0 || slot > STMPC_DQN_GRAD) return fail(STMPC_EINVAL, "NULL argument or slot out of range");
    if (count != dq_nparam(t->h1p, t->Ap)) return fail(STMPC_EINVAL, "count is not the length of a padded slot");
    return read_back(t->rp.device, values, slot == STMPC_DQN_GRAD ? t->base().q.g : net_slot(t->base().q, slot), (size_t)count * sizeof(float));
}
}  // namespace

extern "C" {

int stmpc_dqn_create(stmpc_ctx *c, const stmpc_dqn_cfg *g, stmpc_dqn **out) { return q_create(c, g, out); }
void stmpc_dqn_destroy(stmpc_dqn *t) { q_destroy(t); }
int stmpc_dqn_set_params(stmpc_dqn *t, int slot, const float *values, int64_t count) { return q_set_params(t, slot, values, count); }
int stmpc_dqn_get_params(stmpc_dqn *t, int slot, float *values, int64_t count) { return q_get_params(t, slot, values, count); }
int stmpc_dqn_set_state(stmpc_dqn *t, const int64_t *counters, const float *beta_pow) { return q_set_state(t, counters, beta_pow); }
int stmpc_dqn_get_state(stmpc_dqn *t, int64_t *counters, float *beta_pow) { return q_get_state(t, counters, beta_pow); }
int stmpc_dqn_push_device(stmpc_dqn *t, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_action,
                          const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    return q_push(t, N, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated, d_truncated, stream);
}
int stmpc_dqn_act_device(stmpc_dqn *t, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream) {
    return q_act(t, N, d_obs, obs_stride, eps, d_action, d_debug_q, stream);
}
int stmpc_dqn_update_device(stmpc_dqn *t, int n_updates, double lr, void *stream) { return q_update(t, n_updates, lr, stream); }
int stmpc_dqn_grads_device(stmpc_dqn *t, float *d_grad, void *stream) { return q_grads(t, d_grad, stream); }
int stmpc_dqn_gather_device(stmpc_dqn *t, float *d_rows, void *stream) { return q_gather(t, d_rows, stream); }
int stmpc_dqn_stats_device(stmpc_dqn *t, double *d_out, void *stream) { return q_stats(t, d_out, stream); }
int stmpc_dqn_per_enable(stmpc_dqn *t, const stmpc_per_cfg *g) { return q_per_enable(t, g); }
int stmpc_nstep_enable_dqn(stmpc_dqn *t, const stmpc_nstep_cfg *g) { return q_nstep_enable(t, g); }
int stmpc_nstep_window_dqn(stmpc_dqn *t, const int64_t *idx, int n_idx, double *out) { return q_nstep_window(t, idx, n_idx, out); }
int stmpc_dqn_per_tree_read(stmpc_dqn *t, int64_t first, int64_t count, double *nodes) { return q_per_tree_read(t, first, count, nodes); }
int stmpc_dqn_per_last_device(stmpc_dqn *t, int64_t *d_idx, float *d_td, float *d_weight, void *stream) { return q_per_last(t, d_idx, d_td, d_weight, stream); }
int stmpc_dqn_padded_read(stmpc_dqn *t, int slot, float *values, int64_t count) { return q_padded_read(t, slot, values, count); }

// dbg: float32 [batch][4]
int stmpc_dqn_targets_device(stmpc_dqn *t, float *d_out, void *stream) {
    if (!t || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->rp.device));
    per_launch_sample(t->rp, t->base(), 0, (hipStream_t)stream);
    hipLaunchKernelGGL(k_dqn_fwd, dim3(t->grid.tiles), dim3(AT_THREADS), t->lds, (hipStream_t)stream, t->dev, t->cfg.batch, 0, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_c51_create(stmpc_ctx *c, const stmpc_c51_cfg *g, stmpc_c51 **out) { return q_create(c, g, out); }
void stmpc_c51_destroy(stmpc_c51 *t) { q_destroy(t); }
int stmpc_c51_set_params(stmpc_c51 *t, int slot, const float *values, int64_t count) { return q_set_params(t, slot, values, count); }
int stmpc_c51_get_params(stmpc_c51 *t, int slot, float *values, int64_t count) { return q_get_params(t, slot, values, count); }
int stmpc_c51_set_state(stmpc_c51 *t, const int64_t *counters, const float *beta_pow) {
    // a noisy learner's acting-draw counter travels in the counters' slot C51_NOISY_DRAWS (get_state reads all of them); checked before anything is written
    if (t && counters && t->ex.on && counters[C51_NOISY_DRAWS] < 0) return fail(STMPC_EINVAL, "counters out of range");
    TRY(q_set_state(t, counters, beta_pow));
    if (!t->ex.on) return STMPC_OK;
    const long long draws = counters[C51_NOISY_DRAWS];
    HIPCHK(hipMemcpy(t->rp.cnt.as<long long>() + C51_NOISY_DRAWS, &draws, sizeof draws, hipMemcpyHostToDevice));
    return STMPC_OK;
}
int stmpc_c51_get_state(stmpc_c51 *t, int64_t *counters, float *beta_pow) { return q_get_state(t, counters, beta_pow); }
int stmpc_c51_push_device(stmpc_c51 *t, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride, const int32_t *d_action,
                          const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    return q_push(t, N, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated, d_truncated, stream);
}
int stmpc_c51_act_device(stmpc_c51 *t, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream) {
    return q_act(t, N, d_obs, obs_stride, eps, d_action, d_debug_q, stream);
}
int stmpc_c51_update_device(stmpc_c51 *t, int n_updates, double lr, void *stream) { return q_update(t, n_updates, lr, stream); }
int stmpc_c51_grads_device(stmpc_c51 *t, float *d_grad, void *stream) { return q_grads(t, d_grad, stream); }
int stmpc_c51_gather_device(stmpc_c51 *t, float *d_rows, void *stream) { return q_gather(t, d_rows, stream); }
int stmpc_c51_stats_device(stmpc_c51 *t, double *d_out, void *stream) { return q_stats(t, d_out, stream); }
int stmpc_c51_per_enable(stmpc_c51 *t, const stmpc_per_cfg *g) { return q_per_enable(t, g); }
int stmpc_c51_multi_step_enable(stmpc_c51 *t, const stmpc_nstep_cfg *g) { return q_nstep_enable(t, g); }
int stmpc_c51_per_tree_read(stmpc_c51 *t, int64_t first, int64_t count, double *nodes) { return q_per_tree_read(t, first, count, nodes); }
int stmpc_c51_per_last_device(stmpc_c51 *t, int64_t *d_idx, float *d_td, float *d_weight, void *stream) { return q_per_last(t, d_idx, d_td, d_weight, stream); }
int stmpc_c51_padded_read(stmpc_c51 *t, int slot, float *values, int64_t count) { return q_padded_read(t, slot, values, count); }
int stmpc_c51_replay_read(stmpc_c51 *t, int64_t first, int64_t count, float *rows) { return q_replay_read(t, first, count, rows); }

int stmpc_c51_targets_device(stmpc_c51 *t, float *d_out, void *stream) { return stmpc_c51_dist_device(t, nullptr, d_out, stream); }

// d_dist: float32 [batch][2][K], d_out: float32 [batch][4]; either may be null
int stmpc_c51_dist_device(stmpc_c51 *t, float *d_dist, float *d_out, void *stream) {
    if (!t || (!d_dist && !d_out)) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(t->rp.device));
    per_launch_sample(t->rp, t->base(), 0, (hipStream_t)stream);
    C51Head::fwd_launch(*t, 0, d_out, d_dist, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_c51_project_device(stmpc_c51 *t, int n, const float *d_p, const float *d_reward, const float *d_mask, const float *d_disc, float *d_m, void *stream) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (n < 0) return fail(STMPC_EINVAL, "n is negative");
    if (n == 0) return STMPC_OK;
    if (!d_p || !d_reward || !d_mask || !d_disc || !d_m) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(t->rp.device));
    hipLaunchKernelGGL(k_c51_project, dim3((n + AT_TM - 1) / AT_TM), dim3(AT_THREADS), 0, (hipStream_t)stream, t->dev, n, d_p, d_reward, d_mask, d_disc, d_m);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_c51_dzout_read(stmpc_c51 *t, float *values, int64_t count) {
    if (!t || !values) return fail(STMPC_EINVAL, "NULL argument");
    if (count != (int64_t)t->rp.Bp * t->Ap) return fail(STMPC_EINVAL, "count is not batch rounded up to 16 times the padded logit count");
    return read_back(t->rp.device, values, t->base().aD2, (size_t)count * sizeof(float));
}

}  // extern "C"

// ---- the noisy output layer of a C51 learner (stmpc_noisy_c51_*; kernels in stmpc_c51_noisy_kernels.hpp) -------------------------------------------
namespace {
// a sigma slot between the C-ABI's layout (W1-shaped [n_out][h1] | [n_out]) and the padded one ([Ap][h1p] | [Ap])
std::vector<Seg> noisy_layout(const stmpc_c51 *t) {
    return {{C51Head::n_out(t->cfg), t->cfg.h1, 0, (size_t)t->h1p}, {1, C51Head::n_out(t->cfg), (size_t)t->Ap * t->h1p, 0}};
}
size_t noisy_len(const stmpc_c51 *t) { return (size_t)t->Ap * t->h1p + t->Ap; }
float *noisy_slot(const C51Noisy &z, int slot) { float *const p[4] = {z.dev.sig, z.dev.sigt, z.dev.sm, z.dev.sv}; return p[slot]; }
int noisy_check(const stmpc_c51 *t) {
    if (!t) return fail(STMPC_EINVAL, "learner is NULL");
    if (!t->ex.on) return fail(STMPC_EINVAL, "the noisy output layer is not enabled on this learner (stmpc_noisy_c51_enable)");
    return STMPC_OK;
}
}  // namespace

extern "C" {

// the checks of a stmpc_noisy_cfg and of the learner it goes onto (fresh; synchronises), then the buffers and sigma's start
static int noisy_attach(stmpc_c51 *t, const stmpc_noisy_cfg *g) {
    if (!(g->sigma0 >= 0) || !std::isfinite(g->sigma0)) return fail(STMPC_EINVAL, "sigma0 must be finite and not negative");
    if (t->ex.on) return fail(STMPC_EINVAL, "the noisy output layer is already enabled on this learner");
    long long cn[DG_NCNT];
    TRY(read_back(t->rp.device, cn, t->rp.cnt.p, sizeof cn));
    if (cn[DG_FILL] != 0 || cn[DG_CURSOR] != 0 || cn[DG_FRAMES] != 0 || cn[DG_UPDATES] != 0)
        return fail(STMPC_EINVAL, "the noisy output layer can be enabled on a fresh learner only (fill is " + std::to_string(cn[DG_FILL]) + ", updates " +
                                      std::to_string(cn[DG_UPDATES]) + ")");
    C51Noisy &z = t->ex;
    const size_t ns = noisy_len(t), nf = (size_t)C51_NZ_SETS * (t->h1p + t->Ap);
    TRY(ddpg_zero(z.sig, ns * sizeof(float)));
    TRY(ddpg_zero(z.sigt, ns * sizeof(float)));
    TRY(ddpg_zero(z.sm, ns * sizeof(float)));
    TRY(ddpg_zero(z.sv, ns * sizeof(float)));
    TRY(ddpg_zero(z.f, nf * sizeof(float)));
    for (int s = 0; s < C51_NZ_SETS; ++s) {
        TRY(ddpg_zero(z.we[s], (size_t)t->np * sizeof(float)));
        TRY(ddpg_zero(z.pe[s], (size_t)t->Ap * t->h1p * sizeof(float)));
    }
    z.dev.sig = z.sig.as<float>(); z.dev.sigt = z.sigt.as<float>(); z.dev.sm = z.sm.as<float>(); z.dev.sv = z.sv.as<float>(); z.dev.f = z.f.as<float>();
    z.dev.we0 = z.we[0].as<float>(); z.dev.we1 = z.we[1].as<float>(); z.dev.we2 = z.we[2].as<float>();
    z.dev.pe0 = z.pe[0].as<float>(); z.dev.pe1 = z.pe[1].as<float>(); z.dev.pe2 = z.pe[2].as<float>();
    // sigma = sigma0 / sqrt(h1) everywhere, the target's too (float32 of the fp64 quotient); pad rows and columns stay zero
    std::vector<float> flat((size_t)C51Head::n_out(t->cfg) * (t->cfg.h1 + 1), (float)(g->sigma0 / std::sqrt((double)t->cfg.h1))), pad(ns, 0.f);
    slot_move(noisy_layout(t), flat.data(), pad.data(), true);
    HIPCHK(hipMemcpy(z.dev.sig, pad.data(), ns * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(z.dev.sigt, pad.data(), ns * sizeof(float), hipMemcpyHostToDevice));
    z.sigma0 = g->sigma0;
    z.on = true;
    return STMPC_OK;
}

int stmpc_noisy_c51_enable(stmpc_c51 *t, const stmpc_noisy_cfg *g) {
    if (!t || !g) return fail(STMPC_EINVAL, "NULL argument");
    if (t->pop_member)
        return fail(STMPC_EINVAL, "this learner is a member of a population: the noisy output layer is enabled on the population (stmpc_pop_noisy_c51_enable)");
    return noisy_attach(t, g);
}

int stmpc_noisy_c51_set_params(stmpc_c51 *t, int slot, const float *values, int64_t count) {
    TRY(noisy_check(t));
    TRY(slot_args(t, values, slot, 4));
    return slot_set(t->rp.device, noisy_layout(t), noisy_len(t), noisy_slot(t->ex, slot), values, count, false, [] {});
}

int stmpc_noisy_c51_get_params(stmpc_c51 *t, int slot, float *values, int64_t count) {
    TRY(noisy_check(t));
    TRY(slot_args(t, values, slot, 4));
    return slot_get(t->rp.device, noisy_layout(t), noisy_len(t), noisy_slot(t->ex, slot), values, count);
}

int stmpc_noisy_c51_act_device(stmpc_c51 *t, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream) {
    TRY(noisy_check(t));
    if (N < 0 || obs_stride < t->cfg.n_obs) return fail(STMPC_EINVAL, "N negative, or obs_stride shorter than the observation");
    if (!(eps >= 0 && eps <= 1)) return fail(STMPC_EINVAL, "eps must be in 0 ... 1");
    if (N == 0) return STMPC_OK;
    if (!d_obs || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(t->rp.device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_c51_noisy_compose, dim3(C51Head::compose_blocks(*t)), dim3(256), 0, st, t->dev, t->ex.dev, 1, 0);
    hipLaunchKernelGGL(k_c51_act, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), t->lds, st, t->ex.shadow(t->dev, true), N, d_obs, obs_stride, (float)eps,
                       eps > 0 ? 1 : 0, d_action, d_debug_q);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

int stmpc_noisy_c51_debug_read(stmpc_c51 *t, int what, float *out, int64_t count) {
    TRY(noisy_check(t));
    if (!out || what < 0 || what >= 3 * C51_NZ_SETS) return fail(STMPC_EINVAL, "NULL argument, or no such quantity");
    const int set = what % C51_NZ_SETS, h1 = t->cfg.h1, W = C51Head::n_out(t->cfg);
    const size_t ns = noisy_len(t);
    if (what < STMPC_NOISY_WEFF_ONLINE) {                            // f(e_in) [h1] | f(e_out) [n_out]
        if (count != (int64_t)h1 + W) return fail(STMPC_EINVAL, "count is not h1 + the output rows");
        std::vector<float> pad((size_t)t->h1p + t->Ap);
        TRY(read_back(t->rp.device, pad.data(), t->ex.dev.f + (size_t)set * pad.size(), pad.size() * sizeof(float)));
        memcpy(out, pad.data(), h1 * sizeof(float));
        memcpy(out + h1, pad.data() + t->h1p, W * sizeof(float));
        return STMPC_OK;
    }
    const float *we = t->ex.we[set].as<float>() + dg_o_w1(t->h1p);    // (W1 | b1 are contiguous in the parameter layout)
    if (what >= STMPC_NOISY_WEFF_PADDED_ONLINE) {
        if (count != (int64_t)ns) return fail(STMPC_EINVAL, "count is not the length of the padded W1 | b1");
        return read_back(t->rp.device, out, we, ns * sizeof(float));
    }
    return slot_get(t->rp.device, noisy_layout(t), ns, we, out, count);
}

}  // extern "C"

// ---- populations of discrete learners (stmpc_pop_dqn_*, stmpc_pop_c51_*): P learners of the section above, one launch per kernel, written once for
// both heads; kernels in stmpc_dqn_pop_kernels.hpp and stmpc_c51_pop_kernels.hpp, prioritised replay and the statistics on the core's DdpgDev table
// with stmpc_per_pop_kernels.hpp's and stmpc_ddpg_pop_kernels.hpp's kernels -------------------------------------------------------------------------
template <class L> struct QPop {
    using Member = L;
    using Head = typename L::Head;
    using Dev = typename Head::Dev;
    PopCore core;                         // core.table: the members' base()
    std::vector<L *> members;               // owned; made by q_create, so every lone entry works on a borrowed member
    DevBuf table;                           // Dev [P]: the members' structs (q_pop_upload); a C51 member's v_min, v_max and dz travel in its own
    const Dev *dev() const { return table.as<Dev>(); }
    // one update's launches behind the sampling step, where the population has a sequence of its own (a noisy C51 population): false -- none
    bool own_update(const Grid &, int, int, const DdpgLr &, hipStream_t) const { return false; }
};
struct stmpc_dqn_pop : QPop<stmpc_dqn> {};
// (noisy: stmpc_pop_noisy_c51_enable ran -- every member's C51Noisy is on, and three more tables follow the members: their noise structs and their
// shadow structs for learning and for acting)
struct stmpc_c51_pop : QPop<stmpc_c51> {
    bool noisy = false;
    DevBuf ztab, shadow, shadow_act;
    int noisy_upload() {
        std::vector<C51NoisyDev> z;
        std::vector<C51Dev> s, a;
        for (const stmpc_c51 *t : members) { z.push_back(t->ex.dev); s.push_back(t->ex.shadow(t->dev, false)); a.push_back(t->ex.shadow(t->dev, true)); }
        TRY(upload(ztab, z.data(), z.size()));
        TRY(upload(shadow, s.data(), s.size()));
        return upload(shadow_act, a.data(), a.size());
    }
    // compose, fwd, wgrad, (the priority update,) sigma's and mu's Adam, each over the members: C51Head::noisy_update's launches
    bool own_update(const Grid &g, int B, int Bp, const DdpgLr &lrs, hipStream_t st) const {
        if (!noisy) return false;
        const stmpc_c51 *t = members[0];
        const int P = core.P();
        hipLaunchKernelGGL(k_c51_noisy_compose_pop, dim3(C51Head::compose_blocks(*t), P), dim3(256), 0, st, dev(), ztab.as<C51NoisyDev>(), 0, 1);
        C51Head::fwd_pop(*t, shadow.as<C51Dev>(), g, P, core.lds, B, st);
        C51Head::wgrad_pop(shadow.as<C51Dev>(), g, P, Bp, st);
        if (core.per_any) hipLaunchKernelGGL(k_per_update_pop, dim3(1, P), dim3(PER_THREADS), 0, st, core.dev(), B, 1);
        hipLaunchKernelGGL(k_c51_noisy_adam_pop, dim3(g.ablocks, P), dim3(256), 0, st, dev(), ztab.as<C51NoisyDev>(), lrs, 1);
        return true;
    }
};

static_assert(STMPC_DQN_POP_MAX == DG_POP_MAX && DG_POP_MAX <= 64, "DdpgLr and DqnEps hold one value, and DqnEps::explore one bit, per possible member");
static_assert(STMPC_C51_POP_MAX == DG_POP_MAX && DG_POP_MAX <= 64, "DdpgLr and DqnEps hold one value, and DqnEps::explore one bit, per possible member");

namespace {
// both device tables from the members as they are now: at create, and again once prioritised replay or n_step re-wired members
// (Pop: stmpc_dqn_pop or stmpc_c51_pop)
template <class Pop> int q_pop_upload(Pop *p) {
    std::vector<typename Pop::Dev> host;
    for (const typename Pop::Member *t : p->members) host.push_back(t->dev);
    TRY(upload(p->table, host.data(), host.size()));
    return pop_upload(p->core);
}

template <class Pop> void q_pop_destroy(Pop *p) {
    if (!p) return;
    for (typename Pop::Member *t : p->members) q_destroy(t);
    (void)hipSetDevice(p->core.device);
    delete p;
}

template <class Pop> int q_pop_create(stmpc_ctx *c, const typename Pop::Head::Cfg *cfgs, int P, Pop **out) {
    using H = typename Pop::Head;
    TRY(pop_check_create(c, cfgs, P, out, H::shared, H::same_shape));
    HIPCHK(hipSetDevice(c->device));
    Pop *p = new Pop();
    PopCore &core = p->core;
    core.device = c->device;
    int rc = STMPC_OK;
    for (int m = 0; m < P && !rc; ++m) {
        typename Pop::Member *t = nullptr;
        rc = q_create(c, cfgs + m, &t);
        if (rc) break;
        t->pop_member = true;
        p->members.push_back(t);
    }
    if (!rc) {
        for (typename Pop::Member *t : p->members) core.slots.push_back({&t->rp, &t->base(), nullptr});     // (members is complete: the pointers stay)
        const typename Pop::Member *t0 = p->members[0];
        core.n_obs = t0->cfg.n_obs; core.capacity = t0->cfg.capacity; core.batch = t0->cfg.batch; core.lds = t0->lds;
        rc = q_pop_upload(p);
    }
    if (!rc) rc = H::raise_lds(true, c->device, core.lds);
    if (rc) { q_pop_destroy(p); return rc; }
    *out = p;
    return STMPC_OK;
}

template <class Pop> typename Pop::Member *q_pop_member(Pop *p, int m) {
    if (!p || m < 0 || m >= p->core.P()) { (void)fail(STMPC_EINVAL, "population is NULL, or no such member"); return nullptr; }
    return p->members[m];
}

template <class Pop> int q_pop_act(Pop *p, int n_per_member, const float *d_obs, int obs_stride, const double *eps, int n_eps, int32_t *d_action, float *d_debug_q,
                                   void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    const PopCore &c = p->core;
    TRY(pop_check_rows(c, n_per_member, obs_stride));
    if (!eps) return fail(STMPC_EINVAL, "NULL argument");
    if (n_eps != c.P()) return fail(STMPC_EINVAL, "the eps array has " + std::to_string(n_eps) + " entries, the population " + std::to_string(c.P()) + " members");
    DqnEps e{};
    for (int m = 0; m < c.P(); ++m) {
        if (!(eps[m] >= 0 && eps[m] <= 1)) return fail(STMPC_EINVAL, "member " + std::to_string(m) + "'s eps must be in 0 ... 1");
        e.eps[m] = (float)eps[m];
        if (eps[m] > 0) e.explore |= 1ull << m;                      // (q_act's rule: an exploring call is one with eps > 0)
    }
    if (!d_obs || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(c.device));
    Pop::Head::act_pop(p->dev(), c.P(), c.lds, n_per_member, d_obs, obs_stride, e, d_action, d_debug_q, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class Pop> int q_pop_push(Pop *p, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                                    const int32_t *d_action, const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    const PopCore &c = p->core;
    TRY(pop_check_rows(c, n_per_member, obs_stride));
    TRY(pop_check_push(c, n_per_member));
    if (!d_obs || !d_next_obs || !d_action || !d_reward || !d_terminated || !d_truncated) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(c.device));
    Pop::Head::push_pop(p->dev(), c.P(), n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated, d_truncated, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class Pop> int q_pop_update(Pop *p, int n_updates, const double *lr, int n_lr, void *stream) {
    using H = typename Pop::Head;
    if (!p) return fail(STMPC_EINVAL, "NULL argument");
    const PopCore &c = p->core;
    DdpgLr lrs{};
    TRY(pop_check_update(c, n_updates, n_lr, {{lr, &lrs}}));
    HIPCHK(hipSetDevice(c.device));
    const typename Pop::Member *t = p->members[0];
    const Grid g = t->grid;
    const int P = c.P(), B = c.batch, Bp = t->rp.Bp;
    hipStream_t st = (hipStream_t)stream;
    for (int u = 0; u < n_updates; ++u) {                            // q_update's three launches (five with prioritised members), each over the members
        if (c.per_any) hipLaunchKernelGGL(k_per_sample_pop, dim3(1, P), dim3(PER_THREADS), 0, st, c.dev(), B, Bp, 1);
        if (p->own_update(g, B, Bp, lrs, st)) continue;              // (a noisy C51 population: four launches, six with prioritised members)
        H::fwd_pop(*t, p->dev(), g, P, c.lds, B, st);
        H::wgrad_pop(p->dev(), g, P, Bp, st);
        if (c.per_any) hipLaunchKernelGGL(k_per_update_pop, dim3(1, P), dim3(PER_THREADS), 0, st, c.dev(), B, 1);
        H::adam_pop(p->dev(), g, P, lrs, st);
    }
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class Pop> int q_pop_stats(Pop *p, double *d_out, void *stream) {
    if (!p || !d_out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->core.device));
    hipLaunchKernelGGL(k_ddpg_stats_pop, dim3(1, p->core.P()), dim3(64), 0, (hipStream_t)stream, p->core.dev(), p->core.batch, d_out);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

template <class Pop> int q_pop_per_enable(Pop *p, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_per_enable(p->core, cfgs, enabled, P, [&] { return q_pop_upload(p); });
}

template <class Pop> int q_pop_nstep_enable(Pop *p, const stmpc_nstep_cfg *cfgs, int P) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    return pop_nstep_enable(p->core, cfgs, P, [&] { return q_pop_upload(p); });
}
}  // namespace

extern "C" {

int stmpc_pop_dqn_create(stmpc_ctx *c, const stmpc_dqn_cfg *cfgs, int P, stmpc_dqn_pop **out) { return q_pop_create(c, cfgs, P, out); }
void stmpc_pop_dqn_destroy(stmpc_dqn_pop *p) { q_pop_destroy(p); }
int stmpc_pop_dqn_size(const stmpc_dqn_pop *p) { return p ? p->core.P() : 0; }
stmpc_dqn *stmpc_pop_dqn_member(stmpc_dqn_pop *p, int m) { return q_pop_member(p, m); }
int stmpc_pop_dqn_act_device(stmpc_dqn_pop *p, int n_per_member, const float *d_obs, int obs_stride, const double *eps, int n_eps, int32_t *d_action,
                             float *d_debug_q, void *stream) {
    return q_pop_act(p, n_per_member, d_obs, obs_stride, eps, n_eps, d_action, d_debug_q, stream);
}
int stmpc_pop_dqn_push_device(stmpc_dqn_pop *p, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                              const int32_t *d_action, const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    return q_pop_push(p, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated, d_truncated, stream);
}
int stmpc_pop_dqn_update_device(stmpc_dqn_pop *p, int n_updates, const double *lr, int n_lr, void *stream) { return q_pop_update(p, n_updates, lr, n_lr, stream); }
int stmpc_pop_dqn_stats_device(stmpc_dqn_pop *p, double *d_out, void *stream) { return q_pop_stats(p, d_out, stream); }
int stmpc_pop_dqn_per_enable(stmpc_dqn_pop *p, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) { return q_pop_per_enable(p, cfgs, enabled, P); }
int stmpc_pop_nstep_enable_dqn(stmpc_dqn_pop *p, const stmpc_nstep_cfg *cfgs, int P) { return q_pop_nstep_enable(p, cfgs, P); }
int stmpc_pop_dqn_replay_read(stmpc_dqn *t, int64_t first, int64_t count, float *rows) { return q_replay_read(t, first, count, rows); }

int stmpc_pop_c51_create(stmpc_ctx *c, const stmpc_c51_cfg *cfgs, int P, stmpc_c51_pop **out) { return q_pop_create(c, cfgs, P, out); }
void stmpc_pop_c51_destroy(stmpc_c51_pop *p) { q_pop_destroy(p); }
int stmpc_pop_c51_size(const stmpc_c51_pop *p) { return p ? p->core.P() : 0; }
stmpc_c51 *stmpc_pop_c51_member(stmpc_c51_pop *p, int m) { return q_pop_member(p, m); }
int stmpc_pop_c51_act_device(stmpc_c51_pop *p, int n_per_member, const float *d_obs, int obs_stride, const double *eps, int n_eps, int32_t *d_action,
                             float *d_debug_q, void *stream) {
    return q_pop_act(p, n_per_member, d_obs, obs_stride, eps, n_eps, d_action, d_debug_q, stream);
}
int stmpc_pop_c51_push_device(stmpc_c51_pop *p, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                              const int32_t *d_action, const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream) {
    return q_pop_push(p, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated, d_truncated, stream);
}
int stmpc_pop_c51_update_device(stmpc_c51_pop *p, int n_updates, const double *lr, int n_lr, void *stream) { return q_pop_update(p, n_updates, lr, n_lr, stream); }
int stmpc_pop_c51_stats_device(stmpc_c51_pop *p, double *d_out, void *stream) { return q_pop_stats(p, d_out, stream); }
// (both re-wire the members' structs: a noisy population's shadow tables follow)
int stmpc_pop_c51_per_enable(stmpc_c51_pop *p, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P) {
    TRY(q_pop_per_enable(p, cfgs, enabled, P));
    return p->noisy ? p->noisy_upload() : STMPC_OK;
}
int stmpc_pop_c51_multi_step_enable(stmpc_c51_pop *p, const stmpc_nstep_cfg *cfgs, int P) {
    TRY(q_pop_nstep_enable(p, cfgs, P));
    return p->noisy ? p->noisy_upload() : STMPC_OK;
}
int stmpc_pop_c51_replay_read(stmpc_c51 *t, int64_t first, int64_t count, float *rows) { return q_replay_read(t, first, count, rows); }
int stmpc_pop_c51_multi_step_window(stmpc_c51 *t, const int64_t *idx, int n_idx, double *out) { return q_nstep_window(t, idx, n_idx, out); }

// ---- the noisy output layer of a population of C51 learners (stmpc_pop_noisy_c51_*) ----
// one call on fresh members: all of them get the layer, member m with cfgs[m]'s sigma0
int stmpc_pop_noisy_c51_enable(stmpc_c51_pop *p, const stmpc_noisy_cfg *cfgs, int P) {
    if (!p || !cfgs) return fail(STMPC_EINVAL, "NULL argument");
    if (P != p->core.P()) return fail(STMPC_EINVAL, "the cfg array has " + std::to_string(P) + " entries, the population " + std::to_string(p->core.P()) + " members");
    if (p->noisy) return fail(STMPC_EINVAL, "the noisy output layer is already enabled on this population");
    for (int m = 0; m < P; ++m)
        if (!(cfgs[m].sigma0 >= 0) || !std::isfinite(cfgs[m].sigma0)) return fail(STMPC_EINVAL, "member " + std::to_string(m) + "'s sigma0 must be finite and not negative");
    HIPCHK(hipSetDevice(p->core.device));
    for (int m = 0; m < P; ++m) TRY(noisy_attach(p->members[m], cfgs + m));
    TRY(p->noisy_upload());
    p->noisy = true;
    return STMPC_OK;
}

// stmpc_noisy_c51_act_device per member: every member takes an acting draw of its own, then stmpc_pop_c51_act_device's launch on the shadow structs
int stmpc_pop_noisy_c51_act_device(stmpc_c51_pop *p, int n_per_member, const float *d_obs, int obs_stride, const double *eps, int n_eps, int32_t *d_action,
                                   float *d_debug_q, void *stream) {
    if (!p) return fail(STMPC_EINVAL, "population is NULL");
    if (!p->noisy) return fail(STMPC_EINVAL, "the noisy output layer is not enabled on this population (stmpc_pop_noisy_c51_enable)");
    const PopCore &c = p->core;
    TRY(pop_check_rows(c, n_per_member, obs_stride));
    if (!eps) return fail(STMPC_EINVAL, "NULL argument");
    if (n_eps != c.P()) return fail(STMPC_EINVAL, "the eps array has " + std::to_string(n_eps) + " entries, the population " + std::to_string(c.P()) + " members");
    DqnEps e{};
    for (int m = 0; m < c.P(); ++m) {
        if (!(eps[m] >= 0 && eps[m] <= 1)) return fail(STMPC_EINVAL, "member " + std::to_string(m) + "'s eps must be in 0 ... 1");
        e.eps[m] = (float)eps[m];
        if (eps[m] > 0) e.explore |= 1ull << m;
    }
    if (!d_obs || !d_action) return fail(STMPC_EINVAL, "NULL device pointer");
    HIPCHK(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_c51_noisy_compose_pop, dim3(C51Head::compose_blocks(*p->members[0]), c.P()), dim3(256), 0, st, p->dev(), p->ztab.as<C51NoisyDev>(), 1, 0);
    C51Head::act_pop(p->shadow_act.as<C51Dev>(), c.P(), c.lds, n_per_member, d_obs, obs_stride, e, d_action, d_debug_q, st);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}


}  // extern "C"

// ---- a Q-network as a policy (stmpc_qactor_*): DQNAgent.get_control for N states in one launch; kernel in stmpc_qactor_kernels.hpp ------------------
struct stmpc_qactor {
    int device = 0;
    const stmpc_dqn *learner = nullptr;     // a view (stmpc_qactor_view_dqn): the network is the learner's, read through its struct at every evaluation
    const stmpc_c51 *c51 = nullptr;         // a view of a categorical learner (stmpc_c51actor_view): likewise, through its C51Dev
    bool categorical = false;             // a categorical head (stmpc_c51actor_create / _view): k_c51actor_eval evaluates it; `dev`'s output width is A * K,
                                            // (A + 1) * K of a created dueling one (stmpc_dueling_c51actor_create)
    int dueling = 0;
    int K = 0;                              // a created categorical actor's head: atoms and support (a view reads its learner's)
    double v_min = 0, v_max = 0, dz = 0;
    int target = 0, mode = 0, n_in = 0, A = 0;
    bool limits = false;                    // stmpc_qactor_set_limits was called
    double tick = 0, jerk_min = 0, jerk_max = 0;
    DqnDev dev{};                           // a created actor: base.q (its own network), the shape and the counters ddpg_repack's kernel reads
    DevBuf net[11], cnt, table;             // (net, cnt: empty for a view)
    std::vector<double> table_h;            // the host's copy of `table` (qshield_policy_check compares it with an env's)
    size_t lds = 0;
};

namespace {
int qactor_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling;
    return raise_dynamic_lds((const void *)k_qactor_eval, "k_qactor_eval", ceiling, device, lds);
}
int c51actor_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling;
    return raise_dynamic_lds((const void *)k_c51actor_eval, "k_c51actor_eval", ceiling, device, lds);
}
// the struct k_c51actor_eval gets for a categorical actor
C51Dev c51actor_dev(const stmpc_qactor *q) {
    if (q->c51) return q->c51->dev;
    C51Dev D{};
    D.dq = q->dev; D.K = q->K; D.dueling = q->dueling; D.v_min = q->v_min; D.v_max = q->v_max; D.dz = q->dz;
    return D;
}
// what create and view share: the mode, the table (checked, then uploaded into q), the kernel's dynamic LDS
int qactor_check_table(const double *action_values, int n_actions, int A, int mode) {
    if (mode != STMPC_QACTOR_JERK && mode != STMPC_QACTOR_ACCELERATION) return fail(STMPC_EINVAL, "mode must be STMPC_QACTOR_JERK or STMPC_QACTOR_ACCELERATION");
    if (n_actions != A) return fail(STMPC_EINVAL, "the action table has " + std::to_string(n_actions) + " entries, the network " + std::to_string(A) + " actions");
    for (int i = 0; i < A; ++i)
        if (!std::isfinite(action_values[i])) return fail(STMPC_EINVAL, "action table entry " + std::to_string(i) + " is not finite");
    return STMPC_OK;
}
int qactor_finish(stmpc_qactor *q, const double *action_values, stmpc_qactor **out) {
    q->table_h.assign(action_values, action_values + q->A);
    int rc = upload(q->table, action_values, (size_t)q->A);
    if (!rc) rc = q->categorical ? c51actor_raise_lds(q->device, q->lds) : qactor_raise_lds(q->device, q->lds);
    if (rc) { stmpc_qactor_destroy(q); return rc; }
    *out = q;
    return STMPC_OK;
}
}  // namespace

extern "C" {

int stmpc_qactor_create(stmpc_ctx *c, int n_in, int h1, int n_actions, const float *w0, const float *b0, const float *w1, const float *b1,
                        const double *action_values, int mode, stmpc_qactor **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (!w0 || !b0 || !w1 || !b1 || !action_values) return fail(STMPC_EINVAL, "NULL weight or table pointer");
    if (n_actions < 1 || n_actions > STMPC_ENV_MAX_ACTIONS) return fail(STMPC_EINVAL, "n_actions must be in 1 ... " + std::to_string(STMPC_ENV_MAX_ACTIONS));
    if (n_in < 1 || n_in > AT_KIN - 1 || h1 < 1 || h1 > 1024) return fail(STMPC_EINVAL, "Q-network shape out of range (n_in <= 31, hidden width <= 1024)");
    TRY(qactor_check_table(action_values, n_actions, n_actions, mode));
    HIPCHK(hipSetDevice(c->device));
    const int h1p = (h1 + 15) & ~15, Ap = (n_actions + 15) & ~15;
    const size_t lds = ddpg_tile_bytes(h1p, Ap);
    if (lds + 1024 > (size_t)c->lds_per_block) return fail(STMPC_EINVAL, "Q-network too wide for one workgroup's LDS");
    stmpc_qactor *q = new stmpc_qactor();
    q->device = c->device; q->mode = mode; q->n_in = n_in; q->A = n_actions; q->lds = lds;
    // the learner's own path: net_build's buffers, the slot's segments into the padded layout, k_dqn_adam's re-packing
    DdpgDev &d = q->dev.base;
    d.n_obs = n_in; d.h1 = h1; d.h2 = n_actions; d.h1p = h1p; d.h2p = Ap;
    q->dev.A = n_actions; q->dev.Ap = Ap; q->dev.target_period = 1;
    int rc = net_build(q->net, d.q, n_in, h1p, Ap);
    if (!rc) rc = ddpg_zero(q->cnt, DG_NCNT * sizeof(long long));
    if (!rc) {
        d.cnt = q->cnt.as<long long>();
        const std::vector<Seg> lay = slot_layout(n_in, h1, n_actions, h1p, Ap, false);
        std::vector<float> flat;
        flat.insert(flat.end(), w0, w0 + (size_t)h1 * n_in);
        flat.insert(flat.end(), b0, b0 + h1);
        flat.insert(flat.end(), w1, w1 + (size_t)n_actions * h1);
        flat.insert(flat.end(), b1, b1 + n_actions);
        const int ablocks = make_grid(16, h1p, Ap, false).ablocks;
        rc = slot_set(c->device, lay, (size_t)dg_nparam(h1p, Ap), d.q.w, flat.data(), (int64_t)flat.size(), true,
                      [&] { hipLaunchKernelGGL(k_dqn_adam, dim3(ablocks), dim3(256), 0, (hipStream_t)0, q->dev, 0.f, 1, 1); });
    }
    if (rc) { stmpc_qactor_destroy(q); return rc; }
    return qactor_finish(q, action_values, out);
}

int stmpc_qactor_view_dqn(stmpc_dqn *t, int target, const double *action_values, int n_actions, int mode, stmpc_qactor **out) {
    if (!t || !action_values || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (target != 0 && target != 1) return fail(STMPC_EINVAL, "target must be 0 (online network) or 1 (target network)");
    TRY(qactor_check_table(action_values, n_actions, t->cfg.n_actions, mode));
    HIPCHK(hipSetDevice(t->rp.device));
    stmpc_qactor *q = new stmpc_qactor();   // owns its table alone: destroying it frees nothing of the learner's
    q->device = t->rp.device; q->learner = t; q->target = target; q->mode = mode; q->n_in = t->cfg.n_obs; q->A = t->cfg.n_actions; q->lds = t->lds;
    return qactor_finish(q, action_values, out);
}

}  // extern "C"

namespace {
// stmpc_c51actor_create and stmpc_dueling_c51actor_create: w1 and b1 have (n_actions + dueling) * n_atoms rows
int c51actor_create(stmpc_ctx *c, int n_in, int h1, int n_actions, int n_atoms, int dueling, double v_min, double v_max, const float *w0, const float *b0,
                    const float *w1, const float *b1, const double *action_values, int mode, stmpc_qactor **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (!w0 || !b0 || !w1 || !b1 || !action_values) return fail(STMPC_EINVAL, "NULL weight or table pointer");
    if (n_actions < 1 || n_actions > STMPC_ENV_MAX_ACTIONS) return fail(STMPC_EINVAL, "n_actions must be in 1 ... " + std::to_string(STMPC_ENV_MAX_ACTIONS));
    if (n_in < 1 || n_in > AT_KIN - 1 || h1 < 1 || h1 > 1024) return fail(STMPC_EINVAL, "C51 network shape out of range (n_in <= 31, hidden width <= 1024)");
    if (n_atoms < 2) return fail(STMPC_EINVAL, "n_atoms must be at least 2");
    TRY(c51_check_width(n_actions, n_atoms, dueling));
    if (!std::isfinite(v_min) || !std::isfinite(v_max) || !(v_max > v_min)) return fail(STMPC_EINVAL, "the support needs finite v_min < v_max");
    TRY(qactor_check_table(action_values, n_actions, n_actions, mode));
    HIPCHK(hipSetDevice(c->device));
    const int AK = (n_actions + dueling) * n_atoms, h1p = (h1 + 15) & ~15, Ap = (AK + 15) & ~15;
    const size_t lds = ddpg_tile_bytes(h1p, Ap);
    if (lds + 1024 > (size_t)c->lds_per_block) return fail(STMPC_EINVAL, "C51 network too wide for one workgroup's LDS");
    stmpc_qactor *q = new stmpc_qactor();
    q->device = c->device; q->mode = mode; q->n_in = n_in; q->A = n_actions; q->lds = lds; q->categorical = true;
    q->dueling = dueling; q->K = n_atoms; q->v_min = v_min; q->v_max = v_max; q->dz = (v_max - v_min) / (double)(n_atoms - 1);
    // the C51 learner's own path: net_build's buffers, the slot's segments into the padded layout with A K output rows, k_c51_adam's re-packing
    DdpgDev &d = q->dev.base;
    d.n_obs = n_in; d.h1 = h1; d.h2 = AK; d.h1p = h1p; d.h2p = Ap;
    q->dev.A = n_actions; q->dev.Ap = Ap; q->dev.target_period = 1;
    int rc = net_build(q->net, d.q, n_in, h1p, Ap);
    if (!rc) rc = ddpg_zero(q->cnt, DG_NCNT * sizeof(long long));
    if (!rc) {
        d.cnt = q->cnt.as<long long>();
        const std::vector<Seg> lay = slot_layout(n_in, h1, AK, h1p, Ap, false);
        std::vector<float> flat;
        flat.insert(flat.end(), w0, w0 + (size_t)h1 * n_in);
        flat.insert(flat.end(), b0, b0 + h1);
        flat.insert(flat.end(), w1, w1 + (size_t)AK * h1);
        flat.insert(flat.end(), b1, b1 + AK);
        const int ablocks = make_grid(16, h1p, Ap, false).ablocks;
        const C51Dev D = c51actor_dev(q);
        rc = slot_set(c->device, lay, (size_t)dg_nparam(h1p, Ap), d.q.w, flat.data(), (int64_t)flat.size(), true,
                      [&] { hipLaunchKernelGGL(k_c51_adam, dim3(ablocks), dim3(256), 0, (hipStream_t)0, D, 0.f, 1, 1); });
    }
    if (rc) { stmpc_qactor_destroy(q); return rc; }
    return qactor_finish(q, action_values, out);
}
}  // namespace

extern "C" {

int stmpc_c51actor_create(stmpc_ctx *c, int n_in, int h1, int n_actions, int n_atoms, double v_min, double v_max, const float *w0, const float *b0,
                          const float *w1, const float *b1, const double *action_values, int mode, stmpc_qactor **out) {
    return c51actor_create(c, n_in, h1, n_actions, n_atoms, 0, v_min, v_max, w0, b0, w1, b1, action_values, mode, out);
}

int stmpc_dueling_c51actor_create(stmpc_ctx *c, int n_in, int h1, int n_actions, int n_atoms, double v_min, double v_max, const float *w0, const float *b0,
                                  const float *w1, const float *b1, const double *action_values, int mode, stmpc_qactor **out) {
    return c51actor_create(c, n_in, h1, n_actions, n_atoms, 1, v_min, v_max, w0, b0, w1, b1, action_values, mode, out);
}

int stmpc_c51actor_view(stmpc_c51 *t, int target, const double *action_values, int n_actions, int mode, stmpc_qactor **out) {
    if (!t || !action_values || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (target != 0 && target != 1) return fail(STMPC_EINVAL, "target must be 0 (online network) or 1 (target network)");
    TRY(qactor_check_table(action_values, n_actions, t->cfg.n_actions, mode));
    HIPCHK(hipSetDevice(t->rp.device));
    stmpc_qactor *q = new stmpc_qactor();   // owns its table alone: destroying it frees nothing of the learner's
    q->device = t->rp.device; q->c51 = t; q->categorical = true; q->target = target; q->mode = mode; q->n_in = t->cfg.n_obs; q->A = t->cfg.n_actions;
    q->lds = ddpg_tile_bytes(t->h1p, t->Ap);     // (the learner's own LDS has the m tile behind it, which an evaluation does not need)
    return qactor_finish(q, action_values, out);
}

void stmpc_qactor_destroy(stmpc_qactor *q) {
    if (!q) return;
    (void)hipSetDevice(q->device);
    delete q;
}

int stmpc_qactor_set_limits(stmpc_qactor *q, double tick_length, double minimum_negative_jerk, double maximum_positive_jerk) {
    if (!q) return fail(STMPC_EINVAL, "NULL argument");
    if (!(tick_length > 0) || !std::isfinite(tick_length) || !std::isfinite(minimum_negative_jerk) || !std::isfinite(maximum_positive_jerk) ||
        !(minimum_negative_jerk <= maximum_positive_jerk))
        return fail(STMPC_EINVAL, "tick_length must be positive and the jerk limits ordered, all finite");
    q->tick = tick_length; q->jerk_min = minimum_negative_jerk; q->jerk_max = maximum_positive_jerk; q->limits = true;
    return STMPC_OK;
}

int stmpc_qactor_eval_device(stmpc_ctx *c, const stmpc_qactor *q, const stmpc_policy_features_cfg *f, int N, int Kmax, int step, const double *d_cur_ego4,
                             const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, float *d_feat, int feat_stride,
                             int32_t *d_action, float *d_q, double *d_jerk, void *stream) {
    if (!c || !q || !f) return fail(STMPC_EINVAL, "NULL argument");
    if (N < 1) return fail(STMPC_EINVAL, "N must be positive");
    if (f->time_feature) return fail(STMPC_EINVAL, "a Q-network has no time feature: the features cfg must have time_feature = 0");
    if (q->mode == STMPC_QACTOR_ACCELERATION && !q->limits)
        return fail(STMPC_EINVAL, "acceleration mode needs the tick length and the jerk limits (stmpc_qactor_set_limits)");
    FeatCfg fc;
    TRY(actor_eval_checks(c, q->device, q->n_in, f, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, nullptr, d_feat, feat_stride, d_jerk, &fc));
    return qactor_eval_run(c, q, fc, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_feat, feat_stride, d_action, d_q, d_jerk, stream);
}

}  // extern "C"

// (stmpc_host.hpp) stmpc_qactor_eval_device after its argument checks (N >= 1)
int qactor_eval_run(stmpc_ctx *c, const stmpc_qactor *q, const FeatCfg &fc, int N, int Kmax, int step, const double *d_cur_ego4, const int32_t *d_k,
                    const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, float *d_feat, int feat_stride, int32_t *d_action, float *d_q,
                    double *d_jerk, void *stream) {
    const int *live;
    TRY(rollout_live(c, N, step, &live));
    HIPCHK(hipSetDevice(c->device));
    QActorOut o{q->table.as<double>(), q->tick, q->jerk_min, q->jerk_max, q->mode == STMPC_QACTOR_ACCELERATION, feat_stride, d_feat, d_action, d_q, d_jerk};
    if (q->categorical)
        hipLaunchKernelGGL(k_c51actor_eval, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), q->lds, (hipStream_t)stream, fc, c51actor_dev(q), q->c51 ? q->target : 0, N,
                           Kmax, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, live, o);
    else
        hipLaunchKernelGGL(k_qactor_eval, dim3((N + AT_TM - 1) / AT_TM), dim3(AT_THREADS), q->lds, (hipStream_t)stream, fc, q->learner ? q->learner->dev : q->dev,
                           q->learner ? q->target : 0, N, Kmax, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, live, o);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

// ---- a population of Q-networks as policies (stmpc_pop_qactor_*): P members, one launch per evaluation; kernel in stmpc_qactor_pop_kernels.hpp ------
struct stmpc_qactor_pop {
    int device = 0;
    DevBuf table;                           // QActorMember [P], built once at create.  A view's entry copies its learner's dev.base.q: net_build wires those
                                            // pointers in stmpc_dqn_create and nothing re-wires them before destroy (stmpc_dqn_per_enable and
                                            // stmpc_pop_dqn_per_enable go through Replay::wire, which writes the replay's part of dev.base alone)
    bool categorical = false;               // stmpc_pop_c51actor_create made it: the table is C51ActorMember [P] and k_c51actor_eval_pop evaluates it.  A view's
                                            // entry copies its learner's dev.dq.base.q, shape and support (K, dueling, v_min, v_max, dz): q_create wires them
                                            // (net_build, C51Head::wire) and nothing re-wires them before destroy -- stmpc_c51_per_enable, stmpc_pop_c51_per_enable
                                            // and the multi-step enables go through Replay::wire (the replay's part of dev.dq.base alone), q_pop_upload copies the
                                            // members' structs as they are, and a noisy learner's shadow structs are copies that leave t->dev on mu
    int P = 0, n_in = 0;
    size_t lds = 0;
    // what qshield_policy_check compares with an env, per member: the mode, the limits, the host's copy of the action table
    struct Meta { int mode; double tick, jerk_min, jerk_max; std::vector<double> table; };
    std::vector<Meta> meta;
    const QActorMember *dev() const { return table.as<QActorMember>(); }
    const C51ActorMember *dev_c51() const { return table.as<C51ActorMember>(); }
};

namespace {
int qactor_pop_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling;
    return raise_dynamic_lds((const void *)k_qactor_eval_pop, "k_qactor_eval_pop", ceiling, device, lds);
}
int c51actor_pop_raise_lds(int device, size_t lds) {
    static LdsCeiling ceiling;
    return raise_dynamic_lds((const void *)k_c51actor_eval_pop, "k_c51actor_eval_pop", ceiling, device, lds);
}
// the struct k_qactor_eval gets for this actor
const DqnDev &qactor_dev(const stmpc_qactor *q) { return q->learner ? q->learner->dev : q->dev; }
// what both kinds of population end their create with: the handle around an uploaded member table, the members' meta, the kernel's dynamic LDS
template <class Member> int qactor_pop_finish(stmpc_ctx *c, const stmpc_qactor *const *qactors, const std::vector<Member> &host, bool categorical, stmpc_qactor_pop **out) {
    const int P = (int)host.size();
    HIPCHK(hipSetDevice(c->device));
    stmpc_qactor_pop *p = new stmpc_qactor_pop();
    p->device = c->device; p->categorical = categorical; p->P = P; p->n_in = qactors[0]->n_in; p->lds = qactors[0]->lds;
    for (int m = 0; m < P; ++m) p->meta.push_back({qactors[m]->mode, qactors[m]->tick, qactors[m]->jerk_min, qactors[m]->jerk_max, qactors[m]->table_h});
    int rc = upload(p->table, host.data(), host.size());
    if (!rc) rc = categorical ? c51actor_pop_raise_lds(c->device, p->lds) : qactor_pop_raise_lds(c->device, p->lds);
    if (rc) { stmpc_pop_qactor_destroy(p); return rc; }
    *out = p;
    return STMPC_OK;
}
}  // namespace

extern "C" {

int stmpc_pop_qactor_create(stmpc_ctx *c, const stmpc_qactor *const *qactors, int P, stmpc_qactor_pop **out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    *out = nullptr;
    if (P < 1 || P > STMPC_DDPG_POP_MAX) return fail(STMPC_EINVAL, "a population has 1 ... 64 members, not " + std::to_string(P));
    if (!qactors) return fail(STMPC_EINVAL, "NULL argument");
    std::vector<QActorMember> host;
    for (int m = 0; m < P; ++m) {
        const stmpc_qactor *q = qactors[m];
        if (!q) return fail(STMPC_EINVAL, "member " + std::to_string(m) + " is NULL");
        if (q->device != c->device) return fail(STMPC_EINVAL, "member " + std::to_string(m) + " and the context are on different devices");
        if (q->categorical)
            return fail(STMPC_EINVAL, "member " + std::to_string(m) + " has a categorical (C51) head: a population evaluates Q-networks, one launch needs one head; "
                                      "evaluate a C51 policy alone (stmpc_qactor_eval_device), or C51 policies together (stmpc_pop_c51actor_create)");
        const DqnDev &d = qactor_dev(q), &d0 = qactor_dev(qactors[0]);
        if (q->n_in != qactors[0]->n_in || d.base.h1p != d0.base.h1p || d.Ap != d0.Ap || q->A != qactors[0]->A)
            return fail(STMPC_EINVAL, "the members of a population share n_in, the padded widths and n_actions (member " + std::to_string(m) + " differs from member 0)");
        if (q->mode == STMPC_QACTOR_ACCELERATION && !q->limits)
            return fail(STMPC_EINVAL, "member " + std::to_string(m) + " is in acceleration mode and needs the tick length and the jerk limits (stmpc_qactor_set_limits)");
        host.push_back({d.base.q, q->n_in, d.base.h1p, q->A, d.Ap, q->learner ? q->target : 0, q->mode == STMPC_QACTOR_ACCELERATION, q->table.as<double>(), q->tick,
                        q->jerk_min, q->jerk_max});
    }
    return qactor_pop_finish(c, qactors, host, false, out);
}

int stmpc_pop_c51actor_create(stmpc_ctx *c, const stmpc_qactor *const *members, int P, stmpc_qactor_pop **out) {
    if (out) *out = nullptr;                // (every refusal leaves *out NULL, a NULL context's too)
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    if (P < 1 || P > STMPC_DDPG_POP_MAX) return fail(STMPC_EINVAL, "a population has 1 ... 64 members, not " + std::to_string(P));
    if (!members) return fail(STMPC_EINVAL, "NULL argument");
    std::vector<C51ActorMember> host;
    C51Dev d0{};
    for (int m = 0; m < P; ++m) {
        const stmpc_qactor *q = members[m];
        if (!q) return fail(STMPC_EINVAL, "member " + std::to_string(m) + " is NULL");
        if (q->device != c->device) return fail(STMPC_EINVAL, "member " + std::to_string(m) + " and the context are on different devices");
        if (!q->categorical)
            return fail(STMPC_EINVAL, "member " + std::to_string(m) + " is a Q-network, not a categorical (C51) policy: one launch needs one head; Q-networks "
                                      "share a population of their own (stmpc_pop_qactor_create)");
        const C51Dev d = c51actor_dev(q);
        if (m == 0) d0 = d;
        if (q->n_in != members[0]->n_in || d.dq.base.h1p != d0.dq.base.h1p || d.dq.Ap != d0.dq.Ap || q->A != members[0]->A || d.K != d0.K || d.dueling != d0.dueling)
            return fail(STMPC_EINVAL, "the members of a population share n_in, the padded hidden width, n_actions, n_atoms and the head, dueling or not (member " +
                                      std::to_string(m) + " differs from member 0)");
        if (q->mode == STMPC_QACTOR_ACCELERATION && !q->limits)
            return fail(STMPC_EINVAL, "member " + std::to_string(m) + " is in acceleration mode and needs the tick length and the jerk limits (stmpc_qactor_set_limits)");
        host.push_back({d.dq.base.q, q->n_in, d.dq.base.h1p, q->A, d.dq.Ap, d.K, d.dueling, d.v_min, d.v_max, d.dz, q->c51 ? q->target : 0,
                        q->mode == STMPC_QACTOR_ACCELERATION, q->table.as<double>(), q->tick, q->jerk_min, q->jerk_max});
    }
    return qactor_pop_finish(c, members, host, true, out);
}

void stmpc_pop_qactor_destroy(stmpc_qactor_pop *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

int stmpc_pop_qactor_size(const stmpc_qactor_pop *p) { return p ? p->P : 0; }

int stmpc_pop_qactor_eval_device(stmpc_ctx *c, const stmpc_qactor_pop *p, const stmpc_policy_features_cfg *f, int n_per_member, int Kmax, int step,
                                 const double *d_cur_ego4, const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa,
                                 float *d_feat, int feat_stride, int32_t *d_action, float *d_q, double *d_jerk, void *stream) {
    if (!c || !p || !f) return fail(STMPC_EINVAL, "NULL argument");
    if (n_per_member < 0 || (long long)n_per_member * p->P > 0x7fffffffLL) return fail(STMPC_EINVAL, "n_per_member out of range");
    if (f->time_feature) return fail(STMPC_EINVAL, "a Q-network has no time feature: the features cfg must have time_feature = 0");
    const int N = n_per_member * p->P;
    FeatCfg fc;
    TRY(actor_eval_checks(c, p->device, p->n_in, f, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, nullptr, d_feat, feat_stride, d_jerk, &fc));
    if (N == 0) return STMPC_OK;
    return qactor_pop_eval_run(c, p, fc, n_per_member, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_feat, feat_stride, d_action, d_q, d_jerk, stream);
}

}  // extern "C"

// (stmpc_host.hpp) stmpc_pop_qactor_eval_device after its argument checks (P * n_per_member >= 1)
int qactor_pop_eval_run(stmpc_ctx *c, const stmpc_qactor_pop *p, const FeatCfg &fc, int n_per_member, int Kmax, int step, const double *d_cur_ego4,
                        const int32_t *d_k, const double *d_cur_ox, const double *d_cur_ov, const double *d_cur_oa, float *d_feat, int feat_stride,
                        int32_t *d_action, float *d_q, double *d_jerk, void *stream) {
    const int *live;
    TRY(rollout_live(c, n_per_member * p->P, step, &live));
    HIPCHK(hipSetDevice(c->device));
    const dim3 grid((n_per_member + AT_TM - 1) / AT_TM, p->P);
    if (p->categorical)
        hipLaunchKernelGGL(k_c51actor_eval_pop, grid, dim3(AT_THREADS), p->lds, (hipStream_t)stream, fc, p->dev_c51(), n_per_member, Kmax, d_cur_ego4, d_k, d_cur_ox,
                           d_cur_ov, d_cur_oa, live, d_feat, feat_stride, d_action, d_q, d_jerk);
    else
        hipLaunchKernelGGL(k_qactor_eval_pop, grid, dim3(AT_THREADS), p->lds, (hipStream_t)stream, fc, p->dev(), n_per_member, Kmax, d_cur_ego4, d_k, d_cur_ox,
                           d_cur_ov, d_cur_oa, live, d_feat, feat_stride, d_action, d_q, d_jerk);
    HIPCHK(hipGetLastError());
    return STMPC_OK;
}

// (stmpc_host.hpp) the rollout policy of stmpc_qshield_env_*: a lone Q-actor, or a population on slices of the env's rows
int qshield_policy_check(const stmpc_ctx *c, const stmpc_qactor *q, const stmpc_qactor_pop *pop, int n_per_member, int N, bool acceleration,
                         const double *values, int n_values, double tick, double jerk_min, double jerk_max, int *n_in) {
    if (!q == !pop) return fail(STMPC_EINVAL, "combined shield (Q): exactly one of the Q-actor and the Q-actor population must be given, the other NULL");
    if ((q ? q->device : pop->device) != c->device) return fail(STMPC_EINVAL, "combined shield (Q): the policy and the context are on different devices");
    if (q && n_per_member != 0) return fail(STMPC_EINVAL, "combined shield (Q): n_per_member belongs to a population (0 with a lone Q-actor)");
    if (pop && (n_per_member < 1 || (long long)n_per_member * pop->P != N))
        return fail(STMPC_EINVAL, "combined shield (Q): the population's P * n_per_member must be the env's N (" + std::to_string(pop->P) + " * " +
                                  std::to_string(n_per_member) + " != " + std::to_string(N) + ")");
    const int members = q ? 1 : pop->P;
    for (int m = 0; m < members; ++m) {
        const int mode = q ? q->mode : pop->meta[m].mode;
        const std::vector<double> &table = q ? q->table_h : pop->meta[m].table;
        const std::string who = q ? std::string("the Q-actor") : "member " + std::to_string(m);
        if ((int)table.size() != n_values)
            return fail(STMPC_EINVAL, "combined shield (Q): " + who + " has " + std::to_string(table.size()) + " actions, the env's table n_action_values = " + std::to_string(n_values));
        if ((mode == STMPC_QACTOR_ACCELERATION) != acceleration)
            return fail(STMPC_EINVAL, "combined shield (Q): the mode of " + who + " is not the env's action mode (STMPC_QACTOR_JERK with STMPC_ENV_JERK, STMPC_QACTOR_ACCELERATION with STMPC_ENV_ACCELERATION)");
        if (memcmp(table.data(), values, (size_t)n_values * 8) != 0)
            return fail(STMPC_EINVAL, "combined shield (Q): the action table of " + who + " is not byte-identical to the env's action_values");
        if (acceleration) {
            const bool has = q ? q->limits : true;          // (a population refuses an acceleration member without limits at create)
            const double t = q ? q->tick : pop->meta[m].tick, lo = q ? q->jerk_min : pop->meta[m].jerk_min, hi = q ? q->jerk_max : pop->meta[m].jerk_max;
            if (!has || t != tick || lo != jerk_min || hi != jerk_max)
                return fail(STMPC_EINVAL, "combined shield (Q): the tick length and jerk limits of " + who + " (stmpc_qactor_set_limits) are not the env's");
        }
    }
    *n_in = q ? q->n_in : pop->n_in;
    return STMPC_OK;
}
