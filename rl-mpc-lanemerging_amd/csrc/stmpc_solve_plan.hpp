// stmpc_solve_plan.hpp -- what one batched solve launches, decided in plain C++ before anything touches the device.
// plan_solve() is a pure function of the settings (SolveKnobs), the device's shape, the parameter set and the batch's shape: which windows (tiers)
// there are, their grids and LDS bytes, which k_solve instantiation serves each (KernelVariant), and the order of the launches with their streams
// and events (SolvePlan::steps).  solve_device() in stmpc_solver.hip carries a plan out; tests/solve_plan_check.cpp prints one on a CPU.
// No HIP here: the parameter set is any struct with DevP's fields (stmpc_kernels.hpp).
#ifndef STMPC_SOLVE_PLAN_HPP
#define STMPC_SOLVE_PLAN_HPP

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stmpc.h"

#ifndef STMPC_KERNELS_HPP
// A translation unit without the kernels (host-only tools and tests): the shape constants of stmpc_kernels.hpp, which a HIP translation unit
// includes first.  The same values.
#define STMPC_MAX_TIERS 6
#define STMPC_MAXWAVES 8
#define STMPC_CELL_BYTES 14
#define STMPC_LIST_SLACK (64 * (STMPC_MAXWAVES + 1) * 2)
inline size_t stmpc_chunk_ints(int W) { return (size_t)(W / 64 + 8); }
inline size_t stmpc_tab_bytes(int H, int KT) { return (size_t)H * KT * 24 + (((size_t)H * 4 + 7) & ~(size_t)7); }
#endif

#ifndef STMPC_FAN1
#define STMPC_FAN1 8        /* candidate slots per barrier pair of the wide-lattice kernels outside the standard second window (128 VGPRs); 7 / 11 / 12 measured in round 5, 12 again in round 6 */
#endif
#ifndef STMPC_FAN88
#define STMPC_FAN88 24      /* candidate slots per barrier pair in the standard second window (it has the registers: 256 VGPRs); 12 / 16 / 21 / 24 measured, EXPERIMENTS.md */
#endif

namespace stmpc {
namespace plan {

// ---- settings ------------------------------------------------------------------------------------------------------------------------------
// Every solver setting stmpc_create takes from the environment (from_env), with its default.
struct SolveKnobs {
    int lds_tier_W[STMPC_MAX_TIERS] = {2048, 4096, 8192, 0, 0, 0};   // STMPC_TIERS="512,2048": LDS windows (cells), increasing
    int n_lds_tiers = 0;          // 0 = automatic: {2048, smallest window covering every cell (<= 8192)}
    bool tiers_from_env = false;
    int pen_cells[STMPC_MAX_TIERS] = {0, 0, 0, 0, 0, 0};   // STMPC_PEN_CELLS="a,b,c": penalty-buffer cells per LDS tier (0 = min(W, 4096))
    int max_waves_per_cu = 16;     // STMPC_WAVES_PER_CU
    int lds_headroom = 1024;       // STMPC_LDS_HEADROOM: bytes added to a workgroup's dynamic LDS when counting workgroups per CU
    int waves_override = 0;       // STMPC_NW=n or "a,b,c": waves per workgroup (episode), all tiers or per LDS tier
    int waves_tier[STMPC_MAX_TIERS] = {0, 0, 0, 0, 0, 0};
    bool allow_fastdiv = true;     // STMPC_FASTDIV=0
    int prune = -1;               // STMPC_PRUNE: -1 auto (bounded search only when the fan-out is large), 0 off, 1 on
    double band_override = 0.0;    // STMPC_BAND
    int band_dense = 1;            // STMPC_BAND_DENSE=0/1: dense ordinary bounding attempts (band_pass)
    int tube_dense = 1;            // STMPC_TUBE_DENSE=0/1: dense guided attempt (tube_pass)
    int band_cap = 450;            // STMPC_BAND_CAP: nodes per layer the pre-pass steers its band towards (0 = fixed band); 300 until the pre-pass moved to
                                   // packed single precision (round 3): with candidates at a fifth of their former cost a wider pre-pass pays for itself in
                                   // tighter bounds (10 state seeds at N=4096: 375-600 all within 2 % of each other and 5 % ahead of 300)
    double band2_mult = 0.0;       // STMPC_BAND2_MULT (0 = default: 4 with the node cap, 5 with a fixed band)
    bool force_general = false;    // STMPC_FORCE_GENERAL=1 (tests)
    bool two_phase = false;        // STMPC_TWO_PHASE=1: bound all episodes first, then solve heaviest-first (measured 6 % slower at N=4096)
    bool allow_stage_tab = false;  // STMPC_STAGE_TAB=1: stage the vehicle table in LDS + scalar registers (costs the 4th workgroup per CU)
    bool resume = true;            // STMPC_RESUME=0/1: the wider window continues a checkpointed exact pass instead of starting over
    bool heavy_first = false;      // STMPC_HEAVY_FIRST=1: split tasks are handed out slow starters first (measured: 6.76-6.82 vs 6.81-6.82 ms at N=4096, 13.0 vs 12.2 ms at N=8192 -- long searches side by side slow each other down; off)
    int gsh_max = 4;               // STMPC_GSH=0..4: lanes per source of sparse layers, log2 (0 = one lane per source)
    bool split = true;             // STMPC_SPLIT=0/1: bounding and exact pass of an episode are separate tasks of the first launch (-4 % at N=4096)
    int overlap = -1;              // STMPC_OVERLAP=0/1: start the second LDS tier on its own stream while the first is still running (see k_solve);
                                   // -1 auto: with the bounded (wide fan-out) search, where overflow is common
    // STMPC_CU_RESERVE=n (multiple of 8, experiment): n compute units are kept out of the first window's launch and host the second
    // window's workgroups from the start of the step (CU-masked streams); 0 = off
    int cu_reserve = 0;
    int side_grid = 0;             // STMPC_SIDE_GRID=n: workgroups of the second window's side launch (0 = automatic: the tier's full grid with the bounded
                                   // search, 32 on the narrow lattice where a handful of episodes overflow)
    double last_infl = 1.005;      // STMPC_LAST_INFL: the exact pass's candidate filter lets terminals up to this factor above the bound through (SolveArgs::last_infl); 1 = off
    double bound_infl = 1.00002;   // STMPC_BOUND_INFL: factor on a bounding pass's single-precision path cost (>= 1.00002, the rounding of that total)
    int pool_cap_override = 0;     // STMPC_POOL=n: checkpoint pool entries (tests: a tiny pool must only cost speed)
    int qp_maxiters = STMPC_QP_MAXITERS;   // STMPC_QP_ITERS (experiment: the iteration cap of st.do_st_control's QP; the reference's is 10, st.py:17)
    int tube_w = 96;               // STMPC_TUBE=w: half-width (cells) of the guided bounding attempt, 0 = off (see SolveArgs::guide_tab)
    int prio_thr = 32000;          // STMPC_PRIO=t (0 = off): an overflowing search with more than t (layers left x nodes of the saved layer) ahead of it is served first
                                   // by the second window (SolveArgs::prio_thr): 4.60 -> 4.46 ms over 12 seeds at N = 4096, flat from 25000 to 35000
    int prio_mode = 0;             // STMPC_PRIO_MODE (experiment: which estimate prio_thr is compared with)
    bool bp16 = false;             // STMPC_BP16=1: two-byte back-pointers even where one byte would do
    int retry_move = 0;            // STMPC_RETRY_MOVE=k: see SolveArgs::retry_move
    double retry_mult[3] = {1.05, 1.3, 4.0};    // STMPC_RETRY="a,b,c": growth of a bound that turned out to be below the reference's terminal cost.  Round 2 grew gently
                                                // (1.02, 1.08, 1.3): most failures need less than 0.2 %, but the rare search that fails twice is three ever larger passes
                                                // in a row and ends the step; over 16 state seeds (1.05, 1.3, 4) has the same median and no 5.4-5.8 ms outliers
    int retire_cus = 0, retire_at = 75;   // STMPC_RETIRE_CUS=k, STMPC_RETIRE_AT=percent of N: k compute units leave the first launch once fewer than that many tasks are left (see SolveArgs::cu_tab)

    // "a,b,c": keep(k, value) for the k-th number, up to max_n of them
    template <class F> static void each_number(const char *q, int max_n, F &&keep) {
        for (int n = 0; *q && n < max_n; ++n) {
            keep(n, atoi(q));
            while (*q && *q != ',') ++q;
            if (*q == ',') ++q;
        }
    }
    // (cu_reserve: the wish, checked for its range -- stmpc_create clears it unless the masked streams exist, and overlap without a side stream)
    static SolveKnobs from_env() {
        SolveKnobs k;
        if (const char *w = getenv("STMPC_TIERS")) {
            int n = 0;      // (numbers are read until STMPC_MAX_TIERS - 1 of them have been accepted)
            each_number(w, 1 << 20, [&](int, int v) {
                if (n < STMPC_MAX_TIERS - 1 && v >= 64 && v <= 8192 && (v & (v - 1)) == 0 && (n == 0 || v > k.lds_tier_W[n - 1])) k.lds_tier_W[n++] = v;
            });
            if (n > 0) k.n_lds_tiers = n;
            k.tiers_from_env = n > 0;
        }
        if (const char *w = getenv("STMPC_WAVES_PER_CU")) { int v = atoi(w); if (v >= 1 && v <= 32) k.max_waves_per_cu = v; }
        if (const char *w = getenv("STMPC_LDS_HEADROOM")) { int v = atoi(w); if (v >= 600 && v <= 8192) k.lds_headroom = v; }
        if (const char *w = getenv("STMPC_PEN_CELLS")) each_number(w, STMPC_MAX_TIERS, [&](int n, int v) { if (v >= 128 && v <= 8192 && (v & (v - 1)) == 0) k.pen_cells[n] = v; });
        if (const char *w = getenv("STMPC_NW")) {
            if (strchr(w, ',')) each_number(w, STMPC_MAX_TIERS, [&](int n, int v) { if (v >= 1 && v <= STMPC_MAXWAVES) k.waves_tier[n] = v; });
            else { int v = atoi(w); if (v >= 1 && v <= STMPC_MAXWAVES) k.waves_override = v; }
        }
        if (const char *w = getenv("STMPC_FASTDIV")) k.allow_fastdiv = atoi(w) != 0;
        if (const char *w = getenv("STMPC_PRUNE")) k.prune = atoi(w) != 0 ? 1 : 0;
        if (const char *w = getenv("STMPC_BAND")) k.band_override = atof(w);
        if (const char *w = getenv("STMPC_FORCE_GENERAL")) k.force_general = atoi(w) != 0;
        if (const char *w = getenv("STMPC_TWO_PHASE")) k.two_phase = atoi(w) != 0;
        if (const char *w = getenv("STMPC_BAND2_MULT")) { double v = atof(w); if (v >= 1.0) k.band2_mult = v; }
        if (const char *w = getenv("STMPC_STAGE_TAB")) k.allow_stage_tab = atoi(w) != 0;
        if (const char *w = getenv("STMPC_OVERLAP")) k.overlap = atoi(w) != 0 ? 1 : 0;
        if (const char *w = getenv("STMPC_BAND_DENSE")) k.band_dense = atoi(w) != 0;
        if (const char *w = getenv("STMPC_TUBE_DENSE")) k.tube_dense = atoi(w) != 0;
        if (const char *w = getenv("STMPC_BAND_CAP")) { int v = atoi(w); if (v >= 0) k.band_cap = v; }
        if (const char *w = getenv("STMPC_SPLIT")) k.split = atoi(w) != 0;
        if (const char *w = getenv("STMPC_HEAVY_FIRST")) k.heavy_first = atoi(w) != 0;
        if (const char *w = getenv("STMPC_GSH")) { int v = atoi(w); if (v >= 0 && v <= 4) k.gsh_max = v; }
        if (const char *w = getenv("STMPC_RESUME")) k.resume = atoi(w) != 0;
        if (const char *w = getenv("STMPC_LAST_INFL")) { double v = atof(w); if (v >= 1.0 && v <= 4.0) k.last_infl = v; }
        if (const char *w = getenv("STMPC_BOUND_INFL")) { double v = atof(w); if (v >= 1.00002 && v <= 2.0) k.bound_infl = v; }
        if (const char *w = getenv("STMPC_POOL")) { int v = atoi(w); if (v >= 1) k.pool_cap_override = v; }
        if (const char *w = getenv("STMPC_QP_ITERS")) { int v = atoi(w); if (v >= 0 && v <= 1000) k.qp_maxiters = v; }
        if (const char *w = getenv("STMPC_TUBE")) { int v = atoi(w); if (v >= 0 && v <= 4096) k.tube_w = v; }
        if (const char *w = getenv("STMPC_PRIO")) { int v = atoi(w); if (v >= 0) k.prio_thr = v; }
        if (const char *w = getenv("STMPC_PRIO_MODE")) k.prio_mode = atoi(w);
        if (getenv("STMPC_BP16")) k.bp16 = true;
        if (const char *w = getenv("STMPC_RETRY_MOVE")) { int v = atoi(w); if (v >= 0 && v <= 4) k.retry_move = v; }
        if (const char *w = getenv("STMPC_RETRY")) { double x[3]; if (sscanf(w, "%lf,%lf,%lf", &x[0], &x[1], &x[2]) == 3 && x[0] > 1.0 && x[1] > 1.0 && x[2] > 1.0) for (int i = 0; i < 3; ++i) k.retry_mult[i] = x[i]; }
        if (const char *w = getenv("STMPC_RETIRE_CUS")) { int v = atoi(w); if (v >= 0 && v < 256) k.retire_cus = v; }
        if (const char *w = getenv("STMPC_RETIRE_AT")) { int v = atoi(w); if (v >= 1 && v <= 200) k.retire_at = v; }
        if (const char *w = getenv("STMPC_SIDE_GRID")) { int v = atoi(w); if (v >= 1) k.side_grid = v; }
        if (const char *w = getenv("STMPC_CU_RESERVE")) { int v = atoi(w); if (v >= 8 && v <= 128 && v % 8 == 0) k.cu_reserve = v; }
        return k;
    }
};

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------
struct DeviceShape { int num_cu, lds_per_block; };

// What a plan takes from earlier calls on the context.
struct SolveHistory {
    // Episodes that overflowed the first window ([0]) and that reached the clean-up tier ([1]) in the batch before this one: a mapped pinned word
    // the batch's last launch stores straight into host memory -- no copy, no stall --, read unsynchronised, possibly one batch late, when the next
    // one is set up.  [0]: the narrow lattice starts its second window alongside the first only when there was something for it to do; [1]: a
    // caller that never reads statistics (EpisodeRunner, decide_batch_device) gets the clean-up tier's full grid as well
    int overflow[2] = {0, 0};
    bool last_has_hbm = true;             // the last batch had a clean-up tier ([1] is that tier's count)
    int64_t last_hbm_tier_count = 0;      // episodes the last batch whose statistics were read sent to the clean-up tier
    bool fastdiv_proven = false;          // the context's cached proof that dt, dt^2 and dt^3 of this call's parameters divide exactly (fastdiv_ok, fastdiv2_ok)
};

// The template arguments of one k_solve instantiation (GRID is false in every batched launch); grouped: the kernel of namespace grouped
struct KernelVariant { bool use_lds, fastdiv; int kt, fanmax; bool s1gen; int res, nwx; bool grouped; };

// The instantiations the library is built with: exactly what plan_solve can store in a PlanTier -- launch_k_solve (stmpc_solver.hip) compiles these and
// refuses any other.  46: 32 lone, 14 grouped.
constexpr bool variant_built(const KernelVariant &v) {
    const bool fan = v.fanmax == 9 || v.fanmax == STMPC_FAN1, full = v.nwx == STMPC_MAXWAVES;
    // the HBM window is the last tier, and S1GEN is `last`; it has no staged table, no checkpoints and eight-wave lists (grouped: ordinary division)
    if (!v.use_lds) return v.s1gen && fan && full && v.kt == 0 && v.res == 0 && !(v.grouped && v.fastdiv);
    // the four-wave shape is W 2048 / PW 1024 and the 88 shape W 8192 / PW 4096: a penalty buffer below the window, so a tier always follows
    if ((v.nwx == 4 || v.nwx == 88) && v.s1gen) return false;
    if (v.res == 0) return fan && (full || v.nwx == 4) && (v.kt == 0 || (v.kt == 8 && v.fanmax == 9 && !v.grouped));      // stage_tab requires small_fan
    // checkpointing (resume_wanted): lone, the wide fan, no staged table, the first two of at least two LDS windows
    if (v.grouped || v.kt != 0) return false;
    if (v.res == 1) return v.fanmax == STMPC_FAN1 && (full || v.nwx == 4) && !v.s1gen;      // the window that saves is tier 0 of two: never the last
    return v.res == 2 && ((v.fanmax == STMPC_FAN1 && full) || (v.fanmax == STMPC_FAN88 && v.nwx == 88));       // the 88 shape alone has STMPC_FAN88 slots
}

struct PlanTier {
    int W, PW, waves, grid;     // window and penalty-buffer cells, waves per workgroup, workgroups
    size_t lds_bytes;           // dynamic LDS of a workgroup
    bool lds;                   // an LDS window (false: the HBM-scratch tier)
    KernelVariant variant, variant_resume;      // without / with the checkpoint pool (they differ in the first two windows only)
};

enum class Stream { Main, Side, Masked, Reserved };     // the caller's stream, the side stream, the two CU-masked streams of STMPC_CU_RESERVE
enum class Event { None, Fork, Join, Join0, JoinR, DpEnd };   // (DpEnd: the profiling mark after the last LDS tier)
enum class Op { None, Solve, Order, Order8 };           // a k_solve launch, k_order (by bound), k_order8 (by the predictor's key)
// One step of the schedule: wait for `wait` on `stream`, run `op`, record `record` on `stream`.
struct PlanStep {
    Op op; Stream stream; Event wait, record;
    int tier, phase;            // Solve: phase 0 = bound + exact, 1 = bounding pre-passes only, 2 = exact with the stored bounds
    int grid;                   // Solve: workgroups of this launch (the tier's, or a side launch's own)
};

struct SolvePlan {
    SolveKnobs k;               // the settings the plan was made under (the kernels take band_cap, retry_mult, ... as they are)
    int S_nom, Wg, Kalloc;      // cells of the nominal lattice, the window that covers every cell, vehicle slots
    int nt; PlanTier tier[STMPC_MAX_TIERS];
    bool small_fan, stage_tab, fastdiv, need_hbm_tier, bp_rel8, resume_wanted, overlap, split, heavy_first, reserve, two_phase, guided, retire;
    int prune_on, side_grid, maxshift, pool_cap, retire_from;
    long long retire_left;
    size_t bp_elem, ckpt_stride, pool_bytes;
    double band, band2_mult;
    int n_steps; PlanStep steps[2 * STMPC_MAX_TIERS + 12];
};

// np.arange(start, start + future_s + ds, ds)'s length for start = 0 (stmpc_num_s)
template <class P> int nominal_cells(const P &dp) { const double stop = 0.0 + dp.future_s + dp.ds; return (int)ceil((stop - 0.0) / dp.ds); }

inline int next_pow2(int v) { int w = 1; while (w < v) w <<= 1; return w; }

// Band of the bounding pre-pass and the factor of its second attempt, from a parameter set's weights.  Nominal: half the per-step cost of
// standing still (225 with the reference's weights).  With the node cap (default) the pass starts from 8x that and narrows the band whenever a
// layer expands more than band_cap nodes (dp_pass): wide where few alternatives exist, beam-like where many do -- 15 % fewer expanded nodes in
// total than the best fixed band (sweeps on the H=40 workload: fixed 60..1200, capped 225..8000 x 150..550).  Any value is safe (the exact pass
// re-checks); it only trades pre-pass work for tightness of the bound.
// Second attempt (penalty zone allowed): a wider band, but kept well below the cost of one worst-case step (j_w * j_max^2 ~ 12 k on the
// benchmark lattice): a band that admits those steps keeps everything, and single episodes then take several times longer (measured cliff at
// 44x the nominal band; 32x is used)
template <class P> void band_for(const SolveKnobs &k, const P &d, double *band, double *band2_mult) {
    const double band_nominal = fmax(1.0, 0.5 * d.v_w * d.v_des * d.v_des);
    *band = k.band_override > 0 ? k.band_override : (k.band_cap > 0 ? 8.0 * band_nominal : band_nominal);
    *band2_mult = k.band2_mult > 0 ? k.band2_mult : (k.band_cap > 0 && k.band_override <= 0 ? 4.0 : 5.0);
    if (k.band2_mult <= 0 && k.band_cap > 0) {
        const double dv = fmax(d.v_des, d.v_max - d.v_des), da = fmax(fabs(d.a_min), fabs(d.a_max)), dj = fmax(fabs(d.j_min), fabs(d.j_max));
        const double step_max = d.v_w * dv * dv + d.a_w * da * da + d.j_w * dj * dj;      // dearest single step, penalties aside
        if (step_max > 0 && *band * *band2_mult > 0.7 * step_max) *band2_mult = fmax(1.0, 0.7 * step_max / *band);
    }
}

// grouped: a solver-groups call (kernels of namespace grouped on one fixed set of shapes: no staged vehicle table, no checkpoint / resume); dp is
// then any group's parameters -- every decision depends on fields the groups share.
template <class P>
SolvePlan plan_solve(const SolveKnobs &k, const DeviceShape &dev, const P &dp, int N, int Kmax, bool grouped, const SolveHistory &hist) {
    SolvePlan p{};
    p.k = k;
    const int H = dp.H;
    p.S_nom = nominal_cells(dp);
    p.Kalloc = Kmax > 0 ? Kmax : 1;
    p.fastdiv = k.allow_fastdiv && hist.fastdiv_proven;
    // widest fan-out the dynamics allow (st_cy.pyx:65-93): acceleration- or jerk-limited window, +2 for rounding
    const double fan_acc = (dp.a_max - dp.a_min) * dp.dt2 / dp.ds, fan_jerk = (dp.j_max - dp.j_min) * dp.dt3 / dp.ds;
    const double fan_bound = (fan_acc < fan_jerk ? fan_acc : fan_jerk) + 2.0;
    p.small_fan = fan_bound <= 9.0;
    // the scalar-register vehicle table costs ~48 SGPRs/VGPRs: only with the small-fan kernel (the wide one would spill)
    p.stage_tab = !grouped && k.allow_stage_tab && p.small_fan && p.Kalloc <= 8 && stmpc_tab_bytes(H, 8) <= 4096;
    p.prune_on = k.prune < 0 ? (p.small_fan ? 0 : 1) : k.prune;
    p.two_phase = p.prune_on && k.two_phase;      // bound all episodes first, then solve them heaviest-first

    // tiers: LDS windows in increasing size, then one HBM-scratch tier whose window covers every cell
    p.Wg = next_pow2(p.S_nom + 2 + 128);   // covers every cell plus the 64-cell alignment slack
    PlanTier *const T = p.tier;
    int nt = 0;
    int auto_W[2] = {2048, p.Wg < 8192 ? p.Wg : 8192};
    int n_auto = 2;
    if (auto_W[1] <= auto_W[0]) { auto_W[0] = auto_W[1]; n_auto = 1; }      // one window already covers the lattice
    const int n_lds = k.tiers_from_env ? k.n_lds_tiers : n_auto;
    for (int i = 0; i < n_lds && nt < STMPC_MAX_TIERS - 1; ++i) {
        const int W = k.tiers_from_env ? k.lds_tier_W[i] : auto_W[i];
        if (W > p.Wg && nt > 0) break;
        const int nw = k.waves_tier[i] > 0 ? k.waves_tier[i] : (k.waves_override > 0 ? k.waves_override : (W <= 2048 ? 4 : 8));
        // penalty buffer: 1024 cells for the first (4-wave) tier -- with the 14 B/cell arrays that is 38 KB per
        // workgroup, i.e. 4 workgroups = 16 waves per CU -- and up to 4096 cells for the wider tiers
        int PW = k.pen_cells[i] > 0 ? k.pen_cells[i] : (i == 0 && W <= 2048 ? 1024 : 4096);
        if (PW > W) PW = W;
        const size_t lds = (size_t)W * STMPC_CELL_BYTES + STMPC_LIST_SLACK + (size_t)PW * 8 + ((stmpc_chunk_ints(W) * sizeof(int) + 15) & ~(size_t)15) +
                           stmpc_tab_bytes(H, p.stage_tab ? 8 : 0);
        if (lds + 2048 > (size_t)dev.lds_per_block) break;
        int per_cu = (int)((size_t)dev.lds_per_block / (lds + k.lds_headroom));      // (+ the kernel's static LDS and allocation granularity)
        const int by_waves = k.max_waves_per_cu / nw;
        if (per_cu > by_waves) per_cu = by_waves;
        if (per_cu < 1) per_cu = 1;
        T[nt].W = W; T[nt].PW = PW; T[nt].waves = nw; T[nt].lds = true; T[nt].lds_bytes = lds; T[nt].grid = dev.num_cu * per_cu;
        ++nt;
    }
    // an LDS tier whose window covers every cell cannot overflow: the HBM-scratch tier is only needed beyond that
    p.need_hbm_tier = (nt == 0) || T[nt - 1].W < p.Wg || T[nt - 1].PW < T[nt - 1].W;
    if (p.need_hbm_tier) {
        // Clean-up launch: when the last LDS window already covers every cell, the only episodes that can reach this tier are those whose
        // lattice is not start + n*delta (the LDS kernels are compiled for that form) and rounds whose 64 sources' targets do not fit the
        // penalty buffer -- none in 4096 x 16 benchmark batches.  The launch then exists for correctness only and is sized accordingly: a
        // full persistent grid costs 13 us per step to start and leave on an empty queue (and its spill prologue writes 9 MB), 16 workgroups 3.
        const bool cleanup_only = nt > 0 && T[nt - 1].W >= p.Wg && !k.tiers_from_env && !k.force_general;
        const int nw = k.waves_override > 0 ? k.waves_override : 8;
        // (a batch that sent more than a handful of episodes there -- e.g. identical reset states whose second lattice point is not start + step --
        // gets the full grid from the next step on)
        const int64_t sent_last = hist.last_has_hbm ? (int64_t)hist.overflow[1] : 0;
        T[nt].W = p.Wg; T[nt].PW = p.Wg; T[nt].waves = nw; T[nt].lds = false;
        T[nt].lds_bytes = ((stmpc_chunk_ints(p.Wg) * sizeof(int) + 15) & ~(size_t)15) + 16;
        T[nt].grid = (cleanup_only && hist.last_hbm_tier_count <= 16 && sent_last <= 16) ? 16 : dev.num_cu * (k.max_waves_per_cu / nw > 0 ? k.max_waves_per_cu / nw : 1);
        ++nt;
    }
    p.nt = nt;
    const bool two_lds = nt >= 2 && T[0].lds && T[1].lds;

    // checkpoint / resume across the first two LDS windows (SolveArgs::ckpt, ::pool_bp): a search that cannot build a layer in the first window
    // saves that layer and the back-pointer rows written so far in an entry of a pool and continues in the second window from there.
    // back-pointers: one byte (distance to the predecessor) when no step of the dynamics exceeds 255 cells, else two (its cell)
    p.bp_rel8 = ceil(dp.v_max * dp.dt / dp.ds) + 4.0 <= 255.0 && !k.bp16;
    p.bp_elem = p.bp_rel8 ? 1 : sizeof(uint16_t);
    p.ckpt_stride = 16 + (size_t)T[0].W * 12;
    // Pool: an eighth of the batch (5 % of the benchmark's searches overflow), at least 256 entries, of H x W0 back-pointers + one saved layer
    // (104 KB at H = 40): 53 MB for 4096 episodes, 0.85 GB for 65536 -- round 4 kept both for EVERY episode (0.43 GB / 6.9 GB).  A search that
    // finds the pool exhausted starts over in the wider window (stmpc_stats::pool_exhausted counts them).
    p.pool_cap = k.pool_cap_override > 0 ? k.pool_cap_override : (N / 8 > 256 ? N / 8 : 256);
    if (p.pool_cap > N) p.pool_cap = N;
    if (p.pool_cap > (1 << 22)) p.pool_cap = 1 << 22;            // (the entry number shares a word with the layer)
    p.pool_bytes = (size_t)p.pool_cap * ((size_t)H * T[0].W * p.bp_elem + p.ckpt_stride);
    // (compiled for the wide-fan kernels only; whether the device can spare the pool is the executor's to find out)
    p.resume_wanted = !grouped && k.resume && p.prune_on && !p.small_fan && !p.stage_tab && two_lds;

    // reserved compute units (experiment, STMPC_CU_RESERVE): the first window's persistent grid covers the remaining units only
    const bool reserve_cfg = k.cu_reserve > 0 && p.prune_on && two_lds && !k.two_phase;
    if (reserve_cfg) T[0].grid = T[0].grid / dev.num_cu * (dev.num_cu - k.cu_reserve);
    for (int i = 0; i < nt; ++i) if (T[i].grid > N) T[i].grid = N;

    // second LDS tier started alongside the first (see k_solve): only where overflow is common enough to pay for the
    // extra launch, and not with the two-phase schedule (its first launch of tier 0 only bounds)
    // (narrow lattice, round 5: three of 4096 benchmark states overflow the first window; run after the first launch they cost one search's latency,
    // 0.14 of a 1.0 ms step; alongside it, on a small grid, they are done when it ends -- but a side launch that finds nothing to do costs 40 us of
    // stream hand-overs, so it is started only when the previous batch on this context overflowed)
    const bool overlap_auto = p.prune_on != 0 || (p.small_fan && hist.overflow[0] > 0);
    p.overlap = nt >= 2 && T[1].lds && !p.two_phase && N > T[0].grid && (k.overlap < 0 ? overlap_auto : k.overlap != 0);
    p.side_grid = k.side_grid > 0 ? k.side_grid : (p.small_fan ? 32 : 0);
    p.reserve = reserve_cfg && p.overlap;
    p.split = p.prune_on && !k.two_phase && k.split && N >= 2 * T[0].grid;
    p.heavy_first = p.split && k.heavy_first;
    p.guided = p.prune_on && k.tube_w > 0;
    p.retire = p.overlap && p.split && k.retire_cus > 0 && k.retire_cus < dev.num_cu;
    p.retire_from = dev.num_cu - k.retire_cus; p.retire_left = (long long)N * k.retire_at / 100;
    band_for(k, dp, &p.band, &p.band2_mult);
    p.maxshift = (int)ceil(dp.v_max * dp.dt / dp.ds) + 2 + 66;     // st_cy.pyx:65-93: v <= v_max; + interval rounding to 64-cell blocks

    // the kernel of each tier.  Only the last tier carries the general lattice-coordinate form (S1GEN, see solve_episode); the first window's
    // four-wave workgroups search list segments with 3 compares instead of 7 (NWX 4); checkpointing variants only where they are used: the
    // first window saves (RES 1), the second continues (RES 2)
    const int fm = p.small_fan ? 9 : STMPC_FAN1;
    for (int i = 0; i < nt; ++i) {
        PlanTier &t = T[i];
        const bool last = i == nt - 1;
        const bool std_shape = t.waves == 4 && t.W == 2048 && t.PW == 1024;      // the kernels compiled with these as constants
        const bool std_shape2 = t.waves == 8 && t.W == 8192 && t.PW == 4096;
        KernelVariant v{t.lds, p.fastdiv, t.lds && p.stage_tab ? 8 : 0, fm, last, 0, STMPC_MAXWAVES, grouped};
        if (grouped) {
            // the grouped family: first window in its standard shape, any other LDS window and the HBM window in the general shape
            if (!t.lds) v.fastdiv = false;
            else if (!last && std_shape) v.nwx = 4;
            t.variant = t.variant_resume = v;
            continue;
        }
        if (t.lds && std_shape) v.nwx = 4;
        t.variant = t.variant_resume = v;
        if (two_lds && fm == STMPC_FAN1 && v.kt == 0 && i <= 1) {       // (a lone LDS window never checkpoints: the two coincide)
            KernelVariant &r = t.variant_resume;
            r.res = i + 1;
            if (i == 1) { r.nwx = STMPC_MAXWAVES; if (std_shape2) { r.fanmax = STMPC_FAN88; r.nwx = 88; } }
        }
    }

    // the schedule
    int n = 0;
    auto step = [&](Op op, Stream s, Event wait, Event record, int tier = 0, int phase = 0, int grid = 0) { p.steps[n++] = PlanStep{op, s, wait, record, tier, phase, grid}; };
    if (p.heavy_first) step(Op::Order8, Stream::Main, Event::None, Event::None);
    if (p.two_phase) {                                           // bound every episode, order them heaviest-first
        step(Op::Solve, Stream::Main, Event::None, Event::None, 0, 1, T[0].grid);
        step(Op::Order, Stream::Main, Event::None, Event::None);
    }
    for (int i = 0; i < nt; ++i) {
        const int phase = p.two_phase ? 2 : 0;
        if (p.reserve && i == 0) {
            // the reserved units host second-window workgroups from the start of the step; the masked streams partition the device, so
            // these consumers may always wait for the queue (they cannot be holding a unit a producer needs)
            step(Op::Solve, Stream::Masked, Event::Fork, Event::Join0, 0, phase, T[0].grid);
            step(Op::Solve, Stream::Reserved, Event::Fork, Event::JoinR, 1, 0, (T[1].grid / dev.num_cu > 0 ? T[1].grid / dev.num_cu : 1) * k.cu_reserve);
            step(Op::None, Stream::Main, Event::Join0, Event::None);
            step(Op::None, Stream::Main, Event::JoinR, Event::None);
        } else step(Op::Solve, Stream::Main, Event::None, Event::None, i, phase, T[i].grid);
        if (p.overlap && i == 0) {
            // tier 1 alongside tier 0: queued on the side stream behind the predictor only; its workgroups start when
            // tier 0's persistent workgroups begin to leave CUs.  The main stream then waits for it, and the ordinary
            // launch of tier 1 that follows picks up whatever it left (normally nothing).
            step(Op::Solve, Stream::Side, Event::Fork, Event::Join, 1, 0, (p.side_grid > 0 && p.side_grid < T[1].grid) ? p.side_grid : T[1].grid);
            step(Op::None, Stream::Main, Event::Join, Event::None);
        }
        if ((p.need_hbm_tier && i == nt - 2) || (!p.need_hbm_tier && i == nt - 1) || nt == 1) step(Op::None, Stream::Main, Event::None, Event::DpEnd);   // after the last LDS tier
    }
    p.n_steps = n;
    return p;
}

}  // namespace plan
}  // namespace stmpc

#endif  // STMPC_SOLVE_PLAN_HPP
