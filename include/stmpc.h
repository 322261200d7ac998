/*
 * stmpc.h -- C-ABI of the MI355X-native ST ("MPC") lattice solver.
 *
 * This is the drop-in boundary for the reference's trajectory-search hot path.
 * Each entry point names the reference interface it replaces (paths relative to
 * the reference checkout jlubars/RL-MPC-LaneMerging):
 *
 *   stmpc_solve_grid          <- st_cy.solve_s_t_path_fast           st_cy.pyx:315-399 (call site st.py:740-746)
 *   stmpc_solve_grid_no_jerk  <- st_cy.solve_s_t_path_no_jerk_fast / _djikstra   st_cy.pyx:96-312 (call site st.py:751)
 *   stmpc_build_grid          <- st.find_s_t_obstacles_from_state    st.py:25-70
 *   stmpc_solve_batch[_device]<- st.get_appropriate_base_st_path_and_obstacles (st.py:726-754) applied to N
 *                                independent HighwayState's (prediction.py:9-20), plus the path-distance probe of
 *                                st.test_guaranteed_crash_from_state (st.py:790-802)
 *   stmpc_predict_batch       <- HighwayState.predict_step_with_ego / predict_step_without_ego (prediction.py:22-105)
 *   stmpc_finer_fit_batch     <- st.finer_fit                        st.py:584-723 (QP via cvxopt.solvers.qp, st.py:16-17,722)
 *   stmpc_st_control_batch[_device] <- st.do_st_control              st.py:757-783 applied to N independent states
 *   stmpc_rollout_step_device / stmpc_combined_decide_device <- dqn.RLAgent.do_combined_control  dqn.py:117-200 (the policy
 *                                network stays the caller's; everything around it runs here)
 *   stmpc_first_step[_device] <- st.do_conditional_st_based_on_first_step  st.py:805-814 (one predictor step, the feasibility probe, the controller on takeover)
 *   stmpc_speed_from_jerk_device <- control.get_ego_speed_from_jerk   control.py:160-171
 *   stmpc_policy_features_device <- dqn.get_state_vector_from_base_state  dqn.py:389-446 (+ the float32 cast and TimeFeature input of ddpg.py:41,84)
 *   stmpc_actor_eval_device   <- DDPGAgent.get_control                ddpg.py:83-87 (state vector + the pretrained policy network, one launch)
 *   stmpc_actor_view_ddpg     <- the closing `evaluate` of ddpg.train_ddpg_all_with_lr_drop (the model just trained, evaluated where it lies)
 *   stmpc_qactor_eval_device  <- DQNAgent.get_control                 dqn.py:375-380 (state vector + Q-network + argmax + JERK_VALUES_DQN[a], one launch)
 *   stmpc_pop_qactor_*        <- DQNAgent.get_control for several models  dqn.py:375-380, one launch
 *   stmpc_c51actor_*          <- DQNAgent.get_control's job for RainbowAgent's categorical head  dqn.py:375-380, rainbow.py, one launch
 *   stmpc_actor_pop_*         <- DDPGAgent.load + get_control for several MODEL_NAMEs (ddpg.py:38-44, 83-87; configs/combined_<traffic>_{1,2,3}.json), one launch
 *   stmpc_env_*               <- merge_gym.JerkEnv / ContinuousJerkEnv / AccelerationEnv  merge_gym.py:15-221 with the rewards of
 *                                dqn.get_reward_function (dqn.py:449-563, rl.py:168-174), batched on the SUMO-free world (stmpc_sim_*)
 *   stmpc_rec_*               <- the per-tick histories of control.run_episode (control.py:247-254, 280-289), the position bins of
 *                                stats.StatsAggregator (stats.py:33-52) and RLAgent.plot_st_proportion (dqn.py:101-115, 215-226), and the
 *                                crash dump of st.evaluate_st_and_dump_crash (st.py:822-824, stats.py:75-77)
 *   stmpc_ego_s               <- control.get_ego_s                  control.py:373-380
 *   stmpc_num_s / stmpc_num_t <- the np.arange sizes at st.py:31-32
 *
 * Plain pointers and sizes only; no torch / numpy types.  All floating point is
 * IEEE fp64.  Functions return 0 on success or a negative STMPC_E* code;
 * stmpc_last_error() returns a thread-local message for the last failure.
 * The library has no CPU fallback: without a HIP device every compute entry
 * returns STMPC_ENODEV.
 *
 * Concurrency: a context owns one set of scratch buffers, work counters and overflow queues; AT MOST ONE batched call may be
 * in flight per context (calls on one stream are naturally ordered; calls on different streams, or from different host
 * threads, need a context each).  The "_device" entries are asynchronous with respect to the host -- with these exceptions: the first
 * wide-lattice solve with a set of dynamics / cost parameters builds a small table on the host (a few ms; its upload is queued on the call's
 * stream, so that call cannot be captured in a hipGraph) -- the context keeps the tables of the four most recent parameter sets, so alternating
 * sets neither rebuild nor wait, and only a fifth set waits for the device (hipDeviceSynchronize) before it replaces the least recently used;
 * and stmpc_combined_decide_device / stmpc_first_step_device with sparse_control (one integer comes back to the host, see stmpc_combined_cfg).
 * Environment knobs (STMPC_*) are read once, in stmpc_create.
 * Scratch: back-pointers (one byte per lattice cell of a window and time layer -- the distance to the predecessor -- when no step of the dynamics
 * exceeds 255 cells, else two) live per RESIDENT workgroup (84 MB for the first window's 1024 workgroups at H = 40).  Only a search that overflows
 * the first window keeps anything of its own: an entry of a pool (an eighth of the batch, at least 256 entries; 104 KB each at H = 40: 53 MB for
 * 4096 episodes) that receives its back-pointer rows and the layer it continues from in the next window.  The pool is taken only while it is at most
 * a quarter of the device memory that is free at the time (hipMemGetInfo); without it, or beyond its capacity, overflowing searches start over in
 * the wider window instead of continuing (stmpc_stats: resume_refused, pool_exhausted) -- results are the same bits.
 *
 * Arithmetic contract.  Every operation of the reference's search (st_cy.pyx:34-93) is evaluated as one IEEE-754 fp64 operation in the
 * reference's order; the library is built with FP contraction off.  Two kinds of division are formed without the hardware's division
 * sequence, and both return the correctly rounded quotient, i.e. the same bits as `x / d`:
 *   - by the lattice step (per episode): q = x*r, two residual corrections q += fma(-q, d, x)*r with r = RN(1/d) (Markstein);
 *   - by dt, dt^2, dt^3 (per launch): fma(x, zh, x*zl) with zh = RN(1/d), zl = RN(1/d - zh), used only after stmpc_fastdiv2_check has
 *     enumerated every significand of x whose quotient lies within the sequence's error (2^-105 relative) of a rounding midpoint and
 *     has run the sequence on each of them; a divisor that fails (about one in a hundred; 0.3, 0.09, 0.027 pass) gets the kernels
 *     that divide.  Precondition of that proof: x*zl must not underflow, |x| >~ 1e-290; the dividends here are lattice coordinate
 *     differences (multiples of ~1e-2 m up to a few hundred metres, or exactly 0, for which both forms give 0), so this cannot occur.
 *   Results are bit-identical whichever form runs (STMPC_FASTDIV=0 forces the dividing kernels; the test suite runs both).
 * The bounding pre-pass that precedes the exact search works in single precision; it only supplies an upper bound that the exact
 * pass re-checks (a bound that turns out too low is raised and the pass repeated), so it cannot influence any output bit.
 * Limits the reference does not have: STMPC_QP_NMAX = 64 fine samples in st.finer_fit / st.do_st_control -- the fine grid has
 * floor((len - 1) * dt / tick) + 1 samples, so e.g. H = 40 with dt / tick = 1.5 (59 samples) is accepted and H = 44 at that ratio
 * (65) is refused: fine_len = -1 for that state, reported by stmpc_check_error / stmpc_combined_read_state as STMPC_EINVAL;
 * STMPC_KMAX_LIMIT = 32 vehicles per state; STMPC_S_LIMIT lattice cells (16-bit back-pointers).
 *
 * Errors detected on the device (an impossible solver state, a refused QP) are latched in the context: the asynchronous `_device`
 * entries cannot return them, so call stmpc_check_error at the next point where the host synchronises anyway (stmpc_get_stats,
 * stmpc_combined_read_state and the host-pointer entries do it themselves).
 */
#ifndef STMPC_H
#define STMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STMPC_ABI_VERSION 8   /* bumped whenever an exported signature, a struct layout or the accepted values of a field change (6: stmpc_sim_cfg.yield_overlap must be 2;
                                 7: the vector environment stmpc_env_*; 8: the DDPG learner stmpc_ddpg_*); see stmpc_abi_version() */

#define STMPC_OK        0
#define STMPC_EINVAL   -1   /* bad argument (NULL, size, Kmax/H/S out of range) */
#define STMPC_ENODEV   -2   /* no HIP device / device init failed */
#define STMPC_EHIP     -3   /* a HIP runtime call failed (message has hipGetErrorString) */
#define STMPC_ENOMEM   -4   /* device allocation failed */
#define STMPC_EINTERNAL -5  /* solver reported an impossible state (should not happen) */

#define STMPC_KMAX_LIMIT 32   /* max other vehicles per state */
#define STMPC_H_LIMIT    64   /* max time layers */
#define STMPC_S_LIMIT    65000 /* max position cells (back-pointers are 16-bit) */

/* Settings.* that parameterise the path (config.py:30-37,94-110,143,150).  Field
 * order = st.py:727-734 (grid) then the 11 tunables in st_cy.solve_s_t_path_fast's
 * positional order (st.py:740-746) then grid/predictor constants. */
typedef struct stmpc_params {
    double future_s;        /* Settings.FUTURE_S */
    double ds;              /* Settings.S_DISCRETIZATION */
    double dt;              /* Settings.T_DISCRETIZATION */
    double future_t;        /* Settings.FUTURE_T */
    double start_unc;       /* Settings.START_UNCERTAINTY */
    double unc_per_s;       /* Settings.UNCERTAINTY_PER_SECOND */
    double d_w, v_w, a_w, j_w;      /* D/V/A/J_WEIGHT */
    double v_des;           /* DESIRED_SPEED */
    double v_max;           /* MAX_SPEED */
    double a_min, a_max;    /* MAX_NEGATIVE_ACCELERATION, MAX_POSITIVE_ACCELERATION */
    double j_min, j_max;    /* MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK */
    double min_allowed;     /* MIN_ALLOWED_DISTANCE */
    double car_length;      /* CAR_LENGTH */
    double crash_min_s;     /* CRASH_MIN_S */
    double max_pred_decel;  /* MAX_PREDICTED_DECELERATION */
    double follow_gap;      /* literal 30 at prediction.py:85 */
    double react_thr;       /* HighwayState.ego_reaction_threshold (prediction.py:11) */
    double crash_thr;       /* HighwayState.ego_crash_threshold (prediction.py:12) */
    double comb_min_dist;   /* COMBINATION_MIN_DISTANCE */
} stmpc_params;

/* Per-launch solver statistics (filled by stmpc_get_stats after a batch solve). */
typedef struct stmpc_stats {
    int64_t episodes;        /* N of the last batch */
    int64_t fast_path;       /* episodes finished by the LDS-resident kernel */
    int64_t fallback;        /* episodes whose reachable span overflowed the first LDS window (re-solved in a larger one) */
    int64_t hbm_tier;        /* of those, episodes that ended in the HBM-scratch tier */
    int64_t retries;         /* exact passes repeated because the pre-pass bound was below the reference's terminal cost */
    int64_t nodes_exact;     /* lattice nodes expanded by the exact passes (all tiers, incl. repeated work) */
    int64_t nodes_bound;     /* lattice nodes expanded by the bounding pre-passes */
    double  solve_ms;        /* device time of the last batch (HIP events on the launch stream) */
    double  dp_kernel_ms;    /* device time of the LDS lattice-DP kernel launches (all LDS tiers) */
    int64_t guided;          /* episodes whose bound came from the guided attempt (a tube around the unobstructed optimum) */
    int64_t resume_refused;  /* 1: the batch wanted per-episode back-pointers + checkpoints (an overflowing search then continues in the wider window instead of
                                starting over) and the memory rule turned them down -- they are taken only while they are at most a quarter of the device memory
                                free at that moment (a process shared with torch / RCCL).  Same results, another schedule; re-priced every 64th call. */
    int64_t pool_exhausted;  /* overflowing searches that found the checkpoint pool (an eighth of the batch, at least 256 entries) exhausted and started over in the
                                wider window instead of continuing: same results, more work */
} stmpc_stats;

/* Totals over the launches issued between stmpc_profile(ctx, 1, ..) and stmpc_profile(ctx, 0, &totals). */
typedef struct stmpc_profile_totals {
    int64_t launches;        /* stmpc_solve_batch_device calls */
    int64_t episodes;        /* sum of N */
    double  solve_ms;        /* sum of device time, predictor + DP + second tier (HIP events on the launch stream) */
    double  dp_kernel_ms;    /* sum of device time of the LDS lattice-DP kernel launches (all LDS tiers) */
} stmpc_profile_totals;

typedef struct stmpc_ctx stmpc_ctx;

/* Library / device identification, e.g. "stmpc 0.1 hip gfx950 AMD Instinct MI355X cu=256". */
const char *stmpc_backend_info(void);
const char *stmpc_last_error(void);
/* STMPC_ABI_VERSION the library was built with: a binding compares it with the header it was written against before calling anything else. */
int stmpc_abi_version(void);

/* Context = one HIP device + its staging/scratch buffers.  device < 0 -> current device. */
int  stmpc_create(stmpc_ctx **out, int device);
void stmpc_destroy(stmpc_ctx *ctx);

/* Host-side exact helpers (same libm calls as the reference's Python). */
double stmpc_ego_s(double x, double y);                               /* control.py:373-380 */
int    stmpc_num_s(const stmpc_params *p, double start_s);            /* len(np.arange(...)) st.py:31 */
int    stmpc_num_t(const stmpc_params *p);                            /* len(np.arange(...)) st.py:32 */
double stmpc_path_mean_abs_jerk(const double *s_sequence, int n, double v0, double a0, double dt); /* st.py:274-288 */

/*
 * Batched solve, DEVICE pointers (the hot path; inputs already resident in HBM).
 *   ego      [N][5]     x, y, speed, acceleration, start_s (= get_ego_s(x,y), see stmpc_ego_s)
 *   k_count  [N]        number of other vehicles of each state (<= Kmax), front->back order
 *   other_x  [N][Kmax]  other_xs   (prediction.py:138-141 ordering), entries >= k_count ignored
 *   other_v  [N][Kmax]  other_speeds
 * outputs (any of path_dist / crash may be NULL):
 *   path_idx [N][H]     s index per layer, -1 past best_t   (s_sequence[t] = s_values[path_idx[t]], 0.0 past best_t)
 *   best_t   [N]        deepest layer reached (H-1 = success)            st_cy.pyx:365-369
 *   cost     [N]        accumulated cost of the terminal node (dropped by the reference at st_cy.pyx:393-399)
 *   path_dist[N][H]     distances[t, int((s_t - s_0)/delta_s)] along the path, NaN past best_t   st.py:797-799
 *   crash    [N]        st.test_guaranteed_crash_from_state's verdict    st.py:790-802
 * stream is a hipStream_t (NULL = default stream).  Asynchronous w.r.t. the host.
 */
int stmpc_solve_batch_device(stmpc_ctx *ctx, const stmpc_params *p, int N, int Kmax,
                             const double *d_ego, const int32_t *d_k_count,
                             const double *d_other_x, const double *d_other_v,
                             int32_t *d_path_idx, int32_t *d_best_t, double *d_cost,
                             double *d_path_dist, int32_t *d_crash, void *stream);

/* The same solve with one more output for the multi-GPU gather: action_cost [N][2] fp64 = (path_idx[i][1] as a double -- the cell
 * of the first step, the "action", -1.0 if the path ends at the start cell --, cost[i]) written by the solver's back-track itself, so that the
 * sharded step hands ONE buffer to ONE collective without a packing pass.  d_action_cost may be NULL (= stmpc_solve_batch_device). */
int stmpc_solve_batch_device_ac(stmpc_ctx *ctx, const stmpc_params *p, int N, int Kmax,
                                const double *d_ego, const int32_t *d_k_count,
                                const double *d_other_x, const double *d_other_v,
                                int32_t *d_path_idx, int32_t *d_best_t, double *d_cost,
                                double *d_path_dist, int32_t *d_crash, double *d_action_cost, void *stream);

/* Same with HOST pointers: stages H2D, solves, copies back, synchronises. */
int stmpc_solve_batch(stmpc_ctx *ctx, const stmpc_params *p, int N, int Kmax,
                      const double *ego, const int32_t *k_count,
                      const double *other_x, const double *other_v,
                      int32_t *path_idx, int32_t *best_t, double *cost,
                      double *path_dist, int32_t *crash);

int stmpc_get_stats(stmpc_ctx *ctx, stmpc_stats *out);

/* Synchronises the device and returns (and clears) what the kernels of earlier calls on this context flagged: STMPC_EINTERNAL if a
 * solver kernel met an impossible state (e.g. a queue entry that never appeared: that episode's output rows are then stale),
 * STMPC_EINVAL if st.do_st_control could not re-sample a path (more than STMPC_QP_NMAX fine samples: that state's commanded speed is
 * not valid), else STMPC_OK. */
int stmpc_check_error(stmpc_ctx *ctx);

/* enable != 0: start timing every subsequent stmpc_solve_batch_device launch with its own HIP events (no host
 * synchronisation is added to the launches).  enable == 0: wait for those launches, sum their device times into
 * *out (may be NULL) and stop.  While profiling, stmpc_get_stats reports nothing new. */
int stmpc_profile(stmpc_ctx *ctx, int enable, stmpc_profile_totals *out);

/*
 * Single-episode entry with materialised grids: st_cy.solve_s_t_path_fast's exact
 * argument meaning (st_cy.pyx:315).  HOST pointers.  obstacles [H][S] bytes
 * (non-zero = blocked), distances [H][S], s_values [S], t_values [H];
 * s_sequence_out [H] receives s along the path, 0.0 past the deepest layer reached.
 * Requires H >= 2, S >= 2 (the reference reads s_values[1], t_indices[1] unconditionally).
 */
int stmpc_solve_grid(stmpc_ctx *ctx, const uint8_t *obstacles, const double *s_values, int S,
                     const double *t_values, int H, double ego_start_speed,
                     double ego_start_acceleration, const double *distances,
                     double d_weight, double v_weight, double a_weight, double j_weight,
                     double desired_speed, double max_speed, double negative_acceleration_limit,
                     double positive_acceleration_limit, double negative_jerk_limit,
                     double positive_jerk_limit, double min_allowed_distance,
                     double *s_sequence_out);

/*
 * The reference's two non-production solvers on materialised grids (HOST pointers), same grid arguments as stmpc_solve_grid:
 *   variant 0 <- st_cy.solve_s_t_path_no_jerk_fast      st_cy.pyx:209-312   (node = (t, s))
 *   variant 1 <- st_cy.solve_s_t_path_no_jerk_djikstra  st_cy.pyx:96-206    (node = (t, s, s_prev); the USE_FAST_ST_SOLVER = False
 *                                                                           dispatch of st.py:749-753; needs H*S*S <= 2^28)
 * Both use the constants compiled into the reference's st_cy module (st_cy.pyx:21-31), not Settings.
 */
int stmpc_solve_grid_no_jerk(stmpc_ctx *ctx, int variant, const uint8_t *obstacles, const double *s_values, int S,
                             const double *t_values, int H, double ego_start_speed, const double *distances,
                             double *s_sequence_out);

/*
 * st.find_s_t_obstacles_from_state for one state (HOST pointers): fills
 * obstacles [H][S] (0/1), distances [H][S], s_values [S], t_values [H] with
 * S = stmpc_num_s(p, start_s), H = stmpc_num_t(p).  state5 = x, y, v, a, start_s.
 */
int stmpc_build_grid(stmpc_ctx *ctx, const stmpc_params *p, const double *state5, int k,
                     const double *other_x, const double *other_v,
                     uint8_t *obstacles, double *distances, double *s_values, double *t_values);

/*
 * Batched one-step traffic prediction (HOST pointers), prediction.py:22-105.
 *   mode 0: predict_step_with_ego(selected_speed[i], dt, min_crash_distance)
 *   mode 1: predict_step_without_ego(dt, min_crash_distance)   (selected_speed ignored, may be NULL)
 * state layout as in stmpc_solve_batch but ego is [N][4] = x, y, v, a.  Outputs have the same
 * shapes; crashed [N] receives the crash flag.  stmpc_predict_batch_acc additionally returns other_a_out [N][Kmax] (may be NULL),
 * the new_other_accelerations of prediction.py:86-89,97 (the deceleration applied to a following vehicle, else 0) -- what the RL
 * state vector reads (dqn.get_state_vector_from_base_state, dqn.py:400).  (ABI 2 had given stmpc_predict_batch itself that
 * trailing parameter; ABI 3 restores its original signature and adds the _acc entry.)
 */
int stmpc_predict_batch(stmpc_ctx *ctx, const stmpc_params *p, int mode, int N, int Kmax,
                        const double *ego4, const int32_t *k_count, const double *other_x,
                        const double *other_v, const double *selected_speed, double dt,
                        double min_crash_distance, double *ego4_out, double *other_x_out,
                        double *other_v_out, int32_t *crashed);
int stmpc_predict_batch_acc(stmpc_ctx *ctx, const stmpc_params *p, int mode, int N, int Kmax,
                            const double *ego4, const int32_t *k_count, const double *other_x,
                            const double *other_v, const double *selected_speed, double dt,
                            double min_crash_distance, double *ego4_out, double *other_x_out,
                            double *other_v_out, int32_t *crashed, double *other_a_out);

#define STMPC_QP_NMAX     64   /* max fine samples of st.finer_fit (one wavefront lane per sample) */
#define STMPC_QP_MAXITERS 10   /* solvers.options['maxiters'] = 10, st.py:17 */

/*
 * st.finer_fit (st.py:584-723), batched, HOST pointers: re-samples coarse ST paths (planning step coarse_delta_t)
 * to the simulator tick delta_t by the reference's QP: minimise |x - interp(s)|^2 subject to x_0 = s_0 and speed /
 * acceleration / jerk limits written as finite differences (limits from p: v_max, a_max, a_min, j_max, j_min),
 * solved with cvxopt's coneqp iteration capped at maxiters (the reference uses STMPC_QP_MAXITERS).
 *   s_seq   [N][Hs]  coarse paths, row i valid for len[i] entries (1 <= len[i] <= Hs <= 64)
 *   v0, a0  [N]      start_speed, start_acceleration
 *   bac     [N][4] or NULL: before_s, before_speed, after_s, after_speed (st.py:672-702; +-inf = no such car)
 *   out     [N][n_max] fine paths;  out_len [N] their lengths: 1 when len[i] == 1 (returned as is, st.py:587-588),
 *           -1 when the fine grid would have more than STMPC_QP_NMAX samples (nothing written)
 *   iters   [N] or NULL: iterations done, negated when the cap was reached without meeting cvxopt's tolerances
 */
int stmpc_finer_fit_batch(stmpc_ctx *ctx, const stmpc_params *p, double delta_t, double coarse_delta_t, int maxiters,
                          int N, int Hs, const double *s_seq, const int32_t *len, const double *v0, const double *a0,
                          const double *bac, int n_max, double *out, int32_t *out_len, int32_t *iters);

/*
 * st.do_st_control (st.py:757-783) for N states: lattice search, trailing-zero trim, QP re-sampling when
 * tick_length < p->dt (st.py:771-772), commanded speed (x_1 - x_0) / tick_length, or the current speed when the
 * path has a single point (st.py:775-777).  Inputs as stmpc_solve_batch.  Outputs: speed [N]; best_t [N]
 * (best_t < H-1 <=> "ST Solver finds crash inevitable", st.py:765-766); optional path_idx [N][H], cost [N],
 * fine [N][STMPC_QP_NMAX] + fine_len [N] (the re-sampled path).  The _device form takes device pointers
 * (path_idx, best_t, cost required as scratch) and is asynchronous on `stream`.
 */
int stmpc_st_control_batch(stmpc_ctx *ctx, const stmpc_params *p, double tick_length, int N, int Kmax,
                           const double *ego, const int32_t *k_count, const double *other_x, const double *other_v,
                           double *speed, int32_t *best_t, int32_t *path_idx, double *cost, double *fine,
                           int32_t *fine_len);
int stmpc_st_control_batch_device(stmpc_ctx *ctx, const stmpc_params *p, double tick_length, int N, int Kmax,
                                  const double *d_ego, const int32_t *d_k_count, const double *d_other_x,
                                  const double *d_other_v, int32_t *d_path_idx, int32_t *d_best_t, double *d_cost,
                                  double *d_speed, double *d_fine, int32_t *d_fine_len, void *stream);

/*
 * Combined RL + ST controller, dqn.RLAgent.do_combined_control (dqn.py:117-200), for N independent states, DEVICE pointers.
 * The policy network is the caller's: it proposes one jerk per live episode and rollout step (dqn.py:119,132).  Protocol per tick:
 *   for step = 1 .. max(rollout_length, 1):
 *       action[N] = policy(current state arrays)              (caller, on the device; step 1 uses first_action)
 *       stmpc_rollout_step_device(.., step, ..)               speed from jerk (control.py:160-171), predict_step_with_ego with
 *                                                             COMBINATION_MIN_DISTANCE (dqn.py:136), history / probe-state bookkeeping;
 *                                                             episodes whose rollout ended (crash predicted, x > STOP_X) are left untouched
 *   stmpc_combined_decide_device(..)                          feasibility probe of the rolled-out state (one batched solve), controller solve of
 *                                                             the start state (lattice search + QP re-sampling), decision rules of dqn.py:144-200
 * Outputs: takeover [N] (what the reference appends to takeover_history), reason [N] (0 policy kept, 1 crash predicted, 2 policy too fast,
 * 3 probe rejects the rolled-out state, 4 ST path deemed better), speed [N] (the commanded speed: st.do_st_control's for reasons 1-3, the first
 * re-sampled step for 4, control.get_ego_speed_from_jerk(first_action) for 0).  cur_* arrays are updated in place by the rollout steps;
 * cur_oa [N][Kmax] (may be NULL) receives the other vehicles' accelerations for the policy's state vector.  The rollout history's
 * s coordinates of predicted positions come from the device map of control.get_ego_s (squares as x*x where CPython calls pow).
 */
#define STMPC_ROLLOUT_LIMIT 63
typedef struct stmpc_combined_cfg {
    double tick_length;              /* Settings.TICK_LENGTH */
    double stop_x;                   /* Settings.STOP_X */
    int32_t rollout_length;          /* Settings.ROLLOUT_LENGTH */
    int32_t st_test_rollouts;        /* Settings.ST_TEST_ROLLOUTS */
    int32_t check_rollout_crash;     /* Settings.CHECK_ROLLOUT_CRASH */
    int32_t limit_dqn_speed;         /* Settings.LIMIT_DQN_SPEED */
    int32_t test_rollout_state;      /* Settings.TEST_ROLLOUT_STATE */
    int32_t test_st_strictly_better; /* Settings.TEST_ST_STRICTLY_BETTER */
    int32_t remember_last_choice;    /* Settings.REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED */
    int32_t sparse_control;          /* not a reference flag.  1: like the reference, st.do_st_control(start_state) is solved only for the states whose decision hands
                                        control over (dqn.py:144-155) -- the decide call then makes ONE host round trip (the number of those states) and is no longer
                                        capturable in a hipGraph; ignored (all states are solved) when test_st_strictly_better needs every state's path.  0: all states,
                                        fully asynchronous.  Same decisions and commands either way. */
} stmpc_combined_cfg;
int stmpc_rollout_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_combined_cfg *cfg, int N, int Kmax, int step,
                              const double *d_ego5_start, double *d_cur_ego4, const int32_t *d_k_count, double *d_cur_other_x,
                              double *d_cur_other_v, double *d_cur_other_a, const double *d_action, void *stream);
int stmpc_combined_decide_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_combined_cfg *cfg, int N, int Kmax,
                                 const double *d_ego5_start, const int32_t *d_k_count, const double *d_other_x_start,
                                 const double *d_other_v_start, const double *d_cur_ego4, const double *d_cur_other_x,
                                 const double *d_cur_other_v, const double *d_first_action, const int32_t *d_last_choice_rl,
                                 int32_t *d_takeover, int32_t *d_reason, double *d_speed, void *stream);
/* Decisions taken by stmpc_combined_decide_device on this context and controller solves run for them (equal unless sparse_control). */
int stmpc_combined_counts(stmpc_ctx *ctx, int64_t *decisions, int64_t *control_solves, int reset);

/*
 * The policy network's input for N states on the device: dqn.get_state_vector_from_base_state (dqn.py:389-446: the nearest cars_ahead /
 * cars_behind vehicles in list order as (acceleration, speed [difference], gap, 1), zero tuples where there are fewer, then ego speed,
 * acceleration, x, y; normalised by 9, MAX_SPEED, SENSOR_RADIUS, 300, 100), cast to float32 as the gym wrapper of the reference's RL
 * library hands it to the network (ddpg.py:84: env._make_state), plus, if time_feature, the 21st input of ddpg.py:41 (TimeFeature of
 * autonomous-learning-library 0.5.3): time_scale x d_evals[i] (policy evaluations of that episode so far), after which d_evals[i] counts
 * one up -- for step > 1 only where the context's rollout (stmpc_rollout_step_device) is still going on, because the reference only asks
 * its policy for those states.  The cast and the time feature restate a library that is absent from the reference checkout (parity
 * unpinned); the other 20 entries are pinned to the reference's own function (tests/golden/golden_combined_real.npz).
 * d_feat [N][feat_stride] float32, feat_stride >= stmpc_policy_features_len(cfg).  d_cur_oa may be NULL (accelerations read as 0).
 */
typedef struct stmpc_policy_features_cfg {
    double max_speed;                /* Settings.MAX_SPEED */
    double sensor_radius;            /* Settings.SENSOR_RADIUS */
    double time_scale;               /* TimeFeature.scale: 0.001 */
    int32_t cars_ahead, cars_behind; /* Settings.CARS_AHEAD, Settings.CARS_BEHIND */
    int32_t use_acceleration;        /* Settings.USE_ACCELERATION_OF_OTHER_CARS */
    int32_t use_speed_difference;    /* Settings.USE_SPEED_DIFFERENCE */
    int32_t normalize;               /* Settings.NORMALIZE_VECTOR_INPUT */
    int32_t time_feature;            /* 1: append the TimeFeature input (DDPG agents, ddpg.py:41) */
} stmpc_policy_features_cfg;
int stmpc_policy_features_len(const stmpc_policy_features_cfg *cfg);
int stmpc_policy_features_device(stmpc_ctx *ctx, const stmpc_policy_features_cfg *cfg, int N, int Kmax, int step, const double *d_cur_ego4,
                                 const int32_t *d_k_count, const double *d_cur_other_x, const double *d_cur_other_v, const double *d_cur_other_a,
                                 int32_t *d_evals, float *d_feat, int feat_stride, void *stream);

/*
 * The policy network itself on the device (optional -- a caller may keep the network in its own framework and only take the input vectors from
 * stmpc_policy_features_device): the reference's DDPGAgent.get_control (ddpg.py:83-87) for N states in ONE launch = the state vector above ->
 * Linear(n_in, h1) -> ReLU -> Linear(h1, h2) -> ReLU -> Linear(h2, 1) -> tanh * tanh_scale + tanh_mean (the `all` library's fc_deterministic_policy
 * behind ddpg.py:29-41; 21 -> 400 -> 300 -> 1, scale 5, mean 0 for the reference's pretrained_models/), float32 throughout like the reference's
 * torch modules, hidden layers on the matrix cores (v_mfma_f32_16x16x4_f32: exact f32 fused multiply-adds in a fixed order).
 * stmpc_actor_create takes HOST pointers to row-major weights as torch stores them (w0 [h1][n_in], w1 [h2][h1], w2 [h2], biases) and packs
 * them for the kernel; n_in <= 32, h1, h2 <= 1024 and small enough for one workgroup's LDS.  stmpc_actor_eval_device: arguments as
 * stmpc_policy_features_device (d_feat may be NULL) plus d_jerk [N] fp64, the proposed jerk per state.
 */
typedef struct stmpc_actor stmpc_actor;
int  stmpc_actor_create(stmpc_ctx *ctx, int n_in, int h1, int h2, const float *w0, const float *b0, const float *w1, const float *b1,
                        const float *w2, const float *b2, double tanh_scale, double tanh_mean, stmpc_actor **out);
void stmpc_actor_destroy(stmpc_actor *actor);
int  stmpc_actor_eval_device(stmpc_ctx *ctx, const stmpc_actor *actor, const stmpc_policy_features_cfg *cfg, int N, int Kmax, int step,
                             const double *d_cur_ego4, const int32_t *d_k_count, const double *d_cur_other_x, const double *d_cur_other_v,
                             const double *d_cur_other_a, int32_t *d_evals, float *d_feat, int feat_stride, double *d_jerk, void *stream);

/* Host copies of the context's rollout bookkeeping and intermediate results (synchronises; any pointer may be NULL):
 * live, hist_len, crash_pred, have_test [N]; sel_speed [N]; rollout_s [N][rollout_length + 1]; test_ego4 [N][4], test_ox / test_ov [N][Kmax];
 * probe_crash [N], st_speed [N], fine [N][STMPC_QP_NMAX], fine_len [N] (valid after stmpc_combined_decide_device; with sparse_control st_speed is NaN and
 * fine_len 0 for the states whose decision did not call the controller). */
int stmpc_combined_read_state(stmpc_ctx *ctx, int N, int32_t *live, int32_t *hist_len, int32_t *crash_pred, double *sel_speed,
                              double *rollout_s, int32_t *have_test, double *test_ego4, double *test_ox, double *test_ov,
                              int32_t *probe_crash, double *st_speed, double *fine, int32_t *fine_len);

/*
 * Batched SUMO-free merge episodes: stands in for control.run_episode / control.step (control.py:207-340) so that whole
 * episodes can be run for N environments in lock-step on the device.  The world restates what the reference configures SUMO to do
 * (the "simple traffic distribution", config.py:39): highway vehicles of vType "normal" follow SUMO's Krauss model (Euler form,
 * sigma 0) behind the vehicle ahead and behind the ego once that is on the junction, they enter as control.py:215-226 adds them,
 * the ego obeys its acceleration limits only (speed mode 22, control.py:43) and moves along `ego_route` -- the centre line of its lanes in
 * the reference's network (ramp_0 and the junction's internal lane, merge.net.xml:42,52), whose (x, y) pairs are what TraCI reports and what
 * the reference's planner and trained actors see -- or, without a route, along the straight lines the planner assumes (prediction.py:46-59).
 * It is not SUMO: episode statistics compare with the reference's reports as distributions only.
 *   stmpc_sim_init_device   traffic in its stationary state, ego at the ramp start with control.get_ego_start_speed's draw
 *   stmpc_sim_view_device   planner inputs of every environment (the layout stmpc_solve_batch_device takes; vehicles within the
 *                           sensor radius, front to back; other_a may be NULL).  Kmax: 1 ... 64, the world's vehicle slots per environment --
 *                           the solver's entries take rows of at most STMPC_KMAX_LIMIT; wider rows show the whole world (tests/test_sim_world.py)
 *   stmpc_sim_step_device   one tick with the commanded speeds (limited by the vehicle's acceleration limits); finished environments idle
 *   stmpc_sim_read          host copies: status [N] (0 running, 1 arrived = "merged", 2 crashed, 3 out of time), ticks [N], acc [N][STMPC_SIM_NACC] =
 *                           sum of speeds, max speed, sum |jerk|, (internal), samples, closest distance past CRASH_MIN_S, sum and count of those
 *                           distances; then the reference's "disruption" columns (control.py:289-304, stats.py:64-68: deceleration of the nearest
 *                           vehicle behind the ego while ego_s > disruption_min_s): sum, maximum, samples, samples with a non-zero value; and ego [N][4]
 */
#define STMPC_SIM_NACC 12
typedef struct stmpc_sim_cfg {
    double tick_length;              /* Settings.TICK_LENGTH */
    double other_car_speed;          /* Settings.OTHER_CAR_SPEED */
    double base_traffic_interval;    /* Settings.BASE_TRAFFIC_INTERVAL */
    double spawn_x, despawn_x;       /* ends of the highway edges: -250, 100 (merge.net.xml:45-49) */
    double ego_start_x, ego_start_y; /* departPos 40 on the ramp (control.py:42) */
    double arrive_x;                 /* arrivalPos 50 on highwayahead = x 51.5 (control.py:42) */
    double sensor_radius;            /* Settings.SENSOR_RADIUS */
    double start_speed, start_speed_std, min_start_speed, max_start_speed;   /* control.py:198-204 */
    /* the highway vehicles' SUMO vType (merge_impossible.rou.xml:3 "normal": Krauss, accel 4.5, decel 6.0, minGap 1, tau 0.5, length 5; SUMO's
     * defaults: emergencyDecel 9, width 1.8); speed_dev = deviation of the per-vehicle speed factor (0 in the simple distribution) */
    double veh_accel, veh_decel, veh_min_gap, veh_tau, veh_emergency_decel, veh_length, veh_width, speed_dev;
    int32_t vary_traffic_start_times, randomize_start_speed, max_ticks;
    int32_t yield_overlap;           /* must be 2 (anything else: STMPC_EINVAL).  What a highway vehicle does about an ego that is on the junction but whose rear (plus
                                        minGap) is not yet ahead of the vehicle's front -- the ego "laps in": SUMO's link-leader rule as its effect shows in the
                                        reference's "disruption" columns: a vehicle whose front is behind the ego's front is asked to STOP while the ego laps in
                                        (emergency braking, whatever the ego's speed).  Rounds 3-5 compared four other rules under the values 0, 1, 3, 4 (DESIGN.md
                                        section 9); round 6 froze the world at this one and removed them */
    uint64_t seed;
    const double *ego_route_xy;      /* HOST [ego_route_n][2]: polyline of the ego's lane centre line from the ramp's start to the junction exit, x strictly
                                        increasing (beyond its last point the ego keeps that point's y); read by stmpc_sim_init_device, which keeps a device
                                        copy for the following view / step calls.  NULL / fewer than 2 points: straight lines towards (1.5, -1.5) */
    int32_t ego_route_n;
    int32_t reserved0;
    double disruption_min_s;         /* Settings.MERGE_POINT_X (-50): the "disruption" columns are recorded while the ego's s exceeds it (control.py:289) */
} stmpc_sim_cfg;
int stmpc_sim_init_device(stmpc_ctx *ctx, const stmpc_sim_cfg *cfg, int N, void *stream);
int stmpc_sim_view_device(stmpc_ctx *ctx, const stmpc_sim_cfg *cfg, int N, int Kmax, double *d_ego5, int32_t *d_k_count,
                          double *d_other_x, double *d_other_v, double *d_other_a, void *stream);
int stmpc_sim_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *cfg, int N, const double *d_cmd_speed, void *stream);
int stmpc_sim_read(stmpc_ctx *ctx, int N, int32_t *status, int32_t *ticks, double *acc /* [N][STMPC_SIM_NACC] */, double *ego4);
/* status [N] into a DEVICE array, asynchronously on `stream`: lets a controller loop mask its own per-environment statistics to the
 * environments that are still running without a host round trip. */
int stmpc_sim_status_device(stmpc_ctx *ctx, int N, int32_t *d_status, void *stream);

/*
 * Vector environment: the reference's gym environments (merge_gym.py) for N environments of the world above, stepped in lock-step on the device.
 * One step = the env's action handling -> stmpc_sim_step_device's kernel, unchanged -> reward, terminated / truncated, observation, and for the
 * environments that finished on this tick their final observation and statistics and (autoreset) the reset to their next episode.
 *   stmpc_env_reset_device  stmpc_sim_init_device(sim_cfg) + every environment back to episode 0 (episode 0 IS that sim_init); copies the discrete
 *                           action table (HOST pointer) to the device and synchronises on `stream` for it; d_obs [N][obs_stride] float32 may be NULL
 *   stmpc_env_step_device   asynchronous, no host synchronisation.  d_action: fp64 [N] jerks (STMPC_ENV_CONTINUOUS_JERK, not clipped to the action Box:
 *                           the reference does not clip either) or int32 [N] indices into action_values (discrete modes; an index out of range
 *                           leaves that environment's speed unchanged for the tick and makes the next stmpc_check_error return STMPC_EINVAL).
 *                           Outputs: d_obs [N][obs_stride] float32 (dqn.get_state_vector_from_base_state of the new state, dqn.py:389-446, without
 *                           the TimeFeature input; zeros after a crash or an arrival, merge_gym.py:109,114; with autoreset the start state of the
 *                           next episode where one ended), d_reward [N] fp64 (the reward function + the invalid-action reward, merge_gym.py:110-135),
 *                           d_terminated / d_truncated [N] uint8 (status 1 arrived or 2 crashed / status 3 out of time); where an episode ended:
 *                           d_final_obs [N][obs_stride] (the observation the reference returns for that step) and d_final_stats
 *                           [N][STMPC_ENV_NSTAT] (acc[STMPC_SIM_NACC] as stmpc_sim_read, status, ticks, return of the episode) -- rows of the other
 *                           environments are left as they were; either may be NULL.  Without autoreset a finished environment idles: reward 0,
 *                           both flags 0, observation as on its last step.
 *                           Episode j >= 1 of environment e starts as environment e of stmpc_sim_init_device with seed stmpc_env_episode_seed(seed, j)
 *                           (every field but the draw counter, which starts j * 2^16 further on for j < 2^16 and at an offset taken from the
 *                           episode seed after that: the traffic after the reset is drawn from the run's
 *                           seed by the unchanged world step).  The reset state is the world's start state, not the reference's 20 s warm-up
 *                           (merge_gym.py:142-150).
 *   stmpc_env_reward_device the reward function alone for arbitrary batched states (replay buffers): ego4 [N][4] x, y, v, a; k [N]; other_x [N][Kmax]
 *                           front to back (Kmax <= 64; other_v / other_a are not read and may be NULL); jerk [N]; crashed / arrived [N] int32 (may be NULL)
 *   stmpc_env_drain         host copies of the statistics rows of the episodes finished since the last drain or reset ([n_rows][STMPC_ENV_LOG_COLS]: the
 *                           d_final_stats row, environment, episode index; in completion order); synchronises.  The context keeps at most
 *                           log_capacity rows; *n_dropped counts the ones it had to drop
 *   stmpc_env_episode_ticks_device  ticks of each environment's current episode (0 right after a reset; a DDPG agent's TimeFeature input) into a
 *                           DEVICE int32 [N] array, asynchronously on `stream` (one device-to-device copy)
 *   A context holds one world: stmpc_sim_init_device on it ends the environment (its step entry then returns STMPC_EINVAL until the next
 *   stmpc_env_reset_device), and the action_mode of every step must be the one of the reset (else STMPC_EINVAL).
 *   stmpc_env_episode_seed  host only: the seed of episode `episode` (0: `seed` itself; else splitmix64 of seed + episode * 0x9E3779B97F4A7C15)
 * Exactness: the action handling, rewards and observations are the reference's expressions in its operation order, except that its x ** 2
 * (a libm pow call, not correctly rounded in glibc >= 2.28) is the correctly rounded x * x here.
 */
#define STMPC_ENV_CONTINUOUS_JERK 0  /* ContinuousJerkEnv, "sumo-jerk-continuous-v0" (merge_gym.py:217-227) */
#define STMPC_ENV_JERK            1  /* JerkEnv, "sumo-jerk-v0" (merge_gym.py:99-100: action_values = JERK_VALUES_DQN) */
#define STMPC_ENV_ACCELERATION    2  /* AccelerationEnv, "sumo-accel-v0" (merge_gym.py:187-214: action_values = ACCELERATION_VALUES_DQN) */
#define STMPC_REWARD_CONTINUOUS   0  /* dqn.continuous_reward        dqn.py:463-505 */
#define STMPC_REWARD_SLOTTED      1  /* rl.slotted_reward            rl.py:168-174 */
#define STMPC_REWARD_SLOTTED_JERK 2  /* dqn.slotted_reward_with_jerk dqn.py:557-563 */
#define STMPC_REWARD_ST           3  /* dqn.st_reward                dqn.py:508-554 */
#define STMPC_ENV_MAX_ACTIONS 256
#define STMPC_ENV_NSTAT 15
#define STMPC_ENV_LOG_COLS 17
typedef struct stmpc_env_cfg {
    int32_t action_mode;             /* STMPC_ENV_* (Settings.GYM_ENVIRONMENT, config.py:12) */
    int32_t reward_function;         /* STMPC_REWARD_* (Settings.REWARD_FUNCTION, config.py:59; dqn.get_reward_function, dqn.py:449-460) */
    double tick_length;              /* Settings.TICK_LENGTH */
    double crash_reward, success_reward, time_reward;            /* Settings.CRASH_REWARD, SUCCESS_REWARD, TIME_REWARD (config.py:62-64) */
    double wt_smooth, wt_safe, wt_efficient;                     /* Settings.WT_SMOOTH, WT_SAFE, WT_EFFICIENT (config.py:66-68) */
    double alt_v_weight, alt_a_weight, alt_j_weight, alt_d_weight; /* Settings.ALT_*_WEIGHT (config.py:73-76) */
    double min_follow_distance;      /* Settings.MIN_FOLLOW_DISTANCE (config.py:71) */
    double desired_speed;            /* Settings.DESIRED_SPEED (config.py:94) */
    double car_length;               /* Settings.CAR_LENGTH */
    double invalid_action_penalty;   /* Settings.INVALID_ACTION_PENALTY (config.py:140; merge_gym.py:25) */
    double minimum_negative_jerk, maximum_positive_jerk;         /* Settings.MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK */
    double max_negative_acceleration, max_positive_acceleration; /* Settings.MAX_NEGATIVE_ACCELERATION, MAX_POSITIVE_ACCELERATION */
    double max_speed;                /* Settings.MAX_SPEED */
    const double *action_values;     /* HOST [n_action_values]: JERK_VALUES_DQN / ACCELERATION_VALUES_DQN (config.py:114-115) in index order; copied by
                                        stmpc_env_reset_device (unused by STMPC_ENV_CONTINUOUS_JERK) */
    int32_t n_action_values;
    int32_t autoreset;               /* 1: an environment whose episode ended starts its next one in the same step */
    int32_t log_capacity;            /* episode statistics rows kept between drains (0: 16 N) */
    int32_t reserved0;
    const stmpc_policy_features_cfg *features;  /* the observation (time_feature must be 0) */
} stmpc_env_cfg;
int stmpc_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg, int N, float *d_obs,
                           int obs_stride, void *stream);
int stmpc_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg, int N, const void *d_action,
                          float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs,
                          double *d_final_stats, void *stream);
int stmpc_env_reward_device(stmpc_ctx *ctx, const stmpc_env_cfg *env_cfg, int N, int Kmax, const double *d_ego4, const int32_t *d_k, const double *d_ox,
                            const double *d_ov, const double *d_oa, const double *d_jerk, const int32_t *d_crashed, const int32_t *d_arrived,
                            double *d_reward, void *stream);
int stmpc_env_drain(stmpc_ctx *ctx, int max_rows, double *rows, int64_t *n_rows, int64_t *n_dropped);
int stmpc_env_episode_ticks_device(stmpc_ctx *ctx, int N, int32_t *d_ticks, void *stream);
uint64_t stmpc_env_episode_seed(uint64_t seed, uint32_t episode);

/*
 * DDPG learner on the device, next to the vector environment: the reference's TRAIN_DDPG (ddpg.py:44-80: the `all` library's ddpg preset), restated --
 * the library is absent from the reference checkout, so parity with it is unpinned; the network shapes are those of the reference's checkpoints:
 * actor (n_obs + 1) -> h1 -> ReLU -> h2 -> ReLU -> 1 -> tanh * tanh_scale + tanh_mean, critic (n_obs + 2) -> h1 -> ReLU -> h2 -> ReLU -> 1, float32.
 * Input n_obs of both is the time feature time_scale * ticks; the critic's last input is the action.  Per update, on a minibatch of `batch` replay rows
 * (s, a, r, s', mask) drawn uniformly with replacement from the filled part of the ring:
 *   y = r + gamma * mask * Q_target(s', pi_target(s'));  critic: Adam step on mean((Q(s, a) - y)^2);  actor: Adam step on -mean(Q(s, pi(s))) with the
 *   critic after its step;  both targets: theta_target <- (1 - tau) theta_target + tau theta.
 * Every entry with a `stream` is asynchronous and never synchronises with the host: cursors, counters and Adam's state live on the device, and the
 * launch sequence depends on (batch, N, shapes) alone, so act -> stmpc_env_step_device -> push -> updates may be captured as one single-stream graph.
 *   create          seeded parameters are the caller's business: all parameters start at zero until set_params
 *   set / get_params  HOST float32, one slot at a time: STMPC_DDPG_ACTOR, _ACTOR_TARGET, _ACTOR_M, _ACTOR_V (Adam's moments), STMPC_DDPG_CRITIC, ...;
 *                   a slot is the net's tensors one after the other, row-major as torch stores them: W0 [h1][n_in] | b0 [h1] | W1 [h2][h1] | b1 [h2] |
 *                   W2 [h2] | b2 [1], n_in = n_obs + 1 (actor) or n_obs + 2 (critic); `count` must be that length.  Synchronise.
 *   set / get_state   HOST: counters int64 [STMPC_DDPG_NCOUNTERS] (ring cursor, fill, updates done, noisy acting calls, frames pushed, 0, 0, 0) and Adam's
 *                   running beta powers float32 [4] (actor beta1^t, beta2^t, critic beta1^t, beta2^t).  With the eight slots: a checkpoint (the replay
 *                   ring's contents are not part of it).  Synchronise.
 *   push_device     one environment step into the ring (N <= capacity rows at the cursor, which wraps): d_obs / d_next_obs / d_final_obs [N][obs_stride]
 *                   float32, d_ticks / d_next_ticks [N] int32 (the ticks the observation was made at), d_action / d_reward [N] fp64, d_terminated /
 *                   d_truncated [N] uint8.  Where an episode ended, s' is the d_final_obs row (if given) at ticks + 1; elsewhere d_next_obs at d_next_ticks
 *                   (NULL: ticks + 1).  mask = 0 where terminated, 1 otherwise (a truncation bootstraps).  Rows are stored as float32 [STMPC_DDPG_ROW]:
 *                   [0, 32) s, time feature, action, zeros; [32, 64) s', time feature, zeros; [64] reward; [65] mask
 *   act_device      d_action [N] fp64 = clip(pi(obs, time feature) + noise_std * gauss, action_low, action_high); noise = 0: the greedy action.  gauss is
 *                   Box-Muller on two 24-bit draws of the hash stmpc_ddpg_noise restates, keyed by (seed, noisy acting calls so far, row); d_debug (may be
 *                   NULL) uint32 [N][4]: the two draws, the bits of the float32 gauss, the bits of the float32 greedy action
 *   update_device   n_updates updates with the critic's / the actor's learning rate lr_q / lr_pi; does nothing (on the device) until more than
 *                   replay_start frames have been pushed.  Minibatch row r of update u is ring row stmpc_ddpg_sample_index of (seed, u, r, fill)
 *   grads_device    debug: the gradients of both losses on the minibatch of the current update index into d_grad_actor / d_grad_critic (DEVICE float32,
 *                   slot layout), nothing applied, no replay_start gate; both against the current, un-stepped critic
 *   stats_device    d_out DEVICE fp64 [4]: critic loss and mean Q(s, a) of the last minibatch, fill, updates done
 *   replay_read     debug, HOST: `count` ring rows from row `first` ([count][STMPC_DDPG_ROW]); synchronises.  gather_device: the minibatch of the current
 *                   update index, DEVICE [batch][STMPC_DDPG_ROW]
 *   sample_index, noise   host only, no learner: the generator.  noise returns the standard normal in fp64 and the two draws
 */
#define STMPC_DDPG_ROW 68
#define STMPC_DDPG_NCOUNTERS 8
#define STMPC_DDPG_ACTOR 0
#define STMPC_DDPG_ACTOR_TARGET 1
#define STMPC_DDPG_ACTOR_M 2
#define STMPC_DDPG_ACTOR_V 3
#define STMPC_DDPG_CRITIC 4
#define STMPC_DDPG_CRITIC_TARGET 5
#define STMPC_DDPG_CRITIC_M 6
#define STMPC_DDPG_CRITIC_V 7
typedef struct stmpc_ddpg_cfg {
    int32_t n_obs;                   /* observation entries (20 for the shipped settings; <= 30) */
    int32_t h1, h2;                  /* hidden widths (400, 300; <= 1024) */
    int32_t batch;                   /* minibatch rows B, 16 ... 8192 (100) */
    int32_t capacity;                /* replay rows */
    int32_t reserved0;
    int64_t replay_start;            /* updates start once MORE than this many frames were pushed (5000); < capacity */
    uint64_t seed;                   /* of the minibatch indices and the exploration noise */
    double gamma, tau;               /* 0.99, 0.005 */
    double beta1, beta2, eps;        /* Adam: 0.9, 0.999, 1e-8 */
    double time_scale;               /* time feature = time_scale * ticks (0.001) */
    double tanh_scale, tanh_mean;    /* the actor's squash: half the action Box's width, its centre */
    double noise_std;                /* exploration noise (0.1 * tanh_scale) */
    double action_low, action_high;  /* the action Box */
} stmpc_ddpg_cfg;
typedef struct stmpc_ddpg stmpc_ddpg;
int  stmpc_ddpg_create(stmpc_ctx *ctx, const stmpc_ddpg_cfg *cfg, stmpc_ddpg **out);
void stmpc_ddpg_destroy(stmpc_ddpg *learner);
int  stmpc_ddpg_set_params(stmpc_ddpg *learner, int slot, const float *values, int64_t count);
int  stmpc_ddpg_get_params(stmpc_ddpg *learner, int slot, float *values, int64_t count);
int  stmpc_ddpg_set_state(stmpc_ddpg *learner, const int64_t *counters, const float *beta_pow);
int  stmpc_ddpg_get_state(stmpc_ddpg *learner, int64_t *counters, float *beta_pow);
int  stmpc_ddpg_push_device(stmpc_ddpg *learner, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                            const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward,
                            const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream);
int  stmpc_ddpg_act_device(stmpc_ddpg *learner, int N, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise, double *d_action,
                           uint32_t *d_debug, void *stream);
int  stmpc_ddpg_update_device(stmpc_ddpg *learner, int n_updates, double lr_q, double lr_pi, void *stream);
int  stmpc_ddpg_grads_device(stmpc_ddpg *learner, float *d_grad_actor, float *d_grad_critic, void *stream);
int  stmpc_ddpg_stats_device(stmpc_ddpg *learner, double *d_out, void *stream);
int  stmpc_ddpg_replay_read(stmpc_ddpg *learner, int64_t first, int64_t count, float *rows);
int  stmpc_ddpg_gather_device(stmpc_ddpg *learner, float *d_rows, void *stream);
uint64_t stmpc_ddpg_sample_index(uint64_t seed, uint64_t update, uint32_t row, uint64_t fill);
double stmpc_ddpg_noise(uint64_t seed, uint64_t call, uint32_t row, uint32_t *draw1, uint32_t *draw2);

/*
 * A population of DDPG learners: P independent learners of the section above -- each its own replay ring, networks, Adam state, counters, seed and
 * constants -- sharing one vector environment and advancing with ONE launch per kernel.  The reference trains its agents as one TRAIN_DDPG run
 * (ddpg.py:44-80) per seed: the train_{traffic_type}_{seed}.json configs and the ddpg_*{1,2,...} checkpoints of pretrained_models/README.md; one
 * learner's update occupies a few workgroups of the device, and the members of a population fill the rest.  Member m owns rows
 * [m * n_per_member, (m + 1) * n_per_member) of the step tensors.  Members do not interact, and every member is bit-identical to a lone
 * stmpc_ddpg with its cfg given its slice: the noise and the minibatch indices are keyed by the member's seed, its own counters and the row LOCAL
 * to its slice.  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 *   pop_create      P = 1 ... STMPC_DDPG_POP_MAX configs that share n_obs, h1, h2, batch and capacity (the launch shapes are common); seed, replay_start,
 *                   gamma, tau, the betas, eps, noise_std, the squash and the action Box may differ per member
 *   pop_member      the m-th member as a BORROWED learner handle, valid until pop_destroy (never stmpc_ddpg_destroy it): set / get_params, set /
 *                   get_state, replay_read, grads_device, gather_device -- and the single-learner act / push / update -- work on it as on a lone learner
 *   pop_act_device / pop_push_device   stmpc_ddpg_act_device / stmpc_ddpg_push_device on tensors of P * n_per_member rows, 1 <= n_per_member <= capacity;
 *                   d_debug [P * n_per_member][4].  A member's noisy-acting counter, cursor, fill and frames are its own
 *   pop_update_device   n_updates updates of every member in six launches each; lr_q / lr_pi: HOST fp64 [n_lr], n_lr = P, member m's learning rates
 *                   (they travel as kernel arguments: no copy, no synchronisation, capturable).  A member whose replay_start gate is still shut
 *                   skips its update while the others proceed
 *   pop_stats_device    d_out DEVICE fp64 [P][4]: stmpc_ddpg_stats_device's four numbers per member
 */
#define STMPC_DDPG_POP_MAX 64
typedef struct stmpc_ddpg_pop stmpc_ddpg_pop;
int  stmpc_ddpg_pop_create(stmpc_ctx *ctx, const stmpc_ddpg_cfg *cfgs, int P, stmpc_ddpg_pop **out);
void stmpc_ddpg_pop_destroy(stmpc_ddpg_pop *pop);
int  stmpc_ddpg_pop_size(const stmpc_ddpg_pop *pop);
stmpc_ddpg *stmpc_ddpg_pop_member(stmpc_ddpg_pop *pop, int m);
int  stmpc_ddpg_pop_act_device(stmpc_ddpg_pop *pop, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise,
                               double *d_action, uint32_t *d_debug, void *stream);
int  stmpc_ddpg_pop_push_device(stmpc_ddpg_pop *pop, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs,
                                int obs_stride, const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward,
                                const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream);
int  stmpc_ddpg_pop_update_device(stmpc_ddpg_pop *pop, int n_updates, const double *lr_q, const double *lr_pi, int n_lr, void *stream);
int  stmpc_ddpg_pop_stats_device(stmpc_ddpg_pop *pop, double *d_out, void *stream);

/*
 * TD3 learner (Fujimoto et al. 2018) on the device: the DDPG learner above with two critics, clipped noise on the target action, and the actor and all
 * targets updated only every policy_delay-th update.  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION
 * stays 8.)  With u the updates done so far and the minibatch rows of stmpc_ddpg_sample_index(seed, u, r, fill), one update is
 *   eps_r = clip(target_noise_std * gauss(u, r), -noise_clip, +noise_clip), gauss as stmpc_td3_noise restates it;
 *   a'_r = clip(pi_target(s'_r) + eps_r, action_low, action_high);  y_r = r_r + gamma * mask_r * min(Q1_target(s'_r, a'_r), Q2_target(s'_r, a'_r));
 *   each critic: one Adam step on mean((Q_i(s, a) - y)^2) with lr_q, its own moments and beta powers;
 *   only if (u + 1) % policy_delay == 0: one Adam step of the actor on -mean(Q1(s, pi(s))) with the Q1 just stepped and lr_pi, then the Polyak update
 *   of the actor's and both critics' targets (the actor's beta powers advance only when it steps);  updates += 1.
 * Nothing happens until more than replay_start frames were pushed.  Every update queues the same six launches; whether it is gated or its delayed
 * half is due is decided on the device, so a chain with updates stays free of host synchronisation and capturable.  With target_noise_std = 0,
 * policy_delay = 1 and critic 2 equal to critic 1, every bit of the actor and of both critics equals stmpc_ddpg_update_device's.
 *   create          refuses policy_delay < 1, negative or non-finite noise fields and whatever stmpc_ddpg_create refuses, before any device call
 *   stmpc_td3_base  the BORROWED DDPG learner that owns the actor, critic 1, the ring and the counters, valid until stmpc_td3_destroy (never
 *                   stmpc_ddpg_destroy it).  act_device, push_device, set / get_params, set / get_state, replay_read, gather_device, stats_device
 *                   and stmpc_actor_view_ddpg work on it as on any learner; stmpc_ddpg_update_device and stmpc_ddpg_grads_device on it return
 *                   STMPC_EINVAL and change nothing (they would step critic 1 alone)
 *   set / get_params    critic 2's four slots, HOST float32 in the critic's slot layout: STMPC_TD3_CRITIC2, _CRITIC2_TARGET, _CRITIC2_M, _CRITIC2_V
 *   set / get_state     critic 2's running beta powers, HOST float32 [2]
 *   update_device   n_updates updates with the critics' / the actor's learning rate
 *   grads_device    debug, no replay_start gate, nothing applied: the actor's gradient against the current critic 1, and both critics' gradients
 *                   (DEVICE float32, slot layout)
 *   targets_device  debug: d_out DEVICE float32 [batch][5] = eps, a', Q1_target, Q2_target, y of the minibatch the next update will draw
 *   stats_device    d_out DEVICE fp64 [6]: loss of critic 1, of critic 2, mean Q1(s, a), mean Q2(s, a) of the last minibatch, fill, updates done
 *   stmpc_td3_noise host only, no learner: the standard normal in fp64 of (seed, update, row) and its two draws -- stmpc_ddpg_noise on another stream
 */
#define STMPC_TD3_CRITIC2 0
#define STMPC_TD3_CRITIC2_TARGET 1
#define STMPC_TD3_CRITIC2_M 2
#define STMPC_TD3_CRITIC2_V 3
typedef struct stmpc_td3_cfg {
    stmpc_ddpg_cfg base;             /* everything the DDPG learner takes */
    double target_noise_std;         /* smoothing noise on the target action, absolute (0.2 * tanh_scale) */
    double noise_clip;               /* its clip, absolute (0.5 * tanh_scale) */
    int32_t policy_delay;            /* the actor and the targets step every policy_delay-th update (2); >= 1 */
    int32_t reserved0;
} stmpc_td3_cfg;
typedef struct stmpc_td3 stmpc_td3;
int  stmpc_td3_create(stmpc_ctx *ctx, const stmpc_td3_cfg *cfg, stmpc_td3 **out);
void stmpc_td3_destroy(stmpc_td3 *learner);
stmpc_ddpg *stmpc_td3_base(stmpc_td3 *learner);
int  stmpc_td3_set_params(stmpc_td3 *learner, int slot, const float *values, int64_t count);
int  stmpc_td3_get_params(stmpc_td3 *learner, int slot, float *values, int64_t count);
int  stmpc_td3_set_state(stmpc_td3 *learner, const float *beta_pow2);
int  stmpc_td3_get_state(stmpc_td3 *learner, float *beta_pow2);
int  stmpc_td3_update_device(stmpc_td3 *learner, int n_updates, double lr_q, double lr_pi, void *stream);
int  stmpc_td3_grads_device(stmpc_td3 *learner, float *d_grad_actor, float *d_grad_critic1, float *d_grad_critic2, void *stream);
int  stmpc_td3_targets_device(stmpc_td3 *learner, float *d_out, void *stream);
int  stmpc_td3_stats_device(stmpc_td3 *learner, double *d_out, void *stream);
double stmpc_td3_noise(uint64_t seed, uint64_t update, uint32_t row, uint32_t *draw1, uint32_t *draw2);

/*
 * A population of TD3 learners: what the population of DDPG learners above is to stmpc_ddpg, for stmpc_td3.  P independent TD3 learners -- each its
 * own ring, actor, two critics, Adam state, counters, seed and constants, target_noise_std, noise_clip and policy_delay included -- share one vector
 * environment and advance with ONE launch per kernel: six launches per update whatever P is and whatever the members' counters say.  Member m owns
 * rows [m * n_per_member, (m + 1) * n_per_member) of the step tensors and is bit-identical to a lone stmpc_td3 with its cfg given its slice.
 * (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)  The entries read stmpc_pop_td3_*: the prefix
 * stmpc_td3_ is the lone learner's closed set of twelve.
 *   pop_create      P = 1 ... STMPC_TD3_POP_MAX configs whose bases share n_obs, h1, h2, batch and capacity; everything else may differ per member.
 *                   Each member is made by stmpc_td3_create, whose refusals (policy_delay, the noise fields, the base's) apply per member
 *   pop_member      the m-th member as a BORROWED stmpc_td3, valid until pop_destroy (never stmpc_td3_destroy it): stmpc_td3_base, set / get_params,
 *                   set / get_state, grads_device, targets_device, stats_device -- and, on its base, replay_read, stmpc_actor_view_ddpg and the
 *                   rest of what stmpc_td3_base lists -- work on it as on a lone learner
 *   pop_act_device / pop_push_device   stmpc_ddpg_pop_act_device / stmpc_ddpg_pop_push_device on the members' bases: same arguments, same noise keys
 *   pop_update_device   n_updates updates of every member; lr_q / lr_pi: HOST fp64 [n_lr], n_lr = P (they travel as kernel arguments: no copy, no
 *                   synchronisation, capturable).  A member whose replay_start gate is shut skips its update, and a member whose delayed half is
 *                   not due skips that half, while the others proceed; both are decided on the device from the member's own counters
 *   pop_stats_device    d_out DEVICE fp64 [P][6]: stmpc_td3_stats_device's six numbers per member
 * Refused with STMPC_EINVAL before any launch: P outside 1 ... 64, members that differ in a shared field, n_lr != P, a negative learning rate or
 * n_updates, n_per_member outside 1 ... capacity, NULL pointers.
 */
#define STMPC_TD3_POP_MAX 64            /* == STMPC_DDPG_POP_MAX */
typedef struct stmpc_td3_pop stmpc_td3_pop;
int  stmpc_pop_td3_create(stmpc_ctx *ctx, const stmpc_td3_cfg *cfgs, int P, stmpc_td3_pop **out);
void stmpc_pop_td3_destroy(stmpc_td3_pop *pop);
int  stmpc_pop_td3_size(const stmpc_td3_pop *pop);
stmpc_td3 *stmpc_pop_td3_member(stmpc_td3_pop *pop, int m);
int  stmpc_pop_td3_act_device(stmpc_td3_pop *pop, int n_per_member, const float *d_obs, int obs_stride, const int32_t *d_ticks, int noise,
                              double *d_action, uint32_t *d_debug, void *stream);
int  stmpc_pop_td3_push_device(stmpc_td3_pop *pop, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs,
                               int obs_stride, const int32_t *d_ticks, const int32_t *d_next_ticks, const double *d_action, const double *d_reward,
                               const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream);
int  stmpc_pop_td3_update_device(stmpc_td3_pop *pop, int n_updates, const double *lr_q, const double *lr_pi, int n_lr, void *stream);
int  stmpc_pop_td3_stats_device(stmpc_td3_pop *pop, double *d_out, void *stream);

/*
 * Prioritised replay for a lone DDPG or TD3 learner: the reference's hand-written trainer samples its minibatches from a sum tree (dqn.py:267-349,
 * class SumTree dqn.py:727-794; config.py: USE_PRIORITIZED_ER = True, PER_ALPHA 0.5, PER_MIN_PRIORITY 1e-6, PER_MAX_PRIORITY 4.0), restated.
 * (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.  A learner on which stmpc_per_enable was never
 * called computes what it computed before, bit for bit.)
 *   The tree: L = capacity rounded up to a power of two; 2L - 1 fp64 nodes, root 0, children of i at 2i + 1 and 2i + 2; ring row p is leaf p + L - 1;
 *   unfilled leaves are 0.  An internal node is always recomputed as left + right, so the tree does not depend on the order of the writes.
 *   push            the rows a push writes get leaf weight max_priority ^ alpha (in the push's own launch)
 *   sample          row r of update u: roll = uniform01 of a hash of (seed, u, r) times the root, 53 bits; descent: roll <= left goes left, else roll -=
 *                   left and right.  A leaf at or past fill, or of weight 0, is redrawn up to three times; then the row falls back to
 *                   stmpc_ddpg_sample_index.  stmpc_per_sample_index is this procedure on a HOST tree (the kernel calls the same function)
 *   weights         w_r = (fill * p_r / root) ^ -beta over the largest w of the minibatch, fp64, stored float32; the critic's loss is mean(w (Q - y)^2).
 *                   beta = 0: every w is exactly 1 (the reference applies no correction)
 *   priorities      after the critic pass: leaf[idx_r] = min(|td_r| + min_priority, max_priority) ^ alpha, td_r the float32 Q - y (TD3: of the critic with
 *                   the larger |td|, on every update); of rows with the same index the highest row wins (the reference's loop order).
 *                   alpha = 0.5 is a square root, alpha = 1 the identity, anything else pow
 * One update is two launches more than without (the sampling step, the priority update); both are gated by replay_start like the update, and every
 * counter stays on the device.  gather_device, grads_device and stmpc_td3_targets_device run the sampling step first (ungated), so they see the rows
 * the next update will read.
 *   stmpc_per_enable    on a learner whose ring is empty (a TD3 learner: on its stmpc_td3_base).  STMPC_EINVAL for min_priority <= 0, max_priority <
 *                   min_priority, alpha < 0, beta < 0, a non-empty ring, a member of a population, a second call.  Afterwards stmpc_ddpg_set_state
 *                   refuses counters that would change the ring's cursor or fill
 *   stmpc_per_tree_read     debug, HOST: `count` nodes from node `first`; synchronises
 *   stmpc_per_last_device   DEVICE int64 [batch], float32 [batch], float32 [batch]: the ring rows and weights of the last sampling step and the td of
 *                   the last critic pass
 *   stmpc_per_sample_index  host only, no learner: `leaves` = L, tree = 2L - 1 nodes; -1 for leaves not a power of two or fill outside 1 ... leaves
 */
typedef struct stmpc_per_cfg {
    double alpha;                    /* exponent of the priorities (0.5) */
    double beta;                     /* exponent of the importance weights (0: none) */
    double min_priority;             /* added to |td| (1e-6); > 0 */
    double max_priority;             /* cap of |td| + min_priority, and what new rows enter with (4.0) */
} stmpc_per_cfg;
int  stmpc_per_enable(stmpc_ddpg *learner, const stmpc_per_cfg *cfg);
int  stmpc_per_tree_read(stmpc_ddpg *learner, int64_t first, int64_t count, double *nodes);
int  stmpc_per_last_device(stmpc_ddpg *learner, int64_t *d_idx, float *d_td, float *d_weight, void *stream);
int64_t stmpc_per_sample_index(const double *tree, int64_t leaves, int64_t fill, uint64_t seed, uint64_t update, uint32_t row);

/*
 * Prioritised replay for the two populations: the section above per member, so that "prioritised against uniform" and "which alpha / beta" are sweeps
 * a population runs in one launch sequence.  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.  A
 * population on which neither entry was called launches what it launched before and computes the same bits.)  The entries read stmpc_pop_per_*: the
 * prefixes of the lone entries above and of the two populations are closed sets.
 *   cfgs HOST [P], enabled HOST uint8 [P], P = the population's size: member m gets a sum tree with cfgs[m] where enabled[m] is not 0 and keeps sampling
 *   uniformly where it is 0 (cfgs[m] is then not read); the population may mix both.  Every enabled member passes the checks of the lone enable (the
 *   cfg's ranges, an empty ring) before anything is allocated; then the members' structs change and the population's device table(s) are written anew.
 *   One call per population: STMPC_EINVAL for a second one, for P other than the population's size, NULL pointers, a cfg out of range, a ring that is
 *   not empty.  The lone enable on a borrowed member stays refused.
 * Afterwards a prioritised member is bit-identical to a lone learner with the same cfg and the lone enable, given its slice: pop_push_device sets the
 * pushed rows' leaves in the push's own launch, pop_update_device runs the sampling step in front of the critic pass and the priority update behind
 * the critic's weight gradients, one workgroup per member each -- EIGHT launches per update whatever P is, and only if at least one member is
 * prioritised (else the six of before).  Both steps are gated by the member's own replay_start.  On a borrowed member everything that follows the
 * lone enable works: the tree_read / last_device entries above, gather_device, grads_device, stmpc_td3_targets_device (each with its ungated sampling
 * step), and stmpc_ddpg_set_state's refusal to move the cursor or the fill.
 */
int  stmpc_pop_per_enable_ddpg(stmpc_ddpg_pop *pop, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P);
int  stmpc_pop_per_enable_td3(stmpc_td3_pop *pop, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P);

/*
 * DQN learner on the device for the discrete-action environments (STMPC_ENV_JERK, STMPC_ENV_ACCELERATION): the reference's hand-written trainer
 * (TRAIN_DQN: DQNAgent._train dqn.py:257-359, get_targets dqn.py:673-705, the DQN module dqn.py:566-658), restated.  (Additive: new entries only, no
 * signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8; no entry above changes what it computes.)  The Q-network is n_obs -> h1 ->
 * ReLU -> n_actions, float32, the one shape the reference trains; there is no time feature.  The replay ring, its counters, the minibatch indices
 * and prioritised replay are the DDPG learner's (rows of STMPC_DDPG_ROW float32: [0, 32) s, [32, 64) s', [64] reward, [65] mask, [66] the action
 * index).  Per update, on a minibatch of `batch` rows:
 *   double_dqn: a* = the first argmax of Q(s') (the online network), t = Q_target(s')[a*]; else t = max_a Q_target(s')[a];
 *   g = gamma * t, clipped to [clip_min, clip_max] if clip_targets;  y = r + g, and r alone where the episode terminated (mask = 0);
 *   Adam step on mean_r(w_r * smooth_l1(Q(s_r)[a_r] - y_r)), smooth_l1 with beta 1 (nn.SmoothL1Loss), w = 1 or prioritised replay's weights;
 *   after the step, if the number of updates done is a multiple of target_period: Q_target <- Q (a hard copy).
 * Three launches per update (five with prioritised replay) whose shapes depend on (batch, h1, n_actions) alone; every counter lives on the device
 * and no entry with a `stream` synchronises, so act -> step -> push -> updates may be captured as one single-stream graph.
 *   create          STMPC_EINVAL for n_actions outside 1 ... STMPC_ENV_MAX_ACTIONS, n_obs outside 1 ... 31, h1 outside 1 ... 1024, batch outside
 *                   1 ... 8192, target_period < 1, capacity < 1, replay_start outside 0 ... capacity - 1, constants out of range.  Parameters start at zero
 *   set / get_params  HOST float32, one slot at a time: STMPC_DQN_Q, _Q_TARGET, _Q_M, _Q_V (Adam's moments); a slot is W0 [h1][n_obs] | b0 [h1] |
 *                   W1 [n_actions][h1] | b1 [n_actions], row-major as torch stores them; `count` must be that length.  Synchronise
 *   set / get_state   HOST: counters int64 [STMPC_DDPG_NCOUNTERS] (ring cursor, fill, updates done, exploring acting calls, frames pushed, 0, 0, 0)
 *                   and Adam's running beta powers float32 [2].  Synchronise.  With prioritised replay the cursor and the fill cannot be moved
 *   push_device     as the DDPG learner's without ticks; d_action int32 [N], the indices given to the environment's step (an index outside
 *                   0 ... n_actions - 1, which the environment latches as out of range, is stored clamped)
 *   act_device      d_action int32 [N]: the first maximum of Q(obs) over the n_actions columns.  eps in 0 ... 1 (else STMPC_EINVAL); eps > 0 is an
 *                   exploring call: one hash per (seed, exploring calls so far, row); its top 24 bits / 2^24 are u, and where u < (float)eps the
 *                   action is the hash's next 24 bits modulo n_actions.  The call counter advances on the device.  d_debug_q (may be NULL)
 *                   float32 [N][n_actions]: Q(obs)
 *   update_device   n_updates updates with learning rate lr; does nothing (on the device) until more than replay_start frames were pushed
 *   grads_device    debug: the loss's gradient on the minibatch of the current update index (DEVICE float32, slot layout); nothing applied, no gate
 *   targets_device  debug: DEVICE float32 [batch][4] = a* (without double_dqn: the maximum's index), the target network's Q there, y, Q(s, a)
 *   gather_device   the minibatch of the current update index, DEVICE [batch][STMPC_DDPG_ROW];  stats_device: DEVICE fp64 [4]: the loss (unweighted
 *                   mean) and mean Q(s, a) of the last minibatch, fill, updates done
 *   padded_read     debug, HOST: a slot as the library keeps it -- W0 [h1p][32] | b0 [h1p] | W1 [Ap][h1p] | b1 [Ap], h1p and Ap the next multiples of
 *                   16 -- so that the pad rows and columns can be seen; slots STMPC_DQN_Q ... _Q_V, and STMPC_DQN_GRAD: the last gradient.
 *                   `count` must be 33 h1p + (h1p + 1) Ap.  Synchronises
 *   per_enable, per_tree_read, per_last_device   prioritised replay as stmpc_per_enable and its two readers provide it, on this learner's ring: the
 *                   sampling step in front of the pass, the weights on the loss, the priorities from this pass's own Q(s, a) - y, new rows at
 *                   max_priority ^ alpha
 */
#define STMPC_DQN_Q 0
#define STMPC_DQN_Q_TARGET 1
#define STMPC_DQN_Q_M 2
#define STMPC_DQN_Q_V 3
#define STMPC_DQN_GRAD 4                  /* padded_read only */
typedef struct stmpc_dqn_cfg {
    int32_t n_obs;                   /* observation entries (20 for the shipped settings; <= 31) */
    int32_t h1;                      /* hidden width (256; <= 1024) */
    int32_t n_actions;               /* A: 1 ... STMPC_ENV_MAX_ACTIONS (5: JERK_VALUES_DQN; 20: ACCELERATION_VALUES_DQN) */
    int32_t batch;                   /* minibatch rows B, 1 ... 8192 (BATCH_SIZE 50) */
    int32_t capacity;                /* replay rows (REPLAY_BUFFER_SIZE 50000) */
    int32_t target_period;           /* the target is copied on every target_period-th update (TARGET_NET_FREEZE_PERIOD 500); >= 1 */
    int32_t double_dqn;              /* DOUBLE_DQN (1) */
    int32_t clip_targets;            /* CLIP_TARGETS */
    int64_t replay_start;            /* updates start once MORE than this many frames were pushed; < capacity */
    uint64_t seed;                   /* of the minibatch indices and the exploration draws */
    double gamma;                    /* DISCOUNT_FACTOR (0.999) */
    double beta1, beta2, eps;        /* Adam: 0.9, 0.999, 1e-8 (optim.Adam's defaults) */
    double clip_min, clip_max;       /* CLIP_MIN_REWARD, CLIP_MAX_REWARD (-20, 10) */
} stmpc_dqn_cfg;
typedef struct stmpc_dqn stmpc_dqn;
int  stmpc_dqn_create(stmpc_ctx *ctx, const stmpc_dqn_cfg *cfg, stmpc_dqn **out);
void stmpc_dqn_destroy(stmpc_dqn *learner);
int  stmpc_dqn_set_params(stmpc_dqn *learner, int slot, const float *values, int64_t count);
int  stmpc_dqn_get_params(stmpc_dqn *learner, int slot, float *values, int64_t count);
int  stmpc_dqn_set_state(stmpc_dqn *learner, const int64_t *counters, const float *beta_pow);
int  stmpc_dqn_get_state(stmpc_dqn *learner, int64_t *counters, float *beta_pow);
int  stmpc_dqn_push_device(stmpc_dqn *learner, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                           const int32_t *d_action, const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream);
int  stmpc_dqn_act_device(stmpc_dqn *learner, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream);
int  stmpc_dqn_update_device(stmpc_dqn *learner, int n_updates, double lr, void *stream);
int  stmpc_dqn_grads_device(stmpc_dqn *learner, float *d_grad, void *stream);
int  stmpc_dqn_targets_device(stmpc_dqn *learner, float *d_out, void *stream);
int  stmpc_dqn_gather_device(stmpc_dqn *learner, float *d_rows, void *stream);
int  stmpc_dqn_stats_device(stmpc_dqn *learner, double *d_out, void *stream);
int  stmpc_dqn_per_enable(stmpc_dqn *learner, const stmpc_per_cfg *cfg);
int  stmpc_dqn_per_tree_read(stmpc_dqn *learner, int64_t first, int64_t count, double *nodes);
int  stmpc_dqn_per_last_device(stmpc_dqn *learner, int64_t *d_idx, float *d_td, float *d_weight, void *stream);
int  stmpc_dqn_padded_read(stmpc_dqn *learner, int slot, float *values, int64_t count);

/*
 * A population of DQN learners: what the populations of DDPG and TD3 learners above are to stmpc_ddpg and stmpc_td3, for stmpc_dqn.  P independent
 * DQN learners -- each its own ring, Q-network, target, Adam state, counters, seed and constants, double_dqn, clip_targets, target_period and
 * replay_start included -- share one discrete-action vector environment and advance with ONE launch per kernel: three launches per update whatever
 * P is and whatever the members' counters say, five when at least one member is prioritised; acting, pushing and the statistics are one launch
 * each.  Member m owns rows [m * n_per_member, (m + 1) * n_per_member) of the step tensors and is bit-identical to a lone stmpc_dqn with its cfg
 * given its slice.  The comparisons the reference runs its hand-written trainer for (TRAIN_DQN: DQNAgent._train dqn.py:257-359) -- double against
 * plain targets, clipped against unclipped ones, TARGET_NET_FREEZE_PERIOD, the epsilon schedule, prioritised against uniform replay, seeds, traffic
 * types, reward settings -- are then one run.  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8;
 * no entry above changes what it computes.)  The entries read stmpc_pop_dqn_*: the prefixes stmpc_dqn_ and stmpc_pop_per_ are closed sets.
 *   pop_create      (dqn.py:257-359) P = 1 ... STMPC_DQN_POP_MAX configs that share n_obs, h1, n_actions, batch and capacity (the launch shapes are
 *                   common); everything else may differ per member.  Each member is made by the lone create, whose refusals apply per member
 *   pop_destroy, pop_size   (dqn.py:257-359) the population with its members; the member count (0 for NULL)
 *   pop_member      (dqn.py:257-359) the m-th member as a BORROWED stmpc_dqn, valid until pop_destroy (never destroy it): set / get_params, set /
 *                   get_state, grads_device, targets_device, gather_device, stats_device, padded_read, per_tree_read, per_last_device and
 *                   stmpc_qactor_view_dqn work on it as on a lone learner, as do the lone act, push and update entries.  The lone per_enable refuses
 *   pop_act_device  (dqn.py:257-359, do_dqn_control dqn.py:661-670) the lone act_device per member: d_action int32 [P * n_per_member]; eps HOST fp64
 *                   [n_eps], n_eps = P, one value per member (it travels as a kernel argument).  Member m's exploration hash is keyed by its own
 *                   seed, its own count of exploring calls and the row local to its slice.  A member whose eps is 0 draws nothing and its
 *                   call counter stays, as a lone learner's does under eps = 0.  d_debug_q (may be NULL) float32 [P * n_per_member][n_actions]
 *   pop_push_device (dqn.py:257-359) the lone push_device per member, each slice into its member's ring (and tree, where the member has one)
 *   pop_update_device   (dqn.py:257-359, get_targets dqn.py:673-705) n_updates updates of every member; lr HOST fp64 [n_lr], n_lr = P.  A member
 *                   whose replay_start gate is shut skips its update while the others proceed, and the hard copy of the target follows the
 *                   member's own update count and target_period; both are decided on the device
 *   pop_stats_device    (dqn.py:257-359) d_out DEVICE fp64 [P][4]: the lone stats_device's four numbers per member
 *   pop_per_enable  (dqn.py:257-359, the sum tree of dqn.py:267-349, 727-794) stmpc_pop_per_enable_ddpg for this population: cfgs HOST [P], enabled
 *                   HOST uint8 [P]; one call, on empty rings; afterwards a prioritised member is bit-identical to a lone learner with the lone
 *                   per_enable, a uniform one to the member of a population without the call
 *   pop_replay_read (dqn.py:257-359) debug, HOST: `count` rows of STMPC_DDPG_ROW float32 from row `first` of a learner's ring -- a borrowed member's,
 *                   or a lone stmpc_dqn's, so that the two can be compared; synchronises
 * Refused with STMPC_EINVAL before any launch: P outside 1 ... 64, members that differ in a shared field (the message names the member), n_lr or
 * n_eps other than P, an eps outside 0 ... 1, a negative learning rate or n_updates, n_per_member outside 1 ... capacity, NULL pointers.
 */
#define STMPC_DQN_POP_MAX 64            /* == STMPC_DDPG_POP_MAX */
typedef struct stmpc_dqn_pop stmpc_dqn_pop;
int  stmpc_pop_dqn_create(stmpc_ctx *ctx, const stmpc_dqn_cfg *cfgs, int P, stmpc_dqn_pop **out);
void stmpc_pop_dqn_destroy(stmpc_dqn_pop *pop);
int  stmpc_pop_dqn_size(const stmpc_dqn_pop *pop);
stmpc_dqn *stmpc_pop_dqn_member(stmpc_dqn_pop *pop, int m);
int  stmpc_pop_dqn_act_device(stmpc_dqn_pop *pop, int n_per_member, const float *d_obs, int obs_stride, const double *eps, int n_eps,
                              int32_t *d_action, float *d_debug_q, void *stream);
int  stmpc_pop_dqn_push_device(stmpc_dqn_pop *pop, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs,
                               int obs_stride, const int32_t *d_action, const double *d_reward, const uint8_t *d_terminated,
                               const uint8_t *d_truncated, void *stream);
int  stmpc_pop_dqn_update_device(stmpc_dqn_pop *pop, int n_updates, const double *lr, int n_lr, void *stream);
int  stmpc_pop_dqn_stats_device(stmpc_dqn_pop *pop, double *d_out, void *stream);
int  stmpc_pop_dqn_per_enable(stmpc_dqn_pop *pop, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P);
int  stmpc_pop_dqn_replay_read(stmpc_dqn *learner, int64_t first, int64_t count, float *rows);

/*
 * Multi-step (n-step) returns for the three learners and their populations: the uncorrected n-step target of Rainbow (Hessel et al. 2018,
 * "Multi-step learning": R = sum_k gamma^k r_{t+k+1}, bootstrapped with gamma^n) and of D4PG (Barth-Maron et al. 2018, eq. 5), which the reference's
 * third agent (rainbow.py, the `all` library's rainbow preset with its n_steps) trains with.  (Additive: new entries only, no signature or struct of
 * ABI 8 changes, so STMPC_ABI_VERSION stays 8; the three cfg structs keep their layout, so a caller written before this section stays valid, and a
 * learner on which no enable entry was called -- or one enabled with n_step 1 -- computes what it computed before, bit for bit.  The entries read
 * stmpc_nstep_* / stmpc_pop_nstep_*: the lone learners' prefixes are closed sets.)
 *   The return is formed at sampling time from the ring itself.  A push writes its N rows at cursor + e, so the transition that follows ring row i
 *   in the same env is row (i + N) % capacity as long as every push has N rows.  age(i) = (cursor - 1 - i) mod capacity; row_k = (i + k N) % capacity
 *   exists iff age(i) >= k N.  The window of row i has length m = the smallest k + 1 (k = 0 .. n_step - 1) at which row_k is done (terminated or
 *   truncated), k + 1 == n_step, or row_{k+1} does not exist (the window ran into the ring's newest rows: a shorter return, not a refusal).
 *   R = sum_{k<m} gamma^k r(row_k) and disc = gamma^m, accumulated in fp64 from (double)(float)gamma in k order with unfused operations and rounded to
 *   float32 once; s' and the mask are row_{m-1}'s (a truncated row bootstraps from its final observation with mask 1, a terminated one has mask 0).
 *   DDPG: y = R + disc * mask * Qt(s', pi_t(s')); TD3: the same with the minimum of both target critics; DQN: g = disc * Qsel, clipped if asked,
 *   y = R + g (R alone where mask = 0).  Prioritised replay's priorities come from this target's error.  gather_device then returns row i with s'
 *   and the mask of row_{m-1} and R in the reward's column.
 *   The push of an enabled learner with n_step > 1 writes terminated || truncated into column 67 of the row (zero otherwise, as before).
 *   stmpc_nstep_enable_ddpg / _dqn   on a learner whose ring is empty (a TD3 learner: on its stmpc_td3_base).  STMPC_EINVAL for n_step outside
 *                   1 ... STMPC_NSTEP_MAX, and with n_step > 1 for rows_per_push < 1 or n_step * rows_per_push > capacity, a non-empty ring, a member of
 *                   a population.  Afterwards a push with N != rows_per_push is refused (n_step 1: any N stays legal)
 *   stmpc_pop_nstep_enable_ddpg / _td3 / _dqn   cfgs HOST [P], P = the population's size: member m gets cfgs[m], so "which n" is a sweep one population
 *                   runs; rows_per_push is the population's n_per_member.  Every member passes the lone entry's checks before any changes; then the
 *                   device tables are written anew.  A member is bit-identical to a lone learner with the same cfgs given its slice
 *   stmpc_nstep_window_ddpg / _dqn   debug, HOST: out [n_idx][4] fp64 = R, disc, the ring row of the window's last transition, m for the n_idx ring
 *                   rows idx (each a filled row, else STMPC_EINVAL), so that a test can check every live row and not a sampled subset; synchronises.
 *                   They work on a borrowed member of a population as on a lone learner
 */
#define STMPC_NSTEP_MAX 16
typedef struct stmpc_nstep_cfg {
    int32_t n_step;                  /* the window's length, 1 ... STMPC_NSTEP_MAX (1: one-step targets) */
    int32_t rows_per_push;           /* N of every push: the env's size, a population's n_per_member; read when n_step > 1 */
} stmpc_nstep_cfg;
int  stmpc_nstep_enable_ddpg(stmpc_ddpg *learner, const stmpc_nstep_cfg *cfg);
int  stmpc_nstep_enable_dqn(stmpc_dqn *learner, const stmpc_nstep_cfg *cfg);
int  stmpc_pop_nstep_enable_ddpg(stmpc_ddpg_pop *pop, const stmpc_nstep_cfg *cfgs, int P);
int  stmpc_pop_nstep_enable_td3(stmpc_td3_pop *pop, const stmpc_nstep_cfg *cfgs, int P);
int  stmpc_pop_nstep_enable_dqn(stmpc_dqn_pop *pop, const stmpc_nstep_cfg *cfgs, int P);
int  stmpc_nstep_window_ddpg(stmpc_ddpg *learner, const int64_t *idx, int n_idx, double *out);
int  stmpc_nstep_window_dqn(stmpc_dqn *learner, const int64_t *idx, int n_idx, double *out);

/*
 * Categorical (C51) DQN learner on the device for the discrete-action environments: the distributional head of the reference's third agent
 * (rainbow.py: RainbowAgent, the `all` library's rainbow preset; TRAIN_DQN / EVALUATE_DQN reach it too), after Bellemare, Dabney and Munos 2017,
 * "A Distributional Perspective on Reinforcement Learning", Algorithm 1.  (Additive: new entries only, no signature or struct of ABI 8 changes, so
 * STMPC_ABI_VERSION stays 8; no entry above changes what it computes.)  The network is n_obs -> h1 -> ReLU -> n_actions * n_atoms, float32: action
 * a's n_atoms logits are the contiguous outputs a * n_atoms ... (a + 1) * n_atoms - 1, their softmax is a distribution over the support
 * z_k = v_min + k * dz, dz = (v_max - v_min) / (n_atoms - 1), and Q(s, a) is its mean.  The replay ring, its counters, the minibatch indices,
 * prioritised replay and the multi-step window are the DQN learner's.  Per update, on a minibatch of `batch` rows:
 *   a* = the first maximum over the actions of the expected values of the online network (double_dqn) or the target network on s';
 *   p' = the target network's distribution of a* on s';  b_j = (clamp(R + disc * z_j, v_min, v_max) - v_min) / dz, R alone where the episode
 *   terminated (mask = 0); disc = gamma, or gamma^m of the multi-step window;  m_i = sum_j p'_j * max(0, 1 - |b_j - i|), j in order, in fp64;
 *   row loss l = -sum_i m_i log p_i(s, a) with the stored action a;  Adam step on mean_r(w_r * l_r), w = 1 or prioritised replay's weights;
 *   after the step, if the number of updates done is a multiple of target_period: target <- online (a hard copy).
 * The softmax is formed in fp64 from the float32 logits and rounded once.  Three launches per update (five with prioritised replay); every counter
 * lives on the device and no entry with a `stream` synchronises.  The entries mirror the DQN learner's one for one:
 *   create          STMPC_EINVAL for what the DQN learner's create refuses, and for n_atoms < 2, n_actions * n_atoms > STMPC_C51_MAX_LOGITS, v_max <=
 *                   v_min or a support that is not finite.  clip_targets, clip_min and clip_max are not read: the support's clamp is the clip
 *   set / get_params, set / get_state, push_device, gather_device, per_enable, per_tree_read, per_last_device   as the DQN learner's; a slot is W0
 *                   [h1][n_obs] | b0 [h1] | W1 [n_actions * n_atoms][h1] | b1 [n_actions * n_atoms]; slots STMPC_C51_Q ... STMPC_C51_Q_V.  The
 *                   priority of a row is its loss l (per_last_device's td is l)
 *   act_device      as the DQN learner's on the expected values: the greedy index is their first maximum; the exploration draws have the DQN
 *                   learner's stream and counter rule.  d_debug_q (may be NULL) float32 [N][n_actions]: the expected values
 *   update_device, grads_device   as the DQN learner's
 *   targets_device  debug: DEVICE float32 [batch][4] = a*, the target network's expected value there, l, Q(s, a)
 *   dist_device     debug: d_dist (may be NULL) DEVICE float32 [batch][2][n_atoms] = m and the online distribution p(s, a) of the minibatch of the
 *                   current update index; d_out (may be NULL) as targets_device's; not both NULL
 *   project_device  debug: d_m [n][n_atoms] = the projection of n caller-given distributions d_p [n][n_atoms] under d_reward, d_mask, d_disc
 *                   (float32 [n] each), by the device function the update calls
 *   stats_device    DEVICE fp64 [4]: the loss (unweighted mean of l) and mean Q(s, a) of the last minibatch, fill, updates done
 *   multi_step_enable   stmpc_nstep_enable_dqn for this learner (the stmpc_nstep_ prefix is a closed set): on an empty ring, with its refusals
 *   replay_read     debug, HOST: `count` rows of STMPC_DDPG_ROW float32 from row `first` of the ring; synchronises
 *   dzout_read      debug, HOST: the output layer's gradient of the last pass as the weight gradients read it, float32 [Bp][Ap], Bp = batch rounded up
 *                   to 16: (w / batch) (p - m) in the stored action's block, exact zeros elsewhere.  `count` must be Bp * Ap.  Synchronises
 *   padded_read     debug, HOST: a slot as the library keeps it -- W0 [h1p][32] | b0 [h1p] | W1 [Ap][h1p] | b1 [Ap], h1p and Ap the next multiples of
 *                   16 of h1 and n_actions * n_atoms; slots STMPC_C51_Q ... _Q_V, and STMPC_C51_GRAD: the last gradient.  Synchronises
 */
/*
 * The dueling head (stmpc_c51_cfg.dueling = 1): Wang et al. 2016, "Dueling Network Architectures for Deep Reinforcement Learning", in the categorical
 * form of Hessel et al. 2018, "Rainbow: Combining Improvements in Deep Reinforcement Learning", section "Dueling networks" -- the fifth of the six
 * pieces of the reference's third agent (rainbow.py: the `all` library's rainbow preset).  The head restates the published one; the library is not
 * available, so parity with its own network stays unpinned.  (`dueling` is the field ABI 8 called `reserved`, at the same offset and size, and 0
 * keeps its meaning: no signature or struct layout changes, STMPC_ABI_VERSION stays 8, and with dueling = 0 every entry computes what it computed.)
 *   network         n_obs -> h1 -> ReLU -> (n_actions + 1) * n_atoms.  The output layer holds the n_actions ADVANTAGE blocks first, where the plain
 *                   head's action blocks sit (outputs a * n_atoms ... (a + 1) * n_atoms - 1), and the VALUE block last (outputs n_actions * n_atoms
 *                   ... (n_actions + 1) * n_atoms - 1).  Ap is the next multiple of 16 of (n_actions + 1) * n_atoms
 *   logits          l[a][k] = V[k] + Adv[a][k] - (1 / n_actions) * sum_b Adv[b][k]: the float32 outputs go to fp64, the sum runs in b order, the
 *                   division and the two additions are fp64, one rounding to float32.  Everything behind the logits -- softmax, expected values,
 *                   the first maximum a*, the projection, the cross-entropy, the priorities -- is the plain head's, unchanged
 *   backward        with g[k] = (w / batch) (p[k] - m[k]) of the stored action a: advantage block b receives g[k] * ((b == a) - 1 / n_actions),
 *                   formed in fp64 and rounded once, the value block g[k]; dzout_read is then DENSE over the (n_actions + 1) * n_atoms outputs, and
 *                   its pad columns and the rows at or beyond batch are exact zeros
 *   slots           W0 [h1][n_obs] | b0 [h1] | W1 [(n_actions + 1) * n_atoms][h1] | b1 [(n_actions + 1) * n_atoms] in set / get_params and
 *                   grads_device; padded_read and dzout_read follow the padded width
 *   create          refuses (STMPC_EINVAL) a `dueling` other than 0 or 1, and with dueling = 1 (n_actions + 1) * n_atoms > STMPC_C51_MAX_LOGITS (the
 *                   message names the product and the limit).  sumo-accel-v0 has 20 actions: with a dueling head it takes at most 48 atoms (21 * 48 =
 *                   1008; 21 * 49 = 1029), where the plain head takes 51
 *   populations     the members of a stmpc_pop_c51_create share `dueling` (it sets the network's shape): a mix is refused
 *   policies        stmpc_c51actor_view of a dueling learner evaluates through the learner's own struct, head included; a policy from plain tensors
 *                   with (n_actions + 1) * n_atoms output rows is created by stmpc_dueling_c51actor_create (below the C51 policy's entries)
 */
#define STMPC_C51_Q 0
#define STMPC_C51_Q_TARGET 1
#define STMPC_C51_Q_M 2
#define STMPC_C51_Q_V 3
#define STMPC_C51_GRAD 4                  /* padded_read only */
#define STMPC_C51_MAX_LOGITS 1024         /* n_actions * n_atoms, with a dueling head (n_actions + 1) * n_atoms: the widest layer of the parameter layout */
typedef struct stmpc_c51_cfg {
    int32_t n_obs;                   /* the first sixteen fields are stmpc_dqn_cfg's, in its order */
    int32_t h1;
    int32_t n_actions;
    int32_t batch;
    int32_t capacity;
    int32_t target_period;
    int32_t double_dqn;
    int32_t clip_targets;            /* not read */
    int64_t replay_start;
    uint64_t seed;
    double gamma;
    double beta1, beta2, eps;
    double clip_min, clip_max;       /* not read */
    double v_min, v_max;             /* the support's ends (-10, 10: the C51 paper's) */
    int32_t n_atoms;                 /* K >= 2 (51) */
    int32_t dueling;                 /* 0: the plain head; 1: the dueling head (below).  The field ABI 8 called `reserved` and wanted 0 */
} stmpc_c51_cfg;
typedef struct stmpc_c51 stmpc_c51;
int  stmpc_c51_create(stmpc_ctx *ctx, const stmpc_c51_cfg *cfg, stmpc_c51 **out);
void stmpc_c51_destroy(stmpc_c51 *learner);
int  stmpc_c51_set_params(stmpc_c51 *learner, int slot, const float *values, int64_t count);
int  stmpc_c51_get_params(stmpc_c51 *learner, int slot, float *values, int64_t count);
int  stmpc_c51_set_state(stmpc_c51 *learner, const int64_t *counters, const float *beta_pow);
int  stmpc_c51_get_state(stmpc_c51 *learner, int64_t *counters, float *beta_pow);
int  stmpc_c51_push_device(stmpc_c51 *learner, int N, const float *d_obs, const float *d_next_obs, const float *d_final_obs, int obs_stride,
                           const int32_t *d_action, const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, void *stream);
int  stmpc_c51_act_device(stmpc_c51 *learner, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream);
int  stmpc_c51_update_device(stmpc_c51 *learner, int n_updates, double lr, void *stream);
int  stmpc_c51_grads_device(stmpc_c51 *learner, float *d_grad, void *stream);
int  stmpc_c51_targets_device(stmpc_c51 *learner, float *d_out, void *stream);
int  stmpc_c51_dist_device(stmpc_c51 *learner, float *d_dist, float *d_out, void *stream);
int  stmpc_c51_project_device(stmpc_c51 *learner, int n, const float *d_p, const float *d_reward, const float *d_mask, const float *d_disc, float *d_m,
                              void *stream);
int  stmpc_c51_gather_device(stmpc_c51 *learner, float *d_rows, void *stream);
int  stmpc_c51_stats_device(stmpc_c51 *learner, double *d_out, void *stream);
int  stmpc_c51_per_enable(stmpc_c51 *learner, const stmpc_per_cfg *cfg);
int  stmpc_c51_per_tree_read(stmpc_c51 *learner, int64_t first, int64_t count, double *nodes);
int  stmpc_c51_per_last_device(stmpc_c51 *learner, int64_t *d_idx, float *d_td, float *d_weight, void *stream);
int  stmpc_c51_multi_step_enable(stmpc_c51 *learner, const stmpc_nstep_cfg *cfg);
int  stmpc_c51_replay_read(stmpc_c51 *learner, int64_t first, int64_t count, float *rows);
int  stmpc_c51_dzout_read(stmpc_c51 *learner, float *values, int64_t count);
int  stmpc_c51_padded_read(stmpc_c51 *learner, int slot, float *values, int64_t count);

/*
 * The noisy output layer of the C51 learner: factorised-Gaussian noise (Fortunato et al. 2018, "Noisy Networks for Exploration"; Hessel et al. 2018,
 * "Rainbow", section "Noisy Nets") on the layer h1 -> n_out, n_out = (n_actions + dueling) * n_atoms -- the sixth piece of the reference's third
 * agent (rainbow.py: the `all` library's rainbow preset), which explores through it instead of epsilon-greedy.  It restates the published layer;
 * the library is not available, so parity with its own (its sigma0 included) stays unpinned.
 *   W_eff[n][k] = mu_W[n][k] + sigma_W[n][k] * f(e_out[n]) * f(e_in[k]),  b_eff[n] = mu_b[n] + sigma_b[n] * f(e_out[n]),  f(x) = sign(x) sqrt|x|
 * with e ~ N(0, 1), h1 + n_out of them per draw.  The learner's existing parameters ARE mu: the slots, stmpc_c51actor_view, the greedy
 * stmpc_c51_act_device and everything else that evaluates the mean network keep their meaning and their bits.  (Additive: new entries only, under a
 * prefix of their own because stmpc_c51_ is a closed set; no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8; a learner on which
 * enable never ran computes what it computed.)  Once enabled, stmpc_c51_update_device, _grads_device, _targets_device and _dist_device run the
 * noisy sequence: one update is four launches (six with prioritised replay) -- the draw and the effective parameters of the online and the target
 * net (independent draws, keyed by seed, update index and net), the pass and the weight gradients on them, then Adam on sigma (g_sigma_W = g_W *
 * f_out * f_in, g_sigma_b = g_b * f_out, moments of its own, the target's sigma copied where the hard copy runs) and on mu.  The gradient slot
 * holds the gradient with respect to the effective parameters, which is mu's.
 *   enable          (rainbow.py) on a FRESH learner: STMPC_EINVAL after a push or an update, for a second enable, for a population's member (the
 *                   message names stmpc_pop_noisy_c51_enable, behind the population's entries), and for a sigma0 that is negative or not finite.  sigma starts at sigma0 / sqrt(h1)
 *                   everywhere (0.5: the paper's).  Synchronises
 *   set / get_params    (rainbow.py) HOST float32 [n_out * h1 + n_out]: W1-shaped [n_out][h1] | [n_out], unpadded; slots STMPC_NOISY_SIGMA (the online
 *                   net's sigma), _SIGMA_TARGET, _SIGMA_M, _SIGMA_V (Adam's moments).  Synchronise
 *   act_device      (rainbow.py) stmpc_c51_act_device on a fresh ACTING draw (a stream and a counter of their own: counters[5] of get / set_state,
 *                   advanced by every call; the learning draws and the exploring-call counter do not move unless eps > 0, which is honoured)
 *   debug_read      (rainbow.py) debug, HOST: f(e_in) [h1] | f(e_out) [n_out] of the last learning draw of the online net, of the target net, and of the
 *                   last acting draw (STMPC_NOISY_F_ONLINE, _F_TARGET, _F_ACT; count h1 + n_out); their effective W1 [n_out][h1] | b1 [n_out]
 *                   (STMPC_NOISY_WEFF_ONLINE ...; count n_out * h1 + n_out); the same in the padded layout [Ap][h1p] | [Ap], pad rows and columns exact
 *                   zeros (STMPC_NOISY_WEFF_PADDED_ONLINE ...; count Ap * h1p + Ap).  Synchronises
 */
#define STMPC_NOISY_SIGMA 0
#define STMPC_NOISY_SIGMA_TARGET 1
#define STMPC_NOISY_SIGMA_M 2
#define STMPC_NOISY_SIGMA_V 3
#define STMPC_NOISY_F_ONLINE 0
#define STMPC_NOISY_F_TARGET 1
#define STMPC_NOISY_F_ACT 2
#define STMPC_NOISY_WEFF_ONLINE 3
#define STMPC_NOISY_WEFF_TARGET 4
#define STMPC_NOISY_WEFF_ACT 5
#define STMPC_NOISY_WEFF_PADDED_ONLINE 6
#define STMPC_NOISY_WEFF_PADDED_TARGET 7
#define STMPC_NOISY_WEFF_PADDED_ACT 8
typedef struct stmpc_noisy_cfg {
    double sigma0;                   /* sigma starts at sigma0 / sqrt(h1) (0.5: Fortunato et al. 2018, section 3.2) */
} stmpc_noisy_cfg;
int  stmpc_noisy_c51_enable(stmpc_c51 *learner, const stmpc_noisy_cfg *cfg);
int  stmpc_noisy_c51_set_params(stmpc_c51 *learner, int slot, const float *values, int64_t count);
int  stmpc_noisy_c51_get_params(stmpc_c51 *learner, int slot, float *values, int64_t count);
int  stmpc_noisy_c51_act_device(stmpc_c51 *learner, int N, const float *d_obs, int obs_stride, double eps, int32_t *d_action, float *d_debug_q, void *stream);
int  stmpc_noisy_c51_debug_read(stmpc_c51 *learner, int what, float *out, int64_t count);

/*
 * A population of C51 learners: the population axis of stmpc_ddpg_pop_* / stmpc_pop_td3_* / stmpc_pop_dqn_* for the categorical learner above.  P
 * independent C51 learners -- each its own ring, logits network, target, Adam state, counters, seed and constants, the support [v_min, v_max],
 * double_dqn, target_period, replay_start and n_step included -- share one discrete-action vector environment and advance with ONE launch per
 * kernel: three launches per update whatever P is and whatever the members' counters say, five when at least one member is prioritised; acting,
 * pushing and the statistics are one launch each.  Member m owns rows [m * n_per_member, (m + 1) * n_per_member) of the step tensors and is
 * bit-identical to a lone stmpc_c51 with its cfg given its slice.  What a user compares between runs of the categorical agent (rainbow.py: the
 * `all` library's rainbow preset) -- which support fits the env's returns, double against plain action selection, target_period, gamma, n_step,
 * seeds, prioritised against uniform replay, traffic types, reward settings -- is then one run.  (Additive: new entries only, no signature or struct
 * of ABI 8 changes, so STMPC_ABI_VERSION stays 8; no entry above changes what it computes.)  The entries read stmpc_pop_c51_*: the prefixes
 * stmpc_c51_, stmpc_pop_dqn_, stmpc_pop_per_ and stmpc_pop_nstep_ are closed sets, which is why prioritised replay and n_step are enabled here.
 *   pop_create      (rainbow.py) P = 1 ... STMPC_C51_POP_MAX configs that share n_obs, h1, n_actions, n_atoms, batch and capacity (one network
 *                   shape, one LDS size, one grid); everything else may differ per member -- v_min, v_max and dz travel in the member's own device
 *                   struct.  Each member is made by the lone create, whose refusals apply per member
 *   pop_destroy, pop_size   (rainbow.py) the population with its members; the member count (0 for NULL)
 *   pop_member      (rainbow.py) the m-th member as a BORROWED stmpc_c51, valid until pop_destroy (never destroy it): every lone entry works on it
 *                   as on a lone learner -- set / get_params, set / get_state, grads, targets, dist, project, gather, stats, per_tree_read,
 *                   per_last_device, padded_read, dzout_read, stmpc_c51actor_view, and the lone act, push and update -- but the lone per_enable and
 *                   multi_step_enable, which refuse: both are the population's to set
 *   pop_act_device  (rainbow.py) the lone act_device per member: d_action int32 [P * n_per_member]; eps HOST fp64 [n_eps], n_eps = P, one value per
 *                   member (it travels as a kernel argument).  Member m's exploration hash is keyed by its own seed, its own count of exploring
 *                   calls and the row local to its slice.  A member whose eps is 0 draws nothing and its call counter stays, as a lone learner's
 *                   does under eps = 0.  d_debug_q (may be NULL) float32 [P * n_per_member][n_actions]: the expected values
 *   pop_push_device (rainbow.py) the lone push_device per member, each slice into its member's ring (and tree, where the member has one)
 *   pop_update_device   (rainbow.py) n_updates updates of every member; lr HOST fp64 [n_lr], n_lr = P.  A member whose replay_start gate is shut
 *                   skips its update while the others proceed, and the hard copy of the target follows the member's own update count and
 *                   target_period; both are decided on the device
 *   pop_stats_device    (rainbow.py) d_out DEVICE fp64 [P][4]: the lone stats_device's four numbers per member
 *   pop_per_enable  (rainbow.py) stmpc_pop_dqn_per_enable for this population: cfgs HOST [P], enabled HOST uint8 [P]; one call, on empty rings;
 *                   afterwards a prioritised member is bit-identical to a lone learner with the lone per_enable, a uniform one to the member of a
 *                   population without the call
 *   pop_multi_step_enable   (rainbow.py) stmpc_pop_nstep_enable_dqn for this population: cfgs HOST [P], member m gets cfgs[m]; rows_per_push is the
 *                   population's n_per_member.  Every member passes the lone entry's checks before any changes; then the device tables are
 *                   written anew
 *   pop_replay_read (rainbow.py) debug, HOST: `count` rows of STMPC_DDPG_ROW float32 from row `first` of a learner's ring -- a borrowed member's,
 *                   or a lone stmpc_c51's, so that the two can be compared; synchronises
 *   pop_multi_step_window   (rainbow.py) debug, HOST: stmpc_nstep_window_dqn for a stmpc_c51, borrowed or lone (the stmpc_nstep_ and stmpc_c51_
 *                   prefixes are closed sets, and no other exported name holds "nstep"): out [n_idx][4] fp64 = R, disc, the ring row of the window's last transition, m for the n_idx ring rows idx (each
 *                   a filled row, else STMPC_EINVAL), by the device function the update's gather calls; synchronises
 * Refused with STMPC_EINVAL before any launch: P outside 1 ... 64, members that differ in a shared field (the message names the member and lists
 * the shared fields), n_lr or n_eps other than P, an eps outside 0 ... 1, a negative learning rate or n_updates, n_per_member outside
 * 1 ... capacity, NULL pointers.
 */
#define STMPC_C51_POP_MAX 64            /* == STMPC_DDPG_POP_MAX */
typedef struct stmpc_c51_pop stmpc_c51_pop;
int  stmpc_pop_c51_create(stmpc_ctx *ctx, const stmpc_c51_cfg *cfgs, int P, stmpc_c51_pop **out);
void stmpc_pop_c51_destroy(stmpc_c51_pop *pop);
int  stmpc_pop_c51_size(const stmpc_c51_pop *pop);
stmpc_c51 *stmpc_pop_c51_member(stmpc_c51_pop *pop, int m);
int  stmpc_pop_c51_act_device(stmpc_c51_pop *pop, int n_per_member, const float *d_obs, int obs_stride, const double *eps, int n_eps,
                              int32_t *d_action, float *d_debug_q, void *stream);
int  stmpc_pop_c51_push_device(stmpc_c51_pop *pop, int n_per_member, const float *d_obs, const float *d_next_obs, const float *d_final_obs,
                               int obs_stride, const int32_t *d_action, const double *d_reward, const uint8_t *d_terminated,
                               const uint8_t *d_truncated, void *stream);
int  stmpc_pop_c51_update_device(stmpc_c51_pop *pop, int n_updates, const double *lr, int n_lr, void *stream);
int  stmpc_pop_c51_stats_device(stmpc_c51_pop *pop, double *d_out, void *stream);
int  stmpc_pop_c51_per_enable(stmpc_c51_pop *pop, const stmpc_per_cfg *cfgs, const uint8_t *enabled, int P);
int  stmpc_pop_c51_multi_step_enable(stmpc_c51_pop *pop, const stmpc_nstep_cfg *cfgs, int P);
int  stmpc_pop_c51_replay_read(stmpc_c51 *learner, int64_t first, int64_t count, float *rows);
int  stmpc_pop_c51_multi_step_window(stmpc_c51 *learner, const int64_t *idx, int n_idx, double *out);

/*
 * The noisy output layer for a population of C51 learners (rainbow.py: the noisy layers of the `all` library's rainbow preset, one run per member).
 * (Additive: two new entries under a prefix of their own -- stmpc_pop_c51_ is a closed set --, STMPC_ABI_VERSION stays 8.)  The members share on /
 * off; sigma0 is a member's own.  Member m stays bit-identical to a lone noisy stmpc_c51 with its cfg, seed and sigma0 driven on its slice: the draws
 * are keyed by the member's seed and its own counters, and nothing crosses members.  stmpc_pop_c51_update_device then runs the noisy sequence, four
 * launches per update whatever P is (six with prioritised members); stmpc_pop_c51_act_device stays the mean networks'.  The lone set / get_params,
 * debug_read, act_device and stmpc_c51_set / get_state work on a borrowed member.
 *   pop_enable      (rainbow.py) cfgs HOST [P], member m gets cfgs[m]; one call, on fresh members (before per_enable or multi_step_enable, or after:
 *                   both orders work).  STMPC_EINVAL for P other than the member count, a second call, a sigma0 that is negative or not finite, and
 *                   members that have pushed or updated.  Synchronises
 *   pop_act_device  (rainbow.py) stmpc_noisy_c51_act_device per member with stmpc_pop_c51_act_device's arguments: every member takes an acting draw
 *                   of its own (its counters[5] advances); eps HOST fp64 [n_eps], n_eps = P, honoured per member
 */
int  stmpc_pop_noisy_c51_enable(stmpc_c51_pop *pop, const stmpc_noisy_cfg *cfgs, int P);
int  stmpc_pop_noisy_c51_act_device(stmpc_c51_pop *pop, int n_per_member, const float *d_obs, int obs_stride, const double *eps, int n_eps,
                                    int32_t *d_action, float *d_debug_q, void *stream);

/*
 * A Q-network as the policy of the combined controller and of the first-step shield: DQNAgent.get_control (dqn.py:375-380) -- state vector -> Q ->
 * argmax -> JERK_VALUES_DQN[a] -- for N states in ONE launch, behind which RLAgent.do_combined_control runs as it does behind the DDPG actor.
 * (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8; no entry above changes what it computes.)  The
 * forward pass and the first-maximum argmax are stmpc_dqn_act_device's own code on the same packed operands: Q, the index and the jerk are the bits
 * that entry gives (eps = 0) on the input vectors stmpc_policy_features_device writes with time_feature = 0.
 *   stmpc_qactor_create   (dqn.py:375-380 with DQNAgent.load's network) from HOST row-major tensors as torch stores them: w0 [h1][n_in], b0 [h1],
 *                   w1 [n_actions][h1], b1 [n_actions], and the action table action_values [n_actions] (index -> what the env executes).  The
 *                   tensors go through the learner's own network builder and re-packing kernel: bit-identical to a stmpc_dqn loaded with them.
 *                   STMPC_EINVAL for a NULL argument, n_in outside 1 ... 31, h1 outside 1 ... 1024, n_actions outside 1 ... STMPC_ENV_MAX_ACTIONS,
 *                   a mode that is neither STMPC_QACTOR_JERK nor STMPC_QACTOR_ACCELERATION, a table entry that is not finite.  Synchronises
 *   stmpc_qactor_view_dqn (dqn.py:375-380 on the agent being trained) a BORROWED policy whose network ALIASES the learner's online (target = 0) or
 *                   target (target = 1) Q-network: the learner keeps both packed after every update, so no copy is made, and an evaluation ordered
 *                   after an update ON THE SAME STREAM sees the update.  It owns its action table alone; stmpc_qactor_destroy frees nothing of the
 *                   learner's; destroy it before the learner.  Evaluating reads the network only: no counter, ticket or workspace of the learner is
 *                   touched.  STMPC_EINVAL for a NULL argument, target not 0 or 1, n_actions different from the learner's, a bad mode or table
 *   stmpc_qactor_set_limits   (merge_gym.py:196-204) acceleration mode's constants: Settings.TICK_LENGTH, MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK
 *                   (tick_length > 0, minimum <= maximum, all finite, else STMPC_EINVAL).  Not read in jerk mode
 *   stmpc_qactor_eval_device  (dqn.py:375-380) d_jerk fp64 [N], required; optional (NULL: not written) d_action int32 [N], d_q float32 [N][n_actions],
 *                   d_feat float32 [N][feat_stride].  STMPC_QACTOR_JERK: jerk = action_values[a].  STMPC_QACTOR_ACCELERATION: jerk =
 *                   clip((action_values[a] - the state's ego acceleration) / tick_length, minimum_negative_jerk, maximum_positive_jerk) in fp64 --
 *                   AccelerationEnv._do_action's projected jerk before its speed clamp, with the state's own acceleration for the env's previous
 *                   one; the reference has no evaluator for that env, the rule is this library's.  The state arguments, `step` and the rows of
 *                   finished rollouts are stmpc_actor_eval_device's (step > 1 needs a rollout of N states in the context; without a time feature
 *                   every row is evaluated alike).  STMPC_EINVAL, before anything is launched, for a NULL ctx / qactor / cfg / required pointer,
 *                   N < 1, cfg->time_feature set, stmpc_policy_features_len(cfg) != n_in, feat_stride < n_in with d_feat given, a context on another
 *                   device than the policy's, acceleration mode without stmpc_qactor_set_limits.  Asynchronous
 */
#define STMPC_QACTOR_JERK 0
#define STMPC_QACTOR_ACCELERATION 1
typedef struct stmpc_qactor stmpc_qactor;
int  stmpc_qactor_create(stmpc_ctx *ctx, int n_in, int h1, int n_actions, const float *w0, const float *b0, const float *w1, const float *b1,
                         const double *action_values, int mode, stmpc_qactor **out);
int  stmpc_qactor_view_dqn(stmpc_dqn *learner, int target, const double *action_values, int n_actions, int mode, stmpc_qactor **out);
void stmpc_qactor_destroy(stmpc_qactor *qactor);
int  stmpc_qactor_set_limits(stmpc_qactor *qactor, double tick_length, double minimum_negative_jerk, double maximum_positive_jerk);
int  stmpc_qactor_eval_device(stmpc_ctx *ctx, const stmpc_qactor *qactor, const stmpc_policy_features_cfg *cfg, int N, int Kmax, int step,
                              const double *d_cur_ego4, const int32_t *d_k_count, const double *d_cur_other_x, const double *d_cur_other_v,
                              const double *d_cur_other_a, float *d_feat, int feat_stride, int32_t *d_action, float *d_q, double *d_jerk, void *stream);

/*
 * A categorical (C51) network as such a policy: DQNAgent.get_control's job (dqn.py:375-380) for the distributional head of the reference's third
 * agent (rainbow.py: RainbowAgent) -- state vector -> logits -> E[Z(s, a)] of every action -> first maximum -> the action table -- for N states in
 * ONE launch.  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8; no entry above changes what it
 * computes.)  A C51 policy IS a stmpc_qactor, with a categorical head: stmpc_qactor_eval_device, stmpc_qactor_set_limits, stmpc_qactor_destroy and
 * the lone policy of stmpc_qshield_env_reset_device / _step_device take it as they take a Q-network's, and d_q is then the expected values,
 * float32 [N][n_actions].  The forward pass and the argmax are stmpc_c51_act_device's own code on the same packed operands: the expected values,
 * the index and the jerk are the bits that entry gives (eps = 0, d_debug_q) on the input vectors stmpc_policy_features_device writes with
 * time_feature = 0.  (The two entries are not named stmpc_qactor_...: that prefix and stmpc_c51_... are closed sets.)
 *   stmpc_c51actor_create   (dqn.py:375-380 with RainbowAgent.load's network, rainbow.py) from HOST row-major tensors as C51Learner.export_q writes
 *                   them: w0 [h1][n_in], b0 [h1], w1 [n_actions * n_atoms][h1], b1 [n_actions * n_atoms] (action a's logits are rows a * n_atoms
 *                   ...), the support's n_atoms, v_min, v_max, and the action table.  The tensors go through the C51 learner's own network
 *                   builder, slot layout and re-packing kernel: bit-identical to a stmpc_c51 loaded with them; dz = (v_max - v_min) / (n_atoms - 1)
 *                   in fp64 as that learner forms it.  STMPC_EINVAL for everything stmpc_qactor_create refuses, n_atoms < 2, n_actions * n_atoms >
 *                   STMPC_C51_MAX_LOGITS, a support that is not finite or v_max <= v_min, a network too wide for one workgroup's LDS.  Synchronises
 *   stmpc_c51actor_view     (dqn.py:375-380 on the agent being trained, rainbow.py) a BORROWED policy whose network ALIASES the C51 learner's online
 *                   (target = 0) or target (target = 1) logits network, with stmpc_qactor_view_dqn's rules: no copy, an evaluation ordered after
 *                   an update on the same stream sees the update, it owns its action table alone, destroy it before the learner.  Evaluating reads
 *                   the network, the shape and the support only: no counter, ticket or workspace of the learner is touched.  STMPC_EINVAL for a
 *                   NULL argument, target not 0 or 1, n_actions different from the learner's, a bad mode or table
 * stmpc_pop_qactor_create refuses a categorical member (STMPC_EINVAL): a population of C51 policies does not exist, one launch needs one head.
 */
int  stmpc_c51actor_create(stmpc_ctx *ctx, int n_in, int h1, int n_actions, int n_atoms, double v_min, double v_max, const float *w0, const float *b0,
                           const float *w1, const float *b1, const double *action_values, int mode, stmpc_qactor **out);
int  stmpc_c51actor_view(stmpc_c51 *learner, int target, const double *action_values, int n_actions, int mode, stmpc_qactor **out);

/*
 * A categorical policy with a DUELING head from plain tensors: stmpc_c51actor_create with its arguments, for a network as a dueling C51Learner's
 * export_q writes it -- w1 [(n_actions + 1) * n_atoms][h1], b1 [(n_actions + 1) * n_atoms], the n_actions advantage blocks first and the value block
 * last (the layout of stmpc_c51_cfg.dueling above).  The result is a stmpc_qactor like that entry's, bit-identical to stmpc_c51actor_view of a dueling
 * stmpc_c51 loaded with the same tensors.  STMPC_EINVAL for what stmpc_c51actor_create refuses, with (n_actions + 1) * n_atoms >
 * STMPC_C51_MAX_LOGITS in the width's place.  (Additive: a new entry, STMPC_ABI_VERSION stays 8.  It is not named stmpc_c51actor_...: that prefix is
 * a closed set of two entries.)  Synchronises
 */
int  stmpc_dueling_c51actor_create(stmpc_ctx *ctx, int n_in, int h1, int n_actions, int n_atoms, double v_min, double v_max, const float *w0,
                                   const float *b0, const float *w1, const float *b1, const double *action_values, int mode, stmpc_qactor **out);

/*
 * A population of Q-networks as policies, evaluated in one launch: what stmpc_actor_pop_* is for DDPG actors, for the Q-actors above.  The reference
 * compares its DQN agents run by run (double against plain targets, clipped against unclipped, the freeze period, prioritised against uniform replay,
 * seeds, traffic types), one DQNAgent.get_control (dqn.py:375-380) evaluation process per model.  (Additive: new entries only, no signature or struct
 * of ABI 8 changes, so STMPC_ABI_VERSION stays 8; stmpc_qactor_* above is unchanged.)
 *   stmpc_pop_qactor_create   (dqn.py:375-380 for P models) P = 1 ... STMPC_DDPG_POP_MAX Q-actors -- created ones or stmpc_qactor_view_dqn views, of the
 *                   online or the target network, of a lone learner or of a handle lent by stmpc_pop_dqn_member -- on the context's device, which
 *                   share n_in, the padded hidden width, the padded action width and n_actions itself (one launch shape, one LDS size, one d_q
 *                   layout), else STMPC_EINVAL; also for P out of range, a NULL member, and an acceleration-mode member without
 *                   stmpc_qactor_set_limits.  Mode, action table, limits and online / target may differ per member.  The population holds a DEVICE
 *                   TABLE of the members' descriptions, written once here: a member's table pointer, mode and limits as they are now (a later
 *                   stmpc_qactor_set_limits on a member does not reach the population), and the network's pointers.  A learner's network buffers
 *                   and shape are fixed from stmpc_dqn_create to stmpc_dqn_destroy -- stmpc_dqn_per_enable and stmpc_pop_dqn_per_enable re-wire the
 *                   replay store's part of the learner alone -- so a view's entry stays valid and LIVE: an evaluation ordered after an update on the
 *                   same stream sees the update, as the lone view does.  The members stay the caller's and must outlive the population.  Synchronises
 *   stmpc_pop_qactor_destroy  (dqn.py:375-380) frees the table alone; nothing of a member's
 *   stmpc_pop_qactor_size     (dqn.py:375-380) P; 0 for NULL
 *   stmpc_pop_qactor_eval_device  (dqn.py:375-380) stmpc_qactor_eval_device on arrays of P * n_per_member rows: member m evaluates rows [m *
 *                   n_per_member, (m + 1) * n_per_member), bit-identical to stmpc_qactor_eval_device with that member on that slice; d_q is
 *                   [P * n_per_member][n_actions].  Same argument checks (step > 1 needs a rollout of P * n_per_member states in the context).
 *                   STMPC_EINVAL, before anything is launched, for a NULL ctx / pop / cfg / required pointer, n_per_member < 0 or P * n_per_member
 *                   beyond int32, cfg->time_feature set, stmpc_policy_features_len(cfg) != n_in, feat_stride < n_in with d_feat given, a context on
 *                   another device than the population's.  n_per_member = 0 returns STMPC_OK and launches nothing.  Asynchronous
 */
typedef struct stmpc_qactor_pop stmpc_qactor_pop;
int  stmpc_pop_qactor_create(stmpc_ctx *ctx, const stmpc_qactor *const *qactors, int P, stmpc_qactor_pop **out);
void stmpc_pop_qactor_destroy(stmpc_qactor_pop *pop);
int  stmpc_pop_qactor_size(const stmpc_qactor_pop *pop);
int  stmpc_pop_qactor_eval_device(stmpc_ctx *ctx, const stmpc_qactor_pop *pop, const stmpc_policy_features_cfg *cfg, int n_per_member, int Kmax, int step,
                                  const double *d_cur_ego4, const int32_t *d_k_count, const double *d_cur_other_x, const double *d_cur_other_v,
                                  const double *d_cur_other_a, float *d_feat, int feat_stride, int32_t *d_action, float *d_q, double *d_jerk, void *stream);

/*
 * A population of categorical (C51) policies, evaluated in one launch: the population above for the distributional head of the reference's third
 * agent (rainbow.py: RainbowAgent) doing DQNAgent.get_control's job (dqn.py:375-380).  What a C51 population's sweeps train -- support, double,
 * target period, gamma, multi-step, seed, prioritised replay, sigma0 -- is evaluated side by side, and trained behind the combined controller's
 * shield, instead of one member at a time.  (Additive: one new entry, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8;
 * stmpc_pop_qactor_create keeps refusing a categorical member.  The entry is not named stmpc_pop_qactor_..., stmpc_c51actor_..., stmpc_pop_c51_... or
 * stmpc_c51_...: those prefixes are closed sets.)
 *   stmpc_pop_c51actor_create (dqn.py:375-380 for P models, rainbow.py) P = 1 ... STMPC_DDPG_POP_MAX categorical Q-actors -- stmpc_c51actor_create or
 *                   stmpc_dueling_c51actor_create actors, or stmpc_c51actor_view views, of the online or the target network, of a lone learner or
 *                   of a handle lent by stmpc_pop_c51_member -- on the context's device, which share n_in, the padded hidden width, n_actions,
 *                   n_atoms and the head (dueling or not: one launch shape, one LDS size, one d_q layout).  The support (v_min, v_max), the action
 *                   table, mode, limits and online / target may differ per member.  STMPC_EINVAL, naming the member, with *out NULL and nothing
 *                   launched, for P out of range, a NULL member, a member on another device, a member that is no categorical policy (a Q-network
 *                   goes to stmpc_pop_qactor_create), a shape that differs from member 0's, an acceleration-mode member without
 *                   stmpc_qactor_set_limits.  The result is a stmpc_qactor_pop: stmpc_pop_qactor_destroy, stmpc_pop_qactor_size,
 *                   stmpc_pop_qactor_eval_device and the population of stmpc_qshield_env_reset_device / _step_device take it as they take a
 *                   population of Q-networks, and d_q is then the expected values, float32 [P * n_per_member][n_actions]; member m's rows are
 *                   bit-identical to stmpc_qactor_eval_device with that member on that slice.  The population holds a DEVICE TABLE of the members'
 *                   descriptions, written once here: table pointer, mode and limits as they are now, the network's pointers, the shape and the
 *                   support (dz in fp64 as the owner formed it).  A C51 learner's network buffers, shape and support are fixed from stmpc_c51_create
 *                   to stmpc_c51_destroy -- stmpc_c51_per_enable, stmpc_pop_c51_per_enable, stmpc_c51_multi_step_enable and
 *                   stmpc_pop_c51_multi_step_enable re-wire the replay store's part of the learner alone; a population of learners re-uploads its
 *                   members' structs as they are; stmpc_noisy_c51_enable and stmpc_pop_noisy_c51_enable work on copies of the struct and leave the
 *                   learner's own on the mean weights mu -- so a view's entry stays valid and LIVE: an evaluation ordered after an update on the same
 *                   stream sees the update, as the lone view does.  A view of a noisy learner evaluates mu, as the lone view does.  The members stay
 *                   the caller's and must outlive the population.  Synchronises
 */
int  stmpc_pop_c51actor_create(stmpc_ctx *ctx, const stmpc_qactor *const *members, int P, stmpc_qactor_pop **out);

/*
 * Actors straight from learners, and a population of actors evaluated in one launch.  The reference's workflow ends a training with an evaluation
 * of the model it trained (ddpg.train_ddpg_all_with_lr_drop's closing `evaluate`, ddpg.py:96-117) and publishes a matrix of EVALUATE_COMBINED_DDPG runs, one per
 * MODEL_NAME (DDPGAgent.load + get_control, ddpg.py:38-44, 83-87; configs/combined_<traffic>_{1,2,3}.json, experiment_data/saved_data.csv).  (Additive: new
 * entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 *   stmpc_actor_view_ddpg   a BORROWED actor whose tensors ALIAS the learner's online (target = 0) or target (target = 1) actor: the learner keeps both
 *                   packed for the kernel after every update, so no copy is made, and the output bias is read through a pointer at every evaluation.
 *                   An evaluation ordered after an update ON THE SAME STREAM sees the updated weights; across streams the order is the caller's to
 *                   establish.  The arithmetic is stmpc_actor_eval_device's float32 chain and tanhf, as for the learner's exported file -- not
 *                   stmpc_ddpg_act_device's fp64 output dot.  Valid until the learner is destroyed: destroy the view first, with stmpc_actor_destroy,
 *                   which frees nothing the learner owns.  Works on handles lent by stmpc_ddpg_pop_member; stmpc_actor_eval_device takes a view like
 *                   any actor, from any context on the learner's device.
 *   stmpc_actor_pop_create  P = 1 ... STMPC_DDPG_POP_MAX actors (created or views) that share n_in, the padded hidden widths and the context's device
 *                   (one launch shape, one LDS size), else STMPC_EINVAL; the squash may differ per member.  The members stay the caller's and must
 *                   outlive the population, which holds a device table of their descriptions.
 *   stmpc_actor_pop_eval_device   stmpc_actor_eval_device on arrays of P * n_per_member rows: member m evaluates rows [m * n_per_member, (m + 1) *
 *                   n_per_member), bit-identical to stmpc_actor_eval_device with that member on that slice; same argument checks (step > 1 needs a
 *                   rollout of P * n_per_member states in the context).
 */
typedef struct stmpc_actor_pop stmpc_actor_pop;
int  stmpc_actor_view_ddpg(stmpc_ddpg *learner, int target, stmpc_actor **out);
int  stmpc_actor_pop_create(stmpc_ctx *ctx, const stmpc_actor *const *actors, int P, stmpc_actor_pop **out);
void stmpc_actor_pop_destroy(stmpc_actor_pop *pop);
int  stmpc_actor_pop_size(const stmpc_actor_pop *pop);
int  stmpc_actor_pop_eval_device(stmpc_ctx *ctx, const stmpc_actor_pop *pop, const stmpc_policy_features_cfg *cfg, int n_per_member, int Kmax, int step,
                                 const double *d_cur_ego4, const int32_t *d_k_count, const double *d_cur_other_x, const double *d_cur_other_v,
                                 const double *d_cur_other_a, int32_t *d_evals, float *d_feat, int feat_stride, double *d_jerk, void *stream);

/*
 * Traffic groups: the world of a context split into G groups of n_per_group consecutive environments, each with its own stmpc_sim_cfg, stepped, viewed,
 * recorded, used as a vector environment and reset in the launches of an ungrouped world.  The reference's experiment matrix varies along this axis: its
 * configs/{train,combined,cross,ddpg}_*.json differ in BASE_TRAFFIC_INTERVAL and OTHER_CAR_SPEED -- the highway flow control.py:215-226 inserts -- and each
 * is one process with one merge_gym.py environment.  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 * Group g of a grouped world is, bit for bit, the lone world of n_per_group environments made from cfgs[g]: environment `local` of the group draws
 * as environment `local` of that world (its seed, its episode seeds and counter windows) and lives at row g * n_per_group + local of every array.
 *   May differ between groups: other_car_speed, base_traffic_interval, vary_traffic_start_times, speed_dev, seed, start_speed, start_speed_std,
 *                   min_start_speed, max_start_speed, randomize_start_speed, max_ticks.
 *   Must be equal (else STMPC_EINVAL naming the field): tick_length, spawn_x, despawn_x, ego_start_x, ego_start_y, arrive_x, sensor_radius, the veh_*
 *                   vehicle type, disruption_min_s, yield_overlap and the route (the context keeps one device copy, from cfgs[0]; the others point to
 *                   equal points, or are NULL alike).  Two groups with the same seed see common random numbers; nothing else couples groups.
 *   stmpc_sim_init_groups_device   validates every cfg, uploads the table (synchronises on `stream` for it), sets the world's size to G * n_per_group
 *                   and initialises it; G = 1 ... STMPC_SIM_GROUPS_MAX, n_per_group >= 1.  Ends the environment as stmpc_sim_init_device does;
 *                   stmpc_sim_init_device on the context ends the grouping.  A refused call changes nothing.
 *   stmpc_sim_step_groups_device   stmpc_sim_step_device for a grouped world: takes no cfgs (the context's table is read on the device; no copy, no
 *                   synchronisation).  N must be G * n_per_group.  STMPC_EINVAL on a world without groups -- and the plain stmpc_sim_step_device /
 *                   stmpc_env_step_device return STMPC_EINVAL on a grouped world, which they would step with one cfg.  stmpc_sim_view_device (any
 *                   group's cfg: it reads sensor_radius), stmpc_sim_read, stmpc_sim_status_device and the recorder serve a grouped world unchanged.
 *   stmpc_env_reset_groups_device / stmpc_env_step_groups_device   stmpc_env_reset_device / stmpc_env_step_device on a grouped world; an episode log
 *                   row's environment column holds the global row.  The autoreset re-initialises an environment with its own group's cfg.
 *   stmpc_sim_groups   the current split (0, 0: an ungrouped world)
 */
#define STMPC_SIM_GROUPS_MAX 64
int stmpc_sim_init_groups_device(stmpc_ctx *ctx, const stmpc_sim_cfg *cfgs, int G, int n_per_group, void *stream);
int stmpc_sim_step_groups_device(stmpc_ctx *ctx, const stmpc_params *p, int N, const double *d_cmd_speed, void *stream);
int stmpc_sim_groups(stmpc_ctx *ctx, int *G, int *n_per_group);
int stmpc_env_reset_groups_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *cfgs, int G, int n_per_group, const stmpc_env_cfg *env_cfg,
                                  float *d_obs, int obs_stride, void *stream);
int stmpc_env_step_groups_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_env_cfg *env_cfg, int N, const void *d_action, float *d_obs,
                                 int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats,
                                 void *stream);

/*
 * Controller groups: one batch of the combined controller split into C groups of n_per_group consecutive states, each with its own stmpc_combined_cfg,
 * rolled out and decided in the launches of a lone batch.  The reference compares the combined controller's own settings one process per cell:
 * main.do_grid_search_combined (main.py:62-81) sweeps ROLLOUT_LENGTH x ST_TEST_ROLLOUTS x TEST_ROLLOUT_STATE, its combined_*b configs flip
 * CHECK_ROLLOUT_CRASH, LIMIT_DQN_SPEED, TEST_ST_STRICTLY_BETTER and REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED.  (Additive: new entries only, no
 * signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 * Group g of a grouped batch is, bit for bit, the lone batch of n_per_group states under cfgs[g]: decisions, commands, the cur_* arrays, the rollout
 * bookkeeping and -- through the evaluation mask below -- the policy's evaluation counters.
 *   May differ between groups: rollout_length, st_test_rollouts, check_rollout_crash, limit_dqn_speed, test_rollout_state, test_st_strictly_better,
 *                   remember_last_choice.  Must be equal (else STMPC_EINVAL naming the field): tick_length, stop_x, sparse_control.
 *   stmpc_combined_groups_set     validates every cfg (a rollout_length above STMPC_ROLLOUT_LIMIT in any group is refused), uploads the table and the
 *                   static list of the rows whose group has test_rollout_state set (synchronous copies, once); C = 1 ... STMPC_SIM_GROUPS_MAX,
 *                   n_per_group >= 1.  Ends a grouped rollout that is under way.  A refused call changes nothing.
 *   stmpc_combined_groups_clear   ends the grouping (and a grouped rollout that is under way).
 *   stmpc_rollout_step_groups_device   stmpc_rollout_step_device without a cfg: the context's table is read on the device, so a step copies nothing.  N
 *                   must be C * n_per_group.  Call it for step = 1 .. Rmax, the largest group's max(rollout_length, 1): a step past a group's own
 *                   length leaves that group's rows untouched.  rollout_s has row stride Rmax + 1 for every group (stmpc_combined_read_state:
 *                   [N][Rmax + 1]; a group's history ends at its own length + 1).  While the context's rollout is a grouped one, the policy entries
 *                   (stmpc_policy_features_device, stmpc_actor_eval_device, stmpc_actor_pop_eval_device) count an evaluation at step > 1 only for
 *                   the rows that are live AND whose group has that step -- a lone batch of R steps asks its policy at steps 1 .. R only; `live`
 *                   itself (stmpc_combined_read_state) keeps its meaning.
 *   stmpc_combined_decide_groups_device   stmpc_combined_decide_device for a grouped rollout.  The feasibility probe solves only the rows of the groups
 *                   that test (gathered through the static list: no round trip; a group that does not test can never latch a solver error for its rows).
 *                   With sparse_control the controller is solved for the rows whose own group's branches hand control over (one round trip, as the
 *                   plain entry) -- unless ANY group sets test_st_strictly_better: one such group makes the whole run dense (every row is solved;
 *                   same decisions and commands either way, as stmpc_combined_cfg states).
 *   The plain stmpc_rollout_step_device / stmpc_combined_decide_device ignore the table and behave as without one.  STMPC_EINVAL before any launch,
 *   changing nothing: a grouped step or decide with no table set; N != C * n_per_group; a grouped decide after a plain rollout or a plain decide after a
 *   grouped rollout; step > 1 that does not continue a grouped rollout of this shape.
 */
int stmpc_combined_groups_set(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_combined_cfg *cfgs, int C, int n_per_group);
int stmpc_combined_groups_clear(stmpc_ctx *ctx);
int stmpc_rollout_step_groups_device(stmpc_ctx *ctx, const stmpc_params *p, int N, int Kmax, int step, const double *d_ego5_start, double *d_cur_ego4,
                                     const int32_t *d_k_count, double *d_cur_other_x, double *d_cur_other_v, double *d_cur_other_a,
                                     const double *d_action, void *stream);
int stmpc_combined_decide_groups_device(stmpc_ctx *ctx, const stmpc_params *p, int N, int Kmax, const double *d_ego5_start, const int32_t *d_k_count,
                                        const double *d_other_x_start, const double *d_other_v_start, const double *d_cur_ego4,
                                        const double *d_cur_other_x, const double *d_cur_other_v, const double *d_first_action,
                                        const int32_t *d_last_choice_rl, int32_t *d_takeover, int32_t *d_reason, double *d_speed, void *stream);

/*
 * Solver groups: one batch of the ST solver split into G groups of n_per_group consecutive states, each solved under its own stmpc_params, in the
 * launches of one batch (state i belongs to group i / n_per_group).  The reference tunes the solver along exactly this axis, one process per cell:
 * main.do_grid_search_st (main.py:43-59) runs TASK "ST" over the product of V_WEIGHT, A_WEIGHT, J_WEIGHT, D_WEIGHT, MIN_ALLOWED_DISTANCE and
 * CRASH_MIN_S (288 cells).  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 * Every output row of group g is, bit for bit, the row of a lone call with n_per_group states under groups[g]: path_idx, best_t, cost, path_dist, crash,
 * action_cost, and for the control entry speed, fine and fine_len.  The scheduling statistics of stmpc_stats describe the grouped batch as a whole.
 *   May differ between groups: d_w, v_w, a_w, j_w, min_allowed, crash_min_s.  Every other field must be equal (else STMPC_EINVAL naming the field,
 *                   before any launch): the lattice, the limits, the uncertainty settings, the predictor constants, comb_min_dist.
 *   G = 1 ... STMPC_SOLVER_GROUPS_MAX, n_per_group >= 1, N == G * n_per_group (else STMPC_EINVAL).  G = 1 gives the results of the ungrouped entry.
 *   stmpc_solve_batch_groups_device   stmpc_solve_batch_device_ac (main.py:43-59 over it) with a table of G parameter sets (HOST pointer; its device copy
 *                   is kept while the next call brings an equal table, and replacing it synchronises with the device once).
 *   stmpc_solve_batch_groups          its host-pointer form, as stmpc_solve_batch (action_cost [N][2] may be NULL).
 *   stmpc_st_control_groups_device    stmpc_st_control_batch_device (st.do_st_control, main.py:43-59 over it): the grouped solve, then the re-sampling,
 *                   which reads none of the six fields.
 *   stmpc_solver_groups_sim_step_device   stmpc_sim_step_groups_device (main.py:43-59 over the world step) with the closest-distance statistics of traffic
 *                   group g gated by groups[g].crash_min_s, so that a cell's statistics are those of a lone world under its own CRASH_MIN_S.  The world
 *                   must have traffic groups and the solver groups must coincide with them (same G and n_per_group: cell c pairs traffic c with
 *                   solver c).
 *   stmpc_solver_groups_sim_init_device   stmpc_sim_init_groups_device (main.py:43-59: the world of the whole grid) for G = 1 ... STMPC_SOLVER_GROUPS_MAX
 *                   cells, one traffic group per cell (cfgs[c]: the cell's traffic and seed; the same seed everywhere gives every cell the same
 *                   draws), so that the whole grid is one world.  Everything that serves a world of traffic groups serves it.
 * A grouped call with a table the context has not seen synchronises with the device to replace its copy: such a call cannot be captured in a graph
 * (a repeat with an equal table copies nothing and can).
 * The grouped solve runs one fixed schedule: no staged vehicle table, no checkpoint / resume between the windows.  It honours STMPC_TIERS, STMPC_NW,
 * STMPC_PEN_CELLS, STMPC_PRUNE, STMPC_FASTDIV, STMPC_OVERLAP, STMPC_SIDE_GRID, STMPC_SPLIT, STMPC_TWO_PHASE, STMPC_HEAVY_FIRST, STMPC_BAND, STMPC_BAND_CAP,
 * STMPC_BAND2_MULT, STMPC_BAND_DENSE, STMPC_TUBE, STMPC_TUBE_DENSE, STMPC_BOUND_INFL, STMPC_LAST_INFL, STMPC_RETRY, STMPC_GSH, STMPC_BP16 and
 * STMPC_FORCE_GENERAL, STMPC_WAVES_PER_CU, STMPC_LDS_HEADROOM, STMPC_CU_RESERVE, STMPC_RETIRE_CUS and STMPC_RETIRE_AT.  Without effect on it:
 * STMPC_STAGE_TAB, STMPC_RESUME, STMPC_POOL, STMPC_RETRY_MOVE, STMPC_PRIO and STMPC_PRIO_MODE (all read only by the checkpointing kernels, which the
 * grouped path does not launch).
 */
#define STMPC_SOLVER_GROUPS_MAX 512
int stmpc_solve_batch_groups_device(stmpc_ctx *ctx, const stmpc_params *groups, int G, int n_per_group, int N, int Kmax, const double *d_ego,
                                    const int32_t *d_k_count, const double *d_other_x, const double *d_other_v, int32_t *d_path_idx, int32_t *d_best_t,
                                    double *d_cost, double *d_path_dist, int32_t *d_crash, double *d_action_cost, void *stream);
int stmpc_solve_batch_groups(stmpc_ctx *ctx, const stmpc_params *groups, int G, int n_per_group, int N, int Kmax, const double *ego, const int32_t *k_count,
                             const double *other_x, const double *other_v, int32_t *path_idx, int32_t *best_t, double *cost, double *path_dist,
                             int32_t *crash, double *action_cost);
int stmpc_st_control_groups_device(stmpc_ctx *ctx, const stmpc_params *groups, int G, int n_per_group, double tick_length, int N, int Kmax,
                                   const double *d_ego, const int32_t *d_k_count, const double *d_other_x, const double *d_other_v, int32_t *d_path_idx,
                                   int32_t *d_best_t, double *d_cost, double *d_speed, double *d_fine, int32_t *d_fine_len, void *stream);
int stmpc_solver_groups_sim_step_device(stmpc_ctx *ctx, const stmpc_params *groups, int G, int n_per_group, int N, const double *d_cmd_speed, void *stream);
int stmpc_solver_groups_sim_init_device(stmpc_ctx *ctx, const stmpc_sim_cfg *cfgs, int G, int n_per_group, void *stream);

/*
 * Episode flight recorder on the device, next to the world (stmpc_sim_*): the per-tick histories the reference's evaluation keeps and what it
 * bins over the ego's position, for N environments in lock-step, with nothing crossing to the host until it is read.  (Additive: new entries
 * only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 *   stmpc_rec_create / destroy / reset   <- the history lists of control.run_episode (control.py:247-254) and StatsAggregator.__init__'s
 *                           bins / counts / jerks / speeds (stats.py:33-41).  N environments, Kmax view slots, a ring of `depth` (1 ...
 *                           STMPC_REC_MAX_DEPTH) records per environment, n_edges (2 ... STMPC_REC_MAX_EDGES) finite, strictly increasing bin edges
 *                           (HOST pointer, copied; the reference's are np.arange(-220, 61, 20)), tick_length = Settings.TICK_LENGTH.  The recorder follows
 *                           ONE episode per environment of the context's world as it is at create / reset: after another stmpc_sim_init_device on the
 *                           context every entry returns STMPC_EINVAL until stmpc_rec_reset (which needs the world's N to be the recorder's and zeroes
 *                           everything; asynchronous on `stream`).  The per-environment resets of the vector environment (stmpc_env_step_device with
 *                           autoreset) are not followed.  Destroy the recorder before its context.
 *   stmpc_rec_tick_device <- state_history.append / position_history / speed_history / acceleration_history / jerk_history of control.py:280-289 and
 *                           takeover_history of dqn.py:144-200, plus add_episode_stats' binning (stats.py:44-52) and combined_stats_callback /
 *                           plot_st_proportion (dqn.py:101-115, 215-226).  Call it once per world tick, between the controller and
 *                           stmpc_sim_step_device, with the view arrays the controller consumed (the state BEFORE control, as the reference appends
 *                           it) and the commanded speeds; d_oa and d_takeover (int32 [N]) may be NULL (recorded as 0).  For every environment whose
 *                           status is 0: one record into ring slot (world tick mod depth) and the tick added to the environment's accumulators; an
 *                           environment that has finished is not touched again, so its last min(ticks, depth) records are the run-up to its end.
 *                           Record = [STMPC_REC_HDR + 3 Kmax] fp64: world tick, ego x, y, v, a, s, k, commanded speed, takeover, jerk, then other_x
 *                           [Kmax], other_v [Kmax], other_a [Kmax].  jerk is jerk_history's entry: 0 for an environment's first record, else
 *                           (a - a of the previous record) / tick_length.  Accumulators per environment and bin, STMPC_REC_NQ quantities:
 *                             0 count, 1 takeover count   np.histogram's rule: edge[b] <= x < edge[b+1], last bin closed on the right, outside dropped
 *                             2 sum |jerk|, 3 sum |v|     the loop of stats.py:48-52: the first b with x <= edge[b+1]; x below the first edge -> bin 0
 *                                                         (beyond the last edge the reference's loop fails with an IndexError; dropped here)
 *                           then two totals: ticks with takeover != 0, recorded ticks (percent st solver = their quotient, dqn.py:113).
 *                           Asynchronous, no atomics; within an environment sums are formed in tick order.
 *   stmpc_rec_reduce_device the accumulators summed over the environments into the recorder (and d_out, DEVICE fp64 [STMPC_REC_NQ * (n_edges - 1) + 2],
 *                           if not NULL): row q * (n_edges - 1) + b, then the two totals.  One workgroup per row, a fixed summation tree whose
 *                           shape depends on N alone: equal inputs give equal bits.  Asynchronous
 *   stmpc_rec_read          host copies (synchronises; any pointer may be NULL): ring [N][depth][STMPC_REC_HDR + 3 Kmax] in chronological order with
 *                           length [N] valid records each (the rest zero), acc_env [STMPC_REC_NQ * (n_edges - 1) + 2][N], acc_reduced (reduced by this
 *                           call), status [N] of the world
 */
#define STMPC_REC_HDR 10
#define STMPC_REC_NQ 4
#define STMPC_REC_MAX_DEPTH 64
#define STMPC_REC_MAX_EDGES 32
typedef struct stmpc_rec stmpc_rec;
int  stmpc_rec_create(stmpc_ctx *ctx, int N, int Kmax, int depth, double tick_length, const double *edges, int n_edges, stmpc_rec **out);
void stmpc_rec_destroy(stmpc_rec *rec);
int  stmpc_rec_reset(stmpc_rec *rec, void *stream);
int  stmpc_rec_tick_device(stmpc_rec *rec, int N, int Kmax, const double *d_ego5, const int32_t *d_k, const double *d_ox, const double *d_ov,
                           const double *d_oa, const double *d_cmd_speed, const int32_t *d_takeover, void *stream);
int  stmpc_rec_reduce_device(stmpc_rec *rec, double *d_out, void *stream);
int  stmpc_rec_read(stmpc_rec *rec, double *ring, int32_t *length, double *acc_env, double *acc_reduced, int32_t *status);

/*
 * First-step shield controller, st.do_conditional_st_based_on_first_step(state, start_speed) (st.py:805-814), for N independent states: the
 * reference's cheaper way to put the solver behind a proposed command -- ONE predictor step and at most two solves per tick, where the combined
 * controller rolls out ROLLOUT_LENGTH policy evaluations.  (Additive: new entries only, no signature or struct of ABI 8 changes, so
 * STMPC_ABI_VERSION stays 8.)  It is not a stmpc_combined_cfg: the step predicts with predict_step_with_ego's DEFAULT min_crash_distance
 * (prediction.py:46) while the probe keeps COMBINATION_MIN_DISTANCE - CAR_LENGTH (st.py:800; p->comb_min_dist feeds both in the combined controller),
 * nothing stops at STOP_X, and the proposal is a speed, not a jerk.
 *   stmpc_first_step_device    <- st.py:805-814.  DEVICE pointers, states as stmpc_solve_batch_device takes them (ego5 [N][5], k [N], other_x / other_v
 *                       [N][Kmax]) plus start_speed [N].  Per state: next_state, crashed = predict_step_with_ego(start_speed, tick_length,
 *                       min_crash_distance) (st.py:806; laid out as the solver's state, start_s of the predicted position from the device map of
 *                       control.get_ego_s), crash_guaranteed = st.test_guaranteed_crash_from_state(next_state) (st.py:807: one batched solve over all
 *                       states -- the reference too asks before it looks at `crashed`), then cmd_speed = st.do_st_control(state) where crashed or
 *                       crash_guaranteed (st.py:808-811), else start_speed itself, bit for bit (st.py:813-814).  Outputs: cmd_speed [N], takeover [N]
 *                       (0 / 1), reason [N]: 0 the proposed speed, 1 the step crashed, 2 a crash is guaranteed afterwards (both: 1, the order of the
 *                       reference's `or`).  d_other_a may be NULL and is not read: the predictor takes no accelerations (prediction.py:75-97); the
 *                       argument completes the planner's view (stmpc_sim_view_device) for the caller's convenience.  Asynchronous on `stream` unless
 *                       sparse_control.  A controller path that cannot be re-sampled latches STMPC_EINVAL for stmpc_check_error only where that command
 *                       is used, as in stmpc_combined_decide_device.
 *   stmpc_first_step           the same for HOST pointers: stages, runs, copies back, synchronous (like stmpc_st_control_batch; a latched error is this
 *                       call's).  Optional outputs (any may be NULL) are the intermediate results: crashed [N], crash_guaranteed [N] (the probe's
 *                       verdict for EVERY state, crashed ones included), and the predicted state next_ego [N][5], next_other_x / next_other_v [N][Kmax].
 *   stmpc_first_step_counts    totals of stmpc_first_step_device on this context since the last reset: states decided, states taken over (counted on the
 *                       device by the deciding kernel; reading them synchronises), controller solves run (= takeovers with sparse_control, else =
 *                       decisions).  The combined controller's stmpc_combined_counts are not touched.
 *   stmpc_speed_from_jerk_device   <- control.get_ego_speed_from_jerk (control.py:160-171) for N states: the acceleration ego5[.][3] + jerk * tick_length
 *                       clamped to [p->a_min, p->a_max], the speed ego5[.][2] + that * tick_length clamped to [0, p->v_max] -- the function the combined
 *                       rollout applies inside its step kernel, on its own, so that a policy's jerk becomes this controller's proposal.  DEVICE
 *                       pointers, asynchronous.
 */
typedef struct stmpc_first_step_cfg {
    double tick_length;        /* Settings.TICK_LENGTH */
    double min_crash_distance; /* predict_step_with_ego's default, 5 (prediction.py:46) */
    int    sparse_control;     /* as stmpc_combined_cfg: 1 = solve st.do_st_control only for the taken-over states (ONE host round trip for their number; not
                                  capturable in a hipGraph), 0 = for all states, fully asynchronous.  Same outputs either way. */
} stmpc_first_step_cfg;
int stmpc_first_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_first_step_cfg *cfg, int N, int Kmax, const double *d_ego5,
                            const int32_t *d_k_count, const double *d_other_x, const double *d_other_v, const double *d_other_a /* may be NULL */,
                            const double *d_start_speed, double *d_cmd_speed, int32_t *d_takeover, int32_t *d_reason, void *stream);
int stmpc_first_step(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_first_step_cfg *cfg, int N, int Kmax, const double *ego, const int32_t *k_count,
                     const double *other_x, const double *other_v, const double *start_speed, double *cmd_speed, int32_t *takeover, int32_t *reason,
                     int32_t *crashed, int32_t *crash_guaranteed, double *next_ego, double *next_other_x, double *next_other_v);
int stmpc_first_step_counts(stmpc_ctx *ctx, int64_t *decisions, int64_t *takeovers, int64_t *control_solves, int reset);
int stmpc_speed_from_jerk_device(stmpc_ctx *ctx, const stmpc_params *p, double tick_length, int N, const double *d_ego5, const double *d_jerk,
                                 double *d_speed, void *stream);

/*
 * Reward groups: one vector environment split into R groups of n_per_reward_group consecutive environments, each rewarded under its own stmpc_env_cfg, in
 * the launches of a lone env (three per step).  The reference treats the reward as a per-run setting and compares rewards one TRAIN_DDPG run per setting:
 * dqn.get_reward_function and the four functions it picks (dqn.py:449-563, rl.py:168-174), the weights every file under its configs/ overrides, and the
 * env's INVALID_ACTION_PENALTY and action handling (merge_gym.py:25,83-140).  (Additive: new entries only, no signature or struct of ABI 8 changes, so
 * STMPC_ABI_VERSION stays 8.)
 * Rows [r * n_per_reward_group, (r + 1) * n_per_reward_group) of a grouped env are, bit for bit and through every autoreset, those rows of the env reset
 * through the plain entries with env_cfgs[r] -- observations, rewards, terminated / truncated, final observation and statistics, log rows, returns.  On a
 * world of traffic groups cell c pairs traffic c with reward c, so group r is the lone env of n_per_reward_group environments made from sim_cfgs[r] and
 * env_cfgs[r]; an ungrouped world is one world of R * n_per_reward_group environments whatever the rewards (the reward never feeds back into the world).
 *   May differ between groups: reward_function, crash_reward, success_reward, time_reward, wt_smooth, wt_safe, wt_efficient, alt_v_weight, alt_a_weight,
 *                   alt_j_weight, alt_d_weight, min_follow_distance, desired_speed (the reward's use of it), invalid_action_penalty.
 *   Must be equal (else STMPC_EINVAL naming the field): action_mode, action_values and n_action_values, tick_length, minimum_negative_jerk,
 *                   maximum_positive_jerk, max_negative_acceleration, max_positive_acceleration, max_speed, car_length, autoreset, log_capacity, features
 *                   (equal contents, or the same pointer).
 *   stmpc_reward_groups_env_reset_device (dqn.py:449-563, rl.py:168-174, merge_gym.py:25,83-140)   stmpc_env_reset_device / stmpc_env_reset_groups_device
 *                   with a table of R = 1 ... STMPC_ENV_REWARD_GROUPS_MAX env cfgs: validates everything, initialises the world -- G = 0: an ungrouped
 *                   world of R * n_per_reward_group environments from sim_cfgs[0]; G >= 1: traffic groups, where R must equal G and n_per_reward_group
 *                   n_per_traffic_group --, uploads the table (synchronises on `stream` for it) and resets every environment.  A refused call changes
 *                   nothing.  stmpc_sim_init_device / stmpc_sim_init_groups_device on the context end the env and its grouping.
 *   stmpc_reward_groups_env_step_device (dqn.py:449-563, rl.py:168-174, merge_gym.py:25,83-140)   stmpc_env_step_device on such an env, for either kind
 *                   of world: the arguments of stmpc_env_step_groups_device.  The context's table is read on the device (no copy, no synchronisation);
 *                   env_cfg supplies the shared fields, its reward fields are not read.  STMPC_EINVAL on an env without reward groups -- and the plain
 *                   stmpc_env_step_device / stmpc_env_step_groups_device return STMPC_EINVAL on an env with them, which they would reward with one cfg.
 *   stmpc_reward_groups_env_reward_device (dqn.py:449-563, rl.py:168-174, merge_gym.py:25,83-140)   stmpc_env_reward_device with the context's table: state
 *                   e is rewarded under group e / n_per_reward_group; N <= R * n_per_reward_group.
 *   stmpc_reward_groups_split (dqn.py:449-563, rl.py:168-174, merge_gym.py:25,83-140)   the current split (0, 0: one reward for every environment, or no env)
 */
#define STMPC_ENV_REWARD_GROUPS_MAX 64
int stmpc_reward_groups_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int G, int n_per_traffic_group,
                                         const stmpc_env_cfg *env_cfgs, int R, int n_per_reward_group, float *d_obs, int obs_stride, void *stream);
int stmpc_reward_groups_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_env_cfg *env_cfg, int N, const void *d_action, float *d_obs,
                                        int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs,
                                        double *d_final_stats, void *stream);
int stmpc_reward_groups_env_reward_device(stmpc_ctx *ctx, const stmpc_env_cfg *env_cfg, int N, int Kmax, const double *d_ego4, const int32_t *d_k,
                                          const double *d_ox, const double *d_ov, const double *d_oa, const double *d_jerk, const int32_t *d_crashed,
                                          const int32_t *d_arrived, double *d_reward, void *stream);
int stmpc_reward_groups_split(stmpc_ctx *ctx, int *R, int *n_per_group);

/*
 * Shielded vector environment: stmpc_env_step_device behind the first-step shield, st.do_conditional_st_based_on_first_step (st.py:805-814), without
 * leaving the device -- the loop a policy is DEPLOYED in (episodes: controller "first_step"), for training.  The env's action is a proposal; the shield
 * decides what is executed, and the step tells the learner what that was and how often it was overruled.  (Additive: new entries only, no signature or
 * struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 * One step, on `stream`: the env's action handling + the planner's view of the current state at row stride kmax (what stmpc_sim_view_device writes) + the
 * proposed speed (the speed stmpc_env_step_device would command; a finished environment proposes what its action would command from its last state, as
 * the episode runner does, and an action index out of range proposes the current speed), in one
 * kernel -> the body of stmpc_first_step_device on that view and proposal (the context's stmpc_first_step_counts advance) -> where the shield took over a
 * running environment: the commanded speed becomes the shield's, the projected jerk becomes (clip((cmd - v) / tick, a_min, a_max) - previous_acceleration)
 * / tick (AccelerationEnv._do_action's third branch, merge_gym.py:208-212, of the executed speed) and takeover_penalty * tick_length is added to the tick's
 * invalid-action reward -> the world step and the reward / observation / autoreset kernel of stmpc_env_step_device, unchanged.  The step equals, bit for
 * bit, that composition made from the public entries by a caller.
 *   stmpc_shield_env_reset_device   stmpc_env_reset_device + the context's shield buffers (view, proposal, decision, per-environment takeover counters,
 *                       zeroed) and the first-step controller's for either value of fs.sparse_control, sized here: the step allocates none of them.  STMPC_EINVAL
 *                       (before anything changes) for kmax outside 1 ... STMPC_KMAX_LIMIT and for a takeover_penalty that is negative or not finite.
 *   stmpc_shield_env_step_device    the arguments of stmpc_env_step_device, then d_takeover uint8 [N], d_reason int32 [N] (stmpc_first_step_device's codes),
 *                       d_executed_jerk fp64 [N] (the projected jerk after the shield), d_executed_action fp64 [N] (STMPC_ENV_CONTINUOUS_JERK only, may be
 *                       NULL; must be NULL for a discrete env, whose index is not rewritten: the action's own bits where the proposal stood, else
 *                       d_executed_jerk clipped to [minimum_negative_jerk, maximum_positive_jerk]), d_takeover_ticks int32 [N] (takeovers of the
 *                       environment's current episode up to and including this tick: in the rows where the step reports terminated | truncated, the
 *                       finished episode's).  A finished environment (no autoreset) gets takeover 0, reason 0, executed_jerk 0 and keeps its count.
 *                       Asynchronous with fs.sparse_control = 0; with 1 it makes the one host round trip of stmpc_first_step_device.  STMPC_EINVAL if the
 *                       context's environment was not reset through stmpc_shield_env_reset_device, N differs from the reset, the world has traffic groups
 *                       or the env reward groups, kmax is out of range or differs from the reset's.  The plain stmpc_env_step_device stays legal on such
 *                       an env: it is the unshielded step.
 */
typedef struct stmpc_shield_env_cfg {
    stmpc_first_step_cfg fs;     /* tick_length, min_crash_distance, sparse_control: as stmpc_first_step_device */
    double takeover_penalty;     /* added to the tick's reward as takeover_penalty * tick_length where the shield took over (0: none) */
    int32_t kmax;                /* row stride of the planner view handed to the shield, 1 ... STMPC_KMAX_LIMIT (the solver's vehicles per state) */
    int32_t reserved0;
} stmpc_shield_env_cfg;
int stmpc_shield_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg,
                                  const stmpc_shield_env_cfg *shield_cfg, int N, float *d_obs, int obs_stride, void *stream);
int stmpc_shield_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg,
                                 const stmpc_shield_env_cfg *shield_cfg, int N, const void *d_action, float *d_obs, int obs_stride, double *d_reward,
                                 uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats, uint8_t *d_takeover,
                                 int32_t *d_reason, double *d_executed_jerk, double *d_executed_action, int32_t *d_takeover_ticks, void *stream);

/*
 * Traffic mix: one ungrouped vector environment of N environments in which every episode draws its own traffic type -- domain randomisation at the
 * episode boundary, the autoreset included.  The reference trains one policy per traffic type (configs/train_{low,medium,default,moderate,fast}_*.json
 * differ in BASE_TRAFFIC_INTERVAL and OTHER_CAR_SPEED, control.py:215-226) and its cross_* configs measure such a policy on another type; a mixed env
 * lets one learner meet all of them in every row.  (Additive: new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 * The rule: episode j of environment e runs under type t(e, j) = the first t with u < cum[t], where u is the world's generator (splitmix64, 53 bits)
 * of (mix_seed, e) keyed by the episode index j in place of the draw counter, and cum is the running sum of weights / sum(weights), formed once on the
 * host in fp64, left to right, and set to exactly 1.0 from the last type of positive weight on (a type of weight 0 is never drawn).  The draw takes
 * nothing from the world's own draw counter: episode j starts from the start state of the lone world made from sim_cfgs[t(e, j)], environment e, seed
 * stmpc_env_episode_seed(seed, j), with the counter offset the plain env gives episode j.  So every episode is, bit for bit, episode j of row e of the
 * env reset through stmpc_env_reset_device with sim_cfgs[t(e, j)] when it receives the same actions, and a mix of T = 1 is that env.
 *   May differ between types: base_traffic_interval, other_car_speed, vary_traffic_start_times.
 *   Must be equal (else STMPC_EINVAL naming the field): every other field of stmpc_sim_cfg, the seed included (a mixed world has one seed) and the
 *                   route (equal points, or NULL alike).
 *   stmpc_traffic_mix_env_reset_device   stmpc_env_reset_device with a table of T = 1 ... STMPC_TRAFFIC_MIX_MAX sim cfgs and their weights (each finite
 *                   and >= 0, positive sum): validates everything, uploads the table (synchronises on `stream` for it; the table and the
 *                   per-environment types are sized here to their maximum and never reallocated under a running kernel), draws t(e, 0) and
 *                   resets every environment under it.  d_traffic_type (int32 [N], may be NULL) receives t(e, 0).  A refused call changes nothing.
 *                   stmpc_sim_init_device / stmpc_sim_init_groups_device and every other reset entry end the mix.
 *   stmpc_traffic_mix_env_step_device    stmpc_env_step_device on such an env: the arguments of stmpc_env_step_groups_device (the context keeps the
 *                   world's cfgs), then d_traffic_type int32 [N] (the type of the episode the row is in after this step) and d_final_traffic_type
 *                   int32 [N] (where terminated | truncated: the type of the episode that just ended; elsewhere the current type).  The finishing
 *                   episode's reward, final observation, statistics and log row are made under its own type, the next episode's start state and
 *                   its observation under the type drawn for it.  Three launches, no copy, no synchronisation.  STMPC_EINVAL -- and nothing changes
 *                   -- on an env that was not reset through stmpc_traffic_mix_env_reset_device or whose N differs; every other env step entry and
 *                   stmpc_sim_step_device return STMPC_EINVAL on a mixed env, which they would step under one cfg.  A log row holds its environment
 *                   and episode index, so its type is stmpc_traffic_mix_draw of them: the log has no column for it.
 *   stmpc_traffic_mix_draw               the rule on the host: t(env, episode) for cum[0 .. T) as above (no context; -1 for cum NULL or T outside
 *                   1 ... STMPC_TRAFFIC_MIX_MAX).
 */
#define STMPC_TRAFFIC_MIX_MAX 64
int stmpc_traffic_mix_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int T, const double *weights,
                                       uint64_t mix_seed, const stmpc_env_cfg *env_cfg, int N, float *d_obs, int obs_stride, int32_t *d_traffic_type,
                                       void *stream);
int stmpc_traffic_mix_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_env_cfg *env_cfg, int N, const void *d_action, float *d_obs,
                                      int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs,
                                      double *d_final_stats, int32_t *d_traffic_type, int32_t *d_final_traffic_type, void *stream);
int stmpc_traffic_mix_draw(uint64_t mix_seed, int env, uint32_t episode, const double *cum, int T);

/*
 * Combined-controller shield for the vector environment: stmpc_env_step_device behind dqn.RLAgent.do_combined_control (dqn.py:117-200), the controller
 * the reference deploys and evaluates (EVALUATE_COMBINED_DDPG; episodes: controller "combined"), without leaving the device -- for training.  The env's
 * action is the FIRST action of do_combined_control (the reference's agent.get_control(state)); rollout steps 2 ... L ask `actor` on the device, the
 * decision rules of dqn.py:144-200 choose what is executed, and the step reports it as stmpc_shield_env_step_device does.  (Additive: new entries only,
 * no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8.)
 * One step, on `stream`: the env's action handling + the planner's view of the current state at row stride kmax WITH the other vehicles' accelerations
 * (what stmpc_sim_view_device writes), into the start rows and the rollout's current rows + first_action = the action's jerk + the rollout's time
 * counter, in one kernel -> for step = 1 ... max(rollout_length, 1): from step 2 on the body of stmpc_actor_eval_device on the current rows with the
 * shield's counter, then the body of stmpc_rollout_step_device -> the body of stmpc_combined_decide_device (probe solve, controller solve, decision; the
 * context's stmpc_combined_counts advance) -> where the decision took over a running environment: the executed speed, projected jerk and takeover
 * penalty exactly as stmpc_shield_env_step_device applies them -> the world step and the reward / observation / autoreset kernel of
 * stmpc_env_step_device, unchanged.  The step equals, bit for bit, that composition made from the public entries by a caller.
 * The rollout's time counter (what the actor's TimeFeature input reads at rollout step s >= 2, stmpc_policy_features_device's d_evals):
 *   rollout_time 0 ("env")       it starts every tick at episode ticks + 1, so step s reads time_scale x (ticks + s - 1): the value a policy acting in
 *                                this env (one evaluation per tick, time = the episode's ticks) would read s - 1 ticks later.
 *   rollout_time 1 ("deployed")  a running count of ALL policy evaluations of the environment's current episode -- this tick's proposal counts one, every
 *                                rollout step s >= 2 whose rollout is still going on one more -- the reference's TimeFeature under do_combined_control.
 *                                It restarts when the environment's episode index moves on (autoreset); a finished environment keeps counting.
 *   stmpc_cshield_env_reset_device   stmpc_env_reset_device + every buffer of the step (start and current rows, first action, counter, decision,
 *                       per-environment takeover counters, zeroed; the combined controller's and, for either value of cc.sparse_control, the sparse
 *                       solve's), sized here: the step allocates none.  STMPC_EINVAL (before anything changes) unless env_cfg->action_mode is
 *                       STMPC_ENV_CONTINUOUS_JERK (the rollout policy is a continuous actor), cc.remember_last_choice is 0, kmax is 1 ...
 *                       STMPC_KMAX_LIMIT, takeover_penalty finite and >= 0, rollout_time 0 or 1, and actor (created, or a stmpc_actor_view_ddpg view) is on
 *                       the context's device with n_in = stmpc_policy_features_len(&features).
 *   stmpc_cshield_env_step_device    the arguments of stmpc_env_step_device, the cfg and the actor, then the four per-tick outputs of
 *                       stmpc_shield_env_step_device with `reason` in the combined controller's codes 0-4 (stmpc_combined_decide_device);
 *                       d_executed_action may be NULL.  A finished environment (no autoreset) proposes from its last state and is decided as the
 *                       episode runner decides it, gets takeover 0, reason 0, executed_jerk 0 and keeps its step state.  Asynchronous with
 *                       cc.sparse_control = 0; with 1 it makes the one host round trip of stmpc_combined_decide_device.  STMPC_EINVAL -- and nothing
 *                       changes -- if the context's environment was not reset through stmpc_cshield_env_reset_device, N, kmax, rollout_time or the
 *                       rollout length differ from the reset's, or the world has traffic groups, the env reward groups or a traffic mix.  Every other env
 *                       step entry and stmpc_sim_step_device return STMPC_EINVAL on such an env: they would execute the proposal unprotected.
 *   stmpc_cshield_env_evals_device   d_evals int32 [N]: the count the NEXT step's proposal is evaluated at (stmpc_policy_features_device's d_evals for
 *                       a policy that acts in this env): the episode's ticks under rollout_time 0, the running count under 1 (0 in a new episode).
 */
typedef struct stmpc_cshield_env_cfg {
    stmpc_combined_cfg cc;               /* as stmpc_combined_decide_device; remember_last_choice must be 0 (the env keeps no takeover history per episode) */
    stmpc_policy_features_cfg features;  /* the rollout actor's input (time_feature as the actor was built) */
    double takeover_penalty;             /* added to the tick's reward as takeover_penalty * tick_length where the controller took over (>= 0, finite) */
    int32_t kmax;                        /* row stride of the planner view, 1 ... STMPC_KMAX_LIMIT */
    int32_t rollout_time;                /* 0 "env", 1 "deployed" (above) */
} stmpc_cshield_env_cfg;
int stmpc_cshield_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg,
                                   const stmpc_cshield_env_cfg *shield_cfg, const stmpc_actor *actor, int N, float *d_obs, int obs_stride, void *stream);
int stmpc_cshield_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg,
                                  const stmpc_cshield_env_cfg *shield_cfg, const stmpc_actor *actor, int N, const void *d_action, float *d_obs,
                                  int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, float *d_final_obs, double *d_final_stats,
                                  uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk, double *d_executed_action, int32_t *d_takeover_ticks,
                                  void *stream);
int stmpc_cshield_env_evals_device(stmpc_ctx *ctx, int N, int32_t *d_evals, void *stream);

/*
 * Combined-controller shield for the DISCRETE vector environments (STMPC_ENV_JERK, STMPC_ENV_ACCELERATION): stmpc_env_step_device behind
 * dqn.RLAgent.do_combined_control (dqn.py:117-200), which DQNAgent inherits, with DQNAgent.get_control (dqn.py:375-380) -- a Q-network, its first argmax
 * and the action table -- proposing rollout steps 2 ... L on the device, so that a DQN learner trains in the closed loop it is deployed in.  (Additive:
 * new entries only, no signature or struct of ABI 8 changes, so STMPC_ABI_VERSION stays 8; stmpc_cshield_env_* above keeps every refusal it has.)
 * The env's action INDEX is the controller's first action.  One step, on `stream`: the env's action handling + the planner's view at row stride kmax
 * with the other vehicles' accelerations, into the start rows and the rollout's current rows + first_action, in one kernel -> for step = 1 ...
 * max(rollout_length, 1): from step 2 on the body of stmpc_qactor_eval_device (or of stmpc_pop_qactor_eval_device) on the current rows, then the body
 * of stmpc_rollout_step_device -> the body of stmpc_combined_decide_device (the context's stmpc_combined_counts advance) -> the takeover branch of
 * stmpc_shield_env_step_device with d_executed_action NULL (a takeover's speed is no table entry: the index is not rewritten) -> the world step and the
 * reward / observation / autoreset kernel of stmpc_env_step_device, unchanged.  The step equals, bit for bit, that composition made from the public
 * entries by a caller.
 * first_action is the jerk rollout step 1 applies: action_values[index] under STMPC_ENV_JERK; under STMPC_ENV_ACCELERATION
 * clip((action_values[index] - ego acceleration of the view) / tick_length, minimum_negative_jerk, maximum_positive_jerk) in fp64 -- under both what
 * stmpc_qactor_eval_device returns as d_jerk for that index on that state.  An index out of range latches the error word (stmpc_check_error) for a
 * running environment; running or not, the row commands its current speed and its first_action is 0.0.
 * A Q-network has no time feature, so there is no rollout time counter, no rollout_time and no *_evals_device entry.
 * The policy is EITHER qactor (created, or a stmpc_qactor_view_dqn view: a step queued after stmpc_dqn_update_device rolls out with the updated
 * weights; or a categorical one, stmpc_c51actor_create / stmpc_c51actor_view, likewise after stmpc_c51_update_device) on all N rows with qactor_pop NULL and n_per_member 0, OR qactor_pop with qactor NULL, member m on rows [m * n_per_member, (m + 1) *
 * n_per_member) and P * n_per_member == N.
 *   stmpc_qshield_env_reset_device   stmpc_env_reset_device + every buffer of the step, sized here: the step allocates none.  STMPC_EINVAL (before
 *                       anything changes) for STMPC_ENV_CONTINUOUS_JERK (use stmpc_cshield_env_*), cc.remember_last_choice != 0, kmax outside 1 ...
 *                       STMPC_KMAX_LIMIT, a takeover_penalty that is negative or not finite, features.time_feature != 0, both or neither policy
 *                       pointer, a policy on another device, n_in != stmpc_policy_features_len(&features), and for the lone Q-actor or any member:
 *                       n_actions != env_cfg->n_action_values, a mode that is not the env's action mode, a table that is not byte-identical to
 *                       env_cfg->action_values, in acceleration mode limits (stmpc_qactor_set_limits) that are not the env's; P * n_per_member != N.
 *   stmpc_qshield_env_step_device    the arguments of stmpc_env_step_device (d_action int32 [N]), the cfg and the policy, then d_takeover uint8 [N],
 *                       d_reason int32 [N] (the combined controller's codes 0-4), d_executed_jerk fp64 [N], d_takeover_ticks int32 [N] as
 *                       stmpc_shield_env_step_device writes them.  Asynchronous with cc.sparse_control = 0; with 1 the one host round trip of
 *                       stmpc_combined_decide_device.  STMPC_EINVAL -- and nothing changes -- for every refusal of the reset, if the context's
 *                       environment was not reset through stmpc_qshield_env_reset_device (a stmpc_cshield_env_reset_device context included), if N,
 *                       kmax, the rollout length, the policy pointer, n_per_member or n_action_values differ from the reset's, or the world has
 *                       traffic groups, the env reward groups, the first-step shield or a traffic mix.  Every other env step entry and
 *                       stmpc_sim_step_device return STMPC_EINVAL on such an env: they would execute the proposal unprotected.
 */
typedef struct stmpc_qshield_env_cfg {
    stmpc_combined_cfg cc;               /* as stmpc_combined_decide_device; remember_last_choice must be 0 (the env keeps no takeover history per episode) */
    stmpc_policy_features_cfg features;  /* the Q-network's input (time_feature must be 0) */
    double takeover_penalty;             /* added to the tick's reward as takeover_penalty * tick_length where the controller took over (>= 0, finite) */
    int32_t kmax;                        /* row stride of the planner view, 1 ... STMPC_KMAX_LIMIT */
    int32_t reserved0;
} stmpc_qshield_env_cfg;
int stmpc_qshield_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg,
                                   const stmpc_qshield_env_cfg *shield_cfg, const stmpc_qactor *qactor, const stmpc_qactor_pop *qactor_pop, int n_per_member,
                                   int N, float *d_obs, int obs_stride, void *stream);
int stmpc_qshield_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfg, const stmpc_env_cfg *env_cfg,
                                  const stmpc_qshield_env_cfg *shield_cfg, const stmpc_qactor *qactor, const stmpc_qactor_pop *qactor_pop, int n_per_member,
                                  int N, const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                                  float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk,
                                  int32_t *d_takeover_ticks, void *stream);

/*
 * First-step shield for grouped and mixed-traffic vector environments: stmpc_shield_env_step_device in front of the env's group axes -- traffic groups
 * (the reference's traffic types, configs/train_*_*.json, control.py:215-226), reward groups (its per-run reward settings, dqn.py:449-563,
 * merge_gym.py:25) and the traffic mix -- so that the per-traffic-type training matrix, a reward-shaping sweep and a mixed-traffic policy train in
 * the closed loop of st.do_conditional_st_based_on_first_step (st.py:805-814).  (Additive: new entries only, no signature or struct of ABI 8 changes,
 * so STMPC_ABI_VERSION stays 8.)
 * Nothing in the shield reads the traffic type or the reward.  One step is the lone shielded step, in as many launches: the action stage with the
 * world cfg of the environment's traffic group or of its episode's traffic type and the invalid-action penalty of its reward group -> the body of
 * stmpc_first_step_device on all N rows (the context's stmpc_first_step_counts advance by N) -> the takeover branch of
 * stmpc_shield_env_step_device under the takeover penalty of the environment's group -> the world step and the reward / observation / autoreset
 * kernel of the env's shape (stmpc_env_step_groups_device's, stmpc_reward_groups_env_step_device's, stmpc_traffic_mix_env_step_device's).  Rows of
 * group g are, bit for bit and through every autoreset, the rows of the lone env reset through stmpc_shield_env_reset_device with group g's sim cfg,
 * reward settings and takeover penalty; an episode of the shielded mix is the lone shielded env's episode of the drawn type.
 * The takeover penalties belong to the RESET: takeover_penalties is a host array of P values, P = the number of groups (G, or R), or 1 (one value for
 * every group), or P = 0 (takeover_penalties may be NULL): shield_cfg->takeover_penalty for every group.  Each finite and >= 0.  The step entries
 * check shield_cfg->takeover_penalty as the lone step does and do not read it further: they apply the reset's table.  The mix has no groups: its
 * reset takes shield_cfg->takeover_penalty.
 *   stmpc_shield_traffic_groups_env_reset_device / stmpc_shield_traffic_groups_env_step_device
 *                       stmpc_env_reset_groups_device / stmpc_env_step_groups_device behind the shield.
 *   stmpc_shield_reward_groups_env_reset_device / stmpc_shield_reward_groups_env_step_device
 *                       stmpc_reward_groups_env_reset_device / stmpc_reward_groups_env_step_device behind the shield: G = 0 (an ungrouped world from
 *                       sim_cfgs[0]) or G == R traffic groups that coincide with the reward groups.
 *   stmpc_shield_traffic_mix_env_reset_device / stmpc_shield_traffic_mix_env_step_device
 *                       stmpc_traffic_mix_env_reset_device / stmpc_traffic_mix_env_step_device behind the shield; the step's d_traffic_type and
 *                       d_final_traffic_type follow the shield's outputs.
 * Each reset takes the arguments of its unshielded twin with shield_cfg (and the penalties) after the env cfgs; each step the arguments of its twin
 * with shield_cfg after env_cfg, then the five outputs of stmpc_shield_env_step_device (d_executed_action NULL for a discrete env).  Every argument
 * check of a reset -- the twin's and stmpc_shield_env_reset_device's -- runs before anything changes; the shield's buffers and the penalty table are
 * sized by the reset (the upload synchronises on `stream`), the step allocates nothing.  A step returns STMPC_EINVAL -- before its first launch, the
 * world as it was -- on a context that was not reset through its own reset entry, for another N, and for a kmax that is out of range or not the
 * reset's.  Every other env step entry and the lone stmpc_shield_env_step_device return STMPC_EINVAL on such an env: unlike the lone shielded env,
 * whose unshielded step stmpc_env_step_device stays legal, a shielded env with groups or a mix has no unshielded step.
 */
int stmpc_shield_traffic_groups_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *cfgs, int G, int n_per_group,
                                         const stmpc_env_cfg *env_cfg, const stmpc_shield_env_cfg *shield_cfg, const double *takeover_penalties, int P,
                                         float *d_obs, int obs_stride, void *stream);
int stmpc_shield_traffic_groups_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_env_cfg *env_cfg, const stmpc_shield_env_cfg *shield_cfg, int N,
                                        const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                                        float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason, double *d_executed_jerk,
                                        double *d_executed_action, int32_t *d_takeover_ticks, void *stream);
int stmpc_shield_reward_groups_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int G, int n_per_traffic_group,
                                                const stmpc_env_cfg *env_cfgs, int R, int n_per_reward_group, const stmpc_shield_env_cfg *shield_cfg,
                                                const double *takeover_penalties, int P, float *d_obs, int obs_stride, void *stream);
int stmpc_shield_reward_groups_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_env_cfg *env_cfg, const stmpc_shield_env_cfg *shield_cfg,
                                               int N, const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated,
                                               uint8_t *d_truncated, float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason,
                                               double *d_executed_jerk, double *d_executed_action, int32_t *d_takeover_ticks, void *stream);
int stmpc_shield_traffic_mix_env_reset_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_sim_cfg *sim_cfgs, int T, const double *weights,
                                              uint64_t mix_seed, const stmpc_env_cfg *env_cfg, const stmpc_shield_env_cfg *shield_cfg, int N, float *d_obs,
                                              int obs_stride, int32_t *d_traffic_type, void *stream);
int stmpc_shield_traffic_mix_env_step_device(stmpc_ctx *ctx, const stmpc_params *p, const stmpc_env_cfg *env_cfg, const stmpc_shield_env_cfg *shield_cfg,
                                             int N, const void *d_action, float *d_obs, int obs_stride, double *d_reward, uint8_t *d_terminated,
                                             uint8_t *d_truncated, float *d_final_obs, double *d_final_stats, uint8_t *d_takeover, int32_t *d_reason,
                                             double *d_executed_jerk, double *d_executed_action, int32_t *d_takeover_ticks, int32_t *d_traffic_type,
                                             int32_t *d_final_traffic_type, void *stream);

/* Device arithmetic probe used by the parity tests: out[i] = a[i] op b[i] evaluated on the GPU
 * with the kernels' compile flags. op: 0 div, 1 sqrt(a), 2 mul, 3 add, 4 fma(a,a,b*b), 5 the five-operation
 * quotient a/b of the FASTDIV kernels, 6 their two-operation quotient a/b.  HOST pointers. */
int stmpc_probe_arith(stmpc_ctx *ctx, int op, const double *a, const double *b, double *out, int n);

/* The check the solver applies to dt, dt^2 and dt^3 (st_cy.pyx:46-50 divides by them once per edge) before it launches the kernels
 * that form these quotients as fma(x, zh, x*zl): returns 1 if that equals x / d for every double x (quotient in the normal range),
 * 0 if some x would round differently or the check cannot be completed -- the solver then divides with the ordinary IEEE sequence.
 * *zl (may be NULL) receives RN(1/d - RN(1/d)).  Host-only, no context. */
int stmpc_fastdiv2_check(double d, double *zl);

#ifdef __cplusplus
}
#endif
#endif /* STMPC_H */
