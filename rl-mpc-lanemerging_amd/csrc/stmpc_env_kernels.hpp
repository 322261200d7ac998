// stmpc_env_kernels.hpp -- the reference's gym environments (merge_gym.py: ContinuousJerkEnv, JerkEnv, AccelerationEnv) on the batched
// SUMO-free world of stmpc_cc_kernels.hpp (sim::), one thread per environment, 64-thread blocks.  One env step is three launches:
//   k_env_act    the env's action handling (merge_gym.py:83-100, 193-221): the commanded speed for sim::k_sim_step, the projected jerk
//                and the invalid-action reward;
//   sim::k_sim_step, unchanged;
//   k_env_post   the view of the new state (HighwayState.from_sumo: every vehicle inside the sensor radius, front to back), the reward
//                (dqn.py:459-563, rl.py:168-174), terminated / truncated (merge_gym.py:102-140), the observation (dqn.py:389-446 without the
//                time feature, float32; zeros after a crash or an arrival) and, for an environment that finished, its final observation,
//                its statistics row and -- with autoreset -- the reset to its next episode and the observation of that start state.
// Plain fp64 in the reference's operation order under the library's flags (-ffp-contract=off).  One exception, documented in DESIGN.md
// section 11: the reference's x ** 2 is a libm pow call (not correctly rounded in glibc >= 2.28); here it is the correctly rounded x * x.
#pragma once
#include "stmpc_cc_kernels.hpp"

namespace stmpc {
namespace env {

enum { ACT_CONTINUOUS_JERK = 0, ACT_JERK = 1, ACT_ACCELERATION = 2 };                      // STMPC_ENV_* of include/stmpc.h
enum { R_CONTINUOUS = 0, R_SLOTTED = 1, R_SLOTTED_JERK = 2, R_ST = 3 };                       // STMPC_REWARD_*
constexpr int NSTAT = sim::NACC + 3;        // final statistics row: acc[12], status, ticks, episode return (STMPC_ENV_NSTAT)
constexpr int NLOG = NSTAT + 2;             // episode log row: the statistics row, environment, episode index (STMPC_ENV_LOG_COLS)

struct ECfg {
    double tick, crash_r, success_r, time_r, wt_smooth, wt_safe, wt_eff, alt_v, alt_a, alt_j, alt_d, min_follow, desired_speed, car_length;
    double penalty, j_min, j_max, a_min, a_max, v_max;
    int mode, reward, n_actions, autoreset, log_cap, obs_len;
    const double *actions;                  // device copy of the discrete action table (JERK_VALUES_DQN / ACCELERATION_VALUES_DQN)
    unsigned long long seed;                // the run's seed: episode j >= 1 of an environment starts from episode_seed(seed, j)
    FeatCfg f;                              // time_feature = 0
};
struct EState {                             // device arrays, [N] unless noted
    int *episode;                           // episodes started so far minus one (0 after stmpc_env_reset_device)
    double *prev_a;                         // JerkEnv.previous_acceleration
    double *pjerk, *inv;                    // JerkEnv.projected_jerk, JerkEnv.invalid_action_reward of the current tick
    double *ret;                            // running return of the episode
    double *cmd;                            // commanded speed handed to sim::k_sim_step
    int *live;                              // the environment was running when the tick began
    double *vx, *vv, *va;                   // [N][sim::KS] the view of the new state
    int *k;                                 // vehicles in the view
    double *log;                            // [log_cap][NLOG] finished episodes since the last drain
    unsigned *log_n;                        // rows appended (may exceed log_cap: those rows were dropped)
    unsigned *err;                          // latched: a discrete action index out of range
};

// Seed of episode j of a run seeded `seed` (j = 0: the seed itself, so episode 0 is stmpc_sim_init_device's): splitmix64 of seed + j * golden gamma.
// Restated in rl-mpc-lanemerging_amd/vec_env.py (episode_seed) and by the host entry stmpc_env_episode_seed.
__host__ __device__ __forceinline__ unsigned long long episode_seed(unsigned long long seed, unsigned j) {
    if (j == 0) return seed;
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)j;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}
// Draw counter of episode j after its reset: k_sim_step draws the traffic of every environment from the run's seed, so the draws of episodes
// j < 2^16 start 2^16 apart and do not overlap while an episode draws fewer than 2^16 values.  A tick inserts at most one vehicle and an
// insertion draws at most three values (two for cruise_speed with speed_dev > 0, one for the next delay), so that holds for episodes of up to
// 21845 ticks (MAX_EPISODE_LENGTH 100 s: 500 ticks).  From j = 2^16 on, j << 16 would wrap and replay the offsets of episodes 0, 1, ...; those
// episodes take the high half of their episode seed as the offset instead (pseudo-random starting points: no systematic replay, a 2^-16 chance
// per episode of landing within an earlier episode's window).
__device__ __forceinline__ unsigned episode_ctr(unsigned init_draws, unsigned j, unsigned long long ep_seed) {
    return init_draws + (j < 65536u ? (j << 16) : ((unsigned)(ep_seed >> 32) & 0xFFFF0000u));
}

__device__ __forceinline__ double sq(double x) { return x * x; }

// control.get_ego_speed_from_jerk, control.py:160-171
__device__ __forceinline__ double speed_from_jerk(const ECfg &c, double v, double a, double jerk) {
    double na = a + jerk * c.tick;
    if (na > c.a_max) na = c.a_max;
    if (na < c.a_min) na = c.a_min;
    double nv = v + na * c.tick;
    if (nv > c.v_max) nv = c.v_max;
    if (nv < 0) nv = 0;
    return nv;
}
__device__ __forceinline__ double clip(double x, double lo, double hi) { x = x < lo ? lo : x; return x > hi ? hi : x; }      // np.clip

// JerkEnv._handle_jerk (merge_gym.py:83-96) + control.set_ego_jerk (control.py:174-179): v, a = the ego's speed and acceleration now
// (previous_state.ego_speed and TraCI's values are the same state here), prev_a = previous_acceleration.
__device__ __forceinline__ double handle_jerk(const ECfg &c, double v, double a, double prev_a, double jerk, double &pjerk, double &inv) {
    double pa = prev_a + jerk * c.tick;
    double ps = v + pa * c.tick;
    if (pa > c.a_max || pa < c.a_min) {
        inv = c.penalty * c.tick;
        pa = clip(pa, c.a_min, c.a_max);
    } else if (ps > c.v_max || ps < 0) {
        inv = c.penalty * c.tick;
        ps = clip(ps, 0.0, c.v_max);
        pa = (ps - v) / c.tick;
    } else {
        inv = 0.0;
    }
    pjerk = (pa - prev_a) / c.tick;
    return speed_from_jerk(c, v, a, jerk);
}
// AccelerationEnv._do_action, merge_gym.py:193-214
__device__ __forceinline__ double handle_acceleration(const ECfg &c, double v, double a, double prev_a, double acc, double &pjerk, double &inv) {
    double pa = acc;
    double ps = v + pa * c.tick;
    pjerk = (pa - prev_a) / c.tick;
    if (pjerk > c.j_max) {
        inv = c.penalty * c.tick;
        pjerk = c.j_max;
        return speed_from_jerk(c, v, a, c.j_max);
    } else if (pjerk < c.j_min) {
        inv = c.penalty * c.tick;
        pjerk = c.j_min;
        return speed_from_jerk(c, v, a, c.j_min);
    } else if (ps > c.v_max || ps < 0) {
        inv = c.penalty * c.tick;
        ps = clip(ps, 0.0, c.v_max);
        pa = (ps - v) / c.tick;
        pjerk = (pa - prev_a) / c.tick;
        return ps;
    }
    inv = 0.0;
    return ps;
}

// The reward of one state (dqn.get_reward_function, dqn.py:449-460).  xs: the state's other_xs (front to back, n of them);
// HighwayState.get_closest_cars (prediction.py:162-182) picks the car ahead and the car behind from it.
__device__ __forceinline__ double reward(const ECfg &c, double ex, double ey, double ev, double ea, const double *xs, int n, double jerk, bool crashed, bool arrived) {
    if (c.reward == R_SLOTTED || c.reward == R_SLOTTED_JERK) {               // rl.slotted_reward (rl.py:168-174), dqn.slotted_reward_with_jerk (dqn.py:557-563)
        if (crashed) return c.crash_r;
        if (arrived) return c.success_r;
        if (c.reward == R_SLOTTED) return c.time_r * c.tick;
        return c.time_r * c.tick - c.alt_j * sq(jerk) * c.tick;
    }
    const bool st = c.reward == R_ST;
    double m_abs = 0.0, m_a = 0.0, m_b = 0.0, m_c = 0.0, m_d = 0.0;       // continuous: smooth, safe, efficient; st: speed, acceleration, jerk, distance
    if (crashed) m_abs = -10.0;
    else if (arrived) m_abs = 10.0;
    else {
        int behind = -1, last = -1;
        for (int i = 0; i < n; ++i) {
            if (xs[i] < ex) { behind = i; break; }
            last = i;
        }
        const int front = last;
        if (st) {
            m_c = -sq(jerk) * c.tick;
            m_a = -c.tick * sq(ev - c.desired_speed);
            m_b = -c.tick * sq(ea);
        } else {
            m_a = -fabs(jerk) * c.tick;
        }
        if (dev_ego_s(ex, ey) > 0) {
            const double front_d = front != -1 ? xs[front] - ex - c.car_length : __builtin_inf();
            const double back_d = behind != -1 ? ex - xs[behind] - c.car_length : __builtin_inf();
            const double md = back_d < front_d ? back_d : front_d;                  // Python's min: the first of equal values
            double m;
            if (md < c.min_follow) m = st ? -2.0 / (md > 1.0 ? md : 1.0) : -1.0;    // (max(min_distance, 1): 1 unless min_distance > 1)
            else if (md == __builtin_inf()) m = 0.0;
            else if (md != md) m = 0.0;
            else m = -1.0 / md;
            m *= c.tick;
            if (st) m_d = m; else m_b = m;
        }
        if (!st) m_c = -c.tick * fabs(ev - c.desired_speed);
    }
    if (st) return c.alt_a * m_b + c.alt_d * m_d + c.alt_j * m_c + c.alt_v * m_a + m_abs;
    return c.wt_smooth * m_a + c.wt_safe * m_b + c.wt_eff * m_c + m_abs;
}

// HighwayState.from_sumo (prediction.py:112-142) of environment e into its [KS] view rows: every vehicle inside the sensor radius (plane distance,
// the highway lane at y = -1.6), in list order (front to back) -- k_sim_view's rule without the Kmax cut.
__device__ __forceinline__ int env_view(const sim::Cfg &sc, const sim::State &s, const EState &es, int e) {
    const double ex = s.ego4[e * 4 + 0], ey = s.ego4[e * 4 + 1];
    int k = 0;
    const int n = s.nveh[e];
    double *vx = es.vx + (size_t)e * sim::KS, *vv = es.vv + (size_t)e * sim::KS, *va = es.va + (size_t)e * sim::KS;
    for (int i = 0; i < n; ++i) {
        const double x = s.vx[(size_t)e * sim::KS + i];
        const double dx = x - ex, dy = -1.6 - ey;
        if (sqrt(dx * dx + dy * dy) < sc.sensor_radius) { vx[k] = x; vv[k] = s.vv[(size_t)e * sim::KS + i]; va[k] = s.va[(size_t)e * sim::KS + i]; ++k; }
    }
    es.k[e] = k;
    return k;
}
__device__ __forceinline__ void env_obs(const ECfg &c, const sim::Cfg &sc, const sim::State &s, const EState &es, int e, float *row) {
    env_view(sc, s, es, e);
    dev_policy_features(c.f, e, sim::KS, s.ego4, es.k, es.vx, es.vv, es.va, nullptr, nullptr, row);
}

// The env's action handling for environment e of the arrays `action` points at (ContinuousJerkEnv / JerkEnv / AccelerationEnv._do_action, merge_gym.py:83-100,
// 193-221): a continuous jerk (not clipped to the Box: the reference does not either), or an index into the table of jerks or of accelerations.  The one
// dispatch of k_env_act, k_env_act_rg and k_shield_env_pre.  Returns "the index is out of range": cmd is then left to the caller, pjerk and inv are 0.
__device__ __forceinline__ bool handle_action(const ECfg &c, const void *__restrict__ action, int e, double v, double a, double prev_a, double &cmd, double &pjerk,
                                              double &inv) {
    pjerk = 0.0; inv = 0.0;
    if (c.mode == ACT_CONTINUOUS_JERK) {
        cmd = handle_jerk(c, v, a, prev_a, ((const double *)action)[e], pjerk, inv);
        return false;
    }
    const int idx = ((const int *)action)[e];
    if (idx < 0 || idx >= c.n_actions) return true;
    if (c.mode == ACT_JERK) cmd = handle_jerk(c, v, a, prev_a, c.actions[idx], pjerk, inv);
    else cmd = handle_acceleration(c, v, a, prev_a, c.actions[idx], pjerk, inv);
    return false;
}

// k_env_act's body with the cfg of environment e (the reward groups' kernel passes the group's penalty in it)
__device__ __forceinline__ void env_act_body(const ECfg &c, int e, const sim::State &s, const EState &es, const void *__restrict__ action) {
    const double v = s.ego4[e * 4 + 2], a = s.ego4[e * 4 + 3], prev_a = es.prev_a[e];
    double pjerk, inv, cmd;
    if (handle_action(c, action, e, v, a, prev_a, cmd, pjerk, inv)) {
        es.err[0] = 1u;                                                    // (reported by stmpc_check_error; the ego keeps its speed)
        cmd = __builtin_nan("");
    }
    es.cmd[e] = cmd; es.pjerk[e] = pjerk; es.inv[e] = inv;
}
#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
__global__ void __launch_bounds__(64) k_env_act(ECfg c, int N, sim::State s, EState es, const void *__restrict__ action) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int live = s.status[e] == 0;
    es.live[e] = live;
    if (!live) return;                                                     // (k_sim_step idles finished environments)
    env_act_body(c, e, s, es, action);
}
#endif

// `es` moved on by `off` environments (a traffic group's slice); the episode log, its counter and the error word stay the world's
__device__ __forceinline__ EState estate_slice(const EState &es, size_t off) {
    return EState{es.episode + off, es.prev_a + off, es.pjerk + off, es.inv + off, es.ret + off, es.cmd + off, es.live + off, es.vx + off * sim::KS,
                  es.vv + off * sim::KS, es.va + off * sim::KS, es.k + off, es.log, es.log_n, es.err};
}

// JerkEnv.step after control.step() (merge_gym.py:102-140), then the vector env's bookkeeping: k_env_post's body for the N environments the state
// and step arrays point at.  `seed`: the run's seed of these environments (ECfg::seed; a traffic group's own); `row0`: the world's row of
// environment 0 (the environment column of a log row holds row0 + e).
//
// The body in its two halves, split where the next episode begins (the traffic mix of stmpc_traffic_mix_kernels.hpp draws the next episode's cfg between
// them; every other kernel runs both under its one cfg through env_post_body).  env_post_tick: environment e's tick under the cfg of the episode it is
// in -- the view, the reward, the flags, the observation and, where the episode ended, its final observation, statistics row and log row.  Returns
// "the episode ended and autoreset is on": the caller then starts the next episode with env_post_autoreset.
__device__ __forceinline__ bool env_post_tick(const ECfg &c, const sim::Cfg &sc, int row0, int e, const sim::State &s, const EState &es, float *__restrict__ obs,
                                              int obs_stride, double *__restrict__ rew, unsigned char *__restrict__ term, unsigned char *__restrict__ trunc,
                                              float *__restrict__ final_obs, double *__restrict__ final_stats) {
    const int status = s.status[e];
    float *row = obs + (size_t)e * obs_stride;
    if (!es.live[e]) {                                                     // finished before this tick (autoreset off): idles
        if (status == 3) env_obs(c, sc, s, es, e, row); else for (int q = 0; q < c.obs_len; ++q) row[q] = 0.0f;
        rew[e] = 0.0; term[e] = 0; trunc[e] = 0;
        return false;
    }
    const bool crashed = status == 2, arrived = status == 1;
    const double ex = s.ego4[e * 4 + 0], ey = s.ego4[e * 4 + 1], ev = s.ego4[e * 4 + 2], ea = s.ego4[e * 4 + 3];
    double r;
    if (crashed || arrived) {                                              // HighwayState.empty_state() and the projected jerk; zero observation
        r = reward(c, 0.0, 0.0, 0.0, 0.0, nullptr, 0, es.pjerk[e], crashed, arrived) + es.inv[e];
        for (int q = 0; q < c.obs_len; ++q) row[q] = 0.0f;
    } else {
        const int k = env_view(sc, s, es, e);
        const double jerk = (ea - es.prev_a[e]) / c.tick;
        r = reward(c, ex, ey, ev, ea, es.vx + (size_t)e * sim::KS, k, jerk, false, false) + es.inv[e];
        dev_policy_features(c.f, e, sim::KS, s.ego4, es.k, es.vx, es.vv, es.va, nullptr, nullptr, row);
        if (status == 0) es.prev_a[e] = ea;
    }
    const double ret = es.ret[e] + r;
    rew[e] = r;
    term[e] = crashed || arrived;
    trunc[e] = status == 3;
    if (status == 0) { es.ret[e] = ret; return false; }
    // the episode ended on this tick
    if (final_obs) { float *fo = final_obs + (size_t)e * obs_stride; for (int q = 0; q < c.obs_len; ++q) fo[q] = row[q]; }
    const double *acc = s.acc + (size_t)e * sim::NACC;
    const int ep = es.episode[e];
    if (final_stats) {
        double *fs = final_stats + (size_t)e * NSTAT;
        for (int q = 0; q < sim::NACC; ++q) fs[q] = acc[q];
        fs[sim::NACC] = (double)status; fs[sim::NACC + 1] = (double)s.ticks[e]; fs[sim::NACC + 2] = ret;
    }
    const unsigned slot = atomicAdd(es.log_n, 1u);
    if (slot < (unsigned)c.log_cap) {
        double *lg = es.log + (size_t)slot * NLOG;
        for (int q = 0; q < sim::NACC; ++q) lg[q] = acc[q];
        lg[sim::NACC] = (double)status; lg[sim::NACC + 1] = (double)s.ticks[e]; lg[sim::NACC + 2] = ret; lg[NSTAT] = (double)(row0 + e); lg[NSTAT + 1] = (double)ep;
    }
    if (!c.autoreset) { es.ret[e] = ret; return false; }
    return true;
}
// The autoreset of environment e, whose episode es.episode[e] has just ended: episode j = es.episode[e] + 1 starts from sim_init_env under `sc` -- the
// NEXT episode's cfg -- and episode_seed(seed, j), and its start state is observed into the environment's observation row.
__device__ __forceinline__ void env_post_autoreset(const ECfg &c, const sim::Cfg &sc, unsigned long long seed, int e, const sim::State &s, const EState &es,
                                                   float *__restrict__ row) {
    const unsigned j = (unsigned)es.episode[e] + 1u;
    const unsigned long long ep_seed = episode_seed(seed, j);
    sim::sim_init_env(sc, s, e, ep_seed);
    s.rng[e] = episode_ctr(s.rng[e], j, ep_seed);
    es.episode[e] = (int)j; es.prev_a[e] = 0.0; es.ret[e] = 0.0;          // JerkEnv.reset (merge_gym.py:142-161)
    env_obs(c, sc, s, es, e, row);
}
__device__ __forceinline__ void env_post_body(const ECfg &c, const sim::Cfg &sc, unsigned long long seed, int row0, int N, const sim::State &s, const EState &es,
                                              float *__restrict__ obs, int obs_stride, double *__restrict__ rew, unsigned char *__restrict__ term,
                                              unsigned char *__restrict__ trunc, float *__restrict__ final_obs, double *__restrict__ final_stats) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    if (env_post_tick(c, sc, row0, e, s, es, obs, obs_stride, rew, term, trunc, final_obs, final_stats))
        env_post_autoreset(c, sc, seed, e, s, es, obs + (size_t)e * obs_stride);
}
#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
__global__ void __launch_bounds__(64) k_env_post(ECfg c, sim::Cfg sc, int N, sim::State s, EState es, float *__restrict__ obs, int obs_stride, double *__restrict__ rew,
                                                 unsigned char *__restrict__ term, unsigned char *__restrict__ trunc, float *__restrict__ final_obs,
                                                 double *__restrict__ final_stats) {
    env_post_body(c, sc, c.seed, 0, N, s, es, obs, obs_stride, rew, term, trunc, final_obs, final_stats);
}
#endif

// Observation of every environment's current state and a fresh episode bookkeeping (stmpc_env_reset_device, after k_sim_init).
__device__ __forceinline__ void env_reset_body(const ECfg &c, const sim::Cfg &sc, int N, const sim::State &s, const EState &es, float *__restrict__ obs, int obs_stride) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    es.episode[e] = 0; es.prev_a[e] = 0.0; es.ret[e] = 0.0; es.pjerk[e] = 0.0; es.inv[e] = 0.0; es.live[e] = 1;
    if (obs) env_obs(c, sc, s, es, e, obs + (size_t)e * obs_stride);
}
#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
__global__ void __launch_bounds__(64) k_env_reset(ECfg c, sim::Cfg sc, int N, sim::State s, EState es, float *__restrict__ obs, int obs_stride) {
    env_reset_body(c, sc, N, s, es, obs, obs_stride);
}
#endif

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
// The reward for arbitrary batched states (stmpc_env_reward_device): ego4 [N][4], other_x [N][Kmax] front to back, k [N].
__global__ void __launch_bounds__(64) k_env_reward(ECfg c, int N, int Kmax, const double *__restrict__ ego4, const int *__restrict__ k, const double *__restrict__ ox,
                                                   const double *__restrict__ jerk, const int *__restrict__ crashed, const int *__restrict__ arrived, double *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    int n = k[e];
    n = n < 0 ? 0 : (n > Kmax ? Kmax : n);
    out[e] = reward(c, ego4[(size_t)e * 4 + 0], ego4[(size_t)e * 4 + 1], ego4[(size_t)e * 4 + 2], ego4[(size_t)e * 4 + 3], ox + (size_t)e * Kmax, n, jerk[e],
                    crashed && crashed[e] != 0, arrived && arrived[e] != 0);
}
#endif

}  // namespace env
}  // namespace stmpc
