// stmpc_traffic_mix_kernels.hpp -- the traffic mix: one ungrouped vector environment whose every episode draws its own traffic type.  The reference
// trains one DDPG policy per traffic type (configs/train_{low,medium,default,moderate,fast}_*.json differ in BASE_TRAFFIC_INTERVAL and OTHER_CAR_SPEED,
// the highway flow of control.py:215-226) and its cross_* configs show what such a policy does on another type; here episode j of environment e runs
// under type t(e, j), drawn from a weighted table at every reset -- the autoreset of k_env_post included -- so one learner meets all of them.
//
//   t(e, j) = the first t with u < cum[t],  u = sim::uniform01(mix_seed, e, ctr = j)
// (the world's generator keyed by the episode index in place of the draw counter; `cum`: the running sum of the normalised weights, made once on the
// host in fp64, 1.0 exactly from the last type of positive weight on).  The draw takes nothing from the world's own counter: episode j still starts
// from sim_init_env(cfg of t(e, j), state, e, episode_seed(seed, j)) with the counter episode_ctr gives it.
//
// The type is a per-lane value, so what it selects is read as stmpc_env_groups_kernels.hpp reads a reward group's row: a device table of TrafficRow in
// global memory, read with plain per-lane (vector) loads after the thread's bounds check and patched into a copy of the by-value sim::Cfg that
// carries everything the types share.  (A by-value table in the kernel arguments comes in through scalar loads, one address per wavefront: a per-lane
// index into it would make the compiler copy the array to scratch.)  The table is at most 64 rows of 24 bytes and `cum` 64 doubles: after the first
// wavefront they are served from the L2 / vector L1 of every compute unit.
// Every kernel is the body of its lone twin, called, not copied: sim_init_env / sim_step_body of stmpc_cc_kernels.hpp, env_reset_body /
// env_post_tick / env_post_autoreset of stmpc_env_kernels.hpp.  k_env_post_mix is the one place where two cfgs meet: the finishing episode's view,
// reward, final observation, statistics and log row are its own type's, the start state of the next episode is initialised and observed under the
// type drawn for it.  k_env_act reads no sim cfg and serves a mixed env unchanged.
// Launch shape of the lone env: one thread per environment, 64-thread workgroups, a flat grid over the N rows.  No LDS, no atomic but the log's slot
// counter (env_post_tick's).
#pragma once
#include "stmpc_env_kernels.hpp"

namespace stmpc {
namespace env {

struct TrafficRow {                         // what may differ between traffic types (stmpc_sim_cfg: base_traffic_interval, other_car_speed, vary_traffic_start_times)
    double base_interval, other_speed;
    int vary_interval, pad;
};
struct TrafficMix {
    const TrafficRow *rows;                 // device, [T]
    const double *cum;                      // device, [T]: non-decreasing, cum[T - 1] == 1.0
    int *type;                              // device, [N]: the type of the episode each environment is in
    int T;
    unsigned long long seed;                // the mix seed
};

// The rule (restated in rl-mpc-lanemerging_amd/vec_env.py: traffic_mix_draw; the host entry stmpc_traffic_mix_draw calls this function).
// Always in [0, T): the last type is the answer when no earlier one is.
__host__ __device__ __forceinline__ int mix_draw(unsigned long long mix_seed, int e, unsigned j, const double *cum, int T) {
    unsigned ctr = j;
    const double u = sim::uniform01(mix_seed, e, ctr);
    int t = 0;
    while (t < T - 1 && !(u < cum[t])) ++t;
    return t;
}

// the shared cfg with the traffic of type t (0 <= t < T: mix_draw's value, kept in TrafficMix::type)
__device__ __forceinline__ sim::Cfg cfg_of_type(const sim::Cfg &c, const TrafficMix &m, int t) {
    const TrafficRow r = m.rows[t];
    sim::Cfg o = c;
    o.base_interval = r.base_interval; o.other_speed = r.other_speed; o.vary_interval = r.vary_interval;
    return o;
}

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
// Episode 0 of every environment: its type, k_sim_init's work under that type's cfg, then k_env_reset's.  traffic_type may be NULL.
__global__ void __launch_bounds__(64) k_env_reset_mix(ECfg c, sim::Cfg sc, TrafficMix m, int N, sim::State s, EState es, float *__restrict__ obs, int obs_stride,
                                                      int *__restrict__ traffic_type) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int t = mix_draw(m.seed, e, 0u, m.cum, m.T);
    m.type[e] = t;
    if (traffic_type) traffic_type[e] = t;
    const sim::Cfg ct = cfg_of_type(sc, m, t);
    sim::sim_init_env(ct, s, e, ct.seed);
    env_reset_body(c, ct, N, s, es, obs, obs_stride);
}

// sim::k_sim_step under the cfg of the episode each environment is in
__global__ void __launch_bounds__(64) k_sim_step_mix(DevP p, sim::Cfg sc, TrafficMix m, int N, sim::State s, const double *__restrict__ cmd_speed,
                                                     double crash_min_s) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    sim::sim_step_body(p, cfg_of_type(sc, m, m.type[e]), N, s, cmd_speed, crash_min_s);
}

// k_env_post: the tick under the current type; where the episode ended and autoreset is on, the next episode's type is drawn and stored, and its start
// state is made and observed under that type.  traffic_type: the type of the episode the row is in after this step; final_traffic_type: the type the
// tick ran under -- the finished episode's where terminated | truncated.
__global__ void __launch_bounds__(64) k_env_post_mix(ECfg c, sim::Cfg sc, TrafficMix m, int N, sim::State s, EState es, float *__restrict__ obs, int obs_stride,
                                                     double *__restrict__ rew, unsigned char *__restrict__ term, unsigned char *__restrict__ trunc,
                                                     float *__restrict__ final_obs, double *__restrict__ final_stats, int *__restrict__ traffic_type,
                                                     int *__restrict__ final_traffic_type) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int t = m.type[e];
    int next = t;
    if (env_post_tick(c, cfg_of_type(sc, m, t), 0, e, s, es, obs, obs_stride, rew, term, trunc, final_obs, final_stats)) {
        next = mix_draw(m.seed, e, (unsigned)es.episode[e] + 1u, m.cum, m.T);
        m.type[e] = next;
        env_post_autoreset(c, cfg_of_type(sc, m, next), c.seed, e, s, es, obs + (size_t)e * obs_stride);
    }
    traffic_type[e] = next;
    final_traffic_type[e] = t;
}
#endif

}  // namespace env
}  // namespace stmpc
