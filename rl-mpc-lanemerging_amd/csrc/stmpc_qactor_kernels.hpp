// stmpc_qactor_kernels.hpp -- a trained DQN policy in the combined controller and the episode runner, one launch per evaluation: the reference's
// DQNAgent.get_control (dqn.py:375-380) for N states = state vector (dqn.py:389-446, dev_policy_features, no time feature) -> Q(s) -> first argmax
// -> the action table's entry.  The Q-network is a DQN learner's (stmpc_dqn_kernels.hpp): the forward pass is dqn_q, the function k_dqn_act and
// k_dqn_fwd call, on the same packed operands, and the argmax is dqn_argmax -- so Q, the index and the jerk are the bits learner.act gives on the
// same input vectors, for a view of a learner's network (online or target) as for a network packed from plain tensors by the learner's own path.
//
// gfx950 mapping: k_dqn_act's -- one workgroup of AT_THREADS per AT_TM = 16 states, X 16 x 32, the hidden activations and Q in LDS (DdpgTile), both
// layers v_mfma_f32_16x16x4_f32 loops -- with k_actor_eval's first stage in front: one thread per state writes its input vector into the X tile.
//
// The action table (`A` doubles, device memory, per actor) holds what the learner's env executes for an index:
//   jerk mode (sumo-jerk-v0: JERK_VALUES_DQN)                  jerk = table[a]
//   acceleration mode (sumo-accel-v0: ACCELERATION_VALUES_DQN)  jerk = clip((table[a] - ego acceleration) / tick_length, min_jerk, max_jerk), fp64
// The acceleration rule is AccelerationEnv._do_action's projected jerk (merge_gym.py:194-204) before its speed clamp, with the evaluated state's own
// acceleration in the place of the env's previous_acceleration.  The reference has no evaluator for a network trained on that env (its get_control
// reads JERK_VALUES_DQN whatever the env was): the rule is this project's.
//
// The arithmetic is one __device__ body, qactor_eval_body, with two entries: k_qactor_eval (a lone actor on N rows) and k_qactor_eval_pop of
// stmpc_qactor_pop_kernels.hpp (P actors, each on its own slice of one batch).
#pragma once
#include "stmpc_dqn_kernels.hpp"

namespace stmpc {

struct QActorOut {                  // what one evaluation writes; rows at or beyond N are never written
    const double *table;            // [A] the action table
    double tick, jerk_min, jerk_max;      // acceleration mode's constants (unread in jerk mode)
    int accel;                      // 0: jerk mode, 1: acceleration mode
    int feat_stride;
    float *feat;                    // (may be null) [N][feat_stride]: the input vectors as the network saw them
    int *action;                    // (may be null) [N]: the first maximum's index
    float *q;                       // (may be null) [N][A]: Q(s)
    double *jerk;                   // [N]
};

// The jerk that index a stands for on the state of global row e: the table's entry, or acceleration mode's rule on it (fp64).  Shared with
// k_c51actor_eval (stmpc_c51actor_kernels.hpp)
__device__ __forceinline__ double qactor_jerk(const QActorOut &o, int a, const double *__restrict__ ego4, int e) {
    double v = o.table[a];
    if (o.accel) {
        v = (v - ego4[(size_t)e * 4 + 3]) / o.tick;
        v = v < o.jerk_min ? o.jerk_min : (v > o.jerk_max ? o.jerk_max : v);
    }
    return v;
}

// The evaluation of rows [row0 + 16 blockIdx.x, + 16) with the network of D, as far as row0 + n_rows: row0 = 0 and n_rows = N for a lone actor; a
// member of a population has its slice's first row and length here.  The state arrays, live and the outputs of o are indexed by the global row.
// D: the learner's struct (a view) or one with base.q, base.n_obs, base.h1p, A and Ap alone (a created actor, a population's member); neither the
// counters nor the workspace are read or written.  live (null at step 1) is passed on to dev_policy_features, which reads it for the time feature
// only: without one, the rows of finished rollouts are evaluated like the others and their jerks ignored by the rollout, as k_actor_eval's are
__device__ __forceinline__ void qactor_eval_body(const FeatCfg &f, const DqnDev &D, int target, int row0, int n_rows, int Kmax, const double *__restrict__ ego4,
                                                 const int *__restrict__ k_count, const double *__restrict__ ox, const double *__restrict__ ov,
                                                 const double *__restrict__ oa, const int *__restrict__ live, const QActorOut &o, unsigned char *qa_smem) {
    const DdpgDev &L = D.base;
    const DdpgTile T = ddpg_tile(qa_smem, L.h1p, D.Ap);
    const int tid = threadIdx.x, l0 = blockIdx.x * AT_TM, row = tid >> 5, part = tid & 31, l = l0 + row, e = row0 + l;
    for (int x = tid; x < AT_TM * AT_KIN; x += blockDim.x) T.X[x] = 0.f;       // pad columns and the rows beyond n_rows
    __syncthreads();
    if (tid < AT_TM && l0 + tid < n_rows) dev_policy_features(f, row0 + l0 + tid, Kmax, ego4, k_count, ox, ov, oa, live, nullptr, T.X + tid * AT_KIN);
    __syncthreads();
    if (o.feat && l < n_rows && part < L.n_obs) o.feat[(size_t)e * o.feat_stride + part] = T.X[row * AT_KIN + part];
    dqn_q(D, T, T.X, target != 0);
    float qbest;
    const int a = dqn_argmax(T.H2 + (size_t)row * T.h2_ld, D.A, qbest);
    if (l >= n_rows) return;
    if (o.q) for (int j = part; j < D.A; j += 32) o.q[(size_t)e * D.A + j] = T.H2[(size_t)row * T.h2_ld + j];
    if (part != 0) return;
    o.jerk[e] = qactor_jerk(o, a, ego4, e);
    if (o.action) o.action[e] = a;
}

__global__ void __launch_bounds__(AT_THREADS) k_qactor_eval(FeatCfg f, DqnDev D, int target, int N, int Kmax, const double *__restrict__ ego4,
                                                            const int *__restrict__ k_count, const double *__restrict__ ox, const double *__restrict__ ov,
                                                            const double *__restrict__ oa, const int *__restrict__ live, QActorOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qa_smem[];
    qactor_eval_body(f, D, target, 0, N, Kmax, ego4, k_count, ox, ov, oa, live, o, qa_smem);
}

}  // namespace stmpc
