// stmpc_c51actor_kernels.hpp -- a trained categorical (C51) policy in the combined controller and the episode runner, one launch per evaluation:
// DQNAgent.get_control's job (dqn.py:375-380) for the distributional head of the reference's third agent (rainbow.py), for N states = state vector
// (dqn.py:389-446, dev_policy_features, no time feature) -> logits -> E[Z(s, a)] for every real action -> first maximum -> the action table's entry.
//
// It is k_qactor_eval (stmpc_qactor_kernels.hpp) with the expected values in Q's place.  The first stage is qactor_eval_body's; the forward pass is
// dqn_q on the learner's packed operands, the function k_c51_act and k_c51_fwd call; the argmax is c51_greedy unchanged (fp64 softmax statistics, a
// fixed-order butterfly, a loop over a < A so that pad columns belong to no action, the first maximum of the float32 values); the table is read by
// qactor_jerk, the function k_qactor_eval calls.  So the expected values, the index and the jerk are the bits C51Learner.act gives on the same input
// vectors, for a view of a learner's network (online or target) as for a network packed from plain tensors by the learner's own path.
//
// gfx950 mapping: k_c51_act's -- one workgroup of AT_THREADS per AT_TM = 16 states, 32 lanes per row, X 16 x 32, the hidden activations and the
// A K logits in LDS (DdpgTile: ddpg_tile_bytes(h1p, Ap), no m tile), both layers v_mfma_f32_16x16x4_f32 loops.
//
// The kernel takes the C51Dev by value and reads dq.base.q, the shape (dq.base.n_obs, h1p, dq.A, dq.Ap), K, dueling, v_min and dz, and nothing else: no
// counter, no ticket, no workspace.  An evaluation in the middle of a training leaves the run's bits alone.
//
// The arithmetic is one __device__ body, c51actor_eval_body, with two entries: k_c51actor_eval (a lone actor on N rows) and k_c51actor_eval_pop of
// stmpc_c51actor_pop_kernels.hpp (P actors, each on its own slice of one batch).
#pragma once
#include "stmpc_c51_kernels.hpp"
#include "stmpc_qactor_kernels.hpp"

namespace stmpc {

// The evaluation of rows [row0 + 16 blockIdx.x, + 16) with the network and the support of D, as far as row0 + n_rows: qactor_eval_body's contract
// (stmpc_qactor_kernels.hpp) -- row0 = 0 and n_rows = N for a lone actor, a member of a population has its slice's first row and length here, and the
// state arrays, live and the outputs of o are indexed by the global row.  D: the learner's struct (a view) or one with dq.base.q, dq.base.n_obs,
// dq.base.h1p, dq.A, dq.Ap, K, dueling, v_min, v_max and dz alone (a created actor, a population's member).
// o.q: float32 [rows][A], the expected values (what k_c51_act writes to dbg_q); rows at or beyond row0 + n_rows are never written.  live: see
// qactor_eval_body
__device__ __forceinline__ void c51actor_eval_body(const FeatCfg &f, const C51Dev &D, int target, int row0, int n_rows, int Kmax, const double *__restrict__ ego4,
                                                   const int *__restrict__ k_count, const double *__restrict__ ox, const double *__restrict__ ov,
                                                   const double *__restrict__ oa, const int *__restrict__ live, const QActorOut &o, unsigned char *qa_smem) {
    const DdpgDev &L = D.dq.base;
    const DdpgTile T = ddpg_tile(qa_smem, L.h1p, D.dq.Ap);
    const int tid = threadIdx.x, l0 = blockIdx.x * AT_TM, row = tid >> 5, part = tid & 31, l = l0 + row, e = row0 + l;
    for (int x = tid; x < AT_TM * AT_KIN; x += blockDim.x) T.X[x] = 0.f;       // pad columns and the rows beyond n_rows
    __syncthreads();
    if (tid < AT_TM && l0 + tid < n_rows) dev_policy_features(f, row0 + l0 + tid, Kmax, ego4, k_count, ox, ov, oa, live, nullptr, T.X + tid * AT_KIN);
    __syncthreads();
    if (o.feat && l < n_rows && part < L.n_obs) o.feat[(size_t)e * o.feat_stride + part] = T.X[row * AT_KIN + part];
    dqn_q(D.dq, T, T.X, target != 0);
    if (D.dueling) c51_dueling_combine(D, T.H2 + (size_t)row * T.h2_ld);    // (a dueling head: the advantage blocks become the actions' logits)
    float best;
    const int a = c51_greedy(D, T.H2 + (size_t)row * T.h2_ld, best, o.q && l < n_rows ? o.q + (size_t)e * D.dq.A : nullptr);      // (every lane runs its shuffles)
    if (l >= n_rows || part != 0) return;
    o.jerk[e] = qactor_jerk(o, a, ego4, e);
    if (o.action) o.action[e] = a;
}

__global__ void __launch_bounds__(AT_THREADS) k_c51actor_eval(FeatCfg f, C51Dev D, int target, int N, int Kmax, const double *__restrict__ ego4,
                                                              const int *__restrict__ k_count, const double *__restrict__ ox, const double *__restrict__ ov,
                                                              const double *__restrict__ oa, const int *__restrict__ live, QActorOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qa_smem[];
    c51actor_eval_body(f, D, target, 0, N, Kmax, ego4, k_count, ox, ov, oa, live, o, qa_smem);
}

}  // namespace stmpc
