// stmpc_cc_groups_kernels.hpp -- controller groups: one batch of the combined controller split into C groups of n_per_group consecutive rows, each with
// its own CCfg, in the launches of a lone batch.  The reference varies its evaluation along exactly this axis: main.do_grid_search_combined
// (main.py:62-81) sweeps ROLLOUT_LENGTH x ST_TEST_ROLLOUTS x TEST_ROLLOUT_STATE and its combined_*b configs flip CHECK_ROLLOUT_CRASH, LIMIT_DQN_SPEED,
// TEST_ST_STRICTLY_BETTER and REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED, one EVALUATE_COMBINED_DDPG process per cell.
//
// Every entry is the body of its single-cfg kernel (rollout_step_body / cc_decide_body / cc_select_body of stmpc_cc_kernels.hpp -- not a copy) on the cfg
// blockIdx.y selects from a device table of CCfg.  blockIdx.y is wave-uniform and the table is read before the workgroup's first store, so the struct
// comes in through scalar loads like the by-value argument it replaces.  Workgroup (x, g) serves local rows [64 x, 64 x + 64) of group g: a workgroup
// never spans two groups and a group's tail lanes are masked as a lone batch of n_per_group rows masks them.  The body sees the group's slice of every
// [N]... array, so its row index is the LOCAL row.  rollout_s has ONE row stride for all groups, Rmax + 1 of the longest group; a group's history still
// ends at its own rollout_length + 1.  The host runs Rmax steps: a step past a group's rollout_length leaves that group's rows untouched.
//
// ask [N] (beside the CCState): the rows the policy is to be asked for at the NEXT step -- live, and the group has a next step.  A lone batch of R steps
// asks its policy at steps 1 .. R; without this mask a row of a short group that is still live after its last step would be asked again at step R + 1 and
// carry one evaluation too many in its time feature from then on.  `live` keeps its meaning.
#pragma once
#include "stmpc_cc_kernels.hpp"

namespace stmpc {

template <int KMAX>
__global__ void __launch_bounds__(64) k_rollout_step_groups(DevP p, const CCfg *__restrict__ groups, int n_per_group, int Kmax, int step, int rs,
                                                            const double *__restrict__ ego5_start, double *ego4, const int *__restrict__ k_count, double *ox,
                                                            double *ov, double *oa, const double *__restrict__ action, CCState st, int *ask) {
    const CCfg c = groups[blockIdx.y];
    const size_t off = (size_t)blockIdx.y * n_per_group;
    const CCState gs = cc_state_slice(st, off, rs, Kmax);
    rollout_step_body<KMAX>(p, c, n_per_group, Kmax, step, rs, ego5_start + off * 5, ego4 + off * 4, k_count + off, ox + off * Kmax, ov + off * Kmax,
                            oa ? oa + off * Kmax : nullptr, action + off, gs);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_per_group && step <= c.rollout_length) ask[off + e] = (gs.live[e] && step < c.rollout_length) ? 1 : 0;      // (live[e]: this thread's own store)
}

__global__ void __launch_bounds__(64) k_cc_decide_groups(const CCfg *__restrict__ groups, int n_per_group, int rs, const double *__restrict__ ego5_start,
                                                         const double *__restrict__ first_action, const int *__restrict__ last_choice_rl, CCState st,
                                                         const int *__restrict__ probe_crash, const double *__restrict__ st_speed, const double *__restrict__ fine,
                                                         const int *__restrict__ fine_len, int fine_stride, int *takeover, int *reason_out, double *speed_out,
                                                         unsigned *err) {
    const CCfg c = groups[blockIdx.y];
    const size_t off = (size_t)blockIdx.y * n_per_group;
    cc_decide_body(c, n_per_group, rs, ego5_start + off * 5, first_action + off, last_choice_rl ? last_choice_rl + off : nullptr, cc_state_slice(st, off, rs, 0),
                   probe_crash + off, st_speed + off, fine + off * fine_stride, fine_len + off, fine_stride, takeover + off, reason_out + off, speed_out + off, err);
}

// One workgroup over all N = C * n_per_group rows (global row indices, nothing sliced): row e asks with its own group's flags.
__global__ void __launch_bounds__(1024) k_cc_select_groups(const CCfg *__restrict__ groups, int n_per_group, int N, CCState st, const int *__restrict__ probe_crash,
                                                           int *sel_idx, int *sel_count) {
    cc_select_body([&](int e) -> const CCfg & { return groups[e / n_per_group]; }, N, st, probe_crash, sel_idx, sel_count);
}

// flag[idx[j]] = c_flag[j]: the feasibility probe's verdicts of the compact batch of testing rows, back to their rows
__global__ void __launch_bounds__(64) k_cc_scatter_flag(int M, const int *__restrict__ idx, const int *__restrict__ c_flag, int *flag) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    flag[idx[j]] = c_flag[j];
}

}  // namespace stmpc
