// stmpc_solver_groups_kernels.hpp -- solver groups: one batch of G groups of n_per_group consecutive states, each group solved under its own parameter
// set, in the launches of one batch.  The reference tunes the ST solver along exactly this axis: main.do_grid_search_st (main.py:43-59) runs TASK "ST"
// over the product of V_WEIGHT, A_WEIGHT, J_WEIGHT, D_WEIGHT, MIN_ALLOWED_DISTANCE and CRASH_MIN_S, one process per cell.
//
// The solve kernels here are not copies: stmpc_kernels.hpp is compiled a second time, in namespace stmpc::grouped, with the STMPC_G_* macros selecting an
// episode's parameters from a device table of GroupP, row episode / n_per_group, by plain loads -- grouped::k_predict<KMAX> (one more argument, the
// table) and grouped::k_solve<...> (argument SolveArgsG).  The production kernels are compiled from the same tokens as before: in the first pass the macros
// expand to the kernel argument's own fields.  The episode index is the state's index in the batch wherever the solver reads one: the work counter, the
// overflow queues, the second window's side launch and the checkpoint pool all carry episode ids, never queue positions.
// The groups may differ only in d_w, v_w, a_w, j_w, min_allowed and obst_min_s (= crash_min_s - min_allowed) and in what the host derives from them
// (GroupP::band, ::band2_mult, the guide table); everything a launch decides on the host (tiers, fan-out, fast division, back-pointer width) depends on
// the other fields, which the host has checked to be equal.  k_predict serves 32 / KMAX episodes per wavefront, so a group boundary may fall inside one:
// its table rows are looked up per episode.  The grouped world step is sim_step_body of stmpc_cc_kernels.hpp on the traffic group's own crash_min_s.
#pragma once
#include "stmpc_kernels.hpp"
#include "stmpc_sim_groups_kernels.hpp"

#define STMPC_KERNELS_GROUPED_PASS
#undef STMPC_G_ARGS
#undef STMPC_G_P
#undef STMPC_G_BAND
#undef STMPC_G_BAND2
#undef STMPC_G_PRED_ARG
#undef STMPC_G_PRED_GUIDE
#undef STMPC_G_PRED_OBST_MIN_S
#undef STMPC_G_PRED_MIN_ALLOWED
#define STMPC_G_ARGS SolveArgsG
#define STMPC_G_P(a, e) group_of(a, e).p
#define STMPC_G_BAND(a, e) group_of(a, e).band
#define STMPC_G_BAND2(a, e) group_of(a, e).band2_mult
#define STMPC_G_PRED_ARG GroupTab gsel,
#define STMPC_G_PRED_GUIDE(e) (guide_tab + gsel.groups[(e) / gsel.n_per_group].guide_off)
#define STMPC_G_PRED_OBST_MIN_S(e) gsel.groups[(e) / gsel.n_per_group].p.obst_min_s
#define STMPC_G_PRED_MIN_ALLOWED(e) gsel.groups[(e) / gsel.n_per_group].p.min_allowed
namespace stmpc {
namespace grouped {
#include "stmpc_kernels.hpp"
}  // namespace grouped
}  // namespace stmpc
#undef STMPC_KERNELS_GROUPED_PASS

namespace stmpc {

namespace sim {

#ifdef STMPC_UNIT_ENV        // (the kernels of the unit that launches them)
// k_sim_step_groups with the closest-distance gate (es > crash_min_s) of the traffic group's own solver group: crash_min_s[blockIdx.y]
__global__ void __launch_bounds__(64) k_sim_step_solver_groups(DevP p, const Cfg *__restrict__ groups, int n_per_group, State s, const double *__restrict__ cmd_speed,
                                                               const double *__restrict__ crash_min_s) {
    const Cfg c = groups[blockIdx.y];
    const size_t off = (size_t)blockIdx.y * n_per_group;
    sim_step_body(p, c, n_per_group, state_slice(s, off), cmd_speed + off, crash_min_s[blockIdx.y]);
}
#endif

}  // namespace sim
}  // namespace stmpc
