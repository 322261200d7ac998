// stmpc_fs_kernels.hpp -- device side of the first-step shield controller (reference st.do_conditional_st_based_on_first_step,
// st.py:805-814), batched: one thread per state.  The proposed speed is the caller's (a policy's jerk through
// control.get_ego_speed_from_jerk, or anything else); these kernels do what the reference does with it -- ONE step of the traffic
// predictor (predict_step_with_ego with its default min_crash_distance, prediction.py:46), laid out as the state the feasibility probe
// takes, the list of the states the probe or the step itself rejects, and the choice between the proposed speed and st.do_st_control's.
// The probe and the controller are the existing batched solves; nothing here touches them.
#pragma once
#include "stmpc_cc_kernels.hpp"

namespace stmpc {

enum { FS_PROPOSED = 0, FS_CRASHED = 1, FS_GUARANTEED = 2 };

// st.py:806: next_state, crashed = state.predict_step_with_ego(start_speed, delta_t = TICK_LENGTH), written as the 5-column state the
// solver takes (start_s of the predicted position from the device map of control.get_ego_s) with the rest of each vehicle row zero.
// min_crash_distance is this controller's own (the predictor's default, 5), not COMBINATION_MIN_DISTANCE as in k_rollout_step.  The
// predictor does not read the other vehicles' accelerations (prediction.py:75-97), so none come in -- as in k_rollout_step, where they
// only go out to the policy's next evaluation, which this controller does not have.
template <int KMAX>
__global__ void __launch_bounds__(64) k_fs_step(DevP p, double tick, double min_crash_distance, int N, int Kmax, const double *__restrict__ ego5,
                                                const int *__restrict__ k_count, const double *__restrict__ ox, const double *__restrict__ ov,
                                                const double *__restrict__ start_speed, int *__restrict__ crashed, double *__restrict__ next_ego5,
                                                double *__restrict__ next_ox, double *__restrict__ next_ov) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    DState<KMAX> s;
    s.ex = ego5[(size_t)e * 5 + 0]; s.ey = ego5[(size_t)e * 5 + 1]; s.ev = ego5[(size_t)e * 5 + 2]; s.ea = ego5[(size_t)e * 5 + 3];
    int k = k_count[e];
    k = k < 0 ? 0 : (k > KMAX ? KMAX : k);
    k = k > Kmax ? Kmax : k;
    s.k = k;
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
        const bool in = i < k;
        s.xs[i] = in ? ox[(size_t)e * Kmax + i] : 0.0;
        s.vs[i] = in ? ov[(size_t)e * Kmax + i] : 0.0;
    }
    const bool cr = dev_predict_with_ego<KMAX>(p, s, start_speed[e], tick, min_crash_distance);
    crashed[e] = cr ? 1 : 0;
    next_ego5[(size_t)e * 5 + 0] = s.ex; next_ego5[(size_t)e * 5 + 1] = s.ey; next_ego5[(size_t)e * 5 + 2] = s.ev; next_ego5[(size_t)e * 5 + 3] = s.ea;
    next_ego5[(size_t)e * 5 + 4] = dev_ego_s(s.ex, s.ey);
#pragma unroll
    for (int i = 0; i < KMAX; ++i)
        if (i < Kmax) { next_ox[(size_t)e * Kmax + i] = i < k ? s.xs[i] : 0.0; next_ov[(size_t)e * Kmax + i] = i < k ? s.vs[i] : 0.0; }
}

// Ordered list of the states that st.py:808 hands to st.do_st_control: crashed | guaranteed.  k_cc_select's body, unchanged: its test
// (cc_needs_control) reads exactly these two words when the crash check and the probe are on and the speed limit is off.
__global__ void __launch_bounds__(1024) k_fs_select(int N, const int *__restrict__ crashed, const int *__restrict__ guaranteed, int *sel_idx, int *sel_count) {
    CCfg c{};
    c.check_rollout_crash = 1; c.test_rollout_state = 1;                        // (limit_speed = 0: sel_speed is never read)
    CCState st{};
    st.crash_pred = const_cast<int *>(crashed);
    cc_select_body([&](int) -> const CCfg & { return c; }, N, st, guaranteed, sel_idx, sel_count);
}

// st.py:808-814.  st_speed / fine_len: st.do_st_control's command for the START state (of every state, or scattered to the selected ones).
// Where both tests fail the reason is the step's crash: the reference's `crashed or crash_guaranteed`.  takeovers: the context's running total.
__global__ void __launch_bounds__(64) k_fs_decide(int N, const double *__restrict__ start_speed, const int *__restrict__ crashed, const int *__restrict__ guaranteed,
                                                  const double *__restrict__ st_speed, const int *__restrict__ fine_len, double *cmd_speed, int *takeover,
                                                  int *reason_out, unsigned long long *takeovers, unsigned *err) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    bool take = false;
    if (e < N) {
        const int reason = crashed[e] ? FS_CRASHED : (guaranteed[e] ? FS_GUARANTEED : FS_PROPOSED);
        take = reason != FS_PROPOSED;
        double speed = start_speed[e];
        if (take) {
            speed = st_speed[e];                                                // st.do_st_control(state)
            if (fine_len[e] < 0) atomicOr(err, 1u);                             // ... which could not re-sample its path: the command is not the reference's
        }
        cmd_speed[e] = speed;
        takeover[e] = take ? 1 : 0;
        reason_out[e] = reason;
    }
    const unsigned long long b = __ballot(take);                                // (one wavefront per workgroup)
    if (threadIdx.x == 0 && b) atomicAdd(takeovers, (unsigned long long)__popcll(b));
}

// control.get_ego_speed_from_jerk (control.py:160-171) for N states: dev_speed_from_jerk as k_rollout_step applies it, on its own
__global__ void __launch_bounds__(64) k_fs_speed_from_jerk(CCfg c, int N, const double *__restrict__ ego5, const double *__restrict__ jerk, double *speed) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    speed[e] = dev_speed_from_jerk(c, ego5[(size_t)e * 5 + 2], ego5[(size_t)e * 5 + 3], jerk[e]);
}

}  // namespace stmpc
