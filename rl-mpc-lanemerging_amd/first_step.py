"""First-step shield controller: the reference's ``st.do_conditional_st_based_on_first_step(state, start_speed)`` (st.py:805-814), batched.

Its third way -- next to ``st.do_st_control`` and ``dqn.RLAgent.do_combined_control`` -- to put the solver behind a proposed command, and the
cheapest: ONE step of the traffic predictor with the proposed speed (``predict_step_with_ego`` with its default ``min_crash_distance``,
prediction.py:46), ``st.test_guaranteed_crash_from_state`` on the predicted state, and ``st.do_st_control(state)`` only where the step crashed
or no feasible path exists afterwards; otherwise the proposed speed is commanded as it is.  All of it runs on the GPU
(``stmpc_first_step_device``, csrc/stmpc_fs_kernels.hpp + the existing batched solves); the proposal is the caller's -- in
``episodes.EpisodeRunner(controller="first_step")`` a policy's jerk through ``control.get_ego_speed_from_jerk`` (``speed_from_jerk_device``).
"""
import numpy as np

from . import _capi
from . import control
from .combined import get_ego_speed_from_jerk      # noqa: F401  (the host twin of stmpc_speed_from_jerk_device, control.py:160-171)
from .config import Settings
from .prediction import pack_states

FirstStepCfg = _capi.FirstStepCfg

REASON_PROPOSED, REASON_CRASHED, REASON_GUARANTEED = 0, 1, 2
REASON_NAMES = {REASON_PROPOSED: "proposed speed", REASON_CRASHED: "first step crashes", REASON_GUARANTEED: "no feasible path after the first step"}


def speed_from_jerk_device(ctx, params, tick_length, d_ego5, d_jerk, d_speed=None, stream=0):
    """``control.get_ego_speed_from_jerk`` (control.py:160-171) of every state's speed and acceleration (``d_ego5[:, 2:4]``) with ``d_jerk``, on the
    device; returns ``d_speed`` (fp64 [N], allocated if not given)."""
    import torch
    n = d_ego5.shape[0]
    if d_speed is None:
        d_speed = torch.empty(n, dtype=torch.float64, device=d_ego5.device)
    ctx.speed_from_jerk_device(params, tick_length, n, d_ego5.data_ptr(), d_jerk.data_ptr(), d_speed.data_ptr(), stream)
    return d_speed


class FirstStepController:
    """The device-pointer path: ``decide(d_ego5, d_k, d_ox, d_ov, d_start_speed)`` for N states held in torch tensors (fp64 / int32); nothing
    leaves the GPU (with ``sparse_control`` one integer does: the number of taken-over states).  The output tensors are the controller's own and
    are overwritten by the next call."""

    def __init__(self, n, ctx=None, params=None, cfg=None, sparse_control=False):
        import torch
        self.ctx = ctx or _capi.default_context()
        self.params = params if params is not None else _capi.Params.from_settings(Settings)
        self.cfg = cfg if cfg is not None else FirstStepCfg.from_settings(Settings, sparse_control=sparse_control)
        self.n = int(n)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.cmd_speed = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.takeover = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.reason = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.start_speed = torch.empty(self.n, dtype=torch.float64, device=dev)

    def decide(self, d_ego5, d_k, d_ox, d_ov, d_start_speed, d_oa=None, stream=0):
        """Returns ``{"speed": the command, "takeover", "reason" (REASON_*)}`` (device tensors)."""
        n, K = d_ego5.shape[0], d_ox.shape[1]
        if n != self.n or d_start_speed.shape[0] != n:
            raise ValueError("%d states and %d proposed speeds, this controller was built for %d" % (n, d_start_speed.shape[0], self.n))
        self.ctx.first_step_device(self.params, self.cfg, n, K, d_ego5.data_ptr(), d_k.data_ptr(), d_ox.data_ptr(), d_ov.data_ptr(),
                                   d_oa.data_ptr() if d_oa is not None else 0, d_start_speed.data_ptr(), self.cmd_speed.data_ptr(), self.takeover.data_ptr(),
                                   self.reason.data_ptr(), stream)
        return {"speed": self.cmd_speed, "takeover": self.takeover, "reason": self.reason}

    def decide_jerk(self, d_ego5, d_k, d_ox, d_ov, d_jerk, d_oa=None, stream=0):
        """``decide`` with the proposal given as a jerk (a policy's action): ``control.get_ego_speed_from_jerk`` first (control.py:174-178 is how
        the reference turns a policy's jerk into the speed it commands)."""
        speed_from_jerk_device(self.ctx, self.params, self.cfg.tick_length, d_ego5, d_jerk, self.start_speed, stream)
        return self.decide(d_ego5, d_k, d_ox, d_ov, self.start_speed, d_oa, stream)

    def counts(self, reset=False):
        """(states decided, taken over, controller solves) on this controller's context since the last reset."""
        return self.ctx.first_step_counts(reset)


def decide_batch(states, start_speeds, ctx=None, sparse_control=False):
    """``do_conditional_st_based_on_first_step`` for a list of ``HighwayState`` and one proposed speed each (host arrays in, host arrays out:
    ``stmpc_first_step``).  Returns a dict: ``speed[n]`` (the command), ``takeover[n]`` (bool), ``reason[n]`` (REASON_*), ``crashed[n]``,
    ``crash_guaranteed[n]`` (the probe's verdict for every state, as the reference evaluates it before it looks at ``crashed``) and the predicted
    state as arrays ``next_ego[n,5]``, ``next_other_x``, ``next_other_v``."""
    ctx = ctx or _capi.default_context()
    params = _capi.Params.from_settings(Settings)
    cfg = FirstStepCfg.from_settings(Settings, sparse_control=sparse_control)
    ego5, k, ox, ov = pack_states(states)
    d = ctx.first_step(params, cfg, ego5, k, ox, ov, np.asarray(start_speeds, dtype=np.float64))
    return {"speed": d["cmd_speed"], "takeover": d["takeover"] != 0, "reason": d["reason"], "crashed": d["crashed"] != 0,
            "crash_guaranteed": d["crash_guaranteed"] != 0, "next_ego": d["next_ego"], "next_other_x": d["next_other_x"], "next_other_v": d["next_other_v"]}


def do_conditional_st_based_on_first_step(state, start_speed):
    """The reference's call shape for one state (st.py:805-814): commands the speed through ``control.set_ego_speed`` and returns it."""
    d = decide_batch([state], [start_speed])
    if d["takeover"][0]:
        print("ST solver taking over")
    speed = float(d["speed"][0])
    control.set_ego_speed(speed)
    return speed
