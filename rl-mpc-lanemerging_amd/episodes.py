"""Batched SUMO-free merge episodes: the role of the reference's ``control.run_episode`` /
``control.evaluate_control`` (control.py:207-395) and of the per-episode columns of ``stats.StatsAggregator``
(stats.py:43-111), for N environments stepped in lock-step on one GPU.

The world restates the SUMO scenario the reference configures (Krauss vehicles of the "simple traffic distribution", the ego under
speed mode 22; see ``stmpc_sim_*`` in include/stmpc.h) but is not SUMO: results are comparable with the reference's reported numbers
(experiment_data/saved_data.csv) as DISTRIBUTIONS only.  Every tick is: planner view ->
controller (``st.do_st_control`` for all environments in one launch, the combined controller, or the first-step shield controller of
``first_step.py``) -> world step; nothing but a periodic "all finished?" flag crosses to the host.
"""
import os

import numpy as np

from . import _capi, groups, scenario, synth
from .config import Settings

# scenario constants of the reference's SUMO network and episode runner
SPAWN_X, DESPAWN_X = -250.0, 100.0          # highwayrear starts at x = -250, highwayahead ends at x = 100 (merge.net.xml:45-49)
EGO_START_ARC = 40.0                        # departPos = 40 on the ramp (control.py:42)
ARRIVE_X = 1.5 + 50.0                       # arrivalPos = 50 on highwayahead (control.py:42)
RAMP_START = (-250.47, 28.47)               # first point of lane ramp_0 (merge.net.xml:52)


def ego_start_position(route="lane"):
    """Point 40 m along the ramp from its start: on the lane's centre line (``route="lane"``, what SUMO does) or on the straight line from the
    ramp's start to the junction entry (``route=None``: the world of rounds 3-4, whose ego moves as the predictor assumes)."""
    if route == "lane":
        return scenario.point_at_arc(EGO_START_ARC)
    x0, y0 = RAMP_START
    d = np.hypot(-50.58 - x0, 1.71 - y0)
    ux, uy = (-50.58 - x0) / d, (1.71 - y0) / d
    return x0 + EGO_START_ARC * ux, y0 + EGO_START_ARC * uy


# The traffic types of the reference's experiment matrix (configs/{st,train,combined,cross,ddpg}_*.json differ in these two fields; "heavy" and
# "slow" are what the cross configs call the default traffic next to a medium / moderate network).
TRAFFIC_TYPES = {
    "low": {"BASE_TRAFFIC_INTERVAL": 2.4, "OTHER_CAR_SPEED": 7.0},
    "medium": {"BASE_TRAFFIC_INTERVAL": 1.8, "OTHER_CAR_SPEED": 7.0},
    "default": {"BASE_TRAFFIC_INTERVAL": 1.2, "OTHER_CAR_SPEED": 7.0},
    "moderate": {"BASE_TRAFFIC_INTERVAL": 1.2, "OTHER_CAR_SPEED": 11.0},
    "fast": {"BASE_TRAFFIC_INTERVAL": 1.2, "OTHER_CAR_SPEED": 15.0},
    "heavy": {"BASE_TRAFFIC_INTERVAL": 1.2, "OTHER_CAR_SPEED": 7.0},
    "slow": {"BASE_TRAFFIC_INTERVAL": 1.2, "OTHER_CAR_SPEED": 7.0},
}
_TRAFFIC_KEYS = ("BASE_TRAFFIC_INTERVAL", "OTHER_CAR_SPEED", "VARY_TRAFFIC_START_TIMES", "seed")


def sim_cfg(seed=0, max_episode_length=100.0, route="lane", overrides=None):
    """``route``: "lane" (default) = the ego follows the centre line of its lanes in the reference's network (``scenario.py``; TraCI reports those
    positions), None = the straight lines the planner assumes (prediction.py:46-59; the world of rounds 3-4, kept for the mechanics test).
    ``overrides``: a dict of setting names that take precedence over ``Settings`` for this cfg (``sim_cfgs``: a traffic group's own values)."""
    S = Settings
    ex, ey = ego_start_position(route)
    ov = overrides or {}
    g = lambda name, default: ov[name] if name in ov else getattr(S, name, default)
    return _capi.SimCfg(tick_length=S.TICK_LENGTH, other_car_speed=g("OTHER_CAR_SPEED", 7.0), base_traffic_interval=g("BASE_TRAFFIC_INTERVAL", 1.2),
                        spawn_x=SPAWN_X, despawn_x=DESPAWN_X, ego_start_x=ex, ego_start_y=ey, arrive_x=ARRIVE_X, sensor_radius=g("SENSOR_RADIUS", 125.0),
                        start_speed=g("START_SPEED", 15.0), start_speed_std=g("START_SPEED_VARIANCE", 5.0), min_start_speed=g("MIN_START_SPEED", 5.0),
                        max_start_speed=g("MAX_START_SPEED", 25.0),
                        # SUMO vType "normal" of the simple traffic distribution (merge_impossible.rou.xml:3) + SUMO defaults (emergencyDecel, width)
                        veh_accel=4.5, veh_decel=6.0, veh_min_gap=1.0, veh_tau=0.5, veh_emergency_decel=9.0, veh_length=g("CAR_LENGTH", 5.0), veh_width=1.8, speed_dev=0.0,
                        vary_traffic_start_times=int(bool(g("VARY_TRAFFIC_START_TIMES", True))),
                        randomize_start_speed=int(bool(g("RANDOMIZE_START_SPEED", True))), max_ticks=int(max_episode_length / S.TICK_LENGTH),
                        yield_overlap=2,          # (the one junction rule, include/stmpc.h)
                        seed=int(seed), disruption_min_s=float(g("MERGE_POINT_X", -50.0))).set_route(np.stack(scenario.lane_polyline()[:2], axis=1) if route == "lane" else None)


def traffic_settings(entry):
    """One traffic group as a dict of settings: ``entry`` is a name of ``TRAFFIC_TYPES`` or a dict with BASE_TRAFFIC_INTERVAL and OTHER_CAR_SPEED
    (and optionally VARY_TRAFFIC_START_TIMES and a ``seed``); ValueError for anything else."""
    if isinstance(entry, str):
        if entry not in TRAFFIC_TYPES:
            raise ValueError("unknown traffic type %r (one of %s)" % (entry, ", ".join(TRAFFIC_TYPES)))
        return dict(TRAFFIC_TYPES[entry])
    if not isinstance(entry, dict) or "BASE_TRAFFIC_INTERVAL" not in entry or "OTHER_CAR_SPEED" not in entry:
        raise ValueError("a traffic group is a name of TRAFFIC_TYPES or a dict with BASE_TRAFFIC_INTERVAL and OTHER_CAR_SPEED, not %r" % (entry,))
    unknown = [k for k in entry if k not in _TRAFFIC_KEYS]
    if unknown:
        raise ValueError("a traffic group may set %s, not %s" % (", ".join(_TRAFFIC_KEYS), ", ".join(map(str, unknown))))
    return dict(entry)


def sim_cfgs(traffic, seed=0, max_episode_length=100.0, route="lane"):
    """One ``SimCfg`` per traffic group (a ``_capi.SimCfgTable`` for ``stmpc_sim_init_groups_device``): ``traffic`` is a list of names of
    ``TRAFFIC_TYPES`` or of dicts (``traffic_settings``).  Every cfg comes from ``sim_cfg``'s code path with the group's values in place of the
    global ``Settings``', which are read for everything else and never written.

    Seeds: group g's is its own ``seed`` entry if it has one, else ``vec_env.episode_seed(seed, g)`` -- ``seed`` itself for group 0 (a one-group
    world is the plain world of that seed), splitmix64 of ``seed + g * 0x9E3779B97F4A7C15`` for the others, so groups are different draws.  Give two
    groups the same ``seed`` entry for common random numbers."""
    from . import vec_env
    groups = [traffic_settings(t) for t in traffic]
    if not groups:
        raise ValueError("traffic must name at least one group")
    cfgs = []
    for gi, t in enumerate(groups):
        gseed = int(t.pop("seed")) if "seed" in t else vec_env.episode_seed(seed, gi)
        cfgs.append(sim_cfg(gseed, max_episode_length, route, overrides=t))
    return _capi.SimCfgTable(cfgs)


def traffic_mix_cfgs(traffic_mix, seed=0, max_episode_length=100.0, route="lane"):
    """One ``SimCfg`` per traffic type of a traffic mix (a ``_capi.SimCfgTable`` for ``stmpc_traffic_mix_env_reset_device``): ``traffic_mix`` is a list
    of what ``traffic_settings`` takes.  Every cfg comes from ``sim_cfg``'s code path under the one ``seed`` -- a mixed world is one world, so an entry
    that sets its own ``seed`` is a ValueError, as is an empty list and one of more than ``TRAFFIC_MIX_MAX`` types.  Touches no device."""
    types = [traffic_settings(t) for t in traffic_mix]
    groups.within(len(types), _capi.TRAFFIC_MIX_MAX, "traffic_mix", "traffic types")
    for ti, t in enumerate(types):
        if "seed" in t:
            raise ValueError("a traffic mix has one seed (the env's): type %d must not set its own" % ti)
    return _capi.SimCfgTable([sim_cfg(seed, max_episode_length, route, overrides=t) for t in types])


def _check_traffic(n, traffic, policy, g_max=None):
    """(G, n_per_group) for ``n`` environments in the groups of ``traffic``; ValueError when they do not split or do not coincide with the
    members of a population ``policy``.  ``g_max``: the most groups the world takes (default ``SIM_GROUPS_MAX``; a solver-groups run:
    ``SOLVER_GROUPS_MAX``).  Touches no device."""
    G, npg = groups.split(n, len(traffic), _capi.SIM_GROUPS_MAX if g_max is None else g_max, "traffic")
    groups.coincide("traffic", G, npg, policy=policy)
    return G, npg


def _check_control(n, control, traffic, policy):
    """(C, n_per_cell) for ``n`` environments in the controller groups of ``control``; ValueError when they do not split or do not coincide with
    the traffic groups or the members of a population ``policy`` (cell c pairs member c, traffic c and control c).  Touches no device."""
    from . import combined
    C, npc = groups.split(n, len(control), combined.CONTROL_GROUPS_MAX, "control", "controller")
    groups.coincide("control", C, npc, traffic, policy)
    return C, npc


def _check_solver(n, solver, traffic, controller):
    """(G, n_per_cell) for ``n`` environments in the solver groups of ``solver``; ValueError when the controller is not "st", when they do not split,
    or when they do not coincide with the traffic groups (cell c pairs traffic c with solver c).  Touches no device."""
    if controller != "st":
        raise ValueError("solver groups are settings of the ST controller, not of %r" % (controller,))
    G, npg = groups.split(n, len(solver), _capi.SOLVER_GROUPS_MAX, "solver")
    groups.coincide("solver", G, npg, traffic)
    return G, npg


class EpisodeRunner:
    """N merge episodes stepped in lock-step on the device, one ``tick()`` at a time (``run_episodes`` drives it to the end;
    ``bench.py --workload episodes`` times its ticks).

    ``record``: None (the tick is the plain sequence view -> controller -> step) or a ``report.RecorderConfig``: every tick then also feeds the
    on-device flight recorder (``stmpc_rec_*``) between the controller and the step, and ``result()`` gains ``out["report"]`` (``report.Report``:
    the reference's report row with standard errors, the position profiles, the recorded run-up of every environment).  The recorder follows
    ONE episode per environment -- this runner's -- and is bound to the world this constructor initialises; ``vec_env.MergeVecEnv``'s autoreset
    is not recorded.

    ``policy`` may be an ``actor.ActorPopulation`` (anything with a ``P`` attribute): member m then drives environments
    [m * n_per_member, (m + 1) * n_per_member), ``n`` must be ``policy.n``, and ``result()`` gains ``out["member"]`` (see ``summary_by_member``,
    ``report.Report.by_member``).  The members' environments are different draws of one world, not common random numbers.

    ``traffic``: None (one world from the global ``Settings``) or a list as ``sim_cfgs`` takes: the world then has ``G = len(traffic)`` traffic
    groups of ``n / G`` consecutive environments (``stmpc_sim_init_groups_device``), group g bit-identical to a lone runner of ``n / G``
    environments with that traffic and group g's seed, and ``result()`` gains ``out["traffic_group"]``.  With a population policy too, its P
    must be G and its ``n_per_member`` the group size: cell c pairs member c with traffic c (``cross_matrix`` builds a models x traffic grid).

    ``control`` (combined controller only): None (one ``CombinedCfg`` from the global ``Settings``) or a list of dicts as ``combined.control_cfgs``
    takes: the environments are then ``C = len(control)`` controller groups of ``n / C`` consecutive environments, group c decided under its own
    settings (``stmpc_combined_groups_set``) and bit-identical to a lone runner of ``n / C`` environments with ``control=[control[c]]``, and
    ``result()`` gains ``out["control_group"]``.  With ``traffic`` and / or a population policy too, cell c pairs member c, traffic c and
    control c: the counts and slice sizes must coincide.  Give the traffic groups one ``seed`` for common random numbers across the cells
    (``grid_search_combined``).

    ``solver`` (ST controller only): None (one ``Params`` from the global ``Settings``) or a list of dicts as ``st.param_cfgs`` takes: the environments
    are then ``len(solver)`` solver groups of equal size, group g controlled under its own V/A/J/D_WEIGHT, MIN_ALLOWED_DISTANCE and CRASH_MIN_S
    (``stmpc_st_control_groups_device``) and its closest-distance statistics gated by its own CRASH_MIN_S
    (``stmpc_solver_groups_sim_step_device``), bit-identical to a lone runner of that many environments with ``Settings`` set to the cell; ``result()``
    gains ``out["solver_group"]``.  With ``traffic`` too, cell c pairs traffic c with solver c and the counts must coincide; without it every cell
    gets the default traffic under ``vec_env.episode_seed(seed, c)``.  Give the traffic groups one ``seed`` for common random numbers
    (``grid_search_st``).  Up to ``_capi.SOLVER_GROUPS_MAX`` (512) cells fit one runner (``stmpc_solver_groups_sim_init_device``).  The world of
    such a run always has one traffic group per cell, so ``result()`` holds ``out["traffic_group"]`` (equal to ``solver_group``) even when no
    ``traffic`` was given; with ``record``, the report's settings text (``ST_DESCRIPTION``) is the global ``Settings``', not a cell's -- take a
    cell's settings from ``solver[c]``.

    ``controller="first_step"``: ``st.do_conditional_st_based_on_first_step`` (st.py:805-814, ``first_step.py``) behind ``policy`` -- per tick the
    view, ONE policy evaluation, ``control.get_ego_speed_from_jerk`` of its jerk, ``stmpc_first_step_device``, the world step.  ``policy`` (an actor or
    a population) and ``traffic`` work as for "combined"; ``control`` is refused (its keys are settings of the combined controller)."""

    def __init__(self, n, seed=0, controller="st", policy=None, ctx=None, kmax=32, max_episode_length=100.0, record=None, traffic=None, control=None,
                 solver=None):
        import torch
        self.torch = torch
        if controller not in ("st", "combined", "first_step"):
            # (the policy alone -- TASK EVALUATE_DDPG -- is not on the solver's path: SURVEY section 2 marks ddpg.py out of scope; removed in round 6)
            raise ValueError("controller must be 'st', 'combined' or 'first_step', not %r" % (controller,))
        if hasattr(policy, "P") and int(n) != policy.n:
            raise ValueError("n = %d, the population of policies was built for %d x %d = %d environments" % (n, policy.P, policy.n_per_member, policy.n))
        self.traffic = list(traffic) if traffic is not None else None
        self.control = list(control) if control is not None else None
        self.solver = [dict(c) for c in solver] if solver is not None else None
        self.solver_params = None
        if self.solver is not None:
            from . import st
            self.n_solver, self.n_per_solver = _check_solver(n, self.solver, self.traffic, controller)
            self.solver_params = st.param_cfgs(self.solver)
            if self.traffic is None:               # (the grouped step serves a world of traffic groups: one per cell, of the default traffic)
                self.traffic = [{"BASE_TRAFFIC_INTERVAL": getattr(Settings, "BASE_TRAFFIC_INTERVAL", 1.2), "OTHER_CAR_SPEED": getattr(Settings, "OTHER_CAR_SPEED", 7.0)}
                                for _ in self.solver]
        if self.control is not None and controller != "combined":
            raise ValueError("control groups are settings of the combined controller, not of %r" % (controller,))
        if controller == "first_step" and policy is None:
            raise ValueError("the first-step controller shields a policy's proposal: give one (an actor.DDPGActor, an actor.DQNActor or an actor.ActorPopulation)")
        self.C, self.n_per_cell = _check_control(n, self.control, self.traffic, policy) if self.control is not None else (0, 0)
        self.G, self.n_per_group = (_check_traffic(n, self.traffic, policy, _capi.SOLVER_GROUPS_MAX if self.solver is not None else None)
                                    if self.traffic is not None else (0, 0))
        self.n, self.kmax, self.controller, self.policy = int(n), int(kmax), controller, policy
        self.cfgs = sim_cfgs(self.traffic, seed, max_episode_length) if self.traffic is not None else None
        self.ctx = ctx or _capi.default_context()
        self.params = _capi.Params.from_settings(Settings)
        self.cfg = self.cfgs[0] if self.cfgs is not None else sim_cfg(seed, max_episode_length)      # (what the view reads is equal across groups)
        self.max_ticks = max(c.max_ticks for c in self.cfgs) if self.cfgs is not None else self.cfg.max_ticks
        self.tick_length = Settings.TICK_LENGTH
        dev = torch.device("cuda", torch.cuda.current_device())
        H = _capi.num_t(self.params)
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
        self.d_ego5, self.d_k, self.d_ox, self.d_ov, self.d_oa = z(n, 5), z(n, dtype=torch.int32), z(n, kmax), z(n, kmax), z(n, kmax)
        self.d_path, self.d_bt, self.d_cost, self.d_speed = z(n, H, dtype=torch.int32), z(n, dtype=torch.int32), z(n), z(n)
        self.d_fine, self.d_fine_len = z(n, _capi.QP_NMAX), z(n, dtype=torch.int32)
        self.ccfg = _capi.CombinedCfg.from_settings(Settings, sparse_control=True) if controller == "combined" else None      # (a tick ends with a host-side status check anyway)
        if self.control is not None:
            from . import combined
            self.ccfg = combined.ControlGroups(combined.control_cfgs(self.control, sparse_control=True), self.n_per_cell)
        self.fs = None
        if controller == "first_step":
            from . import first_step
            self.fs = first_step.FirstStepController(n, self.ctx, self.params, sparse_control=True)      # (sparse for the reason above)
            self.cur_ego4 = z(n, 4)
        self.takeovers, self.controlled = z(n), z(n)
        self.last_rl = torch.ones(n, dtype=torch.int32, device=dev)
        self.d_status = z(n, dtype=torch.int32)
        self.ticks_done = 0
        if self.solver is not None:
            self.ctx.sim_init_solver_groups(self.cfgs, self.n_per_group)          # (one traffic group per cell: up to SOLVER_GROUPS_MAX of them)
        elif self.cfgs is not None:
            self.ctx.sim_init_groups(self.cfgs, self.n_per_group)
        else:
            self.ctx.sim_init(self.cfg, n)
        self.recorder = None
        if record is not None:
            from . import report
            if not isinstance(record, report.RecorderConfig):
                raise ValueError("record must be None or a report.RecorderConfig (the recorder follows one episode per environment: this runner's), not %r" % (record,))
            self.recorder = report.Recorder(self.ctx, n, kmax, record, self.tick_length)

    def tick(self):
        """Planner view -> controller -> world step for every environment (finished environments idle)."""
        from . import combined
        torch, ctx, n, kmax = self.torch, self.ctx, self.n, self.kmax
        ctx.sim_view(self.cfg, n, kmax, self.d_ego5.data_ptr(), self.d_k.data_ptr(), self.d_ox.data_ptr(), self.d_ov.data_ptr(),
                     self.d_oa.data_ptr() if self.controller != "st" else 0)
        if self.controller == "st":
            if self.solver_params is not None:
                ctx.st_control_groups_device(self.solver_params, self.n_per_solver, self.tick_length, n, kmax, self.d_ego5.data_ptr(), self.d_k.data_ptr(),
                                             self.d_ox.data_ptr(), self.d_ov.data_ptr(), self.d_path.data_ptr(), self.d_bt.data_ptr(), self.d_cost.data_ptr(),
                                             self.d_speed.data_ptr(), self.d_fine.data_ptr(), self.d_fine_len.data_ptr(), 0)
            else:
                ctx.st_control_batch_device(self.params, self.tick_length, n, kmax, self.d_ego5.data_ptr(), self.d_k.data_ptr(), self.d_ox.data_ptr(),
                                            self.d_ov.data_ptr(), self.d_path.data_ptr(), self.d_bt.data_ptr(), self.d_cost.data_ptr(), self.d_speed.data_ptr(),
                                            self.d_fine.data_ptr(), self.d_fine_len.data_ptr(), 0)
            cmd = self.d_speed
        else:
            if self.controller == "first_step":
                self.cur_ego4.copy_(self.d_ego5[:, :4])
                jerk = self.policy(1, self.cur_ego4, self.d_k, self.d_ox, self.d_ov, self.d_oa).to(torch.float64).contiguous()
                d = self.fs.decide_jerk(self.d_ego5, self.d_k, self.d_ox, self.d_ov, jerk, self.d_oa)
            else:
                d = combined.decide_batch_device(ctx, self.params, self.ccfg, self.d_ego5, self.d_k, self.d_ox, self.d_ov, self.policy, self.last_rl, d_oa=self.d_oa)
            cmd = d["speed"]
            # per-episode takeover share (the reference's stats count the ticks of the episode itself): finished environments keep
            # returning their final state from sim_view, their repeated decisions must not be counted
            ctx.sim_status_device(n, self.d_status.data_ptr())
            running = (self.d_status == 0).to(torch.float64)
            self.takeovers += d["takeover"].to(torch.float64) * running
            self.controlled += running
            self.last_rl = (d["takeover"] == 0).to(torch.int32)
        if self.recorder is not None:
            # the state before control, as the reference appends it to state_history (control.py:280-289), with this tick's command
            self.recorder.tick(n, kmax, self.d_ego5, self.d_k, self.d_ox, self.d_ov, self.d_oa, cmd, d["takeover"] if self.controller != "st" else None)
        if self.solver_params is not None:
            ctx.sim_step_solver_groups(self.solver_params, self.n_per_solver, n, cmd.data_ptr())
        elif self.cfgs is not None:
            ctx.sim_step_groups(self.params, n, cmd.data_ptr())
        else:
            ctx.sim_step(self.params, self.cfg, n, cmd.data_ptr())
        self.ticks_done += 1

    def status(self):
        """Host copy of the status words (synchronises) after raising any latched device-side error."""
        status, _, _, _ = self.ctx.sim_read(self.n)
        self.ctx.check_error()          # (an asynchronous solver / QP error of the ticks since the last check)
        return status

    def result(self):
        status, ticks, acc, ego4 = self.ctx.sim_read(self.n)
        self.ctx.check_error()
        out = stats_columns(status, ticks, acc, self.tick_length)
        out["ego4"] = ego4
        if self.controller != "st":
            out["percent_st"] = (self.takeovers / self.torch.clamp(self.controlled, min=1.0)).cpu().numpy()
        if hasattr(self.policy, "P"):
            out["member"] = np.arange(self.n) // self.policy.n_per_member
        if self.cfgs is not None:
            out["traffic_group"] = np.arange(self.n) // self.n_per_group
        if self.control is not None:
            out["control_group"] = np.arange(self.n) // self.n_per_cell
        if self.solver is not None:
            out["solver_group"] = np.arange(self.n) // self.n_per_solver
        if self.recorder is not None:
            from . import report
            out["report"] = report.Report.from_result(out, self.recorder.read())
        return out


def stats_columns(status, ticks, acc, tick_length):
    """The per-episode columns of the reference's stats report from the world's statistics (``stmpc_sim_read``: status, ticks,
    acc [n][STMPC_SIM_NACC]); used by ``EpisodeRunner.result`` and ``vec_env.MergeVecEnv.drain_episode_stats``."""
    samples = np.maximum(acc[:, 4], 1.0)
    # mean |jerk| as the reference reports it: its jerk history holds a 0 for the first tick (control.py:284-287) and the mean is taken
    # over all ticks (stats.py:60) -- n samples, not n - 1 jerk terms
    out = {"crashed": (status == 2).astype(np.float64), "merged": (status == 1).astype(np.float64), "timed_out": (status == 3).astype(np.float64),
           "mean_speed": acc[:, 0] / samples, "max_speed": acc[:, 1], "mean_abs_jerk": acc[:, 2] / samples,
           "closest_distance": np.where(acc[:, 7] > 0, acc[:, 5], np.nan), "mean_closest_distance": np.where(acc[:, 7] > 0, acc[:, 6] / np.maximum(acc[:, 7], 1.0), np.nan),
           "time_taken": ticks * tick_length, "ticks": ticks, "status": status}
    out["time_to_merge"] = np.where(status == 1, out["time_taken"], np.nan)
    # the reference's "disruption" columns (stats.py:64-68): deceleration of the nearest vehicle behind the ego, per controlled tick past MERGE_POINT_X
    have = acc[:, 10] > 0
    out["mean_disruption"] = np.where(have, acc[:, 8] / np.maximum(acc[:, 10], 1.0), np.nan)
    out["max_disruption"] = np.where(have, acc[:, 9], np.nan)
    out["total_disruption"] = np.where(have, acc[:, 8] * tick_length, np.nan)
    out["disruption_time"] = np.where(have, acc[:, 11] * tick_length, np.nan)
    return out


def run_episodes(n, seed=0, controller="st", policy=None, ctx=None, kmax=32, max_episode_length=100.0, check_every=16, max_ticks=None, record=None, traffic=None,
                 control=None, solver=None):
    """Run ``n`` merge episodes to the end (or for ``max_ticks`` ticks); returns the per-episode columns of the reference's stats report
    (``crashed``, ``merged``, ``mean_speed``, ``max_speed``, ``mean_abs_jerk``, ``closest_distance``, ``mean_closest_distance``,
    ``time_taken``, ``time_to_merge`` (NaN unless merged)) plus ``ticks``, ``status`` (0 still running), ``ego4`` and ``percent_st``
    (the controllers that shield a policy only).

    controller: "st" = ``st.do_st_control`` every tick (TASK "ST"); "combined" = ``do_combined_control`` with ``policy``
    (see ``combined.decide_batch_device``); "first_step" = ``do_conditional_st_based_on_first_step`` behind ``policy`` (``first_step.py``).  record: None, or a ``report.RecorderConfig`` -- the result then holds ``report`` (``report.Report``),
    see ``EpisodeRunner``.  traffic: None, or the traffic groups of ``EpisodeRunner``; the tick limit is then the largest group's ``max_ticks + 1``.
    control: None, or the controller groups of ``EpisodeRunner``.  solver: None, or the solver groups of ``EpisodeRunner``."""
    r = EpisodeRunner(n, seed, controller, policy, ctx, kmax, max_episode_length, record, traffic, control, solver)
    limit = r.max_ticks + 1 if max_ticks is None else min(int(max_ticks), r.max_ticks + 1)
    for tick in range(limit):
        r.tick()
        if tick % check_every == check_every - 1 and (r.status() != 0).all():
            break
    return r.result()


def summary(stats):
    """Column means as the reference's report rows hold them (stats.py:145-158)."""
    return {k: float(np.nanmean(v)) for k, v in stats.items() if k not in ("ticks", "status", "ego4", "report", "member", "traffic_group", "control_group", "solver_group")}


def summary_by_member(stats, P):
    """``summary`` of each member's environments: P dicts, member m from rows [m * n / P, (m + 1) * n / P) of every column (the result of a run
    whose policy was an ``actor.ActorPopulation`` of P members)."""
    return groups.summary_by(stats, P, "members")


def summary_by_group(stats, G):
    """``summary_by_member`` for the G traffic groups of a run with ``traffic``."""
    return groups.summary_by(stats, G, "traffic groups")


def summary_by_control(stats, C):
    """``summary_by_member`` for the C controller groups of a run with ``control``."""
    return groups.summary_by(stats, C, "controller groups")


def summary_by_solver(stats, G):
    """``summary_by_member`` for the G solver groups of a run with ``solver``."""
    return groups.summary_by(stats, G, "solver groups")


def grid_search_st(n_per_cell, seed=0, traffic=None, cells=None, common_random_numbers=True, ctx=None, kmax=16, max_episode_length=100.0, max_ticks=None,
                   check_every=16, record=None):
    """The reference's ``main.do_grid_search_st`` (main.py:43-59: one TASK "ST" process per cell) in ONE run: the ST controller on the traffic type
    ``traffic`` (as ``sim_cfgs`` takes one group; default: the traffic of ``Settings``), once per cell of ``cells`` (default ``st.grid_search_cells()``,
    288 dicts as ``st.param_cfgs`` takes them), ``n_per_cell`` episodes each, every cell a solver group and a traffic group of one runner.
    ``common_random_numbers``: every cell's traffic group gets the same seed (``seed``), so all cells face the same traffic draws and start speeds
    and differ by the solver's settings alone; False: cell c's seed is ``vec_env.episode_seed(seed, c)``.
    Returns ``{"cells": [{"settings": cell, "summary": ``summary`` dict}, ...], "stats": the raw result}``."""
    from . import st, vec_env
    cells = [dict(c) for c in (cells if cells is not None else st.grid_search_cells())]
    if int(n_per_cell) < 1:
        raise ValueError("n_per_cell must be positive")
    st.param_cfgs(cells)                                                # (validates the keys and the count before anything is built)
    base = traffic_settings(traffic) if traffic is not None else {"BASE_TRAFFIC_INTERVAL": getattr(Settings, "BASE_TRAFFIC_INTERVAL", 1.2),
                                                                   "OTHER_CAR_SPEED": getattr(Settings, "OTHER_CAR_SPEED", 7.0)}
    cell_traffic = [dict(base, seed=int(seed) if common_random_numbers else vec_env.episode_seed(seed, c)) for c in range(len(cells))]
    ctx = ctx if ctx is not None else _capi.default_context()
    stats = run_episodes(len(cells) * int(n_per_cell), seed=seed, controller="st", ctx=ctx, kmax=kmax, max_episode_length=max_episode_length,
                         check_every=check_every, max_ticks=max_ticks, record=record, traffic=cell_traffic, solver=cells)
    by = summary_by_solver(stats, len(cells))
    return {"cells": [{"settings": cells[c], "summary": by[c]} for c in range(len(cells))], "stats": stats}


def grid_search_combined(model, traffic, n_per_cell, cells=None, seed=0, common_random_numbers=True, ctx=None, kmax=16, max_episode_length=100.0, record=None,
                         max_ticks=None, check_every=16):
    """The reference's ``main.do_grid_search_combined`` (main.py:62-81: one ``EVALUATE_COMBINED_DDPG`` process per cell) in ONE run: ``model`` (as
    ``actor.population_of`` takes a member: a DDPG model, or a ``DQNLearner`` / ``DQNActor``; or a C51 policy, as ``actor.C51ActorPopulation`` takes one) under the combined controller on the traffic type ``traffic`` (as ``sim_cfgs`` takes one group), once
    per cell of ``cells`` (default ``combined.grid_search_cells()``; dicts as ``combined.control_cfgs`` takes them), ``n_per_cell`` episodes each.
    ``common_random_numbers``: every cell's traffic group gets the same seed (``seed``), so all cells face the same traffic draws and start
    speeds and differ by the controller alone -- something one process per cell cannot give; False: cell c's seed is
    ``vec_env.episode_seed(seed, c)``.
    Returns ``{"cells": [{"settings": cell, "summary": ``summary`` dict}, ...], "stats": the raw result}``."""
    from . import actor, combined
    cells = [dict(c) for c in (cells if cells is not None else combined.grid_search_cells())]
    C = groups.within(len(cells), combined.CONTROL_GROUPS_MAX, "control")
    if int(n_per_cell) < 1:
        raise ValueError("n_per_cell must be positive")
    combined.control_cfgs(cells)                                        # (validates the keys before anything is built)
    t = traffic_settings(traffic)
    if common_random_numbers:
        t["seed"] = int(seed)
    ctx = ctx if ctx is not None else _capi.default_context()
    # (a shipped name or a path is a DDPG model, loaded once; a C51Learner.export_q file, likewise, as a one-row C51Actor)
    one = (actor.C51Actor if actor.all_c51([model]) else actor.DDPGActor)(os.fspath(model), 1, ctx, Settings) if isinstance(model, (str, os.PathLike)) else model
    # (a DQNLearner or a DQNActor: a population of Q-networks; a C51 policy: a population of categorical policies)
    pop = (actor.C51ActorPopulation if actor.all_c51([one]) else actor.population_of)([one] * C, int(n_per_cell), ctx, Settings)
    stats = run_episodes(pop.n, seed=seed, controller="combined", policy=pop, ctx=ctx, kmax=kmax, max_episode_length=max_episode_length, check_every=check_every,
                         max_ticks=max_ticks, record=record, traffic=[dict(t) for _ in range(C)], control=cells)
    by = summary_by_control(stats, C)
    return {"cells": [{"settings": cells[c], "summary": by[c]} for c in range(C)], "stats": stats}


def cross_matrix(models, traffic, n_per_cell, seed=0, ctx=None, kmax=16, max_episode_length=100.0, record=None, max_ticks=None, check_every=16,
                 controller="combined"):
    """The reference's ``combined_{traffic}_{seed}`` diagonal and ``cross_{traffic_1}_network_{traffic_2}_traffic_{seed}`` off-diagonals in ONE run:
    every model of ``models`` (as ``actor.population_of`` takes them: shipped names, paths, DDPG learners and actors -- or, all of them,
    ``DQNLearner``s and ``DQNActor``s, for a matrix of Q-networks; or, all of them, C51 policies as ``actor.C51ActorPopulation`` takes them) under the combined controller on
    every traffic group of ``traffic`` (as ``sim_cfgs`` takes them), ``n_per_cell`` episodes each.  Cell c = i * len(traffic) + j (row-major) pairs
    model i with traffic j: the population repeats each member len(traffic) times, the traffic list is tiled len(models) times, and the cells are
    the groups of one runner (cell c's default seed is ``vec_env.episode_seed(seed, c)``).  ``controller``: "combined" or "first_step" -- the same
    worlds, actors and report under the other shield.
    Returns ``{"matrix": [len(models)][len(traffic)] ``summary`` dicts, "stats": the raw result (with ``member`` = cell and ``traffic_group`` =
    cell), "models": [...], "traffic": [...]}``."""
    from . import actor
    models, traffic = list(models), list(traffic)
    M, T = len(models), len(traffic)
    if controller not in ("combined", "first_step"):
        raise ValueError("cross_matrix runs models under 'combined' or 'first_step', not %r" % (controller,))
    if M < 1 or T < 1:
        raise ValueError("cross_matrix needs at least one model and one traffic group")
    if int(n_per_cell) < 1:
        raise ValueError("n_per_cell must be positive")
    if M * T > _capi.SIM_GROUPS_MAX:
        raise ValueError("%d models x %d traffic groups = %d cells, at most %d fit one run" % (M, T, M * T, _capi.SIM_GROUPS_MAX))
    cell_traffic = [traffic_settings(t) for t in traffic] * M          # (validates the names before anything is built)
    ctx = ctx if ctx is not None else _capi.default_context()
    # (a shipped name or a path is loaded once and its actor repeated along its row; a C51Learner.export_q file, likewise, as a one-row C51Actor)
    loaded = [(actor.C51Actor if actor.all_c51([m]) else actor.DDPGActor)(os.fspath(m), 1, ctx, Settings) if isinstance(m, (str, os.PathLike)) else m for m in models]
    cell_models = [m for m in loaded for _ in range(T)]
    # (every model a C51 policy: a population of categorical policies; a mix of C51 and others is refused by population_of)
    pop = (actor.C51ActorPopulation if actor.all_c51(cell_models) else actor.population_of)(cell_models, int(n_per_cell), ctx, Settings)
    stats = run_episodes(pop.n, seed=seed, controller=controller, policy=pop, ctx=ctx, kmax=kmax, max_episode_length=max_episode_length, check_every=check_every,
                         max_ticks=max_ticks, record=record, traffic=cell_traffic)
    cells = summary_by_group(stats, M * T)
    return {"matrix": [[cells[i * T + j] for j in range(T)] for i in range(M)], "stats": stats, "models": models, "traffic": traffic}
