"""The episode world (``k_sim_init`` / ``k_sim_view`` / ``k_sim_step``, csrc/stmpc_cc_kernels.hpp) against ``oracle/sim_oracle.py``, its host twin in
plain Python fp64 -- BIT FOR BIT: every comparison but the ego's random start speed is ``np.array_equal`` on the values and on their int64 view
(so -0.0 and NaN payloads count), after init and after EVERY tick.  Everything else that steps this world (the vector env, the traffic, controller,
solver and reward groups, the shielded env, the recorder) is tested "bit-identical to the lone world" device against device; this file is where the
lone world itself, the group seeds and the env's episode reset are pinned to the host.

What the device shows: ``sim_read`` (status, ticks, the twelve accumulators, ego4) and ``sim_view`` with Kmax = 64, sensor_radius = 1e9 and other_a
given (every vehicle's x, v, a and the count).  The desired speeds, the insertion delay and the draw counter are not readable; they are pinned
through what they cause over the following ticks (the next insertion's time, the speeds a vehicle accelerates to).

GPU cases (marked ``gpu``; a private ``_capi.Context`` each, never the shared ``gpu_ctx`` world): a. init, b. tick, c. random start speed, d. view,
e. grouped world and vector env; next to case b a queue world (see QUEUE_N) for the one branch no 120-tick episode reaches.  CPU cases (unmarked) keep the GPU cases from passing vacuously: the branch counters of the twin over case b's own
commands, the twin's Krauss helpers against their definitions (not against the kernel), splitmix64's published vector, determinism.
"""
import contextlib
import functools
import math

import numpy as np
import pytest

N, TICKS, MAX_TICKS, VIEW_TICK = 96, 160, 120, 60      # one full workgroup of 64 plus a tail; every episode is over by tick 120 and idles after
KS = 64
BIG_RADIUS = 1e9
SEED_B = 41
CASES_B = [("lane", "default"), ("lane", "fast"), (None, "default"), (None, "fast")]
CAP_OVERRIDES = {"BASE_TRAFFIC_INTERVAL": 1.2, "OTHER_CAR_SPEED": 0.5, "CAR_LENGTH": 3.0}      # stationary traffic that needs more than 64 slots
SEED_C = 58
# The queue world.  A postponed insertion needs a queue that reaches back from the ego (which blocks the highway no earlier than x = -50.58) to the spawn
# point at x = -250: 200 m of jam, which grows by about 7.5 m/s in the "default" traffic and more slowly in "fast".  In case b's worlds (max_ticks = 120,
# i.e. 24 s, of which the ego needs 6 s to reach the junction) that cannot happen whatever the commands; in free flow the insertion test never fails either
# (intervals of at least 1.2 s put the last vehicle 9.8 m ahead).  So the branch gets a world of its own next to case b: "default" traffic, 40 environments,
# 300 ticks, the ego sprinting to the junction and stopping there; every other environment sprints on at tick 215, which dissolves the queue and lets the
# postponed vehicle in.
QUEUE_N, QUEUE_TICKS, QUEUE_RESUME = 40, 300, 215


def _pkg():
    import rl_mpc_lanemerging_amd as pkg
    return pkg


def _orc():
    from oracle import sim_oracle
    return sim_oracle


@contextlib.contextmanager
def _reference_settings(**over):
    """The global Settings at the reference's defaults (plus ``over``) while a cfg, Params or an env is made from them; restored afterwards."""
    pkg = _pkg()
    snap = pkg.Settings.snapshot()
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(over)
    try:
        yield pkg.Settings
    finally:
        pkg.Settings.restore(snap)


def _cfg(traffic, route="lane", seed=SEED_B, vary=1, randomize=0, max_ticks=MAX_TICKS, sensor_radius=None, overrides=None):
    """(SimCfg, Params) of one world: ``traffic`` a name of ``episodes.TRAFFIC_TYPES``; ``max_ticks`` through MAX_EPISODE_LENGTH as the package sets it."""
    from rl_mpc_lanemerging_amd import _capi, episodes
    over = dict(episodes.TRAFFIC_TYPES[traffic], VARY_TRAFFIC_START_TIMES=bool(vary), RANDOMIZE_START_SPEED=bool(randomize))
    over.update(overrides or {})
    if sensor_radius is not None:
        over["SENSOR_RADIUS"] = sensor_radius
    with _reference_settings() as S:
        cfg = episodes.sim_cfg(seed, (max_ticks + 0.5) * S.TICK_LENGTH, route, overrides=over)
        params = _capi.Params.from_settings(S)
    assert cfg.max_ticks == max_ticks
    return cfg, params


def _commands(n=N, ticks=TICKS, seed=2024):
    """Commanded ego speeds [ticks][n] from a seeded host generator.  Columns: 0-23 constant speeds from 0 to 36 m/s (v_max is 30); 24-35 constant with a
    NaN every third tick; 36-47 jumps between 0 and 40 m/s (beyond both acceleration limits) every 3 ... 12 ticks; 48-55 negative commands, from the start
    or after a run-up; 56-63 a fresh uniform(-5, 40) every tick; 64-95 an approach at 14 ... 22 m/s and then a crawl, a stop or a second sprint near or on the
    junction (what makes the highway vehicles follow the ego and brake for it while it laps in)."""
    rng = np.random.default_rng(seed)
    cmd = np.empty((ticks, n))
    cmd[:, 0:24] = np.linspace(0.0, 36.0, 24)
    cmd[:, 24:36] = np.linspace(3.0, 33.0, 12)
    cmd[2::3, 24:36] = np.nan
    for e in range(36, 48):
        t, high = 0, bool(e & 1)
        while t < ticks:
            d = int(rng.integers(3, 13))
            cmd[t:t + d, e] = 40.0 if high else 0.0
            t, high = t + d, not high
    for e in range(48, 56):
        cmd[:, e] = -1.0 - (e - 48)
        if e >= 52:
            cmd[:10 * (e - 50), e] = 18.0
    cmd[:, 56:64] = rng.uniform(-5.0, 40.0, (ticks, 8))
    for e in range(64, 96):
        approach, switch = rng.uniform(14.0, 22.0), int(rng.integers(30, 70))
        cmd[:switch, e] = approach
        cmd[switch:, e] = (0.0, 0.5, 2.0, 6.0)[e % 4]
        if e % 8 >= 6:
            cmd[switch + 35:, e] = 25.0
        if e % 8 == 5:
            cmd[switch + 1::3, e] = np.nan
    return cmd


def _queue_commands():
    cmd = np.zeros((QUEUE_TICKS, QUEUE_N))
    for e in range(QUEUE_N):
        cmd[:19 + e % 4, e] = 26.0 + e % 5
        if e % 2:
            cmd[QUEUE_RESUME:, e] = 30.0
    return cmd


# ---- the twin alone (CPU) ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twin_run(route, traffic):
    """Case b's world stepped by the twin alone through all ticks: the final state, with its branch counters."""
    orc = _orc()
    cfg, params = _cfg(traffic, route)
    c = orc.Cfg(cfg)
    state, cmd = orc.init(c, N), _commands()
    for t in range(TICKS):
        orc.step(state, params, c, cmd[t], params.crash_min_s)
        if t + 1 == VIEW_TICK:                                  # (case d's moment: vehicles in the world and within the package's sensor radius)
            state.view_tick_counts = (np.array([env.nveh for env in state.envs]), orc.view(state, c, KS)["k"])
    return state


@functools.lru_cache(maxsize=None)
def _twin_run_queue():
    orc = _orc()
    cfg, params = _cfg("default", max_ticks=QUEUE_TICKS)
    c = orc.Cfg(cfg)
    state, cmd = orc.init(c, QUEUE_N), _queue_commands()
    for t in range(QUEUE_TICKS):
        orc.step(state, params, c, cmd[t], params.crash_min_s)
    return state


PER_ENV_BRANCHES = ("status_1", "status_2", "status_3", "clamp_a_max", "clamp_a_min", "clamp_zero", "clamp_v_max", "nan_command", "route_vertex",
                    "route_end_crossed", "past_route_end", "follow_binding", "ego_leader_follow", "lap_in_stop", "emergency_floor", "despawn", "insertion",
                    "insertion_postponed", "gap_sample", "disruption_nonzero")


@pytest.mark.parametrize("branch", PER_ENV_BRANCHES)
def test_case_b_commands_reach_every_branch(branch):
    """A condition, not a measurement: over case b's commands the twin takes each branch the GPU comparison is meant to pin, in at least 3
    environments of at least one of case b's worlds.  (If one is not reached the command script changes, never this list.)  One branch cannot be
    reached in those worlds by any command script -- the postponed insertion, see QUEUE_N -- and is reached in the queue world instead, which the
    GPU compares tick by tick like case b's."""
    hits = {case: _twin_run(*case).hits(branch) for case in CASES_B}
    if branch == "insertion_postponed":
        assert max(hits.values()) == 0                           # (should a change of the script reach it there after all, the queue world can go)
        hits = {"queue": _twin_run_queue().hits(branch)}
    assert max(hits.values()) >= 3, hits


def test_queue_world_postpones_insertions_and_makes_them_up():
    orc = _orc()
    state = _twin_run_queue()
    status = orc.read(state)[0]
    assert state.hits("insertion_postponed") >= 10 and state.hits("insertion_after_postponed") >= 5
    assert set(status) == {1, 2, 3} and min((status == s).sum() for s in (1, 2, 3)) >= 3      # (arrivals in the dense traffic too)


@pytest.mark.parametrize("branch", ("straight_approach", "straight_y_floor", "straight_beyond"))
def test_case_b_commands_reach_the_straight_line_branches(branch):
    hits = {case: _twin_run(*case).hits(branch) for case in CASES_B if case[0] is None}
    assert max(hits.values()) >= 3 and min(hits.values()) >= 1, hits


def test_case_b_every_world_ends_and_then_idles():
    orc = _orc()
    for case in CASES_B:
        status, ticks, acc, _ = orc.read(_twin_run(*case))
        assert (status != 0).all() and {2, 3} <= set(status) <= {1, 2, 3} and (case[1] != "fast" or (status == 1).sum() >= 3), case
        assert (ticks[status == 3] == MAX_TICKS).all() and (ticks <= MAX_TICKS).all() and (acc[:, 4] == ticks).all()


def test_case_d_views_hide_and_cut_vehicles():
    """At tick 60 of case b the package's sensor radius hides vehicles, Kmax 8 cuts lists and Kmax 32 holds some whole, in at least 3 environments of
    every world each; finished and running environments are both among them."""
    orc = _orc()
    for case in CASES_B:
        state = _twin_run(*case)
        in_world, in_range = state.view_tick_counts
        assert (in_range < in_world).sum() >= 3 and (in_range > 8).sum() >= 3 and ((in_range > 0) & (in_range < 32)).sum() >= 3, (case, in_world, in_range)
    status_then = [orc.read(_twin_run(*case))[1] for case in CASES_B]
    assert all((ticks < VIEW_TICK).sum() >= 3 and (ticks > VIEW_TICK).sum() >= 3 for ticks in status_then)


def test_slot_cap_cfg_fills_all_64_slots_in_the_twin():
    """Case a's slot-cap cfg (vehicle length 3.0, traffic at 0.5 m/s: minimum spacing 4.25 m over 350 m) ends init with ``x > spawn_x`` and all 64
    slots taken, in every environment; the package's own traffic types never come near the cap."""
    orc = _orc()
    cfg, _ = _cfg("default", overrides=CAP_OVERRIDES)
    assert cfg.veh_length == 3.0 and cfg.other_car_speed == 0.5
    state = orc.init(cfg, N)
    assert state.hits("init_slot_cap") == N and all(env.nveh == KS for env in state.envs)
    assert state.hits("init_min_space") == N
    from rl_mpc_lanemerging_amd import episodes
    for name in episodes.TRAFFIC_TYPES:
        state = orc.init(_cfg(name)[0], N)
        assert state.hits("init_slot_cap") == 0 and max(env.nveh for env in state.envs) < KS


def test_twin_is_deterministic_and_environments_do_not_depend_on_n():
    orc = _orc()
    cfg, params = _cfg("default", "lane")
    cmd, n_small = _commands(), 7
    big = _twin_run("lane", "default")
    runs = []
    for _ in range(2):
        state = orc.init(cfg, n_small)
        for t in range(TICKS):
            orc.step(state, params, cfg, cmd[t, :n_small], params.crash_min_s)
        runs.append(state)
    cfg_big, _ = _cfg("default", "lane", sensor_radius=BIG_RADIUS)
    for state in runs:
        for a, b in zip(orc.read(state), orc.read(big)):
            assert np.array_equal(a, b[:n_small])
        va, vb = orc.view(state, cfg_big, KS), orc.view(big, cfg_big, KS)
        for key in ("ego5", "k", "ox", "ov", "oa"):
            assert np.array_equal(va[key], vb[key][:n_small]), key
        for ea, eb in zip(state.envs, big.envs):
            assert (ea.delay, ea.rng, ea.vc) == (eb.delay, eb.rng, eb.vc)
    other = orc.init(_cfg("default", "lane", seed=SEED_B + 1)[0], n_small)
    assert [e.vx for e in other.envs] != [e.vx for e in runs[0].envs]


# ---- the twin's Krauss helpers against their definitions (never against the kernel) -------------------------------------------------------------
def _brake_distance_loop(speed, decel, ts):
    """Distance covered by a vehicle that reduces its speed by ``decel * ts`` at the start of every step and moves at the new speed for the step
    (SUMO's Euler update), until the speed would fall below zero -- counted a step at a time."""
    dist = 0.0
    while speed - decel * ts >= 0.0 and speed > 0.0:
        speed -= decel * ts
        dist += speed * ts
        if speed == 0.0:
            break
    return dist


def test_brake_gap_is_the_summed_distance_of_a_braking_loop():
    orc = _orc()
    rng = np.random.default_rng(3)
    for decel, ts in ((6.0, 0.2), (6.0, 0.1), (4.5, 0.2), (9.0, 0.25), (2.0, 1.0)):
        red = decel * ts
        speeds = list(rng.uniform(0.0, 40.0, 200)) + [0.0, 0.5 * red]
        for speed in speeds:
            # brakeGapEuler counts the steps in which a whole reduction fits, each travelled at the speed BEFORE the reduction of the next one:
            # steps * speed - red * (1 + ... + steps) = the sum over the loop of the speed after each reduction
            want = _brake_distance_loop(speed, decel, ts)
            got = orc.brake_gap(speed, decel, ts)
            assert abs(got - want) <= 1e-9 * max(1.0, want), (speed, decel, ts, got, want)
    assert orc.brake_gap(0.0, 6.0, 0.2) == 0.0


def _stops_within(v, gap, decel, tau, ts):
    """Distance a vehicle covers from the moment it enters at speed ``v``: it keeps ``v`` for its reaction time and then brakes by ``decel * ts`` per
    step (Euler: each step at the reduced speed); the last, partial reduction brings it to rest."""
    dist = v * tau
    while v > 0.0:
        v = max(v - decel * ts, 0.0)
        dist += v * ts
    return dist


def test_safe_stop_speed_stops_within_the_gap_and_grows_with_it():
    orc = _orc()
    for ts in (0.1, 0.2, 0.25, 1.0):
        for tau in (0.0, 0.5, 1.0):
            for decel in (4.5, 6.0):
                last = 0.0
                for g in np.concatenate([[0.0, 0.0005, 0.001, 0.0011, 0.01], np.linspace(0.05, 150.0, 400)]):
                    v = orc.safe_stop_speed(float(g), decel, tau, ts)
                    assert v >= 0.0 and v >= last, (g, ts, tau, decel, v, last)            # non-decreasing in the gap
                    last = v
                    assert _stops_within(v, g, decel, tau, ts) <= g + 1e-9, (g, ts, tau, decel, v)
                    if g > 1.0:                                                            # and it is the LARGEST such speed: a little faster overshoots
                        assert _stops_within(v * 1.01 + 0.01, g, decel, tau, ts) > g - 0.001 - 1e-9, (g, ts, tau, decel, v)
    assert orc.safe_stop_speed(0.0009, 6.0, 0.5, 0.2) == 0.0


def test_krauss_follow_keeps_behind_a_braking_leader():
    """Follower at ``krauss_follow(gap, lead_v)`` behind a leader ``gap`` ahead that brakes at once with the same deceleration: positions never cross."""
    orc = _orc()
    cfg, _ = _cfg("default")
    c = orc.Cfg(cfg)
    rng = np.random.default_rng(5)
    for gap, lead_v in zip(rng.uniform(0.0, 80.0, 300), rng.uniform(0.0, 20.0, 300)):
        v = orc.krauss_follow(c, float(gap), float(lead_v))
        lead_stop = _brake_distance_loop(float(lead_v), c.veh_decel, c.tick_length)
        assert _stops_within(v, gap + lead_stop, c.veh_decel, c.veh_tau, c.tick_length) <= gap + lead_stop + 1e-9


def test_uniform01_is_splitmix64():
    """splitmix64 (Steele, Lea, Flood: "Fast splittable pseudorandom number generators", 2014; the reference C of Vigna's xoshiro page): from seed 0
    the first outputs are 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F.  Output i is mix(seed + (i + 1) * gamma); the kernel's draw
    ``ctr`` of environment ``env`` is mix(seed + k * gamma) with its own pre-mix k = env * (2^32 + 1) + ctr + 1, so environment 0 under seed 0 IS the
    published stream, and environment 1 starts 2^32 + 1 outputs further on."""
    orc = _orc()
    published = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    for i, want in enumerate(published):
        assert orc.uniform_bits(0, 0, i) == want
        assert orc.uniform01(0, 0, i) == (want >> 11) / 2.0 ** 53
    gamma, m64 = 0x9E3779B97F4A7C15, (1 << 64) - 1
    assert orc.uniform_bits(5, 3, 7) == orc.splitmix64_mix((5 + gamma * (3 * 0x100000001 + 8)) & m64)
    assert orc.uniform_bits(gamma, 0, 0) == published[1]                                   # (a seed moves the stream along)
    assert orc.uniform_bits(0, 0, (1 << 32) + 2) == published[2]                           # the counter wraps at 32 bits ...
    assert orc.uniform_bits((1 << 64) - gamma, 0, 1) == published[0]                       # ... and the state at 64
    from rl_mpc_lanemerging_amd import vec_env
    assert vec_env.episode_seed(0, 1) == published[0] and vec_env.episode_seed(0, 0) == 0  # the group / episode seed rule is the same generator
    assert 0.0 <= min(orc.uniform01(1, e, c) for e in range(20) for c in range(20)) and max(orc.uniform01(1, e, c) for e in range(20) for c in range(20)) < 1.0


def test_fused_sum_of_squares_is_rounded_once():
    orc = _orc()
    a, b = 1.0 + 5 * 2.0 ** -29, 2.0 ** -27                          # a * a leaves 25/64 ulp behind, b * b adds 16/64: together above a half
    assert orc.fma(a, a, b * b) == float.fromhex("0x1.0000005000001p+0") and a * a + b * b == float.fromhex("0x1.0000005000000p+0")
    from fractions import Fraction
    assert Fraction(orc.fma(a, a, b * b)) == Fraction(float(Fraction(a) ** 2 + Fraction(b * b)))
    assert orc.fma(3.0, 3.0, 16.0) == 25.0


def test_start_speed_seed_clips_on_both_sides():
    """Case c's cfg: the twin's own start speeds are clipped to the lower bound in some environments and to the upper bound in others."""
    orc = _orc()
    state = orc.init(_cfg("default", randomize=1, seed=SEED_C)[0], N)
    assert state.start_clip.count(-1) >= 1 and state.start_clip.count(1) >= 1 and state.start_clip.count(0) >= N // 2
    assert all(env.rng >= 4 for env in state.envs)


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b, equal_nan=True):
        return False
    return a.dtype.kind != "f" or np.array_equal(a.view(np.int64), b.view(np.int64))


class _Device:
    """A private context with the buffers ``sim_view`` writes, and the world's host snapshot."""

    def __init__(self, n, ctx=None):
        import torch
        from rl_mpc_lanemerging_amd import _capi
        self.torch, self.n = torch, n
        self.ctx = ctx if ctx is not None else _capi.Context(-1)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.cmd = torch.zeros(n, dtype=torch.float64, device=self.dev)

    def view(self, cfg, kmax, with_acc=True):
        torch, n = self.torch, self.n
        # (filled with a sentinel: the kernel must write every cell, zeros beyond k included)
        ego5 = torch.full((n, 5), -7.0, dtype=torch.float64, device=self.dev)
        k = torch.full((n,), -7, dtype=torch.int32, device=self.dev)
        ox, ov, oa = (torch.full((n, kmax), -7.0, dtype=torch.float64, device=self.dev) for _ in range(3))
        self.ctx.sim_view(cfg, n, kmax, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr() if with_acc else 0)
        torch.cuda.synchronize()
        self.ctx.check_error()
        return {"ego5": ego5.cpu().numpy(), "k": k.cpu().numpy(), "ox": ox.cpu().numpy(), "ov": ov.cpu().numpy(), "oa": oa.cpu().numpy() if with_acc else None}

    def snapshot(self, cfg_big):
        out = self.view(cfg_big, KS)
        out["status"], out["ticks"], out["acc"], out["ego4"] = self.ctx.sim_read(self.n)
        return out

    def set_cmd(self, cmd):
        self.cmd.copy_(self.torch.from_numpy(np.ascontiguousarray(cmd, dtype=np.float64)))
        return self.cmd.data_ptr()


def _twin_snapshot(states, cfg_big):
    """The snapshot of one twin state, or of several stacked (the groups of a grouped world)."""
    orc = _orc()
    parts = []
    for state in states:
        out = orc.view(state, cfg_big, KS)
        out["status"], out["ticks"], out["acc"], out["ego4"] = orc.read(state)
        parts.append(out)
    return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}


SNAP_KEYS = ("status", "ticks", "k", "ego4", "ego5", "acc", "ox", "ov", "oa")


def _first_difference(dev, twin, where):
    for key in SNAP_KEYS:
        if not _bits_equal(dev[key], twin[key]):
            d, t = dev[key], twin[key]
            rows = np.nonzero((d.reshape(len(d), -1).view(np.int64) if d.dtype.kind == "f" else d.reshape(len(d), -1))
                              != (t.reshape(len(t), -1).view(np.int64) if t.dtype.kind == "f" else t.reshape(len(t), -1)))
            e, q = int(rows[0][0]), int(rows[1][0])
            return "%s: %s differs first in environment %d, column %d: device %r, twin %r (%d environments differ)" % (
                where, key, e, q, d.reshape(len(d), -1)[e, q], t.reshape(len(t), -1)[e, q], len(set(rows[0].tolist())))
    return None


def _check_view(dev, twin, ego5_full, kmax, with_acc, where):
    """Case d on one (Kmax, other_a) combination: equal to the twin's view, and by its own properties -- the count within 0 ... Kmax, front to back,
    +0.0 beyond k, ego5[4] the ego's s."""
    problems = []
    for key in ("ego5", "k", "ox", "ov") + (("oa",) if with_acc else ()):
        if not _bits_equal(dev[key], twin[key]):
            problems.append("%s: %s differs from the twin's" % (where, key))
    k = dev["k"]
    if not ((k >= 0) & (k <= kmax)).all():
        return problems + ["%s: count out of range" % where]
    if not _bits_equal(dev["ego5"][:, 4], ego5_full[:, 4]):
        problems.append("%s: ego5[4] is not the ego's s" % where)
    for e in range(len(k)):
        ke = int(k[e])
        if (np.diff(dev["ox"][e, :ke]) >= 0).any():
            problems.append("%s: environment %d is not front to back" % (where, e))
        for key in ("ox", "ov") + (("oa",) if with_acc else ()):
            if dev[key][e, ke:].any() or np.signbit(dev[key][e, ke:]).any():
                problems.append("%s: environment %d: %s is not +0.0 beyond k" % (where, e, key))
    return problems


def _lockstep(dev, states, step_device, step_twin, cfg_big, ticks, after=None):
    """The device and the twin(s) in lock-step: compared after init and after every tick; the first difference (a string) or None.
    ``after(t, device snapshot)``: a hook after the comparison of tick t."""
    diff = _first_difference(dev.snapshot(cfg_big), _twin_snapshot(states, cfg_big), "after init")
    for t in range(ticks):
        if diff is not None:
            break
        step_device(t)
        step_twin(t)
        snap = dev.snapshot(cfg_big)
        diff = _first_difference(snap, _twin_snapshot(states, cfg_big), "after tick %d" % (t + 1))
        if diff is None and after is not None:
            after(t + 1, snap)
    return diff


def _lone_world(cfg, cfg_big, params, n, cmd, ticks, start_speeds_from_device=False, after=None):
    """A lone world of ``n`` environments on a private context against one twin: (first difference or None, the twin's state)."""
    orc = _orc()
    dev = _Device(n)
    dev.ctx.sim_init(cfg, n)
    state = orc.init(cfg, n, start_speeds=dev.ctx.sim_read(n)[3][:, 2].copy() if start_speeds_from_device else None)
    state.device_start_speeds = dev.ctx.sim_read(n)[3][:, 2].copy()
    diff = _lockstep(dev, [state], lambda t: dev.ctx.sim_step(params, cfg, n, dev.set_cmd(cmd[t])),
                     lambda t: orc.step(state, params, cfg, cmd[t], params.crash_min_s), cfg_big, ticks,
                     None if after is None else (lambda t, snap: after(t, snap, dev, state)))
    dev.ctx.close()
    return diff, state


@functools.lru_cache(maxsize=None)
def _device_run_b(route, traffic):
    """Case b (and, at tick VIEW_TICK, case d) once per world.  Returns (first difference or None, case d's problems, the twin's branch hits)."""
    orc = _orc()
    cfg, params = _cfg(traffic, route)
    cfg_big, _ = _cfg(traffic, route, sensor_radius=BIG_RADIUS)
    assert cfg.sensor_radius == 125.0 and cfg_big.sensor_radius == BIG_RADIUS
    problems = []

    def views(t, full, dev, state):
        if t != VIEW_TICK:
            return
        for kmax in (8, 32):
            for with_acc in (True, False):
                where = "Kmax %d, other_a %s" % (kmax, "given" if with_acc else "null")
                problems.extend(_check_view(dev.view(cfg, kmax, with_acc), orc.view(state, cfg, kmax, with_acc), full["ego5"], kmax, with_acc, where))
        problems.append("seen")

    diff, state = _lone_world(cfg, cfg_big, params, N, _commands(), TICKS, after=views)
    if diff is None:
        assert problems and problems[-1] == "seen"
    return diff, tuple(p for p in problems if p != "seen"), {name: state.hits(name) for name in orc.BRANCHES}


@pytest.mark.gpu
@pytest.mark.parametrize("traffic", ["low", "medium", "default", "moderate", "fast"])
@pytest.mark.parametrize("vary", [0, 1])
def test_init_equals_the_twin(traffic, vary):
    """a. N = 96, the five distinct rows of TRAFFIC_TYPES, insertion times fixed and varied, the start speed fixed: counts, positions, speeds,
    accelerations and the zeroed accumulators (acc[5] == 1e300) equal the twin's."""
    orc = _orc()
    cfg, _ = _cfg(traffic, vary=vary)
    cfg_big, _ = _cfg(traffic, vary=vary, sensor_radius=BIG_RADIUS)
    dev = _Device(N)
    dev.ctx.sim_init(cfg, N)
    snap = dev.snapshot(cfg_big)
    dev.ctx.close()
    assert _first_difference(snap, _twin_snapshot([orc.init(cfg, N)], cfg_big), "after init") is None
    assert (snap["acc"][:, 5] == 1e300).all() and not np.delete(snap["acc"], 5, axis=1).any()
    assert (snap["k"] > 5).all() and (snap["status"] == 0).all() and (snap["ticks"] == 0).all()
    assert (snap["ego4"][:, 2] == 15.0).all()


@pytest.mark.gpu
def test_init_stops_at_the_slot_cap():
    """a. Vehicle length 3.0 and traffic at 0.5 m/s: the stationary traffic needs more than 64 slots; nveh == 64 exactly, equal to the twin (which
    reaches the cap on its own: test_slot_cap_cfg_fills_all_64_slots_in_the_twin), and the next ticks, in which no vehicle can enter, stay equal."""
    cfg, params = _cfg("default", overrides=CAP_OVERRIDES)
    cfg_big, _ = _cfg("default", overrides=CAP_OVERRIDES, sensor_radius=BIG_RADIUS)
    first = []
    diff, state = _lone_world(cfg, cfg_big, params, N, _commands(), 12, after=lambda t, snap, dev, state: first.append(snap["k"]) if t == 1 else None)
    assert diff is None, diff
    assert state.hits("init_slot_cap") == N and (first[0] == KS).all()        # (0.1 m a tick: nobody has left after the first one)
    assert state.hits("insertion_no_slot") == N                              # the vehicle that did not fit is due at once, and has no slot


@pytest.mark.gpu
def test_view_takes_the_worlds_64_slots_and_no_more():
    """``stmpc_sim_view_device`` takes rows of up to 64 vehicles (the world's slots; the solver's entries stop at 32) and refuses 0 and 65."""
    from rl_mpc_lanemerging_amd import _capi
    cfg, _ = _cfg("default")
    dev = _Device(8)
    dev.ctx.sim_init(cfg, 8)
    assert (dev.view(cfg, KS)["k"] > 0).all()
    for bad in (0, KS + 1):
        with pytest.raises(_capi.StmpcError):
            dev.view(cfg, bad)
    dev.ctx.close()


@pytest.mark.gpu
def test_queue_world_equals_the_twin():
    """b, continued: the world in which insertions are postponed (see QUEUE_N) and made up for, 300 ticks, compared after every tick."""
    cfg, params = _cfg("default", max_ticks=QUEUE_TICKS)
    cfg_big, _ = _cfg("default", max_ticks=QUEUE_TICKS, sensor_radius=BIG_RADIUS)
    diff, state = _lone_world(cfg, cfg_big, params, QUEUE_N, _queue_commands(), QUEUE_TICKS)
    assert diff is None, diff
    assert state.hits("insertion_postponed") >= 10 and state.hits("insertion_after_postponed") >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("route,traffic", CASES_B)
def test_every_tick_equals_the_twin(route, traffic):
    """b. N = 96, 160 ticks of the scripted commands (``_commands``), max_ticks = 120: state and full view equal the twin's after every tick."""
    diff, _, hits = _device_run_b(route, traffic)
    assert diff is None, diff
    assert hits["status_2"] and hits["status_3"] and hits["insertion"] and hits["despawn"] and hits["lap_in_stop"]


@pytest.mark.gpu
@pytest.mark.parametrize("route,traffic", CASES_B)
def test_view_at_the_packages_radius(route, traffic):
    """d. After tick 60 of case b, the package's own sensor radius (125 m) with Kmax 8 and 32, other_a given and null: equal to the twin's view;
    count, front-to-back order, +0.0 beyond k, ego5[4] == ego_s (that the radius hides vehicles and Kmax 8 cuts lists:
    test_case_d_views_hide_and_cut_vehicles)."""
    diff, problems, _ = _device_run_b(route, traffic)
    assert diff is None, diff
    assert not problems, problems


def _ulp_distance(a, b):
    """Units in the last place between two arrays of positive finite doubles (adjacent doubles have adjacent bit patterns)."""
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


ULP_BOUND = 4


@pytest.mark.gpu
def test_random_start_speed_within_ulps_then_bit_equal():
    """c. ``randomize_start_speed = 1``: the device's start speeds (its ``log`` and ``cos`` are not correctly rounded) equal the twin's
    ``math.log`` / ``math.cos`` version within 4 ulp, and exactly the clip bound where the twin's value is clipped.  The run then goes on with
    the device's start speeds handed to the twin and is bit-equal from there, which pins that exactly two draws were consumed.
    Measured on an MI355X over these 96 draws: at most 1 ulp (2 environments differ; 2 are clipped, one to each bound), so the bound stays at 4."""
    cfg, params = _cfg("default", randomize=1, seed=SEED_C)
    cfg_big, _ = _cfg("default", randomize=1, seed=SEED_C, sensor_radius=BIG_RADIUS)
    diff, state = _lone_world(cfg, cfg_big, params, N, _commands(), 60, start_speeds_from_device=True)
    v_dev, v_host, clip = state.device_start_speeds, np.array(state.start_speed_host), np.array(state.start_clip)
    ulps = _ulp_distance(v_dev, v_host)
    print("start speed: max ulp distance device / host %d (%d environments differ, %d clipped)" % (ulps.max(), (ulps > 0).sum(), (clip != 0).sum()))
    assert (clip == -1).any() and (clip == 1).any()
    assert (v_dev[clip == -1] == cfg.min_start_speed).all() and (v_dev[clip == 1] == cfg.max_start_speed).all()
    assert ulps.max() <= ULP_BOUND, ulps.max()
    assert diff is None, diff
    assert state.hits("insertion") == N                                   # (every environment drew an insertion time after its start speed)


@pytest.mark.gpu
def test_grouped_world_equals_one_twin_per_group():
    """e. A two-group world (``sim_init_groups``: "low" and "fast", 48 environments each) against two twins made WITHOUT ``episodes.sim_cfgs``: group
    g's twin is the lone twin of that traffic under ``vec_env.episode_seed(seed, g)`` with LOCAL environment indices -- the per-group cfg and the seed
    rule pinned to the host, 40 ticks, compared after each."""
    from rl_mpc_lanemerging_amd import episodes, vec_env
    orc = _orc()
    names, npg, seed, ticks = ("low", "fast"), 48, 77, 40
    with _reference_settings(RANDOMIZE_START_SPEED=False) as S:
        table = episodes.sim_cfgs(list(names), seed, (MAX_TICKS + 0.5) * S.TICK_LENGTH)
    twins_cfg = []
    for g, name in enumerate(names):
        c = orc.Cfg(_cfg(name, seed=0)[0])
        c.seed = vec_env.episode_seed(seed, g)
        twins_cfg.append(c)
    assert twins_cfg[0].seed == seed and twins_cfg[1].seed not in (seed, seed + 1)
    cfg_big, params = _cfg("low", sensor_radius=BIG_RADIUS)
    dev, cmd = _Device(2 * npg), _commands()
    dev.ctx.sim_init_groups(table, npg)
    assert dev.ctx.sim_groups() == (2, npg)
    states = [orc.init(c, npg) for c in twins_cfg]
    def step_twins(t):
        for g, (c, state) in enumerate(zip(twins_cfg, states)):
            orc.step(state, params, c, cmd[t, g * npg:(g + 1) * npg], params.crash_min_s)
    diff = _lockstep(dev, states, lambda t: dev.ctx.sim_step_groups(params, 2 * npg, dev.set_cmd(cmd[t])), step_twins, cfg_big, ticks)
    dev.ctx.close()
    assert diff is None, diff
    assert all(state.hits("insertion") >= npg // 2 for state in states)


def _speed_from_jerk(S, v, a, jerk):
    """control.get_ego_speed_from_jerk (control.py:160-171): what the continuous-jerk env commands."""
    na = a + jerk * S.TICK_LENGTH
    na = min(max(na, S.MAX_NEGATIVE_ACCELERATION), S.MAX_POSITIVE_ACCELERATION)
    nv = v + na * S.TICK_LENGTH
    return min(max(nv, 0), S.MAX_SPEED)


@pytest.mark.gpu
def test_vector_env_resets_to_the_twins_episode_init():
    """e. ``MergeVecEnv`` (continuous jerk, autoreset): 72 environments, episodes of 15 ticks, 40 steps of seeded jerks.  The twin is stepped with the
    speed ``control.get_ego_speed_from_jerk`` gives; where its episode ends it is replaced by ``init(cfg, seed=episode_seed(seed, j))`` with the draw
    counter j * 2^16 further on (include/stmpc.h, stmpc_env_step_device) and goes on under the RUN's seed.  After every step the world equals the twin's,
    the flags say which episodes ended, and ``final_stats`` holds the ended episode's accumulators."""
    import torch
    from rl_mpc_lanemerging_amd import _capi, episodes, vec_env
    orc = _orc()
    n, seed, ep_ticks, steps = 72, 19, 15, 40
    rng = np.random.default_rng(8)
    with _reference_settings(RANDOMIZE_START_SPEED=False, MAX_EPISODE_LENGTH=(ep_ticks + 0.5) * 0.2) as S:
        assert S.TICK_LENGTH == 0.2
        env = vec_env.MergeVecEnv(n, "sumo-jerk-continuous-v0", seed=seed, reward="Continuous", autoreset=True)
        cfg = episodes.sim_cfg(seed, float(S.MAX_EPISODE_LENGTH))
        cfg_big = episodes.sim_cfg(seed, float(S.MAX_EPISODE_LENGTH), overrides={"SENSOR_RADIUS": BIG_RADIUS})
        params = _capi.Params.from_settings(S)
        assert cfg.max_ticks == ep_ticks and not cfg.randomize_start_speed
        c = orc.Cfg(cfg)
        dev = _Device(n, env.ctx)
        env.reset()
        state = orc.init(c, n)
        episode = [0] * n
        diff = _first_difference(dev.snapshot(cfg_big), _twin_snapshot([state], cfg_big), "after reset")
        resets = 0
        for t in range(steps):
            if diff is not None:
                break
            jerk = rng.uniform(-6.0, 6.0, n)
            _, _, term, trunc, info = env.step(torch.from_numpy(jerk).to(dev.dev))
            cmd = [_speed_from_jerk(S, e.ego4[2], e.ego4[3], float(j)) for e, j in zip(state.envs, jerk)]
            orc.step(state, params, c, cmd, params.crash_min_s)
            ended = np.array([e.status != 0 for e in state.envs])
            final_acc = orc.read(state)[2]
            for e in np.nonzero(ended)[0]:
                episode[e] += 1
                state.envs[e] = orc.init_env(c, state, int(e), vec_env.episode_seed(seed, episode[e]))
                state.envs[e].rng = (state.envs[e].rng + (episode[e] << 16)) & 0xFFFFFFFF
                resets += 1
            torch.cuda.synchronize()
            if not np.array_equal((term | trunc).cpu().numpy(), ended):
                diff = "after step %d: the device ended episodes in %s, the twin in %s" % (t + 1, np.nonzero((term | trunc).cpu().numpy())[0], np.nonzero(ended)[0])
                break
            stats = info["final_stats"].cpu().numpy()
            if not _bits_equal(stats[ended, :12], final_acc[ended]):
                diff = "after step %d: final_stats differs from the ended episodes' accumulators" % (t + 1)
                break
            diff = _first_difference(dev.snapshot(cfg_big), _twin_snapshot([state], cfg_big), "after step %d" % (t + 1))
        env.check_error()
    assert diff is None, diff
    assert resets >= 2 * n and max(episode) >= 2 and state.hits("insertion") >= n // 2
