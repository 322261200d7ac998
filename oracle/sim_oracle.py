"""Host twin of the episode world: ``k_sim_init`` / ``k_sim_view`` / ``k_sim_step`` (csrc/stmpc_cc_kernels.hpp, namespace ``sim``) restated in
plain Python floats and ints, one environment at a time, in the kernels' operation order.

TEST INFRASTRUCTURE ONLY, like ``st_oracle.py`` -- importable from tests/, never from the product package.  It imports neither the compiled
library nor anything under csrc/: the model is the kernels' comment block (SUMO's ``maximumSafeStopSpeedEuler`` / ``brakeGapEuler``, every
vehicle planning on the positions at the START of the step), the draws are splitmix64 in integers, and ``ego_s`` is ``control.get_ego_s``
(control.py:373-380) with ``x * x`` for the squares as the device evaluates it.

Why bit equality can be asked for: the library is compiled without contraction and without fast-math, ``+ - * / sqrt`` are correctly rounded on
the device (tests/test_gpu_parity.py::test_device_arithmetic_is_ieee), and a Python float is an IEEE binary64 whose ``+ - * /`` and
``math.sqrt`` are correctly rounded too.  Every expression below therefore keeps the kernel's association, and every selection keeps the kernel's
comparison (``a < b ? a : b``, never ``min``), so that equal values, signed zeros and NaN commands take the same side.

Representational notes (causes of differences that are not model differences):
  * the two ``__builtin_fma(a, a, b * b)`` sites -- the route segment length and the straight-line norm -- are ONE rounding of ``a * a + fl(b * b)``:
    ``fma`` below is ``math.fma`` where the interpreter has it, else the exact rational value rounded once by ``float(Fraction)``;
  * ``floor`` keeps the sign of a zero argument (``math.floor`` returns an int and would lose it);
  * ``(int)(speed / red)`` truncates toward zero, as ``int()`` of a float does;
  * the draw counter wraps at 32 bits (the kernel's ``unsigned``), the hash at 64.

Not restated:
  * ``speed_dev > 0`` (Box-Muller speed factors of the vehicles on spawn).  ``episodes.sim_cfg`` fixes it at 0.0, so it is not reachable from the
    package; ``init`` and ``step`` refuse such a cfg.
  * the device's ``log`` and ``cos``.  They are not correctly rounded, so the ego's random start speed (``randomize_start_speed``) cannot be
    bit-pinned: ``init`` takes the start speeds as an argument (hand it the device's), always consumes the two draws, and keeps its own
    ``math.log`` / ``math.cos`` version in ``State.start_speed_host`` (with ``State.start_clip``: -1 / 0 / +1 where that value was clipped to the
    lower bound / not at all / to the upper bound) for a toleranced comparison.

Cfg fields are read by their ``stmpc_sim_cfg`` names (include/stmpc.h) from a ``_capi.SimCfg``-shaped object or a dict; params
(``a_min``, ``a_max``, ``v_max``) likewise from a ``_capi.Params``-shaped object or a dict.
"""
import math
from fractions import Fraction

import numpy as np

KS = 64                 # vehicle slots per environment
NACC = 12               # statistics per environment
INF = float("inf")
_M64 = 0xFFFFFFFFFFFFFFFF
_M32 = 0xFFFFFFFF

if hasattr(math, "fma"):
    fma = math.fma
else:
    def fma(a, b, c):
        """a * b + c with one rounding (finite arguments): the exact rational value, which CPython converts correctly rounded."""
        return float(Fraction(a) * Fraction(b) + Fraction(c))

#: the branches ``init`` and ``step`` count per environment (``State.counts[name][env]``)
BRANCHES = ("status_1", "status_2", "status_3", "clamp_a_max", "clamp_a_min", "clamp_zero", "clamp_v_max", "nan_command", "route_vertex",
            "route_end_crossed", "past_route_end", "straight_approach", "straight_y_floor", "straight_beyond", "follow_binding", "ego_leader_follow",
            "ego_leader_binding", "lap_in_stop", "emergency_floor", "despawn", "insertion", "insertion_postponed", "insertion_after_postponed",
            "insertion_no_slot", "gap_sample", "disruption_nonzero", "init_slot_cap", "init_min_space")


# ---- cfg ---------------------------------------------------------------------------------------------------------------------------------------
_CFG_FIELDS = ("tick_length", "other_car_speed", "base_traffic_interval", "spawn_x", "despawn_x", "ego_start_x", "ego_start_y", "arrive_x", "sensor_radius",
               "start_speed", "start_speed_std", "min_start_speed", "max_start_speed", "veh_accel", "veh_decel", "veh_min_gap", "veh_tau",
               "veh_emergency_decel", "veh_length", "veh_width", "speed_dev", "disruption_min_s")
_CFG_INTS = ("vary_traffic_start_times", "randomize_start_speed", "max_ticks", "seed")


def _get(obj, name):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


class Cfg:
    """A cfg as plain Python values under the header's names, with the route as two lists (``route_x``, ``route_y``; None without a route)."""

    def __init__(self, cfg):
        for name in _CFG_FIELDS:
            setattr(self, name, float(_get(cfg, name)))
        for name in _CFG_INTS:
            setattr(self, name, int(_get(cfg, name)))
        self.seed &= _M64
        if isinstance(cfg, dict):
            xy, n = cfg.get("ego_route_xy"), cfg.get("ego_route_n")
            flat = None if xy is None else [float(v) for v in np.asarray(xy, dtype=np.float64).reshape(-1)]
            n = 0 if flat is None else (len(flat) // 2 if n is None else int(n))
        else:
            n = int(cfg.ego_route_n) if cfg.ego_route_xy else 0
            flat = [float(cfg.ego_route_xy[i]) for i in range(2 * n)] if n else None
        if n >= 2:                                  # (a route of fewer than two points is none: the straight lines)
            self.route_x, self.route_y = flat[0:2 * n:2], flat[1:2 * n:2]
        else:
            self.route_x = self.route_y = None
        if self.speed_dev > 0.0:
            raise ValueError("speed_dev > 0 is not restated by the host twin (not reachable from the package)")


def as_cfg(cfg):
    return cfg if isinstance(cfg, Cfg) else Cfg(cfg)


# ---- draws -------------------------------------------------------------------------------------------------------------------------------------
def splitmix64_mix(z):
    """The output function of splitmix64 (Steele, Lea, Flood 2014): the state ``z`` (already advanced by the golden gamma) to the output."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def uniform_bits(seed, env, ctr):
    """The 64-bit word behind draw ``ctr`` of environment ``env``: splitmix64's output for the state seed + gamma * (env * (2^32 + 1) + ctr + 1)."""
    k = ((int(env) & _M64) * 0x100000001 + (int(ctr) & _M32) + 1) & _M64
    return splitmix64_mix((int(seed) + 0x9E3779B97F4A7C15 * k) & _M64)


def uniform01(seed, env, ctr):
    """Draw ``ctr`` of environment ``env`` under ``seed``, in [0, 1): the top 53 bits of ``uniform_bits`` (exact in binary64)."""
    return float(uniform_bits(seed, env, ctr) >> 11) * (1.0 / 9007199254740992.0)


# ---- Krauss (SUMO's Euler forms) ---------------------------------------------------------------------------------------------------------------
def _floor(x):
    f = float(math.floor(x))
    return math.copysign(0.0, x) if f == 0.0 else f


def brake_gap(speed, decel, ts):
    """Distance covered while braking from ``speed`` with ``decel`` in whole steps of ``ts`` (MSCFModel::brakeGapEuler, headway 0)."""
    red = decel * ts
    steps = int(speed / red)
    return ts * (float(steps) * speed - red * float(steps) * float(steps + 1) / 2.0)


def safe_stop_speed(gap, decel, tau, ts):
    """Largest speed from which a vehicle still stops within ``gap`` when it brakes with ``decel`` after ``tau`` (MSCFModel::maximumSafeStopSpeedEuler)."""
    g = gap - 0.001
    if g < 0.0:
        return 0.0
    b = decel * ts
    t = tau
    s_ = ts
    n = _floor(0.5 - ((t + (math.sqrt((s_ * s_) + (4.0 * ((s_ * (2.0 * g / b - t)) + (t * t)))) * -0.5)) / s_))
    h = 0.5 * n * (n - 1.0) * b * s_ + n * b * t
    r = (g - h) / (n * s_ + t)
    x = n * b + r
    return x if x > 0.0 else 0.0


def krauss_follow(c, gap, lead_speed):
    """The speed that stays safe behind a leader ``gap`` ahead (net of minGap) that may brake with the same deceleration (maximumSafeFollowSpeed)."""
    return safe_stop_speed(gap + brake_gap(lead_speed, c.veh_decel, c.tick_length), c.veh_decel, c.veh_tau, c.tick_length)


def ego_s(x, y):
    """control.get_ego_s (control.py:373-380) with x * x for the squares: merge points (-50.9, 1.72), x = 1.5 and x = -51.0."""
    dx, dy = x - -50.9, y - 1.72
    if x < -50.9:
        return -math.sqrt(dx * dx + dy * dy)
    if x < 1.5:
        return math.sqrt(dx * dx + dy * dy)
    return x - 1.5 + (1.5 - -51.0)


# ---- state -------------------------------------------------------------------------------------------------------------------------------------
class Env:
    __slots__ = ("ego4", "nveh", "vx", "vv", "va", "vc", "delay", "status", "ticks", "rng", "acc")


class State:
    """``envs``: one ``Env`` per environment (ego4 [4], nveh, vx / vv / va / vc [64], delay, status, ticks, rng, acc [12]); ``counts``: branch name
    -> per-environment number of times ``init`` / ``step`` took it."""

    def __init__(self, n):
        self.n = int(n)
        self.envs = []
        self.counts = {name: [0] * self.n for name in BRANCHES}
        self.start_speed_host = [None] * self.n
        self.start_clip = [0] * self.n
        self._postponed = [False] * self.n                    # (bookkeeping of the counters only: the last insertion test of the environment failed)

    def hits(self, name):
        """Number of environments that took branch ``name`` at least once."""
        return sum(1 for v in self.counts[name] if v)


def start_speed_host(c, u1, u2):
    """(v0, clip) of control.get_ego_start_speed (control.py:198-204) with the host's ``math.log`` / ``math.cos``."""
    v0 = c.start_speed + c.start_speed_std * math.sqrt(-2.0 * math.log(u1 if u1 > 1e-300 else 1e-300)) * math.cos(6.283185307179586 * u2)
    if v0 < c.min_start_speed:
        return c.min_start_speed, -1
    if v0 > c.max_start_speed:
        return c.max_start_speed, 1
    return v0, 0


def init_env(c, state, e, seed, start_speed=None):
    """Environment ``e`` of ``k_sim_init`` with ``seed`` in place of the cfg's: the highway traffic in its stationary state, the ego at its start."""
    cnt = state.counts
    ctr = 0
    env = Env()
    env.vx, env.vv, env.va, env.vc = [0.0] * KS, [0.0] * KS, [0.0] * KS, [0.0] * KS
    n = 0
    if c.vary_traffic_start_times:
        head0 = c.base_traffic_interval + uniform01(seed, e, ctr)
        ctr += 1
    else:
        head0 = c.base_traffic_interval + 0.0
    x = c.despawn_x - c.other_car_speed * uniform01(seed, e, ctr) * head0
    ctr += 1
    min_space = c.veh_length + c.veh_min_gap + c.other_car_speed * c.veh_tau
    while x > c.spawn_x and n < KS:
        vc_ = c.other_car_speed                               # (cruise_speed with speed_dev = 0)
        env.vx[n] = x
        env.vv[n] = vc_ if vc_ < c.other_car_speed else c.other_car_speed
        env.va[n] = 0.0
        env.vc[n] = vc_
        n += 1
        if c.vary_traffic_start_times:
            step = c.other_car_speed * (c.base_traffic_interval + uniform01(seed, e, ctr))
            ctr += 1
        else:
            step = c.other_car_speed * (c.base_traffic_interval + 0.0)
        if step > min_space:
            x -= step
        else:
            x -= min_space
            cnt["init_min_space"][e] += 1
    if x > c.spawn_x:
        cnt["init_slot_cap"][e] += 1
    env.nveh = n
    env.delay = (x - c.spawn_x) / (-c.other_car_speed if c.other_car_speed > 0 else -1.0)
    v0 = c.start_speed
    if c.randomize_start_speed:
        u1 = uniform01(seed, e, ctr)
        u2 = uniform01(seed, e, ctr + 1)
        ctr += 2
        v0, clip = start_speed_host(c, u1, u2)
        state.start_speed_host[e], state.start_clip[e] = v0, clip
        if start_speed is not None:
            v0 = float(start_speed)
    env.ego4 = [c.ego_start_x, c.ego_start_y, v0, 0.0]
    env.status, env.ticks, env.rng = 0, 0, ctr & _M32
    env.acc = [0.0] * NACC
    env.acc[5] = 1e300
    return env


def init(cfg, n, seed=None, start_speeds=None):
    """``k_sim_init`` for ``n`` environments; ``seed``: in place of the cfg's (an episode seed of the vector env's reset); ``start_speeds``: [n] values
    to take for the ego's random start speed (the device's) in place of the ``math.log`` / ``math.cos`` ones (read only with ``randomize_start_speed``)."""
    c = as_cfg(cfg)
    seed = c.seed if seed is None else int(seed) & _M64
    state = State(n)
    for e in range(state.n):
        state.envs.append(init_env(c, state, e, seed, None if start_speeds is None else start_speeds[e]))
    return state


def view(state, cfg, kmax, with_acc=True):
    """``k_sim_view``: the planner's view -- ``ego5`` [n][5], ``k`` [n] int32, ``ox`` / ``ov`` / ``oa`` [n][kmax] (``oa`` None without ``with_acc``)."""
    c = as_cfg(cfg)
    n, kmax = state.n, int(kmax)
    ego5, k_count = np.zeros((n, 5)), np.zeros(n, dtype=np.int32)
    ox, ov = np.zeros((n, kmax)), np.zeros((n, kmax))
    oa = np.zeros((n, kmax)) if with_acc else None
    for e, env in enumerate(state.envs):
        ex, ey = env.ego4[0], env.ego4[1]
        ego5[e, :4] = env.ego4
        ego5[e, 4] = ego_s(ex, ey)
        k = 0
        i = 0
        while i < env.nveh and k < kmax:
            x = env.vx[i]
            dx, dy = x - ex, -1.6 - ey
            if math.sqrt(dx * dx + dy * dy) < c.sensor_radius:
                ox[e, k], ov[e, k] = x, env.vv[i]
                if with_acc:
                    oa[e, k] = env.va[i]
                k += 1
            i += 1
        k_count[e] = k                                        # (the rows are zero beyond k)
    return {"ego5": ego5, "k": k_count, "ox": ox, "ov": ov, "oa": oa}


def read(state):
    """What ``stmpc_sim_read`` returns: status [n] int32, ticks [n] int32, acc [n][12], ego4 [n][4]."""
    return (np.array([env.status for env in state.envs], dtype=np.int32), np.array([env.ticks for env in state.envs], dtype=np.int32),
            np.array([env.acc for env in state.envs], dtype=np.float64).reshape(state.n, NACC),
            np.array([env.ego4 for env in state.envs], dtype=np.float64).reshape(state.n, 4))


def step_env(c, p_a_min, p_a_max, p_v_max, state, e, cmd, crash_min_s):
    """One tick of environment ``e`` with the commanded ego speed ``cmd`` (``sim_step_body``)."""
    env = state.envs[e]
    if env.status != 0:
        return
    cnt = state.counts
    dt = c.tick_length
    cx, cy, v_prev = env.ego4[0], env.ego4[1], env.ego4[2]
    sel = float(cmd)
    if not (sel == sel):
        sel = v_prev
        cnt["nan_command"][e] += 1
    hi, lo = v_prev + p_a_max * dt, v_prev + p_a_min * dt
    if sel > hi:
        sel = hi
        cnt["clamp_a_max"][e] += 1
    elif sel < lo:
        sel = lo
        cnt["clamp_a_min"][e] += 1
    if sel < 0:
        sel = 0.0
        cnt["clamp_zero"][e] += 1
    elif sel > p_v_max:
        sel = p_v_max
        cnt["clamp_v_max"][e] += 1
    # ego motion along its route, or along the straight lines the planner assumes
    RX, RY = c.route_x, c.route_y
    if RX is not None and cx < RX[-1]:
        rn = len(RX)
        i = 0
        while i + 2 < rn and RX[i + 1] <= cx:
            i += 1
        left = sel * dt
        px, py = cx, cy
        while left > 0.0 and i + 1 < rn:
            ex, ey = RX[i + 1] - px, RY[i + 1] - py
            seg = math.sqrt(fma(ey, ey, ex * ex))
            if left < seg:
                px += ex / seg * left
                py += ey / seg * left
                left = 0.0
                break
            left -= seg
            px, py = RX[i + 1], RY[i + 1]
            i += 1
            cnt["route_vertex"][e] += 1
        if left > 0.0:
            cnt["route_end_crossed"][e] += 1
        px += left
    elif RX is not None:
        py = cy
        px = cx + sel * dt
        cnt["past_route_end"][e] += 1
    elif cx < 1.5:
        d0, d1 = 1.5 - cx, -1.5 - cy
        nrm = math.sqrt(fma(d1, d1, d0 * d0))
        d0 /= nrm
        d1 /= nrm
        px = cx + d0 * (sel * dt)
        py = cy + d1 * (sel * dt)
        cnt["straight_approach"][e] += 1
        if py < -1.6:
            py = -1.6
            cnt["straight_y_floor"][e] += 1
    else:
        py = cy
        px = cx + sel * dt
        cnt["straight_beyond"][e] += 1
    acc_ego = (sel - v_prev) / dt
    es = ego_s(px, py)
    # highway vehicles (Krauss, front to back), every one planning on the positions at the start of the step
    ego_on_lane = cx >= -50.58
    ego_pos0 = cx
    n = env.nveh
    lead_x, lead_v = INF, 0.0
    crashed = False
    gap_ahead, gap_behind = 100.0, 100.0
    behind_acc, have_behind = 0.0, False
    ego_pos1 = px
    lat = 3.31 * (1.5 - px) / 52.08 if px < 1.5 else 0.0
    vx, vv, va, vcd = env.vx, env.vv, env.va, env.vc
    for i in range(n):
        ox_, ov_ = vx[i], vv[i]
        vnext = ov_ + c.veh_accel * dt
        vdes = vcd[i]
        vnext = vnext if vnext < vdes else vdes
        if lead_x < INF:
            vs = krauss_follow(c, lead_x - c.veh_length - ox_ - c.veh_min_gap, lead_v)
            if vs < vnext:
                vnext = vs
                cnt["follow_binding"][e] += 1
        if ego_on_lane:
            g_net = ego_pos0 - c.veh_length - ox_ - c.veh_min_gap
            vs = INF
            if g_net >= 0.0:
                vs = krauss_follow(c, g_net, v_prev)
                cnt["ego_leader_follow"][e] += 1
                if vs < vnext:
                    cnt["ego_leader_binding"][e] += 1
            elif ego_pos0 > ox_:
                vs = 0.0
                cnt["lap_in_stop"][e] += 1
            vnext = vs if vs < vnext else vnext
        vmin = ov_ - c.veh_emergency_decel * dt
        if vnext < vmin:
            vnext = vmin
            cnt["emergency_floor"][e] += 1
        vnext = 0.0 if vnext < 0.0 else vnext
        nx = ox_ + vnext * dt
        lead_x, lead_v = ox_, ov_
        vx[i], vv[i], va[i] = nx, vnext, (vnext - ov_) / dt
        if px >= -50.58 and lat < c.veh_width and abs(nx - ego_pos1) < c.veh_length:
            crashed = True
        d = abs(nx - px)
        if nx >= px:
            gap_ahead = d if d < gap_ahead else gap_ahead
        else:
            gap_behind = d if d < gap_behind else gap_behind
        if not have_behind and nx < px:
            have_behind = True
            ddx, ddy = nx - px, -1.6 - py
            behind_acc = (vnext - ov_) / dt if math.sqrt(ddx * ddx + ddy * ddy) < c.sensor_radius else 0.0
    gap = gap_ahead if gap_ahead < gap_behind else gap_behind
    # vehicles leaving at the end of the highway (front of the list) and entering at its start
    nn, drop = n, 0
    while drop < nn and vx[drop] > c.despawn_x:
        drop += 1
    if drop:
        for i in range(drop, nn):
            vx[i - drop], vv[i - drop], va[i - drop], vcd[i - drop] = vx[i], vv[i], va[i], vcd[i]
        nn -= drop
        cnt["despawn"][e] += 1
    delay = env.delay
    ctr = env.rng
    if delay <= 0:
        was_postponed, state._postponed[e] = state._postponed[e], False
        room = nn < KS
        if not room:
            cnt["insertion_no_slot"][e] += 1
        if room and nn > 0:
            room = krauss_follow(c, vx[nn - 1] - c.veh_length - c.spawn_x - c.veh_min_gap, vv[nn - 1]) >= c.other_car_speed
            if not room:
                cnt["insertion_postponed"][e] += 1
                state._postponed[e] = True
        if room:
            vc_ = c.other_car_speed
            vx[nn], vv[nn], va[nn], vcd[nn] = c.spawn_x, (vc_ if vc_ < c.other_car_speed else c.other_car_speed), 0.0, vc_
            nn += 1
            if c.vary_traffic_start_times:
                delay = uniform01(c.seed, e, ctr) + c.base_traffic_interval
                ctr = (ctr + 1) & _M32
            else:
                delay = 0.0 + c.base_traffic_interval
            cnt["insertion"][e] += 1
            if was_postponed:
                cnt["insertion_after_postponed"][e] += 1
    delay -= dt
    env.delay, env.rng, env.nveh = delay, ctr, nn
    env.ego4 = [px, py, sel, acc_ego]
    a = env.acc
    tk = env.ticks
    a[0] += sel
    a[1] = sel if sel > a[1] else a[1]
    if tk > 0:
        a[2] += abs((acc_ego - a[3]) / dt)
    a[3] = acc_ego
    a[4] += 1.0
    if es > crash_min_s:
        a[5] = gap if gap < a[5] else a[5]
        a[6] += gap
        a[7] += 1.0
        cnt["gap_sample"][e] += 1
    if es > c.disruption_min_s:
        dis = -behind_acc if behind_acc < 0.0 else 0.0
        a[8] += dis
        a[9] = dis if dis > a[9] else a[9]
        a[10] += 1.0
        if dis != 0.0:
            a[11] += 1.0
            cnt["disruption_nonzero"][e] += 1
    env.ticks = tk + 1
    if px >= c.arrive_x:
        env.status = 1
        cnt["status_1"][e] += 1
    elif crashed:
        env.status = 2
        cnt["status_2"][e] += 1
    elif tk + 1 >= c.max_ticks:
        env.status = 3
        cnt["status_3"][e] += 1


def step(state, params, cfg, cmd, crash_min_s):
    """``k_sim_step``: one tick of every running environment with the commanded ego speeds ``cmd`` [n]; finished environments idle.  The draws of
    the tick are the cfg's seed's whatever seed the state was initialised from (as the vector env's autoreset has it)."""
    c = as_cfg(cfg)
    a_min, a_max, v_max = float(_get(params, "a_min")), float(_get(params, "a_max")), float(_get(params, "v_max"))
    crash_min_s = float(crash_min_s)
    for e in range(state.n):
        step_env(c, a_min, a_max, v_max, state, e, cmd[e], crash_min_s)
