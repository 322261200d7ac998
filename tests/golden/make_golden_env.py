#!/usr/bin/env python3
"""Golden vectors for the vector environment (rl-mpc-lanemerging_amd/vec_env.py, csrc/stmpc_env_kernels.hpp): the reference's own reward
functions and gym action handling, run on recorded inputs.

Build-container only (needs the reference checkout).  What runs is the reference's code, unmodified:
  (a) dqn.continuous_reward, rl.slotted_reward, dqn.slotted_reward_with_jerk, dqn.st_reward (dqn.py:449-563, rl.py:168-174) on ~2000
      prediction.HighwayState's -- no car ahead, no car behind, ego_s <= 0, a gap below MIN_FOLLOW_DISTANCE, crash and arrival included --
      under the reference's defaults and under configs/train_moderate_1.json;
  (b) merge_gym.ContinuousJerkEnv / JerkEnv / AccelerationEnv._do_action (merge_gym.py:83-100, 193-227) over (speed, acceleration, previous
      acceleration, action) tuples that reach every penalty and clamp branch, with INVALID_ACTION_PENALTY = -1.  The env objects are made
      without __init__ (it starts SUMO); control.set_ego_jerk / set_ego_speed are recorders (the TraCI side effect), the former through the
      reference's control.get_ego_speed_from_jerk on the world's speed and acceleration.
``gym`` is absent: a minimal stand-in (Env, spaces.Box / Discrete, envs.register) lets merge_gym.py import.
Inputs are Python floats, as TraCI returns them (so ``x ** 2`` is the libm pow call the reference makes).
Re-run:  python tests/golden/make_golden_env.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import import_reference, REF      # noqa: E402

REWARDS = ("Continuous", "Slotted", "Slotted Jerk", "ST")
ENVS = ("sumo-jerk-continuous-v0", "sumo-jerk-v0", "sumo-accel-v0")
WEIGHT_KEYS = ("TICK_LENGTH", "CRASH_REWARD", "SUCCESS_REWARD", "TIME_REWARD", "WT_SMOOTH", "WT_SAFE", "WT_EFFICIENT", "ALT_V_WEIGHT", "ALT_A_WEIGHT",
               "ALT_J_WEIGHT", "ALT_D_WEIGHT", "MIN_FOLLOW_DISTANCE", "DESIRED_SPEED", "CAR_LENGTH")
ACTION_KEYS = ("TICK_LENGTH", "INVALID_ACTION_PENALTY", "MINIMUM_NEGATIVE_JERK", "MAXIMUM_POSITIVE_JERK", "MAX_NEGATIVE_ACCELERATION",
               "MAX_POSITIVE_ACCELERATION", "MAX_SPEED")


def gym_stand_in():
    gym = types.ModuleType("gym")
    spaces = types.ModuleType("gym.spaces")

    class Env:
        def __init__(self, *a, **kw):
            pass

    class Box:
        def __init__(self, low, high, shape=None):
            self.low, self.high, self.shape = low, high, shape

    class Discrete:
        def __init__(self, n):
            self.n = n

    spaces.Box, spaces.Discrete = Box, Discrete
    gym.Env, gym.spaces = Env, spaces
    gym.envs = types.SimpleNamespace(register=lambda **kw: None)
    sys.modules["gym"] = gym
    sys.modules["gym.spaces"] = spaces


def q(x, scale):
    return np.round(np.asarray(x) * scale) / scale if np.ndim(x) else float(round(x * scale) / scale)


def make_states(n, rng, synth, kmax):
    ego = np.zeros((n, 4))
    k = np.zeros(n, np.int32)
    ox, ov, oa = np.zeros((n, kmax)), np.zeros((n, kmax)), np.zeros((n, kmax))
    crashed, arrived = np.zeros(n, np.int32), np.zeros(n, np.int32)
    jerk = np.zeros(n)
    for i in range(n):
        x = rng.uniform(-200.0, 60.0) if i % 4 else rng.uniform(-48.0, 40.0)      # a quarter in the merge zone (ego_s > 0)
        x = q(x, 256)                                         # (inputs on coarse binary grids: the file stays small, the arithmetic is the same)
        ego[i] = (x, float(synth.road_y(np.array([x]))[0]), q(rng.uniform(0.0, 30.0), 1024), q(rng.uniform(-6.0, 4.5), 1024))
        kind = i % 10
        kk = int(rng.integers(0, kmax + 1))
        xs = np.sort(q(rng.uniform(x - 120.0, x + 120.0, kk), 256))[::-1]
        if kind == 1:
            xs = xs[xs < x]                                   # no car ahead
        elif kind == 2:
            xs = xs[xs >= x]                                  # no car behind
        elif kind == 3 and kk:
            xs[len(xs) // 2] = x + q(rng.uniform(-1.0, 1.0) * 7.5, 256)     # a gap below MIN_FOLLOW_DISTANCE (either side)
            xs = np.sort(xs)[::-1]
        elif kind == 4:
            xs = xs[:0]                                       # nobody within the sensor radius
        kk = len(xs)
        k[i] = kk
        ox[i, :kk] = xs
        ov[i, :kk] = q(rng.uniform(0.0, 15.0, kk), 64)
        oa[i, :kk] = np.where(rng.random(kk) < 0.6, 0.0, q(rng.uniform(-9.0, 2.6, kk), 64))
        jerk[i] = q(rng.normal(0.0, 4.0) if i % 7 else rng.uniform(-60.0, 60.0), 65536)
        u = rng.random()
        crashed[i] = u < 0.04
        arrived[i] = 0.04 <= u < 0.08
    return ego, k, ox, ov, oa, jerk, crashed, arrived


def main():
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    gym_stand_in()
    S, control, prediction, st, st_cy = import_reference()
    import dqn                     # noqa: E402  (the reference's)
    import rl                      # noqa: E402
    import merge_gym               # noqa: E402
    from rl_mpc_lanemerging_amd import synth

    defaults = {k_: getattr(S, k_) for k_ in set(WEIGHT_KEYS) | set(ACTION_KEYS)}
    rng = np.random.default_rng(2024)
    n, kmax = 2000, 8
    ego, k, ox, ov, oa, jerk, crashed, arrived = make_states(n, rng, synth, kmax)
    fns = {"Continuous": dqn.continuous_reward, "Slotted": rl.slotted_reward, "Slotted Jerk": dqn.slotted_reward_with_jerk, "ST": dqn.st_reward}
    rewards = np.zeros((2, len(REWARDS), n))
    weights = np.zeros((2, len(WEIGHT_KEYS)))
    for w in range(2):
        for k_, v_ in defaults.items():
            setattr(S, k_, v_)
        if w == 1:
            S.load_from_file(os.path.join(REF, "configs", "train_moderate_1.json"))
            assert S.REWARD_FUNCTION == "Slotted Jerk"
        weights[w] = [float(getattr(S, q)) for q in WEIGHT_KEYS]
        for r, name in enumerate(REWARDS):
            S.REWARD_FUNCTION = name
            assert dqn.get_reward_function() is fns[name]
            for i in range(n):
                kk = int(k[i])
                if crashed[i] or arrived[i]:
                    state = prediction.HighwayState.empty_state()            # merge_gym.py:108,113
                else:
                    state = prediction.HighwayState((float(ego[i, 0]), float(ego[i, 1])), float(ego[i, 2]), float(ego[i, 3]),
                                                    [float(x) for x in ox[i, :kk]], [float(x) for x in ov[i, :kk]], [float(x) for x in oa[i, :kk]])
                rewards[w, r, i] = float(fns[name](state, float(jerk[i]), bool(crashed[i]), bool(arrived[i])))
    for k_, v_ in defaults.items():
        setattr(S, k_, v_)

    # (b) action handling
    S.INVALID_ACTION_PENALTY = -1.0
    rec = {}
    control.set_ego_jerk = lambda j: rec.__setitem__("cmd", control.get_ego_speed_from_jerk(rec["v"], rec["a"], j))
    control.set_ego_speed = lambda v: rec.__setitem__("cmd", v)
    m = 600
    act_in = np.zeros((len(ENVS), m, 4))           # speed, acceleration (the world's), previous_acceleration, action (jerk or index)
    act_out = np.zeros((len(ENVS), m, 3))          # command, projected jerk, invalid-action reward
    for ei, env_id in enumerate(ENVS):
        cls = {"sumo-jerk-continuous-v0": merge_gym.ContinuousJerkEnv, "sumo-jerk-v0": merge_gym.JerkEnv, "sumo-accel-v0": merge_gym.AccelerationEnv}[env_id]
        env = cls.__new__(cls)
        env.penalty_for_invalid_action = S.INVALID_ACTION_PENALTY
        nact = len(S.ACCELERATION_VALUES_DQN if env_id == "sumo-accel-v0" else S.JERK_VALUES_DQN)
        for i in range(m):
            b = i % 6
            v = q(rng.uniform(0.0, 30.0) if b < 3 else (rng.uniform(0.0, 1.2) if b == 3 else rng.uniform(28.8, 30.0)), 1024)
            pa = q(rng.uniform(-6.0, 4.5), 1024) if b != 4 else float(rng.choice([-6.0, 4.5, -5.75, 4.25]))
            a = pa if i % 3 else q(rng.uniform(-6.0, 4.5), 1024)
            action = q(rng.uniform(-12.0, 12.0), 4096) if env_id == "sumo-jerk-continuous-v0" else int(rng.integers(0, nact))
            env.previous_acceleration = float(pa)
            env.previous_state = prediction.HighwayState((0.0, 0.0), float(v), float(a), [], [], [])
            rec.clear()
            rec["v"], rec["a"] = float(v), float(a)
            env._do_action(action)
            act_in[ei, i] = (v, a, pa, action)
            act_out[ei, i] = (float(rec["cmd"]), float(env.projected_jerk), float(env.invalid_action_reward))
    # (other_v / other_a: no reward reads them; other_x, and every action input, is exact in float32 on the grids above)
    # rewards are stored [function][weight set][state] (equal rows next to each other compress)
    assert np.array_equal(jerk.astype(np.float32).astype(np.float64), jerk)
    assert np.array_equal(ox.astype(np.float32).astype(np.float64), ox) and np.array_equal(act_in.astype(np.float32).astype(np.float64), act_in)
    np.savez_compressed(os.path.join(HERE, "golden_env.npz"), ego4=ego, k_count=k.astype(np.int8), other_x=ox.astype(np.float32),
                        crashed=crashed.astype(np.int8), arrived=arrived.astype(np.int8), jerk=jerk.astype(np.float32),
                        rewards=np.ascontiguousarray(rewards.transpose(1, 0, 2)), reward_names=np.array(REWARDS), weight_keys=np.array(WEIGHT_KEYS), weights=weights,
                        env_ids=np.array(ENVS), act_in=act_in.astype(np.float32), act_out=act_out, action_keys=np.array(ACTION_KEYS),
                        action_vals=np.array([float(getattr(S, q)) for q in ACTION_KEYS]),
                        jerk_values=np.array([float(S.JERK_VALUES_DQN[i]) for i in range(len(S.JERK_VALUES_DQN))]),
                        acceleration_values=np.array([float(S.ACCELERATION_VALUES_DQN[i]) for i in range(len(S.ACCELERATION_VALUES_DQN))]))
    print("golden_env.npz:", os.path.getsize(os.path.join(HERE, "golden_env.npz")), "bytes")


if __name__ == "__main__":
    main()
