"""The first-step shield on grouped and mixed-traffic vector envs, host side (vec_env.GroupedShieldVecEnv; the stmpc_shield_traffic_groups_*,
stmpc_shield_reward_groups_* and stmpc_shield_traffic_mix_* entries of include/stmpc.h).  No GPU: the header against the binding, the cfg tables, and
every refusal that must come before a device call."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import REPO
from stmpc_testlib import capi as _capi

# entry -> its number of arguments
ENTRIES = {"stmpc_shield_traffic_groups_env_reset_device": 12, "stmpc_shield_traffic_groups_env_step_device": 19,
           "stmpc_shield_reward_groups_env_reset_device": 14, "stmpc_shield_reward_groups_env_step_device": 19,
           "stmpc_shield_traffic_mix_env_reset_device": 13, "stmpc_shield_traffic_mix_env_step_device": 21}
METHODS = {"shield_env_step_groups": "stmpc_shield_traffic_groups_env_step_device",
           "shield_env_step_reward_groups": "stmpc_shield_reward_groups_env_step_device", "shield_traffic_mix_env_step": "stmpc_shield_traffic_mix_env_step_device"}


def test_header_declares_the_entries_and_the_abi_stays():
    capi = _capi()
    header = " ".join(open(os.path.join(REPO, "include", "stmpc.h")).read().split())
    declared = {name: args for name, args in re.findall(r"\bint (stmpc_shield_(?:traffic_groups|reward_groups|traffic_mix)_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(declared) == set(ENTRIES) <= set(capi.EXPORTS)
    lib = capi.load()
    for name, n_args in ENTRIES.items():
        assert len(declared[name].split(",")) == n_args == len(getattr(lib, name).argtypes), name
    # additive: no struct of its own (the entries take stmpc_shield_env_cfg, whose layout stays) and the ABI version stays
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8 and "#define STMPC_ABI_VERSION 8 " in header
    assert ctypes.sizeof(capi.ShieldEnvCfg) == ctypes.sizeof(capi.FirstStepCfg) + 16 == 40
    assert [getattr(capi.ShieldEnvCfg, n).offset for n, _ in capi.ShieldEnvCfg._fields_] == [0, 24, 32, 36]
    # a step entry's tail is the lone shielded step's: the same pointer types after N
    lone = lib.stmpc_shield_env_step_device.argtypes
    for name in ("stmpc_shield_traffic_groups_env_step_device", "stmpc_shield_reward_groups_env_step_device"):
        assert list(getattr(lib, name).argtypes[4:]) == list(lone[5:]), name
    assert list(lib.stmpc_shield_traffic_mix_env_step_device.argtypes[4:-3]) == list(lone[5:-1])


def test_context_methods_take_the_entries_arguments():
    capi = _capi()
    for method, entry in METHODS.items():        # (self + the entry's arguments but the context)
        assert len(inspect.signature(getattr(capi.Context, method)).parameters) == ENTRIES[entry], method
    # the resets: a table brings its length (G, R, T) and the penalties theirs (P)
    assert len(inspect.signature(capi.Context.shield_env_reset_groups).parameters) == ENTRIES["stmpc_shield_traffic_groups_env_reset_device"] - 2
    assert len(inspect.signature(capi.Context.shield_env_reset_reward_groups).parameters) == ENTRIES["stmpc_shield_reward_groups_env_reset_device"] - 3
    assert len(inspect.signature(capi.Context.shield_traffic_mix_env_reset).parameters) == ENTRIES["stmpc_shield_traffic_mix_env_reset_device"] - 1


def test_constructor_validation_comes_before_any_device_call(restore_settings):
    _capi()
    import numpy as np
    from rl_mpc_lanemerging_amd import vec_env
    E = vec_env.GroupedShieldVecEnv
    two = [{"REWARD_FUNCTION": "ST"}, {"REWARD_FUNCTION": "Slotted"}]
    with pytest.raises(ValueError, match="needs traffic groups, reward groups or a traffic_mix"):
        E(4)
    # group counts
    with pytest.raises(ValueError):
        E(4, traffic=["default", "low", "fast"])                    # 4 environments do not split into 3 groups
    with pytest.raises(ValueError):
        E(4, traffic=[])
    with pytest.raises(ValueError, match="reward groups"):
        E(5, rewards=two)
    with pytest.raises(ValueError, match="unknown traffic type"):
        E(4, traffic=["default", "rush hour"])
    with pytest.raises(ValueError, match="must coincide"):          # R != G
        E(12, traffic=["default", "low", "fast"], rewards=two)
    # the length and the values of takeover_penalty
    for bad in ((0.0, 0.1, 0.2), (0.0, 0.1, 0.2, 0.3, 0.4), ()):
        with pytest.raises(ValueError, match="takeover_penalty has"):
            E(4, traffic=["default", "low"], takeover_penalty=bad)
    with pytest.raises(ValueError, match="takeover_penalty has"):
        E(4, rewards=two, takeover_penalty=(0.0, 0.1, 0.2))
    with pytest.raises(ValueError, match="takeover_penalty has"):   # (the mix has no groups: one number)
        E(4, traffic_mix=["default", "low"], takeover_penalty=(0.0, 0.1))
    for bad in (-0.1, float("inf"), float("nan"), (0.0, -1.0), (0.0, float("nan")), np.float32(-1)):
        with pytest.raises(ValueError, match="finite and not negative"):
            E(4, traffic=["default", "low"], takeover_penalty=bad)
    with pytest.raises(ValueError, match="takeover_penalty"):
        E(4, traffic=["default", "low"], takeover_penalty="much")
    for bad in (0, -1, 33, 64):
        with pytest.raises(ValueError, match="shield_kmax"):
            E(4, traffic=["default", "low"], shield_kmax=bad)
    # mix arguments
    with pytest.raises(ValueError, match="belong to a traffic_mix"):
        E(4, traffic=["default", "low"], mix_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="belong to a traffic_mix"):
        E(4, rewards=two, mix_seed=3)
    with pytest.raises(ValueError, match="out of scope"):           # (the mix goes with neither kind of groups)
        E(4, traffic=["default", "low"], traffic_mix=["default", "low"])
    with pytest.raises(ValueError, match="out of scope"):
        E(4, rewards=two, traffic_mix=["default", "low"])
    with pytest.raises(ValueError, match="mix_weights has"):
        E(4, traffic_mix=["default", "low"], mix_weights=[1.0])
    with pytest.raises(ValueError, match="mix_weights"):
        E(4, traffic_mix=["default", "low"], mix_weights=[1.0, -1.0])
    with pytest.raises(ValueError, match="must not set its own"):
        E(4, traffic_mix=["default", {"BASE_TRAFFIC_INTERVAL": 2.0, "OTHER_CAR_SPEED": 7.0, "seed": 3}])
    with pytest.raises(ValueError, match="Invalid gym environment"):
        E(4, env_id="sumo-v9", traffic=["default", "low"])


def test_merge_vec_env_still_refuses_these_combinations(restore_settings):
    _capi()
    from rl_mpc_lanemerging_amd import vec_env
    E = vec_env.MergeVecEnv
    with pytest.raises(ValueError, match="a shielded env with traffic or reward groups is out of scope"):
        E(4, shield="first_step", traffic=["default", "low"])
    with pytest.raises(ValueError, match="a shielded env with traffic or reward groups is out of scope"):
        E(4, shield="first_step", rewards=[{"REWARD_FUNCTION": "ST"}, {"REWARD_FUNCTION": "Slotted"}])
    with pytest.raises(ValueError, match="a traffic mix with traffic groups, reward groups or a shield is out of scope"):
        E(4, shield="first_step", traffic_mix=["default", "low"])
    with pytest.raises(ValueError, match="a traffic mix with traffic groups, reward groups or a shield is out of scope"):
        vec_env.TrafficMixVecEnv(4, shield="first_step", traffic_mix=["default", "low"])
    assert issubclass(vec_env.GroupedShieldVecEnv, E) and vec_env.GroupedShieldVecEnv is not E
    p = inspect.signature(vec_env.GroupedShieldVecEnv.__init__).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:8]] == [("n", inspect.Parameter.empty), ("env_id", None), ("seed", 0), ("reward", None), ("autoreset", True),
                                                                 ("ctx", None), ("log_capacity", 0)]
    assert {k: v.default for k, v in list(p.items())[8:]} == {"traffic": None, "rewards": None, "traffic_mix": None, "mix_weights": None, "mix_seed": None,
                                                              "shield_sparse": False, "takeover_penalty": 0.0, "shield_kmax": 32}
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for v in list(p.values())[8:])


def test_the_cfg_tables_are_the_unshielded_envs(restore_settings):
    """The class hands the shield entries the tables its unshielded twins hand theirs: group g's sim cfg, reward cfg and the mix's cumulative weights."""
    capi = _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import episodes, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    S = pkg.Settings
    traffic = ["low", dict(episodes.TRAFFIC_TYPES["fast"], seed=99)]
    t = episodes.sim_cfgs(traffic, 7, float(S.MAX_EPISODE_LENGTH))
    assert len(t) == 2 and (t[0].base_traffic_interval, t[1].other_car_speed) == (2.4, 15.0)
    assert (t[0].seed, t[1].seed) == (7, 99) and t[0].sensor_radius == t[1].sensor_radius
    r = vec_env.reward_cfgs([{"REWARD_FUNCTION": "Continuous"}, {"REWARD_FUNCTION": "ST", "INVALID_ACTION_PENALTY": -1.5}], "sumo-jerk-continuous-v0")
    assert len(r) == 2 and (r[0].reward_function, r[1].reward_function) == (capi.REWARD_CONTINUOUS, capi.REWARD_ST)
    assert r[1].invalid_action_penalty == -1.5 and r[0].invalid_action_penalty == float(S.INVALID_ACTION_PENALTY)
    m = episodes.traffic_mix_cfgs(["low", "fast"], 7, float(S.MAX_EPISODE_LENGTH))
    assert (m[0].seed, m[1].seed) == (7, 7) and vec_env.traffic_mix_cum([1.0, 3.0]) == [0.25, 1.0]
    c = capi.ShieldEnvCfg.from_settings(S, False, 0.5, 16)
    assert (c.takeover_penalty, c.kmax, c.fs.sparse_control) == (0.5, 16, 0)
    ptr, P, keep = capi.Context._penalties((0.0, 0.5))
    assert P == 2 and list(keep) == [0.0, 0.5] and capi.Context._penalties(None)[:2] == (None, 0)
