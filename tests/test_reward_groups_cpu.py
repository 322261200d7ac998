"""Reward groups, host side (vec_env.reward_cfgs, the ``rewards`` argument of MergeVecEnv, the stmpc_reward_groups_* entries of include/stmpc.h).
No GPU: ``reward_cfgs`` fills what a group does not set from the Settings and leaves them alone, refuses unknown keys and names, keeps the
must-be-equal fields equal, the table has the header's layout, and header / library / binding agree on the new entries.
"""
import ctypes
import os
import re

import pytest

from conftest import REPO
from stmpc_testlib import pkg as _pkg

MAY_DIFFER = ("reward_function", "crash_reward", "success_reward", "time_reward", "wt_smooth", "wt_safe", "wt_efficient", "alt_v_weight", "alt_a_weight",
              "alt_j_weight", "alt_d_weight", "min_follow_distance", "desired_speed", "invalid_action_penalty")
MUST_BE_EQUAL = ("action_mode", "tick_length", "car_length", "minimum_negative_jerk", "maximum_positive_jerk", "max_negative_acceleration",
                 "max_positive_acceleration", "max_speed", "n_action_values", "autoreset", "log_capacity")
ENTRIES = {"stmpc_reward_groups_env_reset_device": 11, "stmpc_reward_groups_env_step_device": 13, "stmpc_reward_groups_env_reward_device": 14,
           "stmpc_reward_groups_split": 3}


class _NoDevice:
    """A context that must not be asked for anything."""

    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


def test_reward_cfgs_fills_defaults_from_settings_and_leaves_them_alone(restore_settings):
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides({"WT_SAFE": 0.25, "INVALID_ACTION_PENALTY": -2.0})
    before = pkg.Settings.snapshot()
    groups = [{}, {"REWARD_FUNCTION": "Slotted Jerk", "ALT_J_WEIGHT": 0.1}, {"REWARD_FUNCTION": "ST", "DESIRED_SPEED": 20, "INVALID_ACTION_PENALTY": -1}]
    table = vec_env.reward_cfgs(groups, env_id="sumo-jerk-v0", autoreset=False, log_capacity=77)
    assert pkg.Settings.snapshot() == before
    assert isinstance(table, capi.EnvCfgTable) and len(table) == 3
    plain = vec_env.env_cfg("sumo-jerk-v0", None, False, pkg.Settings, 77)
    want = [{}, {"reward_function": capi.REWARD_SLOTTED_JERK, "alt_j_weight": 0.1},
            {"reward_function": capi.REWARD_ST, "desired_speed": 20.0, "invalid_action_penalty": -1.0}]
    for r in range(3):
        for c in (table[r], table.array[r]):                           # the caller's object and the row the library reads
            for name, _ in capi.EnvCfg._fields_:
                if name in ("action_values", "features", "reserved0"):
                    continue
                assert getattr(c, name) == want[r].get(name, getattr(plain, name)), (r, name)
            assert [c.action_values[i] for i in range(c.n_action_values)] == [-5, -2.5, 0, 2.5, 5]
            assert c.features.contents.time_feature == 0 and c.features.contents.cars_ahead == pkg.Settings.CARS_AHEAD
    assert table[0].wt_safe == 0.25 and table[0].invalid_action_penalty == -2.0 and table[0].reward_function == capi.REWARD_CONTINUOUS
    # another Settings class as S: read, not written
    S2 = vec_env.reward_settings({"TIME_REWARD": -0.5, "REWARD_FUNCTION": "Slotted"})
    assert S2.TIME_REWARD == -0.5 and S2.WT_SAFE == 0.25 and pkg.Settings.TIME_REWARD == -0.1
    t2 = vec_env.reward_cfgs([{}, {"TIME_REWARD": -1}], S=S2)
    assert (t2[0].time_reward, t2[1].time_reward) == (-0.5, -1.0) and t2[0].reward_function == capi.REWARD_SLOTTED
    assert pkg.Settings.snapshot() == before


def test_reward_cfgs_rejects_unknown_keys_and_names(restore_settings):
    _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, vec_env
    with pytest.raises(ValueError, match="may set REWARD_FUNCTION, .*, not TICK_LENGTH"):
        vec_env.reward_cfgs([{}, {"TICK_LENGTH": 0.1}])
    with pytest.raises(ValueError, match="not MAX_SPEED, reward"):
        vec_env.reward_cfgs([{"MAX_SPEED": 20, "reward": "ST"}])
    with pytest.raises(ValueError, match="Invalid reward function Sparse specified in settings"):
        vec_env.reward_cfgs([{"REWARD_FUNCTION": "Sparse"}])
    with pytest.raises(ValueError, match="Invalid gym environment"):
        vec_env.reward_cfgs([{}], env_id="sumo-v0")
    with pytest.raises(ValueError, match="1 ... 64 groups, not 0"):
        vec_env.reward_cfgs([])
    with pytest.raises(ValueError, match="1 ... 64 groups, not 65"):
        vec_env.reward_cfgs([{}] * (capi.ENV_REWARD_GROUPS_MAX + 1))
    with pytest.raises(ValueError, match="a dict of settings"):
        vec_env.reward_cfgs(["ST"])


def test_reward_cfgs_keeps_the_must_be_equal_fields_equal(restore_settings):
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, vec_env
    every = dict(REWARD_FUNCTION="ST", **{k: -1.5 - i for i, k in enumerate(vec_env.REWARD_GROUP_KEYS)})
    assert {"REWARD_FUNCTION", *vec_env.REWARD_GROUP_KEYS} == set(every) and set(vec_env.REWARD_GROUP_KEYS.values()) | {"reward_function"} == set(MAY_DIFFER)
    for env_id in vec_env.ENV_IDS:
        table = vec_env.reward_cfgs([{}, every, {"REWARD_FUNCTION": "Slotted"}], env_id=env_id, log_capacity=5)
        for r in (1, 2):
            for name in MUST_BE_EQUAL:
                assert getattr(table[r], name) == getattr(table[0], name), (env_id, r, name)
            n = table[0].n_action_values
            assert [table[r].action_values[i] for i in range(n)] == [table[0].action_values[i] for i in range(n)]
            assert bytes(table[r].features.contents) == bytes(table[0].features.contents)
        for name in MAY_DIFFER:
            assert getattr(table[1], name) != getattr(table[0], name), name
    # every field of the struct is on exactly one of the two lists (the table, reserved0 and the observation apart)
    fields = {n for n, _ in capi.EnvCfg._fields_}
    assert fields == set(MAY_DIFFER) | set(MUST_BE_EQUAL) | {"action_values", "features", "reserved0"} and not set(MAY_DIFFER) & set(MUST_BE_EQUAL)


def test_the_table_has_the_headers_layout():
    _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, vec_env
    header = open(os.path.join(REPO, "include", "stmpc.h")).read()
    body = re.search(r"typedef struct stmpc_env_cfg \{(.*?)\} stmpc_env_cfg;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [first.split()[-1].lstrip("*")] + [x.strip().lstrip("*") for x in rest]
    assert names == [n for n, _ in capi.EnvCfg._fields_]
    # a table is R structs back to back, each a bytewise copy of the caller's
    table = vec_env.reward_cfgs([{"WT_SAFE": 1.0 + r} for r in range(3)])
    size = ctypes.sizeof(capi.EnvCfg)
    assert size % 8 == 0 and ctypes.sizeof(table.array) == 3 * size
    for r in range(3):
        assert bytes(table.array)[r * size:(r + 1) * size] == bytes(table[r]) and table.array[r].wt_safe == 1.0 + r
    assert ctypes.addressof(table.array[2]) - ctypes.addressof(table.array[0]) == 2 * size


def test_header_library_and_binding_agree_on_the_reward_group_entries():
    _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi
    lib = capi.load()
    header = " ".join(open(os.path.join(REPO, "include", "stmpc.h")).read().split())
    declared = {name: args for name, args in re.findall(r"\bint (stmpc_reward_groups_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(declared) == set(ENTRIES) <= set(capi.EXPORTS)
    for name, args in declared.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")) == ENTRIES[name], name
        # each entry cites the reference it restates
        assert re.search(re.escape(name) + r" \(dqn\.py:449-563, rl\.py:168-174, merge_gym\.py:25,83-140\)", header), name
    assert "#define STMPC_ENV_REWARD_GROUPS_MAX %d" % capi.ENV_REWARD_GROUPS_MAX in header and capi.ENV_REWARD_GROUPS_MAX == 64
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8 and "#define STMPC_ABI_VERSION 8" in header
    for field in MAY_DIFFER + MUST_BE_EQUAL:
        assert field in header[header.index("Reward groups:"):], field


def test_mismatched_shapes_are_refused_before_any_context(restore_settings):
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    three = [{}, {"REWARD_FUNCTION": "ST"}, {"REWARD_FUNCTION": "Slotted"}]
    with pytest.raises(ValueError, match="do not divide into 3 reward groups"):
        vec_env.MergeVecEnv(64, env_id="sumo-jerk-continuous-v0", ctx=_NoDevice(), rewards=three)
    with pytest.raises(ValueError, match="2 traffic groups and 3 reward groups"):
        vec_env.MergeVecEnv(12, env_id="sumo-jerk-continuous-v0", ctx=_NoDevice(), rewards=three, traffic=["low", "fast"])
    with pytest.raises(ValueError, match="not DESIRED_TTC"):
        vec_env.MergeVecEnv(12, env_id="sumo-jerk-continuous-v0", ctx=_NoDevice(), rewards=[{"DESIRED_TTC": 2}])

    class Env:
        continuous, n, obs_dim, sim_cfgs, R, n_per_reward_group = True, 12, 20, None, 3, 4
    cfg = learner.DDPGConfig(n_obs=20)
    with pytest.raises(ValueError, match="3 reward groups, the population 2 members"):
        learner.DDPGPopulation(Env(), (cfg, 2), ctx=_NoDevice())
