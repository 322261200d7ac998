"""vec_env.env_entries: the pure table from an env's shape -- its shield, whether it has a traffic mix, its reward groups R and traffic groups G -- to
the names of the ``_capi.Context`` methods that reset and step it, and ``vec_env._LEAD``, the leading arguments an env binds to each.  No GPU: the
table row by row against literal names, every name and lead against the methods' signatures, and the refusals with the classes' messages."""
import inspect

import pytest

from stmpc_testlib import pkg as _pkg

# (shield, has_mix, R, G) -> (reset, step): the eleven shapes the C entries serve, each name written out
SERVED = {
    (None, False, 0, 0): ("env_reset", "env_step"),
    (None, False, 0, 3): ("env_reset_groups", "env_step_groups"),
    (None, False, 2, 0): ("env_reset_reward_groups", "env_step_reward_groups"),
    (None, False, 2, 2): ("env_reset_reward_groups", "env_step_reward_groups"),
    (None, True, 0, 0): ("traffic_mix_env_reset", "traffic_mix_env_step"),
    ("first_step", False, 0, 0): ("shield_env_reset", "shield_env_step"),
    ("first_step", False, 0, 3): ("shield_env_reset_groups", "shield_env_step_groups"),
    ("first_step", False, 2, 0): ("shield_env_reset_reward_groups", "shield_env_step_reward_groups"),
    ("first_step", False, 2, 2): ("shield_env_reset_reward_groups", "shield_env_step_reward_groups"),
    ("first_step", True, 0, 0): ("shield_traffic_mix_env_reset", "shield_traffic_mix_env_step"),
    ("combined", False, 0, 0): ("cshield_env_reset", "cshield_env_step"),
}
# what follows an entry's leading arguments: a reset's (d_obs, obs_stride), a step's (d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated,
# d_final_obs, d_final_stats); then the shield's five outputs (step), the mix's type outputs (one at the reset, two at the step) and the stream
PER_CALL = {"reset": 2, "step": 8}
SHIELD_OUT, STREAM = 5, 1
# env attribute -> the names of the Context methods' parameters it may be bound to
PARAM_OF = {"params": {"params"}, "sim_cfg": {"sim_cfg"}, "cfg": {"env_cfg"}, "n": {"N"}, "sim_cfgs": {"cfgs", "sim_cfgs"}, "_world": {"sim_cfgs"},
            "n_per_group": {"n_per_group", "n_per_traffic_group"}, "reward_cfgs": {"env_cfgs"}, "n_per_reward_group": {"n_per_reward_group"},
            "mix_cfgs": {"sim_cfgs"}, "mix_weights": {"weights"}, "mix_seed": {"mix_seed"}, "shield_cfg": {"shield_cfg"},
            "takeover_penalties": {"takeover_penalties"}, "_actor": {"actor"}}


def test_the_table_row_by_row():
    _pkg()
    from rl_mpc_lanemerging_amd import vec_env
    assert len(SERVED) == 11 and len(set(SERVED.values())) == 9
    for shape, names in SERVED.items():
        assert vec_env.env_entries(*shape) == names, shape
    assert vec_env.env_entries() == ("env_reset", "env_step")
    # the group counts matter only as none / some / equal
    assert vec_env.env_entries(None, False, 0, 64) == vec_env.env_entries(None, False, 0, 1) == SERVED[(None, False, 0, 3)]
    assert vec_env.env_entries("first_step", False, 5, 5) == SERVED[("first_step", False, 2, 2)]


def test_every_name_is_a_context_method_that_takes_the_envs_call():
    _pkg()
    from rl_mpc_lanemerging_amd import _capi, vec_env
    assert {name for names in SERVED.values() for name in names} == set(vec_env._LEAD)
    for (shield, has_mix, _, _), names in SERVED.items():
        for kind, name in zip(("reset", "step"), names):
            method = getattr(_capi.Context, name)
            assert callable(method), name
            params = list(inspect.signature(method).parameters)
            lead = vec_env._LEAD[name].split()
            tail = (SHIELD_OUT if shield and kind == "step" else 0) + (has_mix * (1 if kind == "reset" else 2))
            assert len(params) == 1 + len(lead) + PER_CALL[kind] + tail + STREAM, name
            assert params[0] == "self" and params[-1] == "stream" and params[1] == "params" == lead[0], name
            for attr, param in zip(lead, params[1:]):                                         # (each lead attribute is what that parameter takes)
                assert param in PARAM_OF[attr], (name, attr, param)
            first = params[1 + len(lead)]
            assert first == ("d_obs" if kind == "reset" else "d_action"), (name, first)       # (the lead ends where the per-call pointers begin)
            if has_mix:
                assert params[-2] == ("d_traffic_type" if kind == "reset" else "d_final_traffic_type"), name
            if shield and kind == "step":
                assert params[-2 - 2 * has_mix] == "d_takeover_ticks", name


def test_refused_shapes_raise_the_classes_messages():
    _pkg()
    from rl_mpc_lanemerging_amd import vec_env
    mix_alone = "a traffic mix with traffic groups, reward groups or a shield is out of scope"
    for shield in (None, "first_step"):
        for R, G in ((0, 2), (2, 0), (2, 2), (2, 3)):
            with pytest.raises(ValueError, match=mix_alone):
                vec_env.env_entries(shield, True, R, G)
        for R, G in ((2, 3), (3, 2), (1, 64)):
            with pytest.raises(ValueError, match="the env has %d traffic groups and %d reward groups: .* must coincide" % (G, R)):
                vec_env.env_entries(shield, False, R, G)
    for bad in ("second_step", "first-step", "", 1, True):
        with pytest.raises(ValueError, match="unknown shield"):
            vec_env.env_entries(bad)
    for has_mix, R, G in ((True, 0, 0), (False, 0, 2), (False, 2, 0), (False, 2, 2)):
        with pytest.raises(ValueError, match="behind the combined shield are out of scope"):
            vec_env.env_entries("combined", has_mix, R, G)


def test_the_classes_raise_the_tables_refusals_before_any_device_call(restore_settings):
    """The shapes the table refuses, through the constructors that can express them: the same messages, and no context is asked for anything."""
    _pkg()
    from rl_mpc_lanemerging_amd import vec_env

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the device was touched (%s)" % name)
    two, three = [{"REWARD_FUNCTION": "ST"}, {"REWARD_FUNCTION": "Slotted"}], ["default", "low", "fast"]
    for make in (lambda: vec_env.MergeVecEnv(12, ctx=NoDevice(), traffic=three, rewards=two),
                 lambda: vec_env.GroupedShieldVecEnv(12, ctx=NoDevice(), traffic=three, rewards=two)):
        with pytest.raises(ValueError, match="the env has 3 traffic groups and 2 reward groups: .* must coincide"):
            make()
    for make in (lambda: vec_env.MergeVecEnv(12, ctx=NoDevice(), traffic=three, traffic_mix=three),
                 lambda: vec_env.GroupedShieldVecEnv(12, ctx=NoDevice(), rewards=two, traffic_mix=three)):
        with pytest.raises(ValueError, match="a traffic mix with traffic groups, reward groups or a shield is out of scope"):
            make()
