"""The learners' Python layer (learner.py, the learner-family methods of _capi.Context): CPU part, no device and no library call.

  * the continuous populations' methods, written once in the binding, reach the C entries they always reached: every ``ddpg_pop_*`` and
    ``td3_pop_*`` method against a literal table of entry names and argument counts, ``member`` raising ``StmpcError`` on a NULL handle;
  * the full call trace of the learner-family ``Context`` methods -- ddpg, td3, dqn, c51, noisy, prioritised replay, n-step; lone and population
    -- is the one recorded before the marshalling was folded into shared helpers: entry, argument order, argument types, scalar values;
  * ``train_ddpg`` under the loop it shares with ``train_dqn``: the calls of every step in order, the drains, the members' returns and takeover
    shares, and ``executed_actions=True``.
"""
import ctypes

import numpy as np
import pytest

from stmpc_testlib import capi as _capi


def _fake_ctx(capi, calls, returns=()):
    """A ``Context`` over a recording library: every entry appends (name, args) to ``calls`` and returns ``returns[name]`` (default 0: STMPC_OK,
    a size of 0, a NULL handle).  ``_chk`` is the real one."""
    returns = dict(returns)

    class _Lib:
        def stmpc_last_error(self):
            return b"refused by the fake"

        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or returns.get(name, 0)
    ctx = object.__new__(capi.Context)
    ctx._lib, ctx._h = _Lib(), None
    return ctx


POP_ENTRIES = {        # (kind, method) -> (C entry, argument count)
    ("ddpg", "create"): ("stmpc_ddpg_pop_create", 4), ("ddpg", "destroy"): ("stmpc_ddpg_pop_destroy", 1), ("ddpg", "size"): ("stmpc_ddpg_pop_size", 1),
    ("ddpg", "member"): ("stmpc_ddpg_pop_member", 2), ("ddpg", "act"): ("stmpc_ddpg_pop_act_device", 9), ("ddpg", "push"): ("stmpc_ddpg_pop_push_device", 13),
    ("ddpg", "update"): ("stmpc_ddpg_pop_update_device", 6), ("ddpg", "stats"): ("stmpc_ddpg_pop_stats_device", 3),
    ("ddpg", "per_enable"): ("stmpc_pop_per_enable_ddpg", 4),
    ("td3", "create"): ("stmpc_pop_td3_create", 4), ("td3", "destroy"): ("stmpc_pop_td3_destroy", 1), ("td3", "size"): ("stmpc_pop_td3_size", 1),
    ("td3", "member"): ("stmpc_pop_td3_member", 2), ("td3", "act"): ("stmpc_pop_td3_act_device", 9), ("td3", "push"): ("stmpc_pop_td3_push_device", 13),
    ("td3", "update"): ("stmpc_pop_td3_update_device", 6), ("td3", "stats"): ("stmpc_pop_td3_stats_device", 3),
    ("td3", "per_enable"): ("stmpc_pop_per_enable_td3", 4),
}


def test_the_binding_routes_the_continuous_populations_to_their_entries():
    capi = _capi()
    calls = []
    ctx = _fake_ctx(capi, calls, {"stmpc_ddpg_pop_member": 7, "stmpc_pop_td3_member": 7, "stmpc_ddpg_pop_size": 3, "stmpc_pop_td3_size": 3})
    for kind, cfg in (("ddpg", capi.DDPGCfg), ("td3", capi.TD3Cfg)):
        m = lambda name: getattr(ctx, "%s_pop_%s" % (kind, name))
        args = {"create": ([cfg(), cfg()],), "destroy": ("h",), "size": ("h",), "member": ("h", 1), "act": ("h", 4, 11, 32, 14, True, 16),
                "push": ("h", 4, 11, 12, 13, 32, 14, 15, 16, 17, 18, 19), "update": ("h", 2, [0.25, 0.5], [1.0, 2.0]), "stats": ("h", 23),
                "per_enable": ("h", [capi.PERCfg(), None])}
        assert len(args) == 9
        for name, a in args.items():
            del calls[:]
            out = m(name)(*a)
            assert [(c[0], len(c[1])) for c in calls] == [POP_ENTRIES[kind, name]], (kind, name, calls)
            if name == "size":
                assert out == 3
            if name == "member":
                assert isinstance(out, ctypes.c_void_p) and out.value == 7
            if name == "create":
                assert isinstance(out, ctypes.c_void_p) and type(calls[0][1][1]).__name__ == cfg.__name__ + "_Array_2" and calls[0][1][2] == 2
            if name == "update":                                    # lr_q before lr_pi, one count for both
                a = calls[0][1]
                assert (a[0], a[1], a[2][0], a[2][1], a[3][0], a[3][1], a[4], a[5]) == ("h", 2, 0.25, 0.5, 1.0, 2.0, 2, 0)
        with pytest.raises(ValueError, match="lr_q has 2 entries, lr_pi 1"):
            m("update")("h", 1, [0.25, 0.5], [1.0])
    # a NULL member is STMPC_EINVAL through the real _chk
    null = _fake_ctx(capi, [])
    for kind in ("ddpg", "td3"):
        with pytest.raises(capi.StmpcError, match="refused by the fake") as e:
            getattr(null, kind + "_pop_member")("h", 64)
        assert e.value.code == capi.STMPC_EINVAL


def _describe(a):
    """An argument as the trace keeps it: a scalar by value, ``byref(x)`` as "&" + x's type, an array of numbers by type and values, anything else
    (a pointer, an array of structs) by its type's name."""
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if hasattr(a, "_obj"):
        return "&" + type(a._obj).__name__
    if isinstance(a, ctypes.Array) and issubclass(a._type_, ctypes._SimpleCData):
        return (type(a).__name__, list(a))
    return type(a).__name__


def _drive(ctx, capi):
    """Every learner-family method of ``Context`` once, with fixed small arguments (device pointers are distinct small integers, the stream is 9)."""
    f3, i8 = np.arange(3, dtype=np.float32), np.arange(8)
    per, ns = capi.PERCfg(), capi.NStepCfg(n_step=3, rows_per_push=4)
    pers, nss = [per, None], [ns, ns]
    # DDPG, lone; prioritised replay on its handle
    ctx.ddpg_create(capi.DDPGCfg())
    ctx.ddpg_destroy("h")
    ctx.ddpg_set_params("h", 2, f3)
    ctx.ddpg_get_params("h", 2, 3)
    ctx.ddpg_set_state("h", i8, np.ones(4))
    ctx.ddpg_get_state("h")
    ctx.ddpg_push("h", 4, 11, 12, 13, 32, 14, 15, 16, 17, 18, 19, 9)
    ctx.ddpg_act("h", 4, 11, 32, 14, True, 16, 20, 9)
    ctx.ddpg_update("h", 2, 0.25, 0.5, 9)
    ctx.ddpg_grads("h", 21, 22, 9)
    ctx.ddpg_stats("h", 23, 9)
    ctx.ddpg_replay_read("h", 1, 2)
    ctx.ddpg_gather("h", 24, 9)
    ctx.per_enable("h", per)
    ctx.per_tree_read("h", 1, 3)
    ctx.per_last("h", 25, 26, 27, 9)
    # TD3, lone
    ctx.td3_create(capi.TD3Cfg())
    ctx.td3_destroy("t")
    ctx.td3_base("t")
    ctx.td3_set_params("t", 1, f3)
    ctx.td3_get_params("t", 1, 3)
    ctx.td3_set_state("t", np.ones(2))
    ctx.td3_get_state("t")
    ctx.td3_update("t", 2, 0.25, 0.5, 9)
    ctx.td3_grads("t", 21, 22, 28, 9)
    ctx.td3_targets("t", 29, 9)
    ctx.td3_stats("t", 23, 9)
    # the continuous populations
    for kind, cfg in (("ddpg", capi.DDPGCfg), ("td3", capi.TD3Cfg)):
        m = lambda name: getattr(ctx, "%s_pop_%s" % (kind, name))
        m("create")([cfg(), cfg()])
        m("destroy")("p")
        m("size")("p")
        m("member")("p", 1)
        m("act")("p", 4, 11, 32, 14, False, 16, 20, 9)
        m("push")("p", 4, 11, 12, 13, 32, 14, 15, 16, 17, 18, 19, 9)
        m("update")("p", 2, [0.25, 0.5], [1.0, 2.0], 9)
        m("stats")("p", 23, 9)
        m("per_enable")("p", pers)
    # the discrete learners, lone and population
    for kind, cfg in (("dqn", capi.DQNCfg), ("c51", capi.C51Cfg)):
        m = lambda name: getattr(ctx, "%s_%s" % (kind, name))
        m("create")(cfg())
        m("destroy")("q")
        m("set_params")("q", 3, f3)
        m("get_params")("q", 3, 3)
        m("set_state")("q", i8, np.ones(2))
        m("get_state")("q")
        m("push")("q", 4, 11, 12, 13, 32, 16, 17, 18, 19, 9)
        m("act")("q", 4, 11, 32, 0.125, 16, 20, 9)
        m("update")("q", 2, 0.25, 9)
        m("grads")("q", 21, 9)
        m("targets")("q", 29, 9)
        m("gather")("q", 24, 9)
        m("stats")("q", 23, 9)
        m("per_enable")("q", per)
        m("per_tree_read")("q", 1, 3)
        m("per_last")("q", 25, 26, 27, 9)
        m("padded_read")("q", 4, 5, 3)
        m("pop_create")([cfg(), cfg(), cfg()])
        m("pop_destroy")("p")
        m("pop_size")("p")
        m("pop_member")("p", 2)
        m("pop_act")("p", 4, 11, 32, [0.0, 0.5, 1.0], 16, 20, 9)
        m("pop_push")("p", 4, 11, 12, 13, 32, 16, 17, 18, 19, 9)
        m("pop_update")("p", 2, [0.25, 0.5, 1.0], 9)
        m("pop_stats")("p", 23, 9)
        m("pop_per_enable")("p", pers)
        m("pop_replay_read")("q", 1, 2)
    # what the C51 learner has on top, and its noisy output layer
    ctx.c51_dist("q", 30, 31, 9)
    ctx.c51_project("q", 5, 32, 33, 34, 35, 36, 9)
    ctx.c51_replay_read("q", 1, 2)
    ctx.c51_dzout_read("q", 7, 20)
    ctx.noisy_c51_enable("q", 0.5)
    ctx.noisy_c51_set_params("q", 1, f3)
    ctx.noisy_c51_get_params("q", 1, 3)
    ctx.noisy_c51_act("q", 4, 11, 32, 0.125, 16, 20, 9)
    ctx.noisy_c51_debug_read("q", 5, 3)
    ctx.c51_pop_noisy_enable("p", [0.5, 0.25])
    ctx.c51_pop_noisy_act("p", 4, 11, 32, [0.0, 0.5], 16, 20, 9)
    # multi-step returns
    for kind in ("ddpg", "dqn", "c51"):
        ctx.nstep_enable(kind, "h", ns)
        ctx.nstep_window(kind, "h", [0, 1, 2])
    for kind in ("ddpg", "td3", "dqn", "c51"):
        ctx.pop_nstep_enable(kind, "p", nss)
    ctx.c51_pop_multi_step_enable("p", nss)
    ctx.c51_pop_multi_step_window("q", [5])


# (entry, arguments as ``_describe`` keeps them), recorded once from the tree before the binding's marshalling was folded, with the ``_drive`` above
# (the type names are ctypes' on LP64 Linux, where c_int64 is c_long and c_uint8 is c_ubyte: the platform the library is built for)
_PERS = ("PERCfg_Array_2", ("c_ubyte_Array_2", [1, 0]), 2)
TRACE = [
    ("stmpc_ddpg_create", ("ctx", "&DDPGCfg", "&c_void_p")), ("stmpc_ddpg_destroy", ("h",)), ("stmpc_ddpg_set_params", ("h", 2, "LP_c_float", 3)),
    ("stmpc_ddpg_get_params", ("h", 2, "LP_c_float", 3)), ("stmpc_ddpg_set_state", ("h", "LP_c_long", "LP_c_float")),
    ("stmpc_ddpg_get_state", ("h", "LP_c_long", "LP_c_float")), ("stmpc_ddpg_push_device", ("h", 4, 11, 12, 13, 32, 14, 15, 16, 17, 18, 19, 9)),
    ("stmpc_ddpg_act_device", ("h", 4, 11, 32, 14, 1, 16, 20, 9)), ("stmpc_ddpg_update_device", ("h", 2, 0.25, 0.5, 9)), ("stmpc_ddpg_grads_device", ("h", 21, 22, 9)),
    ("stmpc_ddpg_stats_device", ("h", 23, 9)), ("stmpc_ddpg_replay_read", ("h", 1, 2, "LP_c_float")), ("stmpc_ddpg_gather_device", ("h", 24, 9)),
    ("stmpc_per_enable", ("h", "&PERCfg")), ("stmpc_per_tree_read", ("h", 1, 3, "LP_c_double")), ("stmpc_per_last_device", ("h", 25, 26, 27, 9)),
    ("stmpc_td3_create", ("ctx", "&TD3Cfg", "&c_void_p")), ("stmpc_td3_destroy", ("t",)), ("stmpc_td3_base", ("t",)), ("stmpc_td3_set_params", ("t", 1, "LP_c_float", 3)),
    ("stmpc_td3_get_params", ("t", 1, "LP_c_float", 3)), ("stmpc_td3_set_state", ("t", "LP_c_float")), ("stmpc_td3_get_state", ("t", "LP_c_float")),
    ("stmpc_td3_update_device", ("t", 2, 0.25, 0.5, 9)), ("stmpc_td3_grads_device", ("t", 21, 22, 28, 9)), ("stmpc_td3_targets_device", ("t", 29, 9)),
    ("stmpc_td3_stats_device", ("t", 23, 9)),
    ("stmpc_ddpg_pop_create", ("ctx", "DDPGCfg_Array_2", 2, "&c_void_p")), ("stmpc_ddpg_pop_destroy", ("p",)),
    ("stmpc_ddpg_pop_size", ("p",)), ("stmpc_ddpg_pop_member", ("p", 1)), ("stmpc_ddpg_pop_act_device", ("p", 4, 11, 32, 14, 0, 16, 20, 9)),
    ("stmpc_ddpg_pop_push_device", ("p", 4, 11, 12, 13, 32, 14, 15, 16, 17, 18, 19, 9)), ("stmpc_ddpg_pop_update_device", ("p", 2, "LP_c_double", "LP_c_double", 2, 9)),
    ("stmpc_ddpg_pop_stats_device", ("p", 23, 9)), ("stmpc_pop_per_enable_ddpg", ("p",) + _PERS),
    ("stmpc_pop_td3_create", ("ctx", "TD3Cfg_Array_2", 2, "&c_void_p")), ("stmpc_pop_td3_destroy", ("p",)), ("stmpc_pop_td3_size", ("p",)),
    ("stmpc_pop_td3_member", ("p", 1)), ("stmpc_pop_td3_act_device", ("p", 4, 11, 32, 14, 0, 16, 20, 9)),
    ("stmpc_pop_td3_push_device", ("p", 4, 11, 12, 13, 32, 14, 15, 16, 17, 18, 19, 9)), ("stmpc_pop_td3_update_device", ("p", 2, "LP_c_double", "LP_c_double", 2, 9)),
    ("stmpc_pop_td3_stats_device", ("p", 23, 9)), ("stmpc_pop_per_enable_td3", ("p",) + _PERS),
    ("stmpc_dqn_create", ("ctx", "&DQNCfg", "&c_void_p")), ("stmpc_dqn_destroy", ("q",)), ("stmpc_dqn_set_params", ("q", 3, "LP_c_float", 3)),
    ("stmpc_dqn_get_params", ("q", 3, "LP_c_float", 3)), ("stmpc_dqn_set_state", ("q", "LP_c_long", "LP_c_float")),
    ("stmpc_dqn_get_state", ("q", "LP_c_long", "LP_c_float")), ("stmpc_dqn_push_device", ("q", 4, 11, 12, 13, 32, 16, 17, 18, 19, 9)),
    ("stmpc_dqn_act_device", ("q", 4, 11, 32, 0.125, 16, 20, 9)), ("stmpc_dqn_update_device", ("q", 2, 0.25, 9)), ("stmpc_dqn_grads_device", ("q", 21, 9)),
    ("stmpc_dqn_targets_device", ("q", 29, 9)), ("stmpc_dqn_gather_device", ("q", 24, 9)), ("stmpc_dqn_stats_device", ("q", 23, 9)),
    ("stmpc_dqn_per_enable", ("q", "&PERCfg")), ("stmpc_dqn_per_tree_read", ("q", 1, 3, "LP_c_double")), ("stmpc_dqn_per_last_device", ("q", 25, 26, 27, 9)),
    ("stmpc_dqn_padded_read", ("q", 4, "LP_c_float", 800)), ("stmpc_pop_dqn_create", ("ctx", "DQNCfg_Array_3", 3, "&c_void_p")), ("stmpc_pop_dqn_destroy", ("p",)),
    ("stmpc_pop_dqn_size", ("p",)), ("stmpc_pop_dqn_member", ("p", 2)), ("stmpc_pop_dqn_act_device", ("p", 4, 11, 32, "LP_c_double", 3, 16, 20, 9)),
    ("stmpc_pop_dqn_push_device", ("p", 4, 11, 12, 13, 32, 16, 17, 18, 19, 9)), ("stmpc_pop_dqn_update_device", ("p", 2, "LP_c_double", 3, 9)),
    ("stmpc_pop_dqn_stats_device", ("p", 23, 9)), ("stmpc_pop_dqn_per_enable", ("p",) + _PERS),
    ("stmpc_pop_dqn_replay_read", ("q", 1, 2, "LP_c_float")),
    ("stmpc_c51_create", ("ctx", "&C51Cfg", "&c_void_p")), ("stmpc_c51_destroy", ("q",)),
    ("stmpc_c51_set_params", ("q", 3, "LP_c_float", 3)), ("stmpc_c51_get_params", ("q", 3, "LP_c_float", 3)), ("stmpc_c51_set_state", ("q", "LP_c_long", "LP_c_float")),
    ("stmpc_c51_get_state", ("q", "LP_c_long", "LP_c_float")), ("stmpc_c51_push_device", ("q", 4, 11, 12, 13, 32, 16, 17, 18, 19, 9)),
    ("stmpc_c51_act_device", ("q", 4, 11, 32, 0.125, 16, 20, 9)), ("stmpc_c51_update_device", ("q", 2, 0.25, 9)), ("stmpc_c51_grads_device", ("q", 21, 9)),
    ("stmpc_c51_targets_device", ("q", 29, 9)), ("stmpc_c51_gather_device", ("q", 24, 9)), ("stmpc_c51_stats_device", ("q", 23, 9)),
    ("stmpc_c51_per_enable", ("q", "&PERCfg")), ("stmpc_c51_per_tree_read", ("q", 1, 3, "LP_c_double")), ("stmpc_c51_per_last_device", ("q", 25, 26, 27, 9)),
    ("stmpc_c51_padded_read", ("q", 4, "LP_c_float", 800)), ("stmpc_pop_c51_create", ("ctx", "C51Cfg_Array_3", 3, "&c_void_p")), ("stmpc_pop_c51_destroy", ("p",)),
    ("stmpc_pop_c51_size", ("p",)), ("stmpc_pop_c51_member", ("p", 2)), ("stmpc_pop_c51_act_device", ("p", 4, 11, 32, "LP_c_double", 3, 16, 20, 9)),
    ("stmpc_pop_c51_push_device", ("p", 4, 11, 12, 13, 32, 16, 17, 18, 19, 9)), ("stmpc_pop_c51_update_device", ("p", 2, "LP_c_double", 3, 9)),
    ("stmpc_pop_c51_stats_device", ("p", 23, 9)), ("stmpc_pop_c51_per_enable", ("p",) + _PERS),
    ("stmpc_pop_c51_replay_read", ("q", 1, 2, "LP_c_float")),
    ("stmpc_c51_dist_device", ("q", 30, 31, 9)), ("stmpc_c51_project_device", ("q", 5, 32, 33, 34, 35, 36, 9)),
    ("stmpc_c51_replay_read", ("q", 1, 2, "LP_c_float")), ("stmpc_c51_dzout_read", ("q", "LP_c_float", 512)), ("stmpc_noisy_c51_enable", ("q", "&NoisyCfg")),
    ("stmpc_noisy_c51_set_params", ("q", 1, "LP_c_float", 3)), ("stmpc_noisy_c51_get_params", ("q", 1, "LP_c_float", 3)),
    ("stmpc_noisy_c51_act_device", ("q", 4, 11, 32, 0.125, 16, 20, 9)), ("stmpc_noisy_c51_debug_read", ("q", 5, "LP_c_float", 3)),
    ("stmpc_pop_noisy_c51_enable", ("p", "NoisyCfg_Array_2", 2)), ("stmpc_pop_noisy_c51_act_device", ("p", 4, 11, 32, "LP_c_double", 2, 16, 20, 9)),
    ("stmpc_nstep_enable_ddpg", ("h", "&NStepCfg")), ("stmpc_nstep_window_ddpg", ("h", "LP_c_long", 3, "LP_c_double")), ("stmpc_nstep_enable_dqn", ("h", "&NStepCfg")),
    ("stmpc_nstep_window_dqn", ("h", "LP_c_long", 3, "LP_c_double")), ("stmpc_c51_multi_step_enable", ("h", "&NStepCfg")),
    ("stmpc_pop_c51_multi_step_window", ("h", "LP_c_long", 3, "LP_c_double")), ("stmpc_pop_nstep_enable_ddpg", ("p", "NStepCfg_Array_2", 2)),
    ("stmpc_pop_nstep_enable_td3", ("p", "NStepCfg_Array_2", 2)), ("stmpc_pop_nstep_enable_dqn", ("p", "NStepCfg_Array_2", 2)),
    ("stmpc_pop_c51_multi_step_enable", ("p", "NStepCfg_Array_2", 2)), ("stmpc_pop_c51_multi_step_enable", ("p", "NStepCfg_Array_2", 2)),
    ("stmpc_pop_c51_multi_step_window", ("q", "LP_c_long", 1, "LP_c_double")),
]


def test_the_learner_bindings_call_trace_is_what_it_was():
    capi = _capi()
    calls = []
    ctx = _fake_ctx(capi, calls, {name: 7 for name in ("stmpc_td3_base", "stmpc_ddpg_pop_member", "stmpc_pop_td3_member", "stmpc_pop_dqn_member",
                                                       "stmpc_pop_c51_member")})
    ctx._h = "ctx"
    _drive(ctx, capi)
    got = [(name, tuple(_describe(a) for a in args)) for name, args in calls]
    ctx._h = None
    assert len(got) == len(TRACE) and len(TRACE) > 100
    for g, want in zip(got, TRACE):
        assert g == want
    learner_entries = {e for e in capi.EXPORTS if any(t in e for t in ("_ddpg_", "_td3_", "_dqn_", "_c51_", "stmpc_per_", "_pop_per_", "_nstep_"))}
    unbound = {"stmpc_ddpg_sample_index", "stmpc_ddpg_noise", "stmpc_td3_noise", "stmpc_per_sample_index",       # module-level functions
               "stmpc_actor_view_ddpg", "stmpc_qactor_view_dqn", "stmpc_pop_c51actor_create", "stmpc_dueling_c51actor_create"}      # the actors'
    assert learner_entries - unbound == {name for name, _ in got}, (learner_entries - unbound) ^ {name for name, _ in got}
    # a lone TD3 learner has no multi-step entries of its own (its ring is its base's): refused by name, before the library is asked
    for call in (lambda: ctx.nstep_enable("td3", "t", capi.NStepCfg()), lambda: ctx.nstep_window("td3", "t", [0])):
        with pytest.raises(ValueError, match="its base's"):
            call()


class _Ticks:
    """``env.episode_ticks``: what ``train_ddpg`` clones before it acts."""

    def __init__(self, env):
        self.env = env

    def clone(self):
        self.env.log.append(("ticks", self.env.steps))
        return "ticks%d" % self.env.steps


class _FakeContinuousEnv:
    """An env of 6 rows that logs what is asked of it; with ``takeovers`` it is a shielded one whose info carries scripted takeovers (torch tensors on
    the CPU, no device) and the action the shield executed."""
    n, continuous, autoreset = 6, True, True

    def __init__(self, log, drains, takeovers=None):
        self.log, self.drains, self.takeovers, self.steps = log, list(drains), takeovers, 0
        self.episode_ticks = _Ticks(self)
        if takeovers is not None:
            import torch
            self.shield, self.torch, self.device = "first_step", torch, torch.device("cpu")

    def reset(self):
        self.log.append(("reset",))
        return "obs0"

    def step(self, action):
        self.log.append(("step", action))
        info = {"final_observation": "fin%d" % self.steps}
        term = trunc = "flag"
        if self.takeovers is not None:
            t = self.torch
            info.update(takeover=t.tensor(self.takeovers[self.steps], dtype=t.bool), executed_action="exec%d" % self.steps)
            term = trunc = t.zeros(self.n, dtype=t.bool)
        self.steps += 1
        return "obs%d" % self.steps, "r%d" % self.steps, term, trunc, info

    def drain_episode_stats(self):
        self.log.append(("drain",))
        ret, env = self.drains.pop(0)
        return {"episode_return": np.array(ret, dtype=np.float64), "env": np.array(env, dtype=np.int64)}


def _fake_ddpg_population(learner, log):
    class _Pop(learner.DDPGPopulation):
        def __init__(self):
            self.P, self.n_per_member = 3, 2

        def __del__(self):
            pass

        def act(self, obs, ticks, noise=True, debug=None):
            log.append(("act", obs, ticks, noise))
            return "a%s" % obs[3:]

        def push(self, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs=None, next_ticks=None):
            log.append(("push", obs, ticks, action, reward, next_obs, final_obs))

        def update(self, n=1, lr_q=None, lr_pi=None):
            log.append(("update", n, lr_q, lr_pi))
    return _Pop()


def test_train_ddpg_runs_the_shared_loop():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    # env.n = 6, P = 3, 30 frames: 5 steps; drain_every = 2: drains after steps 2, 4 and 5
    drains = [([1.0, 2.0, 3.0], [0, 5, 2]), ([4.0], [3]), ([5.0, 6.0], [4, 1])]
    log = []
    lr = lambda i, steps: ([1e-3 * (i + 1)] * 3, 2e-3) if steps == 5 else None
    res = learner.train_ddpg(_FakeContinuousEnv(log, drains), _fake_ddpg_population(learner, log), 30, updates_per_step=2, drain_every=2, lr_schedule=lr)
    want = [("reset",)]
    for i in range(5):
        want += [("ticks", i), ("act", "obs%d" % i, "ticks%d" % i, True), ("step", "a%d" % i),
                 ("push", "obs%d" % i, "ticks%d" % i, "a%d" % i, "r%d" % (i + 1), "obs%d" % (i + 1), "fin%d" % i), ("update", 2, [1e-3 * (i + 1)] * 3, 2e-3)]
        if i in (1, 3, 4):
            want.append(("drain",))
    assert log == want
    assert set(res) == {"steps", "frames", "episodes", "mean_return", "returns", "takeover_share", "member_returns"}
    assert res["steps"] == 5 and res["frames"] == 30 and res["episodes"] == 6 and res["mean_return"] == 3.5 and res["takeover_share"] == 0.0
    assert np.array_equal(res["returns"], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    mr = res["member_returns"]                                      # owner = env // 2: envs 0, 1 -> 0; 2, 3 -> 1; 4, 5 -> 2
    assert len(mr) == 3 and np.array_equal(mr[0], [1.0, 6.0]) and np.array_equal(mr[1], [3.0, 4.0]) and np.array_equal(mr[2], [2.0, 5.0])
    # no schedule: the learner's own rates; no updates asked for: none made
    del log[:]
    learner.train_ddpg(_FakeContinuousEnv(log, [([], [])]), _fake_ddpg_population(learner, log), 6)
    assert [c for c in log if c[0] == "update"] == [("update", 1, None, None)]
    del log[:]
    learner.train_ddpg(_FakeContinuousEnv(log, [([], [])]), _fake_ddpg_population(learner, log), 6, updates_per_step=0)
    assert [c[0] for c in log] == ["reset", "ticks", "act", "step", "push", "drain"]
    # behind a shield: the executed action is what is pushed, and the takeovers are counted for the whole env and per member
    take = [[1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0] * 6, [0] * 6]
    del log[:]
    res = learner.train_ddpg(_FakeContinuousEnv(log, [([], [])] * 3, take), _fake_ddpg_population(learner, log), 30, drain_every=2, executed_actions=True)
    assert [c[3] for c in log if c[0] == "push"] == ["exec%d" % i for i in range(5)] and [c[1] for c in log if c[0] == "step"] == ["a%d" % i for i in range(5)]
    assert res["takeover_share"] == 4 / 30 and res["member_takeover_share"] == [2 / 10, 1 / 10, 1 / 10]
    assert set(res) == {"steps", "frames", "episodes", "mean_return", "returns", "takeover_share", "member_returns", "member_takeover_share"}
    del log[:]
    res = learner.train_ddpg(_FakeContinuousEnv(log, [([], [])] * 3, take), _fake_ddpg_population(learner, log), 30, drain_every=2)
    assert [c[3] for c in log if c[0] == "push"] == ["a%d" % i for i in range(5)] and res["takeover_share"] == 4 / 30
    # a lone learner: the share alone
    lone = object.__new__(learner.DDPGLearner)
    lone.act, lone.push, lone.update = (lambda *a, **kw: "a"), (lambda *a, **kw: None), (lambda *a: None)
    res = learner.train_ddpg(_FakeContinuousEnv([], [([7.0], [2])] * 3, take), lone, 30, drain_every=2)
    assert set(res) == {"steps", "frames", "episodes", "mean_return", "returns", "takeover_share"} and res["takeover_share"] == 4 / 30 and res["episodes"] == 3
