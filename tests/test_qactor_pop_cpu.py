"""A population of Q-networks as policies (``actor.QActorPopulation``, ``actor.population_of``, ``learner.evaluate_dqn_members``, the
stmpc_pop_qactor_ entries) without a GPU: header, library and binding agree; the refusals that are made before any device call; the dispatch
between the two kinds of population.  There is no new host twin: a member's arithmetic is ``actor.q_policy_host``'s on its slice
(test_qactor_cpu.py).  The GPU part is test_qactor_pop.py."""
import ctypes
import types

import numpy as np
import pytest

from stmpc_testlib import capi as _capi, header_entries, header_prototypes, header_text

ENTRIES = {"stmpc_pop_qactor_" + n for n in ("create", "destroy", "size", "eval_device")}


def test_header_library_and_binding_agree_on_the_q_actor_population():
    capi = _capi()
    lib = capi.load()
    protos = header_prototypes("stmpc_pop_qactor_")
    assert set(protos) == ENTRIES == header_entries("stmpc_pop_qactor_") == {n for n in capi.EXPORTS if n.startswith("stmpc_pop_qactor_")}
    for name, args in protos.items():
        fn = getattr(lib, name)                                   # (AttributeError: the library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")), name
    # the evaluation has the lone entry's signature behind (ctx, population, cfg, n_per_member)
    lone = header_prototypes("stmpc_qactor_")["stmpc_qactor_eval_device"]
    assert protos["stmpc_pop_qactor_eval_device"].replace("const stmpc_qactor_pop *pop", "const stmpc_qactor *qactor").replace("int n_per_member", "int N") == lone
    assert lib.stmpc_pop_qactor_eval_device.argtypes == lib.stmpc_qactor_eval_device.argtypes
    assert lib.stmpc_pop_qactor_create.argtypes == lib.stmpc_actor_pop_create.argtypes and lib.stmpc_pop_qactor_destroy.restype is None
    for name in ("create", "destroy", "size", "eval_device"):
        assert callable(getattr(capi.Context, "qactor_pop_" + name)), name
    # the lone actor's closed set did not grow, every declared entry is exported, the ABI is still 8
    assert header_entries("stmpc_qactor_") == {"stmpc_qactor_" + n for n in ("create", "view_dqn", "destroy", "set_limits", "eval_device")}
    assert header_entries("stmpc_") - {"stmpc_params", "stmpc_stats", "stmpc_ctx"} == set(capi.EXPORTS)
    flat = header_text(flat=True)
    assert "typedef struct stmpc_qactor_pop stmpc_qactor_pop;" in flat
    assert "#define STMPC_ABI_VERSION 8" in flat and capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8
    # every entry's line of the section comment names the reference's function it stands for; the header says why the device table stays valid
    text = header_text()
    section = text[text.index("A population of Q-networks as policies"):text.index("typedef struct stmpc_qactor_pop")]
    for tail in ("create", "destroy", "size", "eval_device"):
        line = [ln for ln in section.splitlines() if ("stmpc_pop_qactor_" + tail) in ln.split("(")[0]]
        assert line and "dqn.py:375-380" in line[0], tail
    flat_section = " ".join(section.split())
    assert "fixed from stmpc_dqn_create to stmpc_dqn_destroy" in flat_section and "stmpc_pop_dqn_per_enable" in flat_section


def test_entries_refuse_null_before_touching_a_device():
    capi = _capi()
    lib = capi.load()
    h = ctypes.c_void_p()
    fcfg = capi.FeaturesCfg.from_settings(__import__("rl_mpc_lanemerging_amd").Settings, time_feature=False)
    one = (ctypes.c_void_p * 1)(None)
    assert lib.stmpc_pop_qactor_create(None, one, 1, ctypes.byref(h)) == capi.STMPC_EINVAL and b"NULL" in lib.stmpc_last_error() and not h.value
    assert lib.stmpc_pop_qactor_eval_device(None, None, ctypes.byref(fcfg), 4, 8, 1, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0, 0) == capi.STMPC_EINVAL
    assert b"NULL" in lib.stmpc_last_error()
    assert lib.stmpc_pop_qactor_size(None) == 0
    lib.stmpc_pop_qactor_destroy(None)                              # (a NULL handle is nothing to destroy)


class _NoDevice:
    """A context that must not be asked for anything."""

    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


def _fake_learner(n_obs=20, h1=16, A=5):
    from rl_mpc_lanemerging_amd import learner
    return types.SimpleNamespace(cfg=learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1), action_values=np.arange(float(A)), handle=None, export_q=lambda path: path)


def test_q_actor_population_refuses_before_any_device_call(tmp_path):
    _capi()
    from rl_mpc_lanemerging_amd import Settings, actor, learner
    ctx = _NoDevice()
    L = _fake_learner()
    with pytest.raises(ValueError, match="1 ... 64 members, not 0"):
        actor.QActorPopulation([], 4, ctx, Settings)
    with pytest.raises(ValueError, match="1 ... 64 members, not 65"):
        actor.QActorPopulation([L] * 65, 4, ctx, Settings)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_per_member must be positive"):
            actor.QActorPopulation([L, L], bad, ctx, Settings)
    # a member of another kind: a DDPG actor, a DDPG learner (export_actor, no export_q), a number
    ddpg_actor = object.__new__(actor.DDPGActor)
    ddpg_learner = types.SimpleNamespace(export_actor=None, handle=None)
    for other in (ddpg_actor, ddpg_learner, 3.5):
        with pytest.raises(ValueError, match="a member is an export_q file, a DQNLearner or a DQNActor"):
            actor.QActorPopulation([L, other], 4, ctx, Settings)
    # members of different shapes: a learner, a file and an actor against member 0 (h1 = 16 and 12 share the padded width and pass this check)
    net = learner.init_q_net(20, 48, 5, np.random.default_rng(0))
    path = tmp_path / "q.npz"
    np.savez(path, **net, action_values=np.arange(5.0))
    wide = object.__new__(actor.DQNActor)
    wide.shape, wide.handle = (20, 16, 20), None
    for other, shape in ((_fake_learner(h1=48), "20 -> 48 -> 5"), (str(path), "20 -> 48 -> 5"), (path, "20 -> 48 -> 5"), (wide, "20 -> 16 -> 20"),
                         (_fake_learner(n_obs=19), "19 -> 16 -> 5")):
        with pytest.raises(ValueError, match="member 2 is %s, member 0 is 20 -> 16 -> 5" % shape):
            actor.QActorPopulation([L, _fake_learner(h1=12), other], 4, ctx, Settings)
    # a DQNPopulation is taken member by member
    pop = types.SimpleNamespace(P=3, member=lambda m: [L, L, 7][m])
    with pytest.raises(ValueError, match="not 7"):
        actor.QActorPopulation(pop, 4, ctx, Settings)


def test_population_of_dispatches_on_the_members_kind(monkeypatch):
    _capi()
    from rl_mpc_lanemerging_amd import Settings, actor
    calls = []
    monkeypatch.setattr(actor, "QActorPopulation", lambda members, n, ctx, S: calls.append(("q", list(members), n)) or "qpop")
    monkeypatch.setattr(actor, "ActorPopulation", lambda members, n, ctx, S, **kw: calls.append(("ddpg", members, n, kw)) or "pop")
    L = _fake_learner()
    A = object.__new__(actor.DQNActor)
    A.handle = None
    ddpg_learner = types.SimpleNamespace(export_actor=None, handle=None)
    ddpg_actor = object.__new__(actor.DDPGActor)
    assert actor.population_of([L, A, L], 4, None, Settings) == "qpop" and calls.pop() == ("q", [L, A, L], 4)
    assert actor.population_of((A,), 2, None, Settings) == "qpop" and calls.pop() == ("q", [A], 2)
    # a population of learners counts as its members
    qpop = types.SimpleNamespace(P=2, member=lambda m: L)
    assert actor.population_of(qpop, 3, None, Settings) == "qpop" and calls.pop() == ("q", [L, L], 3)
    # none is a Q-network: today's population with today's arguments; names and paths stay DDPG
    members = ["medium1", ddpg_learner, ddpg_actor]
    assert actor.population_of(members, 4, None, Settings, time_feature=False) == "pop"
    kind, got, n, kw = calls.pop()
    assert kind == "ddpg" and got is members and n == 4 and kw == {"time_feature": False}
    dpop = types.SimpleNamespace(P=2, member=lambda m: ddpg_learner)
    assert actor.population_of(dpop, 4, None, Settings) == "pop" and calls.pop()[1] is dpop
    assert actor.population_of(["q.npz"], 1, None, Settings) == "pop" and calls.pop()[0] == "ddpg"
    # a mix
    for mix in ([L, "medium1"], [ddpg_actor, A], [ddpg_learner, L, L]):
        with pytest.raises(ValueError, match="DDPG and DQN members do not share a population"):
            actor.population_of(mix, 4, None, Settings)
    assert not calls


def test_evaluate_dqn_members_refusals(monkeypatch):
    _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    monkeypatch.setattr(learner._capi, "Context", lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))
    monkeypatch.setattr(actor, "QActorPopulation", lambda *a: (_ for _ in ()).throw(AssertionError("a population was built")))
    L = _fake_learner()
    with pytest.raises(ValueError, match="'combined' or 'first_step', not 'st'"):
        learner.evaluate_dqn_members([L, L], 4, controller="st")
    with pytest.raises(ValueError, match="3 traffic groups for 2 members"):
        learner.evaluate_dqn_members([L, L], 4, traffic=["low", "medium", "fast"])
    pop = object.__new__(learner.DQNPopulation)
    pop.P = 2
    with pytest.raises(ValueError, match="3 traffic groups for 2 members"):
        learner.evaluate_dqn_members(pop, 4, traffic=["low", "medium", "fast"])
    with pytest.raises(ValueError, match="2 traffic groups for 1 members"):
        learner.evaluate_dqn_members(L, 4, traffic=["low", "medium"])


def test_evaluate_members_points_a_dqn_population_to_the_new_function():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    with pytest.raises(ValueError) as err:
        learner.evaluate_members(object.__new__(learner.DQNPopulation), 4)
    assert "evaluate_dqn(pop.member(m)" in str(err.value) and "evaluate_dqn_members(" in str(err.value)
