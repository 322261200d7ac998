"""The combined-controller shield of the discrete vector environments, host side (vec_env.QCombinedShieldVecEnv, _capi.QShieldEnvCfg, the
stmpc_qshield_env_* entries of include/stmpc.h, learner.train_dqn on shielded envs).  No GPU: the header against the binding, every refusal that must
come before a device call, the host twin of the first action, and train_dqn's takeover counting on fake envs (torch on the CPU)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from stmpc_testlib import capi as _capi, header_entries as _header_entries, header_struct_fields as _header_struct_fields, same as _same

ENTRIES = {"stmpc_qshield_env_reset_device": 12, "stmpc_qshield_env_step_device": 22}


def test_header_declares_the_struct_and_the_entries():
    capi = _capi()
    header = " ".join(open(os.path.join(REPO, "include", "stmpc.h")).read().split())
    declared = {name: args for name, args in re.findall(r"\bint (stmpc_qshield_env_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header)}
    assert set(declared) == set(ENTRIES) <= set(capi.EXPORTS)
    assert _header_entries("stmpc_") - {"stmpc_params", "stmpc_stats", "stmpc_ctx"} == set(capi.EXPORTS)          # every declared entry is exported
    lib = capi.load()
    for name, n_args in ENTRIES.items():
        assert len(declared[name].split(",")) == n_args == len(getattr(lib, name).argtypes), name
        assert "dqn.py:117-200" in header and "dqn.py:375-380" in header
    want = _header_struct_fields("stmpc_qshield_env_cfg")
    assert want == [("cc", "stmpc_combined_cfg"), ("features", "stmpc_policy_features_cfg"), ("takeover_penalty", "double"), ("kmax", "int32_t"),
                    ("reserved0", "int32_t")]
    ctype_of = {"stmpc_combined_cfg": capi.CombinedCfg, "stmpc_policy_features_cfg": capi.FeaturesCfg, "double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(n, ctype_of[t]) for n, t in want] == list(capi.QShieldEnvCfg._fields_)
    # stmpc_cshield_env_cfg without rollout_time: the same size and offsets up to kmax
    assert ctypes.sizeof(capi.QShieldEnvCfg) == ctypes.sizeof(capi.CShieldEnvCfg)
    for f in ("cc", "features", "takeover_penalty", "kmax"):
        assert getattr(capi.QShieldEnvCfg, f).offset == getattr(capi.CShieldEnvCfg, f).offset, f
    assert "#define STMPC_ABI_VERSION 8 " in header and capi.ABI_VERSION == 8 == lib.stmpc_abi_version()
    import rl_mpc_lanemerging_amd as pkg
    c = capi.QShieldEnvCfg.from_settings(pkg.Settings, sparse_control=True, takeover_penalty=0.7, kmax=16)
    assert (c.cc.sparse_control, c.cc.tick_length, c.cc.rollout_length, c.takeover_penalty, c.kmax, c.reserved0, c.features.time_feature) == \
        (1, pkg.Settings.TICK_LENGTH, int(pkg.Settings.ROLLOUT_LENGTH), 0.7, 16, 0, 0)
    d = capi.QShieldEnvCfg.from_settings(pkg.Settings)
    assert (d.cc.sparse_control, d.takeover_penalty, d.kmax) == (0, 0.0, 32)
    assert bytes(d.features) == bytes(capi.FeaturesCfg.from_settings(pkg.Settings, time_feature=False))


def test_context_methods_take_the_entries_arguments():
    capi = _capi()
    from rl_mpc_lanemerging_amd import vec_env
    # (self + the entry's arguments but the context; the stream is optional)
    for (name, n_args), method in zip(ENTRIES.items(), vec_env._Q_ENTRIES):
        params = list(inspect.signature(getattr(capi.Context, method)).parameters)
        assert len(params) == n_args and params[-1] == "stream", name
        lead = vec_env._Q_LEAD[method].split()
        assert params[1:1 + len(lead)] == ["params", "sim_cfg", "env_cfg", "shield_cfg", "qactor", "qactor_pop", "n_per_member", "N"], name
        assert params[1 + len(lead)] == ("d_obs" if method.endswith("reset") else "d_action"), name
    assert "d_executed_action" not in inspect.signature(capi.Context.qshield_env_step).parameters
    # the table of MergeVecEnv's shapes is what it was: the new class binds its own pair
    assert not set(vec_env._Q_ENTRIES) & set(vec_env._LEAD) and vec_env.env_entries("combined") == ("cshield_env_reset", "cshield_env_step")


def _table(S, env_id):
    values = S.JERK_VALUES_DQN if env_id == "sumo-jerk-v0" else S.ACCELERATION_VALUES_DQN
    return np.array([values[i] for i in range(len(values))], dtype=np.float64)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


def _fake_q(cls, env_id="sumo-jerk-v0", n=4, ctx=None, engine="hip", **more):
    """A policy object that never touched a device: what the env reads of one before its first device call."""
    capi = _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor
    a = cls.__new__(cls)
    a.n, a.ctx, a.engine, a.handle = n, ctx if ctx is not None else _NoDevice(), engine, None if engine != "hip" else ctypes.c_void_p(1)
    a.fcfg = capi.FeaturesCfg.from_settings(pkg.Settings, time_feature=cls is actor.DDPGActor)
    a.mode = "jerk" if env_id == "sumo-jerk-v0" else "acceleration"
    S = pkg.Settings
    a.action_values = _table(S, env_id)
    a.__dict__.update(more)
    return a                         # (its __del__ finds no usable context to destroy the handle on, and says nothing)


def _fake_pop(env_id="sumo-jerk-v0", P=2, n_per_member=2, ctx=None, members=None):
    from rl_mpc_lanemerging_amd import actor
    p = _fake_q(actor.QActorPopulation, env_id, n=P * n_per_member, ctx=ctx)
    p.P, p.n_per_member = P, n_per_member
    p.members = members if members is not None else [_fake_q(actor.DQNActor, env_id, n=1, ctx=p.ctx) for _ in range(P)]
    return p


def test_vec_env_refuses_before_any_device_call(restore_settings):
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, vec_env
    E = vec_env.QCombinedShieldVecEnv
    for env_id in ("sumo-jerk-v0", "sumo-accel-v0"):
        ok = _fake_q(actor.DQNActor, env_id)
        with pytest.raises(ValueError, match="CombinedShieldVecEnv"):
            E(4, ok, env_id="sumo-jerk-continuous-v0")
        with pytest.raises(ValueError, match="Invalid gym environment"):
            E(4, ok, env_id="sumo-v9")
        for cls in (actor.DDPGActor, actor.ActorPopulation):
            with pytest.raises(ValueError, match="DDPGActor or an ActorPopulation"):
                E(4, _fake_q(cls, env_id), env_id=env_id)
        for bad in (None, "q.npz", object(), _fake_q(actor.DQNActor, env_id, engine="torch")):
            with pytest.raises(ValueError, match="hip-engine actor.DQNActor"):
                E(4, bad, env_id=env_id)
        with pytest.raises(ValueError, match="built for 4 rows"):
            E(8, ok, env_id=env_id)
        with pytest.raises(ValueError, match="P = 2 members x n_per_member = 2"):
            E(6, _fake_pop(env_id), env_id=env_id)
        with pytest.raises(ValueError, match="another context"):
            E(4, ok, env_id=env_id, ctx=_NoDevice())
        other = "sumo-accel-v0" if env_id == "sumo-jerk-v0" else "sumo-jerk-v0"
        with pytest.raises(ValueError, match="mode"):
            E(4, _fake_q(actor.DQNActor, other), env_id=env_id)
        with pytest.raises(ValueError, match="mode"):
            E(4, _fake_q(actor.DQNActor, env_id, mode="jerk" if env_id == "sumo-accel-v0" else "acceleration"), env_id=env_id)
        table = ok.action_values.copy()
        table[1] = np.nextafter(table[1], 9.0)                                   # (one bit off is not the env's table)
        with pytest.raises(ValueError, match="action table of the policy"):
            E(4, _fake_q(actor.DQNActor, env_id, action_values=table), env_id=env_id)
        with pytest.raises(ValueError, match="action table of the policy"):
            E(4, _fake_q(actor.DQNActor, env_id, action_values=ok.action_values[:-1]), env_id=env_id)
        members = [_fake_q(actor.DQNActor, env_id, n=1), _fake_q(actor.DQNActor, env_id, n=1, action_values=table)]
        with pytest.raises(ValueError, match="action table of member 1"):
            E(4, _fake_pop(env_id, members=members), env_id=env_id)
        for bad in (-0.1, float("inf"), float("nan"), "much"):
            with pytest.raises(ValueError, match="takeover_penalty"):
                E(4, ok, env_id=env_id, takeover_penalty=bad)
        for bad in (0, -1, 33, 64):
            with pytest.raises(ValueError, match="shield_kmax"):
                E(4, ok, env_id=env_id, shield_kmax=bad)
        with pytest.raises(ValueError, match="a controller group may set"):
            E(4, ok, env_id=env_id, control={"TICK_LENGTH": 0.1})
        with pytest.raises(ValueError, match="REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED"):
            E(4, ok, env_id=env_id, control={"REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED": True})
        with pytest.raises(ValueError, match="Invalid reward function"):
            E(4, ok, env_id=env_id, reward="Generous")
    pkg.Settings.REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED = True
    with pytest.raises(ValueError, match="REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED"):
        E(4, _fake_q(actor.DQNActor), env_id="sumo-jerk-v0")
    # the continuous env's class keeps its refusal of the discrete ids
    with pytest.raises(ValueError, match="sumo-jerk-continuous-v0"):
        vec_env.CombinedShieldVecEnv(4, _fake_q(actor.DDPGActor), env_id="sumo-jerk-v0")


def test_signatures():
    _capi()
    from rl_mpc_lanemerging_amd import learner, vec_env
    p = inspect.signature(vec_env.QCombinedShieldVecEnv.__init__).parameters
    positional = [("n", inspect.Parameter.empty), ("policy", inspect.Parameter.empty), ("env_id", None), ("seed", 0), ("reward", None), ("autoreset", True),
                  ("ctx", None), ("log_capacity", 0)]
    keyword = [("shield_sparse", False), ("takeover_penalty", 0.0), ("shield_kmax", 32), ("control", None)]
    items = list(p.items())[1:]
    assert [(k, v.default) for k, v in items] == positional + keyword
    assert all(v.kind == inspect.Parameter.KEYWORD_ONLY for _, v in items[len(positional):])
    assert not hasattr(vec_env.QCombinedShieldVecEnv, "rollout_evals")               # no time feature, no counter
    t = inspect.signature(learner.train_dqn).parameters
    assert [(k, v.default) for k, v in list(t.items())[3:]] == [("updates_per_step", 1), ("drain_every", 64), ("eps_schedule", None), ("lr_schedule", None)]
    assert "no shield" not in learner.train_dqn.__doc__


def test_first_action_host_twin_is_the_q_actors_rule(restore_settings):
    """numpy fp64, operation for operation: for every index the twin's jerk is q_policy_host's for a network whose first maximum is that index, on
    accelerations that clip at either edge and that do not; an index out of range gives 0.0 and is flagged."""
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, vec_env
    S = pkg.Settings
    rng = np.random.default_rng(5)
    for env_id, mode in (("sumo-jerk-v0", "jerk"), ("sumo-accel-v0", "acceleration")):
        table = _table(S, env_id)
        A = table.size
        idx = np.tile(np.arange(A), 6)
        acc = np.concatenate([rng.uniform(float(S.MAX_NEGATIVE_ACCELERATION), float(S.MAX_POSITIVE_ACCELERATION), 4 * A), table[np.arange(A)],
                              table[np.arange(A)] - 0.3 * float(S.TICK_LENGTH)])
        got, bad = vec_env.q_first_action_host(env_id, idx, acc, S)
        assert not bad.any() and got.dtype == np.float64
        net = {"w0": np.zeros((4, 3), np.float32), "b0": np.zeros(4, np.float32), "w1": np.zeros((A, 4), np.float32), "b1": np.zeros(A, np.float32)}
        for a in range(A):
            net["b1"][:] = 0
            net["b1"][a] = 1                                           # Q = one-hot(a): the first maximum is a
            rows = idx == a
            _, i, jerk = actor.q_policy_host(net, np.zeros((int(rows.sum()), 3)), table, mode, ego_acc=acc[rows], S=S)
            assert (i == a).all() and _same(got[rows], jerk), (env_id, a)
        lo, hi, tick = float(S.MINIMUM_NEGATIVE_JERK), float(S.MAXIMUM_POSITIVE_JERK), float(S.TICK_LENGTH)
        if mode == "acceleration":
            raw = (table[idx] - acc) / tick
            assert (got == lo).any() and (got == hi).any() and ((got > lo) & (got < hi)).any()
            inside = (raw >= lo) & (raw <= hi)
            assert _same(got[inside], raw[inside]) and _same(got[raw < lo], np.full(int((raw < lo).sum()), lo))
        else:
            assert _same(got, table[idx])
        got, bad = vec_env.q_first_action_host(env_id, [-1, 0, A - 1, A, 2 ** 31 - 1], np.full(5, 0.25), S)
        assert list(bad) == [True, False, False, True, True] and list(got[bad]) == [0.0, 0.0, 0.0] and np.isfinite(got).all()
    with pytest.raises(ValueError, match="discrete env id"):
        vec_env.q_first_action_host("sumo-jerk-continuous-v0", [0], [0.0])


class _FakeShieldedEnv:
    """An env of 6 rows whose info["takeover"] and flags are scripted: torch tensors on the CPU, no device."""
    n, shield = 6, "first_step"

    def __init__(self, takeovers, done, autoreset, drains=None):
        import torch
        self.torch, self.device, self.autoreset = torch, torch.device("cpu"), autoreset
        self.takeovers, self.done, self.steps = takeovers, done, 0
        self.drains = drains

    def reset(self):
        return "obs0"

    def step(self, action):
        t = self.torch
        take, done = t.tensor(self.takeovers[self.steps], dtype=t.bool), t.tensor(self.done[self.steps], dtype=t.bool)
        self.steps += 1
        return "obs%d" % self.steps, "r", done, t.zeros(self.n, dtype=t.bool), {"final_observation": "fin", "takeover": take}

    def drain_episode_stats(self):
        ret, env = self.drains.pop(0) if self.drains else ([], [])
        return {"episode_return": np.array(ret, dtype=np.float64), "env": np.array(env, dtype=np.int64)}


def _fake_learner(cls, calls, **attrs):
    L = object.__new__(cls)
    L.__dict__.update(attrs)
    L.act = lambda obs, ticks, eps=0.0: calls.append(("act", obs, eps)) or "a"
    L.push = lambda *a, **kw: calls.append(("push", a[0], a[4], kw["final_obs"]))
    L.update = lambda n, lr=None: calls.append(("update", n, lr))
    return L


def test_train_dqn_counts_takeovers_on_a_shielded_env():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    take = [[1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 0, 0]]
    done = [[0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]          # row 3 ends at tick 0, row 1 at tick 1
    # with autoreset every row lives on every tick: 4 takeovers of 18 row-ticks; members of 2 rows: (1 + 1) / 6, (1) / 6, (1) / 6
    res = learner.train_dqn(_FakeShieldedEnv(take, done, True), _fake_learner(learner.DQNPopulation, [], P=3, n_per_member=2), 18, drain_every=1)
    assert res["takeover_share"] == 4 / 18 and res["member_takeover_share"] == [2 / 6, 1 / 6, 1 / 6]
    assert set(res) == {"steps", "frames", "episodes", "mean_return", "returns", "takeover_share", "member_returns", "member_takeover_share"}
    # without autoreset a finished row idles: row 3 lives 1 tick, row 1 lives 2 -- 18 - 2 - 1 = 15 live ticks; the scripted takeover of row 1 at
    # tick 2 is what a real env never reports (takeover 0 on a finished row): the count follows info["takeover"], the live ticks the flags
    res = learner.train_dqn(_FakeShieldedEnv(take, done, False), _fake_learner(learner.DQNPopulation, [], P=3, n_per_member=2), 18, drain_every=1)
    assert res["takeover_share"] == 4 / 15 and res["member_takeover_share"] == [2 / 5, 1 / 4, 1 / 6]
    # a lone learner: the share alone; read at the drains -- the last drain is at the last step whatever drain_every is
    calls = []
    res = learner.train_dqn(_FakeShieldedEnv(take, done, False), _fake_learner(learner.DQNLearner, calls), 18, drain_every=64)
    assert res["takeover_share"] == 4 / 15 and "member_takeover_share" not in res
    assert set(res) == {"steps", "frames", "episodes", "mean_return", "returns", "takeover_share"}
    assert [c for c in calls if c[0] == "push"] == [("push", "obs%d" % i, "obs%d" % (i + 1), "fin") for i in range(3)]
    # no takeover at all is 0.0, and train_ddpg counts through the same lines
    none = [[0] * 6] * 3
    assert learner.train_dqn(_FakeShieldedEnv(none, done, True), _fake_learner(learner.DQNLearner, []), 18)["takeover_share"] == 0.0
    assert "_TakeoverShare" in inspect.getsource(learner.train_ddpg) and "_TakeoverShare" in inspect.getsource(learner.train_dqn)
    # (both name it, and both run the one loop that makes it)
    assert "_train(" in inspect.getsource(learner.train_ddpg) and "_train(" in inspect.getsource(learner.train_dqn)
    assert "_TakeoverShare(" in inspect.getsource(learner._train)


class _FakePlainEnv:
    """Today's fake unshielded env: no ``shield`` attribute, no shield keys in ``info``, nothing of torch."""
    n = 6

    def __init__(self, drains, **attrs):
        self.drains, self.steps = list(drains), 0
        self.__dict__.update(attrs)

    def reset(self):
        return "obs0"

    def step(self, action):
        self.steps += 1
        return "obs%d" % self.steps, "r", "term", "trunc", {"final_observation": "fin"}

    def drain_episode_stats(self):
        ret, env = self.drains.pop(0)
        return {"episode_return": np.array(ret, dtype=np.float64), "env": np.array(env, dtype=np.int64)}


def test_train_dqn_on_an_unshielded_env_is_what_it_was():
    """The parent's result, key for key (written out: what train_dqn returned before shields were counted), for an env without a ``shield`` attribute
    and for one whose ``shield`` is None."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    drains = [([1.0, 2.0, 3.0], [0, 5, 2]), ([4.0], [3]), ([], [])]
    for attrs in ({}, {"shield": None}):
        res = learner.train_dqn(_FakePlainEnv(drains, **attrs), _fake_learner(learner.DQNPopulation, [], P=3, n_per_member=2), 16, drain_every=1)
        want = {"steps": 3, "frames": 18, "episodes": 4, "mean_return": 2.5, "returns": np.array([1.0, 2.0, 3.0, 4.0]), "takeover_share": 0.0,
                "member_returns": [np.array([1.0]), np.array([3.0, 4.0]), np.array([2.0])]}
        assert list(res) == list(want)
        for k in want:
            if k == "member_returns":
                assert len(res[k]) == 3 and all(_same(a, b) for a, b in zip(res[k], want[k]))
            elif k == "returns":
                assert _same(res[k], want[k])
            else:
                assert res[k] == want[k] and type(res[k]) is type(want[k]), k
        res = learner.train_dqn(_FakePlainEnv(drains, **attrs), _fake_learner(learner.DQNLearner, []), 18, drain_every=1)
        assert list(res) == ["steps", "frames", "episodes", "mean_return", "returns", "takeover_share"] and res["takeover_share"] == 0.0
