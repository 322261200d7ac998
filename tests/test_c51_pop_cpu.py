"""A population of C51 learners (learner.C51Population, csrc/stmpc_c51_pop_kernels.hpp, stmpc_pop_c51_* of include/stmpc.h): CPU part.

  * header, library and binding agree on exactly the twelve new entries and their argument counts -- the issue's eleven and
    ``stmpc_pop_c51_multi_step_window``, the window read ``member(m).nstep_window`` needs and no entry of a closed prefix can take;
    STMPC_C51_POP_MAX is the other populations' maximum; the closed prefixes stmpc_c51_, stmpc_pop_dqn_, stmpc_pop_per_, stmpc_pop_nstep_ and
    stmpc_nstep_ did not grow, the ABI is still 8 and the cfg struct kept its size;
  * ``C51Population`` refuses, with a ValueError that names the member or the field and before it touches the device, a ``DQNConfig`` member,
    differing ``n_atoms``, a continuous env, a cfg carrying ``per=``, an env it cannot split, and traffic or reward groups that are not one per
    member;
  * the library refuses, without a device, P outside 1 ... max, NULL arguments and members of differing shapes (the message lists the shared
    fields, n_atoms among them);
  * ``train_dqn`` and the refusals of C51 members treat a ``C51Population`` as the issue says: member_returns, and no population of C51 policies.
The GPU part is test_c51_pop.py.
"""
import ctypes

import numpy as np
import pytest

from stmpc_testlib import capi as _capi, header_prototypes, header_text

TAILS = ("create", "destroy", "size", "member", "act_device", "push_device", "update_device", "stats_device", "per_enable", "multi_step_enable", "replay_read",
         "multi_step_window")
ENTRIES = {"stmpc_pop_c51_" + n for n in TAILS}
SHARED = "n_obs, h1, n_actions, n_atoms, batch and capacity"


def test_header_library_and_binding_agree_on_the_c51_population():
    capi = _capi()
    lib = capi.load()
    header = header_text(flat=True)
    declared = header_prototypes("stmpc_pop_c51_")
    assert len(ENTRIES) == 12 and set(declared) == ENTRIES == {n for n in capi.EXPORTS if n.startswith("stmpc_pop_c51_")}
    for name, args in declared.items():
        fn = getattr(lib, name)                                     # (AttributeError: the library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")), name
    # the signatures follow the DQN population's, with stmpc_c51_cfg and stmpc_c51
    dqn = header_prototypes("stmpc_pop_dqn_")
    for tail in TAILS:
        if tail not in ("multi_step_enable", "multi_step_window"):
            want = dqn["stmpc_pop_dqn_" + tail].replace("stmpc_dqn_pop", "stmpc_c51_pop").replace("stmpc_dqn_cfg", "stmpc_c51_cfg").replace("stmpc_dqn *", "stmpc_c51 *")
            assert declared["stmpc_pop_c51_" + tail] == want, tail
            if tail != "create":
                assert getattr(lib, "stmpc_pop_c51_" + tail).argtypes == getattr(lib, "stmpc_pop_dqn_" + tail).argtypes, tail
    assert declared["stmpc_pop_c51_multi_step_enable"] == header_prototypes("stmpc_pop_nstep_")["stmpc_pop_nstep_enable_dqn"].replace("stmpc_dqn_pop", "stmpc_c51_pop")
    assert lib.stmpc_pop_c51_multi_step_enable.argtypes == lib.stmpc_pop_nstep_enable_dqn.argtypes
    assert declared["stmpc_pop_c51_multi_step_window"] == header_prototypes("stmpc_nstep_window_")["stmpc_nstep_window_dqn"].replace("stmpc_dqn *", "stmpc_c51 *")
    assert lib.stmpc_pop_c51_multi_step_window.argtypes == lib.stmpc_nstep_window_dqn.argtypes
    assert not [n for n in ENTRIES if "nstep" in n] and {n for n in capi.EXPORTS if n.startswith("stmpc_nstep_")} == {"stmpc_nstep_enable_ddpg", "stmpc_nstep_enable_dqn", "stmpc_nstep_window_ddpg", "stmpc_nstep_window_dqn"}
    assert lib.stmpc_pop_c51_create.argtypes[1]._type_ is capi.C51Cfg
    assert lib.stmpc_pop_c51_member.restype is ctypes.c_void_p and lib.stmpc_pop_c51_destroy.restype is None
    assert "#define STMPC_C51_POP_MAX %d" % capi.C51_POP_MAX in header and capi.C51_POP_MAX == capi.DQN_POP_MAX == capi.DDPG_POP_MAX == 64
    # DG_POP_MAX, the kernels' own constant (DdpgLr and DqnEps are sized by it), and the static_assert that ties the header's to it
    csrc = lambda name: open(capi.__file__.replace("_capi.py", "csrc/" + name)).read()
    assert "constexpr int DG_POP_MAX = %d;" % capi.C51_POP_MAX in " ".join(csrc("stmpc_ddpg_pop_kernels.hpp").split())
    assert "static_assert(STMPC_C51_POP_MAX == DG_POP_MAX" in csrc("stmpc_learner.hip")
    # additive only
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8 and "#define STMPC_ABI_VERSION 8" in header
    assert ctypes.sizeof(capi.C51Cfg) == 120
    closed = {"stmpc_c51_": 22, "stmpc_pop_dqn_": 10, "stmpc_pop_per_": 2, "stmpc_pop_nstep_": 3}
    for prefix, count in closed.items():
        assert len({n for n in capi.EXPORTS if n.startswith(prefix)}) == count == len(header_prototypes(prefix)), prefix
    for name in ("create", "destroy", "size", "member", "act", "push", "update", "stats", "per_enable", "multi_step_enable", "replay_read", "multi_step_window"):
        assert callable(getattr(capi.Context, "c51_pop_" + name)), name


def test_entries_refuse_null_and_bad_counts_before_touching_a_device():
    capi = _capi()
    lib = capi.load()
    from rl_mpc_lanemerging_amd import learner
    h = ctypes.c_void_p()
    mk = lambda m, **kw: learner.C51Config(**dict(dict(n_actions=5, h1=16, batch=7, capacity=200, n_atoms=17), **kw)).to_c(m)
    cfgs = (capi.C51Cfg * 2)(mk(0), mk(1))
    one = (ctypes.c_double * 1)(0.5)
    assert lib.stmpc_pop_c51_create(None, cfgs, 2, ctypes.byref(h)) == capi.STMPC_EINVAL and not h.value
    assert lib.stmpc_pop_c51_size(None) == 0 and not lib.stmpc_pop_c51_member(None, 0)
    assert lib.stmpc_pop_c51_act_device(None, 1, None, 20, one, 1, None, None, None) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_c51_push_device(None, 1, None, None, None, 20, None, None, None, None, None) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_c51_update_device(None, 1, one, 1, None) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_c51_stats_device(None, None, None) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_c51_per_enable(None, None, None, 0) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_c51_multi_step_enable(None, None, 0) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_c51_replay_read(None, 0, 0, None) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_c51_multi_step_window(None, None, 0, None) == capi.STMPC_EINVAL
    lib.stmpc_pop_c51_destroy(None)
    # what create refuses from its arguments alone: the checks come before the context's device is selected, so a stand-in context will do
    fake = ctypes.create_string_buffer(4096)
    last = lambda: lib.stmpc_last_error().decode()
    for P in (0, -1, capi.C51_POP_MAX + 1):
        assert lib.stmpc_pop_c51_create(fake, cfgs, P, ctypes.byref(h)) == capi.STMPC_EINVAL and not h.value
        assert "a population has 1 ... 64 members, not %d" % P in last()
    assert lib.stmpc_pop_c51_create(fake, None, 2, ctypes.byref(h)) == capi.STMPC_EINVAL and "NULL argument" in last()
    assert lib.stmpc_pop_c51_create(fake, cfgs, 2, None) == capi.STMPC_EINVAL and "NULL argument" in last()
    for who, odd in ((1, dict(n_atoms=21)), (2, dict(h1=32)), (1, dict(batch=8)), (2, dict(capacity=201)), (1, dict(n_actions=20)), (2, dict(n_obs=19))):
        three = [mk(0), mk(1), mk(2)]
        three[who] = mk(who, **odd)
        assert lib.stmpc_pop_c51_create(fake, (capi.C51Cfg * 3)(*three), 3, ctypes.byref(h)) == capi.STMPC_EINVAL and not h.value
        assert "the members of a population share %s (member %d differs from member 0)" % (SHARED, who) in last(), (odd, last())


class _Env:
    """A discrete env whose context must not be asked for."""
    n, obs_dim, continuous = 72, 20, False
    action_space = {"n": 5}

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def ctx(self):
        raise AssertionError("the device was touched")


def test_c51_population_refuses_before_touching_the_device():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    assert issubclass(learner.C51Population, learner.DQNPopulation) and learner.C51Population._api == "c51_pop" and learner.C51Population._cfg_type is learner.C51Config
    assert learner.C51Population._nstep_kind == "c51" and learner.DQNPopulation._api == "dqn_pop" and learner.DQNPopulation._nstep_kind == "dqn"
    assert issubclass(learner._C51PopulationMember, learner.C51Learner) and not learner._C51PopulationMember._owns_handle
    per = learner.PERConfig(alpha=1.0, beta=0.4)
    shape = dict(n_obs=20, h1=16, batch=7, capacity=200)
    mk = lambda **kw: learner.C51Config(**dict(dict(shape, n_atoms=17), **kw))
    cfg = mk()
    # a member that is no C51Config
    with pytest.raises(ValueError, match="member 1's cfg is a DQNConfig, not a C51Config"):
        learner.C51Population(_Env(), [mk(), learner.DQNConfig(**shape), mk()])
    with pytest.raises(ValueError, match="member 0's cfg is a DQNConfig, not a C51Config"):
        learner.C51Population(_Env(), [learner.DQNConfig(**shape)] * 3)
    # differing n_atoms
    with pytest.raises(ValueError, match="member 2 has n_atoms 51, member 0 has 17.*share n_obs, h1, n_actions, n_atoms, batch and capacity"):
        learner.C51Population(_Env(), [mk(), mk(), mk(n_atoms=51)])
    # a continuous env
    with pytest.raises(ValueError, match="C51 needs a discrete action space"):
        learner.C51Population(_Env(continuous=True), (cfg, 3))
    # a cfg that carries per=, alone or as the (cfg, P) pair
    with pytest.raises(ValueError, match="member 1's cfg asks for prioritised replay.*per= argument"):
        learner.C51Population(_Env(), [mk(), mk(per=per), mk()])
    with pytest.raises(ValueError, match="member 0's cfg asks for prioritised replay"):
        learner.C51Population(_Env(), (mk(per=per), 3), per=per)
    with pytest.raises(ValueError, match="per has 2 entries, the population 3 members"):
        learner.C51Population(None, (cfg, 3), per=[per, None])
    # an env it cannot split
    with pytest.raises(ValueError, match="env.n = 70 is not a multiple of the population's 3 members"):
        learner.C51Population(_Env(n=70), (cfg, 3), per=[per, None, per])
    # G != P, R != P
    with pytest.raises(ValueError, match="the env has 2 traffic groups, the population 3 members"):
        learner.C51Population(_Env(sim_cfgs=[None, None], G=2), (cfg, 3))
    with pytest.raises(ValueError, match="the env has 4 reward groups, the population 3 members"):
        learner.C51Population(_Env(R=4), (cfg, 3))
    # another shape than the env's, and a head wider than the widest layer once the env's action count is known
    with pytest.raises(ValueError, match="member 1's cfg has n_obs 19 and 5 actions; the observation has 20 entries and there are 5 actions"):
        learner.C51Population(_Env(), [mk(), mk(n_obs=19), mk()])
    with pytest.raises(ValueError, match="n_actions \\* n_atoms = 20 \\* 52 exceeds the widest layer, 1024"):
        learner.C51Population(_Env(action_space={"n": 20}), (mk(n_atoms=52), 3))
    with pytest.raises(ValueError, match="seeds and init"):
        learner.C51Population(_Env(), (cfg, 3), seeds=[1, 2])


def test_the_binding_routes_the_populations_n_step_to_its_own_entry():
    capi = _capi()
    calls = []

    class _Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, len(a))) or 0
    ctx = object.__new__(capi.Context)
    ctx._lib, ctx._chk = _Lib(), lambda rc: None
    cfgs = [capi.NStepCfg(n_step=3, rows_per_push=24)] * 2
    ctx.pop_nstep_enable("c51", "handle", cfgs)
    ctx.pop_nstep_enable("dqn", "handle", cfgs)
    assert calls == [("stmpc_pop_c51_multi_step_enable", 3), ("stmpc_pop_nstep_enable_dqn", 3)]
    del calls[:]
    assert ctx.nstep_window("c51", "handle", [0, 1, 2]).shape == (3, 4) and ctx.nstep_window("dqn", "handle", [0]).shape == (1, 4)
    assert ctx.c51_pop_multi_step_window("handle", [5]).shape == (1, 4)
    assert calls == [("stmpc_pop_c51_multi_step_window", 4), ("stmpc_nstep_window_dqn", 4), ("stmpc_pop_c51_multi_step_window", 4)]


class _FakeEnv:
    n = 6

    def __init__(self, drains):
        self.drains, self.steps = list(drains), 0

    def reset(self):
        return "obs0"

    def step(self, action):
        self.steps += 1
        return "obs%d" % self.steps, "r", "term", "trunc", {"final_observation": "fin"}

    def drain_episode_stats(self):
        ret, env = self.drains.pop(0)
        return {"episode_return": np.array(ret, dtype=np.float64), "env": np.array(env, dtype=np.int64)}


def test_train_dqn_takes_a_c51_population_and_policy_populations_refuse_it():
    _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    calls = []
    pop = object.__new__(learner.C51Population)
    pop.__dict__.update(P=3, n_per_member=2)
    pop.act = lambda obs, ticks, eps=0.0: calls.append(("act", obs)) or "a"
    pop.push = lambda *a, **kw: calls.append(("push", a[0]))
    pop.update = lambda n, lr=None: calls.append(("update", n))
    res = learner.train_dqn(_FakeEnv([([1.0, 2.0, 3.0], [0, 5, 2]), ([4.0], [3]), ([], [])]), pop, 16, updates_per_step=2, drain_every=1)
    mr = res["member_returns"]                                      # owner = env // 2
    assert len(mr) == 3 and np.array_equal(mr[0], [1.0]) and np.array_equal(mr[1], [3.0, 4.0]) and np.array_equal(mr[2], [2.0])
    assert [c for c in calls if c[0] == "update"] == [("update", 2)] * 3
    # a population of C51 POLICIES does not exist: the three entry points refuse the views with the message they give C51 learners
    member = object.__new__(learner._C51PopulationMember)
    member.__dict__.update(handle=None, cfg=learner.C51Config(n_actions=5))
    pop.member = lambda m: member
    for who, call in (("evaluate_dqn_members", lambda: learner.evaluate_dqn_members(pop, 4)),
                      ("QActorPopulation", lambda: actor.QActorPopulation(pop, 4, None, None)),
                      ("population_of", lambda: actor.population_of(pop, 4, None, None)),
                      ("population_of", lambda: actor.population_of([member, member], 4, None, None))):
        with pytest.raises(ValueError, match="%s: members .* are categorical \\(C51\\) policies, and a population of C51 policies does not exist" % who):
            call()
