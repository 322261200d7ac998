"""A population of categorical (C51) policies (``actor.C51ActorPopulation``, ``learner.evaluate_c51_members``, the entry stmpc_pop_c51actor_create)
without a GPU: header, library and binding agree on the one new entry and the closed prefixes keep their counts; the library's refusals that need no
device; every Python refusal, on stand-ins whose context fails the test when touched; the dispatch of ``episodes.cross_matrix`` and
``grid_search_combined``; the old entry points keep refusing C51 members.  There is no new host twin: a member's arithmetic is
``actor.c51_policy_host``'s on its slice, which the last test states on a small problem.  The GPU part is test_c51actor_pop.py."""
import ctypes
import types

import numpy as np
import pytest

from discrete_testlib import (C51_ACTOR_SHAPES as SHAPES, NEGATIVE_SUPPORT, SUPPORT, NoLibrary, actor_table as _table, c51_actor_net as _net, c51_actor_stub,
                              c51_learner_stub, export_file)
from stmpc_testlib import capi as _capi, header_entries, header_prototypes, header_text

ENTRY = "stmpc_pop_c51actor_create"


def test_header_library_and_binding_agree_on_the_one_new_entry():
    capi = _capi()
    lib = capi.load()
    protos = header_prototypes("stmpc_pop_c51actor_")
    assert set(protos) == {ENTRY} == header_entries("stmpc_pop_c51actor_") == {n for n in capi.EXPORTS if n.startswith("stmpc_pop_c51actor_")}
    args = protos[ENTRY]
    assert len(args.split(",")) == 4 == len(lib.stmpc_pop_c51actor_create.argtypes), args
    assert "const stmpc_qactor *const *members" in args and "int P" in args and "stmpc_qactor_pop **out" in args
    assert lib.stmpc_pop_c51actor_create.argtypes == lib.stmpc_pop_qactor_create.argtypes
    assert callable(capi.Context.c51actor_pop_create)
    # the closed prefixes keep their counts, in the header and in the binding; the name holds neither "noisy" nor "nstep"
    for prefix, count in (("stmpc_c51_", 22), ("stmpc_c51actor_", 2), ("stmpc_pop_c51_", 12), ("stmpc_pop_qactor_", 4)):
        assert len(header_entries(prefix)) == count == len([n for n in capi.EXPORTS if n.startswith(prefix)]), prefix
    assert "noisy" not in ENTRY and "nstep" not in ENTRY
    assert header_entries("stmpc_pop_") == {n for n in capi.EXPORTS if n.startswith("stmpc_pop_")}
    assert header_entries("stmpc_") - {"stmpc_params", "stmpc_stats", "stmpc_ctx"} == set(capi.EXPORTS)
    for name in capi.EXPORTS:
        getattr(lib, name)                                          # (AttributeError: the library does not export it)
    flat = header_text(flat=True)
    assert "#define STMPC_ABI_VERSION 8" in flat and capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8
    # the entry names the reference's function it stands for; the header says why the device table stays valid
    doc = flat[flat.index("A population of categorical (C51) policies"):flat.index("int stmpc_pop_c51actor_create(")]
    at = doc.index(ENTRY + " ")
    assert "dqn.py:375-380" in doc[at:at + 120] and "rainbow.py" in doc[at:at + 160]
    doc = doc.replace(" * ", " ")                                   # (the comment's line starts)
    for words in ("fixed from stmpc_c51_create to stmpc_c51_destroy", "stmpc_c51_per_enable", "stmpc_pop_c51_per_enable", "stmpc_c51_multi_step_enable",
                  "stmpc_pop_c51_multi_step_enable", "stmpc_noisy_c51_enable", "evaluates mu", "stmpc_pop_qactor_create keeps refusing a categorical member"):
        assert words in doc, words


def test_the_entry_refuses_before_touching_a_device():
    capi = _capi()
    lib = capi.load()
    h = ctypes.c_void_p(5)
    bogus = ctypes.c_void_p(8)                                      # a context the checks in front of the device never read
    one = (ctypes.c_void_p * 1)(None)

    def refused(rc, word):
        assert rc == capi.STMPC_EINVAL and word in lib.stmpc_last_error().decode(), (word, lib.stmpc_last_error())
        assert not h.value                                          # *out is NULL after a refusal
        h.value = 5
    refused(lib.stmpc_pop_c51actor_create(None, one, 1, ctypes.byref(h)), "NULL")
    refused(lib.stmpc_pop_c51actor_create(bogus, None, 1, ctypes.byref(h)), "NULL")
    refused(lib.stmpc_pop_c51actor_create(bogus, one, 0, ctypes.byref(h)), "1 ... 64 members, not 0")
    refused(lib.stmpc_pop_c51actor_create(bogus, one, 65, ctypes.byref(h)), "1 ... 64 members, not 65")
    refused(lib.stmpc_pop_c51actor_create(bogus, one, -1, ctypes.byref(h)), "1 ... 64 members, not -1")
    refused(lib.stmpc_pop_c51actor_create(bogus, one, 1, ctypes.byref(h)), "member 0 is NULL")
    assert lib.stmpc_pop_c51actor_create(bogus, one, 1, None) == capi.STMPC_EINVAL and b"NULL" in lib.stmpc_last_error()


def _dqn_learner_stub(n_obs=20, h1=16, A=5):
    from rl_mpc_lanemerging_amd import learner
    return types.SimpleNamespace(cfg=learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1), action_values=np.arange(float(A)), handle=None, export_q=lambda path: path)


def _c51_stub(shape, **cfg):
    L = c51_learner_stub(shape)
    for k, v in cfg.items():
        setattr(L.cfg, k, v)
    return L


def _actor_stub(shape, dueling=False):
    a = c51_actor_stub(shape)
    a.n_atoms, a.dueling = shape[3], dueling
    return a


def test_c51_actor_population_refuses_before_any_device_call(tmp_path):
    _capi()
    from rl_mpc_lanemerging_amd import Settings, actor, learner
    assert issubclass(actor.C51ActorPopulation, actor.QActorPopulation) and "__init__" in vars(actor.C51ActorPopulation)
    for name in ("__call__", "reset", "__del__"):
        assert name not in vars(actor.C51ActorPopulation), name    # (the parent's)
    ctx, shape = NoLibrary(), SHAPES[0]
    L = c51_learner_stub(shape)
    make = lambda members, n=4: actor.C51ActorPopulation(members, n, ctx, Settings)
    with pytest.raises(ValueError, match="1 ... 64 members, not 0"):
        make([])
    with pytest.raises(ValueError, match="1 ... 64 members, not 65"):
        make([L] * 65)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_per_member must be positive"):
            make([L, L], bad)
    # a DQN member -- a learner, an actor, a file -- is pointed to QActorPopulation
    dqn_file = tmp_path / "q.npz"
    np.savez(dqn_file, **learner.init_q_net(20, 16, 5, np.random.default_rng(0)), action_values=_table(5))
    dqn_actor = object.__new__(actor.DQNActor)
    dqn_actor.shape, dqn_actor.handle = (20, 16, 5), None
    for other in (_dqn_learner_stub(), dqn_actor, str(dqn_file), dqn_file):
        with pytest.raises(ValueError, match="member 1 is a Q-network .*QActorPopulation"):
            make([L, other])
    # a member of another kind
    for other in (object.__new__(actor.DDPGActor), types.SimpleNamespace(export_actor=None, handle=None), 3.5, "no_such_file.npz"):
        with pytest.raises(ValueError, match="a member is a C51Learner.export_q file, a C51Learner or a C51Actor"):
            make([L, other])
    # shapes: n_in, the padded hidden width, A, n_atoms and the head, of a learner, a file and an actor against member 0 (h1 = 16 and 12 share the padded width)
    wide = (20, 48, 5, 17)
    wide_file = export_file(tmp_path / "wide.npz", _net(wide, 0), wide)
    atoms = (20, 16, 5, 33)
    atoms_file = export_file(tmp_path / "atoms.npz", _net(atoms, 0), atoms)
    duel_net = _net((20, 16, 6, 17), 0)                             # (A + 1) K = 102 rows: a dueling head of 5 actions
    duel_file = tmp_path / "duel.npz"
    np.savez(duel_file, **duel_net, action_values=_table(5), n_atoms=np.int64(17), v_min=np.float64(-10), v_max=np.float64(10), dueling=np.int64(1))
    first = "member 0 is 20 -> 16 -> 5 x 17 atoms:"
    for other, text in ((_c51_stub(wide), "20 -> 48 -> 5 x 17 atoms"), (wide_file, "20 -> 48 -> 5 x 17 atoms"), (_actor_stub(wide), "20 -> 48 -> 5 x 17 atoms"),
                        (_c51_stub((19, 16, 5, 17)), "19 -> 16 -> 5 x 17 atoms"), (_c51_stub((20, 16, 3, 17)), "20 -> 16 -> 3 x 17 atoms"),
                        (_c51_stub(atoms), "20 -> 16 -> 5 x 33 atoms"), (atoms_file, "20 -> 16 -> 5 x 33 atoms"), (_actor_stub(atoms), "20 -> 16 -> 5 x 33 atoms"),
                        (_c51_stub(shape, dueling=True), "20 -> 16 -> 5 x 17 atoms \\(dueling\\)"), (str(duel_file), "20 -> 16 -> 5 x 17 atoms \\(dueling\\)"),
                        (_actor_stub(shape, dueling=True), "20 -> 16 -> 5 x 17 atoms \\(dueling\\)")):
        with pytest.raises(ValueError, match="member 2 is %s, %s" % (text, first)):
            make([L, _c51_stub((20, 12, 5, 17)), other])
    bad_file = tmp_path / "bad.npz"
    np.savez(bad_file, **_net(shape, 0), action_values=_table(5), n_atoms=np.int64(16), v_min=np.float64(-10), v_max=np.float64(10))      # 85 rows, 16 atoms
    with pytest.raises(ValueError, match="member 1: the last layer has 85 rows"):
        make([L, str(bad_file)])
    # a C51Population is taken member by member
    pop = types.SimpleNamespace(P=3, member=lambda m: [L, L, 7][m])
    with pytest.raises(ValueError, match="not 7"):
        make(pop)


def test_evaluate_c51_members_refusals(monkeypatch, tmp_path):
    _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    monkeypatch.setattr(learner._capi, "Context", lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))
    monkeypatch.setattr(actor, "C51ActorPopulation", lambda *a: (_ for _ in ()).throw(AssertionError("a population was built")))
    L = c51_learner_stub(SHAPES[0])
    with pytest.raises(ValueError, match="'combined' or 'first_step', not 'st'"):
        learner.evaluate_c51_members([L, L], 4, controller="st")
    with pytest.raises(ValueError, match="3 traffic groups for 2 members"):
        learner.evaluate_c51_members([L, L], 4, traffic=["low", "medium", "fast"])
    pop = object.__new__(learner.C51Population)
    pop.P = 2
    with pytest.raises(ValueError, match="3 traffic groups for 2 members"):
        learner.evaluate_c51_members(pop, 4, traffic=["low", "medium", "fast"])
    with pytest.raises(ValueError, match="2 traffic groups for 1 members"):
        learner.evaluate_c51_members(L, 4, traffic=["low", "medium"])
    # a C51Actor (a DQNActor's subclass) and an export_q file in a list pass the kind check: the call gets as far as the traffic count
    c51_file = export_file(tmp_path / "c51.npz", _net(SHAPES[0], 0), SHAPES[0])
    for members in ([c51_actor_stub(SHAPES[0])], [L, c51_actor_stub(SHAPES[0]), c51_file]):
        with pytest.raises(ValueError, match="%d traffic groups for %d members" % (len(members) + 1, len(members))):
            learner.evaluate_c51_members(members, 4, traffic=["low"] * (len(members) + 1))
    # DQN members go to evaluate_dqn_members
    with pytest.raises(ValueError, match="members 1 are Q-networks.*evaluate_dqn_members"):
        learner.evaluate_c51_members([L, _dqn_learner_stub()], 4)
    with pytest.raises(ValueError, match="members 0 are Q-networks.*evaluate_dqn_members"):
        learner.evaluate_c51_members(_dqn_learner_stub(), 4)
    with pytest.raises(ValueError, match="a DQNPopulation's members are Q-networks.*evaluate_dqn_members"):
        learner.evaluate_c51_members(object.__new__(learner.DQNPopulation), 4)
    # the keywords are evaluate_dqn_members'
    import inspect
    assert str(inspect.signature(learner.evaluate_c51_members)) == str(inspect.signature(learner.evaluate_dqn_members))


def test_cross_matrix_and_grid_search_dispatch_on_c51_models(monkeypatch, tmp_path):
    """Every model a C51 policy: a C51ActorPopulation of the cells' members; otherwise population_of, which refuses a mix."""
    _capi()
    from rl_mpc_lanemerging_amd import actor, episodes
    calls = []

    class Stop(Exception):
        pass

    def built(kind):
        def f(members, n, ctx, S, **kw):
            calls.append((kind, list(members), n))
            raise Stop()
        return f
    monkeypatch.setattr(actor, "C51ActorPopulation", built("c51"))
    monkeypatch.setattr(actor, "QActorPopulation", built("q"))
    shape = SHAPES[0]
    L, A, D = c51_learner_stub(shape), _actor_stub(shape), _dqn_learner_stub()
    ctx = NoLibrary()
    with pytest.raises(Stop):
        episodes.cross_matrix([L, A], ["low", "fast"], 8, ctx=ctx)
    assert calls.pop() == ("c51", [L, L, A, A], 8)
    with pytest.raises(Stop):
        episodes.grid_search_combined(L, "medium", 8, cells=[{}, {}, {}], ctx=ctx)
    assert calls.pop() == ("c51", [L, L, L], 8)
    with pytest.raises(Stop):
        episodes.cross_matrix([D], ["low"], 8, ctx=ctx)
    assert calls.pop() == ("q", [D], 8)
    for mix in ([L, D], [D, A]):
        with pytest.raises(ValueError, match="population_of: members .* are categorical \\(C51\\) policies, and a population of C51 policies does not exist"):
            episodes.cross_matrix(mix, ["low"], 8, ctx=ctx)
    assert not calls
    assert actor.all_c51([L, A]) and not actor.all_c51([]) and not actor.all_c51([L, D]) and not actor.all_c51([D])


@pytest.mark.parametrize("kind", ["file", "learner", "actor"])
def test_the_old_entry_points_still_refuse_c51_members(kind, tmp_path, monkeypatch):
    capi = _capi()
    from rl_mpc_lanemerging_amd import Settings, actor, learner
    shape = SHAPES[0]
    member = {"file": lambda: export_file(tmp_path / "c51.npz", _net(shape, 0), shape), "learner": lambda: c51_learner_stub(shape), "actor": lambda: c51_actor_stub(shape)}[kind]()
    monkeypatch.setattr(capi, "Context", lambda *a, **k: NoLibrary())
    for who, call in (("QActorPopulation", lambda: actor.QActorPopulation([member], 2, NoLibrary(), Settings)),
                      ("population_of", lambda: actor.population_of([member], 2, NoLibrary(), Settings)),
                      ("evaluate_dqn_members", lambda: learner.evaluate_dqn_members([member], 2))):
        with pytest.raises(ValueError) as err:
            call()
        msg = str(err.value)
        assert msg.startswith(who + ": members 0 are categorical (C51) policies, and a population of C51 policies does not exist"), msg
        assert "evaluate_dqn or a C51Actor" in msg
        # ... and behind those words, the new class and function
        assert msg.index("C51ActorPopulation") > msg.index("evaluate_dqn or a C51Actor") and "evaluate_c51_members" in msg


def test_a_members_arithmetic_is_c51_policy_host_on_its_slice():
    """No new host twin: the population's contract is rows [m * n_per_member, (m + 1) * n_per_member) = c51_policy_host(member m's net, table, mode
    and support) on that slice.  Three members of one shape with their own nets, tables and supports (one wholly below zero), the last in
    acceleration mode: the twin on a slice sees nothing of the other members -- it equals the twin on the slice taken alone, and a row of one
    member under another member's support or table differs.  (A statement of the contract on the existing twin: it says nothing about the new kernel.)"""
    _capi()
    from rl_mpc_lanemerging_amd import actor
    S = types.SimpleNamespace(TICK_LENGTH=0.25, MINIMUM_NEGATIVE_JERK=-4.0, MAXIMUM_POSITIVE_JERK=2.0)
    shape, n_per, P = SHAPES[0], 17, 3
    n_in, h1, A, K = shape
    rng = np.random.default_rng(5)
    feat = rng.normal(0, 1, (P * n_per, n_in)).astype(np.float32)
    acc = rng.normal(0, 1, P * n_per)
    nets = [_net(shape, 40 + m) for m in range(P)]
    supports = [SUPPORT, NEGATIVE_SUPPORT, (-2.0, 6.0)]
    modes = ["jerk", "jerk", "acceleration"]
    tables = [_table(A, m, modes[m] == "acceleration") for m in range(P)]

    def member(m, rows):
        return actor.c51_policy_host(nets[m], feat[rows], tables[m], modes[m], K, *supports[m], ego_acc=acc[rows], S=S)
    for m in range(P):
        rows = slice(m * n_per, (m + 1) * n_per)
        q, idx, jerk = member(m, rows)
        assert q.shape == (n_per, A) and idx.shape == (n_per,) and jerk.shape == (n_per,)
        whole = member(m, slice(None))                              # the same member on every row: its slice is the slice's own result
        for got, want in zip((q, idx, jerk), whole):
            assert np.array_equal(got, want[rows]), m
        assert idx.min() >= 0 and idx.max() < A
        if modes[m] == "jerk":
            assert np.array_equal(jerk, tables[m][idx])
        else:
            assert np.array_equal(jerk, np.clip((tables[m][idx] - acc[rows]) / 0.25, -4.0, 2.0))
        other = (m + 1) % P
        assert not np.array_equal(q, actor.c51_policy_host(nets[m], feat[rows], tables[m], "jerk", K, *supports[other])[0])
    assert (member(1, slice(n_per, 2 * n_per))[0] < 0).all()
