"""A population of Q-networks as policies on the GPU (``actor.QActorPopulation``, ``k_qactor_eval_pop`` of csrc/stmpc_qactor_pop_kernels.hpp,
the stmpc_pop_qactor_ entries): member m on rows [m * n_per_member, (m + 1) * n_per_member) against a lone ``actor.DQNActor`` with that member on
that slice, bit for bit -- no tolerance anywhere, the population entry calls the lone kernel's body.  Networks (n_obs, h1, A) = (20, 16, 5),
(20, 48, 20), (20, 256, 5); P in {1, 3, 4}; n_per_member in {1, 16, 17, 33}: with 17 and 33 the member boundaries fall inside a 16-row tile of the
global array and every member has a masked tail, so a missing row offset or a tail that writes into the next member shows.  States of
``golden_combined_real.npz`` with 16 vehicle slots, repeated where a case needs more than the golden's 72.

Not covered: the refusal of a member or a context on another device (one device here; the checks are two comparisons of stored device numbers)."""
import ctypes
import types

import numpy as np
import pytest

from discrete_testlib import (JERKS, NAMES, NETS, NETS_WIDE, OUT, SENTINEL, q_dyadic_policy, actor_table as _table, dev as _dev, episode_settings as _episode_settings, policy_states as _states,
                              run_policy as _run, stream as _stream, stub_env as _stub_env, transitions as _transitions, widen as _widen)
from stmpc_testlib import ACTOR_KMAX, capi as _capi, same

PS = [1, 3, 4]
N_PER = [1, 16, 17, 33]
KINDS = ("file", "online", "target", "member")


def _slice(st, sl):
    return {k: v[sl].contiguous() for k, v in st.items()}


def _accel_states(st):
    """Ego accelerations cycling through -20, 0, +20: with a table within +-0.1, an acceleration-mode row is clipped at either edge or not at all
    whatever its action is."""
    n = st["ego4"].shape[0]
    st["ego4"][:, 3] = st["ego4"].new_tensor([-20.0, 0.0, 20.0]).repeat(n // 3 + 1)[:n]
    return st


def _learner(gpu_ctx, shape, seed=5, target_period=4, updates=1, push=True):
    """A lone learner; with ``push`` 32 random transitions, then ``updates`` updates (< target_period: online and target differ)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A = shape
    L = learner.DQNLearner((n_obs, A), learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=16, capacity=64, target_period=target_period, lr=1e-2), seed=seed, ctx=gpu_ctx)
    L.action_values = _table(A)
    if push:
        L.push(*_transitions(np.random.default_rng(seed), 32, n_obs, A))
    if updates:
        L.update(updates)
    return L


def _dqn_pop(gpu_ctx, shape, seeds=(11, 12), updates=1, push=True, per=None):
    """A DQNPopulation of two members on a stub env of 2 x 16 rows, fed one step of random transitions."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A = shape
    env = _stub_env(gpu_ctx, 32, n_obs, A, _table(A))
    cfgs = [learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=16, capacity=64, target_period=4, lr=1e-2, double=bool(m)) for m in range(2)]
    pop = learner.DQNPopulation(env, cfgs, seeds=list(seeds), per=per)
    if push:
        pop.push(*_transitions(np.random.default_rng(seeds[0]), 32, n_obs, A))
    if updates:
        pop.update(updates)
    return pop


_SOURCES = {}


def _sources(gpu_ctx, shape, tmp_path_factory):
    """Per network shape, made once and never changed: a learner after one update with target_period 4, its exported file, a DQNPopulation."""
    if shape not in _SOURCES:
        L = _learner(gpu_ctx, shape)
        params = L.state_dict()["params"]
        assert params["updates"] == 1 and not np.array_equal(params["q"]["w1"], params["q_target"]["w1"])
        path = L.export_q(str(tmp_path_factory.mktemp("qpop") / "q.npz"))
        _SOURCES[shape] = {"learner": L, "file": path, "pop": _dqn_pop(gpu_ctx, shape)}
    return _SOURCES[shape]


def _make(src, kind, n, ctx, S, table, mode):
    """A DQNActor for n rows of one kind: a file actor, a view of the learner's online or target network, a view of DQNPopulation.member(1)."""
    from rl_mpc_lanemerging_amd import actor
    if kind == "file":
        return actor.DQNActor(src["file"], n, ctx, S, mode=mode, action_values=table)
    L = src["pop"].member(1) if kind == "member" else src["learner"]
    keep = L.action_values
    L.action_values = table                                         # (the view copies the table when it is made)
    try:
        return actor.DQNActor.from_learner(L, n, ctx, S, target=kind == "target", mode=mode)
    finally:
        L.action_values = keep


def _assert_members(got, lone, n_per, label):
    for m, want in enumerate(lone):
        for k in OUT:
            assert same(got[k][m * n_per:(m + 1) * n_per], want[k]), (label, "member", m, k)


# ---- 1: outputs against the lone actor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_per", N_PER)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("shape", NETS)
def test_gpu_members_equal_lone_actors(shape, P, n_per, gpu_ctx, restore_settings, tmp_path_factory):
    _members_equal_lone_actors(shape, P, n_per, gpu_ctx, tmp_path_factory)


@pytest.mark.gpu
def test_gpu_two_members_beyond_one_stride(gpu_ctx, restore_settings, tmp_path_factory):
    """The same comparison for two members of (20, 32, 40) -- a lane of k_qactor_eval_pop's argmax owns two columns, three output tiles --, 17 rows
    each, the second in acceleration mode; then two file members of discrete_testlib.q_dyadic_policy's "ties" net, whose copied columns (5, 37),
    (31, 32), (0, 39) hold the maximum on rows: the population's index there is the group's lowest column, and every output equals the lone
    actor's, bit for bit."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor
    shape = NETS_WIDE[0]
    _members_equal_lone_actors(shape, 2, 17, gpu_ctx, tmp_path_factory)
    net, S, states, feat, groups, named = q_dyadic_policy(shape, "ties")
    n_per, A = feat.shape[0], shape[2]
    path = str(tmp_path_factory.mktemp("qties") / "q.npz")
    np.savez(path, **net, action_values=_table(A))
    st = {k: torch.as_tensor(np.ascontiguousarray(np.concatenate([v, v[::-1]])), device=_dev()) for k, v in states.items()}
    tables = [_table(A, m) for m in range(2)]
    pop = _widen(actor.QActorPopulation([actor.DQNActor(path, 1, gpu_ctx, S, action_values=tables[m]) for m in range(2)], n_per, gpu_ctx, S))
    got = _run(pop, st)
    lone = [_run(_widen(actor.DQNActor(path, n_per, gpu_ctx, S, action_values=tables[m])), _slice(st, slice(m * n_per, (m + 1) * n_per))) for m in range(2)]
    _assert_members(got, lone, n_per, "ties")
    for name, rows in named.items():
        assert rows.size >= 1 and (got["action"][rows] == groups[name][0]).all() and (got["action"][2 * n_per - 1 - rows] == groups[name][0]).all(), name
    assert same(got["feat"][:n_per], feat) and same(got["jerk"][n_per:], tables[1][got["action"][n_per:]])
    gpu_ctx.check_error()


def _members_equal_lone_actors(shape, P, n_per, gpu_ctx, tmp_path_factory):
    """jerk, action, q and feat of every member equal a lone DQNActor's on that slice.  The members mix a file actor, an online view, a target view
    (after an update with target_period 4: it differs from online) and a view of a DQNPopulation's member, each with its own table; at A = 20 (and 40) the
    odd members are in acceleration mode, on states that clip at either edge and states inside.  The population is evaluated through the raw
    entry on sentinel-filled outputs with spare rows beyond P * n_per_member, which keep the sentinel."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor
    n, A = P * n_per, shape[2]
    S, st = _states(n)
    if A in (20, 40):
        _accel_states(st)
    src = _sources(gpu_ctx, shape, tmp_path_factory)
    off = N_PER.index(n_per)
    kinds = [KINDS[(m + off) % 4] for m in range(P)]
    modes = ["acceleration" if A in (20, 40) and m % 2 else "jerk" for m in range(P)]
    tables = [_table(A, m, modes[m] == "acceleration") for m in range(P)]
    members = [_make(src, kinds[m], 1, gpu_ctx, S, tables[m], modes[m]) for m in range(P)]
    pop = actor.QActorPopulation(members, n_per, gpu_ctx, S)
    assert (pop.P, pop.n_per_member, pop.n) == (P, n_per, n) and pop.members == members and gpu_ctx.qactor_pop_size(pop.handle) == P
    assert pop.jerk.shape == (n,) and pop.action.shape == (n,) and pop.q.shape == (n, A) and pop.feat.shape == (n, shape[0])
    pop.reset()
    pop.reset(torch.ones(n, dtype=torch.bool, device=_dev()))
    buf = _widen(types.SimpleNamespace(n=n, flen=pop.flen, shape=shape))
    gpu_ctx.qactor_pop_eval_device(pop.handle, pop.fcfg, n_per, ACTOR_KMAX, 1, st["ego4"].data_ptr(), st["k"].data_ptr(), st["ox"].data_ptr(), st["ov"].data_ptr(),
                                   st["oa"].data_ptr(), buf.feat.data_ptr(), pop.flen, buf.action.data_ptr(), buf.q.data_ptr(), buf.jerk.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = {k: getattr(buf, k).cpu().numpy() for k in OUT}
    for k in OUT:
        assert (got[k][n:] == SENTINEL).all() and not (got[k][:n] == SENTINEL).all(), k
    lone = [_run(_widen(_make(src, kinds[m], n_per, gpu_ctx, S, tables[m], modes[m])), _slice(st, slice(m * n_per, (m + 1) * n_per))) for m in range(P)]
    _assert_members(got, lone, n_per, (kinds, modes))
    for m in range(P):
        rows = slice(m * n_per, (m + 1) * n_per)
        if modes[m] == "jerk":
            assert same(got["jerk"][rows], tables[m][got["action"][rows]]), m
        else:
            acc = st["ego4"][rows, 3].cpu().numpy()
            want = np.clip((tables[m][got["action"][rows]] - acc) / S.TICK_LENGTH, S.MINIMUM_NEGATIVE_JERK, S.MAXIMUM_POSITIVE_JERK)
            assert same(got["jerk"][rows], want), m
            if n_per >= 3:
                j = got["jerk"][rows]
                assert (j == S.MAXIMUM_POSITIVE_JERK).any() and (j == S.MINIMUM_NEGATIVE_JERK).any() and (np.abs(j) <= 0.6).any(), m
    # the call of the class fills .jerk and .action always, .q and .feat behind their switches
    pop.q.fill_(SENTINEL)
    pop.feat.fill_(SENTINEL)
    jerk = pop(1, st["ego4"], st["k"], st["ox"], st["ov"], st["oa"])
    torch.cuda.synchronize()
    assert jerk is pop.jerk and same(jerk.cpu().numpy(), got["jerk"][:n]) and same(pop.action.cpu().numpy(), got["action"][:n])
    assert (pop.q == SENTINEL).all() and (pop.feat == SENTINEL).all()
    pop.keep_q = pop.keep_features = True
    pop(1, st["ego4"], st["k"], st["ox"], st["ov"], st["oa"])
    torch.cuda.synchronize()
    assert same(pop.q.cpu().numpy(), got["q"][:n]) and same(pop.feat.cpu().numpy(), got["feat"][:n])
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_sources_a_population_takes(gpu_ctx, restore_settings, tmp_path_factory):
    """A list of a file, a learner and an actor, and a DQNPopulation itself: the members are what DQNActor and DQNActor.from_learner make of them."""
    _capi()
    from rl_mpc_lanemerging_amd import actor
    shape, n_per = NETS[0], 17
    src = _sources(gpu_ctx, shape, tmp_path_factory)
    L = src["learner"]
    S, st = _states(3 * n_per)
    tgt = actor.DQNActor.from_learner(L, 1, gpu_ctx, S, target=True)
    pop = _widen(actor.QActorPopulation([src["file"], L, tgt], n_per, gpu_ctx, S))
    assert [a.learner for a in pop.members] == [None, L, L] and [a.target for a in pop.members] == [False, False, True] and pop.members[2] is tgt
    lone = [_run(_widen(a), _slice(st, slice(m * n_per, (m + 1) * n_per)))
            for m, a in enumerate((actor.DQNActor(src["file"], n_per, gpu_ctx, S), actor.DQNActor.from_learner(L, n_per, gpu_ctx, S),
                                   actor.DQNActor.from_learner(L, n_per, gpu_ctx, S, target=True)))]
    _assert_members(_run(pop, st), lone, n_per, "list")
    dq = src["pop"]
    S, st = _states(2 * n_per)
    pop = _widen(actor.QActorPopulation(dq, n_per, gpu_ctx, S))
    assert pop.P == 2 and [a.learner for a in pop.members] == [dq.member(0), dq.member(1)]
    lone = [_run(_widen(actor.DQNActor.from_learner(dq.member(m), n_per, gpu_ctx, S)), _slice(st, slice(m * n_per, (m + 1) * n_per))) for m in range(2)]
    _assert_members(_run(pop, st), lone, n_per, "DQNPopulation")
    gpu_ctx.check_error()


# ---- 2: liveness ---------------------------------------------------------------------------------------------------------------------------------------
def _state_equal(a, b, label):
    sa, sb = a.state_dict(), b.state_dict()
    assert np.array_equal(sa["counters"], sb["counters"]) and same(sa["params"]["beta_pow"], sb["params"]["beta_pow"]), label
    assert sa["params"]["updates"] == sb["params"]["updates"], label
    for slot in _capi().DQN_SLOTS:
        for k in NAMES:
            assert same(sa["params"][slot][k], sb["params"][slot][k]), (label, slot, k)
    assert same(a.minibatch(), b.minibatch()), label                # (the next update's rows)


@pytest.mark.gpu
def test_gpu_population_is_live_and_leaves_the_learners_alone(gpu_ctx, restore_settings):
    """Evaluate, update(3) the learners behind the views, evaluate again on the same population: the second result equals fresh lone views' (and
    differs from the first), and the learners' state_dict, exploring-call counter and next minibatch equal those of twins with the same pushes and
    updates that were never evaluated."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor
    shape, n_per = NETS[2], 17
    S, st = _states(3 * n_per)
    (La, ta), (Lb, tb) = ([_learner(gpu_ctx, shape, seed=s, target_period=2, updates=0) for _ in range(2)] for s in (3, 4))
    obs = torch.zeros(8, shape[0], dtype=torch.float32, device=_dev())
    for x in (La, ta, Lb, tb):
        x.act(obs, eps=1.0)                                         # one exploring call: the counter the evaluations must not advance
    spec = [(La, False), (Lb, True), (La, True)]
    pop = _widen(actor.QActorPopulation([actor.DQNActor.from_learner(L, 1, gpu_ctx, S, target=t) for L, t in spec], n_per, gpu_ctx, S))
    first = _run(pop, st)
    for x in (La, ta, Lb, tb):
        x.update(3)
    second = _run(pop, st)
    lone = [_run(_widen(actor.DQNActor.from_learner(L, n_per, gpu_ctx, S, target=t)), _slice(st, slice(m * n_per, (m + 1) * n_per))) for m, (L, t) in enumerate(spec)]
    _assert_members(second, lone, n_per, "after update(3)")
    assert same(second["feat"], first["feat"])
    for m in range(3):
        assert not np.array_equal(second["q"][m * n_per:(m + 1) * n_per], first["q"][m * n_per:(m + 1) * n_per]), m
    assert La.state_dict()["counters"][3] == 1 and La.state_dict()["params"]["updates"] == 3
    _state_equal(La, ta, "learner a")
    _state_equal(Lb, tb, "learner b")
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_prioritised_replay_enabled_after_the_population_was_made(gpu_ctx, restore_settings):
    """Enabling prioritised replay re-wires a learner's replay store, not its network: a population made before -- over a lone learner's views and
    over a DQNPopulation -- gives, after the enabling, a push and two updates, the bits of lone views made afterwards."""
    _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    shape, n_per = NETS[0], 17
    n_obs, h1, A = shape
    S, st = _states(2 * n_per)
    per = learner.PERConfig(alpha=0.5)
    # a lone learner: its online and its target network
    L = _learner(gpu_ctx, shape, seed=8, updates=0, push=False)
    pop = _widen(actor.QActorPopulation([actor.DQNActor.from_learner(L, 1, gpu_ctx, S, target=t) for t in (False, True)], n_per, gpu_ctx, S))
    before = _run(pop, st)
    gpu_ctx.dqn_per_enable(L.handle, per.to_c())
    L.push(*_transitions(np.random.default_rng(8), 32, n_obs, A))
    L.update(2)
    assert L.state_dict()["params"]["updates"] == 2 and L.priorities().max() > 0
    after = _run(pop, st)
    lone = [_run(_widen(actor.DQNActor.from_learner(L, n_per, gpu_ctx, S, target=t)), _slice(st, slice(m * n_per, (m + 1) * n_per))) for m, t in enumerate((False, True))]
    _assert_members(after, lone, n_per, "lone learner")
    assert not np.array_equal(after["q"][:n_per], before["q"][:n_per])
    # a DQNPopulation: member 0 prioritised, member 1 uniform
    dq = _dqn_pop(gpu_ctx, shape, seeds=(21, 22), updates=0, push=False)
    pop = _widen(actor.QActorPopulation(dq, n_per, gpu_ctx, S))
    before = _run(pop, st)
    gpu_ctx.dqn_pop_per_enable(dq.handle, [per.to_c(), None])
    dq.push(*_transitions(np.random.default_rng(21), 32, n_obs, A))
    dq.update(2)
    assert list(dq.stats()["updates"]) == [2, 2]
    after = _run(pop, st)
    lone = [_run(_widen(actor.DQNActor.from_learner(dq.member(m), n_per, gpu_ctx, S)), _slice(st, slice(m * n_per, (m + 1) * n_per))) for m in range(2)]
    _assert_members(after, lone, n_per, "DQNPopulation")
    for m in range(2):
        assert not np.array_equal(after["q"][m * n_per:(m + 1) * n_per], before["q"][m * n_per:(m + 1) * n_per]), m
    gpu_ctx.check_error()


# ---- 3: rollout steps ---------------------------------------------------------------------------------------------------------------------------------
def _two_steps(ctx, S, policy, st):
    """Step 1, one rollout step of the context with the policy's jerks, step 2 (which asks the context for a rollout of all the call's rows)."""
    from rl_mpc_lanemerging_amd import _capi as capi
    params, ccfg = capi.Params.from_settings(S), capi.CombinedCfg.from_settings(S)
    cur = {k: st[k].clone().contiguous() for k in ("ego4", "k", "ox", "ov", "oa")}
    n = cur["k"].shape[0]
    out = [_run(policy, cur, 1)]
    ctx.rollout_step_device(params, ccfg, n, ACTOR_KMAX, 1, st["ego5"].data_ptr(), cur["ego4"].data_ptr(), cur["k"].data_ptr(), cur["ox"].data_ptr(), cur["ov"].data_ptr(),
                            cur["oa"].data_ptr(), policy.jerk.data_ptr(), _stream())
    out.append(_run(policy, cur, 2))
    ctx.check_error()
    return out


@pytest.mark.gpu
def test_gpu_rollout_steps(gpu_ctx, restore_settings, tmp_path_factory):
    """Step 1, one rollout step and step 2 through the context's rollout of P * n_per_member states equal the lone actors' on their slices, each on
    a context of its own with a rollout of n_per_member states."""
    capi = _capi()
    from rl_mpc_lanemerging_amd import actor
    shape, P, n_per = NETS[2], 3, 17
    S, st = _states(P * n_per)
    src = _sources(gpu_ctx, shape, tmp_path_factory)
    kinds = ("online", "file", "target")
    tables = [_table(shape[2], m) for m in range(P)]
    pop = _widen(actor.QActorPopulation([_make(src, kinds[m], 1, gpu_ctx, S, tables[m], "jerk") for m in range(P)], n_per, gpu_ctx, S))
    got = _two_steps(gpu_ctx, S, pop, st)
    assert not np.array_equal(got[0]["feat"], got[1]["feat"])       # (the rollout moved the states)
    for m in range(P):
        ctx = capi.Context(-1)
        lone = _two_steps(ctx, S, _widen(_make(src, kinds[m], n_per, ctx, S, tables[m], "jerk")), _slice(st, slice(m * n_per, (m + 1) * n_per)))
        for step in range(2):
            for k in OUT:
                assert same(got[step][k][m * n_per:(m + 1) * n_per], lone[step][k]), ("member", m, "step", step + 1, k)


# ---- 4: the controllers and the episode runner -----------------------------------------------------------------------------------------------------
def _jerk_learner(gpu_ctx, seed=2):
    from rl_mpc_lanemerging_amd import learner
    L = learner.DQNLearner((20, 5), learner.DQNConfig(batch=16, capacity=64), seed=seed, ctx=gpu_ctx)
    L.action_values = JERKS.copy()
    return L


@pytest.mark.gpu
def test_gpu_drop_in_for_the_combined_controller(gpu_ctx, restore_settings, tmp_path_factory):
    """combined.decide_batch_device with the population returns, on member m's rows, what it returns with the lone actor on that slice."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor, combined
    shape, P, n_per = NETS[2], 3, 11
    S, st = _states(P * n_per)
    src = _sources(gpu_ctx, shape, tmp_path_factory)
    kinds = ("online", "target", "member")
    params, cfg = capi.Params.from_settings(S), capi.CombinedCfg.from_settings(S)
    assert cfg.rollout_length > 1

    def decide(policy, s):
        d = combined.decide_batch_device(gpu_ctx, params, cfg, s["ego5"], s["k"], s["ox"], s["ov"], policy, None, _stream(), d_oa=s["oa"])
        torch.cuda.synchronize()
        gpu_ctx.check_error()
        return {k: v.cpu().numpy().copy() for k, v in d.items()}
    got = decide(actor.QActorPopulation([_make(src, k, 1, gpu_ctx, S, _table(5), "jerk") for k in kinds], n_per, gpu_ctx, S), st)
    for m in range(P):
        rows = slice(m * n_per, (m + 1) * n_per)
        want = decide(_make(src, kinds[m], n_per, gpu_ctx, S, _table(5), "jerk"), _slice(st, rows))
        assert set(got) == set(want) and len(want) == 8
        for k in want:
            assert same(got[k][rows], want[k]), (m, k)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["combined", "first_step"])
def test_gpu_episode_runner_reports_members(controller, gpu_ctx, restore_settings):
    """EpisodeRunner with the population: out["member"] = env // n_per_member.  C identical members on C traffic groups with the same seed give
    identical per-group columns, which equal evaluate_dqn of that member on one such group."""
    _capi()
    from rl_mpc_lanemerging_amd import actor, episodes, learner
    S = _episode_settings()
    C, n_per = 3, 16
    L = _jerk_learner(gpu_ctx)
    traffic = [dict(episodes.traffic_settings("medium"), seed=4) for _ in range(C)]
    pop = actor.QActorPopulation([L] * C, n_per, gpu_ctx, S)
    r = episodes.EpisodeRunner(C * n_per, seed=9, controller=controller, policy=pop, ctx=gpu_ctx, kmax=ACTOR_KMAX, max_episode_length=2.0, traffic=traffic)
    for _ in range(r.max_ticks + 1):
        r.tick()
    res = r.result()
    assert np.array_equal(res["member"], np.arange(C * n_per) // n_per) and np.array_equal(res["traffic_group"], res["member"]) and "percent_st" in res
    assert (res["status"] != 0).all() and res["ticks"].max() >= 1
    want = learner.evaluate_dqn(L, n_per, seed=9, kmax=ACTOR_KMAX, max_episode_length=2.0, traffic=traffic[:1], controller=controller)
    for k, v in want.items():
        if k == "traffic_group":
            continue
        for c in range(C):
            assert same(res[k][c * n_per:(c + 1) * n_per], v), (k, "group", c)
    with pytest.raises(ValueError, match="built for 3 x 16 = 48"):
        episodes.EpisodeRunner(32, seed=9, controller=controller, policy=pop, ctx=gpu_ctx, kmax=ACTOR_KMAX)


@pytest.mark.gpu
def test_gpu_evaluate_dqn_members(gpu_ctx, restore_settings):
    """evaluate_dqn_members(DQNPopulation) with episodes of a few ticks: P summary rows, P reports with record= and None without; a lone learner is
    a population of one."""
    _capi()
    from rl_mpc_lanemerging_amd import learner, report
    _episode_settings()
    dq = _dqn_pop(gpu_ctx, NETS[2], updates=0, push=False)
    for m in range(2):
        dq.member(m).action_values = JERKS.copy()
    out = learner.evaluate_dqn_members(dq, 16, seed=1, kmax=ACTOR_KMAX, max_episode_length=2.0)
    assert set(out) == {"stats", "by_member", "reports"} and out["reports"] is None and len(out["by_member"]) == 2
    assert np.array_equal(out["stats"]["member"], np.arange(32) // 16) and (out["stats"]["status"] != 0).all() and out["stats"]["ticks"].max() <= 10
    assert all(set(row) >= {"crashed", "merged", "mean_speed", "percent_st"} for row in out["by_member"])
    out = learner.evaluate_dqn_members(dq, 16, seed=1, kmax=ACTOR_KMAX, max_episode_length=2.0, record=report.RecorderConfig(), traffic=["low", "fast"],
                                       controller="first_step")
    assert len(out["by_member"]) == 2 and len(out["reports"]) == 2 and all(isinstance(r, report.Report) for r in out["reports"])
    one = learner.evaluate_dqn_members(dq.member(1), 16, seed=1, kmax=ACTOR_KMAX, max_episode_length=2.0)
    assert len(one["by_member"]) == 1 and one["stats"]["ticks"].shape == (16,)


@pytest.mark.gpu
def test_gpu_cross_matrix_and_grid_search_take_a_q_network(gpu_ctx, restore_settings):
    """cross_matrix and grid_search_combined with a DQNLearner as the model build their population through actor.population_of: they run and
    return their shapes."""
    _capi()
    from rl_mpc_lanemerging_amd import combined, episodes
    _episode_settings()
    La, Lb = _jerk_learner(gpu_ctx, 2), _jerk_learner(gpu_ctx, 3)
    out = episodes.cross_matrix([La, Lb], ["low", "fast"], 8, seed=1, ctx=gpu_ctx, kmax=ACTOR_KMAX, max_episode_length=2.0)
    assert len(out["matrix"]) == 2 and all(len(row) == 2 for row in out["matrix"]) and out["stats"]["ticks"].shape == (32,)
    assert np.array_equal(out["stats"]["member"], np.arange(32) // 8) and all("crashed" in cell for row in out["matrix"] for cell in row)
    cells = combined.grid_search_cells()[:3]
    out = episodes.grid_search_combined(La, "medium", 8, cells=cells, seed=1, ctx=gpu_ctx, kmax=ACTOR_KMAX, max_episode_length=2.0)
    assert len(out["cells"]) == 3 and [c["settings"] for c in out["cells"]] == cells and out["stats"]["ticks"].shape == (24,)
    with pytest.raises(ValueError, match="DDPG and DQN members do not share a population"):
        episodes.cross_matrix([La, "medium1"], ["low"], 8, ctx=gpu_ctx, kmax=ACTOR_KMAX, max_episode_length=2.0)


# ---- 5: what the library refuses -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_library_refusals(gpu_ctx, restore_settings, tmp_path_factory):
    """Every refusal of the stmpc_pop_qactor_ entries is STMPC_EINVAL with a message, made before anything is launched: the outputs keep their
    sentinel.  (A member or a context on another device cannot be had with one device.)"""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor
    lib = capi.load()
    P, n_per = 3, 17
    n = P * n_per
    S, st = _states(n)
    src = _sources(gpu_ctx, NETS[0], tmp_path_factory)
    L = src["learner"]
    a = [actor.DQNActor.from_learner(L, 1, gpu_ctx, S, target=bool(m % 2)) for m in range(P)]
    h = ctypes.c_void_p()

    def create(handles, count=None, ctx=gpu_ctx._h, arr=True):
        vals = [x.value if isinstance(x, ctypes.c_void_p) else x for x in handles]
        ptr = (ctypes.c_void_p * max(len(vals), 1))(*vals) if arr else None
        return lib.stmpc_pop_qactor_create(ctx, ptr, len(vals) if count is None else count, ctypes.byref(h))

    def refused(rc, word):
        msg = lib.stmpc_last_error().decode()
        assert rc == capi.STMPC_EINVAL and word in msg, (rc, word, msg)
        assert not h.value                                          # no handle came back
    hs = [x.handle for x in a]
    refused(create(hs, ctx=ctypes.c_void_p()), "NULL")
    refused(create(hs, arr=False), "NULL")
    assert lib.stmpc_pop_qactor_create(gpu_ctx._h, (ctypes.c_void_p * 3)(*[x.value for x in hs]), 3, None) == capi.STMPC_EINVAL
    refused(create(hs, count=0), "1 ... 64 members, not 0")
    refused(create(hs * 22, count=65), "1 ... 64 members, not 65")
    refused(create([hs[0], None, hs[2]]), "member 1 is NULL")
    other = actor.DQNActor.from_learner(_sources(gpu_ctx, NETS[1], tmp_path_factory)["learner"], 1, gpu_ctx, S)
    refused(create([hs[0], hs[1], other.handle]), "member 2 differs from member 0")
    wide = actor.DQNActor.from_learner(_sources(gpu_ctx, NETS[2], tmp_path_factory)["learner"], 1, gpu_ctx, S)      # (the same n_in and n_actions, another hidden width)
    refused(create([hs[0], wide.handle]), "member 1 differs from member 0")
    raw = gpu_ctx.qactor_view_dqn(L.handle, L.action_values, mode=capi.QACTOR_MODES["acceleration"])
    refused(create([hs[0], raw]), "member 1 is in acceleration mode and needs")
    gpu_ctx.qactor_set_limits(raw, 0.2, -1.0, 1.0)
    assert create([hs[0], raw]) == capi.STMPC_OK and h.value and lib.stmpc_pop_qactor_size(h) == 2
    lib.stmpc_pop_qactor_destroy(h)
    h.value = None
    # the evaluation
    pop = _widen(actor.QActorPopulation(a, n_per, gpu_ctx, S))
    args = lambda **kw: {**dict(handle=pop.handle, fcfg=pop.fcfg, n_per_member=n_per, Kmax=ACTOR_KMAX, step=1, d_cur_ego4=st["ego4"].data_ptr(), d_k=st["k"].data_ptr(),
                                d_cur_ox=st["ox"].data_ptr(), d_cur_ov=st["ov"].data_ptr(), d_cur_oa=st["oa"].data_ptr(), d_feat=pop.feat.data_ptr(), feat_stride=pop.flen,
                                d_action=pop.action.data_ptr(), d_q=pop.q.data_ptr(), d_jerk=pop.jerk.data_ptr(), stream=_stream()), **kw}
    timed = capi.FeaturesCfg.from_settings(S, time_feature=True)
    wider = capi.FeaturesCfg.from_settings(S, time_feature=False)
    wider.cars_ahead += 1
    for kw, word in ((dict(n_per_member=-1), "n_per_member"), (dict(n_per_member=2 ** 30), "n_per_member"), (dict(fcfg=timed), "time feature"),
                     (dict(fcfg=wider), "input width"), (dict(feat_stride=pop.flen - 1), "feat_stride"), (dict(d_jerk=0), "NULL"), (dict(d_cur_ego4=0), "NULL"),
                     (dict(d_k=0), "NULL"), (dict(d_cur_ox=0), "NULL"), (dict(handle=None), "NULL"), (dict(step=0), "step"), (dict(Kmax=33), "Kmax")):
        with pytest.raises(capi.StmpcError) as err:
            gpu_ctx.qactor_pop_eval_device(**args(**kw))
        assert err.value.code == capi.STMPC_EINVAL and word in str(err.value), (kw, str(err.value))
    with pytest.raises(capi.StmpcError, match="rollout"):          # step 2 asks for the context's rollout of P * n_per_member states, and a new context has none
        capi.Context(-1).qactor_pop_eval_device(**args(step=2))
    assert lib.stmpc_pop_qactor_eval_device(gpu_ctx._h, pop.handle, None, n_per, ACTOR_KMAX, 1, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0, 0) == capi.STMPC_EINVAL
    assert lib.stmpc_pop_qactor_eval_device(None, pop.handle, ctypes.byref(pop.fcfg), n_per, ACTOR_KMAX, 1, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0, 0) == capi.STMPC_EINVAL
    gpu_ctx.qactor_pop_eval_device(**args(n_per_member=0))          # no rows: accepted, and nothing is launched
    gpu_ctx.qactor_pop_eval_device(**args(n_per_member=0, d_jerk=0, d_cur_ego4=0))
    torch.cuda.synchronize()
    for t in (pop.feat, pop.q, pop.action, pop.jerk):
        assert (t == SENTINEL).all()                                # nothing ran
    gpu_ctx.qactor_pop_eval_device(**args())                        # ... and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert not (pop.jerk[:n] == SENTINEL).any() and (pop.jerk[n:] == SENTINEL).all()
    gpu_ctx.qactor_destroy(raw)
    gpu_ctx.check_error()
