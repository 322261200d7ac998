"""A population of DQN learners on the GPU (learner.DQNPopulation, csrc/stmpc_dqn_pop_kernels.hpp, stmpc_pop_dqn_*).  CPU part: test_dqn_pop_cpu.py.

Every comparison is bit equality against the lone ``DQNLearner``: the population's kernels are the lone learner's bodies on the member
``blockIdx.y`` selects.  This file contains no tolerance.

Shapes (n_obs, h1, A, B): (20, 16, 5, 7) and (20, 48, 20, 33) of test_dqn.py's list (the second on sumo-accel-v0), the reference's own
(20, 256, 5, 50) once; rings of at most 256 rows.

The gate in test 1.  A learner's ``replay_start`` must lie below its capacity, and the members of a population share the capacity and the frames per
step.  With capacity 200 (so that every ring wraps) and 12 steps of 24 frames member 2 has the largest legal one, 199: its gate is shut during steps
1 ... 8 and opens at step 9, so the update counts are 12, 10 and 4.  A gate that stays shut THROUGHOUT is test 3's.
"""
import numpy as np
import pytest

from discrete_testlib import (DQN as HEAD, LR, NAMES, PERIOD, Q_SLOTS, WIDE_A, assert_population_run, assert_same as _assert_same, feed as _feed, run_population,
                              same_slots as _same_slots, snapshot as _snapshot, stats_row as _stats_row, stub_env as _stub_env, syn_steps)
from learner_testlib import CAP, N_PER, STEPS, bits64, dev as _dev
from stmpc_testlib import actor_settings, actor_states, bits as _bits, capi as _capi

SEEDS = (11, 12, 13)
REPLAY_START = (0, 48, CAP - 1)                # (module text: 199 is the largest a ring of 200 allows)
EPS = (0.0, 0.3, 1.0)
CASES = [pytest.param((20, 16, 5, 7), id="20-16-5-B7"), pytest.param((20, 48, 20, 33), id="20-48-20-B33-accel"), pytest.param((20, 256, 5, 50), id="20-256-5-B50")]
_cache = {}


# ---- 1, 2, 3: a population on a real env next to lone learners on its slices -----------------------------------------------------------------------------
def _run(gpu_ctx, shape, P, seeds=SEEDS, eps=EPS, replay_start=REPLAY_START, **kw):
    """discrete_testlib.run_population under this module's seeds, eps and replay_start."""
    return run_population(gpu_ctx, HEAD, shape, P, seeds=seeds, eps=eps, replay_start=replay_start, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CASES)
def test_gpu_population_equals_its_members_run_alone(shape, gpu_ctx, restore_settings):
    """P = 3, n = 24 (no multiple of the 16-row acting tile), capacity 200 (every ring wraps), members that differ in seed, gamma, lr, double
    (True, False, True), clip_targets (False, True, False), target_period (1, 3, 5), replay_start (0, 48, 199) and eps (0.0, 0.3, 1.0)."""
    _capi()
    snaps = _cache[shape] = _run(gpu_ctx, shape, 3)
    assert_population_run(snaps, PERIOD)


@pytest.mark.gpu
def test_gpu_members_are_independent(gpu_ctx, restore_settings):
    """Only member 1's seed, target_period and eps change: members 0 and 2 end bit-identical to before, member 1 does not."""
    _capi()
    shape = (20, 16, 5, 7)
    before = _cache.get(shape) or _run(gpu_ctx, shape, 3, alone=False)
    after = _run(gpu_ctx, shape, 3, seeds=(SEEDS[0], 99, SEEDS[2]), target_period=(PERIOD[0], 2, PERIOD[2]), eps=(EPS[0], 0.6, EPS[2]), alone=False)
    _assert_same(before[0], after[0], "member 0")
    _assert_same(before[2], after[2], "member 2")
    assert not np.array_equal(before[1]["ring"], after[1]["ring"])
    assert not np.array_equal(before[1]["params"]["q"]["w1"], after[1]["params"]["q"]["w1"])
    assert not np.array_equal(before[1]["params"]["q_target"]["w1"], after[1]["params"]["q_target"]["w1"])


@pytest.mark.gpu
def test_gpu_population_of_one_and_shut_gates(gpu_ctx, restore_settings):
    """P = 1 equals a DQNLearner; a population is a no-op before any push; a gate shut throughout (replay_start = capacity - 1 with fewer frames
    pushed) leaves that member at 0 updates with every slot as it started."""
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    shape = (20, 16, 5, 7)
    one = _run(gpu_ctx, shape, 1, seeds=(SEEDS[1],), eps=(0.3,))
    assert int(one[0]["counters"][2]) == STEPS and int(one[0]["counters"][3]) == STEPS
    # before any push: nothing to sample, so nothing moves
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(N_PER, env_id="sumo-jerk-v0", seed=7, ctx=gpu_ctx)
    pop = learner.DQNPopulation(env, [HEAD.cfg(shape, 0, capacity=CAP, replay_start=REPLAY_START[0], lr=LR[0])], seeds=[5])
    first = pop.member(0).state_dict()
    pop.update(3)
    sd, st = pop.member(0).state_dict(), pop.stats()
    assert _same_slots(sd["params"], first["params"]) and np.array_equal(sd["counters"], first["counters"]) and not sd["counters"].any()
    assert list(st["updates"]) == [0] and list(st["fill"]) == [0]
    # shut throughout: 5 steps of 24 frames against replay_start 199
    shut = _run(gpu_ctx, shape, 1, seeds=(5,), eps=(1.0,), replay_start=(CAP - 1,), steps=5)
    c = shut[0]["counters"]
    assert (int(c[1]), int(c[2]), int(c[3]), int(c[4])) == (5 * N_PER, 0, 5, 5 * N_PER)
    assert _same_slots(shut[0]["params"], first["params"]) and np.array_equal(shut[0]["params"]["beta_pow"], np.ones(2, np.float32))


# ---- 4, 5: synthetic rings: rows pushed through a stub env --------------------------------------------------------------------------------------------
SYN = (20, 48, 20, 16)                         # (n_obs, h1, A, B): two hidden k blocks, an A that crosses an output tile, one minibatch tile
SYN_RING, SYN_N, SYN_PUSHES = 128, 32, 5       # 160 rows into 128: the rings (and the trees' leaves) wrap


def _syn_cfgs(per=(None, None, None), shape=SYN, **kw):
    A = shape[2]
    return [HEAD.cfg(shape, m, n_actions=A, capacity=SYN_RING, lr=1e-3, per=per[m], **kw) for m in range(3)]


def _syn_steps(P=3, shape=SYN):
    return syn_steps(HEAD, shape, P, SYN_PUSHES, SYN_N)


def _syn_pop(gpu_ctx, per=None, steps=None, shape=SYN, P=3):
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = shape
    pop = learner.DQNPopulation(_stub_env(gpu_ctx, P * SYN_N, n_obs, A), _syn_cfgs(shape=shape)[:P], seeds=list(SEEDS[:P]), per=per)
    for step in steps if steps is not None else _syn_steps(P, shape):
        _feed(pop, step)
    return pop


def _syn_lone(gpu_ctx, m, per=None, steps=None, shape=SYN):
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = shape
    L = learner.DQNLearner((n_obs, A), _syn_cfgs(per=[per] * 3, shape=shape)[m], seed=SEEDS[m], ctx=gpu_ctx)
    for step in steps if steps is not None else _syn_steps(shape=shape):
        _feed(L, step, slice(m * SYN_N, (m + 1) * SYN_N))
    return L


@pytest.mark.gpu
def test_gpu_two_members_beyond_one_stride(gpu_ctx, restore_settings):
    """(20, 32, 40, 16) of WIDE_A -- three output tiles, stored actions of 32 and more, a lane of the argmax with two columns --: two members with
    different seeds, gamma, double (True, False), clip_targets and target_period (1, 3) equal the lone learners bit for bit after the pushes and after
    each of four updates (member 1's hard copy is update 3's); the acting entry on the pushed observations too, greedy and exploring."""
    _capi()
    import torch
    shape = WIDE_A["dqn"][0]
    steps = _syn_steps(2, shape)
    assert max(int(s["action"].max()) for s in steps) >= 32
    pop = _syn_pop(gpu_ctx, None, steps, shape=shape, P=2)
    lone = [_syn_lone(gpu_ctx, m, None, steps, shape=shape) for m in range(2)]
    obs = _dev(steps[0]["obs"])
    for eps in (0.0, 0.5):
        a = pop.act(obs, None, eps=eps).clone()
        assert torch.equal(a, torch.cat([lone[m].act(obs[m * SYN_N:(m + 1) * SYN_N], None, eps=eps) for m in range(2)])) and int(a.max()) < shape[2]
    for u in range(5):
        for m, L in enumerate(lone):
            _assert_same(_snapshot(gpu_ctx, HEAD, pop.member(m), _stats_row(pop.stats(), m)), _snapshot(gpu_ctx, HEAD, L, _stats_row(L.stats())), "member %d after %d updates" % (m, u))
            assert u == 0 or not _same_slots(pop.member(m).state_dict()["params"], first[m])
        if u == 0:
            first = [pop.member(m).state_dict()["params"] for m in range(2)]
        if u < 4:
            pop.update(1)
            for L in lone:
                L.update(1)
    sd = pop.member(1).state_dict()["params"]
    assert list(pop.stats()["updates"]) == [4, 4] and not all(np.array_equal(sd["q_target"][k], sd["q"][k]) for k in NAMES)      # copied at update 3, stepped at 4
    assert not _same_slots(pop.member(0).state_dict()["params"], sd)
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_prioritised_members(gpu_ctx, restore_settings):
    """per = [alpha 0.5, None, alpha 1 with beta]: each prioritised member's tree, last_sample and parameters equal the lone
    DQNLearner(cfg with per=) after the pushes and after each of four updates; the uniform member equals the member of a population without per."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    per = [learner.PERConfig(alpha=0.5), None, learner.PERConfig(alpha=1.0, beta=0.4)]
    steps = _syn_steps()
    pop, plain = _syn_pop(gpu_ctx, per, steps), _syn_pop(gpu_ctx, None, steps)
    assert pop.per == per and plain.per == [None] * 3
    lone = {m: _syn_lone(gpu_ctx, m, per[m], steps) for m in (0, 2)}
    for m, L in lone.items():
        assert np.array_equal(bits64(pop.member(m).priorities()), bits64(L.priorities())), (m, "tree after the pushes")
    for u in range(4):
        pop.update(1)
        plain.update(1)
        for m, L in lone.items():
            L.update(1)
            M = pop.member(m)
            assert np.array_equal(bits64(M.priorities()), bits64(L.priorities())), (m, u, "tree")
            a, b = M.last_sample(), L.last_sample()
            assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(_bits(a["td"]), _bits(b["td"])) and np.array_equal(_bits(a["weight"]), _bits(b["weight"])), (m, u)
            _assert_same(_snapshot(gpu_ctx, HEAD, M, _stats_row(pop.stats(), m)), _snapshot(gpu_ctx, HEAD, L, _stats_row(L.stats())), "prioritised member %d, update %d" % (m, u))
    w = pop.member(2).last_sample()["weight"]
    assert len(set(w.tolist())) > 1 and w.max() == 1.0              # beta = 0.4: the importance weights reached the loss
    _assert_same(_snapshot(gpu_ctx, HEAD, pop.member(1), _stats_row(pop.stats(), 1)), _snapshot(gpu_ctx, HEAD, plain.member(1), _stats_row(plain.stats(), 1)), "the uniform member")
    assert not _same_slots(pop.member(0).state_dict()["params"], plain.member(0).state_dict()["params"])      # prioritised sampling draws other rows
    assert list(pop.stats()["updates"]) == [4, 4, 4]
    with pytest.raises(RuntimeError, match="not enabled"):
        pop.member(1).priorities()
    with pytest.raises(RuntimeError, match="not enabled"):
        pop.member(1).last_sample()
    # one call per population, and only on empty rings
    with pytest.raises(capi.StmpcError, match="already set up on this population"):
        gpu_ctx.dqn_pop_per_enable(pop.handle, [g.to_c() if g is not None else None for g in per])
    with pytest.raises(capi.StmpcError, match="empty ring only"):
        gpu_ctx.dqn_pop_per_enable(plain.handle, [per[0].to_c(), None, None])
    with pytest.raises(RuntimeError, match="not enabled"):
        plain.member(0).priorities()
    with pytest.raises(capi.StmpcError, match="cfgs and enabled have 2 entries, the population 3 members"):
        gpu_ctx.dqn_pop_per_enable(_syn_pop(gpu_ctx, None, []).handle, [per[0].to_c(), None])
    torch.cuda.synchronize()
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_member_handles(gpu_ctx, restore_settings):
    """What a lone learner's calls do on a borrowed member: a state_dict round trip moves member 1 alone; grads and targets equal the lone learner's;
    the lone per_enable is refused; a DQNActor view of member 1 evaluates as member(1).act does on the same vectors."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor, learner
    steps = _syn_steps()
    pop = _syn_pop(gpu_ctx, None, steps)
    pop.update(2)
    lone = [_syn_lone(gpu_ctx, m, None, steps) for m in range(3)]
    for m, L in enumerate(lone):
        L.update(2)
        M = pop.member(m)
        g, t = M.grads(), M.targets()
        gl, tl = L.grads(), L.targets()
        assert all(np.array_equal(_bits(g[k]), _bits(gl[k])) and np.abs(g[k]).max() > 0 for k in NAMES), m
        assert t.shape == (SYN[3], 4) and np.array_equal(_bits(t), _bits(tl)), m
        assert np.array_equal(_bits(M.minibatch()), _bits(L.minibatch())), m
    # a round trip on member 1
    before = [pop.member(m).state_dict() for m in range(3)]
    sd = pop.member(1).state_dict()
    for slot in Q_SLOTS:
        for k in NAMES:
            sd["params"][slot][k] = (sd["params"][slot][k] * np.float32(0.5) + np.float32(0.125)).astype(np.float32)
    sd["params"]["updates"] = 7
    sd["counters"] = None
    pop.member(1).load_state_dict(sd)
    after = [pop.member(m).state_dict() for m in range(3)]
    for m in (0, 2):
        assert _same_slots(after[m]["params"], before[m]["params"]) and np.array_equal(after[m]["counters"], before[m]["counters"]), m
    assert _same_slots(after[1]["params"], sd["params"]) and after[1]["params"]["updates"] == 7 and after[1]["counters"][1] == before[1]["counters"][1]
    assert list(pop.stats()["updates"]) == [2, 7, 2]
    pop.update(1)                                                   # the population reads the member's buffers: the loaded state is what it steps
    L = lone[1]
    L.load_state_dict(sd)
    L.update(1)
    assert _same_slots(pop.member(1).state_dict()["params"], L.state_dict()["params"]) and list(pop.stats()["updates"]) == [3, 8, 3]
    # the lone enable on a member
    with pytest.raises(capi.StmpcError, match="member of a population.*stmpc_pop_dqn_per_enable"):
        gpu_ctx.dqn_per_enable(pop.member(0).handle, learner.PERConfig().to_c())
    # a view of member 1's network as a policy, at test_qactor.py's row count 17
    n, (n_obs, h1, A, B) = 17, SYN
    g_, S = actor_settings()
    device = torch.device("cuda", torch.cuda.current_device())
    st = {k: v[:n].contiguous() for k, v in actor_states(g_, device).items()}
    M = pop.member(1)
    P = actor.DQNActor.from_learner(M, n, gpu_ctx, S)
    P.keep_features = P.keep_q = True
    P(1, st["ego4"], st["k"], st["ox"], st["ov"], st["oa"])
    torch.cuda.synchronize()
    feat = P.feat[:n].clone()
    q = torch.full((n, A), -7.0, dtype=torch.float32, device=device)
    a = M.act(feat, eps=0.0, debug_q=q)
    torch.cuda.synchronize()
    assert feat.shape == (n, n_obs) and np.array_equal(_bits(P.q[:n].cpu().numpy()), _bits(q.cpu().numpy())) and torch.equal(P.action[:n], a)
    assert np.array_equal(P.jerk[:n].cpu().numpy(), M.action_values[a.cpu().numpy()])
    other = pop.member(0).act(feat, eps=0.0).cpu().numpy()
    assert not np.array_equal(other, a.cpu().numpy())               # (member 0's network is another one)
    gpu_ctx.check_error()


# ---- 6: what the library refuses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_library_refusals(gpu_ctx, restore_settings):
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = SYN
    env = _stub_env(gpu_ctx, 3 * SYN_N, n_obs, A)
    ok = dict(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=SYN_RING)
    for odd, who in ((dict(h1=64), 1), (dict(batch=32), 1), (dict(capacity=SYN_RING + 1), 2)):
        cfgs = [learner.DQNConfig(**ok) for _ in range(3)]
        cfgs[who] = learner.DQNConfig(**dict(ok, **odd))
        with pytest.raises(capi.StmpcError, match="share n_obs, h1, n_actions, batch and capacity .member %d differs" % who):
            learner.DQNPopulation(env, cfgs)
    with pytest.raises(capi.StmpcError, match="share n_obs, h1, n_actions, batch and capacity .member 1 differs"):
        gpu_ctx.dqn_pop_create([learner.DQNConfig(**ok).to_c(0), learner.DQNConfig(**dict(ok, n_actions=5)).to_c(1)])
    for P in (0, 65):
        with pytest.raises(capi.StmpcError, match="a population has 1 ... 64 members, not %d" % P):
            learner.DQNPopulation(env, (learner.DQNConfig(**ok), P))
    with pytest.raises(capi.StmpcError, match="target_period"):      # a member's own cfg is the lone create's to refuse
        learner.DQNPopulation(env, [learner.DQNConfig(**ok), learner.DQNConfig(**dict(ok, target_period=0)), learner.DQNConfig(**ok)])
    pop = learner.DQNPopulation(env, (learner.DQNConfig(**ok), 3))
    step = _syn_steps()[0]
    obs = _dev(step["obs"])
    _feed(pop, step)
    for bad in ([1e-3, 1e-3], [1e-3] * 4):
        with pytest.raises(capi.StmpcError, match="learning-rate arrays have %d entries, the population 3 members" % len(bad)):
            pop.update(1, lr=bad)
        with pytest.raises(capi.StmpcError, match="eps array has %d entries, the population 3 members" % len(bad)):
            pop.act(obs, None, eps=bad)
    with pytest.raises(capi.StmpcError, match="learning rate is negative"):
        pop.update(1, lr=[1e-3, -1.0, 1e-3])
    for bad in ([0.0, 1.5, 0.0], 1.5, [0.0, 0.0, -0.1], float("nan")):
        with pytest.raises(capi.StmpcError, match="eps must be in 0 ... 1"):
            pop.act(obs, None, eps=bad)
    with pytest.raises(ValueError, match="48 rows given, the population's env has 96"):
        pop.act(obs[:48], None)
    with pytest.raises(ValueError, match="48 rows given"):
        _feed(pop, {k: v[:48] for k, v in step.items()})
    with pytest.raises(capi.StmpcError, match="n_per_member must be in 1 ... capacity"):
        gpu_ctx.dqn_pop_act(pop.handle, SYN_RING + 1, obs.data_ptr(), obs.stride(0), [0.0] * 3, pop._actions.data_ptr())
    with pytest.raises(capi.StmpcError, match="n_per_member must be in 1 ... capacity"):
        gpu_ctx.dqn_pop_act(pop.handle, 0, obs.data_ptr(), obs.stride(0), [0.0] * 3, pop._actions.data_ptr())
    with pytest.raises(capi.StmpcError, match="no such member"):
        gpu_ctx.dqn_pop_member(pop.handle, 3)
    with pytest.raises(capi.StmpcError, match="rows outside the ring"):
        gpu_ctx.dqn_pop_replay_read(pop.member(0).handle, 0, SYN_RING + 1)
    st = pop.stats()
    assert list(st["updates"]) == [0, 0, 0] and list(st["fill"]) == [SYN_N] * 3 and not pop.member(0).state_dict()["counters"][3]
    pop.update(1, lr=1e-3)                                          # a scalar and an array of the right length are both fine
    pop.update(1, lr=[1e-3, 2e-3, 3e-3])
    assert list(pop.stats()["updates"]) == [2, 2, 2]
    assert pop.act(obs, None, eps=[0.0, 0.5, 1.0]).shape == (3 * SYN_N,) and [int(pop.member(m).state_dict()["counters"][3]) for m in range(3)] == [0, 1, 1]
    # a lone call on a borrowed member stays legal and moves that member alone
    pop.member(1).update(1)
    torch.cuda.synchronize()
    assert list(pop.stats()["updates"]) == [2, 3, 2]
    gpu_ctx.check_error()


# ---- 7: the training loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_train_dqn_on_a_population(gpu_ctx, restore_settings):
    """train_dqn on a population of 2 over an env with two traffic groups: member m trains on traffic m."""
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n = 16
    env = vec_env.MergeVecEnv(2 * n, env_id="sumo-jerk-v0", seed=3, ctx=gpu_ctx, traffic=["low", "fast"])
    cfg = learner.DQNConfig(n_obs=env.obs_dim, h1=32, batch=16, capacity=256, replay_start=20, target_period=4)
    pop = learner.DQNPopulation(env, (cfg, 2), seeds=[5, 6], per=[learner.PERConfig(), None])
    first = [pop.member(m).state_dict()["params"] for m in range(2)]
    eps = lambda i, steps: np.array([0.5, 1.0 - 0.05 * i])          # both schedules may return per-member arrays
    res = learner.train_dqn(env, pop, frames=12 * 2 * n, updates_per_step=2, drain_every=4, eps_schedule=eps, lr_schedule=lambda i, steps: np.array([2e-4, 1e-3]))
    env.check_error()
    st = pop.stats()
    assert res["steps"] == 12 and res["frames"] == 12 * 2 * n and list(st["fill"]) == [12 * n] * 2
    assert list(st["updates"]) == [2 * 11, 2 * 11] and (st["updates"] > 0).all() and np.isfinite(st["loss"]).all() and np.isfinite(st["mean_q"]).all()
    assert np.isfinite(res["returns"]).all() and res["returns"].size == res["episodes"]
    assert len(res["member_returns"]) == 2 and sum(r.size for r in res["member_returns"]) == res["episodes"]
    assert np.array_equal(np.sort(np.concatenate(res["member_returns"])), np.sort(res["returns"]))
    for m in range(2):
        p = pop.member(m).state_dict()["params"]
        assert all(np.isfinite(p[s][k]).all() for s in Q_SLOTS for k in NAMES) and not np.array_equal(p["q"]["w1"], first[m]["q"]["w1"])
    assert pop.member(0).priorities()[0] > 0
    with pytest.raises(ValueError, match="the env has 2 traffic groups, the population 4 members"):
        learner.DQNPopulation(env, (cfg, 4))
    gpu_ctx.check_error()
