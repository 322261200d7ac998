"""A population of C51 learners on the GPU (learner.C51Population, csrc/stmpc_c51_pop_kernels.hpp, stmpc_pop_c51_*).  CPU part: test_c51_pop_cpu.py.

Every comparison is bit equality against the lone ``C51Learner`` (or, for the projection and the multi-step windows, against the host twin on exact
data): the population's kernels are the lone learner's bodies on the member ``blockIdx.y`` selects.  This file contains no tolerance.

Shapes (n_obs, h1, A, K, B) of tests/discrete_testlib.py's list: (20, 16, 5, 17, 7) on sumo-jerk-v0 -- pad columns inside the last tile, K below the lane
count, padded minibatch rows --, (20, 48, 20, 51, 33) on sumo-accel-v0 -- A K = 1020 pads to 1024, the widest layer allowed, every action block
straddles 16-column tiles --, and the shipped (20, 256, 5, 51, 50) in test 1 only.  Rings of at most 256 rows.

The gate in test 1 is test_dqn_pop.py's: capacity 200 and 12 steps of 24 frames, replay_start (0, 48, 199), so the update counts are 12, 10 and 4.

Tests 2 ... 7 run at both small shapes.  Multi-step windows (test 5): ``member(m).nstep_window`` reads every filled ring row's window (R, gamma^m,
the last row, m) through stmpc_pop_c51_multi_step_window and is compared with ``nstep_window_host`` on the member's own ring; the gathered minibatch
is compared with ``nstep_batch_host`` alongside, before each of the four updates.
"""
import numpy as np
import pytest

from discrete_testlib import (C51 as HEAD, C51_SUPPORTS as SUPPORT, DOUBLE, NAMES, PERIOD, Q_SLOTS, assert_population_run, assert_same as _assert_same,
                              dyadic_projection_case, feed as _feed, run_population, same_slots as _same_slots, snapshot as _snapshot, stats_row as _stats_row,
                              stub_env as _stub_env, syn_steps)
from learner_testlib import CAP, bits64, dev as _dev
from stmpc_testlib import actor_settings, actor_states, bits as _bits, capi as _capi

SEEDS = (11, 12, 13)
REPLAY_START = (0, 48, CAP - 1)                # (199 is the largest a ring of 200 allows)
EPS = (0.0, 0.3, 1.0)
CASES = [pytest.param((20, 16, 5, 17, 7), id="20-16-5-K17-B7"), pytest.param((20, 48, 20, 51, 33), id="20-48-20-K51-B33-accel"),
         pytest.param((20, 256, 5, 51, 50), id="20-256-5-K51-B50")]


# ---- 1: a population on a real env next to lone learners on its slices ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", CASES)
def test_gpu_population_equals_its_members_run_alone(shape, gpu_ctx, restore_settings):
    """P = 3, n = 24 (no multiple of the 16-row acting tile), capacity 200 (every ring wraps), members that differ in seed, gamma, lr, double
    (True, False, True), target_period (1, 3, 5), replay_start (0, 48, 199), support ([-10, 10], [-4, 4], [-2, 6]) and eps (0.0, 0.3, 1.0)."""
    _capi()
    assert_population_run(run_population(gpu_ctx, HEAD, shape, 3, seeds=SEEDS, eps=EPS, replay_start=REPLAY_START), PERIOD)


# ---- 2 ... 7: synthetic rings: rows pushed through a stub env ----------------------------------------------------------------------------------------
SMALL, WIDE = (20, 16, 5, 17, 7), (20, 48, 20, 51, 33)
BOTH = [pytest.param(SMALL, id="20-16-5-K17-B7"), pytest.param(WIDE, id="20-48-20-K51-B33")]
SYN_RING, SYN_N, SYN_PUSHES = 128, 24, 6       # 144 rows into 128: the rings (and the trees' leaves) wrap; 5 * 24 <= 128: n_step = 5 is legal


def _syn_cfg(shape, m, **kw):
    """Member m's cfg of the synthetic populations (its own gamma, period, double and support); ``kw`` overrides."""
    return HEAD.cfg(shape, m, **dict(dict(n_actions=shape[2], capacity=SYN_RING, lr=1e-3), **kw))


def _syn_steps(shape, P=3, pushes=SYN_PUSHES):
    return syn_steps(HEAD, shape, P, pushes, SYN_N, draw_all=True)


def _syn_pop(gpu_ctx, shape, cfgs, steps, per=None, seeds=SEEDS):
    from rl_mpc_lanemerging_amd import learner
    pop = learner.C51Population(_stub_env(gpu_ctx, len(cfgs) * SYN_N, shape[0], shape[2]), cfgs, seeds=list(seeds[:len(cfgs)]), per=per)
    for step in steps:
        _feed(pop, step)
    return pop


def _syn_lone(gpu_ctx, shape, cfg, m, steps, seed=None):
    from rl_mpc_lanemerging_amd import learner
    L = learner.C51Learner((shape[0], shape[2]), cfg, seed=SEEDS[m] if seed is None else seed, ctx=gpu_ctx, rows_per_push=SYN_N)
    for step in steps:
        _feed(L, step, slice(m * SYN_N, (m + 1) * SYN_N))
    return L


def _act_push_update(pop, steps, eps, updates=1):
    """The loop on synthetic transitions: act on the step's observations (the actions are kept, the pushed ones are the step's), push, update."""
    acts = []
    for step in steps:
        acts.append(pop.act(_dev(step["obs"]), None, eps=eps).cpu().numpy().copy())
        _feed(pop, step)
        pop.update(updates)
    return acts


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOTH)
def test_gpu_a_members_bits_do_not_depend_on_the_others(shape, gpu_ctx, restore_settings):
    """The same member -- slot 0, eps 0.3, replay_start 48, target_period 3 -- inside P = 3, inside P = 3 with the other two swapped for other cfgs,
    seeds and eps, and as P = 1: its actions at every step and its final snapshot are identical."""
    _capi()
    subject = lambda: _syn_cfg(shape, 1, replay_start=48)
    runs = []
    for others, seeds, eps in (([_syn_cfg(shape, 0), _syn_cfg(shape, 2)], (21, 22, 23), [0.3, 0.0, 1.0]),
                               ([_syn_cfg(shape, 2, gamma=0.5, target_period=2, v_min=-1.0, v_max=1.0), _syn_cfg(shape, 0, double=False, replay_start=100)],
                                (21, 98, 99), [0.3, 0.7, 0.0]),
                               ([], (21,), [0.3])):
        P = 1 + len(others)
        steps = _syn_steps(shape, P)
        pop = _syn_pop(gpu_ctx, shape, [subject()] + others, [], seeds=seeds)
        acts = _act_push_update(pop, steps, eps)
        runs.append(([a[:SYN_N] for a in acts], _snapshot(gpu_ctx, HEAD, pop.member(0), _stats_row(pop.stats(), 0)),
                     pop.member(1).state_dict()["params"]["q"]["w1"] if P > 1 else None))
    (a0, s0, o0), (a1, s1, o1), (a2, s2, _) = runs
    assert int(s0["counters"][2]) == 4 and int(s0["counters"][3]) == SYN_PUSHES       # 24 j > 48 from the third push on; every call explored
    assert len({a.tobytes() for a in a0}) > 1
    for i in range(SYN_PUSHES):
        assert np.array_equal(a0[i], a1[i]) and np.array_equal(a0[i], a2[i]), i
    _assert_same(s0, s1, "others swapped")
    _assert_same(s0, s2, "alone in a population of one")
    assert not np.array_equal(_bits(o0), _bits(o1))                 # (the neighbours did differ)
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOTH)
def test_gpu_a_gate_shut_throughout(shape, gpu_ctx, restore_settings):
    """Member 1's replay_start is 127 and 96 frames are pushed: it keeps its initial parameters and Adam state bit for bit and does 0 updates while
    its neighbours do 4 each; before any push a whole population is a no-op."""
    _capi()
    cfgs = [_syn_cfg(shape, 0), _syn_cfg(shape, 1, replay_start=SYN_RING - 1), _syn_cfg(shape, 2)]
    pop = _syn_pop(gpu_ctx, shape, cfgs, [])
    first = [pop.member(m).state_dict() for m in range(3)]
    pop.update(3)                                                   # nothing to sample: nothing moves
    for m in range(3):
        sd = pop.member(m).state_dict()
        assert _same_slots(sd["params"], first[m]["params"]) and not sd["counters"].any(), m
    _act_push_update(pop, _syn_steps(shape, 3, pushes=4), [1.0, 1.0, 1.0])
    st = pop.stats()
    assert list(st["updates"]) == [4, 0, 4] and list(st["fill"]) == [4 * SYN_N] * 3
    sd = [pop.member(m).state_dict() for m in range(3)]
    assert _same_slots(sd[1]["params"], first[1]["params"]) and np.array_equal(_bits(sd[1]["params"]["beta_pow"]), _bits(np.ones(2, np.float32)))
    assert not any(np.abs(sd[1]["params"][s][k]).max() > 0 for s in ("q_m", "q_v") for k in NAMES)
    c = sd[1]["counters"]
    assert (int(c[1]), int(c[2]), int(c[3]), int(c[4])) == (4 * SYN_N, 0, 4, 4 * SYN_N)
    for m in (0, 2):
        assert not _same_slots(sd[m]["params"], first[m]["params"], ("q",)) and all(np.abs(sd[m]["params"]["q_m"][k]).max() > 0 for k in NAMES), m
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOTH)
def test_gpu_prioritised_members(shape, gpu_ctx, restore_settings):
    """per = [alpha 0.5, None, alpha 1 with beta]: each prioritised member's tree (every node), last_sample and snapshot equal the lone
    C51Learner(cfg with per=) after the pushes and after each of four updates; the uniform member equals the member of a population without per."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    per = [learner.PERConfig(alpha=0.5, max_priority=16.0), None, learner.PERConfig(alpha=1.0, beta=0.4, max_priority=16.0)]
    steps = _syn_steps(shape)
    mk = lambda: [_syn_cfg(shape, m) for m in range(3)]
    pop, plain = _syn_pop(gpu_ctx, shape, mk(), steps, per), _syn_pop(gpu_ctx, shape, mk(), steps, None)
    assert pop.per == per and plain.per == [None] * 3
    lone = {m: _syn_lone(gpu_ctx, shape, _syn_cfg(shape, m, per=per[m]), m, steps) for m in (0, 2)}
    for m, L in lone.items():
        tree = pop.member(m).priorities()
        assert tree.shape == (2 * SYN_RING - 1,) and np.array_equal(bits64(tree), bits64(L.priorities())), (m, "tree after the pushes")
    mixed = 0
    for u in range(4):
        before = {m: pop.member(m).priorities() for m in lone}
        pop.update(1)
        plain.update(1)
        for m, L in lone.items():
            L.update(1)
            M = pop.member(m)
            assert np.array_equal(bits64(M.priorities()), bits64(L.priorities())), (m, u, "tree")
            a, b = M.last_sample(), L.last_sample()
            if m == 2:                                              # beta = 0.4: the weights differ exactly where the sampled leaves' priorities did, and their maximum is 1
                leaf = before[m][SYN_RING - 1 + a["idx"]]
                assert (len(set(a["weight"].tolist())) > 1) == (len(set(leaf.tolist())) > 1) and a["weight"].max() == 1.0, (u, leaf, a["weight"])
                mixed += len(set(leaf.tolist())) > 1
            assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(_bits(a["td"]), _bits(b["td"])) and np.array_equal(_bits(a["weight"]), _bits(b["weight"])), (m, u)
            _assert_same(_snapshot(gpu_ctx, HEAD, M, _stats_row(pop.stats(), m)), _snapshot(gpu_ctx, HEAD, L, _stats_row(L.stats())), "prioritised member %d, update %d" % (m, u))
    # a minibatch that mixes rows with a priority of their own and fresh ones: certain in practice once 33 of 128 rows were visited, not with 7
    assert mixed >= 1 or shape[4] < 33, mixed
    _assert_same(_snapshot(gpu_ctx, HEAD, pop.member(1), _stats_row(pop.stats(), 1)), _snapshot(gpu_ctx, HEAD, plain.member(1), _stats_row(plain.stats(), 1)), "the uniform member")
    assert not _same_slots(pop.member(0).state_dict()["params"], plain.member(0).state_dict()["params"])      # prioritised sampling draws other rows
    assert list(pop.stats()["updates"]) == [4, 4, 4]
    with pytest.raises(RuntimeError, match="not enabled"):
        pop.member(1).priorities()
    with pytest.raises(capi.StmpcError, match="already set up on this population"):
        gpu_ctx.c51_pop_per_enable(pop.handle, [g.to_c() if g is not None else None for g in per])
    with pytest.raises(capi.StmpcError, match="empty ring only"):
        gpu_ctx.c51_pop_per_enable(plain.handle, [per[0].to_c(), None, None])
    torch.cuda.synchronize()
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOTH)
def test_gpu_n_step_per_member(shape, gpu_ctx, restore_settings):
    """n_step = (1, 3, 5) in one population on pushes of 24 rows with terminated and truncated rows: each member is bit-identical to the lone learner
    with that cfg over four updates; member(m).nstep_window on every ring row equals nstep_window_host on the member's own ring (R and gamma^m bit
    for bit, the last row and m exactly) and the lone learner's; the gathered minibatch equals nstep_batch_host before each update."""
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, B = shape[0], shape[4]
    NS = (1, 3, 5)
    steps = _syn_steps(shape)
    mk = lambda m: _syn_cfg(shape, m, n_step=NS[m])
    pop = _syn_pop(gpu_ctx, shape, [mk(m) for m in range(3)], steps)
    lone = [_syn_lone(gpu_ctx, shape, mk(m), m, steps) for m in range(3)]
    for m, L in enumerate(lone):                                    # every filled row's window: R, gamma^m, the last row, m
        M = pop.member(m)
        cn = M.state_dict()["counters"]
        ring = gpu_ctx.c51_pop_replay_read(M.handle, 0, SYN_RING)
        assert int(cn[1]) == SYN_RING and int(cn[0]) == (SYN_PUSHES * SYN_N) % SYN_RING
        got = M.nstep_window(np.arange(SYN_RING))
        want = [learner.nstep_window_host(ring, i, cn[0], cn[1], SYN_N, NS[m], mk(m).gamma) for i in range(SYN_RING)]
        assert got.shape == (SYN_RING, 4) and got.dtype == np.float64
        assert np.array_equal(_bits(got[:, 0].astype(np.float32)), _bits(np.array([w[0] for w in want], dtype=np.float32))), (m, "R")
        assert np.array_equal(got[:, 0], got[:, 0].astype(np.float32).astype(np.float64)) and np.array_equal(got[:, 1], got[:, 1].astype(np.float32).astype(np.float64))
        assert np.array_equal(_bits(got[:, 1].astype(np.float32)), _bits(np.array([w[1] for w in want], dtype=np.float32))), (m, "gamma^m")
        assert np.array_equal(got[:, 2], [w[2] for w in want]) and np.array_equal(got[:, 3], [w[3] for w in want]), (m, "last row, m")
        assert np.array_equal(bits64(got), bits64(L.nstep_window(np.arange(SYN_RING)))), m
        lengths = set(got[:, 3].astype(int).tolist())
        assert lengths == {1} if NS[m] == 1 else (lengths >= {1, 2, 3} and max(lengths) == NS[m]), (m, lengths)
        with pytest.raises(capi.StmpcError):
            M.nstep_window([SYN_RING])                              # not a ring row
    seen_m = set()
    for u in range(4):
        for m, L in enumerate(lone):
            M = pop.member(m)
            cn = M.state_dict()["counters"]
            ring = gpu_ctx.c51_pop_replay_read(M.handle, 0, SYN_RING)
            assert (int(cn[1]), int(cn[2])) == (SYN_RING, u) and bool(ring[:, capi.DONE_COL].any()) == (NS[m] > 1)
            idx = learner.sample_indices_host(SEEDS[m], u, B, SYN_RING)
            b = learner.nstep_batch_host(ring, idx, cn[0], cn[1], SYN_N, NS[m], mk(m).gamma, n_obs, dqn=True)
            rows = M.minibatch()
            assert np.array_equal(_bits(rows), _bits(b["rows"])), (m, u, "windows")
            assert np.array_equal(_bits(rows), _bits(L.minibatch())), (m, u)
            seen_m |= {(m, int(x)) for x in b["m"]}
        pop.update(1)
        for m, L in enumerate(lone):
            L.update(1)
            _assert_same(_snapshot(gpu_ctx, HEAD, pop.member(m), _stats_row(pop.stats(), m)), _snapshot(gpu_ctx, HEAD, L, _stats_row(L.stats())), "n_step %d, update %d" % (NS[m], u))
    assert {k for mm, k in seen_m if mm == 0} == {1} and max(k for mm, k in seen_m if mm == 1) <= 3 and len({k for mm, k in seen_m if mm == 2}) >= 2
    with pytest.raises(capi.StmpcError, match="member of a population.*stmpc_pop_c51_multi_step_enable"):
        gpu_ctx.nstep_enable("c51", pop.member(0).handle, mk(2).to_c_nstep(SYN_N))
    with pytest.raises(capi.StmpcError):                            # a push of another size is refused once a member has n_step > 1
        gpu_ctx.c51_pop_push(pop.handle, SYN_N - 1, 0, 0, 0, n_obs, 0, 0, 0, 0)
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOTH)
def test_gpu_debug_entries_on_a_borrowed_member(shape, gpu_ctx, restore_settings):
    """grads, targets, dist, minibatch and the padded reads of a borrowed member equal the lone learner's on the same state; at K = 17 project on
    dyadic_projection_case(17) (member 1's support is the case's [-8, 8]) equals c51_project_host exactly, at K = 51 (no dyadic dz) project on
    random distributions equals the lone learner's; a state_dict round trip moves member 1 alone and the population
    steps the loaded state; the lone per_enable is refused."""
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, K, B = shape
    if K == 17:
        case_cfg, p, r, mask, disc = dyadic_projection_case(17)
        sup = dict(v_min=case_cfg.v_min, v_max=case_cfg.v_max)
    else:
        rng = np.random.default_rng(5)
        p = rng.random((48, K))
        p, r, mask, disc, sup = p / p.sum(1, keepdims=True), rng.normal(size=48) * 3, (rng.random(48) > 0.25).astype(np.float64), rng.choice([0.5, 0.9, 0.999], 48), {}
    mk = lambda m: _syn_cfg(shape, m, **(sup if m == 1 else {}))
    steps = _syn_steps(shape)
    pop = _syn_pop(gpu_ctx, shape, [mk(m) for m in range(3)], steps)
    pop.update(2)
    lone = [_syn_lone(gpu_ctx, shape, mk(m), m, steps) for m in range(3)]
    for m, L in enumerate(lone):
        L.update(2)
        M = pop.member(m)
        g, gl = M.grads(), L.grads()
        assert all(np.array_equal(_bits(g[k]), _bits(gl[k])) and np.abs(g[k]).max() > 0 for k in NAMES), m
        t, (d, t2), (dl, tl) = M.targets(), M.dist(), L.dist()
        assert t.shape == (B, 4) and d.shape == (B, 2, K) and np.array_equal(_bits(t), _bits(tl)) and np.array_equal(_bits(t2), _bits(tl)) and np.array_equal(_bits(d), _bits(dl)), m
        assert np.array_equal(_bits(M.minibatch()), _bits(L.minibatch())), m
        assert np.array_equal(_bits(gpu_ctx.c51_dzout_read(M.handle, B, A * K)), _bits(gpu_ctx.c51_dzout_read(L.handle, B, A * K))), m
        have, want = (gpu_ctx.c51_padded_read(h, capi.C51_GRAD, h1, A * K) for h in (M.handle, L.handle))
        assert all(np.array_equal(_bits(have[k]), _bits(want[k])) for k in NAMES), m
    got = pop.member(1).project(p, r, mask, disc)
    assert got.dtype == np.float32 and got.shape == (48, K)
    if K == 17:
        want = learner.c51_project_host(p, r, mask, disc, case_cfg)
        assert np.array_equal(got.astype(np.float64), want) and (got.astype(np.float64).sum(1) == 1.0).all()
    assert np.array_equal(_bits(got), _bits(lone[1].project(p, r, mask, disc)))
    assert not np.array_equal(pop.member(0).project(p, r, mask, disc), got)      # (the support is the member's own)
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
    assert _same_slots(after[1]["params"], sd["params"]) and after[1]["params"]["updates"] == 7 and list(pop.stats()["updates"]) == [2, 7, 2]
    pop.update(1)                                                   # the population reads the member's buffers: the loaded state is what it steps
    lone[1].load_state_dict(sd)
    lone[1].update(1)
    assert _same_slots(pop.member(1).state_dict()["params"], lone[1].state_dict()["params"]) and list(pop.stats()["updates"]) == [3, 8, 3]
    # the lone enables on a member
    with pytest.raises(capi.StmpcError, match="member of a population.*stmpc_pop_c51_per_enable"):
        gpu_ctx.c51_per_enable(pop.member(0).handle, learner.PERConfig().to_c())
    with pytest.raises(capi.StmpcError, match="no such member"):
        gpu_ctx.c51_pop_member(pop.handle, 3)
    with pytest.raises(capi.StmpcError, match="eps array has 2 entries, the population 3 members"):
        pop.act(_dev(steps[0]["obs"]), None, eps=[0.0, 0.1])
    with pytest.raises(capi.StmpcError, match="learning-rate arrays have 4 entries, the population 3 members"):
        pop.update(1, lr=[1e-3] * 4)
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOTH)
def test_gpu_train_to_evaluate(shape, gpu_ctx, restore_settings):
    """actor.C51Actor.from_learner(pop.member(m), ...) on the 72 states of the actor tests gives, on member m's rows, the expected values and actions
    of pop.act(eps=0, debug_q=) on the same feature vectors, bit for bit -- and again after one more pop.update, because the view is live."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor
    n_obs, A = shape[0], shape[2]
    steps = _syn_steps(shape)
    pop = _syn_pop(gpu_ctx, shape, [_syn_cfg(shape, m) for m in range(3)], steps)
    pop.update(2)
    g_, S = actor_settings()
    device = torch.device("cuda", torch.cuda.current_device())
    st = actor_states(g_, device)
    n = 3 * SYN_N
    assert st["k"].shape[0] == n
    views = [actor.C51Actor.from_learner(pop.member(m), n, gpu_ctx, S) for m in range(3)]
    for V in views:
        V.keep_features = V.keep_q = True
    q = torch.full((n, A), -7.0, dtype=torch.float32, device=device)
    seen = []
    for rnd in range(2):
        for m, V in enumerate(views):
            sl = slice(m * SYN_N, (m + 1) * SYN_N)
            V(1, st["ego4"], st["k"], st["ox"], st["ov"], st["oa"])
            torch.cuda.synchronize()
            feat = V.feat[:n].clone()
            assert feat.shape == (n, n_obs)
            a = pop.act(feat, None, eps=0.0, debug_q=q)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(V.q[sl].cpu().numpy()), _bits(q[sl].cpu().numpy())) and torch.equal(V.action[sl], a[sl]), (rnd, m)
            assert np.array_equal(V.jerk[sl].cpu().numpy(), pop.member(m).action_values[a[sl].cpu().numpy()]), (rnd, m)
            other = (m + 1) % 3                                     # (another member's rows of the same launch hold another network's values)
            assert not np.array_equal(V.q[other * SYN_N:(other + 1) * SYN_N].cpu().numpy(), q[other * SYN_N:(other + 1) * SYN_N].cpu().numpy()), (rnd, m)
            seen.append(V.q[sl].cpu().numpy().copy())
        pop.update(1)
    assert all(not np.array_equal(seen[m], seen[3 + m]) for m in range(3))      # the update moved every member's values
    assert [int(pop.member(m).state_dict()["counters"][3]) for m in range(3)] == [0, 0, 0]
    gpu_ctx.check_error()


# ---- 8: the training loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_train_dqn_on_a_c51_population(gpu_ctx, restore_settings):
    """train_dqn, unedited, on a population of 3 whose members differ in support, double and n_step, one of them prioritised: member_returns of
    length P, every member's update count advanced, both contexts clean; the policy populations still refuse C51 members."""
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n, P = 16, 3
    env = vec_env.MergeVecEnv(P * n, env_id="sumo-jerk-v0", seed=3, ctx=gpu_ctx)
    cfgs = [learner.C51Config(n_obs=env.obs_dim, h1=32, batch=16, capacity=256, replay_start=20, target_period=4, n_atoms=21, v_min=SUPPORT[m][0], v_max=SUPPORT[m][1],
                              double=DOUBLE[m], n_step=(1, 3, 1)[m]) for m in range(P)]
    pop = learner.C51Population(env, cfgs, seeds=[5, 6, 7], per=[learner.PERConfig(max_priority=16.0), None, None])
    first = [pop.member(m).state_dict()["params"] for m in range(P)]
    eps = lambda i, steps: np.array([0.5, 1.0 - 0.05 * i, 0.2])     # both schedules may return per-member arrays
    res = learner.train_dqn(env, pop, frames=12 * P * n, updates_per_step=2, drain_every=4, eps_schedule=eps, lr_schedule=lambda i, steps: np.array([2e-4, 1e-3, 5e-4]))
    env.check_error()
    gpu_ctx.check_error()
    st = pop.stats()
    assert res["steps"] == 12 and res["frames"] == 12 * P * n and list(st["fill"]) == [12 * n] * P
    assert list(st["updates"]) == [2 * 11] * P and np.isfinite(st["loss"]).all() and (st["loss"] > 0).all() and np.isfinite(st["mean_q"]).all()
    assert np.isfinite(res["returns"]).all() and res["returns"].size == res["episodes"]
    assert len(res["member_returns"]) == P and sum(r.size for r in res["member_returns"]) == res["episodes"]
    assert np.array_equal(np.sort(np.concatenate(res["member_returns"])), np.sort(res["returns"]))
    for m in range(P):
        p = pop.member(m).state_dict()["params"]
        assert all(np.isfinite(p[s][k]).all() for s in Q_SLOTS for k in NAMES) and not np.array_equal(p["q"]["w1"], first[m]["q"]["w1"])
    assert pop.member(0).priorities()[0] > 0
    for who, call in (("evaluate_dqn_members", lambda: learner.evaluate_dqn_members(pop, 4)), ("QActorPopulation", lambda: actor.QActorPopulation(pop, 4, gpu_ctx, pkg.Settings)),
                      ("population_of", lambda: actor.population_of(pop, 4, gpu_ctx, pkg.Settings))):
        with pytest.raises(ValueError, match="%s: members 0, 1, 2 are categorical \\(C51\\) policies" % who):
            call()
    gpu_ctx.check_error()
