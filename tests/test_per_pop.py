"""Prioritised replay in the DDPG / TD3 populations on the GPU (``DDPGPopulation(per=)``, ``TD3Population(per=)``, csrc/stmpc_per_pop_kernels.hpp,
stmpc_pop_per_*).  CPU part: test_per_pop_cpu.py.

Every comparison is bit equality: device against device (a member against the lone learner with the same ``cfg.per`` fed the member's slice, or against
the same member of another population), or device against the host twin ``SumTreeHost`` where only pushes touched a tree.  No tolerance anywhere: the
population's kernels are the lone kernels' bodies on the member the grid selects.

Shapes: the "padded" 20-40-24 network of learner_testlib.SHAPES (the shipped 400 x 300 once per learner kind, at B = 100), N_PER = 24 environments
per member, 12 steps, capacity 200 -- not a power of two, so the tree has 256 leaves of which 56 stay empty, and every ring wraps.  Member 2's
``replay_start`` is 199, the largest a ring of 200 allows (test_td3_pop's module text): its gate is shut during steps 1 ... 8 and opens at step 9.
"""
import numpy as np
import pytest

from learner_testlib import (CAP, N_PER, SHAPES, SHIPPED, STEPS, assert_same as _assert_same, assert_same_td3 as _assert_same_td3, dev as _dev, internal_nodes_are_exact,
                             push as _push, random_td3_problem, snapshot as _snapshot, stats_row as _stats_row, stub_env as _stub_env, td3_init as _init)
from stmpc_testlib import bits as _bits, capi as _capi

KINDS = ["ddpg", "td3"]
SEEDS = (11, 12, 13)
GAMMA, TAU, NOISE = (0.99, 0.95, 0.9), (0.005, 0.01, 0.02), (0.1, 0.2, 0.05)
LR_Q, LR_PI = (2e-4, 1e-3, 5e-4), (2e-4, 3e-4, 1e-4)
TARGET_NOISE, NOISE_CLIP, DELAY = (0.2, 0.1, 0.3), (0.5, 0.25, 0.4), (1, 2, 3)
REPLAY_START = (0, 48, CAP - 1)
ALPHA, BETA, MAX_PRIORITY = (0.5, 1.0, 0.5), (0.0, 0.4, 0.4), (4.0, 2.0, 1.0)
GATED_STEPS = (CAP - 1) // N_PER                # member 2's gate is shut after pushes 1 ... 8
_cache = {}


def _pers(alpha=ALPHA, beta=BETA, max_priority=MAX_PRIORITY):
    from rl_mpc_lanemerging_amd import learner
    return [learner.PERConfig(alpha=alpha[m], beta=beta[m], max_priority=max_priority[m]) for m in range(3)]


def _cfg(kind, shape, B, m, per=None, capacity=CAP, replay_start=None):
    """Member m's cfg; ``per`` only for the lone learner it is compared with (a population takes ``per=`` itself)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape] if isinstance(shape, str) else shape
    kw = dict(n_obs=n_obs, h1=h1, h2=h2, batch=B, capacity=capacity, replay_start=REPLAY_START[m] if replay_start is None else replay_start, gamma=GAMMA[m],
              tau=TAU[m], noise=NOISE[m], lr_q=LR_Q[m], lr_pi=LR_PI[m], per=per)
    if kind == "td3":
        return learner.TD3Config(target_noise=TARGET_NOISE[m], noise_clip=NOISE_CLIP[m], policy_delay=DELAY[m], **kw)
    return learner.DDPGConfig(**kw)


def _nets(kind, shape, m):
    a, q, q2 = _init(shape, m)
    return (a, q, q2) if kind == "td3" else {"actor": a, "critic": q}


def _classes(kind):
    from rl_mpc_lanemerging_amd import learner
    return (learner.TD3Population, learner.TD3Learner) if kind == "td3" else (learner.DDPGPopulation, learner.DDPGLearner)


def _stats(kind, L):
    if kind == "td3":
        return _stats_row(L.stats_td3())
    s = L.stats()
    return [s["critic_loss"], s["mean_q"], float(s["fill"]), float(s["updates"])]


def _pop_stats(kind, ps, m):
    return _stats_row(ps, m) if kind == "td3" else [ps["critic_loss"][m], ps["mean_q"][m], float(ps["fill"][m]), float(ps["updates"][m])]


def _same(kind, a, b, label):
    """Parameters, beta powers, counters, ring and statistics (test_learner_pop / test_td3_pop), and the tree where there is one."""
    (_assert_same_td3 if kind == "td3" else _assert_same)(a, b, label)
    assert (a["tree"] is None) == (b["tree"] is None), label
    if a["tree"] is not None:
        assert np.array_equal(_bits(a["tree"]), _bits(b["tree"])), (label, "tree")


def _same_sample(a, b):
    return set(a) == set(b) == {"idx", "td", "weight"} and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _run(gpu_ctx, kind, shape, B, P, per, seeds=SEEDS, alone=True):
    """STEPS steps of act -> env.step -> push -> update(1) (test_td3_pop._run's loop) of a population of P with ``per`` (None, or a list of P) on one env of
    P * N_PER and, if ``alone``, of the lone learners with ``cfg.per = per[m]`` on their slices, fed the same transitions.  Every step: each prioritised
    member's tree and last_sample() against its lone learner's; while a prioritised member is gated, its tree against ``SumTreeHost`` after the same
    pushes and its last_sample() against zeros.  Returns the members' snapshots and what the run saw."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    Pop, Lone = _classes(kind)
    n = N_PER
    pers = list(per) if per is not None else [None] * P
    env = vec_env.MergeVecEnv(P * n, env_id="sumo-jerk-continuous-v0", seed=7, ctx=gpu_ctx)
    pop = Pop(env, [_cfg(kind, shape, B, m) for m in range(P)], seeds=list(seeds[:P]), init=[_nets(kind, shape, m) for m in range(P)], per=per)
    assert pop.per == pers and len(pop) == P
    lone = [Lone(env, _cfg(kind, shape, B, m, per=pers[m]), seed=seeds[m], init=_nets(kind, shape, m)) for m in range(P)] if alone else []
    host = [learner.SumTreeHost(CAP, g) if g is not None else None for g in pers]
    sl = [slice(m * n, (m + 1) * n) for m in range(P)]
    lr_q, lr_pi = list(LR_Q[:P]), list(LR_PI[:P])
    saw = {"duplicates": [False] * P, "gated_checks": [0] * P, "others_advanced": [0] * P}
    done = [0] * P
    obs = env.reset()
    for i in range(STEPS):
        ticks = env.episode_ticks.clone()
        action = pop.act(obs, ticks, noise=True).clone()
        if alone:
            a_lone = torch.cat([lone[m].act(obs[sl[m]], ticks[sl[m]], noise=True) for m in range(P)])
            assert np.array_equal(_bits(action.cpu().numpy()), _bits(a_lone.cpu().numpy())), "actions of step %d" % i
        nobs, r, term, trunc, info = env.step(action)
        fin = info["final_observation"]
        pop.push(obs, ticks, action, r, nobs, term, trunc, final_obs=fin)
        pop.update(1, lr_q=lr_q, lr_pi=lr_pi)
        for m, L in enumerate(lone):
            L.push(obs[sl[m]], ticks[sl[m]], action[sl[m]], r[sl[m]], nobs[sl[m]], term[sl[m]], trunc[sl[m]], final_obs=fin[sl[m]])
            L.update(1, lr_q=lr_q[m], lr_pi=lr_pi[m])
        obs = nobs
        want = [sum(1 for j in range(1, i + 2) if n * j > REPLAY_START[m]) for m in range(P)]        # the gate is per member
        have = pop.stats()["updates"]
        assert list(have) == want, (i, list(have), want)
        for m in range(P):
            if pers[m] is None:
                continue
            M = pop.member(m)
            tree, ls = M.priorities(), M.last_sample()
            assert tree.size == 511 and internal_nodes_are_exact(tree) and not tree[255 + CAP:].any(), (i, m)
            host[m].push(n)
            if alone:
                assert np.array_equal(_bits(tree), _bits(lone[m].priorities())), "tree of member %d after step %d" % (m, i)
                assert _same_sample(ls, lone[m].last_sample()), "last_sample of member %d after step %d" % (m, i)
            if want[m] == 0:                                        # gated so far: pushes only, and no sampling step has run
                assert np.array_equal(_bits(tree), _bits(host[m].nodes)), "gated member %d after step %d" % (m, i)
                assert not ls["idx"].any() and not ls["td"].any() and not ls["weight"].any(), (i, m)
                saw["gated_checks"][m] += 1
                saw["others_advanced"][m] = max(saw["others_advanced"][m], max(want))
            if want[m] > done[m]:                                   # this step's update ran: its minibatch is what last_sample() shows
                assert ls["idx"].max() < min(CAP, n * (i + 1)) and ls["weight"].max() == 1.0
                saw["duplicates"][m] |= len(set(ls["idx"].tolist())) < B
        done = want
    torch.cuda.synchronize()
    env.check_error()
    ps = pop.stats()
    snaps = []
    for m in range(P):
        M = pop.member(m)
        s = _snapshot(gpu_ctx, M, _pop_stats(kind, ps, m))
        s["tree"] = M.priorities() if pers[m] is not None else None
        snaps.append(s)
        c = s["counters"]
        assert (c[0], c[1], c[2], c[3], c[4]) == ((n * STEPS) % CAP, CAP, want[m], STEPS, n * STEPS) and np.isfinite(s["stats"][:2]).all()
    for m, L in enumerate(lone):
        ref = _snapshot(gpu_ctx, L, _stats(kind, L))
        ref["tree"] = L.priorities() if pers[m] is not None else None
        _same(kind, snaps[m], ref, "member %d vs alone" % m)
    return snaps, saw


# ---- 1, 4 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,B", [pytest.param("padded", 16, id="padded-B16"), pytest.param(SHIPPED, 100, id="400x300-B100")])
def test_gpu_population_equals_its_members_run_alone(kind, shape, B, gpu_ctx, restore_settings):
    """P = 3; the members differ in seed, replay_start (0, 48, 199), alpha (0.5, 1, 0.5), beta (0, 0.4, 0.4), max_priority (4, 2, 1), gamma, tau, acting
    noise, learning rates and (TD3) target_noise, noise_clip, policy_delay.  Trees and last_sample() every step, everything else at the end.
    B = 100: every member met a duplicate index in some update, so the last-duplicate-wins rule of the priority update ran in each."""
    _capi()
    snaps, saw = _cache[kind, shape, B] = _run(gpu_ctx, kind, shape, B, 3, _pers())
    if B == 100:
        assert saw["duplicates"] == [True, True, True], saw
    assert [int(s["counters"][2]) for s in snaps] == [12, 10, 4]
    assert not np.array_equal(snaps[0]["tree"], snaps[1]["tree"]) and not np.array_equal(snaps[1]["tree"], snaps[2]["tree"])
    from rl_mpc_lanemerging_amd import learner
    for s, g in zip(snaps, _pers()):                                # every filled leaf within the member's own bounds, and not all at the new rows' weight
        leaf = s["tree"][255:255 + CAP]
        print("member leaves: %d distinct, %.3e ... %.3e" % (np.unique(leaf).size, leaf.min(), leaf.max()))
        assert leaf.min() >= learner.per_pow(g.min_priority, g.alpha) and leaf.max() <= learner.per_pow(g.max_priority, g.alpha) and np.unique(leaf).size > 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_gate_is_per_member(kind, gpu_ctx, restore_settings):
    """While member 2 is gated (pushes 1 ... 8) its tree is ``SumTreeHost`` after the same pushes, bit for bit, and its last_sample() all zero, while
    members 0 and 1 advance (``_run`` checks both at every step; here: that it did, for as many steps as the gate predicts)."""
    _capi()
    snaps, saw = _cache.get((kind, "padded", 16)) or _run(gpu_ctx, kind, "padded", 16, 3, _pers(), alone=False)
    assert saw["gated_checks"] == [0, 48 // N_PER, GATED_STEPS] and GATED_STEPS == 8
    assert saw["others_advanced"][2] == GATED_STEPS and saw["others_advanced"][1] == 2      # member 0 had done 8 (2) updates when member 2 (1) was last seen gated
    assert snaps[2]["counters"][2] == STEPS - GATED_STEPS


# ---- 2, 6 (a population without per=) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_mixed_population(kind, gpu_ctx, restore_settings):
    """Members (prioritised, uniform, prioritised): the uniform member equals the lone learner without ``per`` (``_run``) and the same member of a population
    without ``per=`` -- which in turn equals its lone uniform learners, as before this feature."""
    capi = _capi()
    pers = _pers()
    mixed, _ = _run(gpu_ctx, kind, "padded", 16, 3, [pers[0], None, pers[2]])
    plain, _ = _run(gpu_ctx, kind, "padded", 16, 3, None)
    assert mixed[1]["tree"] is None and all(s["tree"] is None for s in plain)
    _same(kind, mixed[1], plain[1], "the uniform member vs a population without per=")
    full = _cache.get((kind, "padded", 16))
    if full is not None:                                            # its neighbours are what they are next to a prioritised member 1
        _same(kind, mixed[0], full[0][0], "member 0")
        _same(kind, mixed[2], full[0][2], "member 2")
    assert not np.array_equal(mixed[0]["params"]["critic"]["w1"], plain[0]["params"]["critic"]["w1"])      # prioritisation changed member 0's run
    # priorities() / last_sample() on a uniform member raise
    Pop, _ = _classes(kind)
    env = _stub_env(gpu_ctx, 32)
    pop = Pop(env, [_cfg(kind, "padded", 16, m) for m in range(2)], per=[pers[0], None])
    pop.member(0).priorities()
    for call in (pop.member(1).priorities, pop.member(1).last_sample):
        with pytest.raises(capi.StmpcError, match="not enabled"):
            call()
    gpu_ctx.check_error()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_members_are_independent(kind, gpu_ctx, restore_settings):
    """Only member 1's PERConfig and seed change: members 0 and 2 end with the bits they had, trees included; member 1 does not."""
    _capi()
    before = _cache.get((kind, "padded", 16)) or _run(gpu_ctx, kind, "padded", 16, 3, _pers(), alone=False)
    after, _ = _run(gpu_ctx, kind, "padded", 16, 3, _pers(alpha=(ALPHA[0], 0.7, ALPHA[2]), beta=(BETA[0], 1.0, BETA[2]), max_priority=(MAX_PRIORITY[0], 3.0, MAX_PRIORITY[2])),
                    seeds=(SEEDS[0], 99, SEEDS[2]), alone=False)
    _same(kind, before[0][0], after[0], "member 0")
    _same(kind, before[0][2], after[2], "member 2")
    assert not np.array_equal(before[0][1]["tree"], after[1]["tree"]) and not np.array_equal(before[0][1]["ring"], after[1]["ring"])
    assert not np.array_equal(before[0][1]["params"]["critic"]["w1"], after[1]["params"]["critic"]["w1"])


# ---- synthetic populations: rings filled by the population's push of rows, no env ---------------------------------------------------------------------
def _synthetic(gpu_ctx, kind, P, per, B=16, capacity=CAP, n_per=N_PER, replay_start=0):
    """(population, replay): P members at the padded shape with test_td3_pop's starting networks, nothing pushed; ``replay``: 256 synthetic rows."""
    Pop, _ = _classes(kind)
    pop = Pop(_stub_env(gpu_ctx, P * n_per), [_cfg(kind, "padded", B, m, capacity=capacity, replay_start=replay_start) for m in range(P)], seeds=list(SEEDS[:P]),
              init=[_nets(kind, "padded", m) for m in range(P)], per=per)
    return pop, random_td3_problem("padded", B, seed=80)[2]


def _pop_push(pop, replay, first, n_per):
    """Rows first + m * 7 ... of ``replay`` (modulo its 256) into member m, through the population's own push."""
    rows = np.concatenate([(first + 7 * m + np.arange(n_per)) % 256 for m in range(pop.P)])
    pop.push(_dev(replay["obs"][rows]), _dev(replay["ticks"][rows]), _dev(replay["action"][rows]), _dev(replay["reward"][rows]), _dev(replay["next_obs"][rows]),
             _dev(replay["terminated"][rows]), _dev(replay["truncated"][rows]))


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_power_of_two_capacity(kind, gpu_ctx, restore_settings):
    """Capacity 64 = the leaf count, P = 2, three pushes of 24 of which the third wraps: the trees equal ``SumTreeHost``; then updates keep them exact."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    pers = _pers()[:2]
    pop, replay = _synthetic(gpu_ctx, kind, 2, pers, capacity=64)
    host = [learner.SumTreeHost(64, g) for g in pers]
    for m in range(2):
        assert np.array_equal(pop.member(m).priorities(), host[m].nodes) and host[m].nodes.size == 127
    for j in range(3):
        _pop_push(pop, replay, 24 * j, N_PER)
        for m in range(2):
            host[m].push(N_PER)
            tree = pop.member(m).priorities()
            assert np.array_equal(_bits(tree), _bits(host[m].nodes)) and internal_nodes_are_exact(tree), (j, m)
    assert host[0].fill == 64 and host[0].cursor == 8 and list(pop.stats()["fill"]) == [64, 64]
    pop.update(3)
    for m in range(2):
        tree = pop.member(m).priorities()
        assert internal_nodes_are_exact(tree) and not np.array_equal(tree, host[m].nodes) and (tree[63:] > 0).all()
    assert list(pop.stats()["updates"]) == [3, 3]
    gpu_ctx.check_error()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_population_of_one_equals_a_learner(kind, gpu_ctx, restore_settings):
    _capi()
    snaps, saw = _run(gpu_ctx, kind, "padded", 16, 1, _pers()[:1])
    assert snaps[0]["counters"][2] == STEPS and snaps[0]["tree"] is not None


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_prioritised_population_updates_are_reproducible(kind, gpu_ctx, restore_settings):
    """update(5) equals five update(1), B = 100 from rings of 200 with a push that wraps between the two rounds; two identical runs give identical trees."""
    _capi()
    out = []
    for single in (False, True, True):
        pop, replay = _synthetic(gpu_ctx, kind, 3, _pers(alpha=(0.6, 1.0, 0.5)), B=100, n_per=100)
        for first in (0, 100, 200):                                 # the third push wraps
            _pop_push(pop, replay, first, 100)
            if single:
                for _ in range(5):
                    pop.update(1)
            else:
                pop.update(5)
        members = [pop.member(m) for m in range(3)]
        out.append([(M.priorities(), M.state_dict(), M.last_sample()) for M in members])
        assert list(pop.stats()["updates"]) == [15, 15, 15]
    for other in out[1:]:
        for m, ((t0, s0, l0), (t1, s1, l1)) in enumerate(zip(out[0], other)):
            assert np.array_equal(_bits(t0), _bits(t1)) and internal_nodes_are_exact(t0), m
            assert _same_sample(l0, l1) and np.array_equal(s0["counters"], s1["counters"]), m
            for slot in s0["params"]:
                if isinstance(s0["params"][slot], dict):
                    assert all(np.array_equal(_bits(s0["params"][slot][k]), _bits(s1["params"][slot][k])) for k in s0["params"][slot]), (m, slot)
            assert np.array_equal(_bits(s0["params"]["beta_pow"]), _bits(s1["params"]["beta_pow"]))
    assert not np.array_equal(out[0][0][0], out[0][1][0])
    gpu_ctx.check_error()


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_refusals(kind, gpu_ctx, restore_settings):
    capi = _capi()
    E = capi.StmpcError
    pers = _pers()
    enable = gpu_ctx.td3_pop_per_enable if kind == "td3" else gpu_ctx.ddpg_pop_per_enable
    c = [g.to_c() for g in pers]
    # a second enable, whatever it asks for; the wrong number of entries; a cfg out of range
    pop, replay = _synthetic(gpu_ctx, kind, 3, [pers[0], None, pers[2]])
    for again in (c, [None, c[1], None], [None] * 3):
        with pytest.raises(E, match="already set up"):
            enable(pop.handle, again)
    with pytest.raises(E):                                          # (the lone entry on a member: still refused, and it says why)
        gpu_ctx.per_enable(pop.member(1).handle, c[1])
    with pytest.raises(E, match="population"):
        gpu_ctx.per_enable(pop.member(1).handle, c[1])
    with pytest.raises(E, match="population"):
        gpu_ctx.per_enable(pop.member(0).handle, c[0])
    fresh, _ = _synthetic(gpu_ctx, kind, 3, None)
    with pytest.raises(E, match="2 entries, the population 3 members"):
        enable(fresh.handle, c[:2])
    bad = capi.PERCfg(alpha=0.5, beta=0.0, min_priority=0.0, max_priority=4.0)
    with pytest.raises(E, match="min_priority > 0"):
        enable(fresh.handle, [c[0], bad, None])
    with pytest.raises(E, match="not enabled"):                     # the refused call attached nothing, to member 0 either
        fresh.member(0).priorities()
    # enable after a push
    _pop_push(fresh, replay, 0, N_PER)
    with pytest.raises(E, match="empty"):
        enable(fresh.handle, c)
    with pytest.raises(E, match="empty"):
        enable(fresh.handle, [None, None, c[2]])
    fresh.update(1)                                                 # ... and the population goes on, uniform
    assert list(fresh.stats()["updates"]) == [1, 1, 1]
    # set_state: a prioritised member's cursor and fill stay; a uniform member's move
    _pop_push(pop, replay, 0, N_PER)
    pop.update(1)
    for m in (0, 2, 1):
        h = pop.member(m).handle
        cn, bp = gpu_ctx.ddpg_get_state(h)
        assert (cn[0], cn[1]) == (N_PER, N_PER)
        for i in (0, 1):
            moved = cn.copy()
            moved[i] -= 1
            if m == 1:
                gpu_ctx.ddpg_set_state(h, moved, bp)
                assert gpu_ctx.ddpg_get_state(h)[0][i] == N_PER - 1
            else:
                with pytest.raises(E, match="cursor and fill cannot be set"):
                    gpu_ctx.ddpg_set_state(h, moved, bp)
        pop.member(m).load_state_dict(pop.member(m).state_dict())   # everything else can be set
    gpu_ctx.check_error()


# ---- the debug entries on a borrowed member ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_member_debug_entries(kind, gpu_ctx, restore_settings):
    """minibatch() / grads() / targets() of a prioritised member run their own, ungated sampling step and equal the lone learner's, before and after
    updates; a gated member's (replay_start 199 of 48 frames) sampling step runs too."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    _, Lone = _classes(kind)
    pers = _pers()
    Pop, _ = _classes(kind)
    cfg = lambda m, per=None: _cfg(kind, "padded", 16, m, per=per, replay_start=(0, 0, CAP - 1)[m])
    pop = Pop(_stub_env(gpu_ctx, 3 * N_PER), [cfg(m) for m in range(3)], seeds=list(SEEDS), init=[_nets(kind, "padded", m) for m in range(3)], per=pers)
    replay = random_td3_problem("padded", 16, seed=80)[2]
    lone = [Lone(20, cfg(m, pers[m]), seed=SEEDS[m], init=_nets(kind, "padded", m), ctx=gpu_ctx) for m in range(3)]
    for j in range(2):
        _pop_push(pop, replay, 24 * j, N_PER)
        for m, L in enumerate(lone):
            _push(L, replay, (24 * j + 7 * m + np.arange(N_PER)) % 256)
        for m, L in enumerate(lone):
            M = pop.member(m)
            assert np.array_equal(_bits(M.minibatch()), _bits(L.minibatch())), (j, m)
            ls = M.last_sample()
            assert _same_sample(ls, L.last_sample()) and ls["weight"].max() == 1.0, (j, m)
            assert np.array_equal(ls["idx"], learner.per_sample_host(M.priorities(), SEEDS[m], M.stats()["updates"], 16, N_PER * (j + 1))), (j, m)
            for g, want in zip(M.grads(), L.grads()):
                assert all(np.array_equal(_bits(g[k]), _bits(want[k])) and np.abs(g[k]).max() > 0 for k in learner.TENSORS), (j, m)
            if kind == "td3":
                assert np.array_equal(_bits(M.targets()), _bits(L.targets())), (j, m)
            assert _same_sample(M.last_sample(), L.last_sample()), (j, m)
        pop.update(2)
        for L in lone:
            L.update(2)
    assert list(pop.stats()["updates"]) == [4, 4, 0]
    for m, L in enumerate(lone):
        assert np.array_equal(_bits(pop.member(m).priorities()), _bits(L.priorities())), m
    gpu_ctx.check_error()


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_training_loop(kind, restore_settings):
    """train_ddpg, unedited, on a traffic-group env with a population of prioritised members: member m on traffic m."""
    capi = _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import episodes, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n, P, steps = N_PER, 2, 8
    tr = [dict(episodes.TRAFFIC_TYPES[t], seed=s) for t, s in (("low", 31), ("fast", 33))]
    ctx = capi.Context(-1)
    env = vec_env.MergeVecEnv(P * n, env_id="sumo-jerk-continuous-v0", ctx=ctx, traffic=tr)
    Pop, _ = _classes(kind)
    pers = [learner.PERConfig(), learner.PERConfig(alpha=1.0, beta=0.4)]
    pop = Pop(env, [_cfg(kind, "padded", 16, m, replay_start=n) for m in range(P)], seeds=[5, 6], init=[_nets(kind, "padded", m) for m in range(P)], per=pers)
    res = learner.train_ddpg(env, pop, frames=steps * P * n, drain_every=4)
    env.check_error()
    st = pop.stats()
    assert res["steps"] == steps and list(st["fill"]) == [steps * n] * P and list(st["updates"]) == [steps - 1] * P      # the first push does not open the gate
    assert all(np.isfinite(v).all() for v in st.values()) and len(res["member_returns"]) == P
    for m in range(P):
        M = pop.member(m)
        sd = M.state_dict()["params"]
        assert all(np.isfinite(sd[s][k]).all() for s in sd if isinstance(sd[s], dict) for k in learner.TENSORS)
        tree, g = M.priorities(), pers[m]
        leaf = tree[255:]
        assert tree[0] > 0 and internal_nodes_are_exact(tree) and not leaf[steps * n:].any()
        assert (leaf[:steps * n] >= learner.per_pow(g.min_priority, g.alpha)).all() and (leaf[:steps * n] <= learner.per_pow(g.max_priority, g.alpha)).all()
        assert np.unique(leaf[:steps * n]).size > 16                # seven minibatches of 16 have set priorities of their own
    del pop, env
    ctx.close()
