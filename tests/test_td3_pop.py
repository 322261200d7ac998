"""A population of TD3 learners on the GPU (learner.TD3Population, csrc/stmpc_td3_pop_kernels.hpp, stmpc_pop_td3_*).  CPU part: test_td3_pop_cpu.py.

Every comparison is bit equality against the lone ``TD3Learner`` (or, for degenerate members, against ``DDPGPopulation``): the population's kernels
are the lone learner's bodies on the member ``blockIdx.z`` selects.  The only tolerance in this file is test_actor.py's 5e-5 between the actor
kernel and the acting kernel (two float32 evaluations of one network), as test_td3.py uses it.

Shapes: "padded" 20-40-24 of learner_testlib.SHAPES, rings of at most 256 rows, B in {16, 48}; the shipped 400 x 300 once, at B = 100.

The gate in test 1.  A learner's ``replay_start`` must lie below its capacity (``stmpc_ddpg_create``), and the members of a population share the
capacity and the frames per step.  With capacity 200 (so that every ring wraps) and 12 steps of 24 frames no legal ``replay_start`` keeps a gate
shut for the whole run: member 2 has the largest legal one, 199, so its gate is shut during steps 1 ... 8 -- it stays at 0 updates while members
0 and 1 advance -- and opens at step 9, inside the run.  A gate that stays shut THROUGHOUT is test 2's member 3 (255 frames, replay_start 255).
"""
import numpy as np
import pytest

from learner_testlib import (CAP, N_PER, RING, SHAPES, SHIPPED, STEPS, assert_same_td3 as _assert_same_td3, ddpg_view, degenerate, dev as _dev, push as _push,
                             random_td3_problem, snapshot as _snapshot, stats_row as _stats_row, stub_env as _stub_env, td3_init as _init)
from stmpc_testlib import (ACTOR_N_PER as VIEW_N, actor_eval as _eval, actor_settings as _settings, actor_states as _states, assert_steps_equal as _assert_steps_equal,
                           bits as _bits, capi as _capi)

SEEDS = (11, 12, 13)
GAMMA, TAU, NOISE = (0.99, 0.95, 0.9), (0.005, 0.01, 0.02), (0.1, 0.2, 0.05)
LR_Q, LR_PI = (2e-4, 1e-3, 5e-4), (2e-4, 3e-4, 1e-4)
TARGET_NOISE, NOISE_CLIP, DELAY = (0.2, 0.1, 0.3), (0.5, 0.25, 0.4), (1, 2, 3)
REPLAY_START = (0, 48, CAP - 1)                # (module text: 199 is the largest a ring of 200 allows)
CASES = [pytest.param("padded", 16, id="padded-B16"), pytest.param("padded", 48, id="padded-B48"), pytest.param(SHIPPED, 100, id="400x300-B100")]
DELAYED = ("actor", "actor_m", "actor_v", "actor_target", "critic_target", "critic2_target")
STEPPED = ("critic", "critic_m", "critic_v", "critic2", "critic2_m", "critic2_v")
_cache = {}


def _slots():
    capi = _capi()
    return capi.DDPG_SLOTS + capi.TD3_SLOTS


def _same_slots(a, b, slots):
    from rl_mpc_lanemerging_amd import learner
    return all(np.array_equal(_bits(a[s][k]), _bits(b[s][k])) for s in slots for k in learner.TENSORS)


# ---- 1, 4: a population on a real env next to lone learners on its slices ------------------------------------------------------------------------------
def _cfgs(shape, B, P, seeds_of=None, delay=DELAY, target_noise=TARGET_NOISE):
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape] if isinstance(shape, str) else shape
    return [learner.TD3Config(n_obs=n_obs, h1=h1, h2=h2, batch=B, capacity=CAP, replay_start=REPLAY_START[m], gamma=GAMMA[m], tau=TAU[m], noise=NOISE[m],
                              lr_q=LR_Q[m], lr_pi=LR_PI[m], target_noise=target_noise[m], noise_clip=NOISE_CLIP[m], policy_delay=delay[m]) for m in range(P)]


def _run(gpu_ctx, shape, B, P, seeds=SEEDS, delay=DELAY, target_noise=TARGET_NOISE, alone=True):
    """STEPS steps of act -> env.step -> push -> update(1) of a population of P on one env of P * N_PER and, if ``alone``, of the same learners as
    lone TD3Learners on their slices, fed the same transitions.  Returns the members' snapshots (the population's)."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n = N_PER
    env = vec_env.MergeVecEnv(P * n, env_id="sumo-jerk-continuous-v0", seed=7, ctx=gpu_ctx)
    cfgs = _cfgs(shape, B, P, delay=delay, target_noise=target_noise)
    pop = learner.TD3Population(env, cfgs, seeds=list(seeds[:P]), init=[_init(shape, m) for m in range(P)])
    assert isinstance(pop, learner.DDPGPopulation) and gpu_ctx.td3_pop_size(pop.handle) == P == len(pop)
    lone = [learner.TD3Learner(env, cfgs[m], seed=seeds[m], init=_init(shape, m)) for m in range(P)] if alone else []
    sl = [slice(m * n, (m + 1) * n) for m in range(P)]
    lr_q, lr_pi = list(LR_Q[:P]), list(LR_PI[:P])
    obs = env.reset()
    for i in range(STEPS):
        ticks = env.episode_ticks.clone()
        action = pop.act(obs, ticks, noise=True).clone()
        if alone:
            a_lone = torch.cat([lone[m].act(obs[sl[m]], ticks[sl[m]], noise=True) for m in range(P)])
            assert np.array_equal(_bits(action.cpu().numpy()), _bits(a_lone.cpu().numpy())), "actions of step %d" % i     # before the env sees them
        nobs, r, term, trunc, info = env.step(action)
        fin = info["final_observation"]
        pop.push(obs, ticks, action, r, nobs, term, trunc, final_obs=fin)
        pop.update(1, lr_q=lr_q, lr_pi=lr_pi)
        for m, L in enumerate(lone):
            L.push(obs[sl[m]], ticks[sl[m]], action[sl[m]], r[sl[m]], nobs[sl[m]], term[sl[m]], trunc[sl[m]], final_obs=fin[sl[m]])
            L.update(1, lr_q=lr_q[m], lr_pi=lr_pi[m])
        obs = nobs
        # the gate is per member: updates done so far = the pushes after which MORE than replay_start frames were in
        want = [sum(1 for j in range(1, i + 2) if n * j > REPLAY_START[m]) for m in range(P)]
        have = pop.stats()["updates"]
        assert list(have) == want, (i, list(have), want)
        if P == 3 and n * (i + 1) <= REPLAY_START[2]:
            assert have[2] == 0 and have[0] == i + 1 and have[1] == max(0, i - 1)      # member 2 waits while members 0 and 1 advance
    torch.cuda.synchronize()
    env.check_error()
    ps = pop.stats()
    assert set(ps) == {"critic_loss", "critic2_loss", "mean_q", "mean_q2", "fill", "updates"} and all(len(v) == P for v in ps.values())
    snaps = [_snapshot(gpu_ctx, pop.member(m), _stats_row(ps, m)) for m in range(P)]
    for m, L in enumerate(lone):
        _assert_same_td3(snaps[m], _snapshot(gpu_ctx, L, _stats_row(L.stats_td3())), "member %d vs alone" % m)
    for m in range(P):
        c = snaps[m]["counters"]
        assert (c[0], c[1], c[3], c[4]) == ((n * STEPS) % CAP, CAP, STEPS, n * STEPS) and np.isfinite(snaps[m]["stats"][:4]).all()      # wrapped; own acting counter
    if P == 3:
        assert [int(s["counters"][2]) for s in snaps] == [12, 10, 4]
        assert not np.array_equal(snaps[0]["ring"], snaps[1]["ring"]) and not np.array_equal(snaps[0]["params"]["actor"]["w1"], snaps[2]["params"]["actor"]["w1"])
        # the actors stepped updates // policy_delay times (12 // 1, 10 // 2, 4 // 3): their beta powers, float32 running products of 0.9, say so
        steps = [round(float(np.log(s["params"]["beta_pow"][0]) / np.log(np.float32(0.9)))) for s in snaps]
        assert steps == [12 // delay[0], 10 // delay[1], 4 // delay[2]], steps
    return snaps


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B", CASES)
def test_gpu_population_equals_its_members_run_alone(shape, B, gpu_ctx, restore_settings):
    """P = 3, n = 24 (no multiple of the 16-row acting tile), capacity 200 (every ring wraps), members that differ in seed, gamma, tau, acting noise,
    learning rates, target_noise, noise_clip, policy_delay (1, 2, 3) and replay_start (module text)."""
    _capi()
    _cache[shape, B] = _run(gpu_ctx, shape, B, 3)


@pytest.mark.gpu
def test_gpu_members_are_independent(gpu_ctx, restore_settings):
    """Only member 1's seed, policy_delay and target_noise change: members 0 and 2 end bit-identical to before, member 1 does not."""
    _capi()
    before = _cache.get(("padded", 16)) or _run(gpu_ctx, "padded", 16, 3, alone=False)
    after = _run(gpu_ctx, "padded", 16, 3, seeds=(SEEDS[0], 99, SEEDS[2]), delay=(DELAY[0], 5, DELAY[2]), target_noise=(TARGET_NOISE[0], 0.05, TARGET_NOISE[2]),
                 alone=False)
    _assert_same_td3(before[0], after[0], "member 0")
    _assert_same_td3(before[2], after[2], "member 2")
    assert not np.array_equal(before[1]["ring"], after[1]["ring"])
    assert not np.array_equal(before[1]["params"]["critic2"]["w1"], after[1]["params"]["critic2"]["w1"])


# ---- synthetic populations: rings filled by push of rows, no env -------------------------------------------------------------------------------------
def _triple(params):
    return (params["actor"], params["critic"], params["critic2"])


def _synthetic(gpu_ctx, problems, seeds, rows=None, n_per=16, cls=None):
    """A population whose member m has problem m's cfg and parameters (targets included) and the ``rows[m]`` of its replay in the ring."""
    from rl_mpc_lanemerging_amd import learner
    cls = cls or learner.TD3Population
    P = len(problems)
    td3 = cls is learner.TD3Population
    init = [_triple(p) if td3 else {"actor": p["actor"], "critic": p["critic"]} for _, p, _ in problems]
    pop = cls(_stub_env(gpu_ctx, P * n_per, problems[0][0].n_obs), [c for c, _, _ in problems], seeds=list(seeds), init=init)
    for m, (_, params, replay) in enumerate(problems):
        M = pop.member(m)
        M.load_state_dict({"params": params, "counters": None})
        _push(M, replay, rows[m] if rows else slice(None))          # (the single-learner push on a borrowed member is legal)
    return pop


def _lone(gpu_ctx, problem, seed, rows=slice(None)):
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = problem
    L = learner.TD3Learner(cfg.n_obs, cfg, seed=seed, init=_triple(params), ctx=gpu_ctx)
    L.load_state_dict({"params": params, "counters": None})
    _push(L, replay, rows)
    return L


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_delay_schedule_per_member(gpu_ctx, restore_settings):
    """Members with policy_delay 3, 2, 1 and a fourth whose gate stays shut throughout (255 frames, replay_start 255), seven update(1) calls."""
    _capi()
    delays = (3, 2, 1, 2)
    problems = [random_td3_problem("padded", 48, seed=20 + m, policy_delay=delays[m], replay_start=RING - 1 if m == 3 else 0) for m in range(4)]
    pop = _synthetic(gpu_ctx, problems, seeds=(31, 32, 33, 34), rows=[slice(None)] * 3 + [slice(0, RING - 1)])
    prev = [pop.member(m).state_dict() for m in range(4)]
    assert prev[3]["counters"][4] == RING - 1 and prev[0]["counters"][4] == RING
    for u in range(1, 8):
        pop.update(1)
        new = [pop.member(m).state_dict() for m in range(4)]
        for m in range(3):
            due = u % delays[m] == 0
            a, b = new[m]["params"], prev[m]["params"]
            for slot in DELAYED:
                assert _same_slots(a, b, (slot,)) != due, (u, m, slot)
            assert np.array_equal(_bits(a["beta_pow"][:2]), _bits(b["beta_pow"][:2])) != due, (u, m)
            assert all(not _same_slots(a, b, (slot,)) for slot in STEPPED), (u, m)
            assert not np.array_equal(a["beta_pow"][2:], b["beta_pow"][2:]) and a["updates"] == u
        assert _same_slots(new[3]["params"], prev[3]["params"], _slots()) and np.array_equal(_bits(new[3]["params"]["beta_pow"]), _bits(prev[3]["params"]["beta_pow"]))
        assert np.array_equal(new[3]["counters"], prev[3]["counters"]) and new[3]["params"]["updates"] == 0
        prev = new
    assert list(pop.stats()["updates"]) == [7, 7, 7, 0]
    gpu_ctx.check_error()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_population_of_one_equals_a_learner(gpu_ctx, restore_settings):
    """P = 1 through the population's own act / push / update against one lone TD3Learner: everything bitwise equal after six updates."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = problem = random_td3_problem("padded", 48, seed=41)
    pop = learner.TD3Population(_stub_env(gpu_ctx, RING), (cfg, 1), seeds=[43], init=_triple(params))      # one triple: for every member
    pop.member(0).load_state_dict({"params": params, "counters": None})
    L = _lone(gpu_ctx, problem, 43, rows=slice(0, 0))
    L.load_state_dict({"params": params, "counters": None})
    obs, ticks = _dev(replay["obs"]), _dev(replay["ticks"])
    for noise in (True, False):
        assert np.array_equal(_bits(pop.act(obs, ticks, noise=noise).cpu().numpy()), _bits(L.act(obs, ticks, noise=noise).cpu().numpy())), noise
    _push(pop, replay)
    _push(L, replay)
    for u in range(6):
        pop.update(1)
        L.update(1)
    st = pop.stats()
    _assert_same_td3(_snapshot_ring(gpu_ctx, pop.member(0), _stats_row(st, 0)), _snapshot_ring(gpu_ctx, L, _stats_row(L.stats_td3())), "P = 1")
    assert st["updates"][0] == 6 and not _same_slots(pop.member(0).state_dict()["params"], params, ("actor", "critic", "critic2", "actor_target"))
    gpu_ctx.check_error()


def _snapshot_ring(gpu_ctx, L, stats):
    """learner_testlib.snapshot for a ring of RING rows."""
    sd = L.state_dict()
    return {"params": sd["params"], "counters": sd["counters"], "ring": gpu_ctx.ddpg_replay_read(L.handle, 0, RING), "stats": stats}


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_degenerate_population_is_a_ddpg_population(gpu_ctx, restore_settings):
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    raw = [random_td3_problem("padded", 48, seed=50 + m, gamma=GAMMA[m], tau=TAU[m], lr_q=LR_Q[m], lr_pi=LR_PI[m]) for m in range(3)]
    deg = [degenerate(c, p) + (r,) for c, p, r in raw]
    T = _synthetic(gpu_ctx, deg, seeds=SEEDS)
    D = _synthetic(gpu_ctx, [(c, ddpg_view(p), r) for (c, _, r), (_, p, _) in zip(deg, raw)], seeds=SEEDS, cls=learner.DDPGPopulation)
    for u in range(6):
        T.update(1)
        D.update(1)
    st, sd = T.stats(), D.stats()
    for m in range(3):
        a, b = T.member(m).state_dict(), D.member(m).state_dict()
        assert _same_slots(a["params"], b["params"], capi.DDPG_SLOTS), m
        for slot in ("critic", "critic_target", "critic_m", "critic_v"):
            assert _same_slots({slot: a["params"][slot.replace("critic", "critic2")]}, b["params"], (slot,)), (m, slot)
        assert np.array_equal(_bits(a["params"]["beta_pow"][:4]), _bits(b["params"]["beta_pow"])) and np.array_equal(a["params"]["beta_pow"][4:], b["params"]["beta_pow"][2:])
        assert np.array_equal(a["counters"], b["counters"]) and a["counters"][2] == 6
        assert np.array_equal(_bits(gpu_ctx.ddpg_replay_read(T.member(m).handle, 0, RING)), _bits(gpu_ctx.ddpg_replay_read(D.member(m).handle, 0, RING)))
        assert (st["critic_loss"][m], st["mean_q"][m]) == (st["critic2_loss"][m], st["mean_q2"][m]) == (sd["critic_loss"][m], sd["mean_q"][m])
        assert not _same_slots(a["params"], raw[m][1], ("actor", "critic", "actor_target", "critic_target"))
    gpu_ctx.check_error()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_member_handles(gpu_ctx, restore_settings):
    """targets / grads of a member equal the lone learner's; state_dict round-trips through a member; a view of a member's actor."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor, learner
    problems = [random_td3_problem("padded", 48, seed=60 + m, policy_delay=1 + m) for m in range(3)]
    pop = _synthetic(gpu_ctx, problems, seeds=SEEDS)
    lone = [_lone(gpu_ctx, problems[m], SEEDS[m]) for m in range(3)]
    for _ in range(2):
        for m in range(3):
            M = pop.member(m)
            assert isinstance(M, learner.TD3Learner)
            assert np.array_equal(_bits(M.targets()), _bits(lone[m].targets())), m
            for g, want in zip(M.grads(), lone[m].grads()):
                assert all(np.array_equal(_bits(g[k]), _bits(want[k])) and np.abs(g[k]).max() > 0 for k in learner.TENSORS), m
            assert M.stats_td3() == lone[m].stats_td3() and M.stats() == lone[m].stats()
        pop.update(2)
        for L in lone:
            L.update(2)
    # state_dict -> two more updates -> load_state_dict: the member is back, bit for bit, and continues as the lone learner does from there
    M = pop.member(1)
    saved = M.state_dict()
    assert set(saved["params"]) >= set(_slots()) and saved["params"]["beta_pow"].shape == (6,) and saved["params"]["updates"] == 4
    pop.update(2)
    assert not _same_slots(M.state_dict()["params"], saved["params"], ("critic", "critic2"))
    M.load_state_dict(saved)
    got = M.state_dict()
    assert _same_slots(got["params"], saved["params"], _slots()) and np.array_equal(_bits(got["params"]["beta_pow"]), _bits(saved["params"]["beta_pow"]))
    assert np.array_equal(got["counters"], saved["counters"])
    pop.update(1)
    lone[1].update(1)
    a, b = M.state_dict(), lone[1].state_dict()
    assert _same_slots(a["params"], b["params"], _slots()) and np.array_equal(_bits(a["params"]["beta_pow"]), _bits(b["params"]["beta_pow"])) and a["params"]["updates"] == 5
    # a view of member 1's actor at the shipped shape: the lone learner's view bit for bit, and the population's own greedy action on that slice
    g, S = _settings()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _states(g, dev)
    sprob = [random_td3_problem(SHIPPED, 16, seed=70 + m) for m in range(2)]
    spop = _synthetic(gpu_ctx, sprob, seeds=SEEDS[:2], n_per=VIEW_N)
    slone = _lone(gpu_ctx, sprob[1], SEEDS[1])
    spop.update(2)
    slone.update(2)
    got = _eval(gpu_ctx, S, actor.DDPGActor.from_learner(spop.member(1), VIEW_N, gpu_ctx, S), st)
    _assert_steps_equal(got, _eval(gpu_ctx, S, actor.DDPGActor.from_learner(slone, VIEW_N, gpu_ctx, S), st), "member 1's view")
    feat, jerk = got[0]["feat"], got[0]["jerk"]
    ticks = np.rint(feat[:, 20] / 0.001).astype(np.int32)
    assert np.array_equal(np.float32(0.001) * ticks.astype(np.float32), feat[:, 20])
    obs2, ticks2 = np.zeros((2 * VIEW_N, 20), np.float32), np.zeros(2 * VIEW_N, np.int32)
    obs2[VIEW_N:], ticks2[VIEW_N:] = feat[:, :20], ticks
    greedy = spop.act(_dev(obs2), _dev(ticks2), noise=False).cpu().numpy()[VIEW_N:]
    assert np.array_equal(_bits(greedy), _bits(slone.act(_dev(feat[:, :20]), _dev(ticks), noise=False).cpu().numpy()))
    assert np.abs(greedy - jerk).max() < 5e-5 and np.abs(jerk).max() > 1e-3       # (test_actor.py's bound between the two float32 evaluations)
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_population_validation(gpu_ctx, restore_settings):
    """What the library refuses, with its message; nothing is launched: no counter of a refused population moves and no error is pending."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    n = 16
    env = _stub_env(gpu_ctx, 3 * n)
    ok = dict(n_obs=20, h1=40, h2=24, batch=16, capacity=CAP, replay_start=0)
    for odd in (dict(h1=56), dict(h2=40), dict(batch=32), dict(capacity=CAP + 1)):
        cfgs = [learner.TD3Config(**ok), learner.TD3Config(**dict(ok, **odd)), learner.TD3Config(**ok)]
        with pytest.raises(capi.StmpcError, match="share n_obs, h1, h2, batch and capacity .member 1 differs"):
            learner.TD3Population(env, cfgs)
    for P in (0, 65):
        with pytest.raises(capi.StmpcError, match="a population has 1 ... 64 members, not %d" % P):
            learner.TD3Population(_stub_env(gpu_ctx, 0 if P == 0 else 65), (learner.TD3Config(**ok), P))
    with pytest.raises(capi.StmpcError, match="policy_delay must be at least 1"):      # a member's own validation is stmpc_td3_create's
        learner.TD3Population(env, [learner.TD3Config(**ok), learner.TD3Config(policy_delay=0, **ok), learner.TD3Config(**ok)])
    pop = learner.TD3Population(env, (learner.TD3Config(**ok), 3))
    rng = np.random.default_rng(5)
    obs, nobs = _dev(rng.normal(0, 1, (3 * n, 20)).astype(np.float32)), _dev(rng.normal(0, 1, (3 * n, 20)).astype(np.float32))
    ticks, rew, flag = _dev(rng.integers(0, 100, 3 * n).astype(np.int32)), _dev(rng.normal(0, 1, 3 * n)), _dev(np.zeros(3 * n, bool))
    action = pop.act(obs, ticks).clone()
    pop.push(obs, ticks, action, rew, nobs, flag, flag)
    h, E = pop.handle, capi.StmpcError
    for bad in ([1e-3, 1e-3], [1e-3] * 4):
        with pytest.raises(E, match="learning-rate arrays have %d entries, the population 3 members" % len(bad)):
            pop.update(1, lr_q=bad, lr_pi=bad)
    with pytest.raises(E, match="learning rate is negative"):
        pop.update(1, lr_q=[1e-3, -1.0, 1e-3])
    with pytest.raises(E, match="learning rate is negative"):
        pop.update(1, lr_pi=[1e-3, 1e-3, -1e-9])
    with pytest.raises(E, match="n_updates is negative"):
        pop.update(-1)
    for bad_n in (0, CAP + 1):
        with pytest.raises(E, match="n_per_member must be in 1 ... capacity"):
            gpu_ctx.td3_pop_act(h, bad_n, obs.data_ptr(), 20, ticks.data_ptr(), False, action.data_ptr())
        with pytest.raises(E, match="n_per_member must be in 1 ... capacity"):
            gpu_ctx.td3_pop_push(h, bad_n, obs.data_ptr(), nobs.data_ptr(), 0, 20, ticks.data_ptr(), 0, action.data_ptr(), rew.data_ptr(), flag.data_ptr(), flag.data_ptr())
    with pytest.raises(E, match="obs_stride"):
        gpu_ctx.td3_pop_act(h, n, obs.data_ptr(), 19, ticks.data_ptr(), False, action.data_ptr())
    with pytest.raises(E, match="NULL device pointer"):
        gpu_ctx.td3_pop_act(h, n, 0, 20, ticks.data_ptr(), False, action.data_ptr())
    with pytest.raises(E, match="NULL device pointer"):
        gpu_ctx.td3_pop_push(h, n, obs.data_ptr(), nobs.data_ptr(), 0, 20, ticks.data_ptr(), 0, action.data_ptr(), 0, flag.data_ptr(), flag.data_ptr())
    with pytest.raises(E, match="NULL argument"):
        gpu_ctx.td3_pop_stats(h, 0)
    with pytest.raises(E, match="population is NULL"):
        gpu_ctx.td3_pop_act(None, n, obs.data_ptr(), 20, ticks.data_ptr(), False, action.data_ptr())
    with pytest.raises(E, match="no such member"):
        gpu_ctx.td3_pop_member(h, 3)
    with pytest.raises(ValueError, match="32 rows given"):
        pop.act(obs[:32], ticks[:32])
    st = pop.stats()
    assert list(st["updates"]) == [0, 0, 0] and list(st["fill"]) == [n] * 3
    assert [int(pop.member(m).state_dict()["counters"][3]) for m in range(3)] == [1, 1, 1]      # one noisy acting call each, no more
    pop.update(1, lr_q=1e-3, lr_pi=[1e-3, 2e-3, 3e-3])             # a scalar and an array of the right length are both fine
    assert list(pop.stats()["updates"]) == [1, 1, 1]
    pop.member(1).update(1)                                        # a single-member call on a borrowed member stays legal and moves that member alone
    torch.cuda.synchronize()
    assert list(pop.stats()["updates"]) == [1, 2, 1]
    gpu_ctx.check_error()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shielded", [False, True], ids=["traffic-groups", "first-step-shield"])
def test_gpu_training_loop(shielded, restore_settings):
    """train_ddpg and evaluate_members, unedited, take a TD3Population: member m on traffic m, on a plain env and behind the first-step shield."""
    capi = _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import episodes, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n, P, steps = 24, 2, 8
    tr = [dict(episodes.TRAFFIC_TYPES[t], seed=s) for t, s in (("low", 31), ("fast", 33))]
    ctx = capi.Context(-1)
    make = vec_env.GroupedShieldVecEnv if shielded else vec_env.MergeVecEnv
    env = make(P * n, env_id="sumo-jerk-continuous-v0", ctx=ctx, traffic=tr)
    cfgs = [learner.TD3Config(n_obs=env.obs_dim, h1=40, h2=24, batch=16, capacity=CAP, replay_start=n, policy_delay=1 + m) for m in range(P)]
    pop = learner.TD3Population(env, cfgs, seeds=[5, 6], init=[_init("padded", m) for m in range(P)])
    sched = lambda i, total: (2e-4, np.array([2e-4, 1e-4]))        # a schedule may return scalars or per-member arrays
    res = learner.train_ddpg(env, pop, frames=steps * P * n, drain_every=4, lr_schedule=sched, executed_actions=shielded)
    env.check_error()
    st = pop.stats()
    assert res["steps"] == steps and res["frames"] == steps * P * n and list(st["fill"]) == [steps * n] * P and list(st["updates"]) == [steps - 1] * P
    assert np.isfinite(st["critic_loss"]).all() and np.isfinite(st["critic2_loss"]).all() and 0.0 <= res["takeover_share"] <= 1.0
    assert len(res["member_returns"]) == P and sum(r.size for r in res["member_returns"]) == res["episodes"] == res["returns"].size
    a0, a1 = (pop.member(m).state_dict()["params"] for m in range(P))
    assert all(np.isfinite(a0[s][k]).all() and np.isfinite(a1[s][k]).all() for s in _slots() for k in learner.TENSORS)
    assert not np.array_equal(a0["actor"]["w1"], a1["actor"]["w1"])
    S = pkg.Settings
    out = learner.evaluate_members(pop, n_per_member=8, seed=5, max_episode_length=3.5 * S.TICK_LENGTH)
    assert len(out["by_member"]) == P and np.array_equal(out["stats"]["member"], np.arange(P * 8) // 8) and out["reports"] is None
    del pop, env
    ctx.close()
