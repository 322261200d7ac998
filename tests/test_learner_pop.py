"""A population of DDPG learners (learner.DDPGPopulation, csrc/stmpc_ddpg_pop_kernels.hpp, stmpc_ddpg_pop_* of include/stmpc.h).

CPU: header / library / binding agree on the new entries; ``DDPGPopulation`` refuses an env it cannot split before it touches the device.
GPU: a population equals its members run alone as plain ``DDPGLearner``s on their slices of the same env, bit for bit (actions at every step;
parameters, counters, beta powers, rings and statistics at the end); members do not depend on each other; the library's validation; the
training loop and the export of a member's actor.  Everything at the shipped 400/300 network shape.  No tolerance anywhere except the actor
export's 5e-5 (test_actor.py's): the members run the single learner's own arithmetic.
"""
import numpy as np
import pytest

from learner_testlib import CAP, N_PER, STEPS, assert_same as _assert_same, snapshot as _snapshot
from stmpc_testlib import bits as _bits, capi as _capi, header_prototypes, header_text, linit as _init

SEEDS = (11, 12, 13)
GAMMA, TAU, NOISE = (0.99, 0.95, 0.9), (0.005, 0.01, 0.02), (0.1, 0.2, 0.05)
LR_Q, LR_PI = (2e-4, 1e-3, 5e-4), (2e-4, 3e-4, 1e-4)
REPLAY_START = (0, 48, 120)                    # member 2 is still gated while members 0 and 1 update
_cache = {}


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_population():
    capi = _capi()
    lib = capi.load()
    header = header_text(flat=True)
    declared = header_prototypes("stmpc_ddpg_pop_")
    assert set(declared) >= {"stmpc_ddpg_pop_create", "stmpc_ddpg_pop_destroy", "stmpc_ddpg_pop_member", "stmpc_ddpg_pop_act_device",
                             "stmpc_ddpg_pop_push_device", "stmpc_ddpg_pop_update_device", "stmpc_ddpg_pop_stats_device"}
    assert set(declared) == {n for n in capi.EXPORTS if n.startswith("stmpc_ddpg_pop_")}
    for name, args in declared.items():
        fn = getattr(lib, name)                                   # (AttributeError: the library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")), name
    assert "#define STMPC_DDPG_POP_MAX %d" % capi.DDPG_POP_MAX in header and capi.DDPG_POP_MAX == 64
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8 and "#define STMPC_ABI_VERSION 8" in header


def test_population_refuses_an_env_it_cannot_split_before_touching_the_device():
    _capi()
    from rl_mpc_lanemerging_amd import learner

    class Env:                                                    # an env whose context must not be asked for
        n, obs_dim, continuous = 70, 20, True

        @property
        def ctx(self):
            raise AssertionError("the device was touched")
    cfg = learner.DDPGConfig(n_obs=20, batch=16, capacity=CAP, replay_start=0)
    with pytest.raises(ValueError, match="70 is not a multiple of the population's 3 members"):
        learner.DDPGPopulation(Env(), (cfg, 3))
    with pytest.raises(ValueError, match="70 is not a multiple"):
        learner.DDPGPopulation(Env(), [cfg] * 4, seeds=[1, 2, 3, 4])
    Env.continuous = False
    with pytest.raises(ValueError, match="continuous"):
        learner.DDPGPopulation(Env(), (cfg, 2))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _cfgs(B, P, gamma=GAMMA):
    from rl_mpc_lanemerging_amd import learner
    return [learner.DDPGConfig(n_obs=20, batch=B, capacity=CAP, replay_start=REPLAY_START[m], gamma=gamma[m], tau=TAU[m], noise=NOISE[m], lr_q=LR_Q[m],
                               lr_pi=LR_PI[m]) for m in range(P)]


def _run(gpu_ctx, B, P, seeds=SEEDS, gamma=GAMMA, alone=True):
    """STEPS steps of act -> env.step -> push -> update(1) of a population of P on one env of P * N_PER and, if ``alone``, of the same learners
    as plain DDPGLearners on their slices, fed the same transitions.  Returns the members' snapshots (the population's)."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n = N_PER
    env = vec_env.MergeVecEnv(P * n, env_id="sumo-jerk-continuous-v0", seed=7, ctx=gpu_ctx)
    cfgs = _cfgs(B, P, gamma)
    pop = learner.DDPGPopulation(env, cfgs, seeds=list(seeds[:P]), init=[_init(m) for m in range(P)])
    lone = [learner.DDPGLearner(env, cfgs[m], seed=seeds[m], init=_init(m)) for m in range(P)] if alone else []
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
            assert have[2] == 0 and have[0] == i + 1
    torch.cuda.synchronize()
    env.check_error()
    ps = pop.stats()
    snaps = [_snapshot(gpu_ctx, pop.member(m), [ps["critic_loss"][m], ps["mean_q"][m], float(ps["fill"][m]), float(ps["updates"][m])]) for m in range(P)]
    for m, L in enumerate(lone):
        s = L.stats()
        _assert_same(snaps[m], _snapshot(gpu_ctx, L, [s["critic_loss"], s["mean_q"], float(s["fill"]), float(s["updates"])]), "member %d vs alone" % m)
    for m in range(P):
        c = snaps[m]["counters"]
        assert (c[0], c[1], c[3], c[4]) == ((n * STEPS) % CAP, CAP, STEPS, n * STEPS) and np.isfinite(snaps[m]["stats"][0])      # wrapped; own acting counter
    if P == 3:
        assert snaps[2]["counters"][2] == 7 < snaps[1]["counters"][2] == 10 < snaps[0]["counters"][2] == 12
        assert not np.array_equal(snaps[0]["ring"], snaps[1]["ring"]) and not np.array_equal(snaps[0]["params"]["actor"]["w1"], snaps[2]["params"]["actor"]["w1"])
    return snaps


@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 100])
def test_gpu_population_equals_its_members_run_alone(B, gpu_ctx, restore_settings):
    """P = 3 (odd, > 2: a swapped member index shows), n = 24 (no multiple of the 16-row acting tile: the local-row noise key matters), B = 100 (padded
    minibatch rows), capacity 200 (wraps), members that differ in seed, gamma, tau, noise, learning rates and replay_start."""
    _capi()
    _cache[B] = _run(gpu_ctx, B, 3)


@pytest.mark.gpu
def test_gpu_population_of_one_equals_a_learner(gpu_ctx, restore_settings):
    _capi()
    _run(gpu_ctx, 100, 1)


@pytest.mark.gpu
def test_gpu_members_are_independent(gpu_ctx, restore_settings):
    """Only member 1's seed and gamma change: members 0 and 2 end bit-identical to before, member 1 does not."""
    _capi()
    before = _cache.get(16) or _run(gpu_ctx, 16, 3, alone=False)
    after = _run(gpu_ctx, 16, 3, seeds=(SEEDS[0], 99, SEEDS[2]), gamma=(GAMMA[0], 0.8, GAMMA[2]), alone=False)
    _assert_same(before[0], after[0], "member 0")
    _assert_same(before[2], after[2], "member 2")
    assert not np.array_equal(before[1]["ring"], after[1]["ring"])
    assert not np.array_equal(before[1]["params"]["critic"]["w1"], after[1]["params"]["critic"]["w1"])


@pytest.mark.gpu
def test_gpu_population_validation(gpu_ctx, restore_settings):
    """What the library refuses, with its message; nothing is launched: the counters of a population whose update was refused do not move."""
    capi = _capi()
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(3 * N_PER, env_id="sumo-jerk-continuous-v0", seed=7, ctx=gpu_ctx)
    ok = dict(n_obs=20, batch=16, capacity=CAP, replay_start=0)
    for odd in (dict(h1=384), dict(batch=32), dict(capacity=CAP + 1)):
        cfgs = [learner.DDPGConfig(**ok), learner.DDPGConfig(**dict(ok, **odd)), learner.DDPGConfig(**ok)]
        with pytest.raises(capi.StmpcError, match="share n_obs, h1, h2, batch and capacity .member 1 differs"):
            learner.DDPGPopulation(env, cfgs)
    for P in (0, 65):
        with pytest.raises(capi.StmpcError, match="a population has 1 ... 64 members, not %d" % P):
            learner.DDPGPopulation(env, (learner.DDPGConfig(**ok), P))
    pop = learner.DDPGPopulation(env, (learner.DDPGConfig(**ok), 3))
    obs = env.reset()
    ticks = env.episode_ticks.clone()
    action = pop.act(obs, ticks).clone()
    nobs, r, term, trunc, info = env.step(action)
    pop.push(obs, ticks, action, r, nobs, term, trunc, final_obs=info["final_observation"])
    for bad in ([1e-3, 1e-3], [1e-3] * 4):
        with pytest.raises(capi.StmpcError, match="learning-rate arrays have %d entries, the population 3 members" % len(bad)):
            pop.update(1, lr_q=bad, lr_pi=bad)
    with pytest.raises(capi.StmpcError, match="learning rate is negative"):
        pop.update(1, lr_q=[1e-3, -1.0, 1e-3])
    with pytest.raises(ValueError, match="48 rows given"):
        pop.act(obs[:48], ticks[:48])
    with pytest.raises(capi.StmpcError, match="no such member"):
        gpu_ctx.ddpg_pop_member(pop.handle, 3)
    st = pop.stats()
    assert list(st["updates"]) == [0, 0, 0] and list(st["fill"]) == [N_PER] * 3
    pop.update(1, lr_q=1e-3, lr_pi=[1e-3, 2e-3, 3e-3])             # a scalar and an array of the right length are both fine
    assert list(pop.stats()["updates"]) == [1, 1, 1]
    # a single-member call on a borrowed member stays legal and moves that member alone
    pop.member(1).update(1)
    torch.cuda.synchronize()
    assert list(pop.stats()["updates"]) == [1, 2, 1]
    env.check_error()


@pytest.mark.gpu
def test_gpu_population_training_loop_and_export(gpu_ctx, restore_settings, tmp_path):
    _capi()
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n = 32
    env = vec_env.MergeVecEnv(2 * n, env_id="sumo-jerk-continuous-v0", seed=5, ctx=gpu_ctx)
    cfg = learner.DDPGConfig(n_obs=env.obs_dim, capacity=4096, replay_start=32)
    pop = learner.DDPGPopulation(env, (cfg, 2), seeds=[5, 6], init="medium1")
    sched = lambda i, steps: (2e-4, np.array([2e-4, 1e-4]))       # a schedule may return scalars or per-member arrays
    res = learner.train_ddpg(env, pop, frames=10 * 2 * n, drain_every=4, lr_schedule=sched)
    env.check_error()
    st = pop.stats()
    assert res["steps"] == 10 and list(st["fill"]) == [10 * n] * 2 and list(st["updates"]) == [9, 9] and np.isfinite(st["critic_loss"]).all()
    assert len(res["member_returns"]) == 2 and sum(r.size for r in res["member_returns"]) == res["episodes"] == res["returns"].size
    assert np.array_equal(np.sort(np.concatenate(res["member_returns"])), np.sort(res["returns"]))
    # member 1's actor, exported, is what the population acts with on member 1's slice
    path = pop.member(1).export_actor(str(tmp_path / "actor_member1.npz"))
    w = actor.load_weights(path)
    assert all(np.array_equal(w[k], pop.member(1).state_dict()["params"]["actor"][k]) for k in learner.TENSORS)
    assert not np.array_equal(w["w1"], pop.member(0).state_dict()["params"]["actor"]["w1"])
    obs, ticks = env._obs[env._cur], env.episode_ticks.clone()
    greedy = pop.act(obs, ticks, noise=False).cpu().numpy()[n:]
    pol = actor.DDPGActor(path, n, gpu_ctx, pkg.Settings, engine="torch")
    feat = torch.cat([obs, (np.float32(0.001) * ticks.to(torch.float32)).unsqueeze(1)], 1)[n:]
    with torch.no_grad():
        want = pol.forward(feat).cpu().numpy()
    assert np.abs(greedy - want).max() < 5e-5 and np.abs(want).max() > 0
