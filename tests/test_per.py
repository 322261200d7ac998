"""Prioritised replay on the GPU (learner.PERConfig on DDPGLearner / TD3Learner, csrc/stmpc_per_kernels.hpp, stmpc_per_*).  Twins: test_per_cpu.py;
helpers and problems: learner_testlib.py -- random_td3_problem at the small network 20-40-24, ring rows pushed from its 256 synthetic rows.

Bit for bit wherever the arithmetic allows it: the tree after pushes and after priority updates (alpha 0.5 and 1: sqrt and the identity are correctly
rounded on both sides), the sampled rows for any alpha (the twin descends the device's own tree), weights at beta 0, reproducibility, the gate.
Elsewhere: the weights within 4 float32 ulps of the float64 twin (both sides compute in fp64 and may differ by a few fp64 ulps of pow, which moves
the float32 rounding by at most one step); gradients and ten updates under the parity rule (learner_testlib.check_4x) -- error = max-abs difference to the float64 twin
over its max-abs, bound = 4 x the float32 twin's same error, floor 8 float32 ulps -- the twins fed the device's own rows and weights.
"""
import numpy as np
import pytest

from learner_testlib import (SEED, bits64 as _bits, bits_equal as _bits_equal, check_4x as _check_4x, ddpg_view, internal_nodes_are_exact, push as _push,
                             random_td3_problem, record as _record, rel_err as _rel_err)
from stmpc_testlib import capi as _capi

KINDS = ["ddpg", "td3"]
B2_MIN = 0.05


def _problem(B, lo=21, **kw):
    """``random_td3_problem`` at 20-40-24 under the first generator seed >= lo whose three output biases are at least B2_MIN in magnitude (a property
    of the draw alone).  Ten Adam steps at lr 5e-4 ... 1e-3 move a scalar by up to 1e-2, and k_ddpg_adam's float32 bias corrections put a few 1e-6
    of relative error on what they move (test_td3_cpu.test_float32_adam_on_a_zero_initialised_scalar: the statement the suite pins bit for bit); on
    a bias drawn as small as that sum the parity rule would measure those corrections, not the update.  From 0.05 on they stay below its floor."""
    for seed in range(lo, lo + 64):
        cfg, params, replay = random_td3_problem("padded", B, seed=seed, **kw)
        if min(abs(float(params[s]["b2"][0])) for s in ("actor", "critic", "critic2")) >= B2_MIN:
            return cfg, params, replay
    raise AssertionError("no seed found")


def _make(gpu_ctx, kind, B, per, capacity=256, seed=SEED, **kw):
    """(learner, cfg, params, replay): a lone learner of ``kind`` on _problem's nets (a DDPG learner: without critic 2), nothing pushed."""
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = _problem(B, capacity=capacity, per=per, **kw)
    if kind == "td3":
        L = learner.TD3Learner(cfg.n_obs, cfg, seed=seed, init=(params["actor"], params["critic"], params["critic2"]), ctx=gpu_ctx)
    else:
        cfg = learner.DDPGConfig(n_obs=cfg.n_obs, h1=cfg.h1, h2=cfg.h2, batch=B, capacity=capacity, replay_start=cfg.replay_start, gamma=cfg.gamma, tau=cfg.tau,
                                 lr_q=cfg.lr_q, lr_pi=cfg.lr_pi, time_scale=cfg.time_scale, action_low=cfg.action_low, action_high=cfg.action_high, per=per)
        params = ddpg_view(params)
        L = learner.DDPGLearner(cfg.n_obs, cfg, seed=seed, init={"actor": params["actor"], "critic": params["critic"]}, ctx=gpu_ctx)
    L.load_state_dict({"params": params, "counters": None})
    return L, cfg, params, replay


def _slots(kind):
    capi = _capi()
    return capi.DDPG_SLOTS + (capi.TD3_SLOTS if kind == "td3" else ())


def _twin(kind, params, batch, cfg, dtype, weights, eps=None, grads_only=False):
    from rl_mpc_lanemerging_amd import learner
    if kind == "td3":
        return learner.update_host_td3(params, batch, cfg, dtype, eps=eps, weights=weights, grads_only=grads_only)
    return learner.update_host(params, batch, cfg, dtype, weights=weights, grads_only=grads_only)


def _eps(kind, L):
    """The device's smoothing noise of the next update's rows (TD3; it also runs the sampling step, as the update will)."""
    return L.targets()[:, 0].astype(np.float64) if kind == "td3" else None


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("capacity", [37, 64])
def test_gpu_tree_after_pushes(kind, capacity, gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import learner
    for alpha in (0.5, 1.0):
        per = learner.PERConfig(alpha=alpha)
        L, cfg, params, replay = _make(gpu_ctx, kind, 16, per, capacity=capacity)
        t = learner.SumTreeHost(capacity, per)
        assert np.array_equal(L.priorities(), t.nodes) and t.nodes.size == 127
        first = 0
        for n in (5, 16, 30, 30):                                   # 37: the third wraps; 64: the fourth
            _push(L, replay, slice(first, first + n))
            first += n
            t.push(n)
            tree = L.priorities()
            assert np.array_equal(_bits(tree), _bits(t.nodes)), (alpha, n)
            assert internal_nodes_are_exact(tree)
            cn = gpu_ctx.ddpg_get_state(L.handle)[0]
            assert (cn[0], cn[1]) == (t.cursor, t.fill)
        assert t.fill == capacity and tree[0] == capacity * (2.0 if alpha == 0.5 else 4.0) and not tree[63 + capacity:].any()
    gpu_ctx.check_error()


# ---- 2, 4 (beta 0) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [24, 100])
def test_gpu_sampling_equals_the_twin_on_the_device_tree(kind, B, gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import learner
    L, cfg, params, replay = _make(gpu_ctx, kind, B, learner.PERConfig(alpha=0.7))
    _push(L, replay, slice(0, 200))
    ring = gpu_ctx.ddpg_replay_read(L.handle, 0, 200)
    seen = set()
    for u in range(4):
        tree = L.priorities()
        want = learner.per_sample_host(tree, SEED, u, B, 200)
        mb = L.minibatch()
        assert np.array_equal(L.last_sample()["idx"], want), u       # the debug entry draws what the update will
        L.update(1)
        ls = L.last_sample()
        assert ls["idx"].dtype == np.int64 and np.array_equal(ls["idx"], want), u
        assert np.array_equal(mb.view(np.uint32), ring[want].view(np.uint32)), u
        assert np.array_equal(ls["weight"], np.ones(B, dtype=np.float32))           # beta = 0: exactly 1
        assert not np.array_equal(L.priorities(), tree)
        seen.add(tuple(want))
    assert len(seen) == 4 and L.stats()["updates"] == 4
    assert not np.array_equal(want, learner.sample_indices_host(SEED, 3, B, 200))
    gpu_ctx.check_error()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_gpu_priority_update_equals_the_twin(kind, alpha, gpu_ctx, restore_settings):
    """B = 48 rows from 20 filled: duplicates in every minibatch.  The tree after an update is the tree before it with set(idx_r, priority(td_r)) applied
    in row order.  TD3: |td| is the larger of |Q1 - y| and |Q2 - y|, Q_i by the float64 twin on the rows, y from targets(); bound 64 float32 ulps of
    max(1, |Q|, |y|): three layers whose float32 roundings of O(1) activations pass through weight rows of 1-norm below 4 (fan-ins 22, 40, 24)."""
    import torch
    from rl_mpc_lanemerging_amd import learner
    per = learner.PERConfig(alpha=alpha)
    L, cfg, params, replay = _make(gpu_ctx, kind, 48, per)
    _push(L, replay, slice(0, 20))
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    either = [False, False]
    for u in range(3):
        tree = L.priorities()
        if kind == "td3":
            y = L.targets()[:, 4].astype(np.float64)
            rows, p = L.minibatch(), L.state_dict()["params"]
        L.update(1)
        ls = L.last_sample()
        assert len(set(ls["idx"])) < 48 and ls["idx"].max() < 20
        t = learner.SumTreeHost(cfg.capacity, per)
        t.nodes = tree.copy()
        for i, w in zip(ls["idx"], learner.per_priority_host(ls["td"], per)):
            t.set(i, w)
        after = L.priorities()
        assert np.array_equal(_bits(after), _bits(t.nodes)), u
        assert internal_nodes_are_exact(after) and not np.array_equal(after, tree) and np.abs(ls["td"]).max() > 0
        if kind == "td3":
            b = learner.batch_from_rows(rows, cfg.n_obs)
            x = torch.cat([T(b["s"]), T(b["a"])[:, None]], 1)
            q = [learner._mlp({k: T(p[s][k]) for k in learner.TENSORS}, x).numpy() for s in ("critic", "critic2")]
            want = np.maximum(np.abs(q[0] - y), np.abs(q[1] - y))
            tol = 64 * 2.0 ** -23 * max(1.0, np.abs(q[0]).max(), np.abs(q[1]).max(), np.abs(y).max())
            err = np.abs(np.abs(ls["td"].astype(np.float64)) - want).max()
            print("update %d: |td| against max(|Q1 - y|, |Q2 - y|): worst %.3e, bound %.3e" % (u, err, tol))
            assert err <= tol
            either = [either[c] or bool((np.abs(q[c] - y) > np.abs(q[1 - c] - y) + 2 * tol).any()) for c in (0, 1)]
    assert kind != "td3" or all(either)                             # either critic set some row's priority
    gpu_ctx.check_error()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_importance_weights(kind, gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import learner
    L, cfg, params, replay = _make(gpu_ctx, kind, 100, learner.PERConfig(alpha=0.5, beta=0.4))
    _push(L, replay, slice(0, 200))
    worst = 0.0
    for u in range(4):
        tree = L.priorities()
        L.update(1)
        ls = L.last_sample()
        want = learner.per_weights_host(tree, ls["idx"], 200, 0.4)
        ulps = np.abs(ls["weight"].astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        print("update %d: weights against the float64 twin: worst %.2f float32 ulps; smallest weight %.4f" % (u, ulps.max(), ls["weight"].min()))
        assert ulps.max() <= 4 and ls["weight"].max() == 1.0 and ls["weight"].min() > 0
        if u:
            assert ls["weight"].min() < 0.9                           # the priorities have spread: the correction is not trivial
    _record("per_weights_max_ulps_%s" % kind, worst)
    gpu_ctx.check_error()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [16, 100])
def test_gpu_gradients_against_the_float64_twin(kind, B, gpu_ctx, restore_settings):
    """grads() after two updates (so that priorities and weights have spread) vs the float64 twin fed the rows at the device's idx, the device's
    weights and (TD3) the device's smoothing noise; B = 100 is also the padded-rows case."""
    from rl_mpc_lanemerging_amd import learner
    L, cfg, params, replay = _make(gpu_ctx, kind, B, learner.PERConfig(alpha=0.5, beta=0.4))
    _push(L, replay, slice(0, 200))
    L.update(2)
    sd = L.state_dict()
    ring = gpu_ctx.ddpg_replay_read(L.handle, 0, 200)
    eps = _eps(kind, L)
    g = L.grads()
    ls = L.last_sample()
    assert np.array_equal(ls["idx"], learner.per_sample_host(L.priorities(), SEED, 2, B, 200)) and ls["weight"].max() == 1.0
    batch = learner.batch_from_rows(ring[ls["idx"]], cfg.n_obs)
    _, i64 = _twin(kind, sd["params"], batch, cfg, "float64", ls["weight"], eps, grads_only=True)
    _, i32 = _twin(kind, sd["params"], batch, cfg, "float32", ls["weight"], eps, grads_only=True)
    _, plain = _twin(kind, sd["params"], batch, cfg, "float64", None, eps, grads_only=True)
    names = ("grad_actor", "grad_critic") + (("grad_critic2",) if kind == "td3" else ())
    ratios, ok = {}, True
    for name, dev in zip(names, g):
        for k in learner.TENSORS:
            assert np.abs(i64[name][k]).max() > 0, (name, k)
            ok &= _check_4x("%s B%d %s.%s" % (kind, B, name, k), dev[k], i32[name][k], i64[name][k], ratios)
    _record("per_gradients_%s_B%d" % (kind, B), ratios)
    assert ok, ratios
    assert _rel_err(plain["grad_critic"]["w1"], i64["grad_critic"]["w1"]) > 1e-3          # the weights matter to the gradient checked
    after = L.state_dict()["params"]
    assert _bits_equal(after, sd["params"], _slots(kind)) and after["updates"] == 2
    gpu_ctx.check_error()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_ten_updates_against_the_twin_loop(kind, gpu_ctx, restore_settings):
    """Sample, update, reprioritise, ten times; the float64 and float32 twins are fed the device's idx, weights and (TD3) smoothing noise at each step."""
    from rl_mpc_lanemerging_amd import learner
    L, cfg, params, replay = _make(gpu_ctx, kind, 100, learner.PERConfig(alpha=0.5, beta=0.4))
    _push(L, replay, slice(0, 200))
    ring = gpu_ctx.ddpg_replay_read(L.handle, 0, 200)
    p64 = p32 = L.state_dict()["params"]
    for u in range(10):
        eps = _eps(kind, L)
        L.update(1)
        ls = L.last_sample()
        batch = learner.batch_from_rows(ring[ls["idx"]], cfg.n_obs)
        p64, _ = _twin(kind, p64, batch, cfg, "float64", ls["weight"], eps)
        p32, _ = _twin(kind, p32, batch, cfg, "float32", ls["weight"], eps)
    new = L.state_dict()["params"]
    assert new["updates"] == 10
    ratios, ok = {}, True
    for slot in _slots(kind):
        if slot.endswith(("_m", "_v")):
            continue
        for k in learner.TENSORS:
            ok &= _check_4x("%s 10 updates %s.%s" % (kind, slot, k), new[slot][k], p32[slot][k], p64[slot][k], ratios)
    _record("per_ten_updates_%s_B100" % kind, ratios)
    assert ok, ratios
    gpu_ctx.check_error()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_prioritised_updates_are_reproducible(kind, gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import learner
    out = []
    for single in (False, True):
        L, cfg, params, replay = _make(gpu_ctx, kind, 100, learner.PERConfig(alpha=0.6, beta=0.4), capacity=128)
        first = 0
        for n in (100, 50):                                         # the second push wraps
            _push(L, replay, slice(first, first + n))
            first += n
            if single:
                for _ in range(5):
                    L.update(1)
            else:
                L.update(5)
        out.append((L.priorities(), L.state_dict(), L.last_sample()))
    (t0, s0, l0), (t1, s1, l1) = out
    assert np.array_equal(_bits(t0), _bits(t1)) and internal_nodes_are_exact(t0) and s0["params"]["updates"] == 10
    assert _bits_equal(s0["params"], s1["params"], _slots(kind)) and np.array_equal(s0["params"]["beta_pow"], s1["params"]["beta_pow"])
    assert np.array_equal(s0["counters"], s1["counters"]) and all(np.array_equal(l0[k], l1[k]) for k in l0)
    gpu_ctx.check_error()


# ---- 8, and the refusals that need a device -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_gate_and_refusals(kind, gpu_ctx, restore_settings):
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    per = learner.PERConfig()
    L, cfg, params, replay = _make(gpu_ctx, kind, 32, per, replay_start=150)
    _push(L, replay, slice(0, 100))
    tree, sd = L.priorities(), L.state_dict()
    L.update(3)                                                     # 100 frames: not more than replay_start
    ls = L.last_sample()
    assert np.array_equal(_bits(L.priorities()), _bits(tree)) and not ls["idx"].any() and not ls["weight"].any() and not ls["td"].any()
    after = L.state_dict()
    assert _bits_equal(after["params"], sd["params"], _slots(kind)) and after["params"]["updates"] == 0
    _push(L, replay, slice(100, 200))
    tree = L.priorities()
    L.update(1)
    assert L.stats()["updates"] == 1 and not np.array_equal(L.priorities(), tree)
    # the counters under the tree cannot be moved; everything else can
    cn, bp = gpu_ctx.ddpg_get_state(L.handle)
    for i in (0, 1):
        bad = cn.copy()
        bad[i] -= 1
        with pytest.raises(capi.StmpcError):
            gpu_ctx.ddpg_set_state(L.handle, bad, bp)
    L.load_state_dict(L.state_dict())
    with pytest.raises(capi.StmpcError):                            # a second enable
        gpu_ctx.per_enable(L.handle, per.to_c())
    # a ring that is not empty; a member of a population
    U, _, _, _ = _make(gpu_ctx, kind, 32, None)
    with pytest.raises(capi.StmpcError):
        U.priorities()
    _push(U, replay, slice(0, 10))
    with pytest.raises(capi.StmpcError, match="empty"):
        gpu_ctx.per_enable(U.handle, per.to_c())
    if kind == "td3":
        pop = gpu_ctx.td3_pop_create([cfg.to_c_td3(0), cfg.to_c_td3(1)])
        member = gpu_ctx.td3_base(gpu_ctx.td3_pop_member(pop, 1))
    else:
        pop = gpu_ctx.ddpg_pop_create([cfg.to_c(0), cfg.to_c(1)])
        member = gpu_ctx.ddpg_pop_member(pop, 1)
    with pytest.raises(capi.StmpcError, match="population"):
        gpu_ctx.per_enable(member, per.to_c())
    (gpu_ctx.td3_pop_destroy if kind == "td3" else gpu_ctx.ddpg_pop_destroy)(pop)
    gpu_ctx.check_error()


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_training_loop_with_prioritised_replay(kind, gpu_ctx, restore_settings):
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n, cap, steps = 64, 1000, 40                                    # 2560 frames into 1000 rows of 1024 leaves: wraps, 24 leaves never filled
    env = vec_env.MergeVecEnv(n, env_id="sumo-jerk-continuous-v0", seed=5, ctx=gpu_ctx)
    per = learner.PERConfig()
    Cfg, Lrn = (learner.TD3Config, learner.TD3Learner) if kind == "td3" else (learner.DDPGConfig, learner.DDPGLearner)
    L = Lrn(env, Cfg(n_obs=env.obs_dim, h1=40, h2=24, batch=32, capacity=cap, replay_start=4 * n, per=per), seed=5)
    res = learner.train_ddpg(env, L, frames=steps * n, updates_per_step=2)
    env.check_error()
    st = L.stats()
    assert res["steps"] == steps and st["fill"] == cap and st["updates"] == 2 * (steps - 4) and np.isfinite(st["critic_loss"])
    sd = L.state_dict()["params"]
    assert all(np.isfinite(sd[s][k]).all() for s in _slots(kind) for k in learner.TENSORS) and np.abs(sd["actor"]["w2"]).max() > 0
    tree = L.priorities()
    leaf = tree[1023:]
    assert tree[0] > 0 and internal_nodes_are_exact(tree)
    assert (leaf[:cap] >= learner.per_pow(per.min_priority, per.alpha)).all() and (leaf[:cap] <= learner.per_pow(per.max_priority, per.alpha)).all()
    assert not leaf[cap:].any() and np.unique(leaf[:cap]).size > 100
