"""The dueling head of the C51 learner on the GPU (``learner.C51Config(dueling=True)``, c51_dueling_combine and the dense backward of
csrc/stmpc_c51_kernels.hpp, k_c51actor_eval) against its host twins at the shapes of tests/discrete_testlib.py, (n_obs, h1, A, K, B) =
(20, 16, 2, 16, 5), (20, 16, 5, 17, 7), (12, 32, 3, 33, 16), (20, 48, 19, 51, 33), (20, 256, 5, 51, 64).  Rings have 128 rows, the learner's seed is 11.

Parity rule for float32 results (tests/learner_testlib.py's): per tensor, max-norm error against ``update_host_c51("float64")`` fed the device's own
minibatch rows at most max(4 x the error of ``update_host_c51("float32")``, 8 float32 ulps)."""
import ctypes as C

import numpy as np
import pytest

from discrete_testlib import (C51_DUELING as HEAD, LEARNER_SEED, NAMES, PROBLEM_SEEDS as _PROBLEM_SEEDS, Q_SLOTS, RING, SHAPES as _SHAPES, WIDE_A as _WIDE_A, all_negative_rows, astar_rows,
                              expected_values_host as _expected_values_host, fill as _fill, make_learner as _learner, minibatch_host, pad_mask,
                              pads_are_zero as _pads_are_zero, random_problem, rows_of, stub_env as _stub_env, twins as _twins)
from learner_testlib import FLOOR, bits_equal, bound_4x, check_4x as _check_4x, rel_err
from stmpc_testlib import capi as _capi

SHAPES, PROBLEM_SEEDS = _SHAPES["c51_dueling"] + _WIDE_A["c51_dueling"], _PROBLEM_SEEDS["c51_dueling"]      # tests/discrete_testlib.py's tables; the last index is the head's shape of WIDE_A

# ---- 1: distributions, loss, targets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_gpu_distributions_loss_and_targets(si, double, gpu_ctx, restore_settings):
    """dist() and targets() against the twin fed the device's own minibatch rows, on minibatches where some rows have only negative expected values
    at s'.  a* is compared where the float64 twin's two best values differ by more than the parity bound; at most 10 % of the rows are left out."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    shape = SHAPES[si]
    n_obs, h1, A, K, B = shape
    cfg, params, replay = random_problem(HEAD, shape, PROBLEM_SEEDS[si, double], neg_shift=True, double=double)
    L = _learner(gpu_ctx, HEAD, cfg, params, replay)
    rows = L.minibatch()
    assert L.stats()["fill"] == RING and np.array_equal(rows.view(np.uint32), minibatch_host(replay, cfg)[0].view(np.uint32))
    batch = learner.dqn_batch_from_rows(rows, n_obs)
    i64, i32 = _twins(HEAD, params, batch, cfg)
    neg = all_negative_rows(i64)
    assert neg.any() and not neg.all(), int(neg.sum())
    d, t = L.dist()
    assert d.dtype == t.dtype == np.float32 and d.shape == (B, 2, K) and t.shape == (B, 4) and np.array_equal(t, L.targets())
    tag = "c51 dueling %s %s " % (shape, "double" if double else "plain")
    ok = _check_4x(tag + "m", d[:, 0], i32["dist"][:, 0], i64["dist"][:, 0])
    ok &= _check_4x(tag + "p(s, a)", d[:, 1], i32["dist"][:, 1], i64["dist"][:, 1])
    ok &= _check_4x(tag + "Qt(s', a*)", t[:, 1], i32["targets"][:, 1], i64["targets"][:, 1])
    ok &= _check_4x(tag + "row loss", t[:, 2], i32["row_loss"], i64["row_loss"])
    ok &= _check_4x(tag + "Q(s, a)", t[:, 3], i32["q_values"], i64["q_values"])
    keep, left_out = astar_rows(i64, i32)
    assert left_out <= 0.10
    assert np.array_equal(t[keep, 0].astype(np.int64), i64["targets"][keep, 0].astype(np.int64)) and t[:, 0].min() >= 0 and t[:, 0].max() < A
    assert np.abs(d[:, 0].astype(np.float64).sum(1) - 1).max() <= 8 * FLOOR and np.abs(d[:, 1].astype(np.float64).sum(1) - 1).max() <= 8 * FLOOR
    assert ok
    st = L.stats()
    assert abs(st["loss"] - i64["loss"]) <= 1e-5 * abs(i64["loss"]) and abs(st["mean_q"] - i64["mean_q"]) <= 1e-5 * np.abs(i64["q_values"]).max()
    after = L.state_dict()
    assert bits_equal(after["params"], params, Q_SLOTS, NAMES) and after["params"]["updates"] == 0 and after["dueling"] is True
    gpu_ctx.check_error()


# ---- 2: gradients ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_gpu_gradients(si, gpu_ctx, restore_settings):
    """All four gradient tensors under the parity rule.  dZout is dense: the value block equals (w / B)(p - m) under the rule, advantage block b
    that times ((b == a) - 1 / A); pad columns and padded rows are exact zeros; per k the A advantage blocks sum to zero within four times what the
    float32 twin's sum shows.  The padded gradient slot's pads are exact zeros."""
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    shape = SHAPES[si]
    n_obs, h1, A, K, B = shape
    W = HEAD.width(shape)
    cfg, params, replay = random_problem(HEAD, shape, 320 + si)
    L = _learner(gpu_ctx, HEAD, cfg, params, replay)
    batch = learner.dqn_batch_from_rows(L.minibatch(), n_obs)
    i64, i32 = _twins(HEAD, params, batch, cfg)
    g = L.grads()
    ok = True
    for k in NAMES:
        assert g[k].dtype == np.float32 and g[k].shape == i64["grad"][k].shape == params["q"][k].shape and np.abs(i64["grad"][k]).max() > 0
        ok &= _check_4x("c51 dueling %s grad %s" % (shape, k), g[k], i32["grad"][k], i64["grad"][k])
    pad = pad_mask(n_obs, h1, W)
    _pads_are_zero(gpu_ctx, HEAD, L, [capi.C51_GRAD], pad, "grads")
    have = gpu_ctx.c51_padded_read(L.handle, capi.C51_GRAD, h1, W)
    assert all(np.array_equal(have[k][~pad[k]].reshape(g[k].shape), g[k]) for k in NAMES)
    dz = gpu_ctx.c51_dzout_read(L.handle, B, W)
    assert dz.shape == ((B + 15) & ~15, (W + 15) & ~15) and not dz[B:].any() and not dz[:, W:].any()
    blocks = dz[:B, :W].reshape(B, A + 1, K)

    def want(i):                                                    # [B][A + 1][K] in the twin's dtype: g ((b == a) - 1 / A), and g for the value block
        f = i["dist"].dtype.type
        gk = (i["dist"][:, 1] - i["dist"][:, 0]) / f(B)
        coef = (np.arange(A)[None, :] == np.asarray(batch["a"])[:, None]).astype(i["dist"].dtype) - f(1) / f(A)
        return np.concatenate([coef[:, :, None] * gk[:, None, :], gk[:, None, :]], 1)
    w32, w64 = want(i32), want(i64)
    ok &= _check_4x("c51 dueling %s dZout value block" % (shape,), blocks[:, A], w32[:, A], w64[:, A])
    ok &= _check_4x("c51 dueling %s dZout advantage blocks" % (shape,), blocks[:, :A], w32[:, :A], w64[:, :A])
    assert (np.abs(blocks).max(2) > 0).all()
    tol = max(4 * np.abs(w32[:, :A].astype(np.float64).sum(1)).max(), FLOOR * np.abs(w64).max())
    assert np.abs(blocks[:, :A].astype(np.float64).sum(1)).max() <= tol, (np.abs(blocks[:, :A].astype(np.float64).sum(1)).max(), tol)
    assert ok
    gpu_ctx.check_error()


# ---- 3: Adam and the target copy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_gpu_adam_and_target_copy(si, gpu_ctx, restore_settings):
    """Four updates across target_period = 3: weights and moments equal dqn_adam_host fed the device's own gradient, bit for bit; the target is the
    online net after update 3 and unchanged otherwise; every pad of the five padded arrays stays an exact zero."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    shape = SHAPES[si]
    n_obs, h1, A, K, B = shape
    cfg, params, replay = random_problem(HEAD, shape, 340 + si, target_period=3)
    L = _learner(gpu_ctx, HEAD, cfg, params, replay)
    pad = pad_mask(n_obs, h1, HEAD.width(shape))
    for u in range(4):
        before = L.state_dict()["params"]
        g = L.grads()
        L.update(1)
        after = L.state_dict()["params"]
        for k in NAMES:
            w, m, v, bp = learner.dqn_adam_host(before["q"][k], g[k], before["q_m"][k], before["q_v"][k], before["beta_pow"], cfg.lr, cfg)
            assert np.array_equal(after["q"][k], w) and np.array_equal(after["q_m"][k], m) and np.array_equal(after["q_v"][k], v), (u, k)
            assert np.array_equal(after["q_target"][k], after["q"][k] if (u + 1) % 3 == 0 else before["q_target"][k]), (u, k)
            assert not np.array_equal(after["q"][k], before["q"][k])
        assert np.array_equal(after["beta_pow"], bp) and after["updates"] == u + 1
        _pads_are_zero(gpu_ctx, HEAD, L, range(5), pad, "update %d" % u)
    st = L.stats()
    assert st["updates"] == 4 and st["fill"] == RING and np.isfinite(st["loss"]) and st["loss"] > 0
    gpu_ctx.check_error()


# ---- 4: acting and evaluation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("si", [0, 3, 4, 5])
def test_gpu_acting(si, gpu_ctx, restore_settings):
    """act with eps = 0: the expected values against the twin under the rule, the index their first maximum; exploring draws are the plain head's."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    shape = SHAPES[si]
    n_obs, h1, A, K, B = shape
    cfg, params, replay = random_problem(HEAD, shape, 360 + si)
    L = _learner(gpu_ctx, HEAD, cfg, params, seed=23)
    n = 50                                                          # four tiles, the last one partly filled
    obs = torch.as_tensor(replay["s"][:n].astype(np.float32), device="cuda")
    q = torch.zeros(n, A, dtype=torch.float32, device="cuda")
    greedy = L.act(obs, None, eps=0.0, debug_q=q).cpu().numpy().copy()
    qh = q.cpu().numpy()
    assert greedy.dtype == np.int32 and np.array_equal(greedy, qh.argmax(1))
    ev = _expected_values_host(params["q"], replay["s"][:n], cfg)
    assert _check_4x("c51 dueling %s acting E[Z]" % (shape,), qh, ev["float32"], ev["float64"])
    a = L.act(obs, None, eps=0.25).cpu().numpy().copy()
    explore, idx = learner.dqn_act_host(23, 0, n, 0.25, A)
    assert np.array_equal(a, np.where(explore, idx, greedy)) and explore.any() and not explore.all()
    # ties: an all-zero last layer makes every distribution uniform and every expected value the same: action 0 everywhere
    sd = L.state_dict()
    sd["params"]["q"]["w1"][:] = 0
    sd["params"]["q"]["b1"][:] = 0
    L.load_state_dict(sd)
    assert (L.act(obs, None).cpu().numpy() == 0).all()
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("si", [1, 4])
def test_gpu_actors_give_the_bits_of_act(si, gpu_ctx, restore_settings, tmp_path):
    """C51Actor.from_learner (online and target) and an actor built from export_q give the expected values and the index that act gives on the same
    input vectors, bit for bit; the folded plain actor agrees in action wherever the twin's two best values differ by more than the bound."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor, learner
    from stmpc_testlib import actor_settings, actor_states
    shape = SHAPES[si]
    n_obs, h1, A, K, B = shape
    assert n_obs == 20
    g, S = actor_settings()
    st = actor_states(g, "cuda")
    n = st["ego5"].shape[0]
    cfg, params, _ = random_problem(HEAD, shape, 400 + si)
    L = _learner(gpu_ctx, HEAD, cfg, params)
    table = np.linspace(-2.0, 2.0, A)
    L.action_values = table

    def run(policy):
        policy.keep_features = policy.keep_q = True
        jerk = policy(1, st["ego4"], st["k"], st["ox"], st["ov"], st["oa"]).cpu().numpy().copy()
        return policy.feat.clone(), policy.q.cpu().numpy().copy(), policy.action.cpu().numpy().copy(), jerk
    path = L.export_q(str(tmp_path / "duel.npz"))
    views = {"online": actor.C51Actor.from_learner(L, n, gpu_ctx, S), "target": actor.C51Actor.from_learner(L, n, gpu_ctx, S, target=True),
             "file": actor.C51Actor(path, n, gpu_ctx, S)}
    assert all(v.dueling is True and v.shape == (n_obs, h1, A) for v in views.values())
    feat = None
    L_target = learner.C51Learner((n_obs, A), cfg, seed=1, init=params["q_target"], ctx=gpu_ctx)      # (a learner acts with its online net)
    for name, pol in views.items():
        f, qv, act, jerk = run(pol)
        feat = f if feat is None else feat
        assert torch.equal(f, feat)
        dbg = torch.zeros(n, A, dtype=torch.float32, device="cuda")
        want = (L_target if name == "target" else L).act(f, None, eps=0.0, debug_q=dbg).cpu().numpy()
        assert np.array_equal(qv.view(np.uint32), dbg.cpu().numpy().view(np.uint32)) and np.array_equal(act, want), name
        assert np.array_equal(jerk, table[act]), name
    # the folded plain network, rounded to float32, as a plain C51 actor
    folded = learner.c51_fold_dueling_host(params["q"], A, K)
    fpath = str(tmp_path / "folded.npz")
    np.savez(fpath, **{k: folded[k].astype(np.float32) for k in NAMES}, action_values=table, n_atoms=np.int64(K), v_min=np.float64(cfg.v_min), v_max=np.float64(cfg.v_max))
    plain = actor.C51Actor(fpath, n, gpu_ctx, S)
    assert plain.dueling is False
    _, qp, ap, _ = run(plain)
    _, qd, ad, _ = run(views["online"])
    ev = _expected_values_host(params["q"], feat.cpu().numpy(), cfg)
    top = np.sort(ev["float64"], axis=1)
    bound = max(bound_4x(rel_err(ev["float32"], ev["float64"])), bound_4x(rel_err(qp, ev["float64"]))) * np.abs(ev["float64"]).max()
    keep = top[:, -1] - top[:, -2] > bound
    assert keep.mean() >= 0.9 and np.array_equal(ap[keep], ad[keep]) and np.array_equal(ad[keep], ev["float64"].argmax(1)[keep])
    gpu_ctx.check_error()


# ---- 5: one case each ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_prioritised_replay(gpu_ctx, restore_settings):
    """The priorities are per_priority_host of the device's own row losses; the importance weights reach the gradient."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    per = learner.PERConfig(beta=0.5, max_priority=16.0)
    shape = SHAPES[2]
    cfg, params, replay = random_problem(HEAD, shape, 371, per=per)
    L = _learner(gpu_ctx, HEAD, cfg, params, replay)
    host = learner.SumTreeHost(RING, per)
    host.push(RING)
    assert np.array_equal(L.priorities(), host.nodes)
    for u in range(2):
        idx = learner.per_sample_host(L.priorities(), LEARNER_SEED, u, cfg.batch, RING)
        rows = rows_of(replay, cfg.n_obs)[idx]
        assert np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32))
        before = L.state_dict()["params"]
        g = L.grads()
        w = L.last_sample()["weight"]
        i64, i32 = _twins(HEAD, before, learner.dqn_batch_from_rows(rows, cfg.n_obs), cfg, weights=w)
        assert all(_check_4x("c51 dueling per u%d grad %s" % (u, k), g[k], i32["grad"][k], i64["grad"][k]) for k in NAMES)
        L.update(1)
        ls = L.last_sample()
        assert np.array_equal(ls["idx"], idx) and _check_4x("c51 dueling per u%d row loss" % u, ls["td"], i32["row_loss"], i64["row_loss"]) and (ls["td"] > 0).all()
        pri = learner.per_priority_host(ls["td"], per)
        for r in range(cfg.batch):
            host.set(idx[r], pri[r])
        assert np.array_equal(L.priorities(), host.nodes), u
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_three_step_returns(gpu_ctx, restore_settings):
    """n_step = 3 on pushes of 8 rows with terminated and truncated rows: the twins are fed nstep_batch_host's window of the device's own ring."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    shape = SHAPES[2]
    n_obs, h1, A, K, B = shape
    N = 8
    cfg, params, replay = random_problem(HEAD, shape, 380, n_step=3, gamma=0.9)
    replay["trunc"] = (np.random.default_rng(5).random(RING) < 0.15) & ~replay["term"]
    L = _learner(gpu_ctx, HEAD, cfg, params, rows_per_push=N)
    _fill(L, replay, slice(0, 96), chunk=N)
    cn = L.state_dict()["counters"]
    ring = gpu_ctx.c51_replay_read(L.handle, 0, RING)
    idx = learner.sample_indices_host(LEARNER_SEED, 0, B, 96)
    b = learner.nstep_batch_host(ring, idx, cn[0], cn[1], N, 3, cfg.gamma, n_obs, dqn=True)
    assert len(set(b["m"].tolist())) >= 2 and np.array_equal(L.minibatch().view(np.uint32), b["rows"].view(np.uint32))
    i64, i32 = _twins(HEAD, params, b, cfg, disc=b["disc"])
    d, t = L.dist()
    g = L.grads()
    tag = "c51 dueling n=3 "
    ok = _check_4x(tag + "m", d[:, 0], i32["dist"][:, 0], i64["dist"][:, 0]) and _check_4x(tag + "p(s, a)", d[:, 1], i32["dist"][:, 1], i64["dist"][:, 1])
    ok &= _check_4x(tag + "row loss", t[:, 2], i32["row_loss"], i64["row_loss"])
    for k in NAMES:
        ok &= _check_4x(tag + "grad " + k, g[k], i32["grad"][k], i64["grad"][k])
    assert ok
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_updates_are_reproducible_and_state_round_trips(gpu_ctx, restore_settings):
    _capi()
    cfg, params, replay = random_problem(HEAD, SHAPES[3], 390, target_period=4)
    A_, B_ = _learner(gpu_ctx, HEAD, cfg, params, replay), _learner(gpu_ctx, HEAD, cfg, params, replay)
    A_.update(10)
    B_.update(4)
    mid = B_.state_dict()
    B_.update(6)
    sa, sb = A_.state_dict(), B_.state_dict()
    assert bits_equal(sa["params"], sb["params"], Q_SLOTS, NAMES) and np.array_equal(sa["counters"], sb["counters"]) and np.array_equal(sa["params"]["beta_pow"], sb["params"]["beta_pow"])
    assert A_.stats() == B_.stats() and sa["params"]["updates"] == 10 and not bits_equal(sa["params"], params, ("q",), NAMES)
    C_ = _learner(gpu_ctx, HEAD, cfg, params, replay)
    C_.load_state_dict(mid)
    back = C_.state_dict()
    assert bits_equal(back["params"], mid["params"], Q_SLOTS, NAMES) and np.array_equal(back["counters"], mid["counters"]) and back["dueling"] is True
    C_.update(6)
    sc = C_.state_dict()
    assert bits_equal(sa["params"], sc["params"], Q_SLOTS, NAMES) and np.array_equal(sa["counters"], sc["counters"]) and C_.stats() == A_.stats()
    gpu_ctx.check_error()


# ---- 6: population --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_population_members_equal_lone_learners(gpu_ctx, restore_settings):
    """P = 3 dueling members with different supports and seeds: each is bit-identical to the lone learner on its slice after three updates.  A
    population that mixes dueling and plain members is refused, by the class and by the library."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    shape = SHAPES[1]
    n_obs, h1, A, K, B = shape
    P, n_per = 3, 16
    sups = [(-10.0, 10.0), (-4.0, 4.0), (-2.0, 6.0)]
    probs = [random_problem(HEAD, shape, 500 + m, v_min=sups[m][0], v_max=sups[m][1], double=bool(m % 2)) for m in range(P)]
    env = _stub_env(gpu_ctx, P * n_per, n_obs, A)
    seeds = [11, 12, 13]
    pop = learner.C51Population(env, [p[0] for p in probs], seeds=seeds, init=[p[1]["q"] for p in probs])
    lone = [learner.C51Learner((n_obs, A), probs[m][0], seed=seeds[m], init=probs[m][1]["q"], ctx=gpu_ctx) for m in range(P)]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    for step in range(4):
        sl = slice(step * n_per, (step + 1) * n_per)
        cat = lambda key, dt: dev(np.concatenate([probs[m][2][key][sl] for m in range(P)]).astype(dt))
        s, s2, a, r, term = cat("s", np.float32), cat("s2", np.float32), cat("a", np.int32), cat("r", np.float64), cat("term", bool)
        trunc = torch.zeros_like(term)
        pop.push(s, None, a, r, s2, term, trunc)
        for m in range(P):
            ms = slice(m * n_per, (m + 1) * n_per)
            lone[m].push(s[ms], None, a[ms], r[ms], s2[ms], term[ms], trunc[ms])
    pop.update(3)
    for m in range(P):
        lone[m].update(3)
        a_, b_ = pop.member(m).state_dict(), lone[m].state_dict()
        assert bits_equal(a_["params"], b_["params"], Q_SLOTS, NAMES) and np.array_equal(a_["counters"], b_["counters"]), m
        assert a_["params"]["updates"] == 3 and a_["dueling"] is True and not bits_equal(a_["params"], probs[m][1], ("q",), NAMES)
    obs = dev(np.concatenate([probs[m][2]["s"][:n_per] for m in range(P)]).astype(np.float32))
    qa, qb = torch.zeros(P * n_per, A, device="cuda"), torch.zeros(P * n_per, A, device="cuda")
    act = pop.act(obs, None, eps=0.0, debug_q=qa).cpu().numpy().copy()
    for m in range(P):
        ms = slice(m * n_per, (m + 1) * n_per)
        assert np.array_equal(lone[m].act(obs[ms], None, eps=0.0, debug_q=qb[ms]).cpu().numpy(), act[ms])
    assert torch.equal(qa.view(torch.int32), qb.view(torch.int32))
    with pytest.raises(ValueError, match="member 1 has dueling = False"):
        learner.C51Population(env, [probs[0][0], random_problem(HEAD, shape, 1, dueling=False)[0], probs[2][0]])
    cfgs = (capi.C51Cfg * 2)(probs[0][0].to_c(0), random_problem(HEAD, shape, 1, dueling=False)[0].to_c(0))
    h = C.c_void_p()
    assert capi.load().stmpc_pop_c51_create(gpu_ctx._h, cfgs, 2, C.byref(h)) == capi.STMPC_EINVAL and not h.value
    assert "member 1 differs from member 0" in capi.load().stmpc_last_error().decode()
    gpu_ctx.check_error()


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_library_refusals(gpu_ctx):
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    lib = capi.load()
    last = lambda: lib.stmpc_last_error().decode()
    c = learner.C51Config(n_obs=20, n_actions=5, h1=16, batch=7, capacity=64, n_atoms=17).to_c(0)
    c.dueling = 2
    with pytest.raises(RuntimeError, match="dueling must be 0 or 1"):
        gpu_ctx.c51_create(c)
    c = learner.C51Config(n_obs=20, n_actions=20, h1=16, batch=7, capacity=64, n_atoms=51).to_c(0)      # 1020 logits: the plain head fits
    c.dueling = 1
    with pytest.raises(RuntimeError, match=r"\(n_actions \+ 1\) \* n_atoms = 1071 .*exceeds 1024"):
        gpu_ctx.c51_create(c)
    c.n_atoms = 48
    gpu_ctx.c51_destroy(gpu_ctx.c51_create(c))                      # 21 * 48 = 1008
    # the same widths in the actor's entry
    net = lambda A, K: {"w0": np.zeros((16, 20), np.float32), "b0": np.zeros(16, np.float32), "w1": np.zeros(((A + 1) * K, 16), np.float32),
                        "b1": np.zeros((A + 1) * K, np.float32)}
    with pytest.raises(RuntimeError, match=r"\(n_actions \+ 1\) \* n_atoms = 1071 .*exceeds 1024"):
        gpu_ctx.c51actor_create(net(20, 51), np.arange(20.0), 51, -10.0, 10.0, dueling=True)
    gpu_ctx.qactor_destroy(gpu_ctx.c51actor_create(net(20, 48), np.arange(20.0), 48, -10.0, 10.0, dueling=True))
    gpu_ctx.qactor_destroy(gpu_ctx.c51actor_create(net(19, 51), np.arange(19.0), 51, -10.0, 10.0, dueling=True))
    with pytest.raises(ValueError, match=r"\(A \+ 1\) \* n_atoms"):
        gpu_ctx.c51actor_create(net(5, 17), np.arange(6.0), 17, -10.0, 10.0, dueling=True)
    # load_state_dict across the flag, both ways
    shape = SHAPES[1]
    cfg_d, params_d, _ = random_problem(HEAD, shape, 3)
    cfg_p = learner.C51Config(n_obs=shape[0], n_actions=shape[2], h1=shape[1], batch=shape[4], capacity=RING, n_atoms=shape[3])
    Ld, Lp = _learner(gpu_ctx, HEAD, cfg_d, params_d), learner.C51Learner((shape[0], shape[2]), cfg_p, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="the state is a dueling C51 learner's, this learner has a plain head"):
        Lp.load_state_dict(Ld.state_dict())
    with pytest.raises(ValueError, match="the state is a plain C51 learner's, this learner has a dueling head"):
        Ld.load_state_dict(Lp.state_dict())
    assert last() is not None
    gpu_ctx.check_error()


# ---- 8: the training loop -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_train_dqn_takes_a_dueling_learner(gpu_ctx, restore_settings, tmp_path):
    """train_dqn on sumo-jerk-v0 with a dueling learner for 640 frames: the loss is finite, export_q works, and an episode runs."""
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(64, env_id="sumo-jerk-v0", seed=2, ctx=gpu_ctx)
    cfg = learner.C51Config(n_obs=env.obs_dim, h1=32, batch=50, capacity=256, replay_start=100, target_period=5, n_atoms=51, dueling=True)
    L = learner.C51Learner(env, cfg, seed=6)
    first = L.state_dict()["params"]
    res = learner.train_dqn(env, L, 640, updates_per_step=2, drain_every=4, eps_schedule=lambda i, n: 0.5)
    env.check_error()
    st, sd = L.stats(), L.state_dict()
    assert res["steps"] == 10 and res["frames"] == 640 and st["updates"] == 18 and st["fill"] == 256 and np.isfinite(st["loss"]) and st["loss"] > 0
    assert all(np.isfinite(sd["params"][s][k]).all() for s in Q_SLOTS for k in NAMES)
    assert not np.array_equal(sd["params"]["q"]["w1"], first["q"]["w1"]) and sd["params"]["q"]["w1"].shape == (6 * 51, 32)
    path = L.export_q(str(tmp_path / "duel.npz"))
    with np.load(path) as z:
        assert all(np.array_equal(z[k], sd["params"]["q"][k]) for k in NAMES) and int(z["dueling"]) == 1 and int(z["n_atoms"]) == 51
    out = learner.evaluate_dqn(L, 8, seed=3, kmax=16, max_episode_length=2.0)
    assert out["ticks"].shape == (8,) and (out["status"] != 0).all()
    gpu_ctx.check_error()
