"""The DQN learner on the GPU (``learner.DQNLearner``, csrc/stmpc_dqn_kernels.hpp) against its host twins, at the shapes (n_obs, h1, A, B) =
(20, 16, 5, 7), (20, 48, 20, 33), (20, 256, 5, 50), (12, 32, 17, 16): one and two output tiles, an A that crosses a tile with padding, a B that is
no multiple of 16 and one that is, the reference's own shape.  Rings have at most 256 rows, envs at most 64 environments.

Parity rule for float32 results (tests/learner_testlib.py's): per tensor, max-norm error against ``update_host_dqn("float64")`` at most
max(4 x the error of ``update_host_dqn("float32")``, 8 float32 ulps).

Exactness on dyadic data: the targets, a*, Q(s, a) and the pads are exact at every shape.  A gradient carries the factor 1 / B: for B = 16 the
gradients equal the float64 twin value for value; 1/7, 1/33 and 1/50 are not float32 numbers, so no float32 gradient can equal the float64 one
there, and those shapes' gradients are held to the parity rule above (test_gpu_dyadic_targets_are_exact) -- and each of the four networks has its
gradients checked value for value at a power-of-two B of its own (test_gpu_dyadic_gradients_are_exact: B = 8, 32, 64, 16).

More than 32 actions (discrete_testlib.WIDE_A: (20, 32, 40, 16), (12, 16, 64, 8), (20, 48, 256, 32)): the same two tests, the acting test and the
prioritised-replay body on ``dqn_wide_problem`` -- exact ties across the argmax's strides that hold the row's maximum, stored actions in every
output tile, clip bounds met exactly; test_dqn_cpu.py asserts from the twins alone that none of it is vacuous."""
import os

import numpy as np
import pytest

from conftest import REPO
from discrete_testlib import (DQN as HEAD, GRAD_SHAPES as _GRAD_SHAPES, NAMES, Q_SLOTS, RING, SHAPES as _SHAPES, WIDE_A as _WIDE_A, WIDE_ACT_ROWS, _q64,
                              dqn_dyadic_problem as _dyadic_problem, dqn_wide_problem as _wide_problem, fill as _fill, make_learner as _learner,
                              minibatch_host as _minibatch_host, pad_mask as _pad_mask, pads_are_zero as _pads_are_zero, random_problem as _random_problem, rows_of as _rows,
                              tied_rows as _tied_rows, twins as _twins)
from learner_testlib import bits_equal, check_4x as _check_4x
from stmpc_testlib import capi as _capi

SHAPES, GRAD_SHAPES, WIDE = _SHAPES["dqn"], _GRAD_SHAPES["dqn"], _WIDE_A["dqn"]      # tests/discrete_testlib.py's tables


def dyadic_problem(shape, double, clip, seed=0):
    """(cfg, params, replay, extra): tests/discrete_testlib.py's exact problem for ``shape`` -- ``dqn_wide_problem`` at a shape of WIDE (ties at
    s' that hold the row's maximum, hand-set stored actions, clip bounds that rows meet exactly; ``extra`` names them), else
    ``dqn_dyadic_problem`` (``extra`` None).  ``seed`` is ``dqn_dyadic_problem``'s alone: a WIDE problem's generator seed is the one
    WIDE_DQN_SEEDS holds for (shape, double), found on the CPU, so the targets test and the gradients test run the same WIDE problem (the second
    goes on to the update)."""
    if shape in WIDE:
        return _wide_problem(shape, double, clip)
    return _dyadic_problem(shape, double, clip, seed) + (None,)


def _wide_checks(gpu_ctx, L, cfg, params, replay, extra, batch, i64, t):
    """What only a WIDE problem has: the ring after the push holds A - 1 and 0 where A + 3 and -2 were pushed; the stored actions reach every output
    tile, column 31, column 32 and column A - 1; on every row where a tie group holds the maximum at s', a* is the group's lowest column, group by
    group; with clip_targets, y sits exactly on each bound on the rows the twin names."""
    A, B = cfg.n_actions, cfg.batch
    ring = gpu_ctx.dqn_pop_replay_read(L.handle, 0, cfg.capacity)
    assert np.array_equal(ring.view(np.uint32), _rows(replay, cfg.n_obs, A).view(np.uint32))
    col = _capi().DQN_ACTION_COL
    for r, pushed, stored in extra["hand"]:
        assert replay["a"][r] == pushed and ring[r, col] == stored, (r, pushed, stored, ring[r, col])
    assert (extra["hand"][0][1], extra["hand"][0][2], extra["hand"][1][1], extra["hand"][1][2]) == (A + 3, A - 1, -2, 0)
    stored = set(batch["a"].tolist())
    assert {31, 32, A - 1} <= stored and {a // 16 for a in stored} == set(range((A + 15) // 16)), sorted(stored)
    qn = _q64(params["q" if cfg.double else "q_target"], batch["s2"])
    for name, rows in _tied_rows(qn, extra["groups"]).items():
        low = extra["groups"][name][0]
        print("%s: tie %s on %d rows" % ((cfg.n_obs, cfg.h1, A, B), name, rows.size))
        assert rows.size >= 4 and (i64["targets"][rows, 0] == low).all(), name
        assert (t[rows, 0] == low).all(), ("a* on the rows tied in " + name, t[rows, 0].tolist(), low)
    if cfg.clip_targets:
        live = batch["mask"] > 0
        g = 0.5 * i64["targets"][:, 1]
        for bound, beyond in ((cfg.clip_min, g < cfg.clip_min), (cfg.clip_max, g > cfg.clip_max)):
            on = live & (g == bound)
            assert on.any() and (live & beyond).any()
            assert (t[on | (live & beyond), 2].astype(np.float64) == batch["r"][on | (live & beyond)] + bound).all()


# ---- 1: targets -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("double,clip", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("shape", SHAPES + WIDE)
def test_gpu_dyadic_targets_are_exact(shape, double, clip, gpu_ctx, restore_settings):
    """targets() (a*, Qt(s', a*), y, Q(s, a)) equals update_host_dqn(float64) value for value, on minibatches with rows whose real Q(s') are all
    negative; the gradient tensors: value for value where B is a power of two (B = 16), else -- 1 / B is no float32 number -- under the parity rule."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = shape
    cfg, params, replay, extra = dyadic_problem(shape, double, clip)
    L = _learner(gpu_ctx, HEAD, cfg, params, replay)
    rows, batch = _minibatch_host(replay, cfg)
    assert L.stats()["fill"] == RING and np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32))
    i64, i32 = _twins(HEAD, params, batch, cfg)
    import torch
    with torch.no_grad():
        T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        qn = learner._q_mlp({k: T(params["q" if double else "q_target"][k]) for k in NAMES}, T(batch["s2"])).numpy()
    allneg = (qn < 0).all(1)
    assert allneg.any() and not allneg.all(), int(allneg.sum())     # rows on which a pad column's 0 would beat every real action
    assert shape != WIDE[0] or 4 <= allneg.sum() <= B - 4
    t = L.targets()
    assert t.dtype == np.float32 and t.shape == (B, 4)
    assert np.array_equal(t[:, :3].astype(np.float64), i64["targets"]), np.count_nonzero(t[:, :3].astype(np.float64) != i64["targets"], axis=0)
    assert np.array_equal(t[:, 3].astype(np.float64), i64["q_values"])
    assert t[:, 0].max() < A and (double or (t[allneg, 1] < 0).all())          # (double: the sign seen is the online net's, the value the target's)
    if clip:
        g = 0.5 * i64["targets"][:, 1]
        live = batch["mask"] > 0
        assert (g[live] > cfg.clip_max).any() or (g[live] < cfg.clip_min).any()
    if extra is not None:
        _wide_checks(gpu_ctx, L, cfg, params, replay, extra, batch, i64, t)
        if double:
            assert (_q64(params["q"], batch["s2"]).argmax(1) != _q64(params["q_target"], batch["s2"]).argmax(1)).sum() >= 4
    grad = L.grads()
    ok = True
    for k in NAMES:
        want = i64["grad"][k]
        assert grad[k].dtype == np.float32 and grad[k].shape == want.shape and np.abs(want).max() > 0
        if B & (B - 1) == 0:
            assert np.array_equal(grad[k].astype(np.float64), want), (k, int(np.count_nonzero(grad[k].astype(np.float64) != want)), want.size)
        else:
            ok &= _check_4x("%s grad %s" % (shape, k), grad[k], i32["grad"][k], want)
    assert ok
    after = L.state_dict()["params"]
    assert all(np.array_equal(after[s][k], params[s][k]) for s in ("q", "q_target", "q_m", "q_v") for k in NAMES) and after["updates"] == 0
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("double,clip", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("shape", GRAD_SHAPES + WIDE)
def test_gpu_dyadic_gradients_are_exact(shape, double, clip, gpu_ctx, restore_settings):
    """Every gradient tensor equals update_host_dqn(float64) value for value, at each of the four networks: B is a power of two here (8: half a
    tile of padded rows; 32, 64, 16), so that dz = clamp(diff) / B is exact and every product and partial sum of the backward pass is a float32
    number -- any summation order gives the same bits, and a stray or missing term shows."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = shape
    cfg, params, replay, extra = dyadic_problem(shape, double, clip, seed=2)
    if extra is not None:
        cfg.target_period, cfg.lr = 1, 1e-3
    L = _learner(gpu_ctx, HEAD, cfg, params, replay)
    rows, batch = _minibatch_host(replay, cfg)
    assert np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32))
    _, i64 = learner.update_host_dqn(params, batch, cfg, "float64", grads_only=True)
    assert (np.abs(i64["td"]) > 1).any() and (batch["mask"] == 0).any()
    t = L.targets()
    assert np.array_equal(t[:, :3].astype(np.float64), i64["targets"]) and np.array_equal(t[:, 3].astype(np.float64), i64["q_values"])
    grad = L.grads()
    for k in NAMES:
        want = i64["grad"][k]
        assert grad[k].dtype == np.float32 and grad[k].shape == want.shape and np.abs(want).max() > 0
        assert np.array_equal(grad[k].astype(np.float64), want), (k, int(np.count_nonzero(grad[k].astype(np.float64) != want)), want.size)
    if extra is not None:
        _wide_gradient_checks(gpu_ctx, L, cfg, params, batch, i64)
    gpu_ctx.check_error()


def _wide_gradient_checks(gpu_ctx, L, cfg, params, batch, i64):
    """At a WIDE shape, on top of the exact gradients: dZout is an exact zero outside the stored actions' columns -- read as the padded gradient's
    rows of dW1 = dZout^T H1 and entries of db1 of every column no minibatch row stores, +0.0 by their bits.  (The DQN learner has no read of
    dZout itself, as the C51 learner has.  A stray entry of dZout in a column that ANOTHER row stores is not seen here; it changes that column's
    db1 and row of dW1, which the value-for-value comparison with the float64 twin above holds.)  The pads of the gradient are exact
    zeros after grads() and those of all five padded arrays after one update(1); that update (target_period 1: the hard copy is in it) leaves the
    weights, both moments, the beta powers and the target that ``dqn_adam_host`` gives on the float64 twin's gradient, bit for bit."""
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A = cfg.n_obs, cfg.h1, cfg.n_actions
    pad = _pad_mask(n_obs, h1, A)
    _pads_are_zero(gpu_ctx, HEAD, L, [capi.DQN_GRAD], pad, "grads")
    g = gpu_ctx.dqn_padded_read(L.handle, capi.DQN_GRAD, h1, A)
    unstored = np.setdiff1d(np.arange(g["b1"].size), batch["a"])
    assert unstored.size >= g["b1"].size - cfg.batch and not g["w1"][unstored].view(np.uint32).any() and not g["b1"][unstored].view(np.uint32).any()
    assert all(np.abs(g["w1"][a]).max() > 0 for a in set(batch["a"].tolist()))
    L.update(1)
    _pads_are_zero(gpu_ctx, HEAD, L, range(5), pad, "update")
    after = L.state_dict()["params"]
    for k in NAMES:
        w, m, v, bp = learner.dqn_adam_host(params["q"][k], i64["grad"][k], params["q_m"][k], params["q_v"][k], params["beta_pow"], cfg.lr, cfg)
        for slot, want in (("q", w), ("q_m", m), ("q_v", v), ("q_target", w)):
            assert np.array_equal(after[slot][k].view(np.uint32), want.view(np.uint32)), (slot, k)
        assert not np.array_equal(after["q"][k], params["q"][k])
    assert np.array_equal(after["beta_pow"].view(np.uint32), bp.view(np.uint32)) and after["updates"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_pad_entries_stay_zero(shape, gpu_ctx, restore_settings):
    """The padded arrays themselves (padded_read): the pad rows and columns of the gradient are exact zeros after grads(), and those of the
    gradient, the weights, the target and both of Adam's moments are exact zeros after each of four updates (target_period 2: the hard copy
    included); the entries that are no pads are the slot's, and none of a gradient's is zero by accident of the layout (every real row, column
    and bias is reached)."""
    capi = _capi()
    n_obs, h1, A, B = shape
    cfg, params, replay = _random_problem(HEAD, shape, 61, target_period=2)
    L = _learner(gpu_ctx, HEAD, cfg, params, replay)
    pad = _pad_mask(n_obs, h1, A)
    read = lambda slot: gpu_ctx.dqn_padded_read(L.handle, slot, h1, A)
    g = L.grads()
    _pads_are_zero(gpu_ctx, HEAD, L, [capi.DQN_GRAD], pad, "grads")
    have = read(capi.DQN_GRAD)
    assert all(np.array_equal(have[k][~pad[k]].reshape(g[k].shape), g[k]) for k in NAMES)
    assert (np.abs(g["w0"]).max(0) > 0).all() and np.abs(g["b0"]).max() > 0 and np.abs(g["b1"]).max() > 0
    for u in range(4):
        L.update(1)
        _pads_are_zero(gpu_ctx, HEAD, L, range(5), pad, "update %d" % u)
    sd = L.state_dict()["params"]
    for i, slot in enumerate(capi.DQN_SLOTS):
        arr = read(i)
        assert all(np.array_equal(arr[k][~pad[k]].reshape(sd[slot][k].shape), sd[slot][k]) for k in NAMES), slot
    assert sd["updates"] == 4 and all(np.array_equal(sd["q_target"][k], sd["q"][k]) and np.abs(sd["q_m"][k]).max() > 0 for k in NAMES)
    with pytest.raises(RuntimeError):
        gpu_ctx.dqn_padded_read(L.handle, 5, h1, A)
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_act_reads_only_the_observation_columns(gpu_ctx, restore_settings):
    """Q(obs) and the action do not change when the gap of a strided obs tensor -- where the network's pad inputs would read -- holds 1e30."""
    _capi()
    import torch
    n_obs, h1, A, B = SHAPES[3]
    cfg, params, replay = _random_problem(HEAD, SHAPES[3], 62)
    L = _learner(gpu_ctx, HEAD, cfg, params)
    wide = torch.full((40, 32), 1e30, dtype=torch.float32, device="cuda")
    obs = torch.as_tensor(replay["s"][:40].astype(np.float32), device="cuda")
    wide[:, :n_obs] = obs
    q0, q1 = (torch.zeros(40, A, dtype=torch.float32, device="cuda") for _ in range(2))
    a0 = L.act(obs, None, debug_q=q0).clone()
    a1 = L.act(wide[:, :n_obs], None, debug_q=q1).clone()
    assert torch.equal(q0, q1) and torch.equal(a0, a1) and torch.isfinite(q0).all()
    gpu_ctx.check_error()


# ---- 2: gradients on data of real magnitude --------------------------------------------------------------------------------------------------
def _env_replay(gpu_ctx, A_env_id, n_obs, A, rng, steps=4, n=64):
    """Observations from a stepped MergeVecEnv (random indices); n * steps <= 256 rows."""
    import rl_mpc_lanemerging_amd as pkg
    import torch
    from rl_mpc_lanemerging_amd import vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(n, env_id=A_env_id, seed=4, ctx=gpu_ctx)
    obs = env.reset()
    out = {k: [] for k in ("s", "s2", "r", "term")}
    for i in range(steps):
        a = torch.as_tensor(rng.integers(0, env.action_space["n"], n).astype(np.int32), device="cuda")
        nobs, r, term, trunc, info = env.step(a)
        done = (term | trunc)[:, None]
        out["s"].append(obs.cpu().numpy()[:, :n_obs].copy()); out["s2"].append(torch.where(done, info["final_observation"], nobs).cpu().numpy()[:, :n_obs].copy())
        out["r"].append(r.cpu().numpy().copy()); out["term"].append(term.cpu().numpy().copy())
        obs = nobs
    env.check_error()
    rep = {k: np.concatenate(v) for k, v in out.items()}
    rep["a"] = rng.integers(0, A, rep["r"].size)
    rep["term"] = rep["term"] | (rng.random(rep["r"].size) < 0.15)      # (the few steps end no episode: some rows are made terminal)
    return rep


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_gradients_against_the_float64_twin(shape, gpu_ctx, restore_settings):
    """Normal weights at nn.Linear scale, observations of a stepped sumo-jerk-v0 env: the parity rule, per gradient tensor, and for the targets."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = shape
    rng = np.random.default_rng(7)
    rep = _env_replay(gpu_ctx, "sumo-jerk-v0", n_obs, A, rng)
    cfg = learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=256)
    nrm = lambda fan, *sh: (rng.normal(size=sh) / np.sqrt(fan)).astype(np.float32)
    net = lambda: {"w0": nrm(n_obs, h1, n_obs), "b0": nrm(n_obs, h1), "w1": nrm(h1, A, h1), "b1": nrm(h1, A)}
    params = learner.new_params_dqn(net())
    params["q_target"] = net()
    L = _learner(gpu_ctx, HEAD, cfg, params, rep)
    rows, batch = _minibatch_host(rep, cfg)
    assert np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32))
    i64, i32 = _twins(HEAD, params, batch, cfg)
    t, g = L.targets(), L.grads()
    assert np.array_equal(t[:, 0].astype(np.int64), i64["targets"][:, 0].astype(np.int64))
    ok = _check_4x("%s y" % (shape,), t[:, 2], i32["targets"][:, 2], i64["targets"][:, 2])
    ok &= _check_4x("%s Q(s, a)" % (shape,), t[:, 3], i32["q_values"], i64["q_values"])
    for k in NAMES:
        assert np.abs(i64["grad"][k]).max() > 0
        ok &= _check_4x("%s grad %s" % (shape, k), g[k], i32["grad"][k], i64["grad"][k])
    assert ok
    gpu_ctx.check_error()


# ---- 3: acting ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]] + WIDE)
def test_gpu_acting(shape, gpu_ctx, restore_settings):
    """Behind an env at the two shipped action counts.  At a WIDE shape, without one: the acting net and observations of ``dqn_wide_problem`` -- Q
    equals the float64 forward pass value for value, and on every observation where a tie group holds the maximum the greedy index is the group's
    lowest column, group by group; rows with only negative Q among them."""
    _capi()
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    n_obs, h1, A, B = shape
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n = 50                                                          # four tiles, the last one partly filled
    if shape in WIDE:
        env, extra = None, dyadic_problem(shape, True, False)[3]
        cfg = learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=256)
        L = learner.DQNLearner((n_obs, A), cfg, seed=23, init=extra["acting_net"], ctx=gpu_ctx)
        obs = torch.as_tensor(extra["act_obs"], device="cuda")
        assert obs.shape == (n, n_obs) and n == WIDE_ACT_ROWS
    else:
        env = vec_env.MergeVecEnv(n, env_id="sumo-jerk-v0" if A == 5 else "sumo-accel-v0", seed=9, ctx=gpu_ctx)
        cfg = learner.DQNConfig(n_obs=n_obs, h1=h1, batch=B, capacity=256)
        L = learner.DQNLearner(env, cfg, seed=23)
        obs = env.reset()
    assert cfg.n_actions == A == L.action_values.size
    q = torch.zeros(n, A, dtype=torch.float32, device="cuda")
    greedy = L.act(obs, None, eps=0.0, debug_q=q).cpu().numpy().copy()
    qh = q.cpu().numpy()
    assert greedy.dtype == np.int32 and np.array_equal(greedy, qh.argmax(1))          # numpy's argmax: the first maximum
    net = L.state_dict()["params"]["q"]
    want = np.maximum(obs.cpu().numpy().astype(np.float64) @ net["w0"].astype(np.float64).T + net["b0"], 0) @ net["w1"].astype(np.float64).T + net["b1"]
    assert np.abs(qh - want).max() < 5e-5                            # tests/test_learner.py's acting rule
    if env is None:
        assert np.array_equal(qh.astype(np.float64), want) and np.array_equal(greedy, want.argmax(1))
        allneg = (want < 0).all(1)
        assert allneg.any() and not allneg.all()
        for name, rows in _tied_rows(want, extra["act_groups"]).items():
            print("%s: acting tie %s on %d rows" % (shape, name, rows.size))
            assert rows.size >= 2 and (greedy[rows] == extra["act_groups"][name][0]).all(), ("greedy index on the rows tied in " + name, greedy[rows].tolist())
    assert int(gpu_ctx.dqn_get_state(L.handle)[0][3]) == 0           # a greedy call is no exploring call
    call = 0
    for eps in (0.25, 1.0, 0.25):
        a = L.act(obs, None, eps=eps).cpu().numpy().copy()
        explore, idx = learner.dqn_act_host(23, call, n, eps, A)
        assert np.array_equal(a, np.where(explore, idx, greedy)) and a.min() >= 0 and a.max() < A, (eps, call)
        assert explore.all() if eps == 1.0 else (explore.any() and not explore.all())
        call += 1
        assert int(gpu_ctx.dqn_get_state(L.handle)[0][3]) == call
    assert np.array_equal(L.act(obs, None, eps=0.0).cpu().numpy(), greedy)
    # stepping the env with the returned tensor latches no out-of-range flag
    for _ in range(3 if env is not None else 0):
        obs, r, term, trunc, info = env.step(L.act(obs, None, eps=0.5))
    if env is not None:
        env.check_error()
    # ties: an all-zero last layer yields action 0 everywhere
    p = L.state_dict()
    p["params"]["q"]["w1"][:] = 0
    p["params"]["q"]["b1"][:] = 0
    L.load_state_dict(p)
    assert (L.act(obs, None).cpu().numpy() == 0).all()
    with pytest.raises(RuntimeError):
        L.act(obs, None, eps=1.5)
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_library_refusals(gpu_ctx):
    _capi()
    from rl_mpc_lanemerging_amd import learner
    good = dict(n_obs=20, n_actions=5, h1=16, batch=7, capacity=64)
    for bad in (dict(n_actions=0), dict(n_actions=257), dict(n_obs=32), dict(batch=0), dict(target_period=0), dict(replay_start=64)):
        with pytest.raises(RuntimeError):
            gpu_ctx.dqn_create(learner.DQNConfig(**dict(good, **bad)).to_c(0))
    h = gpu_ctx.dqn_create(learner.DQNConfig(**good).to_c(0))
    gpu_ctx.dqn_destroy(h)


# ---- 4: updates --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]])
def test_gpu_target_schedule_and_gate(shape, gpu_ctx, restore_settings):
    """target_period = 3: over 7 updates the target equals the online weights bit for bit after updates 3 and 6 and is unchanged otherwise; nothing
    moves before replay_start; after each update Adam's state and the weights equal the float32 twin stepped with the device's own gradients."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = _random_problem(HEAD, shape, 31, target_period=3, replay_start=64)
    L = _learner(gpu_ctx, HEAD, cfg, params)
    _fill(L, {k: v[:64] for k, v in replay.items()})                # 64 frames: not MORE than replay_start
    L.update(2)
    sd = L.state_dict()
    assert bits_equal(sd["params"], params, Q_SLOTS, NAMES) and sd["params"]["updates"] == 0 and sd["counters"][1] == 64
    _fill(L, {k: v[64:] for k, v in replay.items()})
    for u in range(7):
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
    st = L.stats()
    assert st["updates"] == 7 and st["fill"] == RING and np.isfinite(st["loss"])
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True])
def test_gpu_updates_are_reproducible(per, gpu_ctx, restore_settings):
    _capi()
    from rl_mpc_lanemerging_amd import learner
    kw = dict(per=learner.PERConfig(beta=0.4)) if per else {}
    cfg, params, replay = _random_problem(HEAD, SHAPES[1], 41, target_period=4, **kw)
    A_, B_ = _learner(gpu_ctx, HEAD, cfg, params, replay), _learner(gpu_ctx, HEAD, cfg, params, replay)
    A_.update(10)
    B_.update(4)
    mid = B_.state_dict()
    B_.update(6)
    sa, sb = A_.state_dict(), B_.state_dict()
    assert bits_equal(sa["params"], sb["params"], Q_SLOTS, NAMES) and np.array_equal(sa["counters"], sb["counters"]) and np.array_equal(sa["params"]["beta_pow"], sb["params"]["beta_pow"])
    assert A_.stats() == B_.stats() and sa["params"]["updates"] == 10
    if not per:                                                     # (a tree is not part of a state_dict: a fresh learner's would be the pushes')
        C_ = _learner(gpu_ctx, HEAD, cfg, params, replay)
        C_.load_state_dict(mid)
        C_.update(6)
        sc = C_.state_dict()
        assert bits_equal(sa["params"], sc["params"], Q_SLOTS, NAMES) and np.array_equal(sa["counters"], sc["counters"]) and C_.stats() == A_.stats()
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_prioritised_replay(gpu_ctx, restore_settings):
    _prioritised_replay(gpu_ctx, SHAPES[1])


@pytest.mark.gpu
def test_gpu_prioritised_replay_beyond_one_stride(gpu_ctx, restore_settings):
    """The same three updates at (20, 32, 40, 16): three output tiles, stored actions of 32 and more."""
    _prioritised_replay(gpu_ctx, WIDE[0])


def _prioritised_replay(gpu_ctx, shape):
    """idx = per_sample_host on the device's tree; after an update the sampled leaves = per_priority_host of the device's own td and the inner sums
    recomputed exactly; new rows enter at max_priority ** alpha; the weights reach the loss; a learner without per keeps its bits."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    per = learner.PERConfig(beta=0.5)
    cfg, params, replay = _random_problem(HEAD, shape, 51, per=per)
    cfg0, _, _ = _random_problem(HEAD, shape, 51)
    L, U = _learner(gpu_ctx, HEAD, cfg, params, replay), _learner(gpu_ctx, HEAD, cfg0, params, replay)
    host = learner.SumTreeHost(RING, per)
    host.push(RING)
    tree = L.priorities()
    leaves = learner.per_leaves(RING)
    assert np.array_equal(tree, host.nodes) and (tree[leaves - 1:leaves - 1 + RING] == per.max_priority ** per.alpha).all()
    for u in range(3):
        tree = L.priorities()
        idx = learner.per_sample_host(tree, 11, u, cfg.batch, RING)
        w = learner.per_weights_host(tree, idx, RING, per.beta)
        rows = _rows(replay, cfg.n_obs)[idx]
        assert np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32))
        before = L.state_dict()["params"]
        g = L.grads()
        ls = L.last_sample()
        ulps = np.abs(ls["weight"].astype(np.float64) - w.astype(np.float64)) / np.spacing(w).astype(np.float64)
        assert np.array_equal(ls["idx"], idx) and ulps.max() <= 4 and ls["weight"].max() == 1.0       # (tests/test_per.py's bound for two fp64 pows)
        w = ls["weight"]
        if u > 0:
            assert len(set(w.tolist())) > 1                         # the weights differ once priorities do
        batch = learner.dqn_batch_from_rows(rows, cfg.n_obs)
        _, i64 = learner.update_host_dqn(before, batch, cfg, "float64", weights=w, grads_only=True)
        _, i32 = learner.update_host_dqn(before, batch, cfg, "float32", weights=w, grads_only=True)
        assert all(_check_4x("per u%d grad %s" % (u, k), g[k], i32["grad"][k], i64["grad"][k]) for k in NAMES)
        L.update(1)
        ls = L.last_sample()
        assert np.array_equal(ls["idx"], idx) and _check_4x("per u%d td" % u, ls["td"], i32["td"], i64["td"])
        pri = learner.per_priority_host(ls["td"], per)
        for r in range(cfg.batch):                                  # of rows with the same index the highest row wins
            host.set(idx[r], pri[r])
        assert np.array_equal(L.priorities(), host.nodes), u
    # a learner without per draws the uniform rows, and differs
    assert np.array_equal(U.minibatch().view(np.uint32), _minibatch_host(replay, cfg0)[0].view(np.uint32))
    U.update(3)
    assert not bits_equal(U.state_dict()["params"], L.state_dict()["params"], Q_SLOTS, NAMES)
    # pushes after updates: the new rows' leaves, the rest untouched
    _fill(L, {k: v[:64] for k, v in replay.items()})
    host.cursor = 0
    host.push(64)
    assert np.array_equal(L.priorities(), host.nodes)
    with pytest.raises(RuntimeError):
        U.priorities()
    gpu_ctx.check_error()


# ---- 5: the training loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("env_id,A", [("sumo-jerk-v0", 5), ("sumo-accel-v0", 20)])
def test_gpu_train_dqn(env_id, A, gpu_ctx, restore_settings, tmp_path):
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)

    def run():
        env = vec_env.MergeVecEnv(64, env_id=env_id, seed=2, ctx=gpu_ctx)
        cfg = learner.DQNConfig(n_obs=env.obs_dim, h1=32, batch=50, capacity=256, replay_start=100, target_period=5, per=learner.PERConfig() if A == 5 else None)
        L = learner.DQNLearner(env, cfg, seed=6)
        first = L.state_dict()["params"]
        res = learner.train_dqn(env, L, 640, updates_per_step=2, drain_every=4, eps_schedule=lambda i, n: 0.5)
        env.check_error()
        return L, first, res

    L, first, res = run()
    st, sd = L.stats(), L.state_dict()
    assert res["steps"] == 10 and res["frames"] == 640 and set(res) == {"steps", "frames", "episodes", "mean_return", "returns", "takeover_share"}
    assert st["updates"] == 2 * 9 and st["fill"] == 256 and np.isfinite(st["loss"])        # updates start once MORE than 100 frames were pushed: steps 2 ... 10
    assert all(np.isfinite(sd["params"][s][k]).all() for s in ("q", "q_target", "q_m", "q_v") for k in NAMES)
    assert not np.array_equal(sd["params"]["q"]["w1"], first["q"]["w1"]) and not np.array_equal(sd["params"]["q"]["b1"], first["q"]["b1"])
    L2, _, res2 = run()
    sd2 = L2.state_dict()
    assert bits_equal(sd["params"], sd2["params"], Q_SLOTS, NAMES) and np.array_equal(sd["counters"], sd2["counters"]) and np.array_equal(res["returns"], res2["returns"])
    path = L.export_q(str(tmp_path / "q.npz"))
    with np.load(path) as z:
        assert all(np.array_equal(z[k], sd["params"]["q"][k]) for k in NAMES) and np.array_equal(z["action_values"], L.action_values) and z["action_values"].size == A
        table = pkg.Settings.JERK_VALUES_DQN if A == 5 else pkg.Settings.ACCELERATION_VALUES_DQN     # the reference's own tables (config.py:114-115)
        assert np.array_equal(z["action_values"], np.array([table[i] for i in range(A)], dtype=np.float64)) and len(table) == A
        assert (z["action_values"][0], z["action_values"][-1]) == ((-5.0, 5.0) if A == 5 else (-6.0, 4.5))
    M = learner.DQNLearner((L.cfg.n_obs, A), learner.DQNConfig(n_obs=L.cfg.n_obs, h1=32, batch=50, capacity=256), init={k: np.load(path)[k] for k in NAMES}, ctx=gpu_ctx)
    assert all(np.array_equal(M.state_dict()["params"]["q"][k], sd["params"]["q"][k]) for k in NAMES)
    gpu_ctx.check_error()


def test_smoke_and_benchmark_read_only_the_repository():
    src = open(os.path.join(REPO, "__graft_entry__.py")).read()
    smoke = src[src.index("def smoke"):]
    assert "reference" not in smoke.replace("REFERENCE_DEFAULT", "")
    bench = open(os.path.join(REPO, "scripts", "dqn_bench.py")).read()
    assert "/root" not in bench and "reference/" not in bench
