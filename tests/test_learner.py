"""The on-device DDPG learner (learner.py, csrc/stmpc_ddpg_kernels.hpp, stmpc_ddpg_* of include/stmpc.h).

CPU: header / library / binding agree; the generator's Python twins equal the C twins; ``update_host`` equals an independent torch.optim.Adam
restatement; ``export_actor`` round-trips.  GPU: replay ring, gradients, Adam + Polyak, padded rows, ten updates, reproducibility, a critic
regression, acting, the training loop and graph capture -- all through the C-ABI.

The parity rule of the floating-point GPU tests (learner_testlib.check_4x, its one definition): error = max-abs difference to ``update_host`` in float64 divided by the float64 tensor's max-abs;
bound = 4 x the same error of ``update_host`` in float32 on the CPU, floor 8 float32 ulps.  The yardstick is the torch float32 twin, never the kernel;
4 covers two float32 evaluations with different summation orders.  Measured ratios go to profiles/learner/parity.json.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from learner_testlib import bound_4x, capi_slots, check_4x as _check_4x, random_problem as _random_problem, record as _record
from stmpc_testlib import capi as _capi, header_entries, header_struct_fields as _header_struct_fields, header_text


def _critic_fixture():
    with np.load(os.path.join(GOLDEN, "critic_ddpg_medium1.npz")) as z:
        return {k: np.array(z[k]) for k in ("w0", "b0", "w1", "b1", "w2", "b2")}


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_learner():
    capi = _capi()
    lib = capi.load()
    declared = header_entries("stmpc_ddpg_")
    assert declared >= {"stmpc_ddpg_create", "stmpc_ddpg_destroy", "stmpc_ddpg_set_params", "stmpc_ddpg_get_params", "stmpc_ddpg_push_device",
                        "stmpc_ddpg_act_device", "stmpc_ddpg_update_device", "stmpc_ddpg_stats_device", "stmpc_ddpg_grads_device",
                        "stmpc_ddpg_sample_index", "stmpc_ddpg_noise"}
    assert declared == {n for n in capi.EXPORTS if n.startswith("stmpc_ddpg_")}
    for name in declared:
        assert getattr(lib, name) is not None and getattr(lib, name).argtypes is not None, name
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    want = _header_struct_fields("stmpc_ddpg_cfg")
    have = list(capi.DDPGCfg._fields_)
    assert [n for n, _ in want] == [n for n, _ in have]
    assert [ctype_of[t] for _, t in want] == [t for _, t in have]
    flat = header_text(flat=True)
    for name, val in (("STMPC_DDPG_ROW", capi.DDPG_ROW), ("STMPC_DDPG_NCOUNTERS", capi.DDPG_NCOUNTERS), ("STMPC_ABI_VERSION", capi.ABI_VERSION),
                      ("STMPC_DDPG_CRITIC_V", len(capi.DDPG_SLOTS) - 1), ("STMPC_DDPG_CRITIC", capi.DDPG_SLOTS.index("critic"))):
        assert "#define %s %d" % (name, val) in flat, name
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8


def test_generator_twins_equal_the_c_twins():
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    cap = 37
    for seed in (0, 1, 12345, 2 ** 63 + 11, 2 ** 64 - 1):
        for update in (0, 1, 2, 999, 2 ** 40 + 3):
            for fill in (1, 5, cap - 1, cap, 2 ** 20):        # fill 1, fill < C, the wrapped ring (fill = C), a large ring
                idx = learner.sample_indices_host(seed, update, 24, fill)
                assert idx.min() >= 0 and idx.max() < fill
                assert [capi.ddpg_sample_index(seed, update, r, fill) for r in range(24)] == list(idx)
        for call in (0, 1, 77, 2 ** 33):
            u1, u2, g = learner.noise_host(seed, call, 16)
            for e in range(16):
                gc, c1, c2 = capi.ddpg_noise(seed, call, e)
                assert (c1, c2) == (int(u1[e]), int(u2[e])) and c1 < 2 ** 24 and c2 < 2 ** 24
                assert abs(gc - g[e]) <= 4 * np.spacing(abs(g[e])) + 1e-300      # two libms' log / cos in fp64
    idx = learner.sample_indices_host(3, 0, 4096, 64)
    assert len(set(idx)) == 64 and np.bincount(idx).max() < 120                 # uniform over the filled part, with replacement
    assert not np.array_equal(idx, learner.sample_indices_host(4, 0, 4096, 64)) and not np.array_equal(idx, learner.sample_indices_host(3, 1, 4096, 64))
    g = np.concatenate([learner.noise_host(5, c, 512)[2] for c in range(8)])
    assert abs(g.mean()) < 0.06 and abs(g.std() - 1) < 0.05


def test_update_host_equals_an_independent_torch_adam_restatement():
    """Steps 1-4 written again with nn.Sequential modules, torch.optim.Adam and loss.backward(), three updates in a row."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    rng = np.random.default_rng(2)
    cfg, params, batch = _random_problem(rng)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)

    def module(net):
        h1, n_in = net["w0"].shape
        h2 = net["w1"].shape[0]
        m = torch.nn.Sequential(torch.nn.Linear(n_in, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(), torch.nn.Linear(h2, 1)).double()
        with torch.no_grad():
            for lin, (w, b) in zip((m[0], m[2], m[4]), (("w0", "b0"), ("w1", "b1"), ("w2", "b2"))):
                lin.weight.copy_(T(net[w])); lin.bias.copy_(T(net[b]))
        return m
    pi, pi_t, q, q_t = module(params["actor"]), module(params["actor_target"]), module(params["critic"]), module(params["critic_target"])
    opt_q = torch.optim.Adam(q.parameters(), lr=cfg.lr_q, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    opt_pi = torch.optim.Adam(pi.parameters(), lr=cfg.lr_pi, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    s, a, r, s2, mask = (T(batch[k]) for k in ("s", "a", "r", "s2", "mask"))
    squash = lambda z: torch.tanh(z) * cfg.tanh_scale + cfg.tanh_mean
    for it in range(3):
        params, info = learner.update_host(params, batch, cfg, "float64")
        with torch.no_grad():
            y = r + cfg.gamma * mask * q_t(torch.cat([s2, squash(pi_t(s2))], 1))[:, 0]
        loss = torch.nn.functional.mse_loss(q(torch.cat([s, a[:, None]], 1))[:, 0], y)
        opt_q.zero_grad(); loss.backward(); opt_q.step()
        aloss = -q(torch.cat([s, squash(pi(s))], 1)).mean()
        opt_pi.zero_grad(); aloss.backward(); opt_pi.step()
        with torch.no_grad():
            for tgt, src in ((pi_t, pi), (q_t, q)):
                for pt, ps in zip(tgt.parameters(), src.parameters()):
                    pt.mul_(1 - cfg.tau).add_(cfg.tau * ps)
        assert abs(info["critic_loss"] - float(loss)) <= 1e-12 * abs(float(loss))
        for slot, mod in (("actor", pi), ("actor_target", pi_t), ("critic", q), ("critic_target", q_t)):
            for k, p in zip(learner.TENSORS, mod.parameters()):
                np.testing.assert_allclose(params[slot][k], p.detach().numpy(), rtol=1e-11, atol=1e-14, err_msg="%s.%s after update %d" % (slot, k, it + 1))
    assert params["updates"] == 3
    # float32 runs the same code, and the numpy Adam twin agrees with update_host's formula in float32 to rounding
    p32, i32 = learner.update_host(learner.new_params(params["actor"], params["critic"]), batch, cfg, "float32")
    assert p32["actor"]["w0"].dtype == np.float32
    st = learner.new_params(params["actor"], params["critic"])
    w, m, v, wt, bp = learner.adam_host(st["critic"]["w1"], i32["grad_critic"]["w1"], st["critic_m"]["w1"], st["critic_v"]["w1"], st["critic_target"]["w1"],
                                        st["beta_pow"][2:], cfg.lr_q, cfg)
    assert w.dtype == np.float32 and np.abs(w - p32["critic"]["w1"]).max() <= 4e-7 * max(1.0, np.abs(w).max()) and np.array_equal(bp, p32["beta_pow"][2:])


def test_export_actor_round_trips(tmp_path):
    _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    rng = np.random.default_rng(4)
    net = learner.init_net(21, 400, 300, rng)
    net["w2"] = rng.normal(0, 0.05, (1, 300)).astype(np.float32)
    path = str(tmp_path / "actor_trained.npz")
    learner.write_actor(path, learner.unflatten(learner.flatten(net), 21, 400, 300), 5.0, 0.0)
    w = actor.load_weights(path)
    assert all(np.array_equal(w[k], net[k]) and w[k].dtype == np.float32 for k in learner.TENSORS) and (w["tanh_scale"], w["tanh_mean"]) == (5.0, 0.0)
    feat = rng.normal(0, 1, (64, 21)).astype(np.float32)
    assert np.array_equal(actor.forward_host(w, feat), actor.forward_host(dict(net, tanh_scale=5.0, tanh_mean=0.0), feat))
    import rl_mpc_lanemerging_amd as pkg
    assert pkg.Settings.LEARNING_RATE == 2e-4 and learner.DDPGConfig().lr_q == 2e-4 and learner.DDPGConfig().noise_std == 0.5


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _filled_learner(gpu_ctx, B, seed=3, n_env=256, steps=24, capacity=8192, learner_seed=None, **cfg_kw):
    """medium1 actor + the critic fixture + a replay filled from real MergeVecEnv steps (actions: the actor's with exploration noise)."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(n_env, seed=seed, ctx=gpu_ctx)
    cfg = learner.DDPGConfig(n_obs=env.obs_dim, batch=B, capacity=capacity, replay_start=cfg_kw.pop("replay_start", 0), **cfg_kw)
    w = actor.load_weights("medium1")
    L = learner.DDPGLearner(env, cfg, seed=seed if learner_seed is None else learner_seed, init={"actor": {k: w[k] for k in learner.TENSORS}, "critic": _critic_fixture()})
    obs = env.reset()
    for _ in range(steps):
        ticks = env.episode_ticks.clone()
        a = L.act(obs, ticks, noise=True)
        nobs, r, term, trunc, info = env.step(a)
        L.push(obs, ticks, a, r, nobs, term, trunc, final_obs=info["final_observation"])
        obs = nobs
    torch.cuda.synchronize()
    env.check_error()
    return env, L


@pytest.mark.gpu
def test_gpu_replay_ring_equals_a_numpy_ring(gpu_ctx, restore_settings):
    import torch
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    n, cap, n_obs = 96, 500, 20
    cfg = learner.DDPGConfig(n_obs=n_obs, batch=64, capacity=cap, replay_start=0)
    L = learner.DDPGLearner(n_obs, cfg, seed=21, ctx=gpu_ctx)
    rng = np.random.default_rng(0)
    ring = np.zeros((cap, capi.DDPG_ROW), dtype=np.float32)
    cursor = fill = 0
    dev = lambda a: torch.as_tensor(a, device="cuda")
    for step in range(7):                                         # 672 rows into 500: wraps
        obs, nobs, fobs = (rng.normal(0, 1, (n, n_obs)).astype(np.float32) for _ in range(3))
        ticks = rng.integers(0, 500, n).astype(np.int32)
        act, rew = rng.uniform(-5, 5, n), rng.normal(0, 3, n)
        kind = rng.integers(0, 4, n)                              # 0, 1: neither; 2: terminated; 3: truncated
        term, trunc = kind == 2, kind == 3
        assert term.any() and trunc.any() and (kind < 2).any()
        L.push(dev(obs), dev(ticks), dev(act), dev(rew), dev(nobs), dev(term), dev(trunc), final_obs=dev(fobs))
        rows = np.zeros((n, capi.DDPG_ROW), dtype=np.float32)
        rows[:, :n_obs], rows[:, n_obs], rows[:, n_obs + 1] = obs, np.float32(0.001) * ticks.astype(np.float32), act.astype(np.float32)
        rows[:, 32:32 + n_obs] = np.where((term | trunc)[:, None], fobs, nobs)
        rows[:, 32 + n_obs] = np.float32(0.001) * (ticks + 1).astype(np.float32)
        rows[:, 64], rows[:, 65] = rew.astype(np.float32), np.where(term, 0, 1)
        ring[(cursor + np.arange(n)) % cap] = rows
        cursor, fill = (cursor + n) % cap, min(cap, fill + n)
        cn, _ = gpu_ctx.ddpg_get_state(L.handle)
        assert (cn[0], cn[1], cn[4]) == (cursor, fill, n * (step + 1))
        assert np.array_equal(gpu_ctx.ddpg_replay_read(L.handle, 0, cap).view(np.uint32), ring.view(np.uint32)), step
        idx = learner.sample_indices_host(21, 0, cfg.batch, fill)
        assert np.array_equal(L.minibatch().view(np.uint32), ring[idx].view(np.uint32)), step
    assert L.stats()["fill"] == cap


@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 100, 1024])
def test_gpu_gradients_against_the_float64_twin(B, gpu_ctx, restore_settings):
    """stmpc_ddpg_grads_device vs update_host(float64, grads_only) per tensor, bound 4 x update_host(float32)'s error (module text).  B = 100 is also
    the padded-rows test: the twins see exactly the 100 sampled rows, so rows 100-111 of the device's tiles must contribute nothing."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    env, L = _filled_learner(gpu_ctx, B)
    sd = L.state_dict()
    fill = int(sd["counters"][1])
    assert fill == 256 * 24
    rows = gpu_ctx.ddpg_replay_read(L.handle, 0, fill)[learner.sample_indices_host(3, 0, B, fill)]
    assert rows.shape[0] == B and np.array_equal(rows, L.minibatch())
    batch = learner.batch_from_rows(rows, 20)
    ga, gq = L.grads()
    _, i64 = learner.update_host(sd["params"], batch, L.cfg, "float64", grads_only=True)
    _, i32 = learner.update_host(sd["params"], batch, L.cfg, "float32", grads_only=True)
    ratios, ok = {}, True
    for net, g in (("critic", gq), ("actor", ga)):
        for k in learner.TENSORS:
            assert np.abs(i64["grad_" + net][k]).max() > 0, (net, k)
            ok &= _check_4x("B%d grad %s.%s" % (B, net, k), g[k], i32["grad_" + net][k], i64["grad_" + net][k], ratios)
    _record("gradients_B%d" % B, ratios)
    assert ok, ratios
    after = L.state_dict()
    assert all(np.array_equal(after["params"][s][k], sd["params"][s][k]) for s in capi_slots() for k in learner.TENSORS) and after["params"]["updates"] == 0


@pytest.mark.gpu
def test_gpu_adam_and_polyak_equal_the_numpy_twin(gpu_ctx, restore_settings):
    """Known gradients (the debug entry's output for the critic; for the actor the debug entry's too, with critic learning rate 0 so that the critic the
    actor pass sees is the un-stepped one) -> parameters, moments, targets and beta powers after two updates vs adam_host, bound 2 float32 ulps.
    Observed on the MI355X: bit for bit (0 ulps, profiles/learner/parity.json "adam_max_ulps") -- under the build's flags the device's sqrtf and division
    are both correctly rounded, so neither needs the 2-ulp allowance; it stays as the bound the check was specified with."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    env, L = _filled_learner(gpu_ctx, 100)
    worst = 0
    for it in range(2):
        sd = L.state_dict()["params"]
        ga, gq = L.grads()
        L.update(1, lr_q=0.0, lr_pi=3e-4)
        new = L.state_dict()["params"]
        for net, g, lr, o in (("critic", gq, 0.0, 2), ("actor", ga, 3e-4, 0)):
            for k in learner.TENSORS:
                w, m, v, wt, bp = learner.adam_host(sd[net][k], g[k], sd[net + "_m"][k], sd[net + "_v"][k], sd[net + "_target"][k], sd["beta_pow"][o:o + 2], lr, L.cfg)
                for name, have, want in (("w", new[net][k], w), ("m", new[net + "_m"][k], m), ("v", new[net + "_v"][k], v), ("target", new[net + "_target"][k], wt)):
                    ulps = np.abs(have.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                    worst = max(worst, float(ulps.max()))
                    assert ulps.max() <= 2, (it, net, k, name, float(ulps.max()))
            assert np.array_equal(new["beta_pow"][o:o + 2], bp)
        assert new["updates"] == it + 1
    # the critic's step with a non-zero rate: its gradient does not depend on the order, so the same check holds for it
    sd = L.state_dict()["params"]
    _, gq = L.grads()
    L.update(1, lr_q=2e-4, lr_pi=0.0)
    new = L.state_dict()["params"]
    for k in learner.TENSORS:
        w, m, v, wt, _ = learner.adam_host(sd["critic"][k], gq[k], sd["critic_m"][k], sd["critic_v"][k], sd["critic_target"][k], sd["beta_pow"][2:], 2e-4, L.cfg)
        for have, want in ((new["critic"][k], w), (new["critic_m"][k], m), (new["critic_v"][k], v), (new["critic_target"][k], wt)):
            ulps = np.abs(have.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            worst = max(worst, float(ulps.max()))
            assert ulps.max() <= 2, (k, float(ulps.max()))
        assert np.abs(new["critic"][k] - sd["critic"][k]).max() > 0
    print("Adam + Polyak vs adam_host: worst difference %.2f float32 ulps" % worst)
    _record("adam_max_ulps", worst)


def _drive_twin(params, ring, cfg, seed, n, dtype, fill, **kw):
    from rl_mpc_lanemerging_amd import learner
    for u in range(n):
        batch = learner.batch_from_rows(ring[learner.sample_indices_host(seed, params["updates"], cfg.batch, fill)], cfg.n_obs)
        params, info = learner.update_host(params, batch, cfg, dtype, **kw)
    return params


@pytest.mark.gpu
def test_gpu_ten_updates_against_the_float64_twin(gpu_ctx, restore_settings):
    """Ten updates (critic step, then the actor step against the stepped critic, Polyak) on a fixed replay vs the float64 twin driven with the same
    sampled indices; the 4 x rule relative to the float32 twin after its own ten updates, per tensor of the four networks."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    env, L = _filled_learner(gpu_ctx, 100)
    sd = L.state_dict()
    fill = int(sd["counters"][1])
    ring = gpu_ctx.ddpg_replay_read(L.handle, 0, fill)
    L.update(10)
    new = L.state_dict()["params"]
    assert new["updates"] == 10
    p64 = _drive_twin(sd["params"], ring, L.cfg, 3, 10, "float64", fill)
    p32 = _drive_twin(sd["params"], ring, L.cfg, 3, 10, "float32", fill)
    ratios, ok = {}, True
    for slot in ("critic", "critic_target", "actor", "actor_target"):
        for k in learner.TENSORS:
            ok &= _check_4x("10 updates %s.%s" % (slot, k), new[slot][k], p32[slot][k], p64[slot][k], ratios)
    _record("ten_updates_B100", ratios)
    assert ok, ratios


@pytest.mark.gpu
def test_gpu_updates_are_reproducible(gpu_ctx, restore_settings):
    """Same seed, same pushes: bit-identical after 20 updates.  Another seed: other minibatches."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    out = []
    for _ in range(2):
        env, L = _filled_learner(gpu_ctx, 100)
        mb = L.minibatch()
        L.update(20)
        out.append((mb, L.state_dict()["params"], L.stats()))
    (mb0, p0, s0), (mb1, p1, s1) = out
    assert np.array_equal(mb0, mb1) and s0 == s1 and s0["updates"] == 20 and np.isfinite(s0["critic_loss"])
    for slot in capi_slots():
        for k in learner.TENSORS:
            assert np.array_equal(p0[slot][k].view(np.uint32), p1[slot][k].view(np.uint32)), (slot, k)
    assert np.array_equal(p0["beta_pow"], p1["beta_pow"])
    env, L = _filled_learner(gpu_ctx, 100, learner_seed=4)
    assert not np.array_equal(L.minibatch(), mb0)
    assert not np.array_equal(learner.sample_indices_host(3, 0, 100, 6144), learner.sample_indices_host(4, 0, 100, 6144))


@pytest.mark.gpu
def test_gpu_critic_regression(gpu_ctx, restore_settings):
    """gamma = 0, actor learning rate 0, fixed replay, 200 updates: the critic regresses onto the rewards.  Its loss over the WHOLE replay ends below its
    start, and within the 4 x rule of the float64 twin's final loss (error of the loss relative to the float64 loss; yardstick: the float32 twin)."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    env, L = _filled_learner(gpu_ctx, 100, gamma=0.0, lr_pi=0.0)
    sd = L.state_dict()
    fill = int(sd["counters"][1])
    ring = gpu_ctx.ddpg_replay_read(L.handle, 0, fill)
    whole = learner.batch_from_rows(ring, 20)

    def loss(critic):
        t = {k: torch.tensor(np.asarray(critic[k]), dtype=torch.float64) for k in learner.TENSORS}
        x = torch.tensor(np.concatenate([whole["s"], whole["a"][:, None]], 1), dtype=torch.float64)
        return float(((learner._mlp(t, x) - torch.tensor(whole["r"], dtype=torch.float64)) ** 2).mean())
    start = loss(sd["params"]["critic"])
    L.update(200)
    new = L.state_dict()["params"]
    assert new["updates"] == 200 and all(np.array_equal(new["actor"][k], sd["params"]["actor"][k]) for k in learner.TENSORS)
    end = loss(new["critic"])
    l64 = loss(_drive_twin(sd["params"], ring, L.cfg, 3, 200, "float64", fill)["critic"])
    l32 = loss(_drive_twin(sd["params"], ring, L.cfg, 3, 200, "float32", fill)["critic"])
    e_dev, e_32 = abs(end - l64) / l64, abs(l32 - l64) / l64
    print("critic regression: loss %.6g -> %.6g; float64 twin %.6g, float32 twin %.6g; errors device %.3e, float32 twin %.3e" % (start, end, l64, l32, e_dev, e_32))
    _record("critic_regression", {"start": start, "device": end, "float64_twin": l64, "float32_twin": l32, "device_err": e_dev, "float32_twin_err": e_32})
    assert end < start
    assert e_dev <= bound_4x(e_32)


@pytest.mark.gpu
def test_gpu_acting(gpu_ctx, restore_settings):
    """Greedy: the torch engine's network on the same features within test_actor.py's 5e-5.  Noise: the draws equal the host twin bit for bit; the
    Gaussian equals the float64 twin within the propagated ulp bounds of the device functions -- ROCm's HIP math API documentation, single-precision
    table: logf 1 ulp, sqrtf 1 ulp, cosf 1 ulp -- plus half an ulp for the final float32 product; the action is the float32 sum, clipped to the Box."""
    _capi()
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, learner
    env, L = _filled_learner(gpu_ctx, 100, steps=3)
    n = env.n
    obs = env.reset()
    for _ in range(5):
        obs = env.step(L.act(obs, env.episode_ticks.clone(), noise=False))[0]
    ticks = env.episode_ticks.clone()
    greedy = L.act(obs, ticks, noise=False).clone()
    pol = actor.DDPGActor("medium1", n, gpu_ctx, pkg.Settings, engine="torch")
    feat = torch.cat([obs, (np.float32(0.001) * ticks.to(torch.float32)).unsqueeze(1)], 1)
    with torch.no_grad():
        want = pol.forward(feat).cpu().numpy()
    assert np.abs(greedy.cpu().numpy() - want).max() < 5e-5
    calls0 = int(gpu_ctx.ddpg_get_state(L.handle)[0][3])
    assert calls0 == 3                                             # the three noisy acting calls of the fill; greedy calls do not count
    U_LOG, U_SQRT, U_COS = 1.0, 1.0, 1.0
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    for call in (calls0, calls0 + 1):
        dbg = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
        a = L.act(obs, ticks, noise=True, debug=dbg).cpu().numpy()
        d = dbg.cpu().numpy().view(np.uint32)
        u1, u2, g64 = learner.noise_host(3, call, n)
        assert np.array_equal(d[:, 0], u1) and np.array_equal(d[:, 1], u2)
        g_dev, greedy_dev = d[:, 2].copy().view(np.float32), d[:, 3].copy().view(np.float32)
        assert np.array_equal(greedy_dev.astype(np.float64), greedy.cpu().numpy())
        logv = np.log((u1.astype(np.float64) + 1) * 2.0 ** -24)
        r = np.sqrt(-2 * logv)
        c = np.cos((np.float32(learner.TWO_PI_F32) * (u2.astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float64))
        rel_log = np.where(logv != 0, U_LOG * ulp(logv) / np.where(logv != 0, np.abs(logv), 1), 0)
        tol = np.abs(c) * (U_SQRT * ulp(r) + 0.5 * r * rel_log) + r * U_COS * ulp(c) + 0.5 * ulp(g64)
        err = np.abs(g_dev.astype(np.float64) - g64)
        print("call %d: Gaussian term, worst error / bound %.3f" % (call, float((err / np.maximum(tol, 1e-300)).max())))
        assert (err <= tol).all()
        expect = np.clip(greedy_dev + np.float32(L.cfg.noise_std) * g_dev, np.float32(-5), np.float32(5)).astype(np.float64)
        assert np.array_equal(a, expect) and a.min() >= -5 and a.max() <= 5 and np.abs(a - greedy_dev).max() > 0.1
    assert int(gpu_ctx.ddpg_get_state(L.handle)[0][3]) == calls0 + 2


@pytest.mark.gpu
def test_gpu_training_loop(gpu_ctx, restore_settings, tmp_path):
    _capi()
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi as capi, actor, combined, combined_bench, control, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n, cap = 1024, 200000
    env = vec_env.MergeVecEnv(n, env_id="sumo-jerk-continuous-v0", seed=5, ctx=gpu_ctx)
    for ups in (1, 2):
        L = learner.DDPGLearner(env, learner.DDPGConfig(n_obs=env.obs_dim, capacity=cap, replay_start=50 * n), seed=5)
        res = learner.train_ddpg(env, L, frames=300 * n, updates_per_step=ups)        # (a RuntimeError of the env would surface here)
        env.check_error()
        st = L.stats()
        assert res["steps"] == 300 and st["fill"] == min(cap, n * 300) and np.isfinite(st["critic_loss"])
        assert st["updates"] == 250 * ups                           # updates start once MORE than replay_start frames were pushed: steps 51 ... 300
    sd = L.state_dict()["params"]
    assert all(np.isfinite(sd[s][k]).all() for s in capi.DDPG_SLOTS for k in learner.TENSORS)
    assert np.abs(sd["actor"]["w2"]).max() > 0
    print("train_ddpg: %d episodes finished in the second run, mean return %.3f (no claim about learning progress)" % (res["episodes"], res["mean_return"]))
    # the exported actor in the combined controller
    path = L.export_actor(str(tmp_path / "actor_loop.npz"))
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    S = pkg.Settings
    m, K = 130, 8
    ego = np.zeros((m, 5)); ego[:, 0] = np.linspace(-220.0, -150.0, m); ego[:, 1] = 20.0; ego[:, 2] = 10.0
    ego[:, 4] = [control.get_ego_s((x, y)) for x, y in ego[:, :2]]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    d_ego, d_k, d_ox, d_ov = t(ego), t(np.zeros(m, np.int32)), t(np.zeros((m, K))), t(np.zeros((m, K)))
    pol = actor.DDPGActor(path, m, gpu_ctx, S, engine="hip")
    d = combined.decide_batch_device(gpu_ctx, capi.Params.from_settings(S), capi.CombinedCfg.from_settings(S), d_ego, d_k, d_ox, d_ov, pol, None,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gpu_ctx.check_error()
    assert torch.isfinite(d["speed"]).all() and torch.isfinite(d["first_action"]).all() and float(d["first_action"].abs().max()) <= 5.0


@pytest.mark.gpu
def test_gpu_chain_captured_as_one_graph(gpu_ctx, restore_settings):
    """act -> step -> push -> update captured on one stream and replayed 5 times equals the same iterations run eagerly, bit for bit: the counters
    and cursors advance on the device."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    results = []
    for mode in ("eager", "graph"):
        env, L = _filled_learner(gpu_ctx, 100, seed=8, steps=4)
        obs = env.reset()
        bufs = [None, torch.zeros(env.n, dtype=torch.int32, device="cuda")]

        def chain():
            o = env._obs[env._cur]
            ticks = bufs[1]
            ticks.copy_(env.episode_ticks)
            a = L.act(o, ticks, noise=True)
            nobs, r, term, trunc, info = env.step(a)
            L.push(o, ticks, a, r, nobs, term, trunc, final_obs=info["final_observation"])
            L.update(1)
        chain()                                                     # (allocations happen here)
        chain()
        if mode == "eager":
            for _ in range(10):
                chain()
        else:
            # the env flips its double-buffered observation on the host, so one graph holds two chains: 5 replays = 10 iterations
            s_ = torch.cuda.Stream()
            s_.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s_):
                chain()
                chain()
            for _ in range(5):
                g.replay()
        torch.cuda.synchronize()
        env.check_error()
        results.append((L.state_dict(), gpu_ctx.ddpg_replay_read(L.handle, 0, L.cfg.capacity), env._obs[env._cur].cpu().numpy()))
    (sd0, ring0, o0), (sd1, ring1, o1) = results
    assert sd0["params"]["updates"] == 12 and np.array_equal(sd0["counters"], sd1["counters"])
    assert np.array_equal(ring0.view(np.uint32), ring1.view(np.uint32)) and np.array_equal(o0, o1)
    for slot in capi_slots():
        for k in learner.TENSORS:
            assert np.array_equal(sd0["params"][slot][k].view(np.uint32), sd1["params"][slot][k].view(np.uint32)), (slot, k)
