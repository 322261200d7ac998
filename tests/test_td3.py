"""The TD3 learner on the GPU (learner.TD3Learner, csrc/stmpc_td3_kernels.hpp, stmpc_td3_*).  Problems: learner_testlib.py, asserted by test_td3_cpu.py.

Ring capacity 256, filled by ``push`` of synthetic rows; shapes "padded" (20-40-24) and "mixed-k" (30-96-48) of learner_testlib.SHAPES, and the
shipped 21-400-300 where a test says so.  Bit for bit wherever the arithmetic allows it (degenerate TD3 = DDPG, the dyadic twin target, the delay
schedule, reproducibility, state round trips); elsewhere the 4 x rule (learner_testlib.py) against ``update_host_td3`` fed the device's own
smoothing noise, and test_gpu_acting's ulp rule for the noise itself.
"""
import numpy as np
import pytest

from learner_testlib import (DYADIC_CASES, GRADIENT_CASES, RING, SEED, SHIPPED, bits_equal as _bits_equal, check_4x as _check_4x, clipped_seed, conditioned_problem,
                             ddpg_view, degenerate, dev as _dev, minibatch_host, push as _push, random_td3_problem, td3_dyadic_problem)
from stmpc_testlib import (ACTOR_N_PER as N_PER, actor_eval as _eval, actor_settings as _settings, actor_states as _states, assert_steps_equal as _assert_steps_equal,
                           capi as _capi)


def _all_slots():
    capi = _capi()
    return capi.DDPG_SLOTS + capi.TD3_SLOTS


def _td3(gpu_ctx, cfg, params, replay, seed=SEED, rows=slice(None)):
    from rl_mpc_lanemerging_amd import learner
    L = learner.TD3Learner(cfg.n_obs, cfg, seed=seed, init=(params["actor"], params["critic"], params["critic2"]), ctx=gpu_ctx)
    L.load_state_dict({"params": params, "counters": None})
    _push(L, replay, rows)
    return L


def _device_batch(gpu_ctx, L, seed, update):
    """The minibatch of ``update`` from the ring as it lies on the device (so the twins see the device's float32 rows)."""
    from rl_mpc_lanemerging_amd import learner
    fill = L.stats()["fill"]
    ring = gpu_ctx.ddpg_replay_read(L.handle, 0, fill)
    return learner.batch_from_rows(ring[learner.sample_indices_host(seed, update, L.cfg.batch, fill)], L.cfg.n_obs)


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,B", [pytest.param("padded", 48, id="padded-B48"), pytest.param(SHIPPED, 100, id="400x300-B100")])
def test_gpu_degenerate_td3_equals_ddpg_bit_for_bit(shape, B, gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = random_td3_problem(shape, B, seed=11)
    cfg, p3 = degenerate(cfg, params)
    T = _td3(gpu_ctx, cfg, p3, replay)
    D = learner.DDPGLearner(cfg.n_obs, cfg, seed=SEED, init={"actor": params["actor"], "critic": params["critic"]}, ctx=gpu_ctx)
    D.load_state_dict({"params": ddpg_view(params), "counters": None})
    _push(D, replay)
    assert np.array_equal(T.minibatch(), D.minibatch())
    start = D.state_dict()["params"]
    for u in range(6):
        T.update(1)
        D.update(1)
        st, sd = T.state_dict(), D.state_dict()
        assert _bits_equal(st["params"], sd["params"], _capi().DDPG_SLOTS), u
        for slot in ("critic", "critic_target", "critic_m", "critic_v"):
            assert _bits_equal({slot: st["params"][slot.replace("critic", "critic2")]}, sd["params"], (slot,)), (u, slot)
        assert np.array_equal(st["params"]["beta_pow"][:4], sd["params"]["beta_pow"]) and np.array_equal(st["params"]["beta_pow"][4:], sd["params"]["beta_pow"][2:])
        assert np.array_equal(st["counters"], sd["counters"]) and st["counters"][2] == u + 1
        s3 = T.stats_td3()
        assert T.stats() == D.stats() and (s3["critic_loss"], s3["mean_q"]) == (s3["critic2_loss"], s3["mean_q2"]) == (D.stats()["critic_loss"], D.stats()["mean_q"])
    assert not _bits_equal(sd["params"], start, ("actor", "critic", "actor_target", "critic_target"))
    gpu_ctx.check_error()


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,gamma", [pytest.param(s, B, g, id="%s-B%d-gamma%g" % (s, B, g)) for s, B, g in DYADIC_CASES])
def test_gpu_dyadic_twin_target_is_exact(shape, B, gamma, gpu_ctx, restore_settings):
    """targets' a', Qt1, Qt2, y and both critics' six gradient tensors equal update_host_td3(float64) value for value: test_td3_cpu.py bounds every
    partial sum below 2^24 units and shows that min takes either critic and mask both values on these very minibatches."""
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = td3_dyadic_problem(shape, B, gamma)
    L = _td3(gpu_ctx, cfg, params, replay)
    rows, batch = minibatch_host(replay, cfg)
    assert L.stats()["fill"] == RING and np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32))
    _, i64 = learner.update_host_td3(params, batch, cfg, "float64", grads_only=True)
    t = L.targets()
    assert t.dtype == np.float32 and t.shape == (B, 5) and np.array_equal(t[:, 0], np.zeros(B, np.float32))
    assert np.array_equal(t[:, 1:].astype(np.float64), i64["targets"]), np.count_nonzero(t[:, 1:].astype(np.float64) != i64["targets"], axis=0)
    ga, g1, g2 = L.grads()
    for name, g in (("grad_critic", g1), ("grad_critic2", g2)):
        for k in learner.TENSORS:
            want = i64[name][k]
            assert g[k].dtype == np.float32 and g[k].shape == want.shape and np.abs(want).max() > 0
            assert np.array_equal(g[k].astype(np.float64), want), (name, k, int(np.count_nonzero(g[k].astype(np.float64) != want)), want.size)
    after = L.state_dict()["params"]
    assert _bits_equal(after, params, _all_slots()) and after["updates"] == 0          # grads() and targets() apply nothing
    gpu_ctx.check_error()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_smoothing_noise(gpu_ctx, restore_settings):
    """eps against the host twin under test_gpu_acting's rule for the Gaussian (logf, sqrtf, cosf 1 ulp each -- ROCm's HIP math API documentation,
    single-precision table -- plus half an ulp for the final float32 product).  sigma = 0.2 * tanh_scale = 1 exactly, so an unclipped eps IS the
    float32 Gaussian and the rule applies as it stands; the clip is 1-Lipschitz, so it holds for the clipped rows too."""
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = random_td3_problem("padded", 100, seed=12, target_noise=0.2, noise_clip=0.5)
    assert (cfg.target_noise_std, cfg.noise_clip_abs) == (1.0, 2.5)
    seed = clipped_seed(cfg)
    L = _td3(gpu_ctx, cfg, params, replay, seed=seed)
    U_LOG, U_SQRT, U_COS = 1.0, 1.0, 1.0
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    for update in (0, 1):
        t = L.targets()
        eps, a2 = t[:, 0], t[:, 1]
        u1, u2, g64 = learner.smoothing_noise_host(seed, update, cfg.batch)
        logv = np.log((u1.astype(np.float64) + 1) * 2.0 ** -24)
        r = np.sqrt(-2 * logv)
        c = np.cos((np.float32(learner.TWO_PI_F32) * (u2.astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float64))
        rel_log = np.where(logv != 0, U_LOG * ulp(logv) / np.where(logv != 0, np.abs(logv), 1), 0)
        tol = np.abs(c) * (U_SQRT * ulp(r) + 0.5 * r * rel_log) + r * U_COS * ulp(c) + 0.5 * ulp(g64)
        err = np.abs(eps.astype(np.float64) - np.clip(g64, -2.5, 2.5))
        print("update %d: smoothing noise, worst error / bound %.3f; %d rows at the clip" % (update, float((err / np.maximum(tol, 1e-300)).max()),
                                                                                           int(np.count_nonzero(np.abs(eps) == 2.5))))
        assert (err <= tol).all()
        assert np.abs(eps).max() <= np.float32(2.5) and a2.min() >= np.float32(-5) and a2.max() <= np.float32(5)
        if update == 0:
            assert np.count_nonzero(np.abs(eps) == np.float32(2.5)) >= 1 and np.count_nonzero(np.abs(g64) > 2.5) >= 2      # the twin shows clipped rows
        assert np.unique(eps).size > cfg.batch // 2
        L.update(1)
    gpu_ctx.check_error()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,B", [pytest.param(s, B, id="%s-B%d" % ("400x300" if s == SHIPPED else s, B)) for s, B in GRADIENT_CASES])
def test_gpu_gradients_against_the_float64_twin(shape, B, gpu_ctx, restore_settings):
    """Both critics and the actor, the twins fed the device's own eps; error against update_host_td3(float64) at most max(4 x the float32 twin's, 8 ulp)."""
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = conditioned_problem(shape, B, 13)           # (a draw whose TD errors do not cancel: learner_testlib.td_error_cancellation)
    L = _td3(gpu_ctx, cfg, params, replay)
    batch = _device_batch(gpu_ctx, L, SEED, 0)
    eps = L.targets()[:, 0]
    assert np.abs(eps).max() > 0
    grads = dict(zip(("grad_actor", "grad_critic", "grad_critic2"), L.grads()))
    _, i64 = learner.update_host_td3(params, batch, cfg, "float64", eps=eps, grads_only=True)
    _, i32 = learner.update_host_td3(params, batch, cfg, "float32", eps=eps, grads_only=True)
    ratios, ok = {}, True
    for name, g in grads.items():
        for k in learner.TENSORS:
            assert np.abs(i64[name][k]).max() > 0, (name, k)
            ok &= _check_4x("B%d %s.%s" % (B, name, k), g[k], i32[name][k], i64[name][k], ratios)
    assert ok, ratios
    assert _bits_equal(L.state_dict()["params"], params, _all_slots())
    gpu_ctx.check_error()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_delay_schedule_and_gate(gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = random_td3_problem("padded", 48, seed=14, policy_delay=3)
    L = _td3(gpu_ctx, cfg, params, replay)
    delayed = ("actor", "actor_m", "actor_v", "actor_target", "critic_target", "critic2_target")
    stepped = ("critic", "critic_m", "critic_v", "critic2", "critic2_m", "critic2_v")
    p64, p32, prev = params, params, L.state_dict()["params"]
    for u in range(7):
        batch = _device_batch(gpu_ctx, L, SEED, u)
        eps = L.targets()[:, 0]
        L.update(1)
        new = L.state_dict()["params"]
        due = u + 1 in (3, 6)
        for slot in delayed:
            assert _bits_equal(new, prev, (slot,)) != due, (u, slot)
        assert np.array_equal(new["beta_pow"][:2], prev["beta_pow"][:2]) != due
        assert all(not _bits_equal(new, prev, (slot,)) for slot in stepped) and new["updates"] == u + 1
        p64, _ = learner.update_host_td3(p64, batch, cfg, "float64", eps=eps)
        p32, _ = learner.update_host_td3(p32, batch, cfg, "float32", eps=eps)
        assert np.array_equal(new["beta_pow"], p64["beta_pow"])
        prev = new
    ratios, ok = {}, True
    for slot in ("actor", "actor_target", "critic", "critic_target", "critic2", "critic2_target"):
        for k in learner.TENSORS:
            ok &= _check_4x("7 updates %s.%s" % (slot, k), prev[slot][k], p32[slot][k], p64[slot][k], ratios)
    assert ok, ratios
    # the gate: with frames <= replay_start an update changes no byte and no counter
    gcfg, gparams, greplay = random_td3_problem("padded", 48, seed=15, replay_start=RING - 1)
    G = _td3(gpu_ctx, gcfg, gparams, greplay, rows=slice(0, RING - 1))
    before = G.state_dict()
    assert before["counters"][4] == RING - 1
    G.update(3)
    after = G.state_dict()
    assert np.array_equal(after["counters"], before["counters"]) and np.array_equal(after["params"]["beta_pow"], before["params"]["beta_pow"])
    assert _bits_equal(after["params"], before["params"], _all_slots())
    _push(G, greplay, slice(RING - 1, RING))                       # one frame more: the gate opens
    G.update(3)
    assert G.stats()["updates"] == 3 and not _bits_equal(G.state_dict()["params"], before["params"], ("critic", "critic2", "actor"))
    gpu_ctx.check_error()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_updates_are_reproducible(gpu_ctx, restore_settings):
    cfg, params, replay = random_td3_problem("mixed-k", 100, seed=16)
    out = []
    for _ in range(2):
        L = _td3(gpu_ctx, cfg, params, replay)
        L.update(10)
        out.append((L.state_dict(), L.stats_td3(), L.targets()))
    (sd0, s0, t0), (sd1, s1, t1) = out
    assert _bits_equal(sd0["params"], sd1["params"], _all_slots()) and np.array_equal(sd0["params"]["beta_pow"], sd1["params"]["beta_pow"])
    assert np.array_equal(sd0["counters"], sd1["counters"]) and s0 == s1 and s0["updates"] == 10 and np.array_equal(t0.view(np.uint32), t1.view(np.uint32))
    assert np.isfinite(s0["critic_loss"]) and np.isfinite(s0["critic2_loss"]) and s0["critic_loss"] != s0["critic2_loss"]
    assert not _bits_equal(sd0["params"], params, ("actor", "critic", "critic2", "actor_target", "critic_target", "critic2_target"))
    gpu_ctx.check_error()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_handles(gpu_ctx, restore_settings, tmp_path):
    import torch
    capi = _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    cfg, params, replay = random_td3_problem("padded", 48, seed=17)
    L = _td3(gpu_ctx, cfg, params, replay)
    L.update(2)
    # the base refuses an update or gradients of its own, and nothing changes
    before = L.state_dict()
    with pytest.raises(capi.StmpcError):
        gpu_ctx.ddpg_update(L.handle, 1, 1e-3, 1e-3)
    buf = torch.zeros(L._lens["critic"] + L._lens["actor"], dtype=torch.float32, device="cuda")
    with pytest.raises(capi.StmpcError):
        gpu_ctx.ddpg_grads(L.handle, buf.data_ptr(), buf.data_ptr() + 4 * L._lens["actor"])
    after = L.state_dict()
    assert _bits_equal(after["params"], before["params"], _all_slots()) and np.array_equal(after["counters"], before["counters"]) and not buf.any()
    # state_dict -> load_state_dict into a fresh learner: bit for bit, and both continue identically
    M = _td3(gpu_ctx, cfg, params, replay)
    M.load_state_dict(before)
    got = M.state_dict()
    assert _bits_equal(got["params"], before["params"], _all_slots()) and np.array_equal(got["params"]["beta_pow"], before["params"]["beta_pow"])
    assert np.array_equal(got["counters"], before["counters"]) and before["params"]["updates"] == 2
    L.update(3)
    M.update(3)
    a, b = L.state_dict(), M.state_dict()
    assert _bits_equal(a["params"], b["params"], _all_slots()) and np.array_equal(a["params"]["beta_pow"], b["params"]["beta_pow"]) and a["params"]["updates"] == 5
    # a view of the TD3 learner's actor: the exported file without the copy, and the learner's own greedy action on the view's input vectors
    g, S = _settings()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _states(g, dev)
    scfg, sparams, sreplay = random_td3_problem(SHIPPED, 16, seed=18)
    T = _td3(gpu_ctx, scfg, sparams, sreplay)
    T.update(2)
    view = actor.DDPGActor.from_learner(T, N_PER, gpu_ctx, S)
    got = _eval(gpu_ctx, S, view, st)
    _assert_steps_equal(got, _eval(gpu_ctx, S, actor.DDPGActor(T.export_actor(str(tmp_path / "td3.npz")), N_PER, gpu_ctx, S, dev), st), "TD3 view")
    feat, jerk = got[0]["feat"], got[0]["jerk"]
    ticks = np.rint(feat[:, 20] / 0.001).astype(np.int32)
    assert np.array_equal(np.float32(0.001) * ticks.astype(np.float32), feat[:, 20])
    greedy = T.act(_dev(feat[:, :20]), _dev(ticks), noise=False).cpu().numpy()
    assert np.abs(greedy - jerk).max() < 5e-5 and np.abs(jerk).max() > 1e-3       # (test_actor.py's bound between the two float32 evaluations)
    gpu_ctx.check_error()


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shield", [None, "first_step"])
def test_gpu_training_loop(shield, restore_settings):
    """train_ddpg, unedited, drives a TD3Learner: twice from the same seeds, finite and bit-identical; updates start once MORE than replay_start frames
    were pushed (step 3 of 40)."""
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi as capi, learner, vec_env
    n, out = 64, []
    for _ in range(2):
        pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
        ctx = capi.Context(-1)
        kw = dict(shield="first_step") if shield else {}
        env = vec_env.MergeVecEnv(n, env_id="sumo-jerk-continuous-v0", seed=5, ctx=ctx, **kw)
        L = learner.TD3Learner(env, learner.TD3Config(n_obs=env.obs_dim, capacity=4096, replay_start=128), seed=5)
        res = learner.train_ddpg(env, L, frames=40 * n, executed_actions=shield is not None)
        env.check_error()
        st = L.stats_td3()
        assert res["steps"] == 40 and st["updates"] == 38 and st["fill"] == 40 * n and np.isfinite(st["critic_loss"]) and np.isfinite(st["critic2_loss"])
        out.append(L.state_dict())
        del L, env
        ctx.close()
    a, b = out
    assert all(np.isfinite(a["params"][s][k]).all() for s in _all_slots() for k in learner.TENSORS)
    assert _bits_equal(a["params"], b["params"], _all_slots()) and np.array_equal(a["counters"], b["counters"])
    assert np.array_equal(a["params"]["beta_pow"], b["params"]["beta_pow"]) and np.abs(a["params"]["actor"]["w2"]).max() > 0
    assert not np.array_equal(a["params"]["critic"]["w0"], a["params"]["critic2"]["w0"])
