"""The TD3 learner (learner.TD3Learner, csrc/stmpc_td3_kernels.hpp, stmpc_td3_* of include/stmpc.h): CPU part, and the problems the GPU part
(test_td3.py) shares.

  * header, library and binding agree on the new entries and on stmpc_td3_cfg;
  * ``smoothing_noise_host`` equals ``stmpc_td3_noise`` and is another stream than the acting noise;
  * degenerate TD3 (no target noise, policy_delay 1, critic 2 = critic 1) is ``update_host`` value for value, float64 and float32, four updates;
  * the delay schedule of ``update_host_td3``;
  * ``td3_dyadic_problem``: ``dyadic_problem`` of test_net_shapes_cpu.py with a second dyadic critic, dyadic target critics, a target actor whose
    last layer is zero (a' = tanh_mean exactly) and gamma in {0.5, 1}: y = r + gamma * mask * min(Qt1, Qt2) and everything downstream of it stays in
    float32 numbers, so the GPU test compares with np.array_equal.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_net_shapes_cpu import SEED, SHAPES, _capi, _dyadic_net, _frac_bits, dyadic_problem, exactness_bits, forward_host, replay_rows_host

RING = 256                      # the GPU tests' ring capacity; the first RING rows of a problem's replay are pushed
# (shape, B, gamma) of the exact cases, CPU and GPU
DYADIC_CASES = [("padded", 16, 0.5), ("padded", 64, 1.0), ("mixed-k", 16, 1.0), ("mixed-k", 64, 0.5)]
# generator seed per case: the first from 5000 on under which test_dyadic_twin_target_is_exact holds (found on the CPU, with the twin alone)
DYADIC_SEEDS = {("padded", 16): 5001, ("padded", 64): 5001, ("mixed-k", 16): 5000, ("mixed-k", 64): 5000}
SHIPPED = (20, 400, 300)
GRADIENT_CASES = [("padded", 48), (SHIPPED, 100)]                 # (shape, B) of the GPU gradient test


def td3_config(cfg, **kw):
    """A TD3Config with the fields of a DDPGConfig ``cfg`` (a dyadic problem's), ring capacity RING, and ``kw`` on top."""
    from rl_mpc_lanemerging_amd import learner
    base = dict(n_obs=cfg.n_obs, h1=cfg.h1, h2=cfg.h2, batch=cfg.batch, capacity=RING, replay_start=cfg.replay_start, gamma=cfg.gamma, tau=cfg.tau,
                lr_q=cfg.lr_q, lr_pi=cfg.lr_pi, time_scale=cfg.time_scale, action_low=cfg.action_low, action_high=cfg.action_high)
    base.update(kw)
    return learner.TD3Config(**base)


def td3_dyadic_problem(shape, B, gamma, seed=None):
    """(cfg, params, replay): see the module text.  One generator seed per case, chosen so that the minibatch of update 0 has rows with Qt1 < Qt2, rows
    with Qt2 < Qt1 and both values of mask (asserted below)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape]
    rng = np.random.default_rng(DYADIC_SEEDS[shape, B] if seed is None else seed)
    cfg, p, replay = dyadic_problem(shape, B, rng)
    cfg = td3_config(cfg, gamma=gamma, target_noise=0.0)
    replay = {k: v[:RING] for k, v in replay.items()}
    params = learner.new_params_td3(p["actor"], p["critic"], _dyadic_net(rng, n_obs + 2, h1, h2, 1.0))
    params["actor_target"] = {k: v.copy() for k, v in p["actor_target"].items()}
    params["actor_target"]["w2"][:] = 0.0
    params["actor_target"]["b2"][:] = 0.0
    params["critic_target"] = {k: v.copy() for k, v in p["critic_target"].items()}
    params["critic2_target"] = {k: v.copy() for k, v in _dyadic_net(rng, n_obs + 2, h1, h2, 1.0).items()}
    return cfg, params, replay


def minibatch_host(replay, cfg, update=0, seed=SEED):
    """(rows, the minibatch dict) a learner with ``seed`` samples at ``update`` from ``replay`` pushed into an empty ring."""
    from rl_mpc_lanemerging_amd import learner
    rows = replay_rows_host(replay, cfg)
    rows = rows[learner.sample_indices_host(seed, update, cfg.batch, rows.shape[0])]
    return rows, learner.batch_from_rows(rows, cfg.n_obs)


def random_td3_problem(shape, B, seed=0, **kw):
    """An ordinary floating-point problem: (cfg, params with targets that differ from the online nets and critic 2 != critic 1, RING replay rows).
    Both tensors of the last layers are drawn away from their zero initialisation (as test_actor_pop._nonzero_last_layers does).  For b2 this matters
    to the 4 x rule on PARAMETERS: a scalar that starts at zero is nothing but the sum of its Adam steps, so its relative error is the steps' -- and
    k_ddpg_adam's float32 bias corrections (running products beta^t, 1 - beta2^t formed in float32; the arithmetic TD3 must share with DDPG bit for
    bit) put 2.6e-6 on such a sum where torch's double-precision corrections put 3e-7 (test_float32_adam_on_a_zero_initialised_scalar)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape] if isinstance(shape, str) else shape
    rng = np.random.default_rng(seed)
    base = dict(n_obs=n_obs, h1=h1, h2=h2, batch=B, capacity=RING, replay_start=0, lr_q=1e-3, lr_pi=5e-4, action_low=-5.0, action_high=5.0)
    base.update(kw)
    cfg = learner.TD3Config(**base)
    nets = [learner.init_net(n_obs + 1, h1, h2, rng), learner.init_net(n_obs + 2, h1, h2, rng), learner.init_net(n_obs + 2, h1, h2, rng)]
    for n in nets:
        n["w2"] = rng.normal(0, 0.1, n["w2"].shape).astype(np.float32)
        n["b2"] = rng.normal(0, 0.1, 1).astype(np.float32)
    params = learner.new_params_td3(*nets)
    for slot in ("actor_target", "critic_target", "critic2_target"):
        for k in learner.TENSORS:
            params[slot][k] = params[slot][k] + rng.normal(0, 0.01, params[slot][k].shape).astype(np.float32)
    kind = rng.integers(0, 4, RING)
    replay = {"obs": rng.normal(0, 1, (RING, n_obs)).astype(np.float32), "next_obs": rng.normal(0, 1, (RING, n_obs)).astype(np.float32),
              "ticks": rng.integers(0, 500, RING).astype(np.int32), "action": rng.uniform(-5, 5, RING), "reward": rng.normal(0, 1, RING),
              "terminated": kind == 2, "truncated": kind == 3}
    return cfg, params, replay


def td_error_cancellation(cfg, params, replay, seed=SEED):
    """The smallest |mean| / rms, on the minibatch of update 0 (float64 twin, host noise), of the per-row terms whose mean is the gradient of an output
    bias: Q_i - y for both critics, and dQ1/da * scale * (1 - tanh^2) for the actor.  Where the terms of a minibatch cancel to a small fraction of
    their size, that gradient's RELATIVE error is rounding noise magnified by the inverse of this number -- in the float32 twin as much as on the
    device -- and the 4 x rule would compare two draws of noise."""
    import torch
    from rl_mpc_lanemerging_amd import learner
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    _, batch = minibatch_host(replay, cfg, 0, seed)
    eps = learner.smoothing_eps_host(learner.smoothing_noise_host(seed, 0, cfg.batch)[2], cfg)
    _, i = learner.update_host_td3(params, batch, cfg, "float64", eps=eps, grads_only=True)
    y = i["targets"][:, 3].mean()
    s = T(batch["s"])
    z = learner._mlp({k: T(params["actor"][k]) for k in learner.TENSORS}, s)
    a = (torch.tanh(z) * cfg.tanh_scale + cfg.tanh_mean).requires_grad_(True)
    q = learner._mlp({k: T(params["critic"][k]) for k in learner.TENSORS}, torch.cat([s, a[:, None]], 1))
    term = (torch.autograd.grad(q.sum(), a)[0] * cfg.tanh_scale * (1 - torch.tanh(z) ** 2)).numpy()
    return min(abs(i["mean_q"] - y) / np.sqrt(i["critic_loss"]), abs(i["mean_q2"] - y) / np.sqrt(i["critic2_loss"]),
               abs(term.mean()) / np.sqrt((term ** 2).mean()))


def conditioned_problem(shape, B, lo, **kw):
    """``random_td3_problem`` under the first generator seed >= lo whose bias-gradient terms cancel to no less than a tenth of their size (found with
    the float64 twin alone, on the CPU)."""
    for seed in range(lo, lo + 64):
        out = random_td3_problem(shape, B, seed=seed, **kw)
        if td_error_cancellation(*out) >= 0.1:
            return out
    raise AssertionError("no seed found")


def ddpg_view(params):
    """The DDPG learner's part of TD3 parameters (critic 2 dropped, beta_pow [4])."""
    p = {k: v for k, v in params.items() if not k.startswith("critic2")}
    p["beta_pow"] = np.array(params["beta_pow"][:4], dtype=np.float32)
    return p


def degenerate(cfg, params):
    """TD3 that must equal DDPG: no target noise, policy_delay 1, critic 2 a copy of critic 1 in all four slots."""
    cfg = td3_config(cfg, target_noise=0.0, policy_delay=1)
    p = dict(params)
    for slot in ("critic", "critic_target", "critic_m", "critic_v"):
        p[slot.replace("critic", "critic2")] = {k: np.array(v) for k, v in params[slot].items()}
    return cfg, p


def clipped_seed(cfg, lo=0, n=64):
    """The first learner seed >= lo whose smoothing noise of update 0 is clipped on some of the cfg.batch rows and not on others (host twin)."""
    from rl_mpc_lanemerging_amd import learner
    for seed in range(lo, lo + n):
        g = learner.smoothing_noise_host(seed, 0, cfg.batch)[2]
        hit = np.abs(cfg.target_noise_std * g) > cfg.noise_clip_abs
        if 2 <= hit.sum() <= cfg.batch - 2:
            return seed
    raise AssertionError("no seed found")


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_td3():
    capi = _capi()
    from test_host_cpu import _header_struct_fields
    lib = capi.load()
    header = open(os.path.join(REPO, "include", "stmpc.h")).read()
    declared = {n for n in re.findall(r"\b(stmpc_[a-z_0-9]+)\s*\(", header) if n.startswith("stmpc_td3_")}
    assert declared == {"stmpc_td3_create", "stmpc_td3_destroy", "stmpc_td3_base", "stmpc_td3_set_params", "stmpc_td3_get_params", "stmpc_td3_set_state",
                        "stmpc_td3_get_state", "stmpc_td3_update_device", "stmpc_td3_grads_device", "stmpc_td3_targets_device", "stmpc_td3_stats_device",
                        "stmpc_td3_noise"}
    assert declared == {n for n in capi.EXPORTS if n.startswith("stmpc_td3_")}
    for name in declared:
        assert getattr(lib, name) is not None and getattr(lib, name).argtypes is not None, name
    ctype_of = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "stmpc_ddpg_cfg": capi.DDPGCfg}
    want = _header_struct_fields("stmpc_td3_cfg")
    have = list(capi.TD3Cfg._fields_)
    assert [n for n, _ in want] == [n for n, _ in have] and [ctype_of[t] for _, t in want] == [t for _, t in have]
    assert ctypes.sizeof(capi.TD3Cfg) == ctypes.sizeof(capi.DDPGCfg) + 24
    flat = " ".join(header.split())
    for i, slot in enumerate(capi.TD3_SLOTS):
        assert "#define STMPC_TD3_%s %d" % (slot.upper(), i) in flat, slot
    assert "#define STMPC_ABI_VERSION 8" in flat and capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8
    assert lib.stmpc_td3_base.restype is ctypes.c_void_p and lib.stmpc_td3_noise.restype is ctypes.c_double
    from rl_mpc_lanemerging_amd import learner
    c = learner.TD3Config()
    assert (c.target_noise_std, c.noise_clip_abs, c.policy_delay) == (0.2 * c.tanh_scale, 0.5 * c.tanh_scale, 2)
    cc = c.to_c_td3(7)
    assert (cc.base.seed, cc.base.batch, cc.target_noise_std, cc.noise_clip, cc.policy_delay) == (7, c.batch, c.target_noise_std, c.noise_clip_abs, 2)


def test_smoothing_noise_twin_equals_the_c_twin_on_its_own_stream():
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    for seed in (0, 1, 12345, 2 ** 63 + 11, 2 ** 64 - 1):
        for update in (0, 1, 77, 2 ** 33):
            u1, u2, g = learner.smoothing_noise_host(seed, update, 16)
            a1, a2, _ = learner.noise_host(seed, update, 16)
            assert not np.array_equal(u1, a1) and not np.array_equal(u2, a2)       # same (seed, call, row), another stream: other draws
            for e in range(16):
                gc, c1, c2 = capi.td3_noise(seed, update, e)
                assert (c1, c2) == (int(u1[e]), int(u2[e])) and c1 < 2 ** 24 and c2 < 2 ** 24
                assert (c1, c2) != capi.ddpg_noise(seed, update, e)[1:]
                assert abs(gc - g[e]) <= 4 * np.spacing(abs(g[e])) + 1e-300      # two libms' log / cos in fp64
    assert learner.TD3_STREAM != learner.NOISE_STREAM
    g = np.concatenate([learner.smoothing_noise_host(5, c, 512)[2] for c in range(8)])
    assert abs(g.mean()) < 0.06 and abs(g.std() - 1) < 0.05
    cfg = learner.TD3Config()
    eps = learner.smoothing_eps_host(g, cfg)
    assert np.abs(eps).max() == cfg.noise_clip_abs and 0 < np.count_nonzero(np.abs(eps) == cfg.noise_clip_abs) < eps.size // 10


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_degenerate_td3_twin_is_the_ddpg_twin(dtype):
    _capi()
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = random_td3_problem("padded", 48, seed=2)
    cfg, p3 = degenerate(cfg, params)
    pd = ddpg_view(params)
    for u in range(4):
        _, batch = minibatch_host(replay, cfg, u)
        p3, i3 = learner.update_host_td3(p3, batch, cfg, dtype)
        pd, idd = learner.update_host(pd, batch, cfg, dtype)
        for slot in capi_slots():
            for k in learner.TENSORS:
                assert p3[slot][k].dtype == np.dtype(dtype) and np.array_equal(p3[slot][k], pd[slot][k]), (u, slot, k)
                if slot.startswith("critic"):
                    assert np.array_equal(p3[slot.replace("critic", "critic2")][k], pd[slot][k]), (u, slot, k)
        assert np.array_equal(p3["beta_pow"][:4], pd["beta_pow"]) and np.array_equal(p3["beta_pow"][4:], pd["beta_pow"][2:]) and p3["updates"] == pd["updates"] == u + 1
        assert i3["critic_loss"] == i3["critic2_loss"] == idd["critic_loss"] and i3["mean_q"] == idd["mean_q"]
        for k in learner.TENSORS:
            assert np.array_equal(i3["grad_critic"][k], idd["grad_critic"][k]) and np.array_equal(i3["grad_actor"][k], idd["grad_actor"][k])
    assert np.abs(pd["actor"]["w1"] - params["actor"]["w1"]).max() > 0


def capi_slots():
    return _capi().DDPG_SLOTS


def test_delay_schedule_of_the_twin():
    """policy_delay = 3, 7 updates: the actor, all three targets and the actor's beta powers change exactly at updates 3 and 6; the critics step every time."""
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    cfg, p, replay = random_td3_problem("padded", 48, seed=3, policy_delay=3)
    eq = lambda a, b: all(np.array_equal(a[k], b[k]) for k in learner.TENSORS)
    delayed = ("actor", "actor_m", "actor_v", "actor_target", "critic_target", "critic2_target")
    for u in range(7):
        _, batch = minibatch_host(replay, cfg, u)
        eps = learner.smoothing_eps_host(learner.smoothing_noise_host(SEED, u, cfg.batch)[2], cfg)
        new, info = learner.update_host_td3(p, batch, cfg, "float64", eps=eps)
        due = u + 1 in (3, 6)
        for slot in delayed:
            assert eq(new[slot], p[slot]) != due, (u, slot)
        assert np.array_equal(new["beta_pow"][:2], p["beta_pow"][:2]) != due and (info["grad_actor"] is not None) == due
        for slot in ("critic", "critic_m", "critic_v", "critic2", "critic2_m", "critic2_v"):
            assert not eq(new[slot], p[slot]), (u, slot)
        assert np.array_equal(new["beta_pow"][2:4], p["beta_pow"][2:4] * np.array([cfg.beta1, cfg.beta2], dtype=np.float32))
        assert np.array_equal(new["beta_pow"][4:], new["beta_pow"][2:4]) and new["updates"] == u + 1
        assert not eq(new["critic"], new["critic2"])
        p = new
    b = np.array([cfg.beta1, cfg.beta2], dtype=np.float32)
    assert np.array_equal(p["beta_pow"][:2], b * b)                 # the actor stepped twice


def target_bits(params, batch, cfg):
    """exactness_bits' measure for what TD3 adds to the critic pass: both target critics on (s', a' = tanh_mean) and y."""
    d = lambda a: np.asarray(a, dtype=np.float64)
    bits = {}

    def stage(name, a, b, bias=None):
        a, b = d(a), d(b)
        e, s = _frac_bits(a) + _frac_bits(b), np.abs(a) @ np.abs(b)
        if bias is not None:
            e, s = max(e, _frac_bits(bias)), s + np.abs(d(bias))
        bits[name] = float(np.log2(max(s.max(), 2.0 ** -e) * 2.0 ** e))
    x2 = np.concatenate([d(batch["s2"]), np.full((len(batch["r"]), 1), cfg.tanh_mean)], 1)
    qt = []
    for slot in ("critic_target", "critic2_target"):
        q = params[slot]
        h1, h2, qv = forward_host(q, x2, np.float64)
        stage(slot + " z1", x2, d(q["w0"]).T, q["b0"])
        stage(slot + " z2", h1, d(q["w1"]).T, q["b1"])
        stage(slot + " Q", h2, d(q["w2"]).T, q["b2"])
        qt.append(qv)
    gm = cfg.gamma * d(batch["mask"])
    stage("y", np.stack([d(batch["r"]), gm * np.minimum(*qt)], 1), np.ones((2, 1)))
    return bits, qt, d(batch["r"]) + gm * np.minimum(*qt)


@pytest.mark.parametrize("shape,B,gamma", [pytest.param(s, B, g, id="%s-B%d-gamma%g" % (s, B, g)) for s, B, g in DYADIC_CASES])
def test_dyadic_twin_target_is_exact(shape, B, gamma):
    _capi()
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = td3_dyadic_problem(shape, B, gamma)
    assert cfg.target_noise_std == 0.0 and cfg.gamma == gamma and cfg.tanh_mean == 0.0 and B & (B - 1) == 0
    _, batch = minibatch_host(replay, cfg)
    bits, (qt1, qt2), y = target_bits(params, batch, cfg)
    for name in ("critic", "critic2"):                             # each critic's passes against y: exactness_bits with y in the reward's place
        sub = exactness_bits(dict(params, critic=params[name]), dict(batch, r=y))
        bits.update({name + ": " + k: v for k, v in sub.items() if not k.startswith("actor")})
    worst = max(bits, key=bits.get)
    print("%s B%d gamma %g: widest %s, %.1f bits" % (shape, B, gamma, worst, bits[worst]))
    assert bits[worst] < 24, bits
    # min is exercised both ways, and mask takes both values
    assert np.count_nonzero(qt1 < qt2) >= 2 and np.count_nonzero(qt2 < qt1) >= 2, (np.count_nonzero(qt1 < qt2), np.count_nonzero(qt2 < qt1))
    assert set(np.unique(batch["mask"])) == {0.0, 1.0}
    _, i32 = learner.update_host_td3(params, batch, cfg, "float32", grads_only=True)
    _, i64 = learner.update_host_td3(params, batch, cfg, "float64", grads_only=True)
    assert i32["targets"].dtype == np.float32 and np.array_equal(i32["targets"].astype(np.float64), i64["targets"])
    assert np.array_equal(i64["targets"][:, 0], np.zeros(B)) and np.array_equal(i64["targets"][:, 3], y)
    assert np.array_equal(i64["targets"][:, 1], qt1) and np.array_equal(i64["targets"][:, 2], qt2)
    for name in ("grad_critic", "grad_critic2"):
        for k in learner.TENSORS:
            g32, g64 = i32[name][k], i64[name][k]
            assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), g64), (name, k)
            assert np.count_nonzero(g64) * 3 >= g64.size, (name, k)
    assert not np.array_equal(i64["grad_critic"]["w1"], i64["grad_critic2"]["w1"])


def test_gpu_seeds_show_a_clipped_row():
    """The seed the GPU smoothing test uses is found here, on the twin alone: at B = 100 some row's noise is clipped by c and some is not."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    cfg = random_td3_problem(SHIPPED, 100)[0]
    assert (cfg.target_noise_std, cfg.noise_clip_abs) == (1.0, 2.5)
    seed = clipped_seed(cfg)
    eps = learner.smoothing_eps_host(learner.smoothing_noise_host(seed, 0, 100)[2], cfg)
    assert 2 <= np.count_nonzero(np.abs(eps) == 2.5) <= 98 and np.abs(eps).max() == 2.5


def test_gradient_problems_are_well_conditioned():
    """The problems of the GPU gradient test: the terms behind every output-bias gradient cancel to no less than a tenth of their rms."""
    _capi()
    for shape, B in GRADIENT_CASES:
        ratio = td_error_cancellation(*conditioned_problem(shape, B, 13))
        print("%s B%d: smallest |mean| / rms of the bias-gradient terms = %.3f" % (shape, B, ratio))
        assert ratio >= 0.1


def test_float32_adam_on_a_zero_initialised_scalar():
    """Why random_td3_problem draws b2 away from zero.  Seven Adam steps on gradients of the size and signs a critic's output bias sees, from w = 0:
    ``adam_host`` (k_ddpg_adam's float32 statement, which the suite pins bit for bit on the device) ends a few 1e-6 from exact Adam, relative to
    the sum -- its bias corrections are float32 running products, and 1 - 0.999^t loses 3e-5 / t of relative precision there -- while on a scalar of
    ordinary size the same steps leave an error at the float32 rounding of the scalar itself."""
    _capi()
    import math
    from rl_mpc_lanemerging_amd import learner
    cfg = learner.TD3Config(lr_q=1e-3)
    g = [-0.645, -0.205, 0.269, 0.406, -0.202, 0.362, 0.537]
    f = np.float32
    for w0, lo, hi in ((0.0, 1e-6, 1e-5), (0.1, 0.0, 1e-7)):
        w = m = v = 0.0
        w += w0
        wd, md, vd, wt, bp = f(w0), f(0), f(0), f(0), np.ones(2, f)
        for k, gk in enumerate(g, 1):
            m, v = cfg.beta1 * m + (1 - cfg.beta1) * gk, cfg.beta2 * v + (1 - cfg.beta2) * gk * gk
            w -= (cfg.lr_q / (1 - cfg.beta1 ** k)) * m / (math.sqrt(v) / math.sqrt(1 - cfg.beta2 ** k) + cfg.eps)
            wd, md, vd, wt, bp = learner.adam_host(wd, f(gk), md, vd, wt, bp, cfg.lr_q, cfg)
        rel = abs(float(wd) - w) / abs(w)
        print("from %.1f: exact %.9g, float32 statement %.9g, relative difference %.2e" % (w0, w, float(wd), rel))
        assert lo <= rel <= hi
