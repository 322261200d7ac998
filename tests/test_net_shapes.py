"""The actor and DDPG kernels (csrc/stmpc_actor_kernels.hpp, csrc/stmpc_ddpg_kernels.hpp and their population entries) at network shapes other than
the shipped 21-400-300-1, on the GPU.  The shapes and what each reaches are learner_testlib.SHAPES.

1. Bit for bit on the exact-arithmetic problems of learner_testlib.py (test_net_shapes_cpu.py asserts, on the CPU, that every partial sum of the critic's passes
   is a float32 number whatever the summation order): the critic's six gradient tensors, the gathered minibatch, the parameters' round trip.
   Acting and the fused k_actor_eval on the same weights: the pre-tanh output is exact, tanh is not, so these two carry the one bound each that the
   test states.
2. The 4 x rule of learner_testlib.py on ordinary random problems, for what cannot be exact: the actor's gradient,
   gamma = 0.99 with targets, padded minibatch rows; then two updates against adam_host within the same 2 ulps.
3. Populations bit-equal to their members alone, and wide networks that keep working after narrower ones were created (the dynamic-LDS attribute
   of a kernel is only ever raised).
No test uses an environment: replays are synthetic pushes, parameters come through ``init=`` / ``load_state_dict``.
"""
import numpy as np
import pytest

from learner_testlib import (CAP, EXACT_CASES, FLOOR, SEED, SHAPES, TIME_SCALE, assert_same as _assert_same, check_4x as _check_4x, dev as _dev, forward_host,
                             host_minibatch, problem, push as _push, random_problem as _random_problem, record as _record, replay_rows_host, snapshot as _snapshot)
from stmpc_testlib import (ACTOR_N as N, ACTOR_N_PER as N_PER, ACTOR_P as P, actor_settings as _settings, actor_states as _states, actor_two_steps as _two_steps,
                           assert_steps_equal as _assert_steps_equal, capi as _capi, slice_steps as _slice_steps)

SMALL = ("one-tile", "padded", "mixed-k", "wide-h2")
# a state vector (FeaturesCfg) as long as the actor's input, per shape: settings overrides, time feature.  one-tile (6 inputs) and wide-h2 (2) have no
# state vector of their length (the shortest is 4, then 7): their fused-kernel actor takes the next longer one, its first columns the learner's W0
FEATURES = {"one-tile": (dict(CARS_AHEAD=1, CARS_BEHIND=0, USE_ACCELERATION_OF_OTHER_CARS=False), False, 7),
            "padded": (dict(CARS_AHEAD=2, CARS_BEHIND=2, USE_ACCELERATION_OF_OTHER_CARS=True), True, 21),
            "mixed-k": (dict(CARS_AHEAD=5, CARS_BEHIND=4, USE_ACCELERATION_OF_OTHER_CARS=False), False, 31),
            "wide-h2": (dict(CARS_AHEAD=0, CARS_BEHIND=0, USE_ACCELERATION_OF_OTHER_CARS=True), False, 4),
            "over-64K": (dict(CARS_AHEAD=2, CARS_BEHIND=2, USE_ACCELERATION_OF_OTHER_CARS=True), True, 21)}


def _exact_learner(gpu_ctx, shape, B):
    """The learner of one exact problem: its parameters (targets included) loaded, its replay pushed."""
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay = problem(shape, B)
    L = learner.DDPGLearner(cfg.n_obs, cfg, seed=SEED, init={"actor": params["actor"], "critic": params["critic"]}, ctx=gpu_ctx)
    L.load_state_dict({"params": params, "counters": None})
    _push(L, replay)
    return L, cfg, params, replay


def _assert_exact_critic_gradients(L, cfg, params, replay, update=0):
    from rl_mpc_lanemerging_amd import learner
    rows, batch = host_minibatch(replay, cfg, update)
    assert np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32))
    _, gq = L.grads()
    _, i64 = learner.update_host(params, batch, cfg, "float64", grads_only=True)
    for k in learner.TENSORS:
        want = i64["grad_critic"][k]
        assert gq[k].dtype == np.float32 and gq[k].shape == want.shape and np.abs(want).max() > 0
        assert np.array_equal(gq[k].astype(np.float64), want), (k, int(np.count_nonzero(gq[k].astype(np.float64) != want)), want.size)


def _assert_params_equal(have, want):
    from rl_mpc_lanemerging_amd import learner
    for slot in _capi().DDPG_SLOTS:
        for k in learner.TENSORS:
            assert np.array_equal(have[slot][k].view(np.uint32), np.asarray(want[slot][k], dtype=np.float32).view(np.uint32)), (slot, k)


# ---- 1. bit for bit -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,B", [pytest.param(s, B, id="%s-B%d" % (s, B)) for s, B in EXACT_CASES])
def test_gpu_critic_gradients_are_exact(shape, B, gpu_ctx, restore_settings):
    """k_replay_push, the gather, ddpg_layer forward and backward (the transposed packing p1t), every job type of k_ddpg_wgrad and k_ddpg_unpad: the six
    tensors equal update_host(float64) value for value.  No summation order can matter: test_net_shapes_cpu.py bounds every partial sum below 2^24 units."""
    L, cfg, params, replay = _exact_learner(gpu_ctx, shape, B)
    assert L.stats()["fill"] == len(replay["ticks"])
    assert np.array_equal(gpu_ctx.ddpg_replay_read(L.handle, 0, len(replay["ticks"])).view(np.uint32), replay_rows_host(replay, cfg).view(np.uint32))
    _assert_exact_critic_gradients(L, cfg, params, replay)
    after = L.state_dict()["params"]
    _assert_params_equal(after, params)                           # grads() applies nothing
    assert after["updates"] == 0 and np.array_equal(after["beta_pow"], params["beta_pow"])
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_acting_on_exact_weights(shape, gpu_ctx, restore_settings):
    """k_ddpg_act (actor_layer's unrolled and tail loops, idle waves, a ragged last round of tiles) for N = 1, 16, 17 and 50 rows.
    The bound: the pre-tanh output z is exact -- the weights and inputs are the exact problem's, so actor_layer's float32 chain and the last layer's
    fp64 dot product round nothing, and the float64 twin's z is the device's.  The kernel then forms float32(tanh_fp64(z)) * scale + mean in float32
    (mean = 0 here).  The twin forms the same from numpy's tanh; two fp64 tanh implementations that differ in the last fp64 place give float32
    roundings t, t' at most one float32 ulp u(t) <= 2^-24 apart (|t| < 1), so the products differ by at most scale * 2^-24 = 5 * 2^-24 before their one
    rounding to a grid no coarser than ulp(scale) = 2^-21 = 8 * 2^-24: after it they are equal or one grid step apart.  Bound: 1 float32 ulp of scale."""
    import torch
    L, cfg, params, replay = _exact_learner(gpu_ctx, shape, 16)
    scale, mean = np.float32(cfg.tanh_scale), np.float32(cfg.tanh_mean)
    assert (scale, mean) == (5.0, 0.0)
    bound = float(np.spacing(scale))
    moved = 0
    for n in (1, 16, 17, 50):
        obs, ticks = replay["obs"][100:100 + n], replay["ticks"][100:100 + n]
        dbg = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
        a = L.act(_dev(obs), _dev(ticks), noise=False, debug=dbg).cpu().numpy()
        greedy = dbg.cpu().numpy().view(np.uint32)[:, 3].copy().view(np.float32)
        x = np.concatenate([obs, (np.float32(TIME_SCALE) * ticks.astype(np.float32))[:, None]], 1)
        z64 = forward_host(params["actor"], x, np.float64)[2]
        assert np.array_equal(forward_host(params["actor"], x, np.float32)[2].astype(np.float64), z64)
        want = np.tanh(z64).astype(np.float32) * scale + mean
        assert want.dtype == np.float32
        err = np.abs(greedy.astype(np.float64) - want.astype(np.float64))
        print("%s N=%d: greedy action, worst error %.3e (bound %.3e), %d of %d rows bit-equal" % (shape, n, err.max(), bound, int((err == 0).sum()), n))
        assert err.max() <= bound, (n, float(err.max()))
        assert np.array_equal(a, greedy.astype(np.float64))       # no noise, inside the Box: the action is the greedy one
        moved += int(np.count_nonzero(np.abs(z64) < 2.0))
    assert moved >= 21                                            # (a quarter of the 84 rows at least: tanh is not saturated)
    assert int(gpu_ctx.ddpg_get_state(L.handle)[0][3]) == 0        # greedy calls do not count
    gpu_ctx.check_error()


def _fused_actor_weights(shape, params, flen, rng):
    """The exact problem's actor for k_actor_eval: W0 widened to ``flen`` columns where no state vector has the learner's input width."""
    w = {k: np.array(v) for k, v in params["actor"].items()}
    n_in = w["w0"].shape[1]
    if flen != n_in:
        assert flen > n_in
        w["w0"] = np.concatenate([w["w0"], rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0], dtype=np.float32), (w["w0"].shape[0], flen - n_in))], 1)
    w["tanh_scale"], w["tanh_mean"] = 5.0, 0.0
    return w


def _eval_fused(gpu_ctx, handle, shape, n=17, K=8):
    """k_actor_eval on ``n`` synthetic states under FEATURES[shape]: (feature vectors, jerks, the host twin's feature vectors)."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi as capi, actor, synth
    flags, tf, flen = FEATURES[shape]
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(flags)
    S = pkg.Settings
    fc = capi.FeaturesCfg.from_settings(S, time_feature=tf)
    ego, kc, ox, ov = synth.generate_states(n, k=7, kmax=K, seed=12, vary_k=True)
    rng = np.random.default_rng(13)
    oa = rng.uniform(-4.0, 2.0, ox.shape)
    evals0 = rng.integers(0, 900, n).astype(np.int32)
    d_ego4, d_k, d_ox, d_ov, d_oa, d_evals = _dev(ego[:, :4]), _dev(kc), _dev(ox), _dev(ov), _dev(oa), _dev(evals0.copy())
    feat = torch.full((n, flen + 3), -7.0, dtype=torch.float32, device="cuda")
    jerk = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    gpu_ctx.actor_eval_device(handle, fc, n, K, 1, d_ego4.data_ptr(), d_k.data_ptr(), d_ox.data_ptr(), d_ov.data_ptr(), d_oa.data_ptr(),
                              d_evals.data_ptr() if tf else 0, feat.data_ptr(), flen + 3, jerk.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gpu_ctx.check_error()
    got = feat.cpu().numpy()
    assert (got[:, flen:] == -7.0).all()                          # nothing written past the vector
    want = np.stack([actor.state_vector_host(S, ego[i, :4], ox[i, :kc[i]], ov[i, :kc[i]], oa[i, :kc[i]], int(evals0[i]) if tf else None) for i in range(n)])
    assert want.shape == (n, flen)
    if tf:
        assert np.array_equal(d_evals.cpu().numpy(), evals0 + 1)
    return got[:, :flen], jerk.cpu().numpy(), want


def _assert_fused(shape, w, feat, jerk, want_feat):
    assert np.array_equal(feat.view(np.uint32), want_feat.view(np.uint32))           # the host twin of test_actor.py, bit for bit
    z = forward_host(w, want_feat, np.float64)[2]
    err = np.abs(jerk - (np.tanh(z) * 5.0))
    print("%s: fused actor, worst jerk error %.3e" % (shape, err.max()))
    assert err.max() < 5e-5, float(err.max())                     # test_actor.py's bound for a float32 chain of another order + tanhf
    assert np.abs(jerk).max() <= 5.0 and np.unique(jerk).size > 4 and np.count_nonzero(np.abs(z) < 2.0) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_fused_actor_kernel_on_exact_weights(shape, gpu_ctx, restore_settings):
    """k_actor_eval through stmpc_actor_create with the exact problem's actor, 17 states (a partial last tile); where the learner's input width is a
    state vector's (padded, over-64K: 21; mixed-k: 31) also through stmpc_actor_view_ddpg on the learner, bit-equal to the created actor."""
    flags, tf, flen = FEATURES[shape]
    L, cfg, params, replay = _exact_learner(gpu_ctx, shape, 16)
    w = _fused_actor_weights(shape, params, flen, np.random.default_rng(3))
    assert w["w0"].shape == (SHAPES[shape][1], flen)
    handle = gpu_ctx.actor_create(w)
    try:
        feat, jerk, want_feat = _eval_fused(gpu_ctx, handle, shape)
        _assert_fused(shape, w, feat, jerk, want_feat)
    finally:
        gpu_ctx.actor_destroy(handle)
    if flen == cfg.n_obs + 1:
        view = gpu_ctx.actor_view_ddpg(L.handle, False)
        try:
            vfeat, vjerk, _ = _eval_fused(gpu_ctx, view, shape)
        finally:
            gpu_ctx.actor_destroy(view)
        assert np.array_equal(vfeat.view(np.uint32), feat.view(np.uint32)) and np.array_equal(vjerk.view(np.uint64), jerk.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL)
def test_gpu_parameters_round_trip(shape, gpu_ctx, restore_settings):
    """load_state_dict -> state_dict over all eight slots with values that are all different: slot_move's and the slot layout's index arithmetic,
    n_obs = 1 and n_obs = 30 (the full 32-wide critic input) included.  Also: the re-packing the upload triggers leaves the parameters alone."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape]
    cfg = learner.DDPGConfig(n_obs=n_obs, h1=h1, h2=h2, batch=16, capacity=64, replay_start=0, action_low=-5.0, action_high=5.0)
    L = learner.DDPGLearner(n_obs, cfg, seed=1, ctx=gpu_ctx)
    rng = np.random.default_rng(8)
    params = {}
    for slot in _capi().DDPG_SLOTS:
        n_in = n_obs + (2 if slot.startswith("critic") else 1)
        flat = rng.permutation(np.arange(1, (n_in + 1) * h1 + (h1 + 2) * h2 + 2)).astype(np.float32) / np.float32(8.0)
        if slot.endswith("_v"):
            flat = np.abs(flat)
        params[slot] = learner.unflatten(flat, n_in, h1, h2)
    params["beta_pow"], params["updates"] = np.array([0.9, 0.999, 0.81, 0.998001], dtype=np.float32), 2
    L.load_state_dict({"params": params, "counters": None})
    sd = L.state_dict()
    _assert_params_equal(sd["params"], params)
    assert np.array_equal(sd["params"]["beta_pow"], params["beta_pow"]) and sd["params"]["updates"] == 2 and sd["counters"][2] == 2
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ddpg", "td3-critic2", "dqn"])
def test_gpu_slot_layout_round_trip_off_the_tile(kind, gpu_ctx, restore_settings):
    """set_params -> get_params of every slot of every handle kind at widths that are no multiples of 16 (h1 = 20, h2 = 24, 3 actions), with values
    that are all different within a slot and between slots: the library's segment list against the C-ABI's slot layout.  TD3: critic 2's four
    slots, which leave critic 1's alone.  DQN: also through padded_read -- the real entries are the slot's, the pad entries exact zeros."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2, A = 5, 20, 24, 3
    rng = np.random.default_rng(9)
    distinct = lambda n, i: (rng.permutation(np.arange(1, n + 1)) + 1000 * i).astype(np.float32) / np.float32(8.0)
    kw = dict(n_obs=n_obs, h1=h1, batch=16, capacity=64, replay_start=0)
    len_ddpg = lambda n_in: (n_in + 1) * h1 + (h1 + 2) * h2 + 1
    if kind == "dqn":
        L = learner.DQNLearner((n_obs, A), learner.DQNConfig(n_actions=A, **kw), seed=1, ctx=gpu_ctx)
        n = (n_obs + 1) * h1 + (h1 + 1) * A
        slots = [(i, n) for i in range(4)]
        put, get = (lambda i, flat: gpu_ctx.dqn_set_params(L.handle, i, flat)), (lambda i, n: gpu_ctx.dqn_get_params(L.handle, i, n))
    elif kind == "ddpg":
        L = learner.DDPGLearner(n_obs, learner.DDPGConfig(h2=h2, **kw), seed=1, ctx=gpu_ctx)
        slots = [(i, len_ddpg(n_obs + (2 if i >= 4 else 1))) for i in range(8)]
        put, get = (lambda i, flat: gpu_ctx.ddpg_set_params(L.handle, i, flat)), (lambda i, n: gpu_ctx.ddpg_get_params(L.handle, i, n))
    else:
        L = learner.TD3Learner(n_obs, learner.TD3Config(h2=h2, **kw), seed=1, ctx=gpu_ctx)
        slots = [(i, len_ddpg(n_obs + 2)) for i in range(4)]
        put, get = (lambda i, flat: gpu_ctx.td3_set_params(L.td3, i, flat)), (lambda i, n: gpu_ctx.td3_get_params(L.td3, i, n))
        critic1 = [gpu_ctx.ddpg_get_params(L.handle, 4 + i, n) for i, n in slots]
    want = [distinct(n, i) for i, n in slots]
    for (i, _), flat in zip(slots, want):
        put(i, flat)
    for (i, n), flat in zip(slots, want):                           # (after all were set: no slot's upload or re-packing reaches another)
        assert np.array_equal(get(i, n).view(np.uint32), flat.view(np.uint32)), (kind, i)
    if kind == "td3-critic2":
        assert all(np.array_equal(gpu_ctx.ddpg_get_params(L.handle, 4 + i, n), critic1[i]) for i, n in slots)
    if kind == "dqn":
        real = {"w0": (slice(0, h1), slice(0, n_obs)), "b0": (slice(0, h1),), "w1": (slice(0, A), slice(0, h1)), "b1": (slice(0, A),)}
        for (i, _), flat in zip(slots, want):
            arr, net = gpu_ctx.dqn_padded_read(L.handle, i, h1, A), learner.unflatten_q(flat, n_obs, h1, A)
            for k, sl in real.items():
                pad = np.ones(arr[k].shape, bool)
                pad[sl] = False
                assert np.array_equal(arr[k][sl], net[k]) and not arr[k][pad].any(), (i, k)
    gpu_ctx.check_error()


# ---- 2. the 4 x rule on random problems ---------------------------------------------------------------------------------------------------------
def _random_replay(rng, n_obs, rows=600):
    kind = rng.integers(0, 5, rows)                               # one in five terminated, one in five truncated
    return {"obs": rng.normal(0, 1, (rows, n_obs)).astype(np.float32), "next_obs": rng.normal(0, 1, (rows, n_obs)).astype(np.float32),
            "ticks": rng.integers(0, 500, rows).astype(np.int32), "action": rng.uniform(-5, 5, rows), "reward": rng.normal(0, 1, rows),
            "terminated": kind == 3, "truncated": kind == 4}


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B", [pytest.param(s, B, id="%s-B%d" % (s, B)) for s in ("padded", "mixed-k") for B in (48, 100)])
def test_gpu_random_problem_by_the_4x_rule(shape, B, gpu_ctx, restore_settings):
    """Random float32 parameters (learner_testlib.random_problem's), gamma = 0.99, targets that differ, a synthetic replay of 600 rows.  B = 48 leaves
    five of k_ddpg_wgrad's eight waves without work, B = 100 has 12 padded rows.  Gradients of both networks by the 4 x rule, then two
    updates against adam_host within its 2 ulps."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape]
    rng = np.random.default_rng(31 + B + n_obs)
    cfg, params, _ = _random_problem(rng, B=B, n_obs=n_obs, h1=h1, h2=h2)
    cfg.capacity, cfg.replay_start = 1024, 0
    assert cfg.gamma == 0.99
    replay = _random_replay(rng, n_obs)
    L = learner.DDPGLearner(n_obs, cfg, seed=SEED, init={"actor": params["actor"], "critic": params["critic"]}, ctx=gpu_ctx)
    L.load_state_dict({"params": params, "counters": None})
    _push(L, replay)
    rows, batch = host_minibatch(replay, cfg)
    assert np.array_equal(L.minibatch().view(np.uint32), rows.view(np.uint32)) and 0 < batch["mask"].sum() < B
    ga, gq = L.grads()
    _, i64 = learner.update_host(params, batch, cfg, "float64", grads_only=True)
    _, i32 = learner.update_host(params, batch, cfg, "float32", grads_only=True)
    ratios, ok = {}, True
    for net, g in (("critic", gq), ("actor", ga)):
        for k in learner.TENSORS:
            assert np.abs(i64["grad_" + net][k]).max() > 0, (net, k)
            ok &= _check_4x("%s B%d grad %s.%s" % (shape, B, net, k), g[k], i32["grad_" + net][k], i64["grad_" + net][k], ratios)
    _record("net_shapes_%s_gradients_B%d" % (shape, B), ratios)
    assert FLOOR == 8 * 2.0 ** -23 and ok, ratios
    worst = 0.0
    for it in range(2):                                           # test_gpu_adam_and_polyak_equal_the_numpy_twin's check
        sd = L.state_dict()["params"]
        ga, gq = L.grads()
        L.update(1, lr_q=0.0, lr_pi=3e-4)
        new = L.state_dict()["params"]
        for net, g, lr, o in (("critic", gq, 0.0, 2), ("actor", ga, 3e-4, 0)):
            for k in learner.TENSORS:
                w, m, v, wt, bp = learner.adam_host(sd[net][k], g[k], sd[net + "_m"][k], sd[net + "_v"][k], sd[net + "_target"][k], sd["beta_pow"][o:o + 2], lr, cfg)
                for name, have, want in (("w", new[net][k], w), ("m", new[net + "_m"][k], m), ("v", new[net + "_v"][k], v), ("target", new[net + "_target"][k], wt)):
                    ulps = np.abs(have.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                    worst = max(worst, float(ulps.max()))
                    assert ulps.max() <= 2, (it, net, k, name, float(ulps.max()))
            assert np.array_equal(new["beta_pow"][o:o + 2], bp)
        assert new["updates"] == it + 1 and np.abs(new["actor"]["w1"] - sd["actor"]["w1"]).max() > 0
    print("%s B%d: Adam + Polyak vs adam_host, worst difference %.2f float32 ulps" % (shape, B, worst))
    _record("net_shapes_%s_adam_max_ulps_B%d" % (shape, B), worst)
    gpu_ctx.check_error()


# ---- 3. populations and coexistence -------------------------------------------------------------------------------------------------------------
class _Rows:
    """What DDPGPopulation asks of an env, without one: the row count, the observation width, the action space's kind and the context."""
    continuous = True

    def __init__(self, n, obs_dim, ctx):
        self.n, self.obs_dim, self.ctx = n, obs_dim, ctx


@pytest.mark.gpu
def test_gpu_ddpg_population_at_the_padded_shape(gpu_ctx, restore_settings):
    """Three members at 21-40-24-1 (pads in both widths), B = 48: after three updates every member equals a lone learner with the same seed, pushes and
    parameters, bit for bit (learner_testlib's snapshot and comparison: parameters, Adam state, counters, ring, statistics)."""
    import torch
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES["padded"]
    P, n_per, seeds = 3, 24, (11, 12, 13)
    cfgs = [learner.DDPGConfig(n_obs=n_obs, h1=h1, h2=h2, batch=48, capacity=CAP, replay_start=0, gamma=(0.99, 0.95, 0.9)[m], tau=(0.005, 0.01, 0.02)[m],
                               lr_q=(2e-4, 1e-3, 5e-4)[m], lr_pi=(2e-4, 3e-4, 1e-4)[m], action_low=-5.0, action_high=5.0) for m in range(P)]
    inits = []
    for m in range(P):
        _, params, _ = _random_problem(np.random.default_rng(200 + m), B=48, n_obs=n_obs, h1=h1, h2=h2)
        inits.append({"actor": params["actor"], "critic": params["critic"]})
    env = _Rows(P * n_per, n_obs, gpu_ctx)
    pop = learner.DDPGPopulation(env, cfgs, seeds=list(seeds), init=inits)
    lone = [learner.DDPGLearner(n_obs, cfgs[m], seed=seeds[m], init=inits[m], ctx=gpu_ctx) for m in range(P)]
    rng = np.random.default_rng(9)
    for step in range(3):
        rp = _random_replay(rng, n_obs, rows=P * n_per)
        t = {k: _dev(v) for k, v in rp.items()}
        pop.push(t["obs"], t["ticks"], t["action"], t["reward"], t["next_obs"], t["terminated"], t["truncated"])
        pop.update(1)
        for m, L in enumerate(lone):
            _push(L, rp, slice(m * n_per, (m + 1) * n_per))
            L.update(1)
    torch.cuda.synchronize()
    ps = pop.stats()
    assert list(ps["updates"]) == [3] * P and list(ps["fill"]) == [3 * n_per] * P
    snaps = []
    for m, L in enumerate(lone):
        s = L.stats()
        snaps.append(_snapshot(gpu_ctx, pop.member(m), [ps["critic_loss"][m], ps["mean_q"][m], float(ps["fill"][m]), float(ps["updates"][m])]))
        _assert_same(snaps[m], _snapshot(gpu_ctx, L, [s["critic_loss"], s["mean_q"], float(s["fill"]), float(s["updates"])]), "member %d vs alone" % m)
        assert np.isfinite(snaps[m]["stats"][0]) and np.abs(snaps[m]["params"]["actor"]["w1"] - inits[m]["actor"]["w1"]).max() > 0
    assert not np.array_equal(snaps[0]["params"]["critic"]["w1"], snaps[1]["params"]["critic"]["w1"])
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_actor_population_at_the_mixed_k_widths(gpu_ctx, restore_settings, tmp_path):
    """Three actors with mixed-k's hidden widths (96, 48: six k blocks -- the unrolled loop, then a tail of one -- and three tiles for eight waves),
    24 rows each, two rollout steps: every member equals the lone actor on its slice, bit for bit (test_actor_pop.py's steps and states, from stmpc_testlib).
    ActorPopulation always feeds the time feature, and no state vector with it has mixed-k's 31 entries; nine vehicles of three entries and the
    five ego entries give 32, the widest input the kernel takes (AT_KIN), which no other test reaches."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, learner
    g, S = _settings()
    pkg.apply_overrides(dict(CARS_AHEAD=5, CARS_BEHIND=4, USE_ACCELERATION_OF_OTHER_CARS=False))
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _states(g, dev)
    paths = []
    for m in range(P):
        rng = np.random.default_rng(300 + m)
        net = learner.init_net(32, 96, 48, rng)
        net["w2"], net["b2"] = rng.normal(0, 0.2, (1, 48)).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32)
        paths.append(str(tmp_path / ("actor%d.npz" % m)))
        learner.write_actor(paths[m], net, 5.0, 0.0)
    pop = actor.ActorPopulation(paths, N_PER, gpu_ctx, S)
    assert (pop.P, pop.n, pop.flen) == (P, N, 32) and pop.members[0].shape == (32, 96, 48)
    got = _two_steps(gpu_ctx, S, pop, st, slice(0, N))
    assert (got[1]["evals"] - got[0]["evals"]).min() == 0 < (got[1]["evals"] - got[0]["evals"]).max()
    for m in range(P):
        sl = slice(m * N_PER, (m + 1) * N_PER)
        lone = actor.DDPGActor(paths[m], N_PER, gpu_ctx, S, dev)
        want = _two_steps(gpu_ctx, S, lone, st, sl)
        _assert_steps_equal(_slice_steps(got, sl), want, "member %d" % m)
        w = actor.load_weights(paths[m])
        ref = actor.forward_host(w, want[0]["feat"], np.float64)
        assert np.abs(want[0]["jerk"] - ref).max() < 5e-5       # and the lone actor is the network (test_actor.py's bound)
    assert np.abs(got[0]["jerk"]).max() <= 5.0 and got[0]["jerk"].std() > 0.05 and (got[0]["feat"][:, 27:31] != 0).any()


@pytest.mark.gpu
def test_gpu_wide_learner_keeps_its_lds_when_narrower_ones_follow(gpu_ctx, restore_settings):
    """A 512 x 512 learner (68.75 KB of dynamic LDS per workgroup), then one at the shipped 400 x 300 (49.9 KB: above the 48 KB at which the attribute is
    set at all), then a one-tile learner: the kernels' dynamic-LDS attribute is raised, never lowered, so the wide learner still acts, updates and gives
    the exact problem's critic gradients."""
    import torch
    from rl_mpc_lanemerging_amd import learner
    wide, cfg, params, replay = _exact_learner(gpu_ctx, "over-64K", 16)
    shipped = learner.DDPGLearner(20, learner.DDPGConfig(n_obs=20, batch=16, capacity=64, replay_start=0, action_low=-5.0, action_high=5.0), seed=2, ctx=gpu_ctx)
    small, scfg, sparams, sreplay = _exact_learner(gpu_ctx, "one-tile", 16)
    assert (shipped.cfg.h1, shipped.cfg.h2) == (400, 300)
    _assert_exact_critic_gradients(wide, cfg, params, replay)
    obs, ticks = replay["obs"][:17], replay["ticks"][:17]
    a = wide.act(_dev(obs), _dev(ticks), noise=False).cpu().numpy()
    z = forward_host(params["actor"], np.concatenate([obs, (np.float32(TIME_SCALE) * ticks.astype(np.float32))[:, None]], 1), np.float64)[2]
    want = (np.tanh(z).astype(np.float32) * np.float32(5.0)).astype(np.float64)
    assert np.abs(a - want).max() <= float(np.spacing(np.float32(5.0)))                     # (the acting test's bound and twin)
    # one update, all six launches, with learning rates 0: Adam's moments and the targets move, the online networks stay, so the next minibatch's
    # critic gradient is still the exact problem's (gamma = 0: it does not see the targets)
    wide.update(1, lr_q=0.0, lr_pi=0.0)
    torch.cuda.synchronize()
    gpu_ctx.check_error()
    after = wide.state_dict()["params"]
    assert after["updates"] == 1 and wide.stats()["updates"] == 1 and np.isfinite(wide.stats()["critic_loss"])
    for k in learner.TENSORS:                                     # a zero learning rate leaves the online nets; the critic's gradient at gamma = 0 needs no more
        assert np.array_equal(after["critic"][k], params["critic"][k]) and np.array_equal(after["actor"][k], params["actor"][k]), k
        assert np.abs(after["critic_m"][k]).max() > 0
    _assert_exact_critic_gradients(wide, cfg, params, replay, update=1)
    # and the narrow ones work next to it
    _assert_exact_critic_gradients(small, scfg, sparams, sreplay)
    shipped.push(_dev(sreplay["obs"][:32, :1].repeat(20, 1)), _dev(sreplay["ticks"][:32]), _dev(sreplay["action"][:32]), _dev(sreplay["reward"][:32]),
                 _dev(sreplay["next_obs"][:32, :1].repeat(20, 1)), _dev(sreplay["terminated"][:32]), _dev(sreplay["truncated"][:32]))
    shipped.update(1)
    assert shipped.stats()["updates"] == 1
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_wide_actor_keeps_its_lds_when_the_shipped_one_follows(gpu_ctx, restore_settings):
    """The same for k_actor_eval (actor_raise_lds has always only raised): a 21-512-512-1 actor, then the shipped medium1, then the wide one evaluates."""
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor
    cfg, params, replay = problem("over-64K", 16)
    w = _fused_actor_weights("over-64K", params, 21, None)
    wide = gpu_ctx.actor_create(w)
    try:
        pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
        shipped = actor.DDPGActor("medium1", 17, gpu_ctx, pkg.Settings)
        assert shipped.shape == (21, 400, 300)
        feat, jerk, want_feat = _eval_fused(gpu_ctx, wide, "over-64K")
        _assert_fused("over-64K", w, feat, jerk, want_feat)
    finally:
        gpu_ctx.actor_destroy(wide)
