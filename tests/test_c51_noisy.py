"""The noisy output layer of the C51 learner on the GPU (``learner.C51Config(noisy=)``, csrc/stmpc_c51_noisy_kernels.hpp, stmpc_noisy_c51_*) against
its host twins, plain and dueling, at (n_obs, h1, A, K, B) = (20, 16, 2, 16, 5), (20, 16, 5, 17, 7) plain and (12, 32, 3, 33, 16),
(20, 48, 19, 51, 33) dueling, and once at the shipped (20, 256, 5, 51, 50).  Rings have 128 rows.

Parity rule for float32 results (tests/learner_testlib.py's): per tensor, max-norm error against ``update_host_c51_noisy("float64")`` fed the
device's own minibatch rows and f vectors at most max(4 x the error of its float32 run, 8 float32 ulps).  The effective parameters, Adam and the
target copy are compared bit for bit."""
import numpy as np
import pytest

from discrete_testlib import (C51, C51_DUELING, LEARNER_SEED, NAMES, Q_SLOTS, RING, expected_values_host, fill as _fill, make_learner as _learner,
                              random_problem)
from learner_testlib import bits_equal, check_4x as _check_4x, dev as _dev, record as _record
from stmpc_testlib import bits as _bits, capi as _capi

CASES = [((20, 16, 2, 16, 5), C51), ((20, 16, 5, 17, 7), C51), ((12, 32, 3, 33, 16), C51_DUELING), ((20, 48, 19, 51, 33), C51_DUELING),
         ((20, 256, 5, 51, 50), C51)]
SMALL = range(4)                 # the shipped shape runs once (the backward test)
SIGMA = ("sigma", "sigma_target", "sigma_m", "sigma_v")
SNAMES = ("w1", "b1")


def _problem(ci, seed, sigma0=0.5, **kw):
    from rl_mpc_lanemerging_amd import learner
    shape, head = CASES[ci]
    cfg, params, replay = random_problem(head, shape, seed, noisy=learner.NoisyConfig(sigma0), **kw)
    return shape, head, cfg, params, replay


def _with_sigma(params, L):
    """The twin's params: the problem's four slots and the learner's sigma slots."""
    sd = L.state_dict()["params"]
    return dict(params, **{s: sd[s] for s in SIGMA})


def _noise_bound(seed, draw, h1, n_out, stream):
    """(f in float64 from the float64 Gaussian, the bound on a device f): test_learner.py's rule for dg_gauss -- logf, sqrtf and cosf good to 1 ulp
    each, half an ulp for the float32 product -- carried through f(e) = sign(e) sqrt|e|: an e within tol of e64 has sqrt|e| within
    sqrt(|e64| + tol) - sqrt(max(|e64| - tol, 0)) (and may have the other sign where |e64| < tol), plus one float32 ulp of f for its rounding."""
    from rl_mpc_lanemerging_amd import learner
    u1, u2, g64 = learner.noise_host(seed, draw, h1 + n_out, stream=stream)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    logv = np.log((u1.astype(np.float64) + 1) * 2.0 ** -24)
    r = np.sqrt(-2 * logv)
    c = np.cos((np.float32(learner.TWO_PI_F32) * (u2.astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float64))
    rel_log = np.where(logv != 0, ulp(logv) / np.where(logv != 0, np.abs(logv), 1), 0)
    tol = np.abs(c) * (ulp(r) + 0.5 * r * rel_log) + r * ulp(c) + 0.5 * ulp(g64)
    f64 = np.sign(g64) * np.sqrt(np.abs(g64))
    a = np.abs(g64)
    tol_f = np.where(a > tol, np.sqrt(a + tol) - np.sqrt(np.maximum(a - tol, 0)), np.sqrt(a + tol) + np.sqrt(tol)) + ulp(f64)
    return f64, tol_f


def _gsigma(g, f_in, f_out):
    """The kernel's g_sigma from the device's gradient and f vectors, in its float32 operation order."""
    return {"w1": (g["w1"] * f_out[:, None]) * f_in[None, :], "b1": g["b1"] * f_out}


# ---- 1: the noise and the effective parameters -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ci", SMALL)
def test_gpu_noise_and_effective_parameters(ci, gpu_ctx, restore_settings):
    """The f vectors of update 0 and 1, online and target, against the host twin under the dg_gauss rule; online differs from target and update u
    from u + 1; W_eff | b_eff of both nets equal c51_noisy_compose_host fed the device's f bit for bit; the padded arrays' pad rows and columns are
    exact zeros; a second learner with the same seed is bit-equal."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    shape, head, cfg, params, replay = _problem(ci, 400 + ci)
    n_obs, h1, A, K, B = shape
    W = head.width(shape)
    L, L2 = (_learner(gpu_ctx, head, cfg, params, replay) for _ in range(2))
    sd = L.state_dict()
    assert sd["noisy"] is True and all((sd["params"][s][k] == (np.float32(0.5 / np.sqrt(h1)) if s in SIGMA[:2] else 0)).all() for s in SIGMA for k in SNAMES)
    seen = []
    for u in range(2):
        L.grads(); L2.grads()                                       # (the learning draw of the current update index, nothing applied)
        for net, which in enumerate(("online", "target")):
            f_in, f_out = L.noise(which)
            f64, tol = _noise_bound(LEARNER_SEED, 2 * u + net, h1, W, learner.NOISY_LEARN_STREAM)
            err = np.abs(np.concatenate([f_in, f_out]).astype(np.float64) - f64)
            print("update %d %s: f, worst error / bound %.3f" % (u, which, float((err / tol).max())))
            assert (err <= tol).all()
            h_in, h_out = learner.c51_noisy_f_host(LEARNER_SEED, 2 * u + net, h1, W)
            assert (np.abs(np.concatenate([h_in, h_out]).astype(np.float64) - f64) <= tol).all()     # (the float32 twin keeps the rule too)
            seen.append(np.concatenate([f_in, f_out]))
            cur = L.state_dict()["params"]
            mu, sg = cur["q_target" if net else "q"], cur["sigma_target" if net else "sigma"]
            want, have = learner.c51_noisy_compose_host(mu, sg, f_in, f_out), L.effective(which)
            assert all(np.array_equal(_bits(have[k]), _bits(want[k])) for k in SNAMES), (u, which)
            assert not np.array_equal(have["w1"], mu["w1"]) and not np.array_equal(have["b1"], mu["b1"])
            pad = L.effective(which, padded=True)
            assert np.array_equal(pad["w1"][:W, :h1], have["w1"]) and np.array_equal(pad["b1"][:W], have["b1"])
            assert not pad["w1"][W:].any() and not pad["w1"][:, h1:].any() and not pad["b1"][W:].any()
            f2 = L2.noise(which)
            assert np.array_equal(_bits(f2[0]), _bits(f_in)) and np.array_equal(_bits(f2[1]), _bits(f_out))
            assert all(np.array_equal(_bits(L2.effective(which)[k]), _bits(have[k])) for k in SNAMES)
        L.update(1); L2.update(1)
    assert all(not np.array_equal(seen[i], seen[j]) for i in range(4) for j in range(i))
    gpu_ctx.check_error()


# ---- 2: the backward pass ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_gpu_targets_distributions_and_gradients(ci, gpu_ctx, restore_settings):
    """dist(), targets(), g_mu and g_sigma against update_host_c51_noisy fed the device's minibatch rows and f vectors, under the parity rule."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    shape, head, cfg, params, replay = _problem(ci, 420 + ci)
    n_obs, h1, A, K, B = shape
    L = _learner(gpu_ctx, head, cfg, params, replay)
    batch = learner.dqn_batch_from_rows(L.minibatch(), n_obs)
    d, t = L.dist()
    g = L.grads()
    f = {w: L.noise(w) for w in ("online", "target")}
    P = _with_sigma(params, L)
    i64, i32 = (learner.update_host_c51_noisy(P, batch, cfg, f, dtype, grads_only=True)[1] for dtype in ("float64", "float32"))
    gs = _gsigma(g, *f["online"])
    ratios, tag, ok = {}, "c51 noisy %s " % (shape,), True
    ok &= _check_4x(tag + "m", d[:, 0], i32["dist"][:, 0], i64["dist"][:, 0], ratios)
    ok &= _check_4x(tag + "p(s, a)", d[:, 1], i32["dist"][:, 1], i64["dist"][:, 1], ratios)
    ok &= _check_4x(tag + "Qt(s', a*)", t[:, 1], i32["targets"][:, 1], i64["targets"][:, 1], ratios)
    ok &= _check_4x(tag + "row loss", t[:, 2], i32["row_loss"], i64["row_loss"], ratios)
    ok &= _check_4x(tag + "Q(s, a)", t[:, 3], i32["q_values"], i64["q_values"], ratios)
    for k in NAMES:
        assert g[k].shape == i64["grad"][k].shape and np.abs(i64["grad"][k]).max() > 0
        ok &= _check_4x(tag + "g_mu " + k, g[k], i32["grad"][k], i64["grad"][k], ratios)
    for k in SNAMES:
        assert np.abs(i64["grad_sigma"][k]).max() > 0
        ok &= _check_4x(tag + "g_sigma " + k, gs[k], i32["grad_sigma"][k], i64["grad_sigma"][k], ratios)
    _record("c51 noisy %s" % (shape,), ratios)
    assert ok
    after = L.state_dict()["params"]
    assert bits_equal(after, params, Q_SLOTS, NAMES) and after["updates"] == 0
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("ci", SMALL)
def test_gpu_sigma0_zero_is_the_plain_learner(ci, gpu_ctx, restore_settings):
    """sigma0 = 0: update 0's targets, distributions and g_mu are value-equal to a plain C51Learner's with the same init, seed and ring."""
    _capi()
    shape, head, cfg, params, replay = _problem(ci, 440 + ci, sigma0=0.0)
    plain_cfg = random_problem(head, shape, 440 + ci)[0]
    N, Pl = _learner(gpu_ctx, head, cfg, params, replay), _learner(gpu_ctx, head, plain_cfg, params, replay)
    assert N.noisy and not Pl.noisy
    (dn, tn), (dp, tp) = N.dist(), Pl.dist()
    gn, gp = N.grads(), Pl.grads()
    assert np.array_equal(dn, dp) and np.array_equal(tn, tp) and all(np.array_equal(gn[k], gp[k]) for k in NAMES)
    eff = N.effective("online")
    assert np.array_equal(eff["w1"], params["q"]["w1"]) and np.array_equal(eff["b1"], params["q"]["b1"])
    gpu_ctx.check_error()


# ---- 3: Adam and the target copy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("period", [1, 3])
@pytest.mark.parametrize("ci", SMALL)
def test_gpu_adam_and_target_copy(ci, period, gpu_ctx, restore_settings):
    """One update with the hard copy (target_period 1) and one without (3): mu, sigma, both targets and all moments equal dqn_adam_host applied to the
    device's own gradients -- g_sigma = (g_W f_out) f_in from the device's g and f -- bit for bit."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    shape, head, cfg, params, replay = _problem(ci, 460 + ci, target_period=period)
    L = _learner(gpu_ctx, head, cfg, params, replay)
    before = L.state_dict()["params"]
    g = L.grads()
    gs = _gsigma(g, *L.noise("online"))
    L.update(1)
    after = L.state_dict()["params"]
    for names, slots, grad in ((NAMES, Q_SLOTS, g), (SNAMES, SIGMA, gs)):
        for k in names:
            w, m, v, bp = learner.dqn_adam_host(before[slots[0]][k], grad[k], before[slots[2]][k], before[slots[3]][k], before["beta_pow"], cfg.lr, cfg)
            assert np.array_equal(_bits(after[slots[0]][k]), _bits(w)) and np.array_equal(_bits(after[slots[2]][k]), _bits(m)), (slots[0], k)
            assert np.array_equal(_bits(after[slots[3]][k]), _bits(v)), (slots[0], k)
            assert np.array_equal(_bits(after[slots[1]][k]), _bits(after[slots[0]][k] if period == 1 else before[slots[1]][k])), (slots[1], k)
            assert not np.array_equal(after[slots[0]][k], before[slots[0]][k])
    assert np.array_equal(after["beta_pow"], bp) and after["updates"] == 1
    gpu_ctx.check_error()


# ---- 4: acting -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ci", [1, 2])
def test_gpu_acting(ci, gpu_ctx, restore_settings):
    """act(noisy=False) is the mean network -- a plain learner's act on the same parameters, bit for bit -- and moves no counter; act() draws: its
    expected values are the twin's on the debug-read effective network under the parity rule, the action their first maximum, only the acting-draw
    counter advances, and two calls in a row draw differently."""
    capi = _capi()
    import torch
    shape, head, cfg, params, replay = _problem(ci, 480 + ci)
    n_obs, h1, A, K, B = shape
    L = _learner(gpu_ctx, head, cfg, params, replay)
    Pl = _learner(gpu_ctx, head, random_problem(head, shape, 480 + ci)[0], params)
    n = 37
    obs = _dev(np.random.default_rng(5).normal(size=(n, n_obs)).astype(np.float32))
    cn0 = L.state_dict()["counters"].copy()
    qm, qp = (torch.zeros(n, A, dtype=torch.float32, device="cuda") for _ in range(2))
    am, ap = L.act(obs, noisy=False, debug_q=qm).clone(), Pl.act(obs, debug_q=qp).clone()
    assert torch.equal(am, ap) and np.array_equal(_bits(qm.cpu().numpy()), _bits(qp.cpu().numpy()))
    assert np.array_equal(L.state_dict()["counters"], cn0)
    with pytest.raises(ValueError, match="noisy=True"):
        Pl.act(obs, noisy=True)
    seen = []
    for call in range(2):
        qn = torch.zeros(n, A, dtype=torch.float32, device="cuda")
        a = L.act(obs, debug_q=qn).cpu().numpy()
        cn = L.state_dict()["counters"]
        assert cn[capi.NOISY_DRAWS] == call + 1 and np.array_equal(np.delete(cn, capi.NOISY_DRAWS), np.delete(cn0, capi.NOISY_DRAWS))
        eff = L.effective("act")
        ev = expected_values_host(dict(params["q"], **eff), obs.cpu().numpy(), cfg)
        assert _check_4x("c51 noisy %s act %d" % (shape, call), qn.cpu().numpy(), ev["float32"], ev["float64"])
        assert np.array_equal(a, np.argmax(qn.cpu().numpy(), 1))    # (the first maximum of the float32 values a caller sees)
        top = np.sort(ev["float64"], 1)
        clear = top[:, -1] - top[:, -2] > 1e-4 * np.abs(ev["float64"]).max()
        assert clear.any() and np.array_equal(a[clear], np.argmax(ev["float64"], 1)[clear])
        seen.append((np.concatenate(L.noise("act")), qn.cpu().numpy()))
    assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1]) and not np.array_equal(seen[0][1], qm.cpu().numpy())
    gpu_ctx.check_error()


# ---- 5: evaluations and round trips ---------------------------------------------------------------------------------------------------------------------
def _snap(L):
    sd = L.state_dict()
    return sd["params"], sd["counters"]


def _same(a, b, label, draws=True):
    capi = _capi()
    (pa, ca), (pb, cb) = a, b
    for slots, names in ((Q_SLOTS, NAMES), (SIGMA, SNAMES)):
        for s in slots:
            for k in names:
                assert np.array_equal(_bits(pa[s][k]), _bits(pb[s][k])), (label, s, k)
    assert np.array_equal(_bits(pa["beta_pow"]), _bits(pb["beta_pow"])), label
    keep = slice(None) if draws else [i for i in range(len(ca)) if i != capi.NOISY_DRAWS]
    assert np.array_equal(ca[keep], cb[keep]), (label, ca, cb)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["uniform", "per", "n_step"])
def test_gpu_evaluation_and_state_round_trip(variant, gpu_ctx, restore_settings):
    """At the second shape: a run with an evaluation in its middle (a noisy and a mean acting call) ends on the bits of a run that never acted, but
    for the acting-draw counter; a state saved mid-run and loaded into a learner that was set back to its fresh state over the same ring continues bit-identically.  Once each
    with prioritised replay and with n_step = 3."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    kw = dict(target_period=3)
    if variant == "per":
        kw["per"] = learner.PERConfig(alpha=0.6, beta=0.4)
    if variant == "n_step":
        kw["n_step"] = 3
    shape, head, cfg, params, replay = _problem(1, 500, **kw)
    mk = lambda: _learner(gpu_ctx, head, _problem(1, 500, **kw)[2], params, rows_per_push=32)
    obs = _dev(np.random.default_rng(6).normal(size=(9, shape[0])).astype(np.float32))
    A_, B_, C_ = mk(), mk(), mk()
    for X in (A_, B_, C_):
        _fill(X, replay, chunk=32)
    fresh = C_.state_dict()
    A_.update(2); B_.update(2); C_.update(2)                        # (C_ too: the ring's priorities are no part of a state)
    _same(_snap(A_), _snap(B_), "two updates")
    mid = A_.state_dict()
    assert mid["noisy"] is True and set(SIGMA) <= set(mid["params"])
    A_.act(obs); A_.act(obs, noisy=False); A_.act(obs)
    A_.update(2); B_.update(2)
    _same(_snap(A_), _snap(B_), "an evaluation in the middle", draws=False)
    assert _snap(A_)[1][5] == 2 and _snap(B_)[1][5] == 0
    assert not np.array_equal(_snap(A_)[0]["sigma"]["w1"], mid["params"]["sigma"]["w1"])
    C_.load_state_dict(fresh)
    _same(_snap(C_), (fresh["params"], fresh["counters"]), "loaded the fresh state")
    assert not np.array_equal(_snap(C_)[0]["sigma"]["w1"], mid["params"]["sigma"]["w1"])
    C_.load_state_dict(mid)
    _same(_snap(C_), (mid["params"], mid["counters"]), "loaded")
    C_.update(2)
    _same(_snap(C_), _snap(B_), "continued from the saved state")
    gpu_ctx.check_error()


# ---- 6: training -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_train_dqn_explores_through_the_noise(gpu_ctx, restore_settings, tmp_path):
    """train_dqn on sumo-jerk-v0 with a noisy dueling learner for 640 frames: it runs, epsilon is 0 (no exploring acting call is counted), every step
    took an acting draw, sigma has moved, and export_q writes the mean network with the ``noisy`` key."""
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(64, env_id="sumo-jerk-v0", seed=2, ctx=gpu_ctx)
    cfg = learner.C51Config(n_obs=env.obs_dim, h1=32, batch=50, capacity=256, replay_start=100, target_period=5, n_atoms=21, dueling=True, noisy=learner.NoisyConfig())
    L = learner.C51Learner(env, cfg, seed=6)
    first = L.state_dict()["params"]
    res = learner.train_dqn(env, L, 640, updates_per_step=2, drain_every=4)
    env.check_error()
    st, sd = L.stats(), L.state_dict()
    assert res["steps"] == 10 and st["updates"] == 18 and np.isfinite(st["loss"]) and st["loss"] > 0
    assert sd["counters"][3] == 0 and sd["counters"][5] == 10 and sd["counters"][4] == 640
    assert all(np.isfinite(sd["params"][s][k]).all() for s in SIGMA for k in SNAMES)
    assert not np.array_equal(sd["params"]["sigma"]["w1"], first["sigma"]["w1"]) and not np.array_equal(sd["params"]["sigma"]["b1"], first["sigma"]["b1"])
    assert not np.array_equal(sd["params"]["q"]["w1"], first["q"]["w1"])
    with np.load(L.export_q(str(tmp_path / "noisy.npz"))) as z:
        assert int(z["noisy"]) == 1 and all(np.array_equal(z[k], sd["params"]["q"][k]) for k in NAMES)


# ---- 7: the mean network is what a policy evaluates ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ci", [1, 3])
def test_gpu_mean_acting_equals_the_c51_actor_view(ci, gpu_ctx, restore_settings):
    """act(noisy=False) on a noisy learner equals actor.C51Actor.from_learner on the same input vectors, actions and expected values bit for bit,
    and moves no counter -- before anything ran, and again after a noisy act() and an update (the view reads mu, not a shadow buffer; the values
    have moved with mu)."""
    _capi()
    import torch
    from discrete_testlib import policy_states, run_policy, widen
    from rl_mpc_lanemerging_amd import actor
    shape, head, cfg, params, replay = _problem(ci, 520 + ci)
    n_obs, h1, A, K, B = shape
    L = _learner(gpu_ctx, head, cfg, params, replay)
    n = 33
    S, st = policy_states(n)
    P = widen(actor.C51Actor.from_learner(L, n, gpu_ctx, S))
    seen = []
    for stage in range(2):
        got = run_policy(P, st)
        cn0 = L.state_dict()["counters"].copy()
        q = torch.zeros(n, A, dtype=torch.float32, device="cuda")
        a = L.act(P.feat[:n], noisy=False, debug_q=q).cpu().numpy()
        assert np.array_equal(_bits(got["q"]), _bits(q.cpu().numpy())) and np.array_equal(got["action"], a), stage
        assert np.array_equal(L.state_dict()["counters"], cn0)
        qn = torch.zeros(n, A, dtype=torch.float32, device="cuda")
        L.act(P.feat[:n], debug_q=qn)                               # a noisy call: other values, and the view's stay
        assert not np.array_equal(qn.cpu().numpy(), got["q"])
        again = run_policy(P, st)
        assert np.array_equal(_bits(again["q"]), _bits(got["q"])) and np.array_equal(again["action"], got["action"])
        seen.append(got["q"])
        L.update(1)
    assert not np.array_equal(seen[0], seen[1])
    gpu_ctx.check_error()


# ---- 8: the library's refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_library_refusals(gpu_ctx, restore_settings):
    """stmpc_noisy_c51_enable refuses a bad sigma0, a second enable, a learner that has pushed or updated and a population's member (naming the
    population's entry); the other entries refuse a plain learner; the population's enable refuses a wrong count, a bad sigma0 and a second call."""
    capi = _capi()
    from discrete_testlib import stub_env
    from rl_mpc_lanemerging_amd import learner
    shape, head = CASES[1]
    n_obs, h1, A, K, B = shape
    plain_cfg, params, replay = random_problem(head, shape, 540)
    Pl = _learner(gpu_ctx, head, plain_cfg, params)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(capi.StmpcError, match="sigma0 must be finite and not negative"):
            gpu_ctx.noisy_c51_enable(Pl.handle, bad)
    for call in (lambda: gpu_ctx.noisy_c51_get_params(Pl.handle, 0, h1 * A * K + A * K), lambda: gpu_ctx.noisy_c51_set_params(Pl.handle, 0, np.zeros(h1 * A * K + A * K)),
                 lambda: gpu_ctx.noisy_c51_debug_read(Pl.handle, 0, h1 + A * K), lambda: gpu_ctx.noisy_c51_act(Pl.handle, 1, 0, n_obs, 0.0, 0)):
        with pytest.raises(capi.StmpcError, match="not enabled on this learner"):
            call()
    gpu_ctx.noisy_c51_enable(Pl.handle, 0.5)                        # (fresh: nothing pushed, no update)
    with pytest.raises(capi.StmpcError, match="already enabled"):
        gpu_ctx.noisy_c51_enable(Pl.handle, 0.5)
    with pytest.raises(capi.StmpcError, match="count is not"):
        gpu_ctx.noisy_c51_get_params(Pl.handle, 0, 3)
    with pytest.raises(capi.StmpcError, match="slot out of range"):
        gpu_ctx.noisy_c51_get_params(Pl.handle, 4, h1 * A * K + A * K)
    pushed = _learner(gpu_ctx, head, random_problem(head, shape, 540)[0], params, replay)
    with pytest.raises(capi.StmpcError, match="fresh learner only"):
        gpu_ctx.noisy_c51_enable(pushed.handle, 0.5)
    pushed.update(1)
    with pytest.raises(capi.StmpcError, match="fresh learner only"):
        gpu_ctx.noisy_c51_enable(pushed.handle, 0.5)
    # a noisy learner's set_state refuses a negative acting-draw counter before it writes anything
    N = _learner(gpu_ctx, head, _problem(1, 540)[2], params, replay)
    N.update(1); N.act(_dev(np.zeros((3, n_obs), dtype=np.float32)))
    cn, bp = gpu_ctx.c51_get_state(N.handle)
    bad = cn.copy(); bad[2], bad[capi.NOISY_DRAWS] = 7, -1
    with pytest.raises(capi.StmpcError, match="counters out of range"):
        gpu_ctx.c51_set_state(N.handle, bad, bp)
    assert np.array_equal(gpu_ctx.c51_get_state(N.handle)[0], cn) and cn[capi.NOISY_DRAWS] == 1 and cn[2] == 1
    # populations
    env = stub_env(gpu_ctx, 32, n_obs, A)
    pop = learner.C51Population(env, [head.cfg(shape, m, capacity=RING) for m in range(2)])
    with pytest.raises(capi.StmpcError, match="stmpc_pop_noisy_c51_enable"):
        gpu_ctx.noisy_c51_enable(pop.member(0).handle, 0.5)
    with pytest.raises(capi.StmpcError, match="not enabled on this population"):
        gpu_ctx.c51_pop_noisy_act(pop.handle, 16, 0, n_obs, [0.0, 0.0], 0)
    with pytest.raises(capi.StmpcError, match="3 entries, the population 2 members"):
        gpu_ctx.c51_pop_noisy_enable(pop.handle, [0.5, 0.5, 0.5])
    with pytest.raises(capi.StmpcError, match="member 1's sigma0"):
        gpu_ctx.c51_pop_noisy_enable(pop.handle, [0.5, -1.0])
    gpu_ctx.c51_pop_noisy_enable(pop.handle, [0.5, 0.0])
    with pytest.raises(capi.StmpcError, match="already enabled on this population"):
        gpu_ctx.c51_pop_noisy_enable(pop.handle, [0.5, 0.0])
    gpu_ctx.check_error()


# ---- 9: a population ------------------------------------------------------------------------------------------------------------------------------------------
POP_SEEDS, POP_SIGMA0, POP_N = (3, 5, 9), (0.5, 0.0, 0.25), 16


def _pop_cfg(head, shape, m, **kw):
    from discrete_testlib import LR
    return head.cfg(shape, m, capacity=RING, lr=LR[m], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("ci", [0, 1])
def test_gpu_population_members_equal_lone_learners(ci, per, gpu_ctx, restore_settings):
    """P = 3 members that differ in seed, sigma0 (one of them 0), gamma, target_period, double and support, against three lone noisy learners fed the
    same transitions: after the pushes and after each of four updates with a noisy acting call in between, every slot, sigma slot, beta power and
    counter of member m equals the lone learner's bit for bit, and so do the actions.  A member's bits do not depend on its neighbours: member 0
    of a population of two with another neighbour ends on the same bits.  ``per``: once with prioritised members."""
    _capi()
    from discrete_testlib import feed, stub_env, syn_steps
    from rl_mpc_lanemerging_amd import learner
    shape, head = CASES[ci]
    n_obs, h1, A, K, B = shape
    n, P = POP_N, 3
    pk = learner.PERConfig(alpha=0.6, beta=0.4) if per else None
    noisy = [learner.NoisyConfig(s) for s in POP_SIGMA0]
    pop = learner.C51Population(stub_env(gpu_ctx, P * n, n_obs, A), [_pop_cfg(head, shape, m) for m in range(P)], seeds=POP_SEEDS, noisy=noisy, per=pk)
    pop2 = learner.C51Population(stub_env(gpu_ctx, 2 * n, n_obs, A), [_pop_cfg(head, shape, m) for m in (0, 2)], seeds=[POP_SEEDS[0], POP_SEEDS[2]],
                                 noisy=[noisy[0], noisy[2]], per=pk)
    lone = [learner.C51Learner(stub_env(gpu_ctx, n, n_obs, A), _pop_cfg(head, shape, m, noisy=noisy[m], per=pk), seed=POP_SEEDS[m]) for m in range(P)]
    assert pop.noisy and all(pop.member(m).noisy and pop.member(m).cfg.noisy.sigma0 == POP_SIGMA0[m] for m in range(P))
    steps = syn_steps(head, shape, P, 4, n, draw_all=True)
    for s in steps:
        feed(pop, s); feed(pop2, s, slice(0, 2 * n))
        for m in range(P):
            feed(lone[m], s, slice(m * n, (m + 1) * n))
    obs = _dev(steps[0]["obs"])
    for u in range(4):
        for m in range(P):
            _same(_snap(pop.member(m)), _snap(lone[m]), "member %d before update %d" % (m, u))
        _same(_snap(pop2.member(0)), _snap(lone[0]), "member 0 with another neighbour, before update %d" % u)
        a = pop.act(obs).cpu().numpy()
        a2 = pop2.act(obs[:2 * n]).cpu().numpy()
        for m in range(P):
            assert np.array_equal(a[m * n:(m + 1) * n], lone[m].act(obs[m * n:(m + 1) * n]).cpu().numpy()), (u, m)
        assert np.array_equal(a2[:n], a[:n])
        pop.update(1); pop2.update(1)
        for L in lone:
            L.update(1)
    for m in range(P):
        _same(_snap(pop.member(m)), _snap(lone[m]), "member %d at the end" % m)
        assert _snap(lone[m])[1][2] == 4 and _snap(lone[m])[1][5] == 4
        f_m, f_l = pop.member(m).noise("online"), lone[m].noise("online")
        assert np.array_equal(_bits(f_m[0]), _bits(f_l[0])) and np.array_equal(_bits(f_m[1]), _bits(f_l[1]))
    sd = _snap(lone[1])[0]
    assert np.abs(sd["sigma"]["w1"]).max() > 0                      # (sigma0 = 0 starts at the mean network and learns)
    st = pop.stats()
    assert list(st["updates"]) == [4] * P and np.isfinite(st["loss"]).all()
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_train_dqn_takes_a_noisy_population(gpu_ctx, restore_settings):
    """train_dqn on sumo-jerk-v0 with a noisy population of two: epsilon is 0 for both, every step took an acting draw per member, sigma has moved."""
    _capi()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(64, env_id="sumo-jerk-v0", seed=2, ctx=gpu_ctx)
    cfgs = [learner.C51Config(n_obs=env.obs_dim, h1=32, batch=50, capacity=256, replay_start=20, target_period=5, n_atoms=21) for _ in range(2)]
    pop = learner.C51Population(env, cfgs, seeds=[6, 7], noisy=[learner.NoisyConfig(0.5), learner.NoisyConfig(0.1)])
    first = [pop.member(m).state_dict()["params"] for m in range(2)]
    res = learner.train_dqn(env, pop, 640, updates_per_step=2, drain_every=4)
    env.check_error()
    assert res["steps"] == 10 and len(res["member_returns"]) == 2
    for m in range(2):
        sd = pop.member(m).state_dict()
        assert sd["counters"][3] == 0 and sd["counters"][5] == 10 and sd["counters"][4] == 320 and sd["params"]["updates"] == 20
        assert not np.array_equal(sd["params"]["sigma"]["w1"], first[m]["sigma"]["w1"]) and np.isfinite(sd["params"]["sigma"]["w1"]).all()
