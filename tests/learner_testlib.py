"""What more than one learner test module uses (DDPG, TD3, DQN, their populations, prioritised replay), each defined once.  Plain functions and
constants: no fixtures, no hooks, nothing heavy at import time -- the package is imported, and its library built, inside the functions.  What is
not about the learner (the binding, bit comparisons, the header, the actor population's steps) is in stmpc_testlib.py.  Import what a module
needs, e.g. ``from learner_testlib import SEED, check_4x as _check_4x, push as _push``.

The parity rule of the floating-point GPU tests: error = max-abs difference to the float64 twin divided by the float64 tensor's max-abs;
bound = 4 x the same error of the float32 twin on the CPU, floor 8 float32 ulps.  The yardstick is the torch float32 twin, never the kernel;
4 covers two float32 evaluations with different summation orders.  ``bound_4x`` is its one definition.
"""
import os
import types

import numpy as np

from stmpc_testlib import REPO, bits, capi, record_json

# ---- the parity rule ---------------------------------------------------------------------------------------------------------------------------
FLOOR = 8 * 2.0 ** -23          # 8 float32 ulps, relative


def rel_err(x, ref):
    scale = np.abs(ref).max()
    return float(np.abs(np.asarray(x, dtype=np.float64) - ref).max() / scale) if scale > 0 else float(np.abs(x).max())


def bound_4x(e_32):
    """The bound on an error whose float32 twin's is ``e_32``."""
    return max(4 * e_32, FLOOR)


def check_4x(label, dev, f32, f64, ratios=None):
    """The parity rule for one tensor; prints (and, given ``ratios``, records there) before the caller asserts."""
    e_dev, e_32 = rel_err(dev, f64), rel_err(f32, f64)
    bound = bound_4x(e_32)
    if ratios is not None:
        ratios[label] = {"device": e_dev, "float32_twin": e_32, "ratio": e_dev / e_32 if e_32 > 0 else None}
    print("%-40s device %.3e  float32 twin %.3e  bound %.3e" % (label, e_dev, e_32, bound))
    return e_dev <= bound


def record(key, value):
    """Merge one entry into profiles/learner/parity.json (evidence; the assertions are in the tests)."""
    record_json(os.path.join(REPO, "profiles", "learner", "parity.json"), key, value)


# ---- bit comparisons ---------------------------------------------------------------------------------------------------------------------------
# All of them compare integer views: +0.0 differs from -0.0, and a NaN equals the NaN with the same bits.  ``bits`` (stmpc_testlib) views an
# array's own 4- or 8-byte words.  ``bits64`` converts to float64 first: it is for the sum trees, which are float64 on both sides but may come as
# lists or float32 leaves on one -- the two are not interchangeable, so both stay.
def bits64(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def bits_equal(a, b, slots, names=None):
    """Slot by slot, tensor by tensor (``names``: learner.TENSORS unless given), as float32 words."""
    from rl_mpc_lanemerging_amd import learner
    names = learner.TENSORS if names is None else names
    return all(np.array_equal(np.asarray(a[s][k], np.float32).view(np.uint32), np.asarray(b[s][k], np.float32).view(np.uint32)) for s in slots for k in names)


def capi_slots():
    return capi().DDPG_SLOTS


# ---- exact-arithmetic DDPG problems (asserted exact by test_net_shapes_cpu.py) ---------------------------------------------------------------------
# name -> (n_obs, h1, h2); what each reaches is in DESIGN.md section 12
SHAPES = {"one-tile": (5, 16, 16), "padded": (20, 40, 24), "mixed-k": (30, 96, 48), "wide-h2": (1, 176, 208), "over-64K": (20, 512, 512)}
BATCHES = (16, 64, 256)
EXACT_CASES = [(s, B) for s in ("one-tile", "padded", "mixed-k", "wide-h2") for B in BATCHES] + [("over-64K", 16)]
SEED = 17                       # the learner's seed: it draws the minibatch rows
REPLAY_ROWS = 320
TIME_SCALE = 0.25               # time feature = 0.25 x ticks: a multiple of 1/4 like the observations (the shipped 0.001 is no dyadic number)


def _sparse_rows(rng, rows, cols, nnz, values, distinct=False):
    """[rows][cols] with ``nnz`` entries per row drawn from ``values`` (none of them 0) at random columns; ``distinct``: no two rows equal."""
    nnz = min(nnz, cols)
    w = np.zeros((rows, cols), dtype=np.float32)
    seen = set()
    for n in range(rows):
        while True:
            row = np.zeros(cols, dtype=np.float32)
            row[rng.choice(cols, nnz, replace=False)] = rng.choice(values, nnz)
            if not distinct or row.tobytes() not in seen:
                break
        seen.add(row.tobytes())
        w[n] = row
    return w


def dyadic_net(rng, n_in, h1, h2, out_scale):
    """One network of the value sets ``dyadic_problem`` documents; ``out_scale`` (a power of two) scales the last layer."""
    half = np.array([-1.0, -0.5, 0.5, 1.0], dtype=np.float32)
    w2 = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (1, h2))
    w2[0, rng.random(h2) < 0.125] = 0.0
    return {"w0": _sparse_rows(rng, h1, n_in, 3, half), "b0": rng.choice(np.array([-0.5, 0.0, 0.5], dtype=np.float32), h1),
            "w1": _sparse_rows(rng, h2, h1, 3, half, distinct=True), "b1": rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), h2),
            "w2": (w2 * np.float32(out_scale)).astype(np.float32), "b2": np.array([0.5 * out_scale], dtype=np.float32)}


def dyadic_problem(shape, B, rng):
    """(cfg, params, replay) for ``shape`` = (n_obs, h1, h2) (or a name of SHAPES) and minibatch size ``B`` (a power of two).

    Value sets (tuned on the CPU until ``exactness_bits`` stayed below 24 for every case of EXACT_CASES):
      observations, next observations, actions   multiples of 1/4 in [-1, 1]
      time feature                               0.25 x ticks, ticks in 0 ... 4 (cfg.time_scale = 0.25)
      rewards                                    multiples of 1/4 in [-2, 2]
      W0, W1                                     three entries of {-1, -1/2, 1/2, 1} per row, the rest 0 (sparse rows keep the sums short); the rows of
                                                 W1 are pairwise different
      b0 in {-1/2, 0, 1/2}, b1 in {0, 1/2, 1}    (b1 >= 0 keeps most second-layer units alive)
      W2                                         -1 or +1, one in eight 0; the actor's scaled by a power of two so that tanh is not saturated
      b2                                         1/2 (times the same power of two)
      gamma = 0                                  y = r: the critic's gradient does not see the target networks (they get values of the same sets)
      dz = 2 (Q - r) / B                         exact because B is a power of two
    The products are then multiples of 2^-3 (layer 0), 2^-5 (layer 1, Q), 2^-(4 + log2 B) (dz) ... 2^-(9 + log2 B) (dW1).  Largest width reached
    over EXACT_CASES: 20.4 bits, in dW2 of mixed-k at B = 256 (printed by test_every_partial_sum_fits_float32); 24 is float32's.
    ``replay``: REPLAY_ROWS transitions as ``DDPGLearner.push`` takes them (numpy)."""
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape] if isinstance(shape, str) else shape
    assert B & (B - 1) == 0
    cfg = learner.DDPGConfig(n_obs=n_obs, h1=h1, h2=h2, batch=B, capacity=512, replay_start=0, gamma=0.0, time_scale=TIME_SCALE, lr_q=1e-3, lr_pi=5e-4,
                             action_low=-5.0, action_high=5.0)
    a_scale = 2.0 ** -int(round(np.log2(np.sqrt(1.5 * h2))))
    params = learner.new_params(dyadic_net(rng, n_obs + 1, h1, h2, a_scale), dyadic_net(rng, n_obs + 2, h1, h2, 1.0))
    params["actor_target"] = {k: v.copy() for k, v in dyadic_net(rng, n_obs + 1, h1, h2, a_scale).items()}
    params["critic_target"] = {k: v.copy() for k, v in dyadic_net(rng, n_obs + 2, h1, h2, 1.0).items()}
    quarter = lambda lo, hi, *sh: (rng.integers(4 * lo, 4 * hi + 1, sh) / 4.0)
    R = REPLAY_ROWS
    kind = rng.integers(0, 4, R)                                  # 0, 1: neither; 2: terminated; 3: truncated
    replay = {"obs": quarter(-1, 1, R, n_obs).astype(np.float32), "next_obs": quarter(-1, 1, R, n_obs).astype(np.float32),
              "ticks": rng.integers(0, 4, R).astype(np.int32), "action": quarter(-1, 1, R), "reward": quarter(-2, 2, R), "terminated": kind == 2,
              "truncated": kind == 3}
    return cfg, params, replay


def replay_rows_host(replay, cfg):
    """The ring rows k_replay_push writes for ``replay`` pushed into an empty ring (test_gpu_replay_ring_equals_a_numpy_ring's twin; no final_obs,
    no next_ticks: s' is next_obs at ticks + 1)."""
    n_obs, R = cfg.n_obs, len(replay["ticks"])
    ts = np.float32(cfg.time_scale)
    rows = np.zeros((R, capi().DDPG_ROW), dtype=np.float32)
    rows[:, :n_obs], rows[:, n_obs], rows[:, n_obs + 1] = replay["obs"], ts * replay["ticks"].astype(np.float32), replay["action"].astype(np.float32)
    rows[:, 32:32 + n_obs], rows[:, 32 + n_obs] = replay["next_obs"], ts * (replay["ticks"] + 1).astype(np.float32)
    rows[:, 64], rows[:, 65] = replay["reward"].astype(np.float32), np.where(replay["terminated"], 0, 1)
    return rows


def host_minibatch(replay, cfg, update=0, seed=SEED):
    """(rows [B][68], the minibatch dict of update_host) the learner with ``seed`` samples at update index ``update`` from ``replay`` pushed into
    an empty ring."""
    from rl_mpc_lanemerging_amd import learner
    rows = replay_rows_host(replay, cfg)
    rows = rows[learner.sample_indices_host(seed, update, cfg.batch, rows.shape[0])]
    return rows, learner.batch_from_rows(rows, cfg.n_obs)


minibatch_host = host_minibatch     # (the TD3 tests' name for it: their copy had the same body)


def forward_host(net, x, dtype):
    """A plain numpy forward pass in ``dtype``: (H1, H2, z) -- hidden activations and the pre-tanh output."""
    f = lambda a: np.asarray(a, dtype=dtype)
    h1 = np.maximum(f(x) @ f(net["w0"]).T + f(net["b0"]), 0)
    h2 = np.maximum(h1 @ f(net["w1"]).T + f(net["b1"]), 0)
    return h1, h2, (h2 @ f(net["w2"]).T + f(net["b2"]))[:, 0]


def frac_bits(a):
    """Smallest e such that every entry of ``a`` is a multiple of 2^-e."""
    a = np.asarray(a, dtype=np.float64)
    for e in range(-8, 64):
        if np.array_equal(a * 2.0 ** e, np.round(a * 2.0 ** e)):
            return e
    raise AssertionError("not dyadic")


def exactness_bits(params, batch):
    """Per stage of the critic's forward pass, backward pass and weight gradients (and of the actor's forward pass): log2 of (the largest sum of
    |a| |b| over the summed index) / (the unit every product is a multiple of).  Below 24, every partial sum of every summation order is a float32
    number.  Computed in float64, which is exact as long as the result holds."""
    q, B = params["critic"], len(batch["r"])
    d = lambda a: np.asarray(a, dtype=np.float64)
    bits = {}

    def stage(name, a, b, bias=None):                             # a [m][k] @ b [k][n] (+ bias [n])
        a, b = d(a), d(b)
        e = frac_bits(a) + frac_bits(b)
        s = np.abs(a) @ np.abs(b)
        if bias is not None:
            e, s = max(e, frac_bits(bias)), s + np.abs(d(bias))
        bits[name] = float(np.log2(max(s.max(), 2.0 ** -e) * 2.0 ** e))

    x = np.concatenate([d(batch["s"]), d(batch["a"])[:, None]], 1)
    h1, h2, qv = forward_host(q, x, np.float64)
    stage("critic z1", x, d(q["w0"]).T, q["b0"])
    stage("critic z2", h1, d(q["w1"]).T, q["b1"])
    stage("critic Q", h2, d(q["w2"]).T, q["b2"])
    stage("Q - r", np.stack([qv, -d(batch["r"])], 1), np.ones((2, 1)))
    dz = 2.0 * (qv - d(batch["r"])) / B
    dz2 = dz[:, None] * d(q["w2"]) * (h2 > 0)
    stage("dZ2", np.abs(dz2).reshape(-1, 1), np.ones((1, 1)))
    stage("dZ1", dz2, d(q["w1"]))
    dz1 = (dz2 @ d(q["w1"])) * (h1 > 0)
    for name, left, right in (("dW1", dz2, h1), ("db1", dz2, np.ones((B, 1))), ("dW2", dz[:, None], h2), ("db2", dz[:, None], np.ones((B, 1))),
                              ("dW0", dz1, x), ("db0", dz1, np.ones((B, 1)))):
        stage(name, left.T, right)
    for slot in ("actor", "actor_target"):
        a = params[slot]
        xs = d(batch["s"] if slot == "actor" else batch["s2"])
        g1, g2, _ = forward_host(a, xs, np.float64)
        stage(slot + " z1", xs, d(a["w0"]).T, a["b0"])
        stage(slot + " z2", g1, d(a["w1"]).T, a["b1"])
        stage(slot + " z", g2, d(a["w2"]).T, a["b2"])
    return bits


def problem(shape, B):
    """The problem of one case: the same for the CPU and the GPU tests (one generator seed per case)."""
    return dyadic_problem(shape, B, np.random.default_rng(1000 + 7 * list(SHAPES).index(shape) + B))


# ---- ordinary floating-point problems ------------------------------------------------------------------------------------------------------------
def random_problem(rng, B=48, n_obs=20, h1=40, h2=24):
    """(cfg, params, one minibatch) of a DDPG learner: random float32 nets, targets that differ from them."""
    from rl_mpc_lanemerging_amd import learner
    cfg = learner.DDPGConfig(n_obs=n_obs, h1=h1, h2=h2, batch=B, lr_q=1e-3, lr_pi=5e-4)
    a_net, q_net = learner.init_net(n_obs + 1, h1, h2, rng), learner.init_net(n_obs + 2, h1, h2, rng)
    a_net["w2"] = rng.normal(0, 0.1, a_net["w2"].shape).astype(np.float32)
    q_net["w2"] = rng.normal(0, 0.1, q_net["w2"].shape).astype(np.float32)
    params = learner.new_params(a_net, q_net)
    for k in learner.TENSORS:                                     # targets that differ from the online nets
        params["actor_target"][k] = params["actor_target"][k] + rng.normal(0, 0.01, params["actor_target"][k].shape).astype(np.float32)
        params["critic_target"][k] = params["critic_target"][k] + rng.normal(0, 0.01, params["critic_target"][k].shape).astype(np.float32)
    batch = {"s": rng.normal(0, 1, (B, n_obs + 1)), "a": rng.uniform(-5, 5, B), "r": rng.normal(0, 1, B), "s2": rng.normal(0, 1, (B, n_obs + 1)),
             "mask": (rng.random(B) > 0.2).astype(np.float64)}
    return cfg, params, batch


# ---- TD3 problems (asserted by test_td3_cpu.py) ------------------------------------------------------------------------------------------------------
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
    """(cfg, params, replay): ``dyadic_problem`` with a second dyadic critic, dyadic target critics, a target actor whose last layer is zero
    (a' = tanh_mean exactly) and gamma in {0.5, 1}.  One generator seed per case, chosen so that the minibatch of update 0 has rows with Qt1 < Qt2,
    rows with Qt2 < Qt1 and both values of mask (asserted by test_dyadic_twin_target_is_exact)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape]
    rng = np.random.default_rng(DYADIC_SEEDS[shape, B] if seed is None else seed)
    cfg, p, replay = dyadic_problem(shape, B, rng)
    cfg = td3_config(cfg, gamma=gamma, target_noise=0.0)
    replay = {k: v[:RING] for k, v in replay.items()}
    params = learner.new_params_td3(p["actor"], p["critic"], dyadic_net(rng, n_obs + 2, h1, h2, 1.0))
    params["actor_target"] = {k: v.copy() for k, v in p["actor_target"].items()}
    params["actor_target"]["w2"][:] = 0.0
    params["actor_target"]["b2"][:] = 0.0
    params["critic_target"] = {k: v.copy() for k, v in p["critic_target"].items()}
    params["critic2_target"] = {k: v.copy() for k, v in dyadic_net(rng, n_obs + 2, h1, h2, 1.0).items()}
    return cfg, params, replay


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


# ---- sum trees ---------------------------------------------------------------------------------------------------------------------------------
def tree_from_leaves(w):
    """The sum tree over leaf weights ``w`` (a power of two of them), every level summed from the one below: brute force, no incremental update."""
    w = np.asarray(w, dtype=np.float64)
    n = np.zeros(2 * w.size - 1)
    n[w.size - 1:] = w
    width = w.size // 2
    while width >= 1:
        n[width - 1:2 * width - 1] = n[2 * width - 1:4 * width - 1:2] + n[2 * width:4 * width:2]
        width //= 2
    return n


def internal_nodes_are_exact(nodes):
    leaves = (nodes.size + 1) // 2
    i = np.arange(leaves - 1)
    return bool(np.array_equal(nodes[i], nodes[2 * i + 1] + nodes[2 * i + 2]))


# ---- on the device -----------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def push(L, replay, rows=slice(None)):
    L.push(dev(replay["obs"][rows]), dev(replay["ticks"][rows]), dev(replay["action"][rows]), dev(replay["reward"][rows]), dev(replay["next_obs"][rows]),
           dev(replay["terminated"][rows]), dev(replay["truncated"][rows]))


def stub_env(gpu_ctx, n, n_obs=20):
    """What a population asks of an env, without one."""
    return types.SimpleNamespace(n=n, obs_dim=n_obs, continuous=True, ctx=gpu_ctx)


# ---- populations against their members run alone (test_learner_pop.py, test_td3_pop.py, test_per_pop.py, test_net_shapes.py) -------------------------
N_PER, CAP, STEPS = 24, 200, 12                # 24: an acting tile with masked tail rows; 200: every ring wraps within 9 pushes


def td3_init(shape, m):
    """Member m's starting networks as an (actor, critic, critic 2) triple: torch's initialisation with last layers that are not zero."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, h2 = SHAPES[shape] if isinstance(shape, str) else shape
    rng = np.random.default_rng(100 + m)
    nets = (learner.init_net(n_obs + 1, h1, h2, rng), learner.init_net(n_obs + 2, h1, h2, rng), learner.init_net(n_obs + 2, h1, h2, rng))
    for net in nets:
        net["w2"] = rng.normal(0, 0.05, (1, h2)).astype(np.float32)
    return nets


def snapshot(gpu_ctx, L, stats):
    sd = L.state_dict()
    return {"params": sd["params"], "counters": sd["counters"], "ring": gpu_ctx.ddpg_replay_read(L.handle, 0, CAP), "stats": stats}


def assert_same(a, b, label):
    """Two snapshots: the DDPG slots, all beta powers, counters, ring and statistics, bit for bit."""
    from rl_mpc_lanemerging_amd import _capi, learner
    for slot in _capi.DDPG_SLOTS:
        for k in learner.TENSORS:
            assert np.array_equal(bits(a["params"][slot][k]), bits(b["params"][slot][k])), (label, slot, k)
    assert np.array_equal(bits(a["params"]["beta_pow"]), bits(b["params"]["beta_pow"])), (label, "beta_pow")
    assert np.array_equal(a["counters"], b["counters"]), (label, a["counters"], b["counters"])
    assert np.array_equal(bits(a["ring"]), bits(b["ring"])), (label, "ring")
    assert np.array_equal(bits(np.array(a["stats"])), bits(np.array(b["stats"]))), (label, a["stats"], b["stats"])


def assert_same_td3(a, b, label):
    """``assert_same`` plus critic 2's four slots."""
    from rl_mpc_lanemerging_amd import learner
    assert_same(a, b, label)
    assert a["params"]["beta_pow"].shape == b["params"]["beta_pow"].shape == (6,)
    for slot in capi().TD3_SLOTS:
        for k in learner.TENSORS:
            assert np.array_equal(bits(a["params"][slot][k]), bits(b["params"][slot][k])), (label, slot, k)


def stats_row(s, m=None):
    keys = ("critic_loss", "critic2_loss", "mean_q", "mean_q2", "fill", "updates")
    return [float(s[k] if m is None else s[k][m]) for k in keys]
