"""DDPG learner on the device, next to ``vec_env.MergeVecEnv``: the reference's ``TRAIN_DDPG`` (ddpg.py:44-80: the ``all`` library's ``ddpg``
preset on ``sumo-jerk-continuous-v0``), whose product is the ``policy.pt`` / ``q.pt`` pairs under ``pretrained_models/``.

``DDPGLearner`` holds a replay ring filled from the env's step tensors, the actor and critic with their targets and Adam state, and runs the
update as six HIP launches (``csrc/stmpc_ddpg_kernels.hpp``); acting, pushing and updating never synchronise with the host.  ``export_actor``
writes the ``.npz`` that ``actor.load_weights`` / ``actor.DDPGActor`` / the combined controller read.  ``DDPGPopulation`` is P such learners
on slices of one env, advanced with one launch per kernel (``csrc/stmpc_ddpg_pop_kernels.hpp``): the reference's per-seed runs
(``train_{traffic_type}_{seed}.json``, pretrained_models/README.md) side by side, each member bit-identical to the run it would have had alone.

The ``all`` library (0.5.3, requirements.txt:10) is absent from the reference checkout: the update below restates its published DDPG with the
preset's documented constants as defaults (``DDPGConfig``); parity with the library itself is unpinned.  The network shapes are the reference's
own checkpoints': actor 21 -> 400 -> ReLU -> 300 -> ReLU -> 1 -> tanh * scale + mean, critic 22 -> 400 -> ReLU -> 300 -> ReLU -> 1 (20 observation
entries, the time feature 0.001 x ticks, the action).

Per update on a minibatch (s, a, r, s', mask), s including the time feature:
  1. y = r + gamma * mask * Q_target(s', pi_target(s')); mask = 0 where the episode terminated (a truncation keeps 1, s' = final_observation)
  2. critic: Adam step on mean((Q(s, a) - y)^2)
  3. actor: Adam step on -mean(Q(s, pi(s))) with the critic after step 2
  4. theta_target <- (1 - tau) theta_target + tau theta, both nets

Host twins (the suite's yardsticks, in the style of ``rewards.py``): ``update_host`` (torch autograd, float64 or float32), ``adam_host`` (numpy
float32 in the kernel's operation order), ``sample_indices_host``, ``noise_host``.

``TD3Learner`` (``TD3Config``, ``csrc/stmpc_td3_kernels.hpp``) is the same learner with TD3's three changes -- two critics and the minimum of their
targets, clipped noise on the target action, the actor and all targets stepped every ``policy_delay``-th update -- in six launches per update that
carry both critics in ``blockIdx.y``; twins: ``update_host_td3``, ``smoothing_noise_host``.  ``TD3Population`` is to it what ``DDPGPopulation`` is
to ``DDPGLearner`` (``csrc/stmpc_td3_pop_kernels.hpp``: the member axis in ``blockIdx.z``).

Prioritised replay (``DDPGConfig(per=PERConfig())``, ``csrc/stmpc_per_kernels.hpp``, ``stmpc_per_*``) is the reference's hand-written trainer's way of
drawing minibatches (dqn.py:267-349, ``SumTree`` dqn.py:727-794; ``USE_PRIORITIZED_ER = True`` in config.py) for ``DDPGLearner`` and ``TD3Learner``:
rows are drawn from a sum tree in proportion to ``min(|td| + min_priority, max_priority) ** alpha`` of their last critic error, new rows enter at
``max_priority ** alpha``, and the critic's loss carries the importance weights ``(fill * p / total) ** -beta`` over their largest (``beta`` 0, the
reference's: none).  Two launches more per update.  Twins: ``SumTreeHost``, ``per_sample_host``, ``per_priority_host``, ``per_weights_host`` and the
``weights=`` argument of ``update_host`` / ``update_host_td3``.  A population takes ``per=`` itself (``DDPGPopulation(..., per=...)``,
``TD3Population`` likewise; ``csrc/stmpc_per_pop_kernels.hpp``, ``stmpc_pop_per_*``): one ``PERConfig`` for all members or one per member, None for a
member that samples uniformly -- prioritised against uniform replay, or a sweep of alpha and beta, in one launch sequence of eight launches per update,
every member bit-identical to the lone learner with that ``cfg.per``.

``DQNLearner`` (``DQNConfig``, ``csrc/stmpc_dqn_kernels.hpp``, ``stmpc_dqn_*``) is the reference's other agent, the hand-written DQN trainer
(TRAIN_DQN: dqn.py:257-359, ``get_targets`` dqn.py:673-705, the ``DQN`` module dqn.py:566-658), for the discrete-action envs ``sumo-jerk-v0`` and
``sumo-accel-v0``: a Q-network n_obs -> h1 -> ReLU -> A on the same ring, counters and sum tree, double DQN targets, SmoothL1 loss, Adam, a hard
target copy every ``target_period`` updates -- three launches per update, five with ``per``.  Twins: ``update_host_dqn``, ``dqn_targets_host``,
``dqn_adam_host``, ``dqn_act_host``, ``dqn_epsilon``; the loop: ``train_dqn``.  ``DQNPopulation`` (``csrc/stmpc_dqn_pop_kernels.hpp``,
``stmpc_pop_dqn_*``) is to it what ``DDPGPopulation`` is to ``DDPGLearner``: P independent DQN learners on slices of one discrete env, the same
three (five) launches per update whatever P is, ``eps`` and ``lr`` per member, ``per=`` per member.

``C51Learner`` (``C51Config``, ``csrc/stmpc_c51_kernels.hpp``, ``stmpc_c51_*``) is the categorical head of the reference's third agent (rainbow.py, the
``all`` library's rainbow preset) on the DQN learner's ring: the network emits ``n_atoms`` logits per action, Q(s, a) is the mean of their softmax over
a fixed support, and the update minimises the cross-entropy against the projected Bellman-shifted target distribution (Bellemare et al. 2017,
Algorithm 1) -- three launches per update, five with ``per``; ``n_step`` as the DQN learner's.  Twins: ``c51_support``, ``c51_project_host``,
``c51_project_scatter_host``, ``c51_targets_host``, ``update_host_c51``; ``train_dqn`` takes it as it takes a ``DQNLearner``.  ``C51Population``
(``csrc/stmpc_c51_pop_kernels.hpp``, ``stmpc_pop_c51_*``) is to it what ``DQNPopulation`` is to ``DQNLearner``: P independent C51 learners -- the
support, ``double``, ``target_period``, ``gamma``, ``n_step``, the seed and ``per=`` per member -- for the launch count of one.
``C51Config(dueling=True)`` gives the learner, its population and ``actor.C51Actor`` the dueling head (Wang et al. 2016, in the categorical form of
Hessel et al. 2018): (A + 1) * n_atoms outputs, the value block last, logits V + Adv - mean Adv formed on the device behind every forward pass, a
dense backward, the same launch count.  It restates the published head; parity with the ``all`` library's own is not pinned.  Twins:
``_c51_logits(dueling=True)``, ``c51_dueling_combine_host`` (the device's operation order), ``c51_fold_dueling_host`` (the plain network with the same
logits).
``C51Config(noisy=NoisyConfig())`` gives the learner the sixth piece of the rainbow preset, the noisy output layer (Fortunato et al. 2018;
``csrc/stmpc_c51_noisy_kernels.hpp``, ``stmpc_noisy_c51_*``): W_eff = mu + sigma * outer(f(e_out), f(e_in)) on the layer h1 -> (A + dueling) * n_atoms,
the existing parameters being mu, a fresh draw per update and net and per acting call, Adam on sigma next to mu -- four launches per update, six with
``per``; ``train_dqn`` then explores through the noise (epsilon 0).  Twins: ``c51_noisy_f_host``, ``c51_noisy_compose_host``,
``update_host_c51_noisy``.  ``C51Population(..., noisy=)`` takes it as it takes ``per=`` -- one ``NoisyConfig`` for all members or one per member
(``sigma0`` may differ), all members on or all off (``stmpc_pop_noisy_c51_*``): four launches per update whatever P is, every member bit-identical
to the lone noisy learner.
"""
import math

import numpy as np

from . import _capi, actor as _actor
from .groups import splitmix64
from .config import Settings

TENSORS = ("w0", "b0", "w1", "b1", "w2", "b2")
_M64 = 0xFFFFFFFFFFFFFFFF
_G = 0x9E3779B97F4A7C15
NOISE_STREAM = 0x6E6F697365
TWO_PI_F32 = float(np.float32(6.2831855))


class PERConfig:
    """The constants of prioritised replay; defaults are the reference's (config.py: PER_ALPHA, PER_MIN_PRIORITY, PER_MAX_PRIORITY; no importance
    weights, so ``beta`` 0).  ``alpha`` 0.5 is a square root and 1 the identity on host and device alike; any other value goes through ``pow``."""

    def __init__(self, alpha=0.5, beta=0.0, min_priority=1e-6, max_priority=4.0):
        self.alpha, self.beta, self.min_priority, self.max_priority = float(alpha), float(beta), float(min_priority), float(max_priority)
        if not (self.min_priority > 0 and self.max_priority >= self.min_priority and self.alpha >= 0 and self.beta >= 0 and
                all(math.isfinite(x) for x in (self.alpha, self.beta, self.max_priority))):
            raise ValueError("prioritised replay needs min_priority > 0, max_priority >= min_priority, alpha >= 0 and beta >= 0, all finite")

    def to_c(self):
        return _capi.PERCfg(alpha=self.alpha, beta=self.beta, min_priority=self.min_priority, max_priority=self.max_priority)


def _check_n_step(n_step):
    n = int(n_step)
    if not 1 <= n <= _capi.NSTEP_MAX:
        raise ValueError("n_step must be in 1 ... %d, not %r" % (_capi.NSTEP_MAX, n_step))
    return n


def nstep_to_c(cfg, rows_per_push):
    """``stmpc_nstep_cfg`` of a learner's cfg and the rows N of every push; with ``cfg.n_step`` > 1 the window of n pushes must fit the ring."""
    N = int(rows_per_push or 0)
    if cfg.n_step > 1 and N < 1:
        raise ValueError("n_step = %d needs the rows of every push: an env, a population's n_per_member, or rows_per_push=" % cfg.n_step)
    if cfg.n_step > 1 and cfg.n_step * N > cfg.capacity:
        raise ValueError("n_step * rows_per_push = %d * %d does not fit the replay's capacity %d" % (cfg.n_step, N, cfg.capacity))
    return _capi.NStepCfg(n_step=cfg.n_step, rows_per_push=N if cfg.n_step > 1 else 0)


class DDPGConfig:
    """The constants of the update; defaults are the ``all`` ddpg preset's as its documentation gives them (``lr``: Settings.LEARNING_RATE).
    ``per``: a ``PERConfig`` for prioritised replay (None: uniform minibatches); it is not part of ``to_c`` -- the learner enables it on its handle."""

    def __init__(self, n_obs=20, h1=400, h2=300, batch=100, capacity=1000000, replay_start=5000, gamma=0.99, tau=0.005, lr_q=None, lr_pi=None,
                 beta1=0.9, beta2=0.999, eps=1e-8, time_scale=0.001, tanh_scale=None, tanh_mean=None, noise=0.1, action_low=None, action_high=None, per=None,
                 n_step=1):
        if per is not None and not isinstance(per, PERConfig):
            raise ValueError("per must be a PERConfig or None")
        self.per = per
        self.n_step = _check_n_step(n_step)                         # multi-step returns (``nstep_window_host``); like ``per`` it travels beside ``to_c``: ``to_c_nstep``
        lo = float(Settings.MINIMUM_NEGATIVE_JERK) if action_low is None else float(action_low)
        hi = float(Settings.MAXIMUM_POSITIVE_JERK) if action_high is None else float(action_high)
        self.n_obs, self.h1, self.h2, self.batch, self.capacity, self.replay_start = int(n_obs), int(h1), int(h2), int(batch), int(capacity), int(replay_start)
        self.gamma, self.tau, self.beta1, self.beta2, self.eps, self.time_scale = float(gamma), float(tau), float(beta1), float(beta2), float(eps), float(time_scale)
        self.lr_q = float(Settings.LEARNING_RATE if lr_q is None else lr_q)
        self.lr_pi = float(Settings.LEARNING_RATE if lr_pi is None else lr_pi)
        self.action_low, self.action_high = lo, hi
        self.tanh_scale = (hi - lo) / 2 if tanh_scale is None else float(tanh_scale)
        self.tanh_mean = (hi + lo) / 2 if tanh_mean is None else float(tanh_mean)
        self.noise_std = float(noise) * self.tanh_scale              # N(0, noise * tanh_scale), clipped to the Box

    def to_c(self, seed):
        return _capi.DDPGCfg(n_obs=self.n_obs, h1=self.h1, h2=self.h2, batch=self.batch, capacity=self.capacity, replay_start=self.replay_start,
                             seed=int(seed) & _M64, gamma=self.gamma, tau=self.tau, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                             time_scale=self.time_scale, tanh_scale=self.tanh_scale, tanh_mean=self.tanh_mean, noise_std=self.noise_std,
                             action_low=self.action_low, action_high=self.action_high)

    def to_c_nstep(self, rows_per_push):
        return nstep_to_c(self, rows_per_push)


# ---- the generator (host twins of dg_hash / stmpc_ddpg_sample_index / stmpc_ddpg_noise) ------------------------------------------------------
def hash3(seed, a, b):
    """splitmix64 of (seed, a, b): two rounds of the generator ``vec_env.episode_seed`` uses."""
    return splitmix64((splitmix64((int(seed) + _G * (int(a) + 1)) & _M64) + _G * (int(b) + 1)) & _M64)


def sample_indices_host(seed, update, batch, fill):
    """Ring rows of the ``batch`` minibatch rows of update ``update`` with ``fill`` rows filled: uniform, with replacement (int64 [batch])."""
    return np.array([hash3(seed, update, r) % int(fill) for r in range(int(batch))], dtype=np.int64)


def noise_host(seed, call, n, stream=NOISE_STREAM):
    """Noisy acting call ``call``, rows 0 .. n-1: (draw1, draw2, gauss) -- the two 24-bit draws (uint32) and Box-Muller on them in float64,
    cos taken at the float32 product 2 pi x draw2 / 2^24 the kernel forms.  ``stream``: the constant that keeps this use of the generator apart."""
    u1, u2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for e in range(n):
        h = hash3((int(seed) & _M64) ^ stream, call, e)
        u1[e], u2[e] = h >> 40, (h >> 8) & 0xFFFFFF
    f1 = (u1.astype(np.float64) + 1.0) * 2.0 ** -24
    theta = (np.float32(TWO_PI_F32) * (u2.astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float64)
    return u1, u2, np.sqrt(-2.0 * np.log(f1)) * np.cos(theta)


# ---- parameters --------------------------------------------------------------------------------------------------------------------------------
def flatten(net):
    """{w0, b0, w1, b1, w2, b2} -> the C-ABI's slot layout (float32)."""
    return np.concatenate([np.asarray(net[k], dtype=np.float32).reshape(-1) for k in TENSORS])


def unflatten(flat, n_in, h1, h2):
    shapes = ((h1, n_in), (h1,), (h2, h1), (h2,), (1, h2), (1,))
    out, o = {}, 0
    for k, sh in zip(TENSORS, shapes):
        n = int(np.prod(sh))
        out[k] = np.array(flat[o:o + n]).reshape(sh)
        o += n
    assert o == len(flat)
    return out


def init_net(n_in, h1, h2, rng):
    """torch's nn.Linear initialisation (uniform +-1/sqrt(fan_in) for weight and bias), the last layer zero (the ``all`` library's Linear0)."""
    u = lambda fan_in, *sh: rng.uniform(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in), size=sh).astype(np.float32)
    return {"w0": u(n_in, h1, n_in), "b0": u(n_in, h1), "w1": u(h1, h2, h1), "b1": u(h1, h2), "w2": np.zeros((1, h2), np.float32), "b2": np.zeros(1, np.float32)}


def zeros_like_net(net):
    return {k: np.zeros_like(np.asarray(net[k], dtype=np.float32)) for k in TENSORS}


def new_params(actor_net, critic_net):
    """The learner's whole parameter state for given online nets: targets = copies, Adam moments zero, beta powers 1, no updates."""
    cp = lambda n: {k: np.array(n[k], dtype=np.float32) for k in TENSORS}
    return {"actor": cp(actor_net), "actor_target": cp(actor_net), "actor_m": zeros_like_net(actor_net), "actor_v": zeros_like_net(actor_net),
            "critic": cp(critic_net), "critic_target": cp(critic_net), "critic_m": zeros_like_net(critic_net), "critic_v": zeros_like_net(critic_net),
            "beta_pow": np.ones(4, dtype=np.float32), "updates": 0}


def batch_from_rows(rows, n_obs):
    """Replay rows [B][68] -> the minibatch dict update_host takes (s, s2 include the time feature)."""
    ns = n_obs + 1
    return {"s": rows[:, :ns], "a": rows[:, ns], "s2": rows[:, 32:32 + ns], "r": rows[:, 64], "mask": rows[:, 65]}


# ---- the update on the host ------------------------------------------------------------------------------------------------------------------
def _mlp(t, x):
    import torch
    h = torch.relu(x @ t["w0"].T + t["b0"])
    h = torch.relu(h @ t["w1"].T + t["b1"])
    return (h @ t["w2"].T + t["b2"])[:, 0]


def _adam_step(P, name, grads, lr, t, cfg):
    """Adam step number ``t`` of net ``name`` of the torch parameter dict ``P`` (slots ``name``, ``name_m``, ``name_v``), bias-corrected."""
    bc1, bc2 = 1.0 - cfg.beta1 ** t, 1.0 - cfg.beta2 ** t
    for k in TENSORS:
        g, m, v = grads[k], P[name + "_m"][k], P[name + "_v"][k]
        m = cfg.beta1 * m + (1 - cfg.beta1) * g
        v = cfg.beta2 * v + (1 - cfg.beta2) * g * g
        P[name + "_m"][k], P[name + "_v"][k] = m, v
        P[name][k] = P[name][k] - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + cfg.eps)


def _polyak(P, name, cfg):
    for k in TENSORS:
        P[name + "_target"][k] = (1 - cfg.tau) * P[name + "_target"][k] + cfg.tau * P[name][k]


def update_host(params, batch, cfg, dtype="float64", lr_q=None, lr_pi=None, grads_only=False, weights=None, disc=None):
    """One update (steps 1-4 of the module text) in torch with autograd, every tensor in ``dtype`` ("float64" or "float32").
    ``params``: as ``new_params`` / ``DDPGLearner.state_dict()["params"]``; returns the new one (numpy arrays of ``dtype``) and a dict with
    ``critic_loss``, ``mean_q``, ``grad_critic``, ``grad_actor``.  ``grads_only``: nothing is applied and BOTH gradients are taken against the
    current critic (``stmpc_ddpg_grads_device``'s mode).  ``weights``: prioritised replay's importance weight per minibatch row, which multiplies
    that row's term of the critic's loss (None: none; ``critic_loss`` stays the unweighted mean, as the device reports it).  ``disc``: the
    target's discount per minibatch row in ``cfg.gamma``'s place (``nstep_batch_host``'s gamma^m; None: ``cfg.gamma``)."""
    import torch
    td = getattr(torch, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=td)
    P = {slot: {k: T(params[slot][k]) for k in TENSORS} for slot in _capi.DDPG_SLOTS}
    s, a, r, s2, mask = (T(batch[k]) for k in ("s", "a", "r", "s2", "mask"))
    scale, mean = cfg.tanh_scale, cfg.tanh_mean
    lr = {"critic": cfg.lr_q if lr_q is None else lr_q, "actor": cfg.lr_pi if lr_pi is None else lr_pi}
    t = int(params["updates"]) + 1

    def adam(name, grads):
        _adam_step(P, name, grads, lr[name], t, cfg)
        _polyak(P, name, cfg)

    with torch.no_grad():
        a2 = torch.tanh(_mlp(P["actor_target"], s2)) * scale + mean
        y = r + (cfg.gamma if disc is None else T(disc)) * mask * _mlp(P["critic_target"], torch.cat([s2, a2[:, None]], 1))
    crit = {k: P["critic"][k].clone().requires_grad_(True) for k in TENSORS}
    q = _mlp(crit, torch.cat([s, a[:, None]], 1))
    loss = ((q - y) ** 2).mean()
    gq = dict(zip(TENSORS, torch.autograd.grad(loss if weights is None else (T(weights) * (q - y) ** 2).mean(), [crit[k] for k in TENSORS])))
    if not grads_only:
        adam("critic", gq)
    act = {k: P["actor"][k].clone().requires_grad_(True) for k in TENSORS}
    pa = torch.tanh(_mlp(act, s)) * scale + mean
    aloss = -_mlp(P["critic"], torch.cat([s, pa[:, None]], 1)).mean()
    gp = dict(zip(TENSORS, torch.autograd.grad(aloss, [act[k] for k in TENSORS])))
    if not grads_only:
        adam("actor", gp)
    out = {slot: {k: P[slot][k].detach().numpy() for k in TENSORS} for slot in _capi.DDPG_SLOTS}
    out["beta_pow"] = np.array(params["beta_pow"], dtype=np.float32) * (1 if grads_only else np.array([cfg.beta1, cfg.beta2] * 2, dtype=np.float32))
    out["updates"] = int(params["updates"]) + (0 if grads_only else 1)
    info = {"critic_loss": float(loss.detach()), "mean_q": float(q.detach().mean()), "grad_critic": {k: gq[k].numpy() for k in TENSORS},
            "grad_actor": {k: gp[k].numpy() for k in TENSORS}}
    return out, info


def adam_host(w, g, m, v, wt, beta_pow, lr, cfg):
    """``k_ddpg_adam`` for one tensor (or one flat slot) in numpy float32, operation for operation: returns (w, m, v, wt, beta_pow) after the step.
    ``beta_pow``: float32 (beta1^(t-1), beta2^(t-1)), the running products the device keeps."""
    f = np.float32
    w, g, m, v, wt = (np.asarray(x, dtype=f) for x in (w, g, m, v, wt))
    b1, b2, tau, eps = f(cfg.beta1), f(cfg.beta2), f(cfg.tau), f(cfg.eps)
    omb1, omb2, omtau = f(1) - b1, f(1) - b2, f(1) - tau
    pw1, pw2 = f(beta_pow[0]) * b1, f(beta_pow[1]) * b2
    step = f(lr) / (f(1) - pw1)
    bc2s = np.sqrt(f(1) - pw2)
    m = b1 * m + omb1 * g
    v = b2 * v + omb2 * (g * g)
    denom = np.sqrt(v) / bc2s + eps
    w = w - step * (m / denom)
    wt = omtau * wt + tau * w
    return w, m, v, wt, np.array([pw1, pw2], dtype=f)


# ---- TD3: configuration and host twins ---------------------------------------------------------------------------------------------------------
TD3_STREAM = 0x7464336E6F697365


class TD3Config(DDPGConfig):
    """``DDPGConfig`` plus TD3's three constants (Fujimoto et al. 2018, their defaults): ``target_noise`` and ``noise_clip`` are fractions of
    ``tanh_scale`` as ``noise`` is; the actor and all targets are updated on every ``policy_delay``-th update."""

    def __init__(self, *args, target_noise=0.2, noise_clip=0.5, policy_delay=2, **kw):
        super().__init__(*args, **kw)
        self.target_noise_std, self.noise_clip_abs = float(target_noise) * self.tanh_scale, float(noise_clip) * self.tanh_scale
        self.policy_delay = int(policy_delay)

    def to_c_td3(self, seed):
        return _capi.TD3Cfg(base=self.to_c(seed), target_noise_std=self.target_noise_std, noise_clip=self.noise_clip_abs, policy_delay=self.policy_delay)


def smoothing_noise_host(seed, update, n):
    """Target smoothing of update ``update``, minibatch rows 0 .. n-1: (draw1, draw2, gauss) as ``noise_host`` forms them, on TD3's own stream."""
    return noise_host(seed, update, n, stream=TD3_STREAM)


def smoothing_eps_host(gauss, cfg, dtype=np.float64):
    """eps = clip(sigma * gauss, -c, +c) in ``dtype`` (float32: the kernel's statement, given the kernel's float32 gauss)."""
    f = np.dtype(dtype).type
    return np.clip(f(cfg.target_noise_std) * np.asarray(gauss, dtype=dtype), -f(cfg.noise_clip_abs), f(cfg.noise_clip_abs))


def new_params_td3(actor_net, critic_net, critic2_net):
    """``new_params`` plus critic 2's four slots; ``beta_pow`` float32 [6]: actor, critic 1, critic 2."""
    p = new_params(actor_net, critic_net)
    p2 = new_params(actor_net, critic2_net)
    for slot in _capi.TD3_SLOTS:
        p[slot] = p2[slot.replace("critic2", "critic")]
    p["beta_pow"] = np.ones(6, dtype=np.float32)
    return p


def update_host_td3(params, batch, cfg, dtype="float64", eps=None, lr_q=None, lr_pi=None, grads_only=False, weights=None, disc=None):
    """One TD3 update in torch with autograd, every tensor in ``dtype``: ``update_host`` with the smoothed, clipped target action, the minimum of
    both target critics, both critics stepped, and -- only if (updates + 1) % cfg.policy_delay == 0 -- the actor stepped against critic 1 and all
    three targets moved.  ``eps``: the smoothing noise per minibatch row (None: zeros); the twin is handed it, it does not draw.
    ``params``: as ``new_params_td3`` / ``TD3Learner.state_dict()["params"]``.  ``info`` carries ``critic_loss`` / ``critic2_loss``, ``mean_q`` /
    ``mean_q2``, ``grad_critic`` / ``grad_critic2`` / ``grad_actor`` (None when the actor did not step) and ``targets`` [B][4] = a', Qt1, Qt2, y.
    ``grads_only``: nothing is applied and all three gradients are taken against the current critics (``stmpc_td3_grads_device``'s mode).
    ``weights``: as ``update_host``'s, on both critics' losses; ``disc``: as ``update_host``'s."""
    import torch
    td = getattr(torch, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=td)
    slots = _capi.DDPG_SLOTS + _capi.TD3_SLOTS
    P = {slot: {k: T(params[slot][k]) for k in TENSORS} for slot in slots}
    s, a, r, s2, mask = (T(batch[k]) for k in ("s", "a", "r", "s2", "mask"))
    e = T(np.zeros(len(batch["r"])) if eps is None else eps)
    scale, mean = cfg.tanh_scale, cfg.tanh_mean
    lr_q, lr_pi = cfg.lr_q if lr_q is None else lr_q, cfg.lr_pi if lr_pi is None else lr_pi
    u = int(params["updates"])
    due = grads_only or (u + 1) % cfg.policy_delay == 0
    with torch.no_grad():
        a2 = torch.clamp((torch.tanh(_mlp(P["actor_target"], s2)) * scale + mean) + e, cfg.action_low, cfg.action_high)
        x2 = torch.cat([s2, a2[:, None]], 1)
        qt1, qt2 = _mlp(P["critic_target"], x2), _mlp(P["critic2_target"], x2)
        y = r + (cfg.gamma if disc is None else T(disc)) * mask * torch.minimum(qt1, qt2)
    info = {"targets": torch.stack([a2, qt1, qt2, y], 1).numpy(), "grad_actor": None}
    for name, tag in (("critic", ""), ("critic2", "2")):
        crit = {k: P[name][k].clone().requires_grad_(True) for k in TENSORS}
        q = _mlp(crit, torch.cat([s, a[:, None]], 1))
        loss = ((q - y) ** 2).mean()
        g = dict(zip(TENSORS, torch.autograd.grad(loss if weights is None else (T(weights) * (q - y) ** 2).mean(), [crit[k] for k in TENSORS])))
        if not grads_only:
            _adam_step(P, name, g, lr_q, u + 1, cfg)
        info["critic%s_loss" % tag], info["mean_q%s" % tag], info["grad_critic%s" % tag] = float(loss.detach()), float(q.detach().mean()), {k: g[k].numpy() for k in TENSORS}
    if due:
        act = {k: P["actor"][k].clone().requires_grad_(True) for k in TENSORS}
        pa = torch.tanh(_mlp(act, s)) * scale + mean
        aloss = -_mlp(P["critic"], torch.cat([s, pa[:, None]], 1)).mean()
        gp = dict(zip(TENSORS, torch.autograd.grad(aloss, [act[k] for k in TENSORS])))
        info["grad_actor"] = {k: gp[k].numpy() for k in TENSORS}
        if not grads_only:
            _adam_step(P, "actor", gp, lr_pi, (u + 1) // cfg.policy_delay, cfg)        # the actor's own step count
            for name in ("actor", "critic", "critic2"):
                _polyak(P, name, cfg)
    out = {slot: {k: P[slot][k].detach().numpy() for k in TENSORS} for slot in slots}
    b = np.array([cfg.beta1, cfg.beta2], dtype=np.float32)
    one = np.ones(2, dtype=np.float32)
    out["beta_pow"] = np.array(params["beta_pow"], dtype=np.float32) * (1 if grads_only else np.concatenate([b if due else one, b, b]))
    out["updates"] = u + (0 if grads_only else 1)
    return out, info


# ---- prioritised replay: host twins (stmpc_per_kernels.hpp) ------------------------------------------------------------------------------------
PER_STREAM = 0x70657264726177
PER_REDRAWS = 3


def per_leaves(capacity):
    """The tree's leaf count: ``capacity`` rounded up to a power of two."""
    n = 1
    while n < int(capacity):
        n *= 2
    return n


def per_pow(p, alpha):
    """p ** alpha as the library forms it: a square root for 0.5, the identity for 1, pow otherwise (float64)."""
    p = np.asarray(p, dtype=np.float64)
    return np.sqrt(p) if alpha == 0.5 else (p.copy() if alpha == 1.0 else np.power(p, np.float64(alpha)))


def per_priority_host(td, cfg):
    """The leaf weights min(|td| + min_priority, max_priority) ** alpha of critic errors ``td`` (float32, as the device reports them); float64."""
    e = np.abs(np.asarray(td, dtype=np.float32).astype(np.float64)) + np.float64(cfg.min_priority)
    return per_pow(np.where(e < cfg.max_priority, e, np.float64(cfg.max_priority)), cfg.alpha)


class SumTreeHost:
    """The reference's ``SumTree`` weights (dqn.py:727-794) for a ring of ``capacity`` rows: ``nodes`` float64 [2 * leaves - 1], root 0, children of
    i at 2i + 1 and 2i + 2, ring row p at leaf p + leaves - 1.  ``push(n)``: the next ``n`` ring rows get ``max_priority ** alpha``; ``set``: one leaf.
    Every internal node on the way up is recomputed as left + right, as ``_update_sum`` does."""

    def __init__(self, capacity, cfg=None):
        self.capacity, self.cfg = int(capacity), cfg if cfg is not None else PERConfig()
        self.leaves = per_leaves(capacity)
        self.nodes = np.zeros(2 * self.leaves - 1, dtype=np.float64)
        self.cursor = self.fill = 0

    def set(self, position, weight):
        i = int(position) + self.leaves - 1
        self.nodes[i] = weight
        while i:
            i = (i - 1) // 2
            self.nodes[i] = self.nodes[2 * i + 1] + self.nodes[2 * i + 2]

    def push(self, n):
        w = float(per_pow(self.cfg.max_priority, self.cfg.alpha))
        for _ in range(int(n)):
            self.set(self.cursor, w)
            self.cursor = (self.cursor + 1) % self.capacity
            self.fill = min(self.fill + 1, self.capacity)


def per_sample_host(nodes, seed, update, batch, fill):
    """Ring rows of the ``batch`` minibatch rows of update ``update`` drawn from the tree ``nodes`` with ``fill`` rows filled (int64 [batch]):
    ``stmpc_per_sample_index``'s procedure in Python floats (IEEE fp64, one operation per operation)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    leaves = (nodes.size + 1) // 2
    tree, total, fill, s = nodes.tolist(), float(nodes[0]), int(fill), (int(seed) & _M64) ^ PER_STREAM
    out = np.zeros(int(batch), dtype=np.int64)
    for r in range(int(batch)):
        pos = None
        for a in range(PER_REDRAWS + 1):
            roll = ((hash3(s, update, r | (a << 32)) >> 11) * 2.0 ** -53) * total
            i = 0
            while i < leaves - 1:
                left = 2 * i + 1
                if roll <= tree[left]:
                    i = left
                else:
                    roll -= tree[left]
                    i = left + 1
            if i - (leaves - 1) < fill and tree[i] > 0.0:
                pos = i - (leaves - 1)
                break
        out[r] = hash3(seed, update, r) % fill if pos is None else pos
    return out


def per_weights_host(nodes, idx, fill, beta):
    """Importance weights float32 [batch] of the rows ``idx``: (fill * p / total) ** -beta over the largest of them, in float64; exactly 1 for
    ``beta`` 0 (and for a row of weight 0, which only the uniform fall-back can draw and which does not count for the largest)."""
    nodes, idx = np.asarray(nodes, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    if beta == 0:
        return np.ones(idx.size, dtype=np.float32)
    p = nodes[idx + (nodes.size + 1) // 2 - 1]
    ok = p > 0
    w = np.ones(idx.size, dtype=np.float64)
    if ok.any():
        w[ok] = np.power(np.float64(fill) * p[ok] / nodes[0], -np.float64(beta)) / np.power(np.float64(fill) * p[ok].min() / nodes[0], -np.float64(beta))
    return w.astype(np.float32)


# ---- multi-step returns: host twins (stmpc_nstep_kernels.hpp) ------------------------------------------------------------------------------------
def nstep_window_host(rows, i, cursor, fill, N, n, gamma):
    """The window of ring row ``i`` as ``nstep_window`` of csrc/stmpc_nstep_kernels.hpp forms it, operation for operation: (R float32, disc
    float32, the ring row of the window's last transition, m).  ``rows``: the whole ring [capacity][68] (column 67: done); ``cursor`` / ``fill``:
    the ring's counters; ``N``: the rows of every push; ``n``: the window's length.  row_k = (i + k N) % capacity exists iff age(i) =
    (cursor - 1 - i) mod capacity >= k N; the window ends with the first k at which row_k is done, k + 1 == n or row_{k+1} does not exist.
    R and disc accumulate in float64 from float64(float32(gamma)) in k order and are rounded to float32 once."""
    cap, i, N, n = len(rows), int(i), int(N), int(n)
    if not 0 <= i < int(fill):
        raise ValueError("row %d is not a filled ring row (fill is %d)" % (i, fill))
    age = (int(cursor) - 1 - i) % cap
    g = float(np.float32(gamma))
    R, gk, k = 0.0, 1.0, 0
    while True:
        row = rows[(i + k * N) % cap]
        term = gk * float(row[64])
        R = term if k == 0 else R + term
        gk = gk * g
        if row[_capi.DONE_COL] != 0 or k + 1 == n or age < (k + 1) * N:
            return np.float32(R), np.float32(gk), (i + k * N) % cap, k + 1
        k += 1


def nstep_batch_host(rows, idx, cursor, fill, N, n, gamma, n_obs, dqn=False):
    """The minibatch dict ``update_host`` / ``update_host_td3`` (``dqn``: ``update_host_dqn`` / ``dqn_targets_host``) take for the ring rows ``idx``
    under n-step returns: s and a of row i, s' and the mask of its window's last row, r = R, plus ``disc`` (gamma^m, for the twins' ``disc=``),
    ``last`` and ``m``."""
    rows = np.asarray(rows)
    win = [nstep_window_host(rows, i, cursor, fill, N, n, gamma) for i in idx]
    g = np.array(rows[np.asarray(idx, dtype=np.int64)])
    last = np.array([w[2] for w in win], dtype=np.int64)
    g[:, 32:64], g[:, 65], g[:, 64] = rows[last, 32:64], rows[last, 65], np.array([w[0] for w in win], dtype=np.float32)
    b = dqn_batch_from_rows(g, n_obs) if dqn else batch_from_rows(g, n_obs)
    b.update(disc=np.array([w[1] for w in win], dtype=np.float32), last=last, m=np.array([w[3] for w in win], dtype=np.int64), rows=g)
    return b


# ---- the learner -------------------------------------------------------------------------------------------------------------------------------
# the columns of ``stats_device``: a DDPG learner's, a TD3 learner's (``stats_td3``) and a discrete learner's; a population's table has one such row per member
_DDPG_STATS = ("critic_loss", "mean_q", "fill", "updates")
_TD3_STATS = ("critic_loss", "critic2_loss", "mean_q", "mean_q2", "fill", "updates")
_DQN_STATS = ("loss", "mean_q", "fill", "updates")


def _stats_dict(keys, s):
    """``stats_device`` on the host as a dict: scalars from a lone learner's row [len(keys)], arrays of length P from a population's table
    [P][len(keys)]; ``fill`` and ``updates`` are integers."""
    out = {}
    for i, k in enumerate(keys):
        col, integer = s[..., i], k in ("fill", "updates")
        out[k] = (int(col) if integer else float(col)) if s.ndim == 1 else (col.astype(np.int64) if integer else col.copy())
    return out


def _check_push(torch, obs, reward, next_obs, terminated, truncated, final_obs):
    """What ``push`` asks of an env step's tensors, whatever the learner."""
    assert obs.dtype == next_obs.dtype == torch.float32 and reward.dtype == torch.float64
    assert terminated.dtype == truncated.dtype == torch.bool and obs.stride(1) == 1 and obs.stride(0) == next_obs.stride(0)
    assert final_obs is None or (final_obs.dtype == torch.float32 and final_obs.stride(0) == obs.stride(0))


def _check_ddpg_act(torch, obs, ticks):
    assert obs.dtype == torch.float32 and ticks.dtype == torch.int32 and obs.stride(1) == 1


def _check_ddpg_push(torch, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs):
    assert action.dtype == torch.float64 and ticks.dtype == torch.int32
    _check_push(torch, obs, reward, next_obs, terminated, truncated, final_obs)


def _check_q_act(torch, obs, debug_q, n_actions):
    assert obs.dtype == torch.float32 and obs.stride(1) == 1
    assert debug_q is None or (debug_q.dtype == torch.float32 and debug_q.is_contiguous() and debug_q.shape == (obs.shape[0], n_actions))


def _check_q_push(torch, obs, action, reward, next_obs, terminated, truncated, final_obs):
    assert action.dtype == torch.int32 and action.is_contiguous()
    _check_push(torch, obs, reward, next_obs, terminated, truncated, final_obs)


class _Learner:
    """What ``DDPGLearner`` and ``DQNLearner`` share word for word: the handle's lifetime, the stream, the output tensor kept per n, the debug reads
    of the replay and the statistics, and ``state_dict`` / ``load_state_dict``.  A subclass names its binding's entries (``ctx.<_api>_<name>``, and
    ``ctx.<_per_api>_<name>`` for prioritised replay), its ``_slots`` and ``_flatten``, reads one slot in ``_slot`` and makes the handle it owns in
    ``_create`` (a population's member borrows that one instead: ``_Borrowed``)."""

    _owns_handle = True                                             # (False: a population's member, whose population sets up what it shares)

    def _call(self, name):
        return getattr(self.ctx, "%s_%s" % (self._api, name))

    def _make_handle(self):
        """What becomes ``self.handle``: the handle the learner's own entries take."""
        return self._create()

    def _enable_nstep(self, env, rows_per_push):
        """``cfg.n_step`` onto the new handle (the ring is empty); ``self.rows_per_push``: the N every push must have when n_step > 1."""
        owner = getattr(self, "_population", None)
        self.rows_per_push = owner.n_per_member if owner is not None else (getattr(env, "n", None) if env is not None else rows_per_push)
        if self._owns_handle and self.cfg.n_step > 1:
            self.ctx.nstep_enable(self._api, self.handle, self.cfg.to_c_nstep(self.rows_per_push))

    def nstep_window(self, idx):
        """Debug: float64 [len(idx)][4] = R, disc, the ring row of the window's last transition, m for the filled ring rows ``idx``
        (``nstep_window_host``'s four); synchronises."""
        return self.ctx.nstep_window(self._api, self.handle, idx)

    def _check_nstep(self, sd):
        if "n_step" in sd and int(sd["n_step"]) != self.cfg.n_step:
            raise ValueError("the state was saved with n_step = %d, this learner has n_step = %d: the rows' done column and the targets differ" % (int(sd["n_step"]), self.cfg.n_step))
        if self.cfg.n_step > 1 and "rows_per_push" in sd and int(sd["rows_per_push"] or 0) != int(self.rows_per_push or 0):
            raise ValueError("the state was saved with %r rows per push, this learner has %r" % (sd["rows_per_push"], self.rows_per_push))

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                self._call("destroy")(self.handle)
            except Exception:
                pass
            self.handle = None

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _out(self, n, dtype):
        """The tensor [n] ``act`` returns: one per n, reused."""
        out = self._actions.get(n)
        if out is None:
            out = self._actions[n] = self.torch.empty(n, dtype=dtype, device=self.device)
        return out

    def minibatch(self):
        """Debug: the replay rows [batch][68] the next update will read (numpy; ``batch_from_rows`` / ``dqn_batch_from_rows``); synchronises."""
        rows = self.torch.empty(self.cfg.batch, _capi.DDPG_ROW, dtype=self.torch.float32, device=self.device)
        self._call("gather")(self.handle, rows.data_ptr(), self._stream())
        return rows.cpu().numpy()

    def priorities(self):
        """Debug, prioritised replay: the sum tree, float64 [2 * leaves - 1] (numpy; ``SumTreeHost``'s layout); synchronises."""
        return getattr(self.ctx, self._per_api + "_tree_read")(self.handle, 0, 2 * per_leaves(self.cfg.capacity) - 1)

    def last_sample(self):
        """Debug, prioritised replay: {"idx" int64, "td" float32, "weight" float32}, [batch] each (numpy) -- the ring rows and importance weights of
        the most recent sampling step (an update's, or ``minibatch`` / ``grads`` / ``targets``') and Q - y of the most recent critic pass (TD3: of
        the critic with the larger magnitude); synchronises."""
        torch, B = self.torch, self.cfg.batch
        idx = torch.zeros(B, dtype=torch.int64, device=self.device)
        td, w = (torch.zeros(B, dtype=torch.float32, device=self.device) for _ in range(2))
        getattr(self.ctx, self._per_api + "_last")(self.handle, idx.data_ptr(), td.data_ptr(), w.data_ptr(), self._stream())
        return {"idx": idx.cpu().numpy(), "td": td.cpu().numpy(), "weight": w.cpu().numpy()}

    def stats_device(self):
        """fp64 [4] device tensor: the (critic's) loss and mean Q(s, a) of the last minibatch, fill, updates done (asynchronous)."""
        self._call("stats")(self.handle, self._stats.data_ptr(), self._stream())
        return self._stats

    def state_dict(self):
        """{"params": the slots (eight of DDPG, four of DQN) as dicts of numpy tensors + beta_pow + updates, "counters": int64 [8]}; the replay ring
        is not part of it; ``n_step`` and ``rows_per_push`` say how its rows were written and are read."""
        cn, bp = self._call("get_state")(self.handle)
        params = {slot: self._slot(i) for i, slot in enumerate(self._slots)}
        params["beta_pow"], params["updates"] = bp, int(cn[2])
        return {"params": params, "counters": cn, "n_step": self.cfg.n_step, "rows_per_push": self.rows_per_push}

    def load_state_dict(self, sd):
        """The inverse; ``counters`` None: only the update count and Adam's beta powers are set (the replay's cursor and fill stay).  A state
        saved under another ``n_step`` is refused (one without the key is taken as it is)."""
        self._check_nstep(sd)
        p = sd["params"]
        for i, slot in enumerate(self._slots):
            self._call("set_params")(self.handle, i, self._flatten(p[slot]))
        cn = sd.get("counters")
        if cn is None:
            cn, _ = self._call("get_state")(self.handle)
            cn[2] = int(p["updates"])
        self._call("set_state")(self.handle, cn, p["beta_pow"])


class DDPGLearner(_Learner):
    """``env_or_dims``: a ``MergeVecEnv`` (continuous-jerk; its context, observation width and action Box are taken over) or the observation width.
    ``cfg``: ``DDPGConfig`` (None: the defaults); ``seed``: of the initialisation, the minibatch indices and the exploration noise;
    ``init``: None (torch's nn.Linear initialisation, last layers zero), the name of a shipped actor ("medium1": that actor, a fresh critic), or a
    dict ``{"actor": net, "critic": net}`` of numpy tensors.  ``rows_per_push``: with ``cfg.n_step`` > 1 and no env, the rows N every push
    will have (an env's ``n`` otherwise); a push with another N is then refused."""

    _api, _per_api, _slots, _flatten = "ddpg", "per", _capi.DDPG_SLOTS, staticmethod(flatten)

    def __init__(self, env_or_dims, cfg=None, seed=0, init=None, ctx=None, rows_per_push=None):
        import torch
        self.torch = torch
        env = None if isinstance(env_or_dims, int) else env_or_dims
        if env is not None and not env.continuous:
            raise ValueError("DDPG needs the continuous action space (sumo-jerk-continuous-v0)")
        self.cfg = cfg if cfg is not None else DDPGConfig(n_obs=env.obs_dim if env is not None else int(env_or_dims))
        n_obs = env.obs_dim if env is not None else int(env_or_dims)
        if self.cfg.n_obs != n_obs:
            raise ValueError("cfg.n_obs is %d, the observation has %d entries" % (self.cfg.n_obs, n_obs))
        self.ctx = ctx if ctx is not None else (env.ctx if env is not None else _capi.Context(-1))
        self.seed = int(seed)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.handle = self._make_handle()
        self._enable_nstep(env, rows_per_push)
        if self.cfg.per is not None:                                # (a population member's handle refuses: the population enables its members)
            self.ctx.per_enable(self.handle, self.cfg.per.to_c())
        c = self.cfg
        rng = np.random.default_rng(self.seed)
        if isinstance(init, dict):
            a_net, q_net = init["actor"], init["critic"]
        else:
            a_net, q_net = init_net(c.n_obs + 1, c.h1, c.h2, rng), init_net(c.n_obs + 2, c.h1, c.h2, rng)
            if init is not None:
                w = _actor.load_weights(init)
                if abs(w["tanh_scale"] - c.tanh_scale) > 0 or abs(w["tanh_mean"] - c.tanh_mean) > 0:
                    raise ValueError("the shipped actor's squash is not this action Box's")
                a_net = {k: w[k] for k in TENSORS}
        self._lens = {"actor": flatten(a_net).size, "critic": flatten(q_net).size}
        if self._lens["actor"] != (c.n_obs + 2) * c.h1 + (c.h1 + 2) * c.h2 + 1:
            raise ValueError("the actor's tensors do not have the shape %d -> %d -> %d -> 1" % (c.n_obs + 1, c.h1, c.h2))
        self.load_state_dict({"params": self._initial_params(a_net, q_net, rng), "counters": None})
        z = lambda *sh, dtype=torch.float64: torch.zeros(sh, dtype=dtype, device=self.device)
        self._stats = z(4)
        self._actions = {}

    def _create(self):
        return self.ctx.ddpg_create(self.cfg.to_c(self.seed))

    def _initial_params(self, a_net, q_net, rng):
        """The parameter state a new learner starts from; ``rng`` stands after the draws of the actor and the critic."""
        return new_params(a_net, q_net)

    def _slot(self, i):
        c, which = self.cfg, "critic" if i >= 4 else "actor"
        return unflatten(self.ctx.ddpg_get_params(self.handle, i, self._lens[which]), c.n_obs + (2 if i >= 4 else 1), c.h1, c.h2)

    # -- acting / replay / update: asynchronous ---------------------------------------------------------------------------------------------
    def act(self, obs, ticks, noise=True, debug=None):
        """Actions fp64 [n] for observations float32 [n][n_obs] and episode ticks int32 [n] (``MergeVecEnv.episode_ticks``): the actor's output,
        plus N(0, cfg.noise_std) exploration noise if ``noise``, clipped to the action Box.  The returned tensor is reused by the next call
        with the same n.  ``debug``: uint32 [n][4] device tensor for the draws (debugging)."""
        n = obs.shape[0]
        out = self._out(n, self.torch.float64)
        _check_ddpg_act(self.torch, obs, ticks)
        self.ctx.ddpg_act(self.handle, n, obs.data_ptr(), obs.stride(0), ticks.data_ptr(), noise, out.data_ptr(), debug.data_ptr() if debug is not None else 0,
                          self._stream())
        return out

    def push(self, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs=None, next_ticks=None):
        """One env step into the replay ring: ``obs`` / ``ticks`` as given to ``act``, ``action`` fp64 [n], and what ``env.step`` returned
        (``final_obs = info["final_observation"]``).  Where an episode ended, s' is the final observation at ticks + 1."""
        _check_ddpg_push(self.torch, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs)
        self.ctx.ddpg_push(self.handle, obs.shape[0], obs.data_ptr(), next_obs.data_ptr(), final_obs.data_ptr() if final_obs is not None else 0, obs.stride(0),
                           ticks.data_ptr(), next_ticks.data_ptr() if next_ticks is not None else 0, action.data_ptr(), reward.data_ptr(),
                           terminated.data_ptr(), truncated.data_ptr(), self._stream())

    def update(self, n=1, lr_q=None, lr_pi=None):
        """``n`` updates (each: critic step, actor step, both Polyak updates); on the device nothing happens until more than cfg.replay_start
        frames were pushed.  ``lr_q`` / ``lr_pi``: this call's learning rates (a schedule is the caller's; default cfg's)."""
        self.ctx.ddpg_update(self.handle, n, self.cfg.lr_q if lr_q is None else lr_q, self.cfg.lr_pi if lr_pi is None else lr_pi, self._stream())

    def grads(self):
        """Debug: (actor gradient, critic gradient) on the current update index's minibatch as dicts of numpy tensors; nothing applied; synchronises."""
        torch, c = self.torch, self.cfg
        ga = torch.empty(self._lens["actor"], dtype=torch.float32, device=self.device)
        gq = torch.empty(self._lens["critic"], dtype=torch.float32, device=self.device)
        self.ctx.ddpg_grads(self.handle, ga.data_ptr(), gq.data_ptr(), self._stream())
        return unflatten(ga.cpu().numpy(), c.n_obs + 1, c.h1, c.h2), unflatten(gq.cpu().numpy(), c.n_obs + 2, c.h1, c.h2)

    def stats(self):
        """``stats_device`` as a dict; synchronises."""
        return _stats_dict(_DDPG_STATS, self.stats_device().cpu().numpy())

    def export_actor(self, path):
        """Write the online actor as the ``.npz`` ``actor.load_weights`` reads (w0 ... b2 float32, tanh_scale, tanh_mean)."""
        write_actor(path, self._slot(0), self.cfg.tanh_scale, self.cfg.tanh_mean)
        return path


class TD3Learner(DDPGLearner):
    """TD3 on the device (``csrc/stmpc_td3_kernels.hpp``, ``stmpc_td3_*``): ``DDPGLearner`` with a second critic, clipped noise on the target action
    and the actor and all targets updated every ``cfg.policy_delay``-th update (``TD3Config``; module text of ``update_host_td3``).

    ``self.handle`` is the BASE: a DDPG learner handle borrowed from the TD3 handle, which owns the actor, critic 1, the ring and the counters --
    so ``act`` / ``push`` / ``stats`` / ``export_actor`` / ``minibatch`` are inherited as they are, and ``train_ddpg``, ``actor.DDPGActor.from_learner``
    and a shielded env's ``policy=`` take a ``TD3Learner`` like any learner.  ``init``: as ``DDPGLearner``'s, or a triple (actor, critic, critic 2)
    of nets (critic 2 None, or no triple: a fresh draw from the next values of the same rng)."""

    def __init__(self, env_or_dims, cfg=None, seed=0, init=None, ctx=None, rows_per_push=None):
        self._critic2_init = None
        if isinstance(init, (tuple, list)):
            a_net, q_net, self._critic2_init = init
            init = {"actor": a_net, "critic": q_net}
        if cfg is None:
            cfg = TD3Config(n_obs=env_or_dims if isinstance(env_or_dims, int) else env_or_dims.obs_dim)
        super().__init__(env_or_dims, cfg, seed=seed, init=init, ctx=ctx, rows_per_push=rows_per_push)
        self._stats6 = self.torch.zeros(6, dtype=self.torch.float64, device=self.device)

    def _create(self):
        return self.ctx.td3_create(self.cfg.to_c_td3(self.seed))

    def _make_handle(self):
        self.td3 = self._create()
        return self.ctx.td3_base(self.td3)

    def _initial_params(self, a_net, q_net, rng):
        c = self.cfg
        q2 = self._critic2_init if self._critic2_init is not None else init_net(c.n_obs + 2, c.h1, c.h2, rng)
        return new_params_td3(a_net, q_net, q2)

    def __del__(self):
        self.handle = None                                          # the TD3 handle destroys its base
        if getattr(self, "td3", None) is not None:
            try:
                self.ctx.td3_destroy(self.td3)
            except Exception:
                pass
            self.td3 = None

    def update(self, n=1, lr_q=None, lr_pi=None):
        """``n`` TD3 updates, six launches each whatever the counters say: both critics step; on every cfg.policy_delay-th update the actor steps and
        all targets move; nothing happens until more than cfg.replay_start frames were pushed."""
        self.ctx.td3_update(self.td3, n, self.cfg.lr_q if lr_q is None else lr_q, self.cfg.lr_pi if lr_pi is None else lr_pi, self._stream())

    def grads(self):
        """Debug: (actor gradient against critic 1, critic 1's gradient, critic 2's gradient) on the current update index's minibatch; nothing applied;
        synchronises."""
        torch, c = self.torch, self.cfg
        ga = torch.empty(self._lens["actor"], dtype=torch.float32, device=self.device)
        g1, g2 = (torch.empty(self._lens["critic"], dtype=torch.float32, device=self.device) for _ in range(2))
        self.ctx.td3_grads(self.td3, ga.data_ptr(), g1.data_ptr(), g2.data_ptr(), self._stream())
        return (unflatten(ga.cpu().numpy(), c.n_obs + 1, c.h1, c.h2),) + tuple(unflatten(g.cpu().numpy(), c.n_obs + 2, c.h1, c.h2) for g in (g1, g2))

    def targets(self):
        """Debug: float32 [batch][5] = eps, a', Qt1, Qt2, y of the minibatch the next update will draw (numpy); synchronises."""
        out = self.torch.zeros(self.cfg.batch, 5, dtype=self.torch.float32, device=self.device)
        self.ctx.td3_targets(self.td3, out.data_ptr(), self._stream())
        return out.cpu().numpy()

    def stats_td3(self):
        """Both critics' numbers as a dict; synchronises.  (``stats`` stays critic 1's four.)"""
        self.ctx.td3_stats(self.td3, self._stats6.data_ptr(), self._stream())
        return _stats_dict(_TD3_STATS, self._stats6.cpu().numpy())

    def state_dict(self):
        """``DDPGLearner.state_dict`` plus critic 2's four slots; ``beta_pow`` float32 [6]: actor, critic 1, critic 2."""
        c = self.cfg
        sd = super().state_dict()
        for i, slot in enumerate(_capi.TD3_SLOTS):
            sd["params"][slot] = unflatten(self.ctx.td3_get_params(self.td3, i, self._lens["critic"]), c.n_obs + 2, c.h1, c.h2)
        sd["params"]["beta_pow"] = np.concatenate([sd["params"]["beta_pow"], self.ctx.td3_get_state(self.td3)])
        return sd

    def load_state_dict(self, sd):
        self._check_nstep(sd)
        p = sd["params"]
        super().load_state_dict({"params": dict(p, beta_pow=p["beta_pow"][:4]), "counters": sd.get("counters")})
        for i, slot in enumerate(_capi.TD3_SLOTS):
            self.ctx.td3_set_params(self.td3, i, flatten(p[slot]))
        self.ctx.td3_set_state(self.td3, p["beta_pow"][4:6])


def per_member(value, P, default=None):
    """What a population's call takes per member -- a learning rate, an eps -- as a float64 array: ``value`` None gives ``default``, a scalar is
    repeated ``P`` times, and an array is taken as it is (the library checks a given array's length)."""
    if value is None:
        return default
    value = np.asarray(value, dtype=np.float64)
    return np.full(P, float(value)) if value.ndim == 0 else value


class _Borrowed:
    """In front of a lone learner's class, one member of a population as that learner: where the lone learner creates the handle it owns, the
    member's is borrowed from the population (its binding's ``member`` entry), which outlives it; everything else -- the seeded initialisation,
    what a TD3 learner takes from its handle and a discrete learner from the env, included -- is the lone learner's code."""

    _owns_handle = False

    def __init__(self, population, m, env, cfg, seed, init):
        self._population, self._borrowed = population, population._call("member")(population.handle, m)
        super().__init__(env, cfg, seed=seed, init=init, ctx=population.ctx)

    def _create(self):
        return self._borrowed

    def __del__(self):
        self.handle = None                                          # the population destroys its members (no lone learner's ``__del__`` runs)


class _PopulationMember(_Borrowed, DDPGLearner):
    """One member of a ``DDPGPopulation`` as a ``DDPGLearner`` (``stmpc_ddpg_pop_member``)."""


class DDPGPopulation:
    """P independent DDPG learners on one ``MergeVecEnv``, advanced together: one launch per kernel instead of one per member and kernel
    (``csrc/stmpc_ddpg_pop_kernels.hpp``).  The reference trains one agent per ``train_{traffic_type}_{seed}.json`` config, a ``TRAIN_DDPG`` run
    (ddpg.py:44-80) each, and compares them (pretrained_models/README.md); a population is those runs side by side on one device.

    ``cfgs``: a list of ``DDPGConfig`` or ``(cfg, P)``; the members share n_obs, h1, h2, batch and capacity and may differ in everything else.
    ``env.n`` must be ``P * n_per_member``: member m owns environments [m * n_per_member, (m + 1) * n_per_member).  ``seeds``: one per member
    (None: 0 .. P-1); ``init``: as ``DDPGLearner``'s, for every member, or a list of P.  Member m starts exactly as
    ``DDPGLearner(seed=seeds[m], init=...)`` does and stays bit-identical to that learner driven on its slice alone.
    ``act`` / ``push`` / ``update`` / ``stats_device`` / ``stats`` are ``DDPGLearner``'s on the whole env's tensors; ``member(m)`` is a
    ``DDPGLearner`` view (``state_dict``, ``load_state_dict``, ``export_actor``, ``grads``, ``minibatch``).

    ``env`` may have traffic groups (``MergeVecEnv(traffic=[...])``) when there are as many as members: member m then trains on traffic m -- the
    reference's ``train_{traffic}_{seed}.json`` runs for several traffic types in one launch sequence -- and stays bit-identical to a lone
    learner on a lone env of that traffic.

    ``env`` may have reward groups (``MergeVecEnv(rewards=[...])``) when there are as many as members (``env.R == P``, so that
    ``n_per_member == env.n_per_reward_group``): member m's slice is reward group m, so member m trains under reward m -- the reference's
    reward-shaping comparison, one ``TRAIN_DDPG`` run per config, in one launch sequence -- and stays bit-identical to a lone learner fed that
    slice of the lone env made under reward m.  Nothing else changes: the population reads the env's reward tensor row by row.
    ``evaluate_members`` / ``episodes.summary_by_member`` then compare the policies the rewards produced on one common report.

    ``per``: prioritised replay (module text) -- None, one ``PERConfig`` for every member, or a list of P entries, each a ``PERConfig`` or None
    (that member samples uniformly).  It is the population's argument, not the members' cfgs' (a cfg with ``per=`` is refused): the population
    enables its members' trees in one call before anything is pushed.  ``self.per`` is the per-member list.  A prioritised member is
    bit-identical to ``DDPGLearner(cfg with per=...)`` on its slice, a uniform one to the member of a population without ``per``; one update is
    eight launches whatever P is (six when no member is prioritised).  ``member(m).priorities()`` / ``.last_sample()`` read member m's tree and
    last minibatch (they raise on a uniform member).

    ``n_step`` is a member's cfg's like any other constant, so "which n" is a sweep: member m forms ``cfgs[m].n_step``-step returns from pushes
    of ``n_per_member`` rows and stays bit-identical to the lone learner with that cfg; ``member(m).nstep_window(idx)`` reads its windows."""

    _api, _stat_keys = "ddpg_pop", _DDPG_STATS                      # the binding's entries (ctx.<_api>_create, ...) and the columns of a stats row
    _nstep_kind = "ddpg"                                            # which stmpc_pop_nstep_enable_* entry sets the members' n_step
    _cfg_type, _action_dtype = DDPGConfig, "float64"                # what a (cfg, P) pair holds, and the dtype of the tensor ``act`` returns

    def _call(self, name):
        return getattr(self.ctx, "%s_%s" % (self._api, name))

    def _check_env(self, env):
        if not env.continuous:
            raise ValueError("DDPG needs the continuous action space (sumo-jerk-continuous-v0)")

    def _check_cfgs(self, env):
        for c in self.cfgs:
            if c.n_obs != env.obs_dim:
                raise ValueError("cfg.n_obs is %d, the observation has %d entries" % (c.n_obs, env.obs_dim))

    def _default_rates(self):
        self._lr_q, self._lr_pi = np.array([c.lr_q for c in self.cfgs]), np.array([c.lr_pi for c in self.cfgs])

    def _create_handle(self):
        return self._call("create")([c.to_c(s) for c, s in zip(self.cfgs, self.seeds)])

    def _make_member(self, m, env, init):
        return _PopulationMember(self, m, env, self.cfgs[m], self.seeds[m], init)

    def __init__(self, env, cfgs, seeds=None, init=None, ctx=None, per=None):
        if isinstance(cfgs, tuple) and len(cfgs) == 2 and isinstance(cfgs[0], self._cfg_type):
            cfgs = [cfgs[0]] * int(cfgs[1])
        self.cfgs = list(cfgs)
        P = self.P = len(self.cfgs)
        for m, c in enumerate(self.cfgs):
            if getattr(c, "per", None) is not None:
                raise ValueError("member %d's cfg asks for prioritised replay (per=): a population enables it for its members itself; give the "
                                 "PERConfig to the population's per= argument (one for all members, or a list with one entry per member)" % m)
        if per is None or isinstance(per, PERConfig):
            per = [per] * P
        elif not isinstance(per, (list, tuple)):
            raise ValueError("per must be None, a PERConfig, or a list with a PERConfig or None per member")
        self.per = list(per)
        if len(self.per) != P:
            raise ValueError("per has %d entries, the population %d members" % (len(self.per), P))
        for m, g in enumerate(self.per):
            if g is not None and not isinstance(g, PERConfig):
                raise ValueError("per[%d] is a %s, not a PERConfig or None" % (m, type(g).__name__))
        self._check_env(env)
        # (a member count outside 1 ... DDPG_POP_MAX is the library's to refuse)
        if 1 <= P <= _capi.DDPG_POP_MAX and env.n % P:
            raise ValueError("env.n = %d is not a multiple of the population's %d members" % (env.n, P))
        if getattr(env, "sim_cfgs", None) is not None and env.G != P:
            # (equal sizes: G == P makes group m's environments member m's)
            raise ValueError("the env has %d traffic groups, the population %d members: member m trains on traffic m, so they must coincide" % (env.G, P))
        if getattr(env, "R", 0) and env.R != P:
            # (equal sizes: R == P makes reward group m's environments member m's, n_per_member == n_per_reward_group)
            raise ValueError("the env has %d reward groups, the population %d members: member m trains under reward m, so they must coincide" % (env.R, P))
        self.seeds = list(range(P)) if seeds is None else [int(x) for x in seeds]
        inits = list(init) if isinstance(init, (list, tuple)) else [init] * P
        if len(self.seeds) != P or len(inits) != P:
            raise ValueError("seeds and init (if a list) have one entry per member")
        self._check_cfgs(env)
        import torch
        self.torch = torch
        self.env_n, self.n_per_member = env.n, (env.n // P if P >= 1 else 0)
        self.ctx = ctx if ctx is not None else env.ctx
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.handle = self._create_handle()
        if any(c.n_step > 1 for c in self.cfgs):                    # (the rings are empty; member m forms cfgs[m].n_step-step returns from pushes of n_per_member rows)
            self.ctx.pop_nstep_enable(self._nstep_kind, self.handle, [c.to_c_nstep(self.n_per_member) for c in self.cfgs])
        if any(g is not None for g in self.per):                    # (the rings are empty: nothing was pushed yet)
            self._call("per_enable")(self.handle, [g.to_c() if g is not None else None for g in self.per])
        self._members = [self._make_member(m, env, inits[m]) for m in range(P)]
        self._default_rates()
        self._stats = torch.zeros(P, len(self._stat_keys), dtype=torch.float64, device=self.device)
        self._actions = torch.empty(env.n, dtype=getattr(torch, self._action_dtype), device=self.device)

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                self._call("destroy")(self.handle)
            except Exception:
                pass
            self.handle = None

    def __len__(self):
        return self.P

    def member(self, m):
        return self._members[m]

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _rows(self, t):
        if t.shape[0] != self.env_n:
            raise ValueError("%d rows given, the population's env has %d" % (t.shape[0], self.env_n))

    def act(self, obs, ticks, noise=True, debug=None):
        """``DDPGLearner.act`` for all members: row e is acted on by member e // n_per_member.  The returned tensor is reused by the next call."""
        self._rows(obs)
        _check_ddpg_act(self.torch, obs, ticks)
        self._call("act")(self.handle, self.n_per_member, obs.data_ptr(), obs.stride(0), ticks.data_ptr(), noise, self._actions.data_ptr(),
                          debug.data_ptr() if debug is not None else 0, self._stream())
        return self._actions

    def push(self, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs=None, next_ticks=None):
        """``DDPGLearner.push`` for all members: each member's slice of the step goes into its own ring."""
        self._rows(obs)
        _check_ddpg_push(self.torch, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs)
        self._call("push")(self.handle, self.n_per_member, obs.data_ptr(), next_obs.data_ptr(), final_obs.data_ptr() if final_obs is not None else 0,
                           obs.stride(0), ticks.data_ptr(), next_ticks.data_ptr() if next_ticks is not None else 0, action.data_ptr(), reward.data_ptr(),
                           terminated.data_ptr(), truncated.data_ptr(), self._stream())

    def _lr(self, lr, default):
        return per_member(lr, self.P, default)

    def update(self, n=1, lr_q=None, lr_pi=None):
        """``n`` updates of every member, six launches each (eight with prioritised members); a member whose replay_start gate is still shut skips its own.  ``lr_q`` / ``lr_pi``:
        a scalar or one value per member (default: each member's cfg's)."""
        self._call("update")(self.handle, n, self._lr(lr_q, self._lr_q), self._lr(lr_pi, self._lr_pi), self._stream())

    def stats_device(self):
        """fp64 [P][4] device tensor ([P][6] of a ``TD3Population``): per member, the lone learner's row -- the loss(es) and mean Q(s, a) of the last
        minibatch, fill, updates done (asynchronous)."""
        self._call("stats")(self.handle, self._stats.data_ptr(), self._stream())
        return self._stats

    def stats(self):
        """The same as a dict of arrays of length P with the lone learner's keys (``TD3Learner.stats_td3``'s of a ``TD3Population``); synchronises."""
        return _stats_dict(self._stat_keys, self.stats_device().cpu().numpy())


class _TD3PopulationMember(_Borrowed, TD3Learner):
    """One member of a ``TD3Population`` as a ``TD3Learner`` (``stmpc_pop_td3_member``): the TD3 handle is borrowed, and so is its base."""


def _is_net_triple(x):
    return isinstance(x, (tuple, list)) and len(x) == 3 and isinstance(x[0], dict) and "w0" in x[0]


class TD3Population(DDPGPopulation):
    """P independent TD3 learners on one ``MergeVecEnv``, advanced together: ``DDPGPopulation`` for ``TD3Learner`` (``csrc/stmpc_td3_pop_kernels.hpp``,
    ``stmpc_pop_td3_*``): six launches per update whatever P is.  The members share n_obs, h1, h2, batch and capacity and may differ in everything
    else -- ``target_noise``, ``noise_clip``, ``policy_delay``, ``replay_start``, gamma, tau, seed, learning rates: whether a member is gated, or
    its delayed half due, is decided on the device from its own counters.

    ``cfgs``: a list of ``TD3Config`` or ``(TD3Config, P)`` (a plain ``DDPGConfig`` is refused).  ``init``: as ``TD3Learner``'s -- a dict, or an
    (actor, critic, critic 2) triple of nets -- for every member, or a list of P of those.  Member m starts exactly as
    ``TD3Learner(seed=seeds[m], init=...)`` does, critic 2's fresh draw included, and stays bit-identical to that learner driven on its slice alone.
    ``act`` / ``push`` / ``update`` and what ``DDPGPopulation`` says about traffic and reward groups hold unchanged; ``stats_device`` is fp64 [P][6]
    and ``stats`` has the keys of ``TD3Learner.stats_td3``; ``member(m)`` is a ``TD3Learner`` view (``grads``, ``targets``, ``stats_td3``,
    ``state_dict`` / ``load_state_dict`` with all twelve slots and six beta powers, ``export_actor``).  ``train_ddpg``, ``evaluate_members`` and
    ``actor.ActorPopulation`` take it as they take a ``DDPGPopulation``.  ``per``: as ``DDPGPopulation``'s; a prioritised member's priorities follow
    the critic with the larger error, as ``TD3Learner``'s do."""

    _api, _stat_keys = "td3_pop", _TD3_STATS
    _nstep_kind = "td3"

    def __init__(self, env, cfgs, seeds=None, init=None, ctx=None, per=None):
        if isinstance(cfgs, tuple) and len(cfgs) == 2 and isinstance(cfgs[0], DDPGConfig):
            cfgs = [cfgs[0]] * int(cfgs[1])
        cfgs = list(cfgs)
        for m, c in enumerate(cfgs):
            if not isinstance(c, TD3Config):
                raise ValueError("member %d's cfg is a %s, not a TD3Config: a TD3Population takes TD3Configs (a plain DDPGConfig has no target_noise, "
                                 "noise_clip or policy_delay)" % (m, type(c).__name__))
        if _is_net_triple(init):                                    # one triple for every member, not a list of three members
            init = [init] * len(cfgs)
        super().__init__(env, cfgs, seeds=seeds, init=init, ctx=ctx, per=per)

    def _create_handle(self):
        return self._call("create")([c.to_c_td3(s) for c, s in zip(self.cfgs, self.seeds)])

    def _make_member(self, m, env, init):
        return _TD3PopulationMember(self, m, env, self.cfgs[m], self.seeds[m], init)


# ---- DQN: the discrete agent (csrc/stmpc_dqn_kernels.hpp, stmpc_dqn_*) ---------------------------------------------------------------------------
DQN_TENSORS = ("w0", "b0", "w1", "b1")
DQN_STREAM = 0x64716E657870


class DQNConfig:
    """The constants of the DQN update; defaults are the reference's config.py (hidden_size 256 of ``DQN()``, BATCH_SIZE, REPLAY_BUFFER_SIZE,
    DISCOUNT_FACTOR, LEARNING_RATE, TARGET_NET_FREEZE_PERIOD -- counted in updates here, in episodes there --, DOUBLE_DQN, CLIP_MIN_REWARD /
    CLIP_MAX_REWARD; Adam: ``optim.Adam``'s defaults).  ``n_actions`` None: the env's.  ``per``: a ``PERConfig`` for prioritised replay
    (USE_PRIORITIZED_ER), None: uniform minibatches."""

    def __init__(self, n_obs=20, n_actions=None, h1=256, batch=50, capacity=50000, replay_start=0, gamma=0.999, lr=2e-4, target_period=500, double=True,
                 clip_targets=False, clip_min=-20.0, clip_max=10.0, beta1=0.9, beta2=0.999, eps=1e-8, per=None, n_step=1):
        if per is not None and not isinstance(per, PERConfig):
            raise ValueError("per must be a PERConfig or None")
        self.per = per
        self.n_step = _check_n_step(n_step)                         # multi-step returns; travels beside ``to_c``: ``to_c_nstep``
        self.n_obs, self.n_actions, self.h1, self.batch = int(n_obs), (None if n_actions is None else int(n_actions)), int(h1), int(batch)
        self.capacity, self.replay_start, self.target_period = int(capacity), int(replay_start), int(target_period)
        self.gamma, self.lr, self.beta1, self.beta2, self.eps = float(gamma), float(lr), float(beta1), float(beta2), float(eps)
        self.double, self.clip_targets, self.clip_min, self.clip_max = bool(double), bool(clip_targets), float(clip_min), float(clip_max)

    def to_c(self, seed):
        return _capi.DQNCfg(n_obs=self.n_obs, h1=self.h1, n_actions=self.n_actions, batch=self.batch, capacity=self.capacity, target_period=self.target_period,
                            double_dqn=int(self.double), clip_targets=int(self.clip_targets), replay_start=self.replay_start, seed=int(seed) & _M64,
                            gamma=self.gamma, beta1=self.beta1, beta2=self.beta2, eps=self.eps, clip_min=self.clip_min, clip_max=self.clip_max)

    def to_c_nstep(self, rows_per_push):
        return nstep_to_c(self, rows_per_push)


def dqn_epsilon(iteration, eps_start=1.0, eps_end=0.1, decay_coefficient=0.25, decay_rate=30000):
    """The reference's exploration schedule (dqn.py:275-276; EPS_START, EPS_END, EPS_DECAY_COEFFICIENT, EPS_DECAY_RATE of config.py)."""
    return eps_end + (eps_start - eps_end) * math.exp(-decay_coefficient * math.floor(iteration / decay_rate))


def dqn_act_host(seed, call, n, eps, A):
    """Exploring acting call ``call``, rows 0 .. n-1: (explore bool [n], index int32 [n]) -- ``k_dqn_act``'s draws in integer arithmetic: u = the
    hash's top 24 bits / 2^24 < float32(eps), the index the hash's next 24 bits modulo ``A``.  ``eps`` 0: no row explores (and the device draws nothing)."""
    bound = float(np.float32(eps)) * 2.0 ** 24                      # (exact: a float32 times a power of two)
    explore, idx = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int32)
    for e in range(n):
        h = hash3((int(seed) & _M64) ^ DQN_STREAM, call, e)
        explore[e] = eps > 0 and (h >> 40) < bound
        idx[e] = ((h >> 16) & 0xFFFFFF) % int(A)
    return explore, idx


def init_q_net(n_obs, h1, A, rng):
    """torch's nn.Linear initialisation (uniform +-1/sqrt(fan_in) for weight and bias) of both layers, as the reference's ``DQN()`` has it."""
    u = lambda fan_in, *sh: rng.uniform(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in), size=sh).astype(np.float32)
    return {"w0": u(n_obs, h1, n_obs), "b0": u(n_obs, h1), "w1": u(h1, A, h1), "b1": u(h1, A)}


def flatten_q(net):
    return np.concatenate([np.asarray(net[k], dtype=np.float32).reshape(-1) for k in DQN_TENSORS])


def unflatten_q(flat, n_obs, h1, A):
    out, o = {}, 0
    for k, sh in zip(DQN_TENSORS, ((h1, n_obs), (h1,), (A, h1), (A,))):
        n = int(np.prod(sh))
        out[k] = np.array(flat[o:o + n]).reshape(sh)
        o += n
    assert o == len(flat)
    return out


def new_params_dqn(q_net):
    """The learner's whole parameter state for a given online net: the target a copy, Adam's moments zero, beta powers 1, no updates."""
    cp = lambda: {k: np.array(q_net[k], dtype=np.float32) for k in DQN_TENSORS}
    zero = lambda: {k: np.zeros_like(np.asarray(q_net[k], dtype=np.float32)) for k in DQN_TENSORS}
    return {"q": cp(), "q_target": cp(), "q_m": zero(), "q_v": zero(), "beta_pow": np.ones(2, dtype=np.float32), "updates": 0}


def dqn_batch_from_rows(rows, n_obs):
    """Replay rows [B][68] of a DQN learner -> the minibatch dict ``update_host_dqn`` takes."""
    return {"s": rows[:, :n_obs], "a": rows[:, _capi.DQN_ACTION_COL].astype(np.int64), "s2": rows[:, 32:32 + n_obs], "r": rows[:, 64], "mask": rows[:, 65]}


def _q_mlp(t, x):
    import torch
    return torch.relu(x @ t["w0"].T + t["b0"]) @ t["w1"].T + t["b1"]


def dqn_targets_host(params, batch, cfg, dtype="float64", disc=None):
    """``get_targets`` (dqn.py:673-705) in torch, every tensor in ``dtype``: [B][3] = a* (``cfg.double``: the first argmax of the online net on s';
    else the target net's), the target net's Q(s') there, y = r + clip(gamma * that), r alone on a terminated row.  ``disc``: the discount per
    row in ``cfg.gamma``'s place (``nstep_batch_host``'s gamma^m; None: ``cfg.gamma``)."""
    import torch
    td = getattr(torch, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=td)
    with torch.no_grad():
        s2, r, mask = T(batch["s2"]), T(batch["r"]), T(batch["mask"])
        qt = _q_mlp({k: T(params["q_target"][k]) for k in DQN_TENSORS}, s2)
        astar = torch.argmax(_q_mlp({k: T(params["q"][k]) for k in DQN_TENSORS}, s2) if cfg.double else qt, dim=1, keepdim=True)
        qsel = torch.gather(qt, 1, astar).flatten()
        g = (cfg.gamma if disc is None else T(disc)) * qsel
        if cfg.clip_targets:
            g = torch.clamp(g, cfg.clip_min, cfg.clip_max)
        y = torch.where(mask != 0, r + g, r)
    return torch.stack([astar.flatten().to(td), qsel, y], 1).numpy()


def update_host_dqn(params, batch, cfg, dtype="float64", weights=None, grads_only=False, lr=None, disc=None):
    """One DQN update in torch with autograd, every tensor in ``dtype`` ("float64" or "float32"): the targets of ``dqn_targets_host``, the
    SmoothL1 loss (beta 1) of Q(s)[a] against them as a mean over the minibatch -- ``weights``: prioritised replay's importance weight per row,
    multiplying that row's term --, one bias-corrected Adam step, and the hard copy of the target if the new update count is a multiple of
    ``cfg.target_period``.  ``params``: as ``new_params_dqn`` / ``DQNLearner.state_dict()["params"]``; returns the new one and a dict with ``loss``
    (unweighted), ``mean_q``, ``q_values``, ``td`` (Q(s, a) - y), ``targets`` ([B][3]) and ``grad``.  ``grads_only``: nothing is applied.
    ``disc``: as ``dqn_targets_host``'s."""
    import torch
    td = getattr(torch, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=td)
    P = {slot: {k: T(params[slot][k]) for k in DQN_TENSORS} for slot in _capi.DQN_SLOTS}
    tg = dqn_targets_host(params, batch, cfg, dtype, disc=disc)
    y = T(tg[:, 2])
    net = {k: P["q"][k].clone().requires_grad_(True) for k in DQN_TENSORS}
    q = torch.gather(_q_mlp(net, T(batch["s"])), 1, torch.tensor(np.asarray(batch["a"], dtype=np.int64))[:, None]).flatten()
    terms = torch.nn.functional.smooth_l1_loss(q, y, reduction="none", beta=1.0)
    loss = terms.mean()
    grads = dict(zip(DQN_TENSORS, torch.autograd.grad(loss if weights is None else (T(weights) * terms).mean(), [net[k] for k in DQN_TENSORS])))
    u = int(params["updates"])
    if not grads_only:
        t = u + 1
        bc1, bc2 = 1.0 - cfg.beta1 ** t, 1.0 - cfg.beta2 ** t
        for k in DQN_TENSORS:
            m = cfg.beta1 * P["q_m"][k] + (1 - cfg.beta1) * grads[k]
            v = cfg.beta2 * P["q_v"][k] + (1 - cfg.beta2) * grads[k] * grads[k]
            P["q_m"][k], P["q_v"][k] = m, v
            P["q"][k] = P["q"][k] - ((cfg.lr if lr is None else lr) / bc1) * m / (v.sqrt() / math.sqrt(bc2) + cfg.eps)
            if t % cfg.target_period == 0:
                P["q_target"][k] = P["q"][k].clone()
    out = {slot: {k: P[slot][k].detach().numpy() for k in DQN_TENSORS} for slot in _capi.DQN_SLOTS}
    out["beta_pow"] = np.array(params["beta_pow"], dtype=np.float32) * (1 if grads_only else np.array([cfg.beta1, cfg.beta2], dtype=np.float32))
    out["updates"] = u + (0 if grads_only else 1)
    info = {"loss": float(loss.detach()), "mean_q": float(q.detach().mean()), "q_values": q.detach().numpy(), "td": (q.detach() - y).numpy(), "targets": tg,
            "grad": {k: grads[k].numpy() for k in DQN_TENSORS}}
    return out, info


def dqn_adam_host(w, g, m, v, beta_pow, lr, cfg):
    """``k_dqn_adam``'s step for one tensor (or one flat slot) in numpy float32, operation for operation: (w, m, v, beta_pow) after it."""
    f = np.float32
    w, g, m, v = (np.asarray(x, dtype=f) for x in (w, g, m, v))
    b1, b2, eps = f(cfg.beta1), f(cfg.beta2), f(cfg.eps)
    pw1, pw2 = f(beta_pow[0]) * b1, f(beta_pow[1]) * b2
    step, bc2s = f(lr) / (f(1) - pw1), np.sqrt(f(1) - pw2)
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * (g * g)
    return w - step * (m / (np.sqrt(v) / bc2s + eps)), m, v, np.array([pw1, pw2], dtype=f)


class _QLearner(_Learner):
    """What ``DQNLearner`` and ``C51Learner`` share: everything but the head.  A subclass names itself for the refusals (``_name``), the cfg a learner
    made without one gets (``_cfg_type``), the network's output width as its factors (``_out_shape``) and the net a learner made without one starts
    from (``_init_net``); ``_check_cfg_type`` and ``_check_width`` are the two halves of a head's own cfg check, each where its refusal always came."""

    _cfg_type = None

    def _check_cfg_type(self):
        pass

    def _check_width(self):
        pass

    def __init__(self, env_or_dims, cfg=None, seed=0, init=None, ctx=None, rows_per_push=None):
        env = None if isinstance(env_or_dims, (tuple, list)) else env_or_dims
        if env is not None and env.continuous:
            raise ValueError(self._name + " needs a discrete action space (sumo-jerk-v0 or sumo-accel-v0), not the continuous jerk env")
        n_obs, A = (env.obs_dim, int(env.action_space["n"])) if env is not None else (int(env_or_dims[0]), int(env_or_dims[1]))
        self.cfg = cfg if cfg is not None else self._cfg_type(n_obs=n_obs)
        self._check_cfg_type()
        if self.cfg.n_actions is None:
            self.cfg.n_actions = A
        if self.cfg.n_obs != n_obs or self.cfg.n_actions != A:
            raise ValueError("cfg has n_obs %d and %d actions; the observation has %d entries and there are %d actions" % (self.cfg.n_obs, self.cfg.n_actions, n_obs, A))
        for name, ok in (("n_actions in 1 ... 256", 1 <= A <= 256), ("n_obs in 1 ... 31", 1 <= n_obs <= 31), ("batch >= 1", self.cfg.batch >= 1),
                         ("target_period >= 1", self.cfg.target_period >= 1)):
            if not ok:
                raise ValueError(self._name + " needs " + name)
        self._check_width()
        # the env's table, index -> jerk or acceleration (what its cfg hands the library); without an env the indices stand for themselves
        self.action_values = np.array(env.cfg._actions, dtype=np.float64) if env is not None else np.arange(A, dtype=np.float64)
        self.env_id = getattr(env, "env_id", None)                    # (what actor.DQNActor.from_learner's default mode reads; None without an env)
        if self.action_values.shape != (A,):
            raise ValueError("the env's action table has %d entries, its action space %d" % (self.action_values.size, A))
        import torch
        self.torch = torch
        self.ctx = ctx if ctx is not None else (env.ctx if env is not None else _capi.Context(-1))
        self.seed = int(seed)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.handle = self._make_handle()
        self._enable_nstep(env, rows_per_push)
        if self.cfg.per is not None:                                # (a population member's handle refuses: the population enables its members)
            self._call("per_enable")(self.handle, self.cfg.per.to_c())
        c, out = self.cfg, self._out_shape()
        self._n_out = int(np.prod(out))
        net = init if init is not None else self._init_net(np.random.default_rng(self.seed))
        self._len = flatten_q(net).size
        if self._len != (c.n_obs + 1) * c.h1 + (c.h1 + 1) * self._n_out:
            raise ValueError("the net's tensors do not have the shape %d -> %d -> %s" % (c.n_obs, c.h1, " * ".join("%d" % f for f in out)))
        self.load_state_dict({"params": new_params_dqn(net), "counters": None})
        self._stats = torch.zeros(4, dtype=torch.float64, device=self.device)
        self._actions = {}

    def _create(self):
        return self._call("create")(self.cfg.to_c(self.seed))

    def _slot(self, i):
        return unflatten_q(self._call("get_params")(self.handle, i, self._len), self.cfg.n_obs, self.cfg.h1, self._n_out)

    # -- acting / replay / update: asynchronous ---------------------------------------------------------------------------------------------
    def act(self, obs, ticks=None, eps=0.0, debug_q=None):
        """Action indices int32 [n] (what ``MergeVecEnv.step`` takes) for observations float32 [n][n_obs]: the first maximum of Q(obs) -- of a
        categorical learner, of the expected values E[Z(obs, a)] --; with ``eps`` > 0 a row explores with that probability and then takes a uniform
        index (``dqn_act_host``).  ``ticks`` is accepted for ``DDPGLearner``'s signature and not read: the network has no time feature.  The
        returned tensor is reused by the next call with the same n.  ``debug_q``: float32 [n][n_actions] device tensor for Q(obs) (the expected
        values)."""
        n = obs.shape[0]
        out = self._out(n, self.torch.int32)
        _check_q_act(self.torch, obs, debug_q, self.cfg.n_actions)
        self._call("act")(self.handle, n, obs.data_ptr(), obs.stride(0), eps, out.data_ptr(), debug_q.data_ptr() if debug_q is not None else 0, self._stream())
        return out

    def push(self, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs=None, next_ticks=None):
        """One env step into the replay ring: ``obs`` as given to ``act``, ``action`` int32 [n], and what ``env.step`` returned
        (``final_obs = info["final_observation"]``: s' where an episode ended).  ``ticks`` / ``next_ticks`` are not read."""
        _check_q_push(self.torch, obs, action, reward, next_obs, terminated, truncated, final_obs)
        self._call("push")(self.handle, obs.shape[0], obs.data_ptr(), next_obs.data_ptr(), final_obs.data_ptr() if final_obs is not None else 0, obs.stride(0),
                           action.data_ptr(), reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), self._stream())

    def update(self, n=1, lr=None):
        """``n`` updates; on the device nothing happens until more than cfg.replay_start frames were pushed.  ``lr``: this call's learning rate."""
        self._call("update")(self.handle, n, self.cfg.lr if lr is None else lr, self._stream())

    def grads(self):
        """Debug: the loss's gradient on the current update index's minibatch as a dict of numpy tensors; nothing applied; synchronises."""
        g = self.torch.empty(self._len, dtype=self.torch.float32, device=self.device)
        self._call("grads")(self.handle, g.data_ptr(), self._stream())
        return unflatten_q(g.cpu().numpy(), self.cfg.n_obs, self.cfg.h1, self._n_out)

    def targets(self):
        """Debug: float32 [batch][4] of the minibatch the next update will draw -- DQN: a*, the target net's Q(s') there, y, Q(s, a); C51: a*, the
        target net's expected value there, the row loss l, Q(s, a) --; synchronises."""
        out = self.torch.zeros(self.cfg.batch, 4, dtype=self.torch.float32, device=self.device)
        self._call("targets")(self.handle, out.data_ptr(), self._stream())
        return out.cpu().numpy()

    def stats(self):
        """``stats_device`` as a dict; synchronises."""
        return _stats_dict(_DQN_STATS, self.stats_device().cpu().numpy())


class DQNLearner(_QLearner):
    """DQN on the device for the discrete-action envs (``MergeVecEnv("sumo-jerk-v0")``, ``"sumo-accel-v0"``): the reference's TRAIN_DQN
    (dqn.py:257-359) with ``DDPGLearner``'s interface.  ``env_or_dims``: such an env (its context, observation width, action count and action table
    are taken over) or ``(n_obs, n_actions)``.  ``init``: None (torch's nn.Linear initialisation) or a net {w0, b0, w1, b1}.
    One update is three HIP launches (five with ``cfg.per``); acting, pushing and updating never synchronise with the host.
    ``rows_per_push``: as ``DDPGLearner``'s."""

    _api, _per_api, _slots, _flatten = "dqn", "dqn_per", _capi.DQN_SLOTS, staticmethod(flatten_q)
    _name, _cfg_type = "DQN", DQNConfig

    def _out_shape(self):
        return (self.cfg.n_actions,)

    def _init_net(self, rng):
        return init_q_net(self.cfg.n_obs, self.cfg.h1, self.cfg.n_actions, rng)

    def export_q(self, path):
        """Write the online Q-network as an ``.npz``: w0, b0, w1, b1 (float32) and ``action_values`` (the env's table, index -> jerk or acceleration)."""
        with open(path, "wb") as fh:
            np.savez_compressed(fh, **self._slot(0), action_values=self.action_values)
        return path


class _DQNPopulationMember(_Borrowed, DQNLearner):
    """One member of a ``DQNPopulation`` as a ``DQNLearner`` (``stmpc_pop_dqn_member``)."""


class DQNPopulation(DDPGPopulation):
    """P independent DQN learners on one discrete-action ``MergeVecEnv`` (``sumo-jerk-v0``, ``sumo-accel-v0``), advanced together: three launches
    per update whatever P is (five when at least one member is prioritised), one each for acting, pushing and the statistics
    (``csrc/stmpc_dqn_pop_kernels.hpp``, ``stmpc_pop_dqn_*``).  The reference trains its DQN agent one TRAIN_DQN run (dqn.py:257-359) at a time; what
    it compares between runs -- double against plain targets, clipped against unclipped ones, TARGET_NET_FREEZE_PERIOD, the epsilon schedule,
    prioritised against uniform replay, seeds, traffic types, reward settings -- is a population's members side by side.

    ``cfgs``: a list of ``DQNConfig`` or ``(cfg, P)``; the members share n_obs, h1, n_actions, batch and capacity and may differ in everything
    else.  ``env.n`` must be ``P * n_per_member``: member m owns environments [m * n_per_member, (m + 1) * n_per_member).  ``seeds``: one per
    member (None: 0 .. P-1); ``init``: as ``DQNLearner``'s, for every member, or a list of P.  Member m starts exactly as
    ``DQNLearner(seed=seeds[m], init=...)`` does and stays bit-identical to that learner driven on its slice alone.  Traffic groups and reward
    groups: as ``DDPGPopulation``'s (as many as members; member m trains on traffic m, under reward m).  ``per``: as ``DDPGPopulation``'s -- None,
    one ``PERConfig``, or a list of P entries, each a ``PERConfig`` or None; a cfg that carries ``per=`` is refused.

    ``act`` / ``push`` / ``update`` / ``stats_device`` / ``stats`` are ``DQNLearner``'s on the whole env's tensors, with ``eps`` and ``lr`` a scalar
    or one value per member.  A member whose eps is 0 draws nothing and its acting counter stays, as the lone learner's under ``eps=0``.
    ``member(m)`` is a ``DQNLearner`` view: ``state_dict`` / ``load_state_dict``, ``grads``, ``targets``, ``minibatch``, ``priorities``,
    ``last_sample``, ``export_q``, ``actor.DQNActor.from_learner(pop.member(m), ...)`` and ``evaluate_dqn(pop.member(m), ...)`` work on it.
    ``train_dqn`` takes a population.  ``evaluate_dqn_members(pop, n_per_member)`` evaluates all members' Q-networks in one launch per tick
    (``actor.QActorPopulation``)."""

    _api, _stat_keys = "dqn_pop", _DQN_STATS
    _nstep_kind = "dqn"
    _cfg_type, _action_dtype = DQNConfig, "int32"

    def _check_env(self, env):
        if env.continuous:
            raise ValueError("DQN needs a discrete action space (sumo-jerk-v0 or sumo-accel-v0), not the continuous jerk env")

    def _check_cfgs(self, env):
        A = int(env.action_space["n"])
        for m, c in enumerate(self.cfgs):
            if c.n_actions is None:
                c.n_actions = A
            if c.n_obs != env.obs_dim or c.n_actions != A:
                raise ValueError("member %d's cfg has n_obs %d and %d actions; the observation has %d entries and there are %d actions"
                                 % (m, c.n_obs, c.n_actions, env.obs_dim, A))

    def _default_rates(self):
        self._lr_default = np.array([c.lr for c in self.cfgs])

    def _make_member(self, m, env, init):
        return _DQNPopulationMember(self, m, env, self.cfgs[m], self.seeds[m], init)

    def act(self, obs, ticks=None, eps=0.0, debug_q=None):
        """``DQNLearner.act`` for all members: row e is acted on by member e // n_per_member; int32 [env.n], reused by the next call.  ``eps``: a
        scalar or one value per member.  ``debug_q``: float32 [env.n][n_actions]."""
        self._rows(obs)
        _check_q_act(self.torch, obs, debug_q, self.cfgs[0].n_actions)
        self._call("act")(self.handle, self.n_per_member, obs.data_ptr(), obs.stride(0), per_member(eps, self.P), self._actions.data_ptr(),
                          debug_q.data_ptr() if debug_q is not None else 0, self._stream())
        return self._actions

    def push(self, obs, ticks, action, reward, next_obs, terminated, truncated, final_obs=None, next_ticks=None):
        """``DQNLearner.push`` for all members: each member's slice of the step goes into its own ring."""
        self._rows(obs)
        _check_q_push(self.torch, obs, action, reward, next_obs, terminated, truncated, final_obs)
        self._call("push")(self.handle, self.n_per_member, obs.data_ptr(), next_obs.data_ptr(), final_obs.data_ptr() if final_obs is not None else 0,
                           obs.stride(0), action.data_ptr(), reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), self._stream())

    def update(self, n=1, lr=None):
        """``n`` updates of every member, three launches each (five with prioritised members); a member whose replay_start gate is still shut skips
        its own.  ``lr``: a scalar or one value per member (default: each member's cfg's)."""
        self._call("update")(self.handle, n, self._lr(lr, self._lr_default), self._stream())


# ---- C51: the categorical DQN agent (csrc/stmpc_c51_kernels.hpp, stmpc_c51_*) ---------------------------------------------------------------------
class NoisyConfig:
    """The noisy output layer of a C51 learner (``C51Config(noisy=...)``): sigma starts at ``sigma0 / sqrt(h1)`` everywhere.  0.5 is the paper's
    (Fortunato et al. 2018, section 3.2); the ``all`` rainbow preset's own value could not be read (the library is absent from the reference
    checkout).  ``sigma0 = 0`` starts from the mean network (sigma still learns)."""

    def __init__(self, sigma0=0.5):
        self.sigma0 = float(sigma0)
        if not (math.isfinite(self.sigma0) and self.sigma0 >= 0):
            raise ValueError("NoisyConfig needs a finite sigma0 >= 0, not %r" % (sigma0,))


NOISY_LEARN_STREAM, NOISY_ACT_STREAM = 0x6E7A6C726E, 0x6E7A616374     # C51_NOISY_LEARN_STREAM, C51_NOISY_ACT_STREAM of csrc/stmpc_c51_noisy_kernels.hpp
NOISY_TENSORS = ("w1", "b1")                                          # what a sigma slot holds


def c51_noisy_f_host(seed, draw, h1, n_out, stream=NOISY_LEARN_STREAM):
    """(f_in float32 [h1], f_out float32 [n_out]) of noise draw ``draw``: f(e) = sign(e) sqrt|e| of ``noise_host``'s Gaussians, variate k < h1 for
    e_in and h1 + n for e_out -- the Gaussian rounded to float32 as the kernel holds it, f formed in float64 and rounded to float32 once.  The learning
    stream's draw is 2 * update + net (0 online, 1 target); the acting stream's (``NOISY_ACT_STREAM``) the learner's acting-draw counter."""
    e = noise_host(seed, draw, int(h1) + int(n_out), stream=stream)[2].astype(np.float32).astype(np.float64)
    f = (np.sign(e) * np.sqrt(np.abs(e))).astype(np.float32)
    return f[:h1], f[h1:]


def c51_noisy_compose_host(mu, sigma, f_in, f_out):
    """``k_c51_noisy_compose``'s effective output layer in numpy, operation for operation: {w1, b1} float32 from float32 ``mu`` {w1 [n_out][h1], b1},
    ``sigma`` likewise and the float32 f vectors -- W_eff = float32(mu + sigma * (f_out * f_in)) in float64 (the inner product is exact there, the
    other two operations round), b_eff = float32(mu_b + sigma_b * f_out)."""
    d = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    fo, fi = d(f_out), d(f_in)
    return {"w1": (d(mu["w1"]) + d(sigma["w1"]) * (fo[:, None] * fi[None, :])).astype(np.float32), "b1": (d(mu["b1"]) + d(sigma["b1"]) * fo).astype(np.float32)}


def _c51_noisy_effective(net, sigma, f_in, f_out):
    """The effective net of torch tensors: the mathematical statement in the tensors' dtype."""
    return {"w0": net["w0"], "b0": net["b0"], "w1": net["w1"] + sigma["w1"] * (f_out[:, None] * f_in[None, :]), "b1": net["b1"] + sigma["b1"] * f_out}


def update_host_c51_noisy(params, batch, cfg, f, dtype="float64", weights=None, grads_only=False, lr=None, disc=None):
    """``update_host_c51`` for a learner with the noisy output layer, every tensor in ``dtype``.  ``params``: the four slots and ``sigma``,
    ``sigma_target``, ``sigma_m``, ``sigma_v`` ({w1, b1} each); ``f``: {"online": (f_in, f_out), "target": (f_in, f_out)}, the draws' f vectors
    (inputs: ``c51_noisy_f_host``'s or the device's).  The target side runs on the effective target net (and, ``cfg.double``, the effective online
    one); the loss on the effective online net with mu and sigma as autograd's leaves; Adam steps both and the hard copy copies both.  Returns the
    new params and ``update_host_c51``'s info with ``grad`` = g_mu and ``grad_sigma`` = g_sigma."""
    import torch
    td = getattr(torch, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=td)
    A, K, B = cfg.n_actions, cfg.n_atoms, len(batch["r"])
    duel = bool(getattr(cfg, "dueling", False))
    slots = tuple(_capi.C51_SLOTS)
    P = {slot: {k: T(params[slot][k]) for k in DQN_TENSORS} for slot in slots}
    S = {slot: {k: T(params[slot][k]) for k in NOISY_TENSORS} for slot in _capi.NOISY_SLOTS}
    fo = {net: (T(f[net][0]), T(f[net][1])) for net in ("online", "target")}
    with torch.no_grad():
        eff = {"q": {k: v.numpy() for k, v in _c51_noisy_effective(P["q"], S["sigma"], *fo["online"]).items()},
               "q_target": {k: v.numpy() for k, v in _c51_noisy_effective(P["q_target"], S["sigma_target"], *fo["target"]).items()}}
    tg = c51_targets_host(eff, batch, cfg, dtype, disc=disc)
    m = T(tg["m"])
    mu = {k: P["q"][k].clone().requires_grad_(True) for k in DQN_TENSORS}
    sg = {k: S["sigma"][k].clone().requires_grad_(True) for k in NOISY_TENSORS}
    a = torch.tensor(np.asarray(batch["a"], dtype=np.int64))
    logp = torch.log_softmax(_c51_logits(_c51_noisy_effective(mu, sg, *fo["online"]), T(batch["s"]), A, K, duel), -1)[torch.arange(B), a]
    terms = -(m * logp).sum(-1)
    loss = terms.mean()
    leaves = [mu[k] for k in DQN_TENSORS] + [sg[k] for k in NOISY_TENSORS]
    gl = torch.autograd.grad(loss if weights is None else (T(weights) * terms).mean(), leaves)
    grads, gsig = dict(zip(DQN_TENSORS, gl[:4])), dict(zip(NOISY_TENSORS, gl[4:]))
    u = int(params["updates"])
    if not grads_only:
        t = u + 1
        bc1, bc2 = 1.0 - cfg.beta1 ** t, 1.0 - cfg.beta2 ** t
        for W, M, V, Wt, G, names in ((P["q"], P["q_m"], P["q_v"], P["q_target"], grads, DQN_TENSORS),
                                      (S["sigma"], S["sigma_m"], S["sigma_v"], S["sigma_target"], gsig, NOISY_TENSORS)):
            for k in names:
                M[k] = cfg.beta1 * M[k] + (1 - cfg.beta1) * G[k]
                V[k] = cfg.beta2 * V[k] + (1 - cfg.beta2) * G[k] * G[k]
                W[k] = W[k] - ((cfg.lr if lr is None else lr) / bc1) * M[k] / (V[k].sqrt() / math.sqrt(bc2) + cfg.eps)
                if t % cfg.target_period == 0:
                    Wt[k] = W[k].clone()
    out = {slot: {k: P[slot][k].detach().numpy() for k in DQN_TENSORS} for slot in slots}
    out.update({slot: {k: S[slot][k].detach().numpy() for k in NOISY_TENSORS} for slot in _capi.NOISY_SLOTS})
    out["beta_pow"] = np.array(params["beta_pow"], dtype=np.float32) * (1 if grads_only else np.array([cfg.beta1, cfg.beta2], dtype=np.float32))
    out["updates"] = u + (0 if grads_only else 1)
    p = logp.detach().exp()
    q = (p * T(c51_support(cfg))).sum(-1)
    row_loss = terms.detach().numpy()
    info = {"loss": float(loss.detach()), "mean_q": float(q.mean()), "q_values": q.numpy(), "td": row_loss, "row_loss": row_loss,
            "targets": np.stack([tg["astar"].astype(row_loss.dtype), tg["q_next"], row_loss], 1), "dist": np.stack([tg["m"], p.numpy()], 1),
            "ev_next": tg["ev_next"], "grad": {k: grads[k].numpy() for k in DQN_TENSORS}, "grad_sigma": {k: gsig[k].numpy() for k in NOISY_TENSORS}}
    return out, info


class C51Config(DQNConfig):
    """``DQNConfig`` plus the categorical head's support: ``n_atoms`` atoms z_k = v_min + k (v_max - v_min) / (n_atoms - 1).  The defaults 51, -10, 10 are
    the C51 paper's (Bellemare et al. 2017); the ``all`` rainbow preset's own values could not be read (the library is absent from the reference
    checkout).  ``clip_targets`` / ``clip_min`` / ``clip_max`` are not read: the support's clamp is the clip.

    ``dueling``: the dueling head (Wang et al. 2016, in the categorical form of Hessel et al. 2018, section "Dueling networks").  The network is then
    n_obs -> h1 -> ReLU -> (A + 1) * n_atoms -- the A advantage blocks first, rows a * n_atoms ... of w1 and b1, the value block last -- and the
    logits of action a are l[a][k] = V[k] + Adv[a][k] - mean_b Adv[b][k].  It restates the published head; parity with the ``all`` library's own
    stays unpinned, for the same reason.  The widest layer holds 1024 outputs: ``sumo-accel-v0`` (20 actions) takes at most 48 atoms with it.

    ``noisy``: None, or a ``NoisyConfig`` for factorised-Gaussian noise on the output layer (Fortunato et al. 2018), plain or dueling."""

    def __init__(self, *args, n_atoms=51, v_min=-10.0, v_max=10.0, dueling=False, noisy=None, **kw):
        super().__init__(*args, **kw)
        self.n_atoms, self.v_min, self.v_max, self.dueling = int(n_atoms), float(v_min), float(v_max), bool(dueling)
        if noisy is not None and not isinstance(noisy, NoisyConfig):
            raise ValueError("noisy must be None or a NoisyConfig, not %r" % (noisy,))
        self.noisy = noisy
        if self.n_atoms < 2:
            raise ValueError("C51 needs n_atoms >= 2, not %d" % self.n_atoms)
        if not (math.isfinite(self.v_min) and math.isfinite(self.v_max) and self.v_max > self.v_min):
            raise ValueError("C51 needs a finite support with v_max > v_min, not [%r, %r]" % (self.v_min, self.v_max))
        self.check_width()

    def check_width(self):
        if self.n_actions is not None and (self.n_actions + self.dueling) * self.n_atoms > _capi.C51_MAX_LOGITS:
            raise ValueError("%s * n_atoms = %d * %d exceeds the widest layer, %d"
                             % ("(n_actions + 1)" if self.dueling else "n_actions", self.n_actions + self.dueling, self.n_atoms, _capi.C51_MAX_LOGITS))

    @property
    def n_blocks(self):
        """The output layer's blocks of n_atoms rows: n_actions, and the value block of a dueling head."""
        return self.n_actions + int(self.dueling)

    def to_c(self, seed):
        base = super().to_c(seed)
        return _capi.C51Cfg(v_min=self.v_min, v_max=self.v_max, n_atoms=self.n_atoms, dueling=int(self.dueling), **{n: getattr(base, n) for n, _ in _capi.DQNCfg._fields_})


def c51_support(cfg, dtype=np.float64):
    """The atoms z_k = v_min + k dz [n_atoms], formed in float64 as the kernels form them, then cast to ``dtype``."""
    dz = (cfg.v_max - cfg.v_min) / (cfg.n_atoms - 1)
    return (np.float64(cfg.v_min) + np.arange(cfg.n_atoms, dtype=np.float64) * np.float64(dz)).astype(dtype)


def _c51_positions(r, mask, disc, cfg, dtype):
    """b [n][K]: the positions on the support of the shifted atoms clamp(r + disc z_j, v_min, v_max); r alone where mask == 0 (a select)."""
    f = np.dtype(dtype).type
    r, mask, disc = (np.asarray(x, dtype=dtype).reshape(-1) for x in (r, mask, disc))
    z = c51_support(cfg, dtype)
    t = np.where(mask[:, None] != 0, r[:, None] + disc[:, None] * z[None, :], np.broadcast_to(r[:, None], (r.size, z.size)))
    t = np.clip(t, f(cfg.v_min), f(cfg.v_max))
    return (t - f(cfg.v_min)) / f((cfg.v_max - cfg.v_min) / (cfg.n_atoms - 1))


def c51_project_host(p, r, mask, disc, cfg, dtype="float64"):
    """The categorical projection in gather form, ``c51_project_row`` of csrc/stmpc_c51_kernels.hpp in numpy, every number in ``dtype``:
    m_i = sum_j p_j max(0, 1 - |b_j - i|), the terms added in j order.  ``p`` [n][K]; ``r``, ``mask``, ``disc`` [n].  Right where b_j is an integer."""
    p = np.asarray(p, dtype=dtype)
    b = _c51_positions(r, mask, disc, cfg, dtype)
    i = np.arange(cfg.n_atoms).astype(dtype)
    m = np.zeros_like(p)
    for j in range(cfg.n_atoms):
        m = m + p[:, j:j + 1] * np.maximum(0, 1 - np.abs(b[:, j:j + 1] - i[None, :]))
    return m


def c51_project_scatter_host(p, r, mask, disc, cfg):
    """The textbook statement (Bellemare et al. 2017, Algorithm 1) in float64, one atom at a time: l = floor(b_j), u = ceil(b_j), m_l += p_j (u - b_j),
    m_u += p_j (b_j - l) -- with the customary correction where b_j is an integer (l == u: both weights vanish and the plain loop loses p_j):
    m_l += p_j.  For the suite's comparison only."""
    p = np.asarray(p, dtype=np.float64)
    b = _c51_positions(r, mask, disc, cfg, "float64")
    m = np.zeros_like(p)
    for n in range(p.shape[0]):
        for j in range(cfg.n_atoms):
            lo, up = int(math.floor(b[n, j])), int(math.ceil(b[n, j]))
            if lo == up:
                m[n, lo] += p[n, j]
            else:
                m[n, lo] += p[n, j] * (up - b[n, j])
                m[n, up] += p[n, j] * (b[n, j] - lo)
    return m


def init_c51_net(n_obs, h1, A, n_atoms, rng, dueling=False):
    """``init_q_net`` with A * n_atoms outputs: action a's logits are rows a * n_atoms ... (a + 1) * n_atoms - 1 of w1 and b1.  ``dueling``:
    (A + 1) * n_atoms outputs, the A advantage blocks in those rows and the value block behind them."""
    return init_q_net(n_obs, h1, (A + bool(dueling)) * n_atoms, rng)


def _c51_logits(t, x, A, K, dueling=False):
    """Logits [n][A][K] of a net of torch tensors.  ``dueling``: l[a][k] = V[k] + Adv[a][k] - mean_b Adv[b][k] of the (A + 1) * K outputs, the
    mathematical statement in the tensors' dtype (float64: the yardstick; the device's own operation order is ``c51_dueling_combine_host``)."""
    if not dueling:
        return _q_mlp(t, x).reshape(x.shape[0], A, K)
    out = _q_mlp(t, x).reshape(x.shape[0], A + 1, K)
    adv, val = out[:, :A], out[:, A:]
    return val + adv - adv.mean(1, keepdim=True)


def c51_dueling_combine_host(out, A, K):
    """``c51_dueling_combine`` of csrc/stmpc_c51_kernels.hpp in numpy, operation for operation: float32 outputs ``out`` [n][(A + 1) * K] (the output
    layer's: advantage blocks, then the value block) -> float32 logits [n][A][K].  The inputs go to float64, the sum over b runs in b order, the
    division by A and the two additions are float64, (V + Adv) first, and the result is rounded to float32 once."""
    o = np.asarray(out, dtype=np.float32).astype(np.float64).reshape(-1, A + 1, K)
    s = np.zeros((o.shape[0], K), dtype=np.float64)
    for b in range(A):
        s = s + o[:, b]
    return ((o[:, A:A + 1] + o[:, :A]) - (s / np.float64(A))[:, None, :]).astype(np.float32)


def c51_fold_dueling_host(net, A, K):
    """The PLAIN C51 network {w0, b0, w1 [A * K][h1], b1 [A * K]} (float64) with the logits of the dueling network ``net`` {w0, b0, w1 [(A + 1) * K][h1],
    b1}: W'[a K + k] = W_V[k] + W_A[a][k] - mean_b W_A[b][k], the biases likewise -- the combine is linear in the output layer.  For users who want a
    plain ``.npz`` (``C51Actor`` takes it without the ``dueling`` key), and an independent check of the head."""
    w1, b1 = np.asarray(net["w1"], dtype=np.float64).reshape(A + 1, K, -1), np.asarray(net["b1"], dtype=np.float64).reshape(A + 1, K)
    fw = w1[A:] + w1[:A] - w1[:A].mean(0, keepdims=True)
    fb = b1[A:] + b1[:A] - b1[:A].mean(0, keepdims=True)
    return {"w0": np.asarray(net["w0"], dtype=np.float64), "b0": np.asarray(net["b0"], dtype=np.float64), "w1": fw.reshape(A * K, -1), "b1": fb.reshape(A * K)}


def c51_targets_host(params, batch, cfg, dtype="float64", disc=None):
    """The target side of one update in ``dtype``: {"ev_next" [B][A]: the expected values on s' of the net that picks a* (``cfg.double``: the online
    one), "astar" int64 [B]: their first maximum, "q_next" [B]: the target net's expected value at a*, "p_next" [B][K]: its distribution there,
    "m" [B][K]: ``c51_project_host`` of it under (r, mask, disc)}.  ``disc``: the discount per row (``nstep_batch_host``'s; None: ``cfg.gamma``)."""
    import torch
    td = getattr(torch, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=td)
    A, K, B = cfg.n_actions, cfg.n_atoms, len(batch["r"])
    duel = bool(getattr(cfg, "dueling", False))
    z = T(c51_support(cfg))
    with torch.no_grad():
        s2 = T(batch["s2"])
        pt = torch.softmax(_c51_logits({k: T(params["q_target"][k]) for k in DQN_TENSORS}, s2, A, K, duel), -1)
        ps = torch.softmax(_c51_logits({k: T(params["q"][k]) for k in DQN_TENSORS}, s2, A, K, duel), -1) if cfg.double else pt
        ev = (ps * z).sum(-1)
        astar = torch.argmax(ev, dim=1)
        p_next = pt[torch.arange(B), astar]
        q_next = (p_next * z).sum(-1)
    d = np.full(B, cfg.gamma) if disc is None else np.asarray(disc)
    m = c51_project_host(p_next.numpy(), np.asarray(batch["r"]), np.asarray(batch["mask"]), d, cfg, dtype)
    return {"ev_next": ev.numpy(), "astar": astar.numpy(), "q_next": q_next.numpy(), "p_next": p_next.numpy(), "m": m}


def update_host_c51(params, batch, cfg, dtype="float64", weights=None, grads_only=False, lr=None, disc=None):
    """One C51 update in torch with autograd, every tensor in ``dtype``: the projected target distribution of ``c51_targets_host``, the row loss
    l = -sum_i m_i log_softmax(logits(s)[a])_i, its mean over the minibatch -- ``weights``: prioritised replay's importance weight per row --, one
    bias-corrected Adam step and the hard copy of the target as ``update_host_dqn`` has them.  Returns the new params and a dict with
    ``update_host_dqn``'s keys -- ``loss`` (unweighted), ``mean_q``, ``q_values`` (the expected value of the stored action), ``td`` (the row loss: the
    priority), ``targets`` ([B][3]: a*, the target net's expected value there, l), ``grad`` -- plus ``dist`` ([B][2][K]: m and p(s, a)), ``row_loss``
    and ``ev_next``.  With ``cfg.dueling`` the nets have (A + 1) * K output rows and the logits are the dueling head's (``_c51_logits``)."""
    import torch
    td = getattr(torch, dtype)
    T = lambda a: torch.tensor(np.asarray(a), dtype=td)
    A, K, B = cfg.n_actions, cfg.n_atoms, len(batch["r"])
    P = {slot: {k: T(params[slot][k]) for k in DQN_TENSORS} for slot in _capi.C51_SLOTS}
    tg = c51_targets_host(params, batch, cfg, dtype, disc=disc)
    m = T(tg["m"])
    net = {k: P["q"][k].clone().requires_grad_(True) for k in DQN_TENSORS}
    a = torch.tensor(np.asarray(batch["a"], dtype=np.int64))
    logp = torch.log_softmax(_c51_logits(net, T(batch["s"]), A, K, bool(getattr(cfg, "dueling", False))), -1)[torch.arange(B), a]
    terms = -(m * logp).sum(-1)
    loss = terms.mean()
    grads = dict(zip(DQN_TENSORS, torch.autograd.grad(loss if weights is None else (T(weights) * terms).mean(), [net[k] for k in DQN_TENSORS])))
    u = int(params["updates"])
    if not grads_only:
        t = u + 1
        bc1, bc2 = 1.0 - cfg.beta1 ** t, 1.0 - cfg.beta2 ** t
        for k in DQN_TENSORS:
            mm = cfg.beta1 * P["q_m"][k] + (1 - cfg.beta1) * grads[k]
            vv = cfg.beta2 * P["q_v"][k] + (1 - cfg.beta2) * grads[k] * grads[k]
            P["q_m"][k], P["q_v"][k] = mm, vv
            P["q"][k] = P["q"][k] - ((cfg.lr if lr is None else lr) / bc1) * mm / (vv.sqrt() / math.sqrt(bc2) + cfg.eps)
            if t % cfg.target_period == 0:
                P["q_target"][k] = P["q"][k].clone()
    out = {slot: {k: P[slot][k].detach().numpy() for k in DQN_TENSORS} for slot in _capi.C51_SLOTS}
    out["beta_pow"] = np.array(params["beta_pow"], dtype=np.float32) * (1 if grads_only else np.array([cfg.beta1, cfg.beta2], dtype=np.float32))
    out["updates"] = u + (0 if grads_only else 1)
    p = logp.detach().exp()
    q = (p * T(c51_support(cfg))).sum(-1)
    row_loss = terms.detach().numpy()
    info = {"loss": float(loss.detach()), "mean_q": float(q.mean()), "q_values": q.numpy(), "td": row_loss, "row_loss": row_loss,
            "targets": np.stack([tg["astar"].astype(row_loss.dtype), tg["q_next"], row_loss], 1), "dist": np.stack([tg["m"], p.numpy()], 1),
            "ev_next": tg["ev_next"], "grad": {k: grads[k].numpy() for k in DQN_TENSORS}}
    return out, info


class C51Learner(_QLearner):
    """Categorical DQN on the device for the discrete-action envs, with ``DQNLearner``'s interface (``train_dqn`` takes either).  ``env_or_dims``: a
    discrete env or ``(n_obs, n_actions)``; ``cfg``: ``C51Config``; ``init``: None (torch's nn.Linear initialisation, ``init_c51_net``) or a net
    {w0, b0, w1 [A * n_atoms][h1], b1 [A * n_atoms]} ((A + 1) * n_atoms rows with ``cfg.dueling``: the value block last).  One update is three HIP
    launches (five with ``cfg.per``), with either head; four (six) with ``cfg.noisy``, whose parameters these tensors are the mean of."""

    _api, _per_api, _slots, _flatten = "c51", "c51_per", _capi.C51_SLOTS, staticmethod(flatten_q)
    _name, _cfg_type = "C51", C51Config

    @property
    def noisy(self):
        return getattr(self.cfg, "noisy", None) is not None

    def _create(self):
        """The new handle, with the noisy output layer enabled on it while it is fresh (a population's member never gets here: ``_Borrowed``)."""
        h = super()._create()
        if self.noisy:
            self.ctx.noisy_c51_enable(h, self.cfg.noisy.sigma0)
        return h

    def _sigma_len(self):
        return self._n_out * (self.cfg.h1 + 1)

    def _sigma_slot(self, i):
        flat = self.ctx.noisy_c51_get_params(self.handle, i, self._sigma_len())
        n = self._n_out * self.cfg.h1
        return {"w1": flat[:n].reshape(self._n_out, self.cfg.h1).copy(), "b1": flat[n:].copy()}

    def act(self, obs, ticks=None, eps=0.0, debug_q=None, noisy=None):
        """``_QLearner.act``.  ``noisy``: None -- noisy iff the learner is --; False: the mean network (bit-identical to ``actor.C51Actor.from_learner``;
        draws nothing, advances nothing); True: a fresh acting draw of the output layer's noise (a plain learner refuses).  ``eps`` is honoured either
        way."""
        if noisy is None:
            noisy = self.noisy
        if not noisy:
            return super().act(obs, ticks, eps=eps, debug_q=debug_q)
        if not self.noisy:
            raise ValueError("noisy=True needs a learner with the noisy output layer (C51Config(noisy=NoisyConfig())); this one is plain")
        n = obs.shape[0]
        out = self._out(n, self.torch.int32)
        _check_q_act(self.torch, obs, debug_q, self.cfg.n_actions)
        self.ctx.noisy_c51_act(self.handle, n, obs.data_ptr(), obs.stride(0), eps, out.data_ptr(), debug_q.data_ptr() if debug_q is not None else 0, self._stream())
        return out

    def noise(self, which="online"):
        """Debug: (f_in float32 [h1], f_out float32 [n_out]) of the last learning draw of the ``"online"`` or the ``"target"`` net, or of the last
        ``"act"`` draw; synchronises."""
        f = self.ctx.noisy_c51_debug_read(self.handle, _capi.NOISY_F[which], self.cfg.h1 + self._n_out)
        return f[:self.cfg.h1].copy(), f[self.cfg.h1:].copy()

    def effective(self, which="online", padded=False):
        """Debug: the effective output layer {w1, b1} of that draw as the kernels read it; ``padded``: in the library's layout [Ap][h1p], [Ap];
        synchronises."""
        rows, cols = ((self._n_out + 15) & ~15, (self.cfg.h1 + 15) & ~15) if padded else (self._n_out, self.cfg.h1)
        flat = self.ctx.noisy_c51_debug_read(self.handle, _capi.NOISY_F[which] + (6 if padded else 3), rows * cols + rows)
        return {"w1": flat[:rows * cols].reshape(rows, cols).copy(), "b1": flat[rows * cols:].copy()}

    def _check_cfg_type(self):
        if not isinstance(self.cfg, C51Config):
            raise ValueError("cfg must be a C51Config")

    def _check_width(self):
        self.cfg.check_width()

    def _out_shape(self):
        return (self.cfg.n_blocks, self.cfg.n_atoms)

    def _init_net(self, rng):
        return init_c51_net(self.cfg.n_obs, self.cfg.h1, self.cfg.n_actions, self.cfg.n_atoms, rng, self.cfg.dueling)

    def state_dict(self):
        """``_Learner.state_dict`` with the head's flag (``dueling``) and ``noisy``, which ``load_state_dict`` compares; a noisy learner's params
        carry the four sigma slots ({w1, b1} each) and its counters the acting draws (``counters[5]``)."""
        sd = super().state_dict()
        sd["dueling"] = bool(self.cfg.dueling)
        sd["noisy"] = self.noisy
        if self.noisy:
            for i, slot in enumerate(_capi.NOISY_SLOTS):
                sd["params"][slot] = self._sigma_slot(i)
        return sd

    def load_state_dict(self, sd):
        """``_Learner.load_state_dict``; a state written by the other head is refused (one without the ``dueling`` key is taken as it is, as one
        without ``n_step`` is)."""
        if "dueling" in sd and bool(sd["dueling"]) != bool(self.cfg.dueling):
            raise ValueError("the state is a %s C51 learner's, this learner has a %s head (cfg.dueling = %r)"
                             % ("dueling" if sd.get("dueling", False) else "plain", "dueling" if self.cfg.dueling else "plain", self.cfg.dueling))
        if "noisy" in sd and bool(sd["noisy"]) != self.noisy:
            raise ValueError("the state is a %s C51 learner's, this learner has a %s output layer (cfg.noisy = %r)"
                             % ("noisy" if sd["noisy"] else "plain", "noisy" if self.noisy else "plain", getattr(self.cfg, "noisy", None)))
        super().load_state_dict({k: v for k, v in sd.items() if k not in ("dueling", "noisy")})
        if self.noisy:
            for i, slot in enumerate(_capi.NOISY_SLOTS):
                if slot in sd["params"]:
                    t = sd["params"][slot]
                    self.ctx.noisy_c51_set_params(self.handle, i, np.concatenate([np.asarray(t["w1"], dtype=np.float32).ravel(), np.asarray(t["b1"], dtype=np.float32).ravel()]))

    def dist(self):
        """Debug: (float32 [batch][2][n_atoms] = the projected target distribution m and the online distribution p(s, a); ``targets()``'s array) of
        the minibatch the next update will draw, from one pass; synchronises."""
        d = self.torch.zeros(self.cfg.batch, 2, self.cfg.n_atoms, dtype=self.torch.float32, device=self.device)
        out = self.torch.zeros(self.cfg.batch, 4, dtype=self.torch.float32, device=self.device)
        self.ctx.c51_dist(self.handle, d.data_ptr(), out.data_ptr(), self._stream())
        return d.cpu().numpy(), out.cpu().numpy()

    def project(self, p, reward, mask, disc):
        """Debug: the device's projection of caller-given distributions ``p`` [n][n_atoms] under ``reward``, ``mask``, ``disc`` [n] (numpy in, float32
        numpy out): the device function the update calls; synchronises."""
        torch = self.torch
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=self.device)
        p, reward, mask, disc = t(p), t(reward), t(mask), t(disc)
        assert p.shape == (reward.numel(), self.cfg.n_atoms) and mask.numel() == disc.numel() == reward.numel()
        m = torch.zeros_like(p)
        self.ctx.c51_project(self.handle, p.shape[0], p.data_ptr(), reward.data_ptr(), mask.data_ptr(), disc.data_ptr(), m.data_ptr(), self._stream())
        return m.cpu().numpy()

    def export_q(self, path):
        """Write the online logits network as an ``.npz``: w0, b0, w1, b1 (float32), ``action_values`` and the head's ``n_atoms``, ``v_min``, ``v_max``
        and ``dueling`` (0 / 1; a reader takes a file without the key as 0).  Of a noisy learner it is the MEAN network; ``noisy`` (0 / 1) says so
        and readers ignore it."""
        with open(path, "wb") as fh:
            np.savez_compressed(fh, **self._slot(0), action_values=self.action_values, n_atoms=np.int64(self.cfg.n_atoms), v_min=np.float64(self.cfg.v_min),
                                v_max=np.float64(self.cfg.v_max), dueling=np.int64(self.cfg.dueling), noisy=np.int64(getattr(self.cfg, "noisy", None) is not None))
        return path


class _C51PopulationMember(_Borrowed, C51Learner):
    """One member of a ``C51Population`` as a ``C51Learner`` (``stmpc_pop_c51_member``)."""


class C51Population(DQNPopulation):
    """P independent C51 learners on one discrete-action ``MergeVecEnv``, advanced together: three launches per update whatever P is (five when at
    least one member is prioritised), one each for acting, pushing and the statistics (``csrc/stmpc_c51_pop_kernels.hpp``, ``stmpc_pop_c51_*``).
    The questions a user has about the categorical agent -- which support ``[v_min, v_max]`` fits this env's returns, double against plain action
    selection, which ``target_period``, ``gamma``, ``n_step`` and seed, prioritised against uniform replay -- are a population's members side by side.

    ``cfgs``: a list of ``C51Config`` or ``(cfg, P)``; the members share n_obs, h1, n_actions, n_atoms, ``dueling``, batch and capacity and may differ
    in everything else, the support included.  ``env``, ``seeds``, ``init``, ``per``, traffic groups and reward groups: as ``DQNPopulation``'s.  Member
    m starts exactly as ``C51Learner(seed=seeds[m], init=...)`` does and stays bit-identical to that learner driven on its slice alone.

    ``act`` / ``push`` / ``update`` / ``stats_device`` / ``stats`` are ``DQNPopulation``'s; ``act(..., debug_q=)`` gives the expected values
    float32 [env.n][n_actions].  ``member(m)`` is a ``C51Learner`` view: ``state_dict`` / ``load_state_dict``, ``grads``, ``targets``, ``dist``,
    ``project``, ``minibatch``, ``priorities``, ``last_sample``, ``nstep_window``, ``export_q``, ``actor.C51Actor.from_learner(pop.member(m), ...)`` and
    ``evaluate_dqn(pop.member(m), ...)`` work on it.  ``train_dqn`` takes a population.  A population of C51 POLICIES does not exist:
    ``evaluate_dqn_members``, ``actor.QActorPopulation`` and ``actor.population_of`` refuse a ``C51Population`` as they refuse C51 members: its
    policies are evaluated together by ``evaluate_c51_members`` and ``actor.C51ActorPopulation``."""

    _api = "c51_pop"
    _nstep_kind = "c51"                                             # (``ctx.pop_nstep_enable`` routes it to stmpc_pop_c51_multi_step_enable)
    _cfg_type, _action_dtype = C51Config, "int32"

    def __init__(self, env, cfgs, seeds=None, init=None, ctx=None, per=None, noisy=None):
        """``noisy``: the noisy output layer (``NoisyConfig``) -- None, one for every member, or a list of P (``sigma0`` may differ per member; the
        members are all noisy or all plain).  Like ``per`` it is the population's argument: a cfg that carries ``noisy=`` is refused.  Member m is then
        bit-identical to ``C51Learner(cfg with noisy=noisy[m], seed=seeds[m])`` on its slice; ``act`` draws per member (``act(noisy=False)``: the mean
        networks), ``train_dqn`` with ``eps_schedule=None`` uses epsilon 0, one update is four launches (six with prioritised members)."""
        import copy
        if isinstance(cfgs, tuple) and len(cfgs) == 2 and isinstance(cfgs[0], self._cfg_type):
            cfgs = [cfgs[0]] * int(cfgs[1])
        cfgs = list(cfgs)
        for m, c in enumerate(cfgs):
            if getattr(c, "noisy", None) is not None:
                raise ValueError("member %d's cfg asks for the noisy output layer (noisy=): a population enables it for its members itself; give the "
                                 "NoisyConfig to the population's noisy= argument (one for all members, or a list with one entry per member)" % m)
        if noisy is None or isinstance(noisy, NoisyConfig):
            noisy = [noisy] * len(cfgs)
        elif not isinstance(noisy, (list, tuple)):
            raise ValueError("noisy must be None, a NoisyConfig, or a list with one NoisyConfig per member")
        noisy = list(noisy)
        if len(noisy) != len(cfgs):
            raise ValueError("noisy has %d entries, the population %d members" % (len(noisy), len(cfgs)))
        for m, g in enumerate(noisy):
            if g is not None and not isinstance(g, NoisyConfig):
                raise ValueError("noisy[%d] is a %s, not a NoisyConfig" % (m, type(g).__name__))
            if (g is None) != (noisy[0] is None):
                raise ValueError("member %d is %s, member 0 is %s: the members of a population are all noisy or all plain (one launch sequence)"
                                 % (m, "plain" if g is None else "noisy", "plain" if noisy[0] is None else "noisy"))
        self.noisy_cfgs = noisy
        if self.noisy:                                              # (the members' views read their cfg: each gets a copy that carries its own)
            cfgs = [copy.copy(c) for c in cfgs]
            for c, g in zip(cfgs, noisy):
                if isinstance(c, C51Config):
                    c.noisy = g
        super().__init__(env, cfgs, seeds=seeds, init=init, ctx=ctx, per=per)

    @property
    def noisy(self):
        return bool(self.noisy_cfgs) and self.noisy_cfgs[0] is not None

    def _create_handle(self):
        """The new population, with the noisy output layer enabled on its members while they are fresh."""
        h = super()._create_handle()
        if self.noisy:
            try:
                self.ctx.c51_pop_noisy_enable(h, [g.sigma0 for g in self.noisy_cfgs])
            except Exception:
                self._call("destroy")(h)
                raise
        return h

    def act(self, obs, ticks=None, eps=0.0, debug_q=None, noisy=None):
        """``DQNPopulation.act``.  ``noisy``: None -- noisy iff the population is --; False: the mean networks (nothing drawn, nothing advanced); True:
        every member takes a fresh acting draw (a plain population refuses).  ``eps`` is honoured either way."""
        if noisy is None:
            noisy = self.noisy
        if not noisy:
            return super().act(obs, ticks, eps=eps, debug_q=debug_q)
        if not self.noisy:
            raise ValueError("noisy=True needs a population with the noisy output layer (C51Population(..., noisy=NoisyConfig())); this one is plain")
        self._rows(obs)
        _check_q_act(self.torch, obs, debug_q, self.cfgs[0].n_actions)
        self.ctx.c51_pop_noisy_act(self.handle, self.n_per_member, obs.data_ptr(), obs.stride(0), per_member(eps, self.P), self._actions.data_ptr(),
                                   debug_q.data_ptr() if debug_q is not None else 0, self._stream())
        return self._actions

    def _check_env(self, env):
        if env.continuous:
            raise ValueError("C51 needs a discrete action space (sumo-jerk-v0 or sumo-accel-v0), not the continuous jerk env")

    def _check_cfgs(self, env):
        for m, c in enumerate(self.cfgs):
            if not isinstance(c, C51Config):
                raise ValueError("member %d's cfg is a %s, not a C51Config" % (m, type(c).__name__))
        super()._check_cfgs(env)
        for m, c in enumerate(self.cfgs):
            c.check_width()
            if c.n_atoms != self.cfgs[0].n_atoms:
                raise ValueError("member %d has n_atoms %d, member 0 has %d: the members share n_obs, h1, n_actions, n_atoms, batch and capacity"
                                 % (m, c.n_atoms, self.cfgs[0].n_atoms))
            if bool(c.dueling) != bool(self.cfgs[0].dueling):
                raise ValueError("member %d has dueling = %r, member 0 has %r: the members share the head (it sets the network's shape)"
                                 % (m, c.dueling, self.cfgs[0].dueling))

    def _make_member(self, m, env, init):
        return _C51PopulationMember(self, m, env, self.cfgs[m], self.seeds[m], init)


class _TakeoverShare:
    """What ``train_ddpg`` and ``train_dqn`` (their loop, ``_train``) count on a shielded env: the ticks on which the shield overruled the action and
    the live ticks, summed on the device at every step (no host synchronisation) and read at the drains.  Without autoreset a finished environment
    idles: not a live tick.  ``P`` > 0: per member too, the owner of row e being e // ``n_per_member``."""

    def __init__(self, env, P=0, n_per_member=0):
        torch = env.torch
        self.env, self.P = env, int(P)
        self.taken, self.lived = torch.zeros((), dtype=torch.int64, device=env.device), torch.zeros((), dtype=torch.int64, device=env.device)
        self.alive = torch.ones(env.n, dtype=torch.bool, device=env.device)
        self.takeover_ticks = self.live_ticks = 0
        if self.P:
            self.owner = torch.arange(env.n, device=env.device) // int(n_per_member)
            self.member_taken, self.member_lived = (torch.zeros(self.P, dtype=torch.int64, device=env.device) for _ in range(2))
            self.member_ticks = ([0] * self.P, [0] * self.P)

    def step(self, info, term, trunc):
        self.taken += info["takeover"].sum()
        self.lived += self.alive.sum()
        if self.P:
            self.member_taken.index_add_(0, self.owner, info["takeover"].to(self.env.torch.int64))
            self.member_lived.index_add_(0, self.owner, self.alive.to(self.env.torch.int64))
        if not self.env.autoreset:
            self.alive &= ~(term | trunc)

    def read(self):
        """At a drain: the loop has just synchronised."""
        self.takeover_ticks, self.live_ticks = int(self.taken.item()), int(self.lived.item())
        if self.P:
            self.member_ticks = (self.member_taken.tolist(), self.member_lived.tolist())

    @property
    def share(self):
        return self.takeover_ticks / self.live_ticks if self.live_ticks else 0.0

    @property
    def member_share(self):
        return [t / l if l else 0.0 for t, l in zip(*self.member_ticks)]


def _train(env, learner, frames, updates_per_step, drain_every, act, pushed_action, update):
    """The loop of ``train_ddpg`` and ``train_dqn``: act -> env.step -> push -> update, ``-(-frames // env.n)`` times, with a drain of the finished
    episodes' statistics (the only synchronisation) every ``drain_every`` steps and after the last, a shielded env's takeovers counted by
    ``_TakeoverShare``, and the result dict -- with ``member_returns`` (and behind a shield ``member_takeover_share``) when ``learner`` is a
    population.  The callers supply what differs: ``act(i, steps, obs) -> (ticks, action)``, ``pushed_action(action, info)`` and ``update(i, steps)``,
    this step's ``updates_per_step`` updates under the schedule's value."""
    pop = isinstance(learner, DDPGPopulation)
    steps = -(-int(frames) // env.n)
    obs = env.reset()
    returns, envs = [], []
    shield = _TakeoverShare(env, learner.P if pop else 0, learner.n_per_member if pop else 0) if getattr(env, "shield", None) is not None else None
    for i in range(steps):
        ticks, action = act(i, steps, obs)
        next_obs, reward, term, trunc, info = env.step(action)
        learner.push(obs, ticks, pushed_action(action, info), reward, next_obs, term, trunc, final_obs=info["final_observation"])
        if shield is not None:
            shield.step(info, term, trunc)
        if updates_per_step:
            update(i, steps)
        obs = next_obs
        if (i + 1) % drain_every == 0 or i + 1 == steps:
            drained = env.drain_episode_stats()
            returns.append(drained["episode_return"])
            envs.append(drained["env"])
            if shield is not None:
                shield.read()
    returns = np.concatenate(returns) if returns else np.zeros(0)
    out = {"steps": steps, "frames": steps * env.n, "episodes": int(returns.size), "mean_return": float(returns.mean()) if returns.size else float("nan"),
           "returns": returns, "takeover_share": shield.share if shield is not None else 0.0}
    if pop:
        owner = (np.concatenate(envs) if envs else np.zeros(0, dtype=np.int64)) // learner.n_per_member
        out["member_returns"] = [returns[owner == m] for m in range(learner.P)]
        if shield is not None:
            out["member_takeover_share"] = shield.member_share
    return out


def train_dqn(env, learner, frames, updates_per_step=1, drain_every=64, eps_schedule=None, lr_schedule=None):
    """The loop of the reference's ``DQNAgent._train`` on the device: act (epsilon-greedy) -> env.step -> push -> ``updates_per_step`` updates,
    until ``frames`` transitions were collected (rounded up to whole steps of env.n).  ``eps_schedule(step, steps) -> eps`` (None:
    ``dqn_epsilon(step)``, the reference's decay with the step for the episode number); ``lr_schedule(step, steps) -> lr``.  Synchronises only
    every ``drain_every`` steps.  The result has ``train_ddpg``'s keys.
    ``learner`` may be a ``DQNPopulation`` (both schedules may then return per-member arrays); the result then also carries ``member_returns``:
    the drained returns of each member's environments, a list of P arrays (owner = env index // n_per_member), as ``train_ddpg``'s does.
    A learner with the noisy output layer (``C51Config(noisy=...)``) explores through its noise: with ``eps_schedule=None`` its epsilon is 0 (an
    explicit schedule is honoured).
    On a shielded env (a discrete ``MergeVecEnv(shield="first_step")``, ``vec_env.GroupedShieldVecEnv`` or ``vec_env.QCombinedShieldVecEnv``) the
    result's ``takeover_share`` is the share of the live ticks on which the shield overruled the action (summed on the device, read at the drains,
    by ``_train``'s ``_TakeoverShare`` as for ``train_ddpg``; 0.0 on an env without a ``shield``), and with a ``DQNPopulation`` ``member_takeover_share`` is that share per member,
    a list of P floats (owner = env index // n_per_member)."""
    default_eps = (lambda i: 0.0) if getattr(learner, "noisy", False) else dqn_epsilon

    def act(i, steps, obs):
        return None, learner.act(obs, None, eps=eps_schedule(i, steps) if eps_schedule is not None else default_eps(i))

    def update(i, steps):
        learner.update(updates_per_step, lr_schedule(i, steps) if lr_schedule is not None else None)
    return _train(env, learner, frames, updates_per_step, drain_every, act, lambda action, info: action, update)


def write_actor(path, net, tanh_scale, tanh_mean):
    """The file format of ``actor.load_weights`` for a net {w0, b0, w1, b1, w2, b2}."""
    with open(path, "wb") as fh:
        np.savez_compressed(fh, **{k: np.asarray(net[k], dtype=np.float32) for k in TENSORS}, tanh_scale=np.float64(tanh_scale), tanh_mean=np.float64(tanh_mean))


def train_ddpg(env, learner, frames, updates_per_step=1, drain_every=64, lr_schedule=None, executed_actions=False):
    """The loop of the reference's ``DDPGAgent.train`` on the device: act with noise -> env.step -> push -> ``updates_per_step`` updates, until
    ``frames`` transitions were collected (rounded up to whole steps of env.n).  Synchronises only every ``drain_every`` steps, to drain the
    finished episodes' statistics.  ``lr_schedule(step, steps) -> (lr_q, lr_pi)``: e.g. the preset's cosine schedule, computed on the host.
    Returns {"steps", "frames", "episodes", "mean_return" (of the drained episodes), "returns" (array)}.
    ``learner`` may be a ``DDPGPopulation`` (the schedule may then return per-member arrays); the result then also carries
    ``member_returns``: the drained returns of each member's environments, a list of P arrays.
    On a shielded env (``MergeVecEnv(shield="first_step")``, ``vec_env.CombinedShieldVecEnv``) the result's ``takeover_share`` is the share of the live ticks on which the shield
    overruled the action (summed on the device, read at the drains, by ``_train``'s ``_TakeoverShare``; 0.0 on an unshielded env) -- with a population ``member_takeover_share`` is that
    share per member, as ``train_dqn``'s --, and ``executed_actions=True`` (continuous env only,
    else ValueError) pushes ``info["executed_action"]`` -- what the shield let through or put in the action's place -- instead of the action."""
    shielded = getattr(env, "shield", None) is not None
    if executed_actions and not (shielded and env.continuous):
        raise ValueError("executed_actions=True needs a shielded continuous env (MergeVecEnv(env_id='sumo-jerk-continuous-v0', shield='first_step') or a "
                         "CombinedShieldVecEnv)")

    def act(i, steps, obs):
        ticks = env.episode_ticks.clone()
        return ticks, learner.act(obs, ticks, noise=True)

    def update(i, steps):
        lr_q, lr_pi = lr_schedule(i, steps) if lr_schedule is not None else (None, None)
        learner.update(updates_per_step, lr_q, lr_pi)
    pushed_action = (lambda action, info: info["executed_action"]) if executed_actions else (lambda action, info: action)
    return _train(env, learner, frames, updates_per_step, drain_every, act, pushed_action, update)


def _check_members_controller(controller):
    if controller not in ("combined", "first_step"):
        raise ValueError("members are evaluated under 'combined' or 'first_step', not %r" % (controller,))


def _evaluate_population(members, P, population_cls, n_per_member, seed, kmax, max_episode_length, record, ctx, traffic, controller):
    """What ``evaluate_members``, ``evaluate_dqn_members`` and ``evaluate_c51_members`` do once they have refused what is not theirs: one run of
    ``P * n_per_member`` episodes whose policy is ``population_cls(members, ...)``, on a new context unless one is given, summarised per member."""
    from . import episodes
    if traffic is not None and len(traffic) != P:
        raise ValueError("%d traffic groups for %d members: member m is evaluated on traffic m" % (len(traffic), P))
    ctx = ctx if ctx is not None else _capi.Context(-1)
    pop = population_cls(members, n_per_member, ctx, Settings)
    stats = episodes.run_episodes(pop.n, seed=seed, controller=controller, policy=pop, ctx=ctx, kmax=kmax, max_episode_length=max_episode_length, record=record,
                                  traffic=traffic)
    rep = stats.get("report")
    return {"stats": stats, "by_member": episodes.summary_by_member(stats, pop.P),
            "reports": rep.by_member(pop.P, traffic) if rep is not None else None}


def evaluate_members(source, n_per_member, seed=0, kmax=16, max_episode_length=100.0, record=None, ctx=None, traffic=None, controller="combined"):
    """The reference's per-model ``EVALUATE_COMBINED_DDPG`` -- and the evaluation ``train_ddpg_all_with_lr_drop`` (ddpg.py:96-117) ends with -- for
    every member at once: ``n_per_member`` merge episodes per member under the combined controller, in ONE run of P * n_per_member environments
    whose policy is an ``actor.ActorPopulation``.  ``source``: a ``DDPGPopulation`` or a ``DDPGLearner`` (zero-copy views of the weights as they
    are on the device: nothing is exported or uploaded), or a list as ``ActorPopulation`` takes (names, paths, learners, actors).
    ``ctx``: the evaluation's context; by default a new one, because a context holds one world and the training env has its own.
    Returns ``{"stats": run_episodes' columns + "member", "by_member": P summary rows, "reports": P ``report.Report``s (None without ``record``)}``.
    The members' episodes are different draws of one world (identically distributed, not common random numbers).
    ``traffic``: None, or one traffic group per member (as ``episodes.sim_cfgs`` takes them): member m is evaluated on traffic m, and its report
    row carries that traffic's TRAFFIC_DESCRIPTION.  ``controller``: "combined", or "first_step" for the one-step shield of ``first_step.py``."""
    _check_members_controller(controller)
    if isinstance(source, DQNPopulation):
        raise ValueError("a DQNPopulation's members are Q-networks: evaluate them all in one launch with evaluate_dqn_members(pop, n_per_member, ...), or "
                         "one at a time with evaluate_dqn(pop.member(m), ...); evaluate_members builds a population of DDPG actors")
    members = source if isinstance(source, (DDPGPopulation, list, tuple)) else [source]
    return _evaluate_population(members, len(members), _actor.ActorPopulation, n_per_member, seed, kmax, max_episode_length, record, ctx, traffic, controller)


def evaluate_dqn_members(source, n_per_member, seed=0, kmax=16, max_episode_length=100.0, record=None, ctx=None, traffic=None, controller="combined"):
    """``evaluate_members`` for Q-networks: ``n_per_member`` merge episodes per member under the combined controller, in ONE run of P *
    n_per_member environments whose policy is an ``actor.QActorPopulation`` -- one launch per evaluation whatever P is, where
    ``evaluate_dqn(pop.member(m), ...)`` takes P runners, P worlds and P launch sequences per tick.  ``source``: a ``DQNPopulation`` or a
    ``DQNLearner`` (zero-copy views of the online networks as they are on the device), or a list as ``QActorPopulation`` takes (``export_q`` files,
    learners, ``DQNActor``s).  ``ctx``, ``traffic``, ``controller`` and the returned dict -- ``stats`` with ``member``, ``by_member``, ``reports``
    -- are ``evaluate_members``'."""
    _check_members_controller(controller)
    members = source if isinstance(source, (DQNPopulation, list, tuple)) else [source]
    if isinstance(members, C51Population):
        _actor.refuse_c51_members([members.member(m) for m in range(members.P)], "evaluate_dqn_members")
    if not isinstance(members, DQNPopulation):
        _actor.refuse_c51_members(members, "evaluate_dqn_members")      # (before a context exists: a C51 policy is evaluated alone, by evaluate_dqn)
    P = members.P if isinstance(members, DQNPopulation) else len(members)
    return _evaluate_population(members, P, _actor.QActorPopulation, n_per_member, seed, kmax, max_episode_length, record, ctx, traffic, controller)


def evaluate_c51_members(source, n_per_member, seed=0, kmax=16, max_episode_length=100.0, record=None, ctx=None, traffic=None, controller="combined"):
    """``evaluate_dqn_members`` for categorical (C51) policies: ``n_per_member`` merge episodes per member under the combined controller, in ONE
    run of P * n_per_member environments whose policy is an ``actor.C51ActorPopulation`` -- one launch per evaluation whatever P is, where
    ``evaluate_dqn(pop.member(m), ...)`` takes P runners, P worlds and P launch sequences per tick.  ``source``: a ``C51Population`` or a
    ``C51Learner`` (zero-copy views of the online networks as they are on the device; a noisy learner's view evaluates its mean weights), or a list
    as ``C51ActorPopulation`` takes (``C51Learner.export_q`` files, learners, ``C51Actor``s).  The keywords, the refusals and the returned dict --
    ``stats`` with ``member``, ``by_member``, ``reports`` -- are ``evaluate_dqn_members``'; a DQN member is refused (``evaluate_dqn_members`` is
    theirs) before a context exists."""
    _check_members_controller(controller)
    if isinstance(source, DQNPopulation) and not isinstance(source, C51Population):
        raise ValueError("a DQNPopulation's members are Q-networks, not categorical (C51) policies: evaluate them with evaluate_dqn_members(pop, n_per_member, ...)")
    members = source if isinstance(source, (C51Population, list, tuple)) else [source]
    P = members.P if isinstance(members, C51Population) else len(members)
    if not isinstance(members, C51Population):
        q = [m for m, item in enumerate(members) if _actor._is_q_member(item) and not isinstance(item, _actor.C51Actor)]      # (a C51Actor is a DQNActor's subclass)
        if q:
            raise ValueError("evaluate_c51_members: members %s are Q-networks, not categorical (C51) policies (one launch needs one head); evaluate them with "
                             "evaluate_dqn_members" % ", ".join(map(str, q)))
    return _evaluate_population(members, P, _actor.C51ActorPopulation, n_per_member, seed, kmax, max_episode_length, record, ctx, traffic, controller)


def evaluate_dqn(source, n, seed=0, kmax=16, max_episode_length=100.0, record=None, ctx=None, traffic=None, controller="combined"):
    """The reference's evaluation of its DQN agent -- ``DQNAgent.get_control`` (dqn.py:375-380) behind ``RLAgent.do_combined_control`` -- for ``n``
    merge episodes in one run, with an ``actor.DQNActor`` as the policy.  ``source``: a ``DQNLearner`` (a zero-copy view of its online network as it
    is on the device), a file written by ``DQNLearner.export_q``, or a ``DQNActor`` built for ``n`` states on ``ctx``.  A categorical policy is
    evaluated the same way, with an ``actor.C51Actor``: ``source`` is then a ``C51Learner`` (a view of its online network), a file written by
    ``C51Learner.export_q`` (recognised by its ``n_atoms``), or a ``C51Actor``.
    ``ctx``: the evaluation's context; by default a new one (a ``DQNActor``'s own), because a context holds one world and the training env has its
    own.  ``controller``: "combined", or "first_step" for the one-step shield of ``first_step.py``.  ``traffic``: None, or the traffic groups of
    ``episodes.EpisodeRunner``.  Returns ``run_episodes``' columns (with ``report`` when ``record`` is given)."""
    from . import episodes
    if controller not in ("combined", "first_step"):
        raise ValueError("a DQN policy is evaluated under 'combined' or 'first_step', not %r" % (controller,))
    if isinstance(source, _actor.DQNActor):
        policy = source
        if policy.n != int(n):
            raise ValueError("n = %d, the DQNActor was built for %d states" % (n, policy.n))
        ctx = ctx if ctx is not None else policy.ctx
    else:
        ctx = ctx if ctx is not None else _capi.Context(-1)
        if isinstance(source, C51Learner):
            policy = _actor.C51Actor.from_learner(source, n, ctx, Settings)
        elif isinstance(source, DQNLearner):
            policy = _actor.DQNActor.from_learner(source, n, ctx, Settings)
        else:
            policy = (_actor.C51Actor if _actor._is_c51_file(source) else _actor.DQNActor)(source, n, ctx, Settings)
    return episodes.run_episodes(int(n), seed=seed, controller=controller, policy=policy, ctx=ctx, kmax=kmax, max_episode_length=max_episode_length, record=record,
                                 traffic=traffic)
