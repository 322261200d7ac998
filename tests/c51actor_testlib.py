"""What tests/test_c51actor_cpu.py and tests/test_c51actor.py share: the four network shapes, the nets, the stand-ins of the refusal tests, and the
one-step composition of the combined-shield env from the public entries (the construction of tests/test_qshield_env.py's ``_compose`` for a step
from the reset's world, where every row is in its episode 0).  Plain functions, nothing heavy at import time; the package is imported inside them."""
import types

import numpy as np

from stmpc_testlib import capi

# (n_in, h1, A, K): K below, just above and well above one 32-lane pass; A K = 85, 99, 1020, 255 leave pad columns in the last 16-column tile
SHAPES = [(20, 16, 5, 17), (20, 32, 3, 33), (20, 48, 20, 51), (20, 256, 5, 51)]
ROWS = [1, 16, 17, 33]
NAMES = ("w0", "b0", "w1", "b1")
JERKS = np.array([-5.0, -2.5, 0.0, 2.5, 5.0])     # JERK_VALUES_DQN
SUPPORT = (-10.0, 10.0)
NEGATIVE_SUPPORT = (-10.0, -1.0)                    # wholly below zero: a pad column's logits of 0 would mean an expected value above every real one
# test_c51actor_cpu.py asserts that under this seed the float64 twin alone keeps at least 99 % of the rows at every shape (top-two gap > 1e-9)
TWIN_SEED = 3
TWIN_ROWS = 400


def table(A):
    return JERKS.copy() if A == 5 else np.linspace(-4.75, 4.75, A)


def net(shape, seed, spread=3.0):
    """nn.Linear-scale tensors n_in -> h1 -> A K with the last layer scaled by ``spread``: distributions away from uniform."""
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_in, h1, A, K = shape
    n = learner.init_c51_net(n_in, h1, A, K, np.random.default_rng(seed))
    n["w1"] = (n["w1"] * spread).astype(np.float32)
    return n


def zero_head(n):
    """The net with a zero last layer: every action's distribution is uniform, every expected value the support's centre -- an exact tie."""
    out = {k: v.copy() for k, v in n.items()}
    out["w1"][:], out["b1"][:] = 0, 0
    return out


def config(shape, support=SUPPORT, **kw):
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_in, h1, A, K = shape
    kw = {**dict(batch=16, capacity=64, lr=1e-2), **kw}
    return learner.C51Config(n_obs=n_in, n_actions=A, h1=h1, n_atoms=K, v_min=support[0], v_max=support[1], **kw)


def export_file(path, n, shape, support=SUPPORT, action_values=None):
    """A file as ``C51Learner.export_q`` writes it."""
    with open(path, "wb") as fh:
        np.savez(fh, **{k: n[k] for k in NAMES}, action_values=table(shape[2]) if action_values is None else action_values, n_atoms=np.int64(shape[3]),
                 v_min=np.float64(support[0]), v_max=np.float64(support[1]))
    return str(path)


class NoLibrary:
    """A context stand-in whose every attribute access fails the test: the refusals are made before any library call."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def c51_learner_stub(shape):
    """What ``actor._is_dqn_learner`` took for a DQN learner on the parent commit: ``export_q``, ``handle`` and a cfg with the DQN fields -- of a C51."""
    return types.SimpleNamespace(cfg=config(shape), action_values=table(shape[2]), handle=NoLibrary(), export_q=lambda path: path, env_id=None, ctx=NoLibrary())


def c51_actor_stub(shape):
    capi()
    from rl_mpc_lanemerging_amd import actor
    a = actor.C51Actor.__new__(actor.C51Actor)
    a.handle, a.shape, a.ctx = None, shape[:3], NoLibrary()
    return a


# ---- one step of QCombinedShieldVecEnv from the public entries ---------------------------------------------------------------------------------
def compose_first_step(env_id, policy_of, act, n, seed, kmax, settings):
    """The env's first step after reset made from the public entries on a context of its own: stmpc_sim_init_device, stmpc_sim_view_device, the host
    twin of the first action, stmpc_rollout_step_device (step 1) + the policy's call and stmpc_rollout_step_device (steps 2 ... L),
    stmpc_combined_decide_device, the action handling's command, stmpc_sim_step_device, stmpc_policy_features_device and stmpc_env_reward_device on
    the wide view.  ``policy_of(ctx)`` builds the rollout policy of ``n`` rows.  Returns obs0 and, per row, takeover, reason, executed_jerk, obs,
    reward, term, trunc, and the rolled-out ego rows."""
    import torch
    from rl_mpc_lanemerging_amd import _capi, combined, episodes, rewards, vec_env
    S = settings()
    ctx = _capi.Context(-1)
    policy = policy_of(ctx)
    params = _capi.Params.from_settings(S)
    ccfg = combined.control_cfgs([{}], sparse_control=False)[0]
    L = max(int(ccfg.rollout_length), 1)
    cfg = episodes.sim_cfg(seed, float(S.MAX_EPISODE_LENGTH))
    ecfg = vec_env.env_cfg(env_id, "Continuous", autoreset=False)
    fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=False)
    dev = lambda a, dtype=None: torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")
    WIDE = 32
    feat, rew = z(n, 20, dtype=torch.float32), z(n)
    tick = float(S.TICK_LENGTH)
    a_min, a_max = float(S.MAX_NEGATIVE_ACCELERATION), float(S.MAX_POSITIVE_ACCELERATION)

    def view(K):
        b = (z(n, 5), z(n, dtype=torch.int32), z(n, K), z(n, K), z(n, K))
        ctx.sim_view(cfg, n, K, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), b[4].data_ptr())
        return b

    def features(b):
        e4 = b[0][:, :4].contiguous()
        assert int(b[1].max()) < WIDE
        ctx.policy_features_device(fcfg, n, WIDE, 1, e4.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), b[4].data_ptr(), 0, feat.data_ptr(), 20)
        return e4, feat.cpu().numpy().copy()

    ctx.sim_init(cfg, n)
    out = {"obs0": features(view(WIDE))[1]}
    b = view(kmax)
    e5 = b[0].cpu().numpy()
    fa, bad = vec_env.q_first_action_host(env_id, act, e5[:, 3], S)
    assert not bad.any()
    first = dev(fa, torch.float64)
    cur4, cox, cov, coa = b[0][:, :4].clone().contiguous(), b[2].clone(), b[3].clone(), b[4].clone()
    for step in range(1, L + 1):
        a = first if step == 1 else policy(step, cur4, b[1], cox, cov, coa)
        ctx.rollout_step_device(params, ccfg, n, kmax, step, b[0].data_ptr(), cur4.data_ptr(), b[1].data_ptr(), cox.data_ptr(), cov.data_ptr(), coa.data_ptr(), a.data_ptr())
    take_d, reason_d, speed_d = z(n, dtype=torch.int32), z(n, dtype=torch.int32), z(n)
    ctx.combined_decide_device(params, ccfg, n, kmax, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), cur4.data_ptr(), cox.data_ptr(), cov.data_ptr(),
                               first.data_ptr(), 0, take_d.data_ptr(), reason_d.data_ptr(), speed_d.data_ptr())
    take, speed = take_d.cpu().numpy() != 0, speed_d.cpu().numpy().copy()
    handled = [rewards.handle_action(env_id, float(e5[i, 2]), float(e5[i, 3]), 0.0, int(act[i])) for i in range(n)]
    cmd, pj, inv = (np.array([h[i] for h in handled]) for i in range(3))
    out.update(takeover=take, reason=reason_d.cpu().numpy().copy(), rolled=cur4.cpu().numpy().copy(),
               executed_jerk=np.where(take, (np.clip((speed - e5[:, 2]) / tick, a_min, a_max) - 0.0) / tick, pj))
    d_speed = dev(np.where(take, speed, cmd))
    ctx.sim_step(params, cfg, n, d_speed.data_ptr())
    status, _, _, ego4 = ctx.sim_read(n)
    wide = view(WIDE)
    e4, f = features(wide)
    crashed, arrived = status == 2, status == 1
    jerk = np.where(crashed | arrived, out["executed_jerk"], (ego4[:, 3] - 0.0) / tick)
    d_jerk, d_cr, d_ar = dev(jerk), dev(crashed.astype(np.int32)), dev(arrived.astype(np.int32))
    ctx.env_reward(ecfg, n, WIDE, e4.data_ptr(), wide[1].data_ptr(), wide[2].data_ptr(), d_jerk.data_ptr(), d_cr.data_ptr(), d_ar.data_ptr(), rew.data_ptr())
    out.update(obs=f, reward=rew.cpu().numpy().copy() + inv, term=crashed | arrived, trunc=status == 3, status=status)
    ctx.check_error()
    ctx.close()
    return out
