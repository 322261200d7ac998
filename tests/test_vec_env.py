"""The vector environment (rl-mpc-lanemerging_amd/vec_env.py, rewards.py, csrc/stmpc_env_kernels.hpp): the reference's gym environments
(merge_gym.py) with the rewards of dqn.get_reward_function on the batched world.

CPU: the host twins equal the reference's own functions (tests/golden/golden_env.npz, make_golden_env.py) bit for bit; the C-ABI mirror and the
settings.  GPU: the kernels against the goldens and the twins, one env step against the world's own entries driven by the twins, the
per-environment reset, terminal semantics and an end-to-end run with a pretrained actor (no statistical claim against the reference: the
world is not SUMO)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO, load_golden
from stmpc_testlib import capi as _capi, header_struct_fields as _header_struct_fields

ENVS = ("sumo-jerk-continuous-v0", "sumo-jerk-v0", "sumo-accel-v0")


def _apply(S, keys, vals):
    for k, v in zip(keys, vals):
        setattr(S, str(k), float(v))


def _twin_rewards(g, w, name, square):
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import rewards
    _apply(pkg.Settings, g["weight_keys"], g["weights"][w])
    fn = rewards.get_reward_function(name)
    out = np.zeros(g["ego4"].shape[0])
    for i in range(out.size):
        kk, e = int(g["k_count"][i]), g["ego4"][i]
        out[i] = fn((float(e[0]), float(e[1])), float(e[2]), float(e[3]), [float(x) for x in g["other_x"][i, :kk]], float(g["jerk"][i]),
                    bool(g["crashed"][i]), bool(g["arrived"][i]), square=square)
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_reward_twins_equal_the_reference(restore_settings):
    from rl_mpc_lanemerging_amd import rewards
    g = load_golden("golden_env.npz")
    for w in range(2):
        for r, name in enumerate(g["reward_names"]):
            assert np.array_equal(_twin_rewards(g, w, str(name), rewards.pow2), g["rewards"][r, w]), (w, name)
    # the branches the goldens were made to cover
    ego_s = np.array([__import__("rl_mpc_lanemerging_amd").control.get_ego_s((x, y)) for x, y in g["ego4"][:, :2]])
    live = (g["crashed"] == 0) & (g["arrived"] == 0)
    assert (live & (ego_s <= 0)).sum() > 100 and (live & (ego_s > 0)).sum() > 100
    assert g["crashed"].sum() > 20 and g["arrived"].sum() > 20
    ahead = np.array([(g["other_x"][i, :g["k_count"][i]] >= g["ego4"][i, 0]).any() for i in range(live.size)])
    behind = np.array([(g["other_x"][i, :g["k_count"][i]] < g["ego4"][i, 0]).any() for i in range(live.size)])
    assert (live & ~ahead).sum() > 50 and (live & ~behind).sum() > 50
    assert np.isfinite(g["rewards"]).all()


def test_action_twins_equal_the_reference(restore_settings):
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import rewards
    g = load_golden("golden_env.npz")
    S = pkg.Settings
    _apply(S, g["action_keys"], g["action_vals"])
    assert list(g["jerk_values"]) == [S.JERK_VALUES_DQN[i] for i in range(len(S.JERK_VALUES_DQN))]
    assert list(g["acceleration_values"]) == [S.ACCELERATION_VALUES_DQN[i] for i in range(len(S.ACCELERATION_VALUES_DQN))]
    for ei, env_id in enumerate(g["env_ids"]):
        got = np.array([rewards.handle_action(str(env_id), float(v), float(a), float(pa), float(act) if ei == 0 else int(act))
                        for v, a, pa, act in g["act_in"][ei]], dtype=np.float64)
        assert np.array_equal(got, g["act_out"][ei]), env_id
        assert (g["act_out"][ei, :, 2] != 0).sum() > 100              # every env reaches its penalty branches


def test_env_cfg_mirror_and_episode_seed():
    capi = _capi()
    from rl_mpc_lanemerging_amd import vec_env
    ctype_of = {"double": ctypes.c_double, "int32_t": ctypes.c_int32, "double *": ctypes.POINTER(ctypes.c_double),
                "stmpc_policy_features_cfg *": ctypes.POINTER(capi.FeaturesCfg)}
    want = _header_struct_fields("stmpc_env_cfg")
    have = list(capi.EnvCfg._fields_)
    assert [n for n, _ in want] == [n for n, _ in have]
    assert [ctype_of[t] for _, t in want] == [t for _, t in have]
    header = open(os.path.join(REPO, "include", "stmpc.h")).read()
    for name, val in (("STMPC_ENV_NSTAT", capi.ENV_NSTAT), ("STMPC_ENV_LOG_COLS", capi.ENV_LOG_COLS), ("STMPC_REWARD_ST", capi.REWARD_ST),
                      ("STMPC_ENV_ACCELERATION", capi.ENV_ACCELERATION), ("STMPC_ABI_VERSION", capi.ABI_VERSION)):
        assert "#define %s %d" % (name, val) in " ".join(header.split()), name
    for seed in (0, 1, 7, 2 ** 63 + 5, 2 ** 64 - 1):
        for j in (0, 1, 2, 3, 1000, 2 ** 32 - 1):
            assert capi.env_episode_seed(seed, j) == vec_env.episode_seed(seed, j)
    assert vec_env.episode_seed(5, 0) == 5 and len({vec_env.episode_seed(5, j) for j in range(1000)}) == 1000


def test_settings_defaults_and_train_config(restore_settings):
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import rewards
    S = pkg.Settings
    assert S.GYM_ENVIRONMENT == "sumo-jerk-continuous-v0" and S.REWARD_FUNCTION == "Continuous"
    assert (S.CRASH_REWARD, S.SUCCESS_REWARD, S.TIME_REWARD) == (-10, 10, -0.1)
    assert (S.WT_SMOOTH, S.WT_SAFE, S.WT_EFFICIENT, S.MIN_FOLLOW_DISTANCE) == (0.1, 0.1, 0.01, 3)
    assert (S.ALT_V_WEIGHT, S.ALT_A_WEIGHT, S.ALT_J_WEIGHT, S.ALT_D_WEIGHT) == (0.0001, 0.01, 0.05, 0.05)
    assert S.INVALID_ACTION_PENALTY == 0.0 and S.MAX_EPISODE_LENGTH == 100
    assert S.JERK_VALUES_DQN == {0: -5, 1: -2.5, 2: 0, 3: 2.5, 4: 5} and len(S.ACCELERATION_VALUES_DQN) == 20
    g = load_golden("golden_env.npz")
    d = dict(zip([str(k) for k in g["weight_keys"]], g["weights"][0]))
    assert all(float(getattr(S, k)) == v for k, v in d.items())
    S.load_from_file(os.path.join(REPO, "tests", "golden", "train_moderate_1.json"))          # the reference's configs/train_moderate_1.json
    assert S.REWARD_FUNCTION == "Slotted Jerk" and S.ALT_J_WEIGHT == 0.1 and S.OTHER_CAR_SPEED == 11.0
    assert rewards.get_reward_function() is rewards.slotted_reward_with_jerk
    with pytest.raises(ValueError):
        rewards.get_reward_function("Sparse")


def test_vec_env_validates_names(restore_settings):
    _capi()
    from rl_mpc_lanemerging_amd import vec_env
    with pytest.raises(ValueError):
        vec_env.MergeVecEnv(4, env_id="sumo-jerk-v1")
    with pytest.raises(ValueError):
        vec_env.MergeVecEnv(4, reward="Sparse")
    with pytest.raises(ValueError):
        vec_env.env_cfg("sumo-accel-v0", "Dense")
    c = vec_env.env_cfg("sumo-accel-v0", "ST")
    assert c.n_action_values == 20 and c.reward_function == 3 and c.action_mode == 2
    lo, hi = vec_env.observation_bounds()
    assert lo.shape == (20,) and (lo == -1).all() and (hi == 1).all()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


@pytest.mark.gpu
def test_gpu_reward_kernel_equals_the_goldens(gpu_ctx, restore_settings):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import rewards, vec_env
    g = load_golden("golden_env.npz")
    n, K = g["ego4"].shape[0], g["other_x"].shape[1]
    ego, k = _dev(g["ego4"], torch.float64), _dev(g["k_count"], torch.int32)
    ox, jerk = _dev(g["other_x"], torch.float64), _dev(g["jerk"], torch.float64)
    cr, ar = _dev(g["crashed"], torch.int32), _dev(g["arrived"], torch.int32)
    checked = 0
    for w in range(2):
        for r, name in enumerate(g["reward_names"]):
            _apply(pkg.Settings, g["weight_keys"], g["weights"][w])
            cfg = vec_env.env_cfg("sumo-jerk-continuous-v0", str(name))
            out = torch.empty(n, dtype=torch.float64, device="cuda")
            gpu_ctx.env_reward(cfg, n, K, ego.data_ptr(), k.data_ptr(), ox.data_ptr(), jerk.data_ptr(), cr.data_ptr(), ar.data_ptr(), out.data_ptr())
            got = out.cpu().numpy()
            ref = g["rewards"][r, w]
            # the reference squares with libm pow (not correctly rounded), the kernel with x * x: states where that differs are pinned to the twin
            # with the correctly rounded square instead, every other one to the reference
            twin = _twin_rewards(g, w, str(name), rewards.mul2)
            differs = twin != ref
            assert differs.sum() <= 0.01 * n, (name, differs.sum())
            assert np.array_equal(got[~differs], ref[~differs]), (w, name)
            assert np.array_equal(got, twin), (w, name)
            checked += int((~differs).sum())
    assert checked > 15000


def _run_parity(gpu_ctx, env_id, reward_name, n=256, ticks=200, seed=11):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, episodes, rewards, vec_env
    S = pkg.Settings
    ctx_b = _capi.Context(-1)
    env = vec_env.MergeVecEnv(n, env_id=env_id, seed=seed, reward=reward_name, autoreset=False, ctx=gpu_ctx)
    obs = env.reset()
    cfg_b = episodes.sim_cfg(seed, float(S.MAX_EPISODE_LENGTH))
    ctx_b.sim_init(cfg_b, n)
    K = 32
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")
    ego5, kb, oxb, ovb, oab = z(n, 5), z(n, dtype=torch.int32), z(n, K), z(n, K), z(n, K)
    fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=False)
    feat = z(n, env.obs_dim, dtype=torch.float32)
    params = _capi.Params.from_settings(S)
    fn = rewards.get_reward_function(reward_name)
    rng = np.random.default_rng(seed)
    prev_a = np.zeros(n)

    def view_b():
        ctx_b.sim_view(cfg_b, n, K, ego5.data_ptr(), kb.data_ptr(), oxb.data_ptr(), ovb.data_ptr(), oab.data_ptr())
        e4 = ego5[:, :4].contiguous()                       # (the features take [n][4] ego rows)
        ctx_b.policy_features_device(fcfg, n, K, 1, e4.data_ptr(), kb.data_ptr(), oxb.data_ptr(), ovb.data_ptr(), oab.data_ptr(), 0, feat.data_ptr(), env.obs_dim)
        return ego5.cpu().numpy(), kb.cpu().numpy(), oxb.cpu().numpy(), feat.cpu().numpy()

    e5, kk, xx, ff = view_b()
    assert np.array_equal(obs.cpu().numpy(), ff)
    seen = set()
    for t in range(ticks):
        status0 = ctx_b.sim_read(n)[0]
        if env_id == "sumo-jerk-continuous-v0":
            act = rng.normal(0.0, 4.0, n)
        else:
            act = rng.integers(0, env.action_space["n"], n).astype(np.int32)
        cmd, pj, inv = np.zeros(n), np.zeros(n), np.zeros(n)
        for i in range(n):
            cmd[i], pj[i], inv[i] = rewards.handle_action(env_id, float(e5[i, 2]), float(e5[i, 3]), float(prev_a[i]),
                                                          float(act[i]) if env.continuous else int(act[i]))
        o, r, term, trunc, info = env.step(torch.as_tensor(act, device="cuda"))
        ctx_b.sim_step(params, cfg_b, n, _dev(cmd).data_ptr())
        sa, sb = gpu_ctx.sim_read(n), ctx_b.sim_read(n)
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y), t
        status = sb[0]
        e5, kk, xx, ff = view_b()
        o, r, term, trunc = o.cpu().numpy(), r.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy()
        for i in range(n):
            if status0[i] != 0:
                assert r[i] == 0.0 and not term[i] and not trunc[i]
                continue
            crashed, arrived = status[i] == 2, status[i] == 1
            if crashed or arrived:
                want = fn((0, 0), 0, 0, [], pj[i], crashed, arrived, square=rewards.mul2) + inv[i]
                assert not o[i].any()
            else:
                jerk = (float(e5[i, 3]) - prev_a[i]) / S.TICK_LENGTH
                want = fn((float(e5[i, 0]), float(e5[i, 1])), float(e5[i, 2]), float(e5[i, 3]), [float(x) for x in xx[i, :kk[i]]], jerk, False, False,
                          square=rewards.mul2) + inv[i]
                assert np.array_equal(o[i], ff[i]), (t, i)
                if status[i] == 0:
                    prev_a[i] = e5[i, 3]
            assert r[i] == want, (t, i, r[i], want)
            assert bool(term[i]) == (crashed or arrived) and bool(trunc[i]) == (status[i] == 3)
            seen.add(int(status[i]))
            if inv[i] != 0:
                seen.add("penalty")
    gpu_ctx.check_error()
    ctx_b.close()
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,reward_name", [("sumo-jerk-continuous-v0", "Continuous"), ("sumo-jerk-v0", "ST"), ("sumo-accel-v0", "Slotted Jerk")])
def test_gpu_step_parity_with_world_and_host_twins(env_id, reward_name, gpu_ctx, restore_settings):
    import rl_mpc_lanemerging_amd as pkg
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.Settings.INVALID_ACTION_PENALTY = -1.0
    pkg.Settings.MAX_EPISODE_LENGTH = 30         # (150 ticks: the 200 compared ticks see timeouts too)
    seen = _run_parity(gpu_ctx, env_id, reward_name)
    assert 0 in seen and 3 in seen and "penalty" in seen, seen


@pytest.mark.gpu
def test_gpu_autoreset_is_exact(gpu_ctx, restore_settings):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, episodes, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    S = pkg.Settings
    S.MAX_EPISODE_LENGTH = 6.0                   # 30 ticks: every environment ends an episode at least twice in 70 ticks
    n, seed, K = 256, 23, 32
    a = vec_env.MergeVecEnv(n, seed=seed, reward="Continuous", autoreset=True, ctx=gpu_ctx)
    ctx_b = _capi.Context(-1)
    b = vec_env.MergeVecEnv(n, seed=seed, reward="Continuous", autoreset=False, ctx=ctx_b)
    obs_a = a.reset().clone()
    b.reset()
    cfg = episodes.sim_cfg(seed, float(S.MAX_EPISODE_LENGTH))
    fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=False)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")

    def world(ctx, c=cfg):
        ego5, k, ox, ov, oa, feat = z(n, 5), z(n, dtype=torch.int32), z(n, K), z(n, K), z(n, K), z(n, 20, dtype=torch.float32)
        ctx.sim_view(c, n, K, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr())
        e4 = ego5[:, :4].contiguous()
        ctx.policy_features_device(fcfg, n, K, 1, e4.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr(), 0, feat.data_ptr(), 20)
        return ctx.sim_read(n), ego5.cpu().numpy(), feat.cpu().numpy()

    # episode 0 is sim_init with the same seed, bit for bit
    ctx_c = _capi.Context(-1)
    ctx_c.sim_init(cfg, n)
    ra, ea, fa = world(gpu_ctx)
    rc, ec, fc = world(ctx_c)
    for x, y in zip(ra, rc):
        assert np.array_equal(x, y)
    assert np.array_equal(ea, ec) and np.array_equal(fa, fc) and np.array_equal(obs_a.cpu().numpy(), fc)
    # the start states of episodes 1 and 2: environment e of a fresh sim_init seeded episode_seed(seed, j)
    fresh = {}
    for j in (1, 2):
        ctx_c.sim_init(episodes.sim_cfg(vec_env.episode_seed(seed, j), float(S.MAX_EPISODE_LENGTH)), n)
        fresh[j] = world(ctx_c)
    ctx_c.close()
    rng = np.random.default_rng(5)
    episode = np.zeros(n, np.int64)
    finals0 = {}
    for t in range(70):
        act = torch.as_tensor(rng.normal(0.0, 3.0, n), device="cuda")
        o, r, term, trunc, info = a.step(act)
        b.step(act)
        done = (term | trunc).cpu().numpy()
        ra, ea, fa = world(gpu_ctx)
        rb, eb, fb = world(ctx_b)
        o = o.cpu().numpy()
        fs = info["final_stats"].cpu().numpy()
        for i in np.nonzero(done)[0]:
            episode[i] += 1
            j = int(episode[i])
            if j == 1:
                finals0[i] = fs[i].copy()
            if j in fresh:
                (st_, tk_, acc_, ego4_), e5, ff = fresh[j]
                assert ra[0][i] == 0 and ra[1][i] == 0 and np.array_equal(ra[2][i], acc_[i]) and np.array_equal(ra[3][i], ego4_[i]), (t, i, j)
                assert np.array_equal(ea[i], e5[i]) and np.array_equal(fa[i], ff[i]) and np.array_equal(o[i], ff[i]), (t, i, j)
        # environments still in episode 0 are untouched: the no-autoreset run has the same state
        same = episode == 0
        for x, y in zip(ra, rb):
            assert np.array_equal(x[same], y[same]), t
        assert np.array_equal(ea[same], eb[same])
    assert (episode >= 2).all(), episode.min()
    # the final statistics of episode 0 are the no-autoreset run's world row
    st_b, tk_b, acc_b, _ = ctx_b.sim_read(n)
    for i, row in finals0.items():
        assert np.array_equal(row[:12], acc_b[i]) and row[12] == st_b[i] and row[13] == tk_b[i], i
    stats = a.drain_episode_stats()
    assert len(stats["env"]) == int(episode.sum())
    assert set(stats) >= {"crashed", "merged", "timed_out", "mean_speed", "max_speed", "mean_abs_jerk", "closest_distance", "time_taken", "ticks",
                          "status", "episode_return", "env", "episode"}
    ctx_b.close()


@pytest.mark.gpu
def test_gpu_terminal_semantics(gpu_ctx, restore_settings):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    S = pkg.Settings
    S.INVALID_ACTION_PENALTY = -1.0
    n = 256
    # half the egos keep their start speed (arrivals), half push a jerk beyond the Box (penalised; crashes); the Slotted Jerk reward of a crash /
    # an arrival is CRASH_REWARD / SUCCESS_REWARD plus the penalty, that of the other two functions -10 / 10 plus the penalty
    for reward_name, crash_r, success_r in (("Slotted Jerk", S.CRASH_REWARD, S.SUCCESS_REWARD), ("Continuous", -10.0, 10.0), ("ST", -10.0, 10.0)):
        env = vec_env.MergeVecEnv(n, seed=3, reward=reward_name, autoreset=False, ctx=gpu_ctx)
        env.reset()
        push = np.arange(n) % 2 == 1
        seen = set()
        for t in range(260):
            act = torch.as_tensor(np.where(push, 12.0, 0.0), device="cuda")
            o, r, term, trunc, info = env.step(act)
            term_h, r_h = term.cpu().numpy(), r.cpu().numpy()
            if term_h.any():
                fo = info["final_observation"].cpu().numpy()[term_h]
                status = info["status"].cpu().numpy()[term_h]
                assert not fo.any() and not o.cpu().numpy()[term_h].any()
                rr = r_h[term_h]
                ok = ((status == 2) & ((rr == crash_r) | (rr == crash_r - 0.2))) | ((status == 1) & ((rr == success_r) | (rr == success_r - 0.2)))
                assert ok.all(), (reward_name, rr[~ok], status[~ok])
                seen |= set(status.tolist())
        assert {1, 2} <= seen, (reward_name, seen)
    # a forced timeout: truncated, a real final observation, a reward from the state
    S.MAX_EPISODE_LENGTH = 2.0
    env = vec_env.MergeVecEnv(n, seed=4, reward="Continuous", autoreset=True, ctx=gpu_ctx)
    env.reset()
    for t in range(10):
        o, r, term, trunc, info = env.step(torch.zeros(n, dtype=torch.float64, device="cuda"))
    trunc_h = trunc.cpu().numpy()
    assert trunc_h.all() and not term.cpu().numpy().any()
    fo = info["final_observation"].cpu().numpy()
    assert np.abs(fo).sum(axis=1).min() > 0 and not np.array_equal(fo, o.cpu().numpy())
    assert (info["status"].cpu().numpy() == 3).all() and (info["final_stats"].cpu().numpy()[:, 13] == 10).all()
    assert np.isfinite(r.cpu().numpy()).all() and (r.cpu().numpy() < 0).all()
    # an action index out of range: a latched STMPC_EINVAL, not a fault
    env = vec_env.MergeVecEnv(n, env_id="sumo-jerk-v0", seed=4, reward="Slotted", ctx=gpu_ctx)
    env.reset()
    act = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    act[7] = 99
    env.step(act)
    with pytest.raises(_capi.StmpcError) as ei:
        env.check_error()
    assert ei.value.code == _capi.STMPC_EINVAL
    env.step(torch.full((n,), 2, dtype=torch.int32, device="cuda"))
    env.check_error()                            # (cleared)


@pytest.mark.gpu
def test_gpu_pretrained_actor_drives_the_env(gpu_ctx, restore_settings):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.Settings.load_from_file(os.path.join(REPO, "tests", "golden", "train_moderate_1.json"))
    n = 1024
    env = vec_env.MergeVecEnv(n, seed=9, ctx=gpu_ctx)
    pol = actor.DDPGActor("ddpg_moderate1", n, gpu_ctx, pkg.Settings, engine="torch")
    obs = env.reset()
    finished = np.zeros(n, bool)
    all_finite = torch.ones((), dtype=torch.bool, device="cuda")      # every tick's rewards, checked at the drains (no extra sync)
    rows = []
    total = 0
    with torch.no_grad():
        for t in range(1000):
            feat = torch.cat([obs, 0.001 * env.episode_ticks.to(torch.float32).unsqueeze(1)], dim=1)      # TimeFeature: ticks of the episode
            jerk = pol.forward(feat).to(torch.float64)
            obs, r, term, trunc, info = env.step(jerk)
            all_finite &= torch.isfinite(r).all()
            if t % 100 == 99:
                assert bool(all_finite), t
                s = env.drain_episode_stats()
                finished[s["env"]] = True
                total += len(s["env"])
                rows.append(s)
    assert finished.all()
    assert set(rows[0]) >= {"crashed", "merged", "timed_out", "mean_speed", "max_speed", "mean_abs_jerk", "closest_distance", "mean_closest_distance",
                            "time_taken", "ticks", "status", "time_to_merge", "mean_disruption", "max_disruption", "total_disruption", "disruption_time"}
    print("ddpg_moderate1 on the env: %d episodes in 1000 ticks of %d environments" % (total, n))


@pytest.mark.gpu
def test_gpu_step_does_not_synchronise(gpu_ctx, restore_settings):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    env = vec_env.MergeVecEnv(512, seed=1, ctx=gpu_ctx)
    env.reset()
    act = torch.zeros(512, dtype=torch.float64, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(20):
            env.step(act)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    env.drain_episode_stats()


@pytest.mark.gpu
def test_gpu_context_holds_one_world(gpu_ctx, restore_settings):
    """The episode tick counter is the world's; a context holds one world (a second env or a plain sim_init ends the first), and the action mode
    of a step must be the reset's."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, episodes, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.Settings.MAX_EPISODE_LENGTH = 3.0                     # 15 ticks: resets within the run
    n = 128
    env = vec_env.MergeVecEnv(n, seed=2, reward="Slotted", ctx=gpu_ctx)
    env.reset()
    assert not env.episode_ticks.cpu().numpy().any()
    ticks = np.zeros(n, np.int64)
    for t in range(40):
        _, _, term, trunc, _ = env.step(torch.zeros(n, dtype=torch.float64, device="cuda"))
        ticks += 1
        ticks[(term | trunc).cpu().numpy()] = 0
        assert np.array_equal(env.episode_ticks.cpu().numpy(), ticks), t
    assert np.array_equal(gpu_ctx.sim_read(n)[1], ticks)
    # a step with another action mode than the reset's: STMPC_EINVAL, nothing launched
    other = vec_env.env_cfg("sumo-accel-v0", "Slotted")
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")
    act, obs, rew, tr = z(n, dtype=torch.int32), z(n, 20, dtype=torch.float32), z(n), z(n, dtype=torch.bool)
    with pytest.raises(_capi.StmpcError) as ei:
        gpu_ctx.env_step(env.params, env.sim_cfg, other, n, act.data_ptr(), obs.data_ptr(), 20, rew.data_ptr(), tr.data_ptr(), tr.data_ptr())
    assert ei.value.code == _capi.STMPC_EINVAL
    # a second env on the same context ends the first
    env2 = vec_env.MergeVecEnv(n, seed=3, reward="Slotted", ctx=gpu_ctx)
    env2.reset()
    with pytest.raises(RuntimeError):
        env.step(torch.zeros(n, dtype=torch.float64, device="cuda"))
    env2.step(torch.zeros(n, dtype=torch.float64, device="cuda"))
    # so does a plain world init on it
    gpu_ctx.sim_init(episodes.sim_cfg(4, 3.0), n)
    with pytest.raises(_capi.StmpcError):
        env2.step(torch.zeros(n, dtype=torch.float64, device="cuda"))
    # by default every env has a context of its own
    a, b = vec_env.MergeVecEnv(n, seed=5), vec_env.MergeVecEnv(n, seed=6)
    assert a.ctx is not b.ctx
    a.reset(), b.reset()
    a.step(torch.zeros(n, dtype=torch.float64, device="cuda")), b.step(torch.zeros(n, dtype=torch.float64, device="cuda"))
    gpu_ctx.check_error()
