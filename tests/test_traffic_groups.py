"""Traffic groups on the GPU (csrc/stmpc_sim_groups_kernels.hpp; stmpc_sim_*_groups_* / stmpc_env_*_groups_* of include/stmpc.h; the ``traffic``
arguments of episodes.EpisodeRunner, vec_env.MergeVecEnv, learner.DDPGPopulation and episodes.cross_matrix).

The contract: group g of a grouped world is, bit for bit, the lone world of n_per_group environments made from cfgs[g].  Every comparison here is
``np.array_equal`` on the raw bits, against LONE objects built through the plain entries with the group's traffic in the global Settings -- the
path a user had before groups existed.  The shape is the smallest that can go wrong: G = 3 groups (low, default, fast; three seeds),
n_per_group = 24 (no multiple of the 64-lane workgroup: every group has a masked tail, and a workgroup that spanned groups would mix cfgs from row
24 on), Kmax = 16.  No tolerance anywhere.
"""
import numpy as np
import pytest

from stmpc_testlib import pkg as _pkg, bits as _bits, same as _same, settings_of as _settings_of, linit as _linit

NPG, G, KMAX, TICKS = 24, 3, 16, 40
N = G * NPG
NAMES, SEEDS = ("low", "default", "fast"), (31, 32, 33)
_cache = {}


def _traffic(names=NAMES, seeds=SEEDS):
    from rl_mpc_lanemerging_amd import episodes
    return [dict(episodes.TRAFFIC_TYPES[t], seed=s) for t, s in zip(names, seeds)]


def _sl(g):
    return slice(g * NPG, (g + 1) * NPG)


# ---- cases 1-4: the world under the ST controller -----------------------------------------------------------------------------------------------
def _world_snapshot(r):
    """sim_read and sim_view of a runner's world, as host arrays."""
    import torch
    n, dev = r.n, r.d_ego5.device
    ego5, k = torch.zeros(n, 5, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    ox, ov, oa = (torch.zeros(n, KMAX, dtype=torch.float64, device=dev) for _ in range(3))
    r.ctx.sim_view(r.cfg, n, KMAX, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr())
    status, ticks, acc, ego4 = r.ctx.sim_read(n)
    r.ctx.check_error()
    return {"status": status, "ticks": ticks, "acc": acc, "ego4": ego4, "ego5": ego5.cpu().numpy(), "k": k.cpu().numpy(), "ox": ox.cpu().numpy(),
            "ov": ov.cpu().numpy(), "oa": oa.cpu().numpy()}


def _st_run(gpu_ctx, key, n, seed=0, traffic=None, lone_of=None):
    """TICKS ticks of ``n`` environments under the ST controller; snapshots at init, after every 8th tick and at the end.  ``traffic``: a grouped
    world; ``lone_of``: a plain world with that group's traffic in the Settings.  Computed once per key, then only read."""
    if key in _cache:
        return _cache[key]
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import episodes
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    with _settings_of(lone_of or {}):
        r = episodes.EpisodeRunner(n, seed=seed, controller="st", ctx=gpu_ctx, kmax=KMAX, traffic=traffic)
    assert gpu_ctx.sim_groups() == ((len(traffic), n // len(traffic)) if traffic is not None else (0, 0))
    snaps = [_world_snapshot(r)]
    for t in range(1, TICKS + 1):
        r.tick()
        if t % 8 == 0 or t == TICKS:
            snaps.append(_world_snapshot(r))
    out = {"snaps": snaps, "result": r.result()}
    _cache[key] = out
    return out


def _assert_slices(grouped, g, lone, label, at=None):
    for i, (a, b) in enumerate(zip(grouped["snaps"], lone["snaps"])):
        if at is not None and i not in at:
            continue
        for k in b:
            assert _same(a[k][_sl(g)], b[k]), (label, "group %d" % g, "snapshot %d" % i, k)


@pytest.mark.gpu
def test_gpu_init_of_every_group_is_the_lone_world(gpu_ctx, restore_settings):
    tr = _traffic()
    grouped = _st_run(gpu_ctx, "grouped", N, traffic=tr)
    for g in range(G):
        lone = _st_run(gpu_ctx, ("lone", g), NPG, seed=SEEDS[g], lone_of=tr[g])
        _assert_slices(grouped, g, lone, "init", at=(0,))
    s0 = grouped["snaps"][0]
    assert (s0["status"] == 0).all() and (s0["ticks"] == 0).all() and (s0["k"] > 0).any()
    # the three groups are different worlds: other speeds in the view, other vehicle counts
    assert s0["ov"][_sl(0)].max() <= 7.0 < s0["ov"][_sl(2)].max() <= 15.0
    assert not np.array_equal(s0["ox"][_sl(0)], s0["ox"][_sl(1)])


@pytest.mark.gpu
def test_gpu_stepping_every_group_is_the_lone_world(gpu_ctx, restore_settings):
    tr = _traffic()
    grouped = _st_run(gpu_ctx, "grouped", N, traffic=tr)
    assert len(grouped["snaps"]) == 1 + TICKS // 8
    for g in range(G):
        lone = _st_run(gpu_ctx, ("lone", g), NPG, seed=SEEDS[g], lone_of=tr[g])
        _assert_slices(grouped, g, lone, "stepping")
        for k, v in lone["result"].items():
            assert _same(grouped["result"][k][_sl(g)], v), (g, k)
    assert np.array_equal(grouped["result"]["traffic_group"], np.arange(N) // NPG) and "traffic_group" not in _cache[("lone", 0)]["result"]
    last = grouped["snaps"][-1]
    assert last["ticks"].max() == TICKS and (last["ego4"][:, 2] > 0).any() and (last["acc"][:, 4] > 0).all()
    # the grouped run itself is reproducible
    again = _st_run(gpu_ctx, "grouped again", N, traffic=tr)
    for a, b in zip(grouped["snaps"], again["snaps"]):
        for k in a:
            assert _same(a[k], b[k]), ("reproducible", k)


@pytest.mark.gpu
def test_gpu_one_group_is_the_plain_world(gpu_ctx, restore_settings):
    tr = _traffic()
    plain = _st_run(gpu_ctx, ("lone", 0), NPG, seed=SEEDS[0], lone_of=tr[0])
    one = _st_run(gpu_ctx, "one group", NPG, traffic=tr[:1])
    for a, b in zip(one["snaps"], plain["snaps"]):
        for k in a:
            assert _same(a[k], b[k]), k
    # and a one-group world of the default seed is the plain world of that seed
    dflt = _st_run(gpu_ctx, "one group, default seed", NPG, seed=SEEDS[0], traffic=["low"])
    for k in plain["snaps"][-1]:
        assert _same(dflt["snaps"][-1][k], plain["snaps"][-1][k]), k


@pytest.mark.gpu
def test_gpu_groups_are_independent(gpu_ctx, restore_settings):
    """Only group 1's interval and seed change: groups 0 and 2 stay bit-identical, group 1 does not."""
    tr = _traffic()
    before = _st_run(gpu_ctx, "grouped", N, traffic=tr)
    other = [tr[0], dict(tr[1], BASE_TRAFFIC_INTERVAL=1.5, seed=77), tr[2]]
    after = _st_run(gpu_ctx, "grouped, group 1 changed", N, traffic=other)
    for a, b in zip(before["snaps"], after["snaps"]):
        for k in a:
            assert _same(a[k][_sl(0)], b[k][_sl(0)]) and _same(a[k][_sl(2)], b[k][_sl(2)]), k
    assert not _same(before["snaps"][0]["ox"][_sl(1)], after["snaps"][0]["ox"][_sl(1)])
    assert not _same(before["snaps"][-1]["acc"][_sl(1)], after["snaps"][-1]["acc"][_sl(1)])


# ---- case 5: the vector environment through its autoresets ---------------------------------------------------------------------------------------
def _env_run(gpu_ctx, n, actions, seed=0, traffic=None, lone_of=None):
    import torch
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides({"MAX_EPISODE_LENGTH": 3.0})              # 15 ticks: every environment starts at least its third episode within 40 steps
    with _settings_of(lone_of or {}):
        env = vec_env.MergeVecEnv(n, env_id="sumo-jerk-continuous-v0", seed=seed, ctx=gpu_ctx, traffic=traffic)
    steps = [{"obs": env.reset().cpu().numpy()}]
    for a in actions:
        obs, rew, term, trunc, info = env.step(torch.as_tensor(a, device=env.device))
        steps.append({"obs": obs.cpu().numpy(), "reward": rew.cpu().numpy(), "terminated": term.cpu().numpy(), "truncated": trunc.cpu().numpy(),
                      "final_observation": info["final_observation"].cpu().numpy(), "final_stats": info["final_stats"].cpu().numpy(),
                      "ticks": env.episode_ticks.cpu().numpy()})
    return steps, env.drain_episode_stats()


@pytest.mark.gpu
def test_gpu_vec_env_groups_equal_lone_envs_through_autoreset(gpu_ctx, restore_settings):
    tr = _traffic()
    rng = np.random.default_rng(5)
    actions = rng.uniform(-1.5, 1.5, (TICKS, N))                   # (mostly valid jerks; 15-tick episodes end out of time unless they crash)
    steps, log = _env_run(gpu_ctx, N, actions, traffic=tr)
    # a condition on the inputs: every environment was reset at least twice
    assert np.bincount(log["env"], minlength=N).min() >= 2, np.bincount(log["env"], minlength=N)
    assert np.array_equal(log["traffic_group"], log["env"] // NPG) and set(log["traffic_group"]) == {0, 1, 2}
    for g in range(G):
        lsteps, llog = _env_run(gpu_ctx, NPG, actions[:, _sl(g)], seed=SEEDS[g], lone_of=tr[g])
        for i, (a, b) in enumerate(zip(steps, lsteps)):
            for k in b:
                assert _same(a[k][_sl(g)], b[k]), ("group %d" % g, "step %d" % i, k)
        # the log: the same rows as sets; the slot order is an atomic's, both sides are sorted by (environment, episode)
        mine = log["traffic_group"] == g
        assert mine.sum() == len(llog["env"]) and (llog["traffic_group"] == 0).all()
        assert np.array_equal(log["env"][mine], llog["env"] + g * NPG)
        for k in llog:
            if k not in ("env", "traffic_group"):
                assert _same(log[k][mine], llog[k]), ("group %d" % g, "log", k)
    final = steps[-1]
    assert not _same(final["obs"][_sl(0)], final["obs"][_sl(1)]) and (log["episode"] >= 1).any()


# ---- case 6: a population of learners, member m on traffic m -----------------------------------------------------------------------------------
CAP, STEPS, BATCH = 200, 12, 16
L_SEEDS = (11, 12, 13)
GAMMA, TAU, NOISE = (0.99, 0.95, 0.9), (0.005, 0.01, 0.02), (0.1, 0.2, 0.05)
LR_Q, LR_PI = (2e-4, 1e-3, 5e-4), (2e-4, 3e-4, 1e-4)
REPLAY_START = (0, 48, 120)


def _lcfg(m):
    from rl_mpc_lanemerging_amd import learner
    return learner.DDPGConfig(n_obs=20, batch=BATCH, capacity=CAP, replay_start=REPLAY_START[m], gamma=GAMMA[m], tau=TAU[m], noise=NOISE[m], lr_q=LR_Q[m],
                              lr_pi=LR_PI[m])


def _train(env, L, lr_q, lr_pi):
    """STEPS steps of act -> step -> push -> update; the actions of every step."""
    actions = []
    obs = env.reset()
    for _ in range(STEPS):
        ticks = env.episode_ticks.clone()
        action = L.act(obs, ticks, noise=True).clone()
        actions.append(action.cpu().numpy())
        nobs, r, term, trunc, info = env.step(action)
        L.push(obs, ticks, action, r, nobs, term, trunc, final_obs=info["final_observation"])
        L.update(1, lr_q=lr_q, lr_pi=lr_pi)
        obs = nobs
    env.check_error()
    return np.stack(actions)


def _lsnapshot(ctx, L, stats):
    sd = L.state_dict()
    return {"params": sd["params"], "counters": sd["counters"], "ring": ctx.ddpg_replay_read(L.handle, 0, CAP), "stats": np.array(stats, dtype=np.float64)}


@pytest.mark.gpu
def test_gpu_population_on_traffic_groups_equals_lone_learners_on_lone_envs(gpu_ctx, restore_settings):
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, learner, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    tr = _traffic()
    env = vec_env.MergeVecEnv(N, env_id="sumo-jerk-continuous-v0", ctx=gpu_ctx, traffic=tr)
    pop = learner.DDPGPopulation(env, [_lcfg(m) for m in range(G)], seeds=list(L_SEEDS), init=[_linit(m) for m in range(G)])
    acts = _train(env, pop, list(LR_Q), list(LR_PI))
    ps = pop.stats()
    snaps = [_lsnapshot(gpu_ctx, pop.member(m), [ps["critic_loss"][m], ps["mean_q"][m], ps["fill"][m], ps["updates"][m]]) for m in range(G)]
    assert snaps[2]["counters"][2] == 7 < snaps[1]["counters"][2] == 10 < snaps[0]["counters"][2] == 12      # updates done: the gates are per member
    for m in range(G):
        with _settings_of(tr[m]):
            lenv = vec_env.MergeVecEnv(NPG, env_id="sumo-jerk-continuous-v0", seed=SEEDS[m], ctx=gpu_ctx)
        L = learner.DDPGLearner(lenv, _lcfg(m), seed=L_SEEDS[m], init=_linit(m))
        lacts = _train(lenv, L, LR_Q[m], LR_PI[m])
        for i in range(STEPS):
            assert _same(acts[i][_sl(m)], lacts[i]), ("member %d" % m, "actions of step %d" % i)
        s = L.stats()
        want = _lsnapshot(gpu_ctx, L, [s["critic_loss"], s["mean_q"], s["fill"], s["updates"]])
        for slot in capi.DDPG_SLOTS:
            for k in learner.TENSORS:
                assert _same(snaps[m]["params"][slot][k], want["params"][slot][k]), (m, slot, k)
        assert _same(snaps[m]["params"]["beta_pow"], want["params"]["beta_pow"]) and np.array_equal(snaps[m]["counters"], want["counters"]), m
        assert _same(snaps[m]["ring"], want["ring"]), (m, "ring")
        assert _same(snaps[m]["stats"], want["stats"]), (m, snaps[m]["stats"], want["stats"])
    assert not np.array_equal(snaps[0]["ring"], snaps[1]["ring"])


# ---- case 7: the combined controller, reports, the cross matrix --------------------------------------------------------------------------------
ACTORS = ("low1", "medium1", "fast1")


def _combined_settings():
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import combined_bench
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    return pkg.Settings


def _assert_cell(got, sl, lone, label, extra=()):
    cols = [k for k in lone if k != "report"]
    assert "ego4" in cols and "percent_st" in cols
    for k in cols:
        assert _same(got[k][sl], lone[k]), (label, k)
    a, b = got["report"]._rec, lone["report"]._rec
    for k in ("ring", "length", "status"):
        assert _same(a[k][sl], b[k]), (label, k)
    assert _same(np.ascontiguousarray(a["acc_env"][:, sl]), b["acc_env"]), (label, "acc_env")


@pytest.mark.gpu
def test_gpu_combined_runner_reports_and_cross_matrix(gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import actor, episodes, report
    S = _combined_settings()
    tr = _traffic()
    rec = lambda: report.RecorderConfig(depth=8)
    pop = actor.ActorPopulation(list(ACTORS), NPG, gpu_ctx, S)
    got = episodes.run_episodes(N, controller="combined", policy=pop, ctx=gpu_ctx, kmax=KMAX, max_ticks=TICKS, record=rec(), traffic=tr)
    assert np.array_equal(got["traffic_group"], np.arange(N) // NPG) and np.array_equal(got["member"], got["traffic_group"])
    assert got["ticks"].max() == TICKS
    parts = got["report"].by_group(G, tr)
    lones = []
    for g in range(G):
        with _settings_of(tr[g]):
            lone = episodes.run_episodes(NPG, seed=SEEDS[g], controller="combined", policy=actor.DDPGActor(ACTORS[g], NPG, gpu_ctx, S), ctx=gpu_ctx, kmax=KMAX,
                                         max_ticks=TICKS, record=rec())
            lone_row = lone["report"].row()
        lones.append(lone)
        _assert_cell(got, _sl(g), lone, "cell %d" % g)
        # the group's report: what a recorder of the lone run holds, and the lone run's report row -- its TRAFFIC_DESCRIPTION included
        for k, v in lone["report"].profiles().items():
            assert _same(parts[g].profiles()[k], v), (g, k)
        row = parts[g].row()
        assert row["TRAFFIC_DESCRIPTION"] == lone_row["TRAFFIC_DESCRIPTION"] == "uniform-%s-%s-varying" % (tr[g]["OTHER_CAR_SPEED"], tr[g]["BASE_TRAFFIC_INTERVAL"])
        assert set(row) == set(lone_row)
        for k, v in lone_row.items():
            assert row[k] == v or (v != v and row[k] != row[k]), (g, k)
    assert [p.row()["TRAFFIC_DESCRIPTION"] for p in parts] == ["uniform-7.0-2.4-varying", "uniform-7.0-1.2-varying", "uniform-15.0-1.2-varying"]
    assert got["report"].by_member(G)[2].row()["TRAFFIC_DESCRIPTION"] == "uniform-7.0-1.2-varying"        # without traffic: the global Settings', as before
    by = episodes.summary_by_group(got, G)
    for g in range(G):
        want = episodes.summary(lones[g])
        assert set(by[g]) == set(want)
        for k, v in want.items():
            assert _same(np.float64(by[g][k]), np.float64(v)), (g, k)
    # cross_matrix: 2 models x 2 traffic types at 24 per cell = a hand-built runner of four cells, entry [i][j] the summary of cell 2 i + j
    models, traffic = ["low1", "fast1"], [tr[0], tr[2]]
    cm = episodes.cross_matrix(models, traffic, NPG, ctx=gpu_ctx, kmax=KMAX, max_ticks=TICKS)
    hand_pop = actor.ActorPopulation(["low1", "low1", "fast1", "fast1"], NPG, gpu_ctx, S)
    hand = episodes.run_episodes(4 * NPG, controller="combined", policy=hand_pop, ctx=gpu_ctx, kmax=KMAX, max_ticks=TICKS, traffic=[tr[0], tr[2], tr[0], tr[2]])
    assert len(cm["matrix"]) == 2 and all(len(r) == 2 for r in cm["matrix"]) and cm["models"] == models and cm["traffic"] == traffic
    for k, v in hand.items():
        assert _same(cm["stats"][k], v), k
    for i in range(2):
        for j in range(2):
            c = 2 * i + j
            want = episodes.summary({k: v[c * NPG:(c + 1) * NPG] for k, v in hand.items()})
            assert set(cm["matrix"][i][j]) == set(want)
            for k, v in want.items():
                assert _same(np.float64(cm["matrix"][i][j][k]), np.float64(v)), (i, j, k)
    # cell (0, 0) is model low1 on the low traffic with seed 31: group 0 of the run above
    for k in ("ego4", "ticks", "status", "percent_st"):
        assert _same(cm["stats"][k][:NPG], got[k][_sl(0)]), k
    assert not _same(cm["stats"]["ego4"][NPG:2 * NPG], cm["stats"]["ego4"][3 * NPG:])


# ---- case 8: refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refusals(gpu_ctx, restore_settings):
    """None of these launches a kernel or changes the world: sim_read before equals sim_read after, and no error is latched."""
    import torch
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, episodes, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    ctx = gpu_ctx
    tr = _traffic()
    dev = torch.device("cuda", torch.cuda.current_device())
    params = capi.Params.from_settings(pkg.Settings)
    cmd = torch.full((N,), 10.0, dtype=torch.float64, device=dev)

    def refused(match, call, *args):
        before = ctx.sim_read(ctx_n[0])
        with pytest.raises(capi.StmpcError, match=match) as e:
            call(*args)
        assert e.value.code == capi.STMPC_EINVAL
        after = ctx.sim_read(ctx_n[0])
        assert all(_same(a, b) for a, b in zip(before, after)) and ctx.sim_groups() == split[0]
        ctx.check_error()

    # an ungrouped world: the grouped step entries refuse it
    ctx.sim_init(episodes.sim_cfg(3), N)
    ctx_n, split = [N], [(0, 0)]
    refused("no traffic groups", ctx.sim_step_groups, params, N, cmd.data_ptr())
    # ... and every bad table is refused without ending it
    cfgs = lambda **kw: episodes.sim_cfgs(tr, **kw)
    refused("G must be 1 ... STMPC_SIM_GROUPS_MAX", ctx.sim_init_groups, episodes.sim_cfgs(["low"] * 65), NPG)
    refused("G must be 1 ... STMPC_SIM_GROUPS_MAX", ctx.sim_init_groups, capi.SimCfgTable([]), NPG)
    refused("n_per_group must be positive", ctx.sim_init_groups, cfgs(), 0)

    def differs(field, value):
        t = cfgs()
        setattr(t.array[1], field, value)
        return t
    for field, value in (("tick_length", 0.1), ("spawn_x", -200.0), ("despawn_x", 90.0), ("ego_start_x", -210.0), ("ego_start_y", 20.0), ("arrive_x", 60.0),
                         ("sensor_radius", 100.0), ("veh_accel", 4.0), ("veh_decel", 5.0), ("veh_min_gap", 2.0), ("veh_tau", 1.0), ("veh_emergency_decel", 10.0),
                         ("veh_length", 4.0), ("veh_width", 2.0), ("disruption_min_s", -40.0)):
        refused("must share %s \\(it differs in group 1\\)" % field, ctx.sim_init_groups, differs(field, value), NPG)
    refused("yield_overlap must be 2", ctx.sim_init_groups, differs("yield_overlap", 1), NPG)        # (make_simcfg's own refusal comes first)
    refused("base_traffic_interval must be positive", ctx.sim_init_groups, differs("base_traffic_interval", 0.0), NPG)
    t = cfgs()
    t.array[2].ego_route_xy, t.array[2].ego_route_n = None, 0
    refused("must share ego_route_xy \\(it differs in group 2", ctx.sim_init_groups, t, NPG)
    t = cfgs()
    route = np.ctypeslib.as_array(t.array[1].ego_route_xy, (t.array[1].ego_route_n, 2)).copy()
    route[3, 1] += 0.25
    t.array[1].ego_route_xy = route.ctypes.data_as(type(t.array[1].ego_route_xy))
    refused("must share ego_route_xy \\(it differs in group 1", ctx.sim_init_groups, t, NPG)
    # a grouped world: the plain step entries and a wrong N are refused
    ctx.sim_init_groups(cfgs(), NPG)
    split[0] = (G, NPG)
    assert ctx.sim_groups() == (G, NPG)
    refused("has traffic groups", ctx.sim_step, params, episodes.sim_cfg(3), N, cmd.data_ptr())
    ctx_n[0] = N
    with pytest.raises(capi.StmpcError, match="N does not match stmpc_sim_init_groups_device") as e:
        ctx.sim_step_groups(params, N - 1, cmd.data_ptr())
    assert e.value.code == capi.STMPC_EINVAL
    # the vector environment: plain step on a grouped env, grouped step on a plain env, grouped step with a wrong N
    env = vec_env.MergeVecEnv(N, env_id="sumo-jerk-continuous-v0", ctx=ctx, traffic=tr)
    obs = env.reset()
    rew, term, trunc = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.bool, device=dev), torch.zeros(N, dtype=torch.bool, device=dev)
    step_args = (cmd.data_ptr(), obs.data_ptr(), env.obs_dim, rew.data_ptr(), term.data_ptr(), trunc.data_ptr())
    refused("has traffic groups", ctx.env_step, params, env.sim_cfg, env.cfg, N, *step_args)
    with pytest.raises(capi.StmpcError, match="N does not match") as e:
        ctx.env_step_groups(params, env.cfg, N - 1, *step_args)
    assert e.value.code == capi.STMPC_EINVAL
    plain = vec_env.MergeVecEnv(N, env_id="sumo-jerk-continuous-v0", ctx=ctx)
    plain.reset()                                                  # stmpc_sim_init_device ends the grouping
    split[0] = (0, 0)
    assert ctx.sim_groups() == (0, 0)
    refused("no traffic groups", ctx.env_step_groups, params, env.cfg, N, *step_args)
    with pytest.raises(RuntimeError, match="another MergeVecEnv was reset"):
        env.step(cmd)
    # a grouped sim_init ends the environment, as the plain one does
    ctx.sim_init_groups(cfgs(), NPG)
    split[0] = (G, NPG)
    refused("N does not match stmpc_env_reset_groups_device", ctx.env_step_groups, params, env.cfg, N, *step_args)
    ctx.check_error()
