"""First-step shield controller on the GPU (csrc/stmpc_fs_kernels.hpp; stmpc_first_step* / stmpc_speed_from_jerk_device of include/stmpc.h;
first_step.py; ``controller="first_step"`` of episodes.EpisodeRunner / cross_matrix / learner.evaluate_members).

Parity is with the reference's own ``st.do_conditional_st_based_on_first_step`` (st.py:805-814) through tests/golden/golden_first_step.npz: 1620
(state, proposed speed) pairs under configs/combined_medium_1.json, every branch populated (59 crashed in the step, 23 guaranteed to crash afterwards,
1538 left to the proposal), padded from the fixture's 8 vehicle slots to Kmax = 16.  Every comparison is on the raw bits; there is no tolerance
anywhere.  The fixture batch is run ONCE (dense and sparse) and shared; the subsets (N = 1, 64, 65) are compared with its rows -- states are
independent, so a row's outputs do not depend on the batch it is solved in.
"""
import numpy as np
import pytest

from conftest import load_golden
from stmpc_testlib import pkg as _pkg, bits as _bits, same as _same, settings_of as _settings_of

KMAX = 16
TICKS = 30
GROUP_TICKS = 100       # the population / traffic test runs until egos are in the merge zone, where the shield takes over (30 ticks end on the ramp)
_cache = {}


def _settings():
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import combined_bench
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    return pkg.Settings


def _pad(a):
    out = np.zeros((a.shape[0], KMAX))
    out[:, :a.shape[1]] = a
    return out


def _fixture():
    if "g" not in _cache:
        g = load_golden("golden_first_step.npz")
        for key in ("other_x", "other_v", "next_other_x", "next_other_v"):
            g[key] = _pad(g[key])
        _cache["g"] = g
    return _cache["g"]


def _run(ctx, rows, sparse):
    """``stmpc_first_step`` on the fixture rows ``rows`` and the context's counters for that call."""
    from rl_mpc_lanemerging_amd import _capi
    S = _settings()
    g = _fixture()
    params, cfg = _capi.Params.from_settings(S), _capi.FirstStepCfg.from_settings(S, sparse_control=sparse)
    ctx.first_step_counts(reset=True)
    out = ctx.first_step(params, cfg, g["ego"][rows], g["k_count"][rows], g["other_x"][rows], g["other_v"][rows], g["start_speed"][rows])
    out["counts"] = ctx.first_step_counts(reset=True)
    return out


def _full(ctx):
    """The whole fixture, dense and sparse, and ``stmpc_st_control_batch`` of its start states: computed once, then only read."""
    if "full" not in _cache:
        from rl_mpc_lanemerging_amd import _capi
        S = _settings()
        g = _fixture()
        every = slice(0, g["ego"].shape[0])
        st = ctx.st_control_batch(_capi.Params.from_settings(S), S.TICK_LENGTH, g["ego"], g["k_count"], g["other_x"], g["other_v"])
        _cache["full"] = {"dense": _run(ctx, every, False), "sparse": _run(ctx, every, True), "st_speed": st["speed"]}
    return _cache["full"]


OUTPUTS = ("cmd_speed", "takeover", "reason", "crashed", "crash_guaranteed", "next_ego", "next_other_x", "next_other_v")


@pytest.mark.gpu
def test_gpu_decision_parity_with_the_reference(gpu_ctx, restore_settings):
    g, d = _fixture(), _full(gpu_ctx)["dense"]
    n = g["ego"].shape[0]
    assert n == 1620
    crashed = g["crashed"] != 0
    assert np.array_equal(d["crashed"], g["crashed"])
    # the predicted state, bit for bit: ego x, y, v, a, its start_s, the vehicles' positions and speeds (zero past each state's own)
    for q, name in enumerate(("x", "y", "v", "a", "start_s")):
        bad = np.nonzero(_bits(d["next_ego"][:, q]) != _bits(g["next_ego"][:, q]))[0]
        assert bad.size == 0, ("next ego " + name, bad[:8], d["next_ego"][bad[:8], q], g["next_ego"][bad[:8], q])
    assert _same(d["next_other_x"], g["next_other_x"]) and _same(d["next_other_v"], g["next_other_v"])
    # st.test_guaranteed_crash_from_state of the predicted state, wherever the step itself did not crash
    assert np.array_equal(d["crash_guaranteed"][~crashed], g["crash_guaranteed"][~crashed])
    assert np.array_equal(d["takeover"], (g["branch"] != 0).astype(np.int32))
    assert np.array_equal(d["reason"], g["branch"])
    assert (np.bincount(d["reason"], minlength=3) == [1538, 59, 23]).all()
    # where both tests fail the reason is the step's crash: the order of the reference's `or`
    both = crashed & (g["crash_guaranteed"] != 0)
    assert both.any() and (d["reason"][both] == 1).all()


@pytest.mark.gpu
def test_gpu_commanded_speed(gpu_ctx, restore_settings):
    g, full = _fixture(), _full(gpu_ctx)
    d, take = full["dense"], full["dense"]["takeover"] != 0
    assert take.sum() == 82
    assert _same(d["cmd_speed"][~take], g["start_speed"][~take])            # the proposal itself, not a recomputation of it
    assert _same(d["cmd_speed"][take], full["st_speed"][take])              # st.do_st_control(state) of the START state
    assert np.isfinite(d["cmd_speed"]).all()
    assert (d["cmd_speed"][take] != g["start_speed"][take]).any()


@pytest.mark.gpu
def test_gpu_sparse_and_dense_agree(gpu_ctx, restore_settings):
    g, full = _fixture(), _full(gpu_ctx)
    n = g["ego"].shape[0]
    for k in OUTPUTS:
        assert _same(full["sparse"][k], full["dense"][k]), k
    taken = int((g["branch"] != 0).sum())
    assert full["sparse"]["counts"] == (n, taken, taken) and full["dense"]["counts"] == (n, taken, n)
    keep, take = np.nonzero(g["branch"] == 0)[0], np.nonzero(g["branch"] != 0)[0]
    # no takeover at all (the sparse form solves nothing), nothing but takeovers, one state, one workgroup and a one-lane tail
    cases = {"none taken": keep[:64], "all taken": take[:64], "one": take[:1], "one kept": keep[:1], "tail": np.arange(600, 665)}
    assert (g["branch"][cases["tail"]] != 0).any() and (g["branch"][cases["tail"]] == 0).any()
    for label, rows in cases.items():
        want_taken = int((g["branch"][rows] != 0).sum())
        for sparse in (False, True):
            got = _run(gpu_ctx, rows, sparse)
            for k in OUTPUTS:
                assert _same(got[k], full["dense"][k][rows]), (label, sparse, k)
            assert got["counts"] == (len(rows), want_taken, want_taken if sparse else len(rows)), (label, sparse)


@pytest.mark.gpu
def test_gpu_speed_from_jerk(gpu_ctx, restore_settings):
    import torch
    from rl_mpc_lanemerging_amd import _capi, first_step
    S = _settings()
    g = _fixture()
    t, amax, amin, vmax = S.TICK_LENGTH, S.MAX_POSITIVE_ACCELERATION, S.MAX_NEGATIVE_ACCELERATION, S.MAX_SPEED
    # (speed, acceleration, jerk): the fixture's triples, then the clamps -- each limit reached exactly, passed by one ulp and by a lot, both signs of zero
    edges = [(10.0, amax, 5.0), (10.0, amax, 0.0), (10.0, np.nextafter(amax, 0), 5.0), (10.0, amax - 5.0 * t, 5.0), (10.0, amin, -5.0), (10.0, amin, 0.0),
             (10.0, amin + 5.0 * t, -5.0), (10.0, np.nextafter(amin, 0), -5.0), (0.0, 0.0, 0.0), (0.0, -0.0, -0.0), (0.0, amin, -5.0), (0.1, amin, -5.0),
             (-amin * t, amin, 0.0), (np.nextafter(-amin * t, 1), amin, 0.0), (vmax, 0.0, 0.0), (vmax, amax, 5.0), (vmax - amax * t, amax, 0.0),
             (np.nextafter(vmax, 0), 1e-9, 0.0), (vmax, -1.0, 5.0), (12.5, 0.3, -2.0), (3.0, 100.0, 5.0), (3.0, -100.0, -5.0)]
    v = np.concatenate([g["ego"][:, 2], [e[0] for e in edges]])
    a = np.concatenate([g["ego"][:, 3], [e[1] for e in edges]])
    j = np.concatenate([g["jerk"], [e[2] for e in edges]])
    n = v.size
    assert n % 64 != 0
    want = np.array([first_step.get_ego_speed_from_jerk(float(v_), float(a_), float(j_)) for v_, a_, j_ in zip(v, a, j)], dtype=np.float64)
    assert _same(want[:g["jerk"].size], g["start_speed"])                      # the host function is the one the fixture was recorded with
    assert (want == 0).any() and (want == vmax).any()
    ego5 = np.zeros((n, 5))
    ego5[:, 2], ego5[:, 3] = v, a
    dev = torch.device("cuda", torch.cuda.current_device())
    d_ego5, d_j = torch.as_tensor(ego5, device=dev), torch.as_tensor(j, device=dev)
    got = first_step.speed_from_jerk_device(gpu_ctx, _capi.Params.from_settings(S), t, d_ego5, d_j)
    torch.cuda.synchronize()
    bad = np.nonzero(_bits(got.cpu().numpy()) != _bits(want))[0]
    assert bad.size == 0, (bad[:8], v[bad[:8]], a[bad[:8]], j[bad[:8]])


def _tensors(n, dev):
    import torch
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    return z(n, 5), z(n, dtype=torch.int32), z(n, KMAX), z(n, KMAX), z(n, KMAX)


@pytest.mark.gpu
def test_gpu_runner_is_the_hand_driven_loop(gpu_ctx, restore_settings):
    import torch
    from rl_mpc_lanemerging_amd import _capi, actor, combined_bench, episodes
    S = _settings()
    n, seed, ctx = 48, 5, gpu_ctx
    dev = torch.device("cuda", torch.cuda.current_device())
    name = combined_bench.COMBINED_MEDIUM_1_ACTOR
    r = episodes.EpisodeRunner(n, seed=seed, controller="first_step", policy=actor.DDPGActor(name, n, ctx, S, dev), ctx=ctx, kmax=KMAX)
    per_tick = []
    for _ in range(TICKS):
        r.tick()
        per_tick.append((r.fs.cmd_speed.cpu().numpy().copy(), r.fs.takeover.cpu().numpy().copy()))
    got = r.result()
    # by hand, through the entries: view / actor_eval / speed_from_jerk / first_step (dense here, sparse in the runner) / sim_step
    params, cfg = _capi.Params.from_settings(S), episodes.sim_cfg(seed)
    fcfg = _capi.FirstStepCfg.from_settings(S, sparse_control=False)
    pol = actor.DDPGActor(name, n, ctx, S, dev)
    ego5, k, ox, ov, oa = _tensors(n, dev)
    speed, cmd = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    take, reason = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.sim_init(cfg, n)
    taken, running_ticks = np.zeros(n), np.zeros(n)
    for t in range(TICKS):
        running = ctx.sim_read(n)[0] == 0
        ctx.sim_view(cfg, n, KMAX, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr())
        jerk = pol(1, ego5[:, :4].contiguous().clone(), k, ox, ov, oa)
        ctx.speed_from_jerk_device(params, S.TICK_LENGTH, n, ego5.data_ptr(), jerk.data_ptr(), speed.data_ptr())
        ctx.first_step_device(params, fcfg, n, KMAX, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr(), speed.data_ptr(), cmd.data_ptr(),
                              take.data_ptr(), reason.data_ptr())
        ctx.sim_step(params, cfg, n, cmd.data_ptr())
        assert _same(cmd.cpu().numpy(), per_tick[t][0]), ("commanded speed", t)
        assert _same(take.cpu().numpy(), per_tick[t][1]), ("takeover", t)
        taken += take.cpu().numpy() * running
        running_ticks += running
    status, ticks, acc, ego4 = ctx.sim_read(n)
    ctx.check_error()
    want = episodes.stats_columns(status, ticks, acc, S.TICK_LENGTH)
    for key, val in want.items():
        assert _same(got[key], val), key
    assert _same(got["ego4"], ego4) and got["ticks"].max() == TICKS
    assert _same(got["percent_st"], taken / np.maximum(running_ticks, 1.0))


@pytest.mark.gpu
def test_gpu_combined_runner_is_unchanged(gpu_ctx, restore_settings):
    """``controller="combined"`` (the default of cross_matrix / evaluate_members) still is the tick it was: view -> combined.decide_batch_device with the
    takeover memory -> world step, driven by hand through entries this controller does not touch, column for column."""
    import torch
    from rl_mpc_lanemerging_amd import _capi, actor, combined, combined_bench, episodes
    S = _settings()
    n, seed, ctx = 48, 5, gpu_ctx
    dev = torch.device("cuda", torch.cuda.current_device())
    name = combined_bench.COMBINED_MEDIUM_1_ACTOR
    got = episodes.run_episodes(n, seed=seed, controller="combined", policy=actor.DDPGActor(name, n, ctx, S, dev), ctx=ctx, kmax=KMAX, max_ticks=TICKS)
    params, cfg = _capi.Params.from_settings(S), episodes.sim_cfg(seed)
    ccfg = _capi.CombinedCfg.from_settings(S, sparse_control=True)
    pol = actor.DDPGActor(name, n, ctx, S, dev)
    ego5, k, ox, ov, oa = _tensors(n, dev)
    last_rl = torch.ones(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    taken, controlled = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    ctx.sim_init(cfg, n)
    for _ in range(TICKS):
        ctx.sim_view(cfg, n, KMAX, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr())
        d = combined.decide_batch_device(ctx, params, ccfg, ego5, k, ox, ov, pol, last_rl, d_oa=oa)
        ctx.sim_status_device(n, status.data_ptr())
        running = (status == 0).to(torch.float64)
        taken += d["takeover"].to(torch.float64) * running
        controlled += running
        last_rl = (d["takeover"] == 0).to(torch.int32)
        ctx.sim_step(params, cfg, n, d["speed"].data_ptr())
    st, ticks, acc, ego4 = ctx.sim_read(n)
    ctx.check_error()
    want = episodes.stats_columns(st, ticks, acc, S.TICK_LENGTH)
    want["ego4"] = ego4
    want["percent_st"] = (taken / torch.clamp(controlled, min=1.0)).cpu().numpy()
    assert set(got) == set(want)
    for key, val in want.items():
        assert _same(got[key], val), key


@pytest.mark.gpu
def test_gpu_population_and_traffic_groups(gpu_ctx, restore_settings):
    """2 models x 2 traffic types x 12 environments in one runner: every cell is the lone runner of its actor on its traffic, bit for bit, and the
    recorder's ``percent st solver`` is takeovers / ticks of the per-tick outputs."""
    from rl_mpc_lanemerging_amd import actor, episodes, learner, report
    S = _settings()
    ctx, npc = gpu_ctx, 12
    models = ["low1", "fast1"]
    traffic = [dict(episodes.TRAFFIC_TYPES["low"], seed=41), dict(episodes.TRAFFIC_TYPES["fast"], seed=42)]
    cell_models, cell_traffic = [m for m in models for _ in traffic], traffic * 2
    n = 4 * npc
    rec = lambda: report.RecorderConfig(depth=8)
    r = episodes.EpisodeRunner(n, controller="first_step", policy=actor.ActorPopulation(cell_models, npc, ctx, S), ctx=ctx, kmax=KMAX, record=rec(),
                               traffic=cell_traffic)
    taken, running_ticks = np.zeros(n), np.zeros(n)
    for _ in range(GROUP_TICKS):
        running = ctx.sim_read(n)[0] == 0
        r.tick()
        taken += r.fs.takeover.cpu().numpy() * running
        running_ticks += running
    got = r.result()
    print("takeovers per cell over %d ticks:" % GROUP_TICKS, taken.reshape(4, npc).sum(axis=1), "running ticks:", running_ticks.reshape(4, npc).sum(axis=1))
    assert np.array_equal(got["member"], np.arange(n) // npc) and np.array_equal(got["traffic_group"], got["member"]) and "control_group" not in got
    want_percent = taken / np.maximum(running_ticks, 1.0)
    assert taken.sum() > 0 and running_ticks.max() == GROUP_TICKS
    assert _same(got["percent_st"], want_percent)
    assert _same(got["report"].percent_st(), want_percent)                      # the recorder's own totals, fed from d_takeover
    assert _same(got["report"].lists()[report.PERCENT_ST], want_percent)       # Report's "percent st solver" column exists for this controller
    prof = got["report"].profiles()
    assert prof["takeover_counts"].sum() == taken.sum() and prof["counts"].sum() == running_ticks.sum()
    # the same call through cross_matrix: controller is passed through, the default stays the combined controller
    cm = episodes.cross_matrix(models, traffic, npc, ctx=ctx, kmax=KMAX, max_ticks=10, controller="first_step")
    hand = episodes.run_episodes(n, controller="first_step", policy=actor.ActorPopulation(cell_models, npc, ctx, S), ctx=ctx, kmax=KMAX, max_ticks=10,
                                 traffic=cell_traffic)
    assert set(cm["stats"]) == set(hand)
    for key, val in hand.items():
        assert _same(cm["stats"][key], val), key
    # every cell against the lone runner of its actor and traffic cfg
    for c in range(4):
        sl = slice(c * npc, (c + 1) * npc)
        with _settings_of(cell_traffic[c]):
            lone = episodes.run_episodes(npc, seed=cell_traffic[c]["seed"], controller="first_step", policy=actor.DDPGActor(cell_models[c], npc, ctx, S), ctx=ctx,
                                         kmax=KMAX, max_ticks=GROUP_TICKS, record=rec())
        for key in [q for q in lone if q != "report"]:
            assert _same(got[key][sl], lone[key]), (c, key)
        a, b = got["report"]._rec, lone["report"]._rec
        for key in ("ring", "length", "status"):
            assert _same(a[key][sl], b[key]), (c, key)
        assert _same(np.ascontiguousarray(a["acc_env"][:, sl]), b["acc_env"]), (c, "acc_env")
    assert not _same(got["ego4"][:npc], got["ego4"][2 * npc:3 * npc])           # (same traffic draws, another actor: the cells do differ)
    # evaluate_members passes the controller through as well (a short episode limit keeps it to 20 ticks)
    ev = learner.evaluate_members(models, npc, kmax=KMAX, max_episode_length=4.0, ctx=ctx, traffic=traffic, controller="first_step")
    pop = actor.ActorPopulation(models, npc, ctx, S)
    hand = episodes.run_episodes(2 * npc, controller="first_step", policy=pop, ctx=ctx, kmax=KMAX, max_episode_length=4.0, traffic=traffic)
    for key in ("ego4", "ticks", "status", "percent_st"):
        assert _same(ev["stats"][key], hand[key]), key
