"""The episode flight recorder (stmpc_rec_*, csrc/stmpc_rec_kernels.hpp) and the evaluation report built on it (report.py).

CPU: the host twins ``report_host`` / ``bin_profiles_host`` and ``Report`` against the reference's unmodified ``stats.StatsAggregator`` and
``combined_stats_callback`` (tests/golden/golden_stats.npz, made by tests/golden/make_golden_stats.py): lists, counts, histograms, binned sums
and means bit for bit (same calls in the same order); standard errors within relative 1e-12 (same formula over at most 40 terms: the
summation-order rounding is bounded by about 40 x 2^-53 = 4.4e-15, 1e-12 is that with headroom and far below any error of the formula).
Header, library and binding agree on the new entries and constants; the ABI version is still 8.

GPU: the device recorder against a host-stepped twin (rings with wrap-around and partially filled, per-environment accumulators bit for bit,
reduced bins within the reordering bound n_terms x 2^-52), every ending frozen, replay, the combined controller's takeover share,
reproducibility, the off switch and the refusals.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from stmpc_testlib import capi as _capi

ST_TRAFFIC = dict(BASE_TRAFFIC_INTERVAL=2.4, OTHER_CAR_SPEED=7.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- CPU: the host twins against the reference's stats.py ------------------------------------------------------------------------------------
def _golden_episodes(g):
    """The golden's inputs as the ``episode_stats`` dicts control.run_episode returns (Python floats in lists)."""
    def split(key, lens=None):
        lens = g["len_" + key] if lens is None else lens
        return [[v.item() for v in part] for part in np.split(g["in_" + key], np.cumsum(lens)[:-1])]
    xs, ys, speed, jerk = split("xs"), split("ys"), split("speed"), split("jerk")
    closest, disruption, takeover = split("closest"), split("disruption"), split("takeover", g["len_xs"])
    return [{"position_history": list(zip(xs[i], ys[i])), "speed_history": speed[i], "jerk_history": jerk[i], "closest_vehicle_history": closest[i],
             "disruption_history": disruption[i], "takeover_history": takeover[i], "crashed": bool(g["crashed"][i]), "merged": bool(g["merged"][i]),
             "simulation_time_taken": g["simulation_time_taken"][i].item()} for i in range(len(xs))]


def _golden_lists(g):
    return {str(name): g["list_%d" % j] for j, name in enumerate(g["stat_names"])}


def test_golden_covers_the_cases_the_report_must_handle():
    g = load_golden("golden_stats.npz")
    eps = _golden_episodes(g)
    status = ["merged" if e["merged"] else "crashed" if e["crashed"] else "timed_out" for e in eps]
    assert len(eps) == 40 and all(status.count(s) >= 5 for s in ("merged", "crashed", "timed_out"))
    assert any(len(e["closest_vehicle_history"]) == 0 and len(e["disruption_history"]) == 0 for e in eps)
    assert any(len(e["position_history"]) == 1 for e in eps)
    xs = g["in_xs"]
    for edge in (-200.0, 0.0, 40.0):
        assert (xs == edge).any(), edge
    assert (~np.isin(xs, g["bins"])).sum() > 1000 and (xs < g["bins"][0]).any()


def test_report_host_equals_the_reference_bit_for_bit():
    _capi()
    from rl_mpc_lanemerging_amd import report
    g = load_golden("golden_stats.npz")
    h = report.report_host(_golden_episodes(g), g["bins"], float(g["tick_length"]))
    want = _golden_lists(g)
    assert set(h["lists"]) == set(want)
    for name, values in want.items():
        assert _same_bits(h["lists"][name], values), name
    assert np.array_equal(h["counts"], g["counts"]) and np.array_equal(h["counts"], g["hist_all"])
    assert np.array_equal(h["takeover_counts"], g["hist_st"])
    assert _same_bits(h["jerks"], g["jerks"]) and _same_bits(h["speeds"], g["speeds"])
    # the means are np.mean on the same lists
    for j, name in enumerate(g["stat_names"]):
        assert _same_bits(np.mean(h["lists"][str(name)]), g["averages"][j]), name


def test_report_equals_the_reference_lists_means_and_standard_errors():
    _capi()
    from rl_mpc_lanemerging_amd import report
    g = load_golden("golden_stats.npz")
    rep = report.Report.from_histories(_golden_episodes(g), g["bins"], float(g["tick_length"]))
    want = _golden_lists(g)
    lists, avg, std = rep.lists(), rep.averages(), rep.stds()
    assert set(lists) == set(want)
    for j, name in enumerate(str(s) for s in g["stat_names"]):
        assert _same_bits(lists[name], want[name]), name
        assert _same_bits(avg[name], g["averages"][j]), name
        print("%-30s sem %.17g reference %.17g" % (name, std[name], g["stds"][j]))
        assert abs(std[name] - g["stds"][j]) <= 1e-12 * abs(g["stds"][j]), name
    prof = rep.profiles()
    assert np.array_equal(prof["counts"], g["counts"]) and _same_bits(prof["jerks"], g["jerks"]) and _same_bits(prof["speeds"], g["speeds"])
    with np.errstate(divide="ignore", invalid="ignore"):
        assert _same_bits(prof["avg_jerks"], g["jerks"] / g["counts"]) and _same_bits(prof["avg_speeds"], g["speeds"] / g["counts"])
        assert _same_bits(prof["st_proportion"], g["hist_st"] / g["hist_all"])
    row = rep.row()
    for j, name in enumerate(str(s) for s in g["stat_names"]):
        assert row[name] == avg[name] and (row[name + "_std"] == std[name] or np.isnan(std[name]))
    assert not any(k.startswith("clock_time") or k == "TIME" for k in row)
    merged = rep.merged_columns()
    assert _same_bits(merged["mean_abs_jerk_merged"][g["merged"]], want["mean_abs_jerk_merged"]) and np.isnan(merged["closest_distance_merged"][~g["merged"]]).all()


def test_the_two_bin_rules_differ_exactly_on_the_edges():
    """np.histogram: edge[b] <= x < edge[b + 1], last bin closed, outside dropped; the loop of stats.py:48-52: first b with x <= edge[b + 1],
    below the first edge -> bin 0.  Worked by hand for edges (0, 10, 20)."""
    _capi()
    from rl_mpc_lanemerging_amd import report
    xs = [-5.0, 0.0, 3.0, 10.0, 10.0, 12.0, 20.0]
    out = report.bin_profiles_host(xs, [1.0] * 7, [2.0] * 7, [False, True, False, True, False, False, True], [0.0, 10.0, 20.0])
    assert out["counts"].tolist() == [2.0, 4.0]                 # -5 dropped; 10 opens the second bin; 20 closes it
    assert out["takeover_counts"].tolist() == [1.0, 2.0]
    assert out["jerks"].tolist() == [5.0, 2.0]                  # -5 counted in bin 0; both 10s still in the first bin
    assert out["speeds"].tolist() == [10.0, 4.0]


def test_header_library_and_binding_agree_on_the_recorder():
    capi = _capi()
    lib = capi.load()
    header = open(os.path.join(REPO, "include", "stmpc.h")).read()
    declared = {n for n in re.findall(r"\b(stmpc_[a-z_0-9]+)\s*\(", header) if n.startswith("stmpc_rec_")}
    assert declared == {"stmpc_rec_create", "stmpc_rec_destroy", "stmpc_rec_reset", "stmpc_rec_tick_device", "stmpc_rec_reduce_device", "stmpc_rec_read"}
    assert declared == {n for n in capi.EXPORTS if n.startswith("stmpc_rec_")}
    for name in declared:
        assert getattr(lib, name) is not None and getattr(lib, name).argtypes is not None, name
    flat = " ".join(header.split())
    for name, val in (("STMPC_REC_HDR", capi.REC_HDR), ("STMPC_REC_NQ", capi.REC_NQ), ("STMPC_REC_MAX_DEPTH", capi.REC_MAX_DEPTH),
                      ("STMPC_REC_MAX_EDGES", capi.REC_MAX_EDGES), ("STMPC_ABI_VERSION", capi.ABI_VERSION)):
        assert "#define %s %d" % (name, val) in flat, name
    assert len(capi.REC_COLUMNS) == capi.REC_HDR and len(capi.REC_QUANTITIES) == capi.REC_NQ
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8
    # every refusal of stmpc_rec_create happens before the device is touched
    h = ctypes.c_void_p()
    edges = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    assert lib.stmpc_rec_create(None, 4, 8, 8, 0.2, edges, 3, ctypes.byref(h)) == capi.STMPC_EINVAL


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------
def _apply_st_settings():
    import rl_mpc_lanemerging_amd as pkg
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(ST_TRAFFIC)


_RUNS = {}


def _stepped_st_run(gpu_ctx, kmax, max_episode_length, n_ticks, n=70, depth=8, seed=5):
    """An ``EpisodeRunner`` with a recorder, ticked by hand; after every tick the view the tick consumed and its commands are copied to the host
    and appended to the histories of the environments that were running before it.  Computed once per shape and shared (read-only)."""
    key = (kmax, max_episode_length, n_ticks)
    if key in _RUNS:
        return _RUNS[key]
    from rl_mpc_lanemerging_amd import episodes, report
    _apply_st_settings()
    r = episodes.EpisodeRunner(n, seed=seed, controller="st", ctx=gpu_ctx, kmax=kmax, max_episode_length=max_episode_length, record=report.RecorderConfig(depth=depth))
    hist = [[] for _ in range(n)]
    for _ in range(n_ticks):
        before = r.status()
        r.tick()
        ego5, k, ox, ov, cmd = (t.cpu().numpy() for t in (r.d_ego5, r.d_k, r.d_ox, r.d_ov, r.d_speed))
        for e in np.nonzero(before == 0)[0]:
            prev = hist[e][-1]["ego5"][3] if hist[e] else None
            jerk = 0.0 if prev is None else (ego5[e, 3] - prev) / r.tick_length
            hist[e].append({"tick": len(hist[e]), "ego5": ego5[e].copy(), "k": int(k[e]), "ox": ox[e].copy(), "ov": ov[e].copy(), "cmd": cmd[e], "jerk": jerk})
    _RUNS[key] = (r, r.result(), hist)
    return _RUNS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kmax,max_episode_length,n_ticks", [(32, 100.0, 60), (16, 100.0, 60), (32, 1.0, 8)])
def test_ring_and_accumulators_equal_a_host_stepped_twin(kmax, max_episode_length, n_ticks, gpu_ctx, restore_settings):
    capi = _capi()
    from rl_mpc_lanemerging_amd import report
    n, depth = 70, 8
    r, res, hist = _stepped_st_run(gpu_ctx, kmax, max_episode_length, n_ticks)
    rec = res["report"]._rec
    bins = rec["bins"]
    nb = len(bins) - 1
    if max_episode_length == 1.0:
        assert r.cfg.max_ticks == 5 and (res["status"] == 3).all() and all(len(h) == 5 for h in hist)      # the partially filled ring
    else:
        assert min(len(h) for h in hist) > depth                                                           # wrap-around
    twin = np.zeros((capi.REC_NQ * nb + 2, n))
    for e in range(n):
        L = min(len(hist[e]), depth)
        assert rec["length"][e] == L, e
        ring = rec["ring"][e]
        for i, want in enumerate(hist[e][-L:]):
            row = ring[i]
            head = np.concatenate([[want["tick"]], want["ego5"], [want["k"], want["cmd"], 0.0, want["jerk"]]])
            assert _same_bits(row[:capi.REC_HDR], head), (e, i, row[:capi.REC_HDR], head)
            veh = row[capi.REC_HDR:]
            assert _same_bits(veh[:kmax], want["ox"]) and _same_bits(veh[kmax:2 * kmax], want["ov"]) and not veh[2 * kmax:].any(), (e, i)
        assert not ring[L:].any()
        p = report.bin_profiles_host([h["ego5"][0] for h in hist[e]], [h["jerk"] for h in hist[e]], [h["ego5"][2] for h in hist[e]], None, bins)
        twin[:, e] = np.concatenate([p["counts"], p["takeover_counts"], p["jerks"], p["speeds"], [0.0, len(hist[e])]])
    assert _same_bits(rec["acc_env"], twin)          # counts exact; sums bit for bit: within an environment the device adds in tick order, as the twin does
    assert twin[:nb].sum() > 0 and twin[2 * nb:3 * nb].sum() > 0
    red, want = rec["acc_reduced"], twin.sum(axis=1)
    count_rows = list(range(0, 2 * nb)) + [capi.REC_NQ * nb, capi.REC_NQ * nb + 1]
    assert np.array_equal(red[count_rows], want[count_rows])
    err = np.abs(red - want)
    print("reduced sums: largest relative difference to the twin's sum %.3g (bound %.3g)" % ((err / np.maximum(want, 1e-300)).max(), n * 2.0 ** -52))
    assert (err <= n * 2.0 ** -52 * want).all()
    prof = res["report"].profiles()
    assert np.array_equal(prof["counts"], red[:nb]) and _same_bits(prof["jerks"], red[2 * nb:3 * nb])


@pytest.mark.gpu
def test_replay_reproduces_the_recorded_commands(gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import report
    _, res, hist = _stepped_st_run(gpu_ctx, 32, 100.0, 60)
    _apply_st_settings()
    traces = res["report"].traces()
    assert len(traces) == 70
    for e in (0, 33, 69):
        tr = traces[e]
        assert tr.env == e and len(tr) == 8 and [s["tick"] for s in tr] == [h["tick"] for h in hist[e][-8:]]
        out = report.replay(tr, gpu_ctx)
        assert _same_bits(out["speed"], [s["cmd"] for s in tr]), (e, out["speed"], [s["cmd"] for s in tr])
        assert out["path_idx"].shape[0] == 8 and out["cost"].shape == (8,)


@pytest.mark.gpu
def test_every_ending_is_frozen_at_its_last_running_tick(gpu_ctx, restore_settings):
    """The C-level sequence sim_view -> command -> rec_tick -> sim_step.  Environments 0-34 are commanded MAX_SPEED every tick (they reach the
    junction at full speed and hit the highway traffic: status 2 after 33-45 ticks), 35-69 take the controller's speeds; the world's time limit
    (26 s = 130 ticks) lies inside the spread of the controller's merge times (118-147 ticks with this seed under a 100 s limit), so the faster
    of those arrive (status 1) and the slower run out of time (status 3).  (The first limit tried, 24 s, gave 4 / 35 / 31; 26 s splits the
    controller's half more evenly.  The assertion below is what makes the test non-vacuous.)"""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, episodes, report
    _apply_st_settings()
    n, kmax, depth = 70, 32, 8
    S = pkg.Settings
    ctx, params, cfg = gpu_ctx, _capi.Params.from_settings(S), episodes.sim_cfg(seed=11, max_episode_length=26.0)
    dev = torch.device("cuda", torch.cuda.current_device())
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    H = _capi.num_t(params)
    ego5, k, ox, ov = z(n, 5), z(n, dtype=torch.int32), z(n, kmax), z(n, kmax)
    path, bt, cost, speed, status = z(n, H, dtype=torch.int32), z(n, dtype=torch.int32), z(n), z(n), z(n, dtype=torch.int32)
    fast = torch.arange(n, device=dev) < n // 2
    ctx.sim_init(cfg, n)
    rec = report.Recorder(ctx, n, kmax, report.RecorderConfig(depth=depth), S.TICK_LENGTH)

    def one_tick():
        ctx.sim_view(cfg, n, kmax, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr())
        ctx.st_control_batch_device(params, S.TICK_LENGTH, n, kmax, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), path.data_ptr(), bt.data_ptr(),
                                    cost.data_ptr(), speed.data_ptr())
        cmd = torch.where(fast, torch.full_like(speed, float(S.MAX_SPEED)), speed)
        rec.tick(n, kmax, ego5, k, ox, ov, None, cmd)
        ctx.sim_step(params, cfg, n, cmd.data_ptr())
        return cmd

    views, cmds, last_live = [], [], np.full(n, -1)
    for tick in range(cfg.max_ticks + 1):
        ctx.sim_status_device(n, status.data_ptr())
        before = status.cpu().numpy()
        if (before != 0).all():
            break
        cmd = one_tick()
        views.append(ego5.cpu().numpy())
        cmds.append(cmd.cpu().numpy())
        last_live[before == 0] = tick
    a = rec.read()
    ctx.check_error()
    st = a["status"]
    print("endings:", {s: int((st == s).sum()) for s in (0, 1, 2, 3)})
    assert (st == 1).any() and (st == 2).any() and (st == 3).any() and not (st == 0).any()       # not vacuous: every ending occurs
    for e in range(n):
        L = min(last_live[e] + 1, depth)
        assert a["length"][e] == L
        last = a["ring"][e, L - 1]
        assert last[0] == last_live[e] and _same_bits(last[1:6], views[last_live[e]][e]) and _same_bits(last[7], cmds[last_live[e]][e]), (e, st[e])
        assert a["ring"][e, :L, 0].tolist() == list(range(last_live[e] - L + 1, last_live[e] + 1))
    for _ in range(3):                                   # everything has ended: further ticks must change nothing
        one_tick()
    b = rec.read()
    for key in ("ring", "length", "acc_env", "acc_reduced", "status"):
        assert np.array_equal(a[key], b[key]), key
    status_h, ticks, acc, _ = ctx.sim_read(n)
    rep = report.Report.from_result(episodes.stats_columns(status_h, ticks, acc, S.TICK_LENGTH), b)
    assert sorted(t.env for t in rep.crashed_traces()) == np.nonzero(st == 2)[0].tolist()
    assert sorted(t.env for t in rep.traces(status=(1, 3))) == np.nonzero((st == 1) | (st == 3))[0].tolist()
    assert np.array_equal(ticks, last_live + 1) and np.array_equal(a["acc_env"][-1], ticks)
    rec.close()


@pytest.mark.gpu
def test_combined_controller_takeover_share_comes_from_the_recorder(gpu_ctx, restore_settings):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, combined_bench, episodes, report
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1_TRAFFIC)
    n, kmax, depth = 70, 16, 8
    bins = np.arange(-180.0, 1.0, 20.0)                  # the start of the ramp and the highway past x = 0 lie outside the edges
    policy = actor.DDPGActor("runs/ddpg_medium1_extended", n, gpu_ctx, pkg.Settings, torch.device("cuda", torch.cuda.current_device()))
    r = episodes.EpisodeRunner(n, seed=21, controller="combined", policy=policy, ctx=gpu_ctx, kmax=kmax, record=report.RecorderConfig(depth=depth, bins=bins))
    inside_takeovers = np.zeros(len(bins) - 1)
    total = outside = 0
    for _ in range(120):
        before = r.status()
        if (before != 0).all():
            break
        r.tick()
        now = r.recorder.read()
        for e in np.nonzero(before == 0)[0]:
            newest = now["ring"][e, now["length"][e] - 1]
            x, took = newest[1], newest[8] != 0
            total += took
            if took and bins[0] <= x <= bins[-1]:
                inside_takeovers[min(np.searchsorted(bins, x, side="right") - 1, len(bins) - 2)] += 1
            outside += took and not (bins[0] <= x <= bins[-1])
    res = r.result()
    rep = res["report"]
    assert _same_bits(rep.percent_st(), res["percent_st"])
    acc = rep._rec["acc_env"]
    assert acc[-2].sum() == total and total > 0
    prof = rep.profiles()
    print("takeovers: %d, of them outside the edges %d; per bin %s" % (total, outside, prof["takeover_counts"].tolist()))
    assert np.array_equal(prof["takeover_counts"], inside_takeovers) and prof["takeover_counts"].sum() == total - outside


@pytest.mark.gpu
def test_recorded_runs_are_reproducible_and_the_recorder_changes_nothing(gpu_ctx, restore_settings):
    from rl_mpc_lanemerging_amd import episodes, report
    _apply_st_settings()
    run = lambda record: episodes.run_episodes(70, seed=9, controller="st", ctx=gpu_ctx, max_ticks=40, record=record)
    a, b, plain = run(report.RecorderConfig(depth=8)), run(report.RecorderConfig(depth=8)), run(None)
    assert _same_bits(a["report"]._rec["acc_reduced"], b["report"]._rec["acc_reduced"]) and a["report"]._rec["acc_reduced"][-1] == a["ticks"].sum() > 0
    assert _same_bits(a["report"]._rec["ring"], b["report"]._rec["ring"])
    assert "report" not in plain and set(a) - {"report"} == set(plain)
    for key, value in plain.items():
        assert np.array_equal(a[key], value, equal_nan=True), key


@pytest.mark.gpu
def test_recorder_refusals(gpu_ctx, restore_settings):
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, episodes, report
    _apply_st_settings()
    n, kmax = 70, 32
    ctx, cfg, tick_length = gpu_ctx, episodes.sim_cfg(seed=3), pkg.Settings.TICK_LENGTH
    ctx.sim_init(cfg, n)

    def refused(fn):
        with pytest.raises(_capi.StmpcError) as ei:
            fn()
        assert ei.value.code == _capi.STMPC_EINVAL, ei.value

    for depth in (0, 65):
        refused(lambda: ctx.rec_create(n, kmax, depth, tick_length, report.DEFAULT_BINS))
    refused(lambda: ctx.rec_create(n, kmax, 8, tick_length, np.arange(33.0)))            # more than 32 edges
    refused(lambda: ctx.rec_create(n, kmax, 8, tick_length, [0.0]))
    refused(lambda: ctx.rec_create(n, kmax, 8, tick_length, [0.0, 2.0, 1.0]))
    refused(lambda: ctx.rec_create(n, 33, 8, tick_length, report.DEFAULT_BINS))
    refused(lambda: ctx.rec_create(0, kmax, 8, tick_length, report.DEFAULT_BINS))
    dev = torch.device("cuda", torch.cuda.current_device())
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    ego5, k, ox, ov, cmd = z(n + 1, 5), z(n + 1, dtype=torch.int32), z(n + 1, kmax), z(n + 1, kmax), z(n + 1)
    rec = report.Recorder(ctx, n, kmax, report.RecorderConfig(depth=8), tick_length)
    rec.tick(n, kmax, ego5, k, ox, ov, None, cmd)                                         # (the accepted call)
    refused(lambda: rec.tick(n + 1, kmax, ego5, k, ox, ov, None, cmd))
    refused(lambda: rec.tick(n, 16, ego5, k, ox, ov, None, cmd))
    other = report.Recorder(ctx, 64, kmax, report.RecorderConfig(depth=8), tick_length)   # not this world's N: never bound
    refused(lambda: other.tick(64, kmax, ego5, k, ox, ov, None, cmd))
    refused(other.reset)
    ctx.sim_init(cfg, n)                                                                  # the world starts over: the recorder's episode is gone
    refused(lambda: rec.tick(n, kmax, ego5, k, ox, ov, None, cmd))
    refused(rec.read)
    refused(rec.reduce)
    rec.reset()
    rec.tick(n, kmax, ego5, k, ox, ov, None, cmd)
    assert rec.read()["length"].tolist() == [1] * n
    ctx.check_error()
    rec.close()
    other.close()
