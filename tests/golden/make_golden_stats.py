#!/usr/bin/env python3
"""Golden vectors for the evaluation report (rl-mpc-lanemerging_amd/report.py, csrc/stmpc_rec_kernels.hpp): the reference's own
``stats.StatsAggregator`` (stats.py) and ``dqn.RLAgent.combined_stats_callback`` (dqn.py:101-115), unmodified, fed with synthetic
``episode_stats`` dicts of the shape ``control.run_episode`` returns (control.py:324-338).

Build-container only (needs the reference checkout, scipy, pandas, matplotlib).  The 40 episodes cover: merged, crashed and timed-out episodes; an
episode with empty ``closest_vehicle_history`` and ``disruption_history``; x values lying exactly on bin edges (-200.0, 0.0, 40.0 and the closed
right end 60.0) as well as between them and below the first edge; one episode of a single tick.  Recorded: the inputs (ragged histories as
concatenated arrays + lengths), ``get_stats()``, ``get_stat_averages(report_stds=True)`` (both without the two wall-clock columns, which are
not reproducible), ``counts`` / ``jerks`` / ``speeds`` and the two histograms ``plot_st_proportion`` takes (dqn.py:217-218).  Numbers only.
Re-run:  python tests/golden/make_golden_stats.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import import_reference      # noqa: E402

N_EPISODES = 40
CLOCK = ("clock_time_per_episode", "clock_time_per_step")
TICK = 0.2


def synthetic_episode(rng, i):
    """Episode i as control.run_episode would return it: Python floats / bools in lists."""
    kind = ("merged", "merged", "merged", "crashed", "timed_out")[i % 5]
    ticks = 1 if i == 7 else int(rng.integers(20, 160))
    v = np.clip(10.0 + np.cumsum(rng.normal(0.0, 0.4, ticks)), 0.5, 25.0)
    x0 = float(rng.uniform(-235.0, -205.0))                # some episodes start below the first edge (-220)
    xs = x0 + np.concatenate([[0.0], np.cumsum(v[:-1] * TICK)])
    end = {"merged": 51.4, "crashed": float(rng.uniform(-60.0, 20.0)), "timed_out": float(rng.uniform(-150.0, 45.0))}[kind]
    if ticks > 1:
        xs = x0 + (xs - x0) * ((end - x0) / (xs[-1] - x0))  # monotone, ends where that kind of episode ends
    if i == 7:
        kind = "crashed"
    # exact edge values: the tick nearest to an edge is moved onto it (the order of the x values is kept)
    for edge in ((-200.0, 0.0, 40.0) if i % 2 == 0 else (-200.0,)) + ((60.0,) if i == 4 else ()):
        if edge == 60.0:
            xs[-1] = 60.0
        elif ticks > 1 and xs[0] < edge < xs[-1]:
            xs[int(np.argmin(np.abs(xs - edge)))] = edge
    acc = np.concatenate([[0.0], np.diff(v) / TICK])
    jerk = np.concatenate([[0.0], np.diff(acc) / TICK])
    ys = np.where(xs < -50.9, 1.72 + (xs + 50.9) * -0.134, -1.5)
    past = xs > -50.0
    closest = rng.uniform(5.0, 100.0, int(past.sum()))
    disruption = np.where(rng.random(int(past.sum())) < 0.2, rng.uniform(0.0, 9.0, int(past.sum())), 0.0)
    if i == 13 or i == 7:                                   # never past the merge point: both histories empty (a crashed / timed-out episode)
        closest, disruption = closest[:0], disruption[:0]
        kind = "crashed" if i == 7 else "timed_out"
    if kind == "merged" and closest.size == 0:
        closest, disruption = np.array([50.0]), np.array([0.0])
    takeover = rng.random(ticks) < (0.3 if i % 6 == 0 else 0.03)
    return {"crashed": kind == "crashed", "merged": kind == "merged", "state_history": [None] * ticks, "control_history": [float(s) for s in v],
            "position_history": [(float(a), float(b)) for a, b in zip(xs, ys)], "speed_history": [float(s) for s in v],
            "acceleration_history": [float(a) for a in acc], "disruption_history": [float(d) for d in disruption],
            "jerk_history": [0] + [float(j) for j in jerk[1:]], "closest_vehicle_history": [float(c) for c in closest],
            "simulation_time_taken": ticks * TICK, "end_time": 1.0 + i, "start_time": 0.5}, [bool(t) for t in takeover]


def ragged(seqs, dtype=np.float64):
    return np.array([x for s in seqs for x in s], dtype=dtype), np.array([len(s) for s in seqs], dtype=np.int32)


def main():
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    S = import_reference()[0]
    import dqn                                              # noqa: E402  (the reference's)
    import stats                                            # noqa: E402  (the reference's, unmodified)
    assert S.TICK_LENGTH == TICK
    rng = np.random.default_rng(20261017)
    agent = types.SimpleNamespace(all_xs=[], takeover_xs=[], takeover_history=[])
    agg = stats.StatsAggregator()
    agg.add_custom_stat_callback(lambda ep: dqn.RLAgent.combined_stats_callback(agent, ep))
    episodes, takeovers = [], []
    for i in range(N_EPISODES):
        ep, take = synthetic_episode(rng, i)
        episodes.append(ep)
        takeovers.append(take)
        agent.takeover_history.extend(take)                 # what do_combined_control appends, one per tick (dqn.py:144-200)
        agg.add_episode_stats(ep)
    bins = np.arange(-220, 61, 20)                          # default_bins of plot_st_proportion (dqn.py:216)
    assert np.array_equal(bins, agg.bins)
    hist_all, _ = np.histogram(agent.all_xs, bins=bins)
    hist_st, _ = np.histogram(agent.takeover_xs, bins=bins)
    lists = {k: v for k, v in agg.get_stats().items() if k not in CLOCK}
    averages, stds = agg.get_stat_averages(report_stds=True)
    out = {"bins": bins.astype(np.float64), "tick_length": np.array(TICK), "counts": agg.counts, "jerks": agg.jerks, "speeds": agg.speeds,
           "hist_all": hist_all.astype(np.int64), "hist_st": hist_st.astype(np.int64),
           "crashed": np.array([ep["crashed"] for ep in episodes]), "merged": np.array([ep["merged"] for ep in episodes]),
           "simulation_time_taken": np.array([ep["simulation_time_taken"] for ep in episodes])}
    for key, src in (("xs", [[p[0] for p in ep["position_history"]] for ep in episodes]), ("ys", [[p[1] for p in ep["position_history"]] for ep in episodes]),
                     ("speed", [ep["speed_history"] for ep in episodes]), ("jerk", [ep["jerk_history"] for ep in episodes]),
                     ("closest", [ep["closest_vehicle_history"] for ep in episodes]), ("disruption", [ep["disruption_history"] for ep in episodes])):
        out["in_" + key], out["len_" + key] = ragged(src)
    out["in_takeover"], _ = ragged(takeovers, dtype=np.bool_)
    names = sorted(lists)
    out["stat_names"] = np.array(names)
    for j, name in enumerate(names):
        out["list_%d" % j] = np.asarray(lists[name], dtype=np.float64)
    out["averages"] = np.array([averages[name] for name in names])
    out["stds"] = np.array([stds[name] for name in names])
    path = os.path.join(HERE, "golden_stats.npz")
    np.savez_compressed(path, **out)
    status = ["merged" if ep["merged"] else "crashed" if ep["crashed"] else "timed_out" for ep in episodes]
    print("%d episodes (%s), %d ticks, %d on an edge, %d bytes" % (N_EPISODES, ", ".join("%d %s" % (status.count(s), s) for s in ("merged", "crashed", "timed_out")),
                                                                  out["in_xs"].size, int(np.isin(out["in_xs"], bins).sum()), os.path.getsize(path)))
    for name in names:
        print("  %-30s n %2d  mean %.6g  sem %.6g" % (name, len(lists[name]), averages[name], stds[name]))


if __name__ == "__main__":
    main()
