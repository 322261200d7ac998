#!/usr/bin/env python3
"""Cost of the episode flight recorder: ms per ``EpisodeRunner.tick()`` with ``record=None`` and with ``report.RecorderConfig(depth=32)``, for
both controllers, at several N.  The two runners (a context each, same seed, so the same episodes) are brought to mid-episode, then timed in
alternating windows of WINDOW ticks in one process, warm; the figure is the median over the rounds.  Writes profiles/report/report_bench.json and
prints it as one JSON line.
   usage: python scripts/report_bench.py [--n 4096 65536] [--controllers st combined] [--rounds 3] [--pre 60] [--out PATH]
--summarize-trace DIR turns the kernel-stats CSV of `rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python scripts/report_bench.py --n 4096
--controllers st --rounds 1 --out ''` into the table of profiles/report/kernel_stats.txt (printed)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
WINDOW = 20


def summarize_trace(directory):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_stats.csv under %s" % directory)
    rows = list(csv.DictReader(open(paths[0])))
    print("%-64s %8s %12s %12s" % ("kernel", "calls", "avg_us", "total_us"))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        print("%-64s %8d %12.2f %12.1f" % (r["Name"][:64], int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e3))


def window(runner, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(WINDOW):
        runner.tick()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / WINDOW


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--controllers", nargs="+", default=["st", "combined"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pre", type=int, default=60, help="untimed ticks before the first window (the egos are then mid-ramp, as in bench.py --workload episodes)")
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--seed", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "report", "report_bench.json"))
    ap.add_argument("--summarize-trace", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        return summarize_trace(a.summarize_trace)
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, actor, combined_bench, episodes, episodes_bench, report
    if pkg.build.needs_build():
        pkg.build.build()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"metric": "ms per EpisodeRunner.tick(), record=None against RecorderConfig(depth=%d); medians of %d rounds of %d ticks, interleaved" % (a.depth, a.rounds, WINDOW),
           "backend": _capi.backend_info(), "runs": []}
    for controller in a.controllers:
        # the traffic and controller settings of bench.py --workload episodes (episodes_bench.py)
        pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
        pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
        pkg.apply_overrides(episodes_bench.TRAIN_MODERATE_1_ENV)
        for n in a.n:
            kmax = 16 if controller == "combined" else 32
            runners = []
            for record in (None, report.RecorderConfig(depth=a.depth)):
                ctx = _capi.Context(-1)
                policy = actor.DDPGActor("runs/ddpg_moderate1_extended", n, ctx, pkg.Settings, dev) if controller == "combined" else None
                runners.append(episodes.EpisodeRunner(n, seed=a.seed, controller=controller, policy=policy, ctx=ctx, kmax=kmax, record=record))
            for r in runners:
                for _ in range(a.pre):
                    r.tick()
            times = ([], [])
            for _ in range(a.rounds):
                for i, r in enumerate(runners):
                    times[i].append(window(r, torch))
            res = [r.result() for r in runners]
            same = all((res[0][k] == res[1][k]).all() or k == "ego4" for k in ("ticks", "status"))
            t_off, t_on = statistics.median(times[0]), statistics.median(times[1])
            ring_mb = n * (_capi.REC_HDR + 3 * kmax) * 8 / 1e6
            out["runs"].append({"controller": controller, "n": n, "kmax": kmax, "depth": a.depth, "tick_ms_record_none": 1e3 * t_off, "tick_ms_recorded": 1e3 * t_on,
                                "overhead_ms": 1e3 * (t_on - t_off), "overhead_percent": 100.0 * (t_on / t_off - 1.0), "rounds_ms_record_none": [1e3 * t for t in times[0]],
                                "rounds_ms_recorded": [1e3 * t for t in times[1]], "record_mb_per_tick": ring_mb, "same_episodes_in_both_runners": bool(same),
                                "still_running_at_end": float((res[0]["status"] == 0).mean()), "ticks": int(runners[0].ticks_done)})
            for r in runners:
                if r.recorder is not None:
                    r.recorder.close()
            del runners, res, r, policy, ctx
            torch.cuda.empty_cache()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
