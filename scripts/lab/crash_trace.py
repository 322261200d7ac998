"""Run-up of environments of the batched episodes to their end, from the on-device flight recorder (analysis tool): the whole batch runs without a
per-tick synchronisation, the environments are chosen afterwards.
usage: crash_trace.py <interval> <seed> <n> [env ...]      (no env: every crashed environment; the table is the last 25 recorded ticks of each)"""
import sys; sys.path.insert(0, '.')
import numpy as np
import rl_mpc_lanemerging_amd as pkg
from rl_mpc_lanemerging_amd import episodes, report, _capi
interval, seed, n = float(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
envs = [int(a) for a in sys.argv[4:]]
pkg.apply_overrides(pkg.REFERENCE_DEFAULT); pkg.apply_overrides(dict(BASE_TRAFFIC_INTERVAL=interval, OTHER_CAR_SPEED=7.0))
res = episodes.run_episodes(n, seed=seed, controller="st", kmax=32, record=report.RecorderConfig(depth=25))
rep = res["report"]
traces = [t for t in rep.traces() if t.env in envs] if envs else rep.crashed_traces()
print("status counts", {s: int((res["status"] == s).sum()) for s in (0, 1, 2, 3)}, "| traces of", [t.env for t in traces])
for tr in traces:
    print("env", tr.env, "status", tr.status, "at tick", int(res["ticks"][tr.env]) - 1)
    again = report.replay(tr)          # best_t and the re-sampled path's length are not recorded: solved again from the recorded states
    for s, bt, fl in zip(tr, again["best_t"], again["fine_len"]):
        e5 = s["ego5"]
        near = sorted(zip(s["other_x"] - e5[0], s["other_v"]), key=lambda q: abs(q[0]))[:4]
        print("t %3d ego x %.2f y %.2f v %.2f a %.2f s %.2f | cmd %.2f best_t %d fine_len %d | nearest dx,v: %s" % (s["tick"], e5[0], e5[1], e5[2], e5[3], e5[4], s["cmd"], bt, fl, " ".join("(%.1f,%.1f)" % q for q in sorted(near))))
