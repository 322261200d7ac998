#!/usr/bin/env python3
"""Host time of one ``env.step()`` call of the vector envs (vec_env.MergeVecEnv plain, behind the first-step shield and with a traffic mix;
vec_env.GroupedShieldVecEnv on traffic groups and on a mix): what the Python layer and the C entry cost the calling thread, which a GPU-bound step
time hides.  Per env, microseconds per call:
  queued_*   -- ``--window`` calls back to back from an idle queue, timed before any synchronisation (the enqueue with launches outstanding);
  idle_*     -- one call from an idle queue (a synchronisation before each): no launch waits for queue space;
  c_entry_*  -- of the idle call, the time inside the library's entries (the context's library handle is wrapped to time them);
  python_*   -- the idle call minus that: the Python layer alone.
Median and minimum over the windows / calls.  Prints one JSON line.   usage: python scripts/env_host_probe.py [--n 4100] [--windows 40] [--window 10] [--envs shield ...]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TYPES = ["low", "default", "fast", "low", "default"]


class TimedLib:
    """The loaded library with every entry's wall time added up in ``spent`` (seconds)."""

    def __init__(self, lib):
        self._lib, self._wrapped, self.spent = lib, {}, 0.0

    def __getattr__(self, name):
        fn = self._wrapped.get(name)
        if fn is None:
            raw = getattr(self._lib, name)

            def fn(*args):
                t0 = time.perf_counter()
                rc = raw(*args)
                self.spent += time.perf_counter() - t0
                return rc
            self._wrapped[name] = fn
        return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4100)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--envs", nargs="+", default=None, help="a subset of: plain shield mix shield_groups shield_mix")
    a = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, combined_bench, vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    n = -(-a.n // len(TYPES)) * len(TYPES)
    kw = dict(seed=1, env_id="sumo-jerk-continuous-v0")
    make = {"plain": lambda c: vec_env.MergeVecEnv(n, ctx=c, **kw),
            "shield": lambda c: vec_env.MergeVecEnv(n, ctx=c, shield="first_step", **kw),
            "mix": lambda c: vec_env.MergeVecEnv(n, ctx=c, traffic_mix=TYPES[:3], **kw),
            "shield_groups": lambda c: vec_env.GroupedShieldVecEnv(n, ctx=c, traffic=TYPES, **kw),
            "shield_mix": lambda c: vec_env.GroupedShieldVecEnv(n, ctx=c, traffic_mix=TYPES[:3], **kw)}
    med_min = lambda v: {"median": float(np.median(v)) * 1e6, "min": float(min(v)) * 1e6}
    out = {"n": n, "windows": a.windows, "window": a.window, "backend": _capi.backend_info(), "envs": {}}
    for name, mk in make.items():
        if a.envs is not None and name not in a.envs:
            continue
        ctx = _capi.Context(-1)
        lib = ctx._lib = TimedLib(ctx._lib)
        env = mk(ctx)
        env.reset()
        act = torch.zeros(n, dtype=torch.float64, device="cuda")
        for _ in range(20):
            env.step(act)
        queued, idle, c_entry = [], [], []
        for _ in range(a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.window):
                env.step(act)
            queued.append((time.perf_counter() - t0) / a.window)
        for _ in range(a.windows * a.window):
            torch.cuda.synchronize()
            lib.spent = 0.0
            t0 = time.perf_counter()
            env.step(act)
            idle.append(time.perf_counter() - t0)
            c_entry.append(lib.spent)
        torch.cuda.synchronize()
        env.check_error()
        python = [t - c for t, c in zip(idle, c_entry)]
        out["envs"][name] = {"queued_us": med_min(queued), "idle_us": med_min(idle), "c_entry_us": med_min(c_entry), "python_us": med_min(python)}
        ctx._lib = lib._lib
        del env
        ctx.close()
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
