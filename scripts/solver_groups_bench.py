#!/usr/bin/env python3
"""Solver groups next to lone calls: one grouped st_control call of the 288 cells of main.do_grid_search_st x n states against the same 288 slices
controlled by lone calls one after another (the parent's entry, same process, same context), at a few n.  The outputs are compared bit for bit
before a row is recorded.  The lone loop is 288 calls through the Python binding per repetition, so the ratio includes their host overhead: that is
what a sweep without groups costs a caller of this package.  No target ratio: what is measured is written to profiles/solver/groups_bench.json.
Usage: scripts/solver_groups_bench.py [--n 1,4,16] [--reps 5] [--out profiles/solver/groups_bench.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,4,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "solver", "groups_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, st, synth
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    S = pkg.Settings
    cells = st.grid_search_cells()
    table = st.param_cfgs(cells)
    G, H, K = len(cells), _capi.num_t(table[0]), 8
    ctx = _capi.Context(0)
    dev = torch.device("cuda", 0)
    rows = []
    for n in [int(x) for x in args.n.split(",")]:
        N = G * n
        ego, kc, ox, ov = synth.generate_states(n, k=6, kmax=K, seed=11)
        tile = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate([a] * G))).to(dev)      # every cell sees the same n states
        d_ego, d_k, d_ox, d_ov = tile(ego), tile(kc), tile(ox), tile(ov)
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
        out = {name: (z(N, H, dtype=torch.int32), z(N, dtype=torch.int32), z(N), z(N), z(N, _capi.QP_NMAX), z(N, dtype=torch.int32)) for name in ("grouped", "lone")}

        def grouped():
            p, b, c, s, f, fl = out["grouped"]
            ctx.st_control_groups_device(table, n, S.TICK_LENGTH, N, K, d_ego.data_ptr(), d_k.data_ptr(), d_ox.data_ptr(), d_ov.data_ptr(), p.data_ptr(), b.data_ptr(),
                                         c.data_ptr(), s.data_ptr(), f.data_ptr(), fl.data_ptr())

        def lone():
            p, b, c, s, f, fl = out["lone"]
            for g in range(G):
                r = slice(g * n, (g + 1) * n)
                ctx.st_control_batch_device(table[g], S.TICK_LENGTH, n, K, d_ego[r].data_ptr(), d_k[r].data_ptr(), d_ox[r].data_ptr(), d_ov[r].data_ptr(), p[r].data_ptr(),
                                            b[r].data_ptr(), c[r].data_ptr(), s[r].data_ptr(), f[r].data_ptr(), fl[r].data_ptr())

        times = {}
        for name, fn in (("grouped", grouped), ("lone", lone)):
            fn()
            torch.cuda.synchronize()
            ctx.check_error()
            best = float("inf")
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            times[name] = best
        for a, b in zip(out["grouped"], out["lone"]):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "grouped and lone outputs differ"
        rows.append({"n_per_cell": n, "cells": G, "grouped_ms": times["grouped"] * 1e3, "lone_loop_ms": times["lone"] * 1e3,
                     "lone_over_grouped": times["lone"] / times["grouped"], "outputs_equal": True})
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump({"backend": _capi.backend_info(), "timing": "best of %d, wall clock around a synchronised call" % args.reps, "rows": rows}, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
