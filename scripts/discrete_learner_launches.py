#!/usr/bin/env python3
"""The launch sequence of the discrete learners, for a kernel trace: a lone learner.DQNLearner, a lone learner.C51Learner, a learner.DQNPopulation of
two and a learner.C51Population of two, each at n_obs 4, h1 16, 3 actions, batch 8, capacity 64 (5 atoms), eight rows per member and push.  Each
does one act with eps > 0, one push, three updates, one grads, one targets and one stats (a population: its member 0's grads and targets), first
with uniform minibatches and then, made anew, with prioritised replay.  The host code decides which kernels are launched, in which order and with
which grid, workgroup and LDS size, so two builds whose host code does the same show the same list.
   usage: rocprofv3 --kernel-trace -f csv -d DIR -o t -- python scripts/discrete_learner_launches.py
          python scripts/discrete_learner_launches.py --launches <DIR/.../t_kernel_trace.csv>
                  (one line per launch in start order: the kernel's name, its grid, its workgroup size and its LDS bytes)"""
import csv
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N_OBS, H1, A, BATCH, CAPACITY, ATOMS, ROWS, P, EPS = 4, 16, 3, 8, 64, 5, 8, 2, 0.5


def launches(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id") or 0)))

    def size(r, what):
        if what + "_X" in r:
            return "x".join(r[what + "_" + axis] for axis in "XYZ")
        return r[what]
    lds = lambda r: r["LDS_Block_Size"] if "LDS_Block_Size" in r else r["Group_Segment_Size"]
    return ["%s grid=%s workgroup=%s lds=%s" % (r["Kernel_Name"], size(r, "Grid_Size"), size(r, "Workgroup_Size"), lds(r)) for r in rows]


class _Dims:
    """What a population reads of its env when nothing is stepped: the sizes, the action table and the context."""
    continuous, obs_dim, action_space, env_id = False, N_OBS, {"n": A}, None
    cfg = types.SimpleNamespace(_actions=[-1.0, 0.0, 1.0])

    def __init__(self, n, ctx):
        self.n, self.ctx = n, ctx


def main():
    import numpy as np
    import torch
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        raise SystemExit("build the library first (__graft_entry__.build())")
    from rl_mpc_lanemerging_amd import _capi, learner
    ctx = _capi.Context(-1)
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    shape = dict(n_obs=N_OBS, n_actions=A, h1=H1, batch=BATCH, capacity=CAPACITY)
    makes = {
        "dqn": lambda per: learner.DQNLearner((N_OBS, A), learner.DQNConfig(per=per, **shape), seed=1, ctx=ctx),
        "c51": lambda per: learner.C51Learner((N_OBS, A), learner.C51Config(per=per, n_atoms=ATOMS, **shape), seed=1, ctx=ctx),
        "dqn-population": lambda per: learner.DQNPopulation(_Dims(P * ROWS, ctx), (learner.DQNConfig(**shape), P), per=per),
        "c51-population": lambda per: learner.C51Population(_Dims(P * ROWS, ctx), (learner.C51Config(n_atoms=ATOMS, **shape), P), per=per),
    }
    for per in (None, learner.PERConfig()):
        for kind, make in makes.items():
            L = make(per)
            n = P * ROWS if kind.endswith("population") else ROWS
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
            obs, nobs = t(rng.normal(size=(n, N_OBS)).astype(np.float32)), t(rng.normal(size=(n, N_OBS)).astype(np.float32))
            reward, term, trunc = t(rng.normal(size=n)), t(rng.random(n) < 0.2), t(np.zeros(n, dtype=bool))
            action = L.act(obs, None, eps=EPS)
            L.push(obs, None, action, reward, nobs, term, trunc)
            L.update(3)
            one = L.member(0) if kind.endswith("population") else L
            one.grads()
            one.targets()
            stats = L.stats()
            torch.cuda.synchronize()
            ctx.check_error()
            print(kind, "uniform" if per is None else "prioritised", "updates", np.asarray(stats["updates"]).tolist(), "fill", np.asarray(stats["fill"]).tolist(), flush=True)
            del L, one
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--launches":
        print("\n".join(launches(sys.argv[2])))
    else:
        main()
