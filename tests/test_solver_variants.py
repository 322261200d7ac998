"""Every reachable k_solve variant against the oracle: the cases of tests/solver_variant_cases.py (staged vehicle table, grouped solves on the wide-fan
lattice, the penalty-buffer overflow, waves per workgroup, and every shipped knob whose contract is "only trades speed"), each on a fresh context
under its STMPC_* settings, bit for bit against the CPU oracle's layered DP -- and then the statistics that prove the window the case is about saw an
episode.  tests/test_solver_variants_cpu.py shows, from the launch plan, which kernels each case launches.

The statistics every case showed are kept in profiles/solver/variant_cases_stats.json (evidence; the assertions are here)."""
import os

import numpy as np
import pytest

import solver_variant_cases as svc
from conftest import REPO, load_golden
from stmpc_testlib import check_solve as _check, record_json

pytestmark = pytest.mark.gpu

STATS = os.path.join(REPO, "profiles", "solver", "variant_cases_stats.json")
COUNTERS = ("episodes", "fallback", "hbm_tier", "retries", "guided", "pool_exhausted", "resume_refused")
KEYS = ("path_idx", "best_t", "cost", "crash", "path_dist")


class _World:
    """Parameters, states and oracle results of the table, each made once and shared by the cases (nothing here is written after it is made)."""

    def __init__(self):
        self.states, self.oracle = {}, {}

    def params(self, case):
        """(the lone Params, or the groups' ParamsTable; H)"""
        import rl_mpc_lanemerging_amd as pkg
        from rl_mpc_lanemerging_amd import _capi, st
        pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
        pkg.Settings.CRASH_MIN_S = 20
        pkg.apply_overrides(svc.LATTICES[case["lattice"]])
        pkg.apply_overrides(case["settings"])
        p = _capi.Params.from_settings(pkg.Settings)
        return (st.param_cfgs(case["groups"], pkg.Settings) if case["groups"] else p), _capi.num_t(p)

    def batch(self, name):
        if name not in self.states:
            from rl_mpc_lanemerging_amd import synth
            spec = svc.BATCHES[name]
            if "golden" in spec:
                g = load_golden(spec["golden"])
                a = tuple(np.ascontiguousarray(g[k]) for k in ("ego", "k_count", "other_x", "other_v"))
            else:
                ego, kc, ox, ov = synth.generate_states(**spec["synth"])
                kmax = spec["synth"]["kmax"]
                a = (ego, kc, np.ascontiguousarray(ox[:, :kmax]), np.ascontiguousarray(ov[:, :kmax]))
            for x in a:
                x.setflags(write=False)
            self.states[name] = a
        return self.states[name]

    def ref(self, case, p, cell=None):
        """The oracle's result for the case's batch under one parameter set."""
        from oracle import st_oracle as orc
        key = (case["lattice"], tuple(sorted(case["settings"].items())), tuple(sorted(cell.items())) if cell is not None else None, case["batch"])
        if key not in self.oracle:
            r = orc.solve_batch(orc.OrcParams.from_dict(p.as_dict()), *self.batch(case["batch"]), solver="layered", nthreads=16)
            self.oracle[key] = {k: r[k] for k in KEYS}
            for x in self.oracle[key].values():
                x.setflags(write=False)
        return self.oracle[key]


@pytest.fixture(scope="module")
def world():
    return _World()


def _equal(res, ref, H, rows=slice(None)):
    got = {k: res[k][rows] for k in KEYS}
    _check(got, ref, H)
    assert np.array_equal(got["cost"].view(np.uint64), ref["cost"].view(np.uint64)), "cost bits"


def _holds(stats, cond):
    counter, op, value = cond
    return stats[counter] > value if op == ">" else stats[counter] == value


@pytest.mark.parametrize("case", svc.CASES, ids=lambda c: c["name"])
def test_case_equals_the_oracle(case, world, restore_settings, monkeypatch):
    from rl_mpc_lanemerging_amd import _capi, st
    for knob, value in case["knobs"].items():
        monkeypatch.setenv(knob, value)
    p, H = world.params(case)
    states = world.batch(case["batch"])
    n = len(states[0])
    assert (n * len(case["groups"]) if case["groups"] else n) == case["N"] and states[2].shape[1] == case["Kmax"]
    ctx = _capi.Context(0)
    try:
        try:
            if case["groups"]:
                batch = tuple(np.ascontiguousarray(np.concatenate([a] * len(case["groups"]))) for a in states)
                res = st.solve_arrays_groups(p, n, *batch, ctx=ctx)
                stats = ctx.stats()
                lone = [st.solve_arrays(*states, p[g], ctx) for g in range(len(case["groups"]))]
            else:
                res = st.solve_arrays(*states, p, ctx)
                stats = ctx.stats()
        except _capi.StmpcError as e:
            pytest.exit("the device reported an error in case %s (%s): nothing more is started on it" % (case["name"], e), returncode=3)
        record_json(STATS, case["name"], {"knobs": case["knobs"], "N": case["N"], "stats": {k: int(stats[k]) for k in COUNTERS}})
        print(case["name"], {k: int(stats[k]) for k in COUNTERS})
        if case["groups"]:
            differ = False
            for g, cell in enumerate(case["groups"]):
                rows = slice(g * n, (g + 1) * n)
                _equal(res, world.ref(case, p[g], cell), H, rows)                   # the oracle under the group's parameters
                _equal(lone[g], world.ref(case, p[g], cell), H)
                for key in KEYS:                                                       # the lone call under them
                    assert np.array_equal(res[key][rows], lone[g][key], equal_nan=True), key
                first = np.where(res["best_t"][rows] >= 1, res["path_idx"][rows][:, 1], -1).astype(np.float64)
                assert np.array_equal(res["action_cost"][rows][:, 0], first)           # the fused (first-step cell, cost) rows
                assert np.array_equal(res["action_cost"][rows][:, 1].view(np.uint64), res["cost"][rows].view(np.uint64))
                differ |= g > 0 and not np.array_equal(res["path_idx"][rows], res["path_idx"][:n])
            assert differ, "the groups must not all drive alike"
        else:
            _equal(res, world.ref(case, p), H)
        # conditions, not tolerances: a case whose intended window saw no episode proves nothing
        assert stats["episodes"] == case["N"] and stats["resume_refused"] == 0      # (the audit's plans take the checkpoint pool as granted)
        for cond in case["expect"]:
            assert _holds(stats, cond), (cond, {k: int(stats[k]) for k in COUNTERS})
    finally:
        ctx.close()
