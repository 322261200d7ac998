"""Which of the library's 46 k_solve instantiations a GPU test launches, and which of them it hands work -- answered on a CPU, from the pure launch
plan (csrc/stmpc_solve_plan.hpp through tests/solve_plan_check.cpp) of every case of tests/solver_variant_cases.py on an MI355X's shape.

The variants launched and given work by the named cases are exactly the variants built; the checker's `reachable` sweep over the knobs that choose
kernels guards the rules variant_built prunes by.  profiles/solver/variant_coverage.txt is the printed table, and must equal the computation."""
import os
import subprocess

import pytest

import solver_variant_cases as svc
from conftest import REPO
from stmpc_testlib import build_plan_checker, fastdiv_proven, pkg as _pkg, plan_args, plan_of

COVERAGE = os.path.join(REPO, "profiles", "solver", "variant_coverage.txt")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_plan_checker(tmp_path_factory.mktemp("solver_variants"))


def params_of(case):
    """The case's stmpc_params as a dict (a grouped case: the base the cells are laid over -- the plan reads none of the fields a cell may set but
    v_w, a_w and j_w, and those for the band alone)."""
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import _capi
    snap = pkg.Settings.snapshot()
    try:
        pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
        pkg.Settings.CRASH_MIN_S = 20
        pkg.apply_overrides(svc.LATTICES[case["lattice"]])
        pkg.apply_overrides(case["settings"])
        p = _capi.Params.from_settings(pkg.Settings)
        return p.as_dict(), _capi.num_t(p)
    finally:
        pkg.Settings.restore(snap)


def launches_of(checker, case):
    """[(variant, tier, built)] of the case's plan on a fresh context, in launch order, and the number of tiers."""
    p, H = params_of(case)
    inputs = dict(svc.DEVICE, N=case["N"], Kmax=case["Kmax"], grouped=case["groups"] is not None, fastdiv_proven=fastdiv_proven(p["dt"]), H=H, params=[p],
                  knobs=case["knobs"])
    lines = plan_of(checker, inputs)
    assert lines[-1] == "pure 1"
    nt = int(lines[0].split()[2])
    out, tier = [], None
    for line in lines:
        if line.startswith("step solve "):
            tier = int(line.split()[9])
        elif line.startswith("launch "):
            name, rest = line[len("launch "):].split(" | ")
            out.append((name, tier, rest.split()[7] == "1"))
    return out, nt


def given_work(case, tier, nt):
    """Whether the case's conditions prove that the launch of `tier` saw an episode: the first window sees every episode; a later LDS window what
    the first passed on (fallback > 0); the HBM tier what is counted for it (hbm_tier > 0), and every window before it then passed something on.
    Under STMPC_FORCE_GENERAL the episodes go from the first window straight to the last tier."""
    if case["N"] == 0:
        return False
    if tier == 0:
        return True
    need = {(c, op) for c, op, v in case["expect"] if op == ">" and v >= 0}
    forced = case["knobs"].get("STMPC_FORCE_GENERAL") == "1"
    if forced:
        return tier == nt - 1
    if ("hbm_tier", ">") in need:
        return True
    return tier == 1 and ("fallback", ">") in need


@pytest.fixture(scope="module")
def coverage(checker):
    """variant -> {"launch": [case names], "work": [case names]} over every case, the suite's existing settings included."""
    cov = {}
    for case in svc.ALL:
        launches, nt = launches_of(checker, case)
        for name, tier, built in launches:
            assert built, "%s: the plan launches a variant the library does not build: %s" % (case["name"], name)
            slot = cov.setdefault(name, {"launch": [], "work": []})
            if case["name"] not in slot["launch"]:
                slot["launch"].append(case["name"])
            if given_work(case, tier, nt) and case["name"] not in slot["work"]:
                slot["work"].append(case["name"])
    return cov


def _label(names):
    """Case names for the table: the suite's existing settings by their test, once each."""
    by = {c["name"]: c for c in svc.ALL}
    out = []
    for n in names:
        label = n if by[n]["test"] is None else "[" + by[n]["test"].split("::")[1] + "]"
        if label not in out:
            out.append(label)
    return out


def render(cov, built):
    lines = ["# k_solve variants by the cases of tests/solver_variant_cases.py: variant | cases that launch it | cases that give it work",
             "# ([test]: a setting another GPU test runs).  Written by tests/test_solver_variants_cpu.py from the launch plan on %d compute units with" % svc.DEVICE["num_cu"],
             "# %d B of LDS." % svc.DEVICE["lds_per_block"]]
    for v in sorted(built):
        c = cov.get(v, {"launch": [], "work": []})
        lines.append("%s | %s | %s" % (v, " ".join(_label(c["launch"])) or "-", " ".join(_label(c["work"])) or "-"))
    return "\n".join(lines) + "\n"


def _built(checker):
    return [l for l in subprocess.run([checker, "variants"], check=True, capture_output=True, text=True).stdout.split("\n") if l]


def test_the_table_is_well_formed():
    pkg = _pkg()
    assert {k: pkg.SYNTHETIC_H40A21[k] for k in svc.H40A21} == svc.H40A21
    knobs = set()
    for c in svc.CASES:
        assert c["test"] is None and c["batch"] in svc.BATCHES and c["lattice"] in svc.LATTICES and c["exercises"], c["name"]
        assert c["N"] <= 640, c["name"]                     # (about 600 states at the most; the golden file as it is)
        assert all(op in (">", "==") for _, op, _ in c["expect"])
        knobs |= set(c["knobs"])
    for c in svc.ELSEWHERE:
        assert c["test"] and "::" in c["test"]
    # every shipped knob that no other test sets is set by a case here; the excluded one by none
    assert knobs >= {"STMPC_STAGE_TAB", "STMPC_PEN_CELLS", "STMPC_NW", "STMPC_SPLIT", "STMPC_PRIO", "STMPC_PRIO_MODE", "STMPC_RETRY", "STMPC_RETRY_MOVE", "STMPC_RETIRE_CUS",
                     "STMPC_RETIRE_AT", "STMPC_SIDE_GRID", "STMPC_BP16", "STMPC_BOUND_INFL", "STMPC_BAND2_MULT", "STMPC_LDS_HEADROOM", "STMPC_TIERS", "STMPC_FASTDIV", "STMPC_RESUME"}
    assert not knobs & set(svc.EXCLUDED_KNOBS) and "STMPC_CU_RESERVE" in svc.EXCLUDED_KNOBS
    # two of the grouped cells share their guide table, and the cells differ in every field a cell may set but A_WEIGHT and J_WEIGHT
    w = [(c["V_WEIGHT"], c.get("A_WEIGHT"), c.get("J_WEIGHT")) for c in svc.CELLS4]
    assert len(set(w)) == 3 and {c["V_WEIGHT"] for c in svc.CELLS4} == {0.0, 0.5, 10.0}
    assert {c["D_WEIGHT"] for c in svc.CELLS4} == {0.0, 10.0} and {c["MIN_ALLOWED_DISTANCE"] for c in svc.CELLS4} == {0, 8} and len({c["CRASH_MIN_S"] for c in svc.CELLS4}) > 1


@pytest.mark.parametrize("case", svc.CASES, ids=lambda c: c["name"])
def test_case_launches_what_it_claims(checker, case):
    """Every launch of the case's plan is a kernel the library builds, every kernel the case is there for is among them, and the case's conditions
    give it work."""
    launches, nt = launches_of(checker, case)
    assert launches and all(built for _, _, built in launches)
    worked = {name for name, tier, _ in launches if given_work(case, tier, nt)}
    for name in case["exercises"]:
        assert name in {l[0] for l in launches}, (name, launches)
        assert name in worked, "%s launches %s but no condition of it proves the kernel saw an episode" % (case["name"], name)


def test_every_built_variant_is_run(checker, coverage):
    """built == launched and given work by a named case, 46 of them: no kernel the library holds goes unexercised, and none is launched that it lacks."""
    built = _built(checker)
    assert len(built) == len(set(built)) == 46
    worked = {v for v, c in coverage.items() if c["work"]}
    assert worked == set(coverage) == set(built), (sorted(set(built) - worked), sorted(set(coverage) - set(built)))


def test_reachable_sweep_finds_nothing_new(checker, coverage):
    """The checker's sweep of the knobs that choose kernels (windows, waves, staged table, division, resume, bounded search, penalty cells, lone and
    grouped, N below and above the grid, Kmax 0 / 8 / 9) over the table's lattices: nothing it meets is unbuilt (one of variant_built's rules would be wrong) or uncovered."""
    built = set(_built(checker))
    met = set()
    for lattice in svc.LATTICES:
        p, H = params_of({"lattice": lattice, "settings": {}})
        out = subprocess.run([checker, "reachable", str(svc.DEVICE["num_cu"]), str(svc.DEVICE["lds_per_block"])] + plan_args(p, H), check=True, capture_output=True, text=True).stdout
        met |= {l for l in out.split("\n") if l}
    assert len(met) > 30
    assert met <= built, sorted(met - built)
    assert met <= {v for v, c in coverage.items() if c["work"]}, sorted(met - {v for v, c in coverage.items() if c["work"]})


def test_committed_coverage_table_is_current(checker, coverage):
    text = render(coverage, _built(checker))
    if os.environ.get("STMPC_WRITE_VARIANT_COVERAGE") == "1":
        with open(COVERAGE, "w") as fh:
            fh.write(text)
    assert os.path.exists(COVERAGE), "profiles/solver/variant_coverage.txt is missing (STMPC_WRITE_VARIANT_COVERAGE=1 writes it)"
    assert open(COVERAGE).read() == text, "profiles/solver/variant_coverage.txt differs from the computation (STMPC_WRITE_VARIANT_COVERAGE=1 rewrites it)"
