"""The solver's launch plan (csrc/stmpc_solve_plan.hpp) on a CPU, against the launches the parent commit made on an MI355X.

profiles/solver/launch_plan_parent.json holds, for eight solve calls (wide and narrow lattice, N below and above the first grid, two-phase, no overlap /
no resume, small windows, staged table, solver groups), the inputs and every k_solve launch of the commit before the plan existed: kernel name, workgroups,
block, dynamic LDS bytes, in order.  tests/solve_plan_check.cpp prints plan_solve's answer for the same inputs; the two must be equal."""
import json
import os
import subprocess

import pytest

from stmpc_testlib import build_plan_checker, plan_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(REPO, "profiles", "solver", "launch_plan_parent.json")))["cases"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_plan_checker(tmp_path_factory.mktemp("solve_plan"))


@pytest.mark.parametrize("case", RECORD, ids=lambda c: "case%d" % c["case"])
def test_plan_equals_the_parents_launches(checker, case):
    lines = plan_of(checker, case["inputs"])
    got = []
    for line in lines:
        if line.startswith("launch "):
            name, rest = line[len("launch "):].split(" | ")
            f = rest.split()
            got.append({"kernel": name, "grid": int(f[1]), "block": int(f[3]), "lds": int(f[5])})
            assert f[7] == "1", "the planner emitted a variant the dispatch does not build: " + name
    want = [{k: l[k] for k in ("kernel", "grid", "block", "lds")} for l in case["launches"]]
    assert got == want
    # the stream of each launch, from the schedule
    streams = [l.split()[3] for l in lines if l.startswith("step solve ")]
    assert streams == [l["stream"] for l in case["launches"]]
    assert lines[-1] == "pure 1", "two calls of plan_solve on equal inputs differ"


def test_record_covers_the_plan_flags():
    """The eight cases flip what they are meant to flip: side launch or none, N below the first grid, narrow and wide fan-out, staged table, grouped."""
    by = {c["case"]: c for c in RECORD}
    assert len(RECORD) == 8
    assert [l["stream"] for l in by[1]["launches"]].count("side") == 1 and all(l["stream"] == "main" for l in by[2]["launches"] + by[5]["launches"])
    assert by[2]["launches"][0]["grid"] == by[2]["inputs"]["N"] < by[1]["launches"][0]["grid"]
    assert ", 9, " in by[3]["launches"][0]["kernel"] and ", 8, 9, " in by[7]["launches"][0]["kernel"]
    assert len(by[4]["launches"]) == len(by[1]["launches"]) and by[4]["launches"][0] == by[4]["launches"][1]
    assert all(l["kernel"].startswith("grouped::") for l in by[8]["launches"]) and by[8]["inputs"]["grouped"]


def test_variant_list_is_the_librarys(checker):
    """variant_built (the list the dispatch compiles from, and DESIGN.md section 4 tabulates) names exactly the batched k_solve kernels of the library:
    the rows of profiles/solver/resource_usage_variants.txt, less stmpc_solve_grid's one GRID kernel."""
    listed = subprocess.run([checker, "variants"], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    rows = [l for l in open(os.path.join(REPO, "profiles", "solver", "resource_usage_variants.txt")) if "k_solve<" in l and not l.startswith(("#", "k_solve<false, true,"))]
    assert len(listed) == len(set(listed)) == 46 and sorted(listed) == sorted(r[:r.index(">") + 1] for r in rows)
