"""Solver groups, host side (st.param_cfgs / grid_search_cells, the solver argument of EpisodeRunner, episodes.summary_by_solver, the
stmpc_*_groups entries of include/stmpc.h that take a table of stmpc_params).  No GPU: the grid against main.py:44-51 written out here, param_cfgs
leaves the global Settings alone, header / library / binding agree, and every pairing mismatch is a ValueError raised before a context is asked for
anything."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import REPO
from stmpc_testlib import pkg as _pkg

ENTRIES = {"stmpc_solve_batch_groups_device", "stmpc_solve_batch_groups", "stmpc_st_control_groups_device", "stmpc_solver_groups_sim_step_device",
           "stmpc_solver_groups_sim_init_device"}


class _NoDevice:
    """A context that must not be asked for anything."""

    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


def test_grid_search_cells_are_the_reference_product():
    _pkg()
    from rl_mpc_lanemerging_amd import st
    grid = {"V_WEIGHT": [0.5, 1.0], "A_WEIGHT": [0.0, 10.0], "J_WEIGHT": [0.0, 10.0, 50.0], "D_WEIGHT": [0.0, 10.0, 100.0, 1000.0],
            "MIN_ALLOWED_DISTANCE": [5, 6], "CRASH_MIN_S": [10, 15, 20]}                      # main.py:44-51
    want = [dict(zip(grid.keys(), values)) for values in itertools.product(*grid.values())]
    cells = st.grid_search_cells()
    assert len(cells) == 288 == 2 * 2 * 3 * 4 * 2 * 3
    assert cells[0] == {"V_WEIGHT": 0.5, "A_WEIGHT": 0.0, "J_WEIGHT": 0.0, "D_WEIGHT": 0.0, "MIN_ALLOWED_DISTANCE": 5, "CRASH_MIN_S": 10}
    assert cells[-1] == {"V_WEIGHT": 1.0, "A_WEIGHT": 10.0, "J_WEIGHT": 50.0, "D_WEIGHT": 1000.0, "MIN_ALLOWED_DISTANCE": 6, "CRASH_MIN_S": 20}
    assert cells == want and [list(c) for c in cells] == [list(grid)] * 288
    assert cells[1]["CRASH_MIN_S"] == 15 and cells[3]["MIN_ALLOWED_DISTANCE"] == 6          # the last key varies fastest


def test_param_cfgs_validates_and_leaves_settings_alone(restore_settings):
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, st
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    before = pkg.Settings.snapshot()
    base = capi.Params.from_settings(pkg.Settings)
    cells = [{}, {"V_WEIGHT": 1.0, "A_WEIGHT": 0.0, "J_WEIGHT": 50.0, "D_WEIGHT": 1000.0, "MIN_ALLOWED_DISTANCE": 6, "CRASH_MIN_S": 10}, {"CRASH_MIN_S": 15}]
    table = st.param_cfgs(cells)
    assert pkg.Settings.snapshot() == before
    assert isinstance(table, capi.ParamsTable) and len(table) == 3
    want = [{}, {"v_w": 1.0, "a_w": 0.0, "j_w": 50.0, "d_w": 1000.0, "min_allowed": 6.0, "crash_min_s": 10.0}, {"crash_min_s": 15.0}]
    for g in range(3):
        for p in (table[g], table.array[g]):                      # the copy handed out and the row the library reads
            for name, _ in capi.Params._fields_:
                assert getattr(p, name) == want[g].get(name, getattr(base, name)), (g, name)
    # another settings object is read in place of the global one
    class Other(pkg.Settings):
        V_WEIGHT = 7.0
    assert st.param_cfgs([{}], Other)[0].v_w == 7.0 and st.param_cfgs([{}])[0].v_w == base.v_w
    assert pkg.Settings.snapshot() == before
    with pytest.raises(ValueError, match="not DESIRED_SPEED"):
        st.param_cfgs([{"V_WEIGHT": 1.0}, {"DESIRED_SPEED": 20.0}])
    with pytest.raises(ValueError, match="1 ... %d groups, not 0" % capi.SOLVER_GROUPS_MAX):
        st.param_cfgs([])
    with pytest.raises(ValueError, match="not %d" % (capi.SOLVER_GROUPS_MAX + 1)):
        st.param_cfgs([{}] * (capi.SOLVER_GROUPS_MAX + 1))
    assert len(st.param_cfgs(st.grid_search_cells())) == 288


def test_header_library_and_binding_agree_on_the_solver_group_entries():
    _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi
    lib = capi.load()
    header = " ".join(open(os.path.join(REPO, "include", "stmpc.h")).read().split())
    declared = {name: args for name, args in re.findall(r"\bint (stmpc_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header) if name in ENTRIES}
    assert set(declared) == ENTRIES <= set(capi.EXPORTS)
    for name, args in declared.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")), name
        assert ("const stmpc_sim_cfg *cfgs" if name.endswith("sim_init_device") else "const stmpc_params *groups") + ", int G, int n_per_group" in args, name
    assert "#define STMPC_SOLVER_GROUPS_MAX %d" % capi.SOLVER_GROUPS_MAX in header and capi.SOLVER_GROUPS_MAX >= 288
    assert header.count("main.py:43-59") >= 5
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8 and "#define STMPC_ABI_VERSION 8" in header
    # the table is stmpc_params rows, back to back
    import ctypes
    t = capi.ParamsTable([capi.Params(ds=0.05), capi.Params(ds=0.1)])
    assert ctypes.sizeof(t.array) == 2 * ctypes.sizeof(capi.Params) == 2 * 24 * 8 and t.array[1].ds == 0.1


def test_summary_by_solver():
    _pkg()
    from rl_mpc_lanemerging_amd import episodes
    stats = {"status": np.array([1, 1, 2, 2, 1, 2]), "ticks": np.arange(6), "merged": np.array([1.0, 1, 0, 0, 1, 0]),
             "closest_distance": np.array([4.0, np.nan, 2.0, 6.0, np.nan, 1.0]), "solver_group": np.arange(6) // 2}
    by = episodes.summary_by_solver(stats, 3)
    assert [b["merged"] for b in by] == [1.0, 0.0, 0.5] and [b["closest_distance"] for b in by] == [4.0, 4.0, 1.0]
    assert "solver_group" not in by[0] and "solver_group" not in episodes.summary(stats)
    with pytest.raises(ValueError, match="do not split into 4 solver groups"):
        episodes.summary_by_solver(stats, 4)


def test_pairing_rules_are_checked_before_any_context(restore_settings):
    pkg = _pkg()
    from rl_mpc_lanemerging_amd import episodes
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    nodev = _NoDevice()
    a, b = {"CRASH_MIN_S": 10}, {"D_WEIGHT": 1000.0}
    with pytest.raises(ValueError, match="settings of the ST controller, not of 'combined'"):
        episodes.EpisodeRunner(4, controller="combined", ctx=nodev, solver=[a, b])
    with pytest.raises(ValueError, match="settings of the ST controller, not of 'first_step'"):
        episodes.run_episodes(4, controller="first_step", policy=object(), ctx=nodev, solver=[a, b])
    with pytest.raises(ValueError, match="7 environments do not split into 2 solver groups"):
        episodes.EpisodeRunner(7, ctx=nodev, solver=[a, b])
    with pytest.raises(ValueError, match="the traffic has 3 groups, the solver 2"):
        episodes.EpisodeRunner(12, ctx=nodev, traffic=["low", "default", "fast"], solver=[a, b])
    with pytest.raises(ValueError, match="not ROLLOUT_LENGTH"):
        episodes.EpisodeRunner(4, ctx=nodev, solver=[a, {"ROLLOUT_LENGTH": 3}])
    with pytest.raises(ValueError, match="1 ... 512 groups, not 513"):
        episodes.EpisodeRunner(513, ctx=nodev, solver=[a] * 513)
    with pytest.raises(ValueError, match="1 ... 64 groups, not 65"):                    # (without solver groups the traffic groups keep their limit)
        episodes.EpisodeRunner(65, ctx=nodev, traffic=["low"] * 65)
    assert episodes._check_solver(288, [a] * 288, None, "st") == (288, 1)
    assert episodes._check_traffic(288, ["low"] * 288, None, 512) == (288, 1)
    with pytest.raises(ValueError, match="n_per_cell must be positive"):
        episodes.grid_search_st(0, ctx=nodev)
    with pytest.raises(ValueError, match="not TICK_LENGTH"):
        episodes.grid_search_st(4, ctx=nodev, cells=[{"TICK_LENGTH": 0.1}])
    assert episodes._check_solver(12, [a, b], ["low", "fast"], "st") == (2, 6)
