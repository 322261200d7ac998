"""Solver groups on the GPU (main.py:43-59, do_grid_search_st): a batch split into G groups of n_per_group states, each under its own V/A/J/D_WEIGHT,
MIN_ALLOWED_DISTANCE and CRASH_MIN_S, against lone calls under each cell and against the CPU oracle.  Everything is compared bit for bit, on the
reference's own lattice (H = 18, S = 3001) with states of tests/golden/golden_default.npz."""
import numpy as np
import pytest

from conftest import load_golden, settings_from_golden

pytestmark = pytest.mark.gpu

# four cells of the grid: between them A_WEIGHT = 0, J_WEIGHT = 0, D_WEIGHT = 0 and 1000, MIN_ALLOWED_DISTANCE 5 and 6, CRASH_MIN_S 10 and 20
CELLS = [{"V_WEIGHT": 0.5, "A_WEIGHT": 0.0, "J_WEIGHT": 0.0, "D_WEIGHT": 0.0, "MIN_ALLOWED_DISTANCE": 5, "CRASH_MIN_S": 10},
         {"V_WEIGHT": 1.0, "A_WEIGHT": 10.0, "J_WEIGHT": 10.0, "D_WEIGHT": 1000.0, "MIN_ALLOWED_DISTANCE": 6, "CRASH_MIN_S": 20},
         {"V_WEIGHT": 1.0, "A_WEIGHT": 0.0, "J_WEIGHT": 50.0, "D_WEIGHT": 10.0, "MIN_ALLOWED_DISTANCE": 5, "CRASH_MIN_S": 20},
         {"V_WEIGHT": 0.5, "A_WEIGHT": 10.0, "J_WEIGHT": 0.0, "D_WEIGHT": 100.0, "MIN_ALLOWED_DISTANCE": 6, "CRASH_MIN_S": 10}]
# Five states every group receives, picked with the CPU oracle: in each of them the four cells disagree in path_idx, in 1, 6 and 13 also in crash, in 6, 13
# and 61 also in best_t -- a kernel that ignored the table could not pass.
STATES = [0, 1, 6, 13, 61]
NPG = len(STATES)
KEYS = ("path_idx", "best_t", "crash")


def _same(a, b, rows=slice(None)):
    for key in KEYS:
        assert np.array_equal(a[key][rows], b[key]), key
    assert np.array_equal(a["cost"][rows].view(np.uint64), b["cost"].view(np.uint64)), "cost bits"
    assert np.array_equal(a["path_dist"][rows].view(np.uint64), b["path_dist"].view(np.uint64)), "path_dist bits"


def _same_oracle(a, ref, rows=slice(None)):
    for key in KEYS:
        assert np.array_equal(a[key][rows], ref[key]), key
    assert np.array_equal(a["cost"][rows].view(np.uint64), ref["cost"].view(np.uint64)), "cost bits"
    m = ~np.isnan(ref["path_dist"])
    assert np.array_equal(np.isnan(a["path_dist"][rows]), ~m) and np.array_equal(a["path_dist"][rows][m], ref["path_dist"][m]), "path_dist"


@pytest.fixture(scope="module")
def case():
    """The states (the five, once per group), the table of the four cells and, per cell, the oracle's result for the five states."""
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import st
    from oracle import st_oracle as orc
    snap = pkg.Settings.snapshot()
    g = load_golden("golden_default.npz")
    settings_from_golden(g)
    table = st.param_cfgs(CELLS, pkg.Settings)
    pkg.Settings.restore(snap)
    five = tuple(np.ascontiguousarray(g[k][STATES]) for k in ("ego", "k_count", "other_x", "other_v"))
    batch = tuple(np.ascontiguousarray(np.concatenate([a] * len(CELLS))) for a in five)
    oracle = [orc.solve_batch(orc.OrcParams.from_dict(p.as_dict()), *five, solver="layered", nthreads=4) for p in table]
    assert any(not np.array_equal(oracle[0]["path_idx"], o["path_idx"]) or not np.array_equal(oracle[0]["crash"], o["crash"]) for o in oracle[1:])
    return {"g": g, "table": table, "five": five, "batch": batch, "oracle": oracle}


def _group_lone_oracle(ctx, case):
    from rl_mpc_lanemerging_amd import st
    res = st.solve_arrays_groups(case["table"], NPG, *case["batch"], ctx=ctx)
    differ = False
    for c, p in enumerate(case["table"]):
        rows = slice(c * NPG, (c + 1) * NPG)
        lone = st.solve_arrays(*case["five"], p, ctx)
        _same(res, lone, rows)
        _same_oracle(res, case["oracle"][c], rows)
        differ |= c > 0 and (not np.array_equal(res["path_idx"][rows], res["path_idx"][:NPG]) or not np.array_equal(res["crash"][rows], res["crash"][:NPG]))
        # the fused (first-step cell, cost) rows
        first = np.where(res["best_t"][rows] >= 1, res["path_idx"][rows][:, 1], -1).astype(np.float64)
        assert np.array_equal(res["action_cost"][rows][:, 0], first)
        assert np.array_equal(res["action_cost"][rows][:, 1].view(np.uint64), res["cost"][rows].view(np.uint64))
    assert differ, "at least two groups must differ in path_idx or crash"
    return res


def test_group_equals_lone_equals_oracle(gpu_ctx, case):
    """G = 4 groups of 5 states (N = 20: the group boundaries fall inside k_predict's wavefronts): group g's rows are a lone stmpc_solve_batch's under
    cell g and the oracle's."""
    _group_lone_oracle(gpu_ctx, case)


@pytest.mark.parametrize("fastdiv", ["1", "0"])
def test_group_equals_lone_with_first_window_overflow(case, fastdiv, monkeypatch):
    """The same with the first window forced to overflow (a knob setting of test_window_overflow_falls_back_exactly, with either division): the
    overflow queue and the wider windows look the group up by the episode's index too."""
    from rl_mpc_lanemerging_amd import _capi
    monkeypatch.setenv("STMPC_TIERS", "256,512")
    monkeypatch.setenv("STMPC_FASTDIV", fastdiv)
    ctx = _capi.Context(0)
    _group_lone_oracle(ctx, case)
    assert ctx.stats()["fallback"] > 0
    ctx.close()


def test_overflow_with_the_side_launch(case, monkeypatch):
    """A batch larger than the first window's grid (4 groups x the 320 golden states on one workgroup per compute unit), with the second window
    started alongside the first (STMPC_OVERLAP=1): the side launch consumes the overflow queue while it fills, by episode index."""
    from rl_mpc_lanemerging_amd import _capi, st
    from oracle import st_oracle as orc
    monkeypatch.setenv("STMPC_TIERS", "256,512")
    monkeypatch.setenv("STMPC_OVERLAP", "1")
    monkeypatch.setenv("STMPC_WAVES_PER_CU", "4")
    g = case["g"]
    all_ = tuple(np.ascontiguousarray(g[k]) for k in ("ego", "k_count", "other_x", "other_v"))
    n = len(all_[0])
    batch = tuple(np.ascontiguousarray(np.concatenate([a] * len(CELLS))) for a in all_)
    ctx = _capi.Context(0)
    res = st.solve_arrays_groups(case["table"], n, *batch, ctx=ctx)
    assert ctx.stats()["fallback"] > 0
    for c, p in enumerate(case["table"]):
        ref = orc.solve_batch(orc.OrcParams.from_dict(p.as_dict()), *all_, solver="layered", nthreads=8)
        _same_oracle(res, ref, slice(c * n, (c + 1) * n))
    ctx.close()


def test_one_group_and_288_groups(gpu_ctx, case):
    """G = 1 is the ungrouped entry; G = 288 with one state per group is 288 lone oracle solves (the whole grid, one table row per episode)."""
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi, st
    from oracle import st_oracle as orc
    p = case["table"][1]
    g = case["g"]
    many = tuple(np.ascontiguousarray(g[k][:37]) for k in ("ego", "k_count", "other_x", "other_v"))
    one = st.solve_arrays_groups([p], 37, *many, ctx=gpu_ctx)
    _same(one, st.solve_arrays(*many, p, gpu_ctx))
    snap = pkg.Settings.snapshot()
    settings_from_golden(g)
    grid = st.param_cfgs(st.grid_search_cells(), pkg.Settings)
    pkg.Settings.restore(snap)
    assert len(grid) == 288 <= _capi.SOLVER_GROUPS_MAX
    idx = [STATES[c % NPG] for c in range(288)]
    batch = tuple(np.ascontiguousarray(g[k][idx]) for k in ("ego", "k_count", "other_x", "other_v"))
    res = st.solve_arrays_groups(grid, 1, *batch, ctx=gpu_ctx)
    for c, q in enumerate(grid):
        ref = orc.solve_batch(orc.OrcParams.from_dict(q.as_dict()), *(a[c:c + 1] for a in batch), solver="layered", nthreads=1)
        _same_oracle(res, ref, slice(c, c + 1))


def test_st_control_groups(gpu_ctx, case):
    """The grouped control entry: speed, fine and fine_len (and the paths under them) of group g are the lone control entry's under cell g."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import _capi
    ego, kc, ox, ov = case["batch"]
    N, K, H = len(ego), ox.shape[1], _capi.num_t(case["table"][0])
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(a).to(dev) for a in (ego, kc, ox, ov)]
    path, bt = torch.zeros(N, H, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    cost, speed = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
    fine, flen = torch.zeros(N, _capi.QP_NMAX, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    tick = pkg.Settings.TICK_LENGTH
    gpu_ctx.st_control_groups_device(case["table"], NPG, tick, N, K, *(t.data_ptr() for t in d), path.data_ptr(), bt.data_ptr(), cost.data_ptr(), speed.data_ptr(),
                                     fine.data_ptr(), flen.data_ptr())
    torch.cuda.synchronize()
    gpu_ctx.check_error()
    speeds = []
    for c, p in enumerate(case["table"]):
        rows = slice(c * NPG, (c + 1) * NPG)
        lone = gpu_ctx.st_control_batch(p, tick, *case["five"], want_paths=True)
        assert np.array_equal(speed.cpu().numpy()[rows].view(np.uint64), lone["speed"].view(np.uint64))
        assert np.array_equal(flen.cpu().numpy()[rows], lone["fine_len"])
        for i in range(NPG):
            n = max(int(lone["fine_len"][i]), 0)
            assert np.array_equal(fine.cpu().numpy()[rows][i, :n].view(np.uint64), lone["fine"][i, :n].view(np.uint64))
        assert np.array_equal(path.cpu().numpy()[rows], lone["path_idx"]) and np.array_equal(bt.cpu().numpy()[rows], lone["best_t"])
        speeds.append(lone["speed"])
    assert any(not np.array_equal(speeds[0], s) for s in speeds[1:])


def test_episodes_groups_equal_lone_runners(gpu_ctx, restore_settings, monkeypatch):
    """EpisodeRunner(n=32, solver=[a, b], traffic of one seed) for 40 ticks against two lone runners of 16 environments with Settings patched to the
    cell: status, ticks, ego4 and every stats column.  The cells differ in CRASH_MIN_S too, and closest_distance must show it: the egos start 180 m
    along the ramp (s = -21.6) instead of 40 m, so that they pass s = 10 and s = 20, where the gates open, within the 40 ticks (8 s)."""
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import episodes
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    monkeypatch.setattr(episodes, "EGO_START_ARC", 180.0)
    a = {"V_WEIGHT": 0.5, "A_WEIGHT": 10.0, "J_WEIGHT": 10.0, "D_WEIGHT": 10.0, "MIN_ALLOWED_DISTANCE": 5, "CRASH_MIN_S": 10}
    b = {"V_WEIGHT": 1.0, "A_WEIGHT": 0.0, "J_WEIGHT": 50.0, "D_WEIGHT": 1000.0, "MIN_ALLOWED_DISTANCE": 6, "CRASH_MIN_S": 20}
    traffic = [dict(episodes.TRAFFIC_TYPES["default"], seed=7) for _ in range(2)]
    both = episodes.run_episodes(32, controller="st", ctx=gpu_ctx, kmax=16, max_ticks=40, traffic=traffic, solver=[a, b])
    assert np.array_equal(both["solver_group"], np.arange(32) // 16)
    lone = []
    for cell in (a, b):
        snap = pkg.Settings.snapshot()
        pkg.apply_overrides(cell)
        lone.append(episodes.run_episodes(16, controller="st", ctx=gpu_ctx, kmax=16, max_ticks=40, traffic=traffic[:1]))
        pkg.Settings.restore(snap)
    for c in range(2):
        rows = slice(c * 16, (c + 1) * 16)
        for key, col in lone[c].items():
            if key == "traffic_group":
                continue
            assert np.array_equal(np.asarray(both[key])[rows], np.asarray(col), equal_nan=True), (c, key)
    cd = both["closest_distance"]
    assert np.isfinite(cd[:16]).any(), "no ego passed CRASH_MIN_S = 10: the gate was never open"
    assert not np.array_equal(cd[:16], cd[16:], equal_nan=True), "the groups' CRASH_MIN_S gates must act on closest_distance"


def test_more_cells_than_traffic_groups_in_one_runner(gpu_ctx, restore_settings, monkeypatch):
    """72 cells of the grid (more than STMPC_SIM_GROUPS_MAX = 64) as one runner of one environment per cell on one traffic seed, 12 ticks: the first
    cell, cell 64 and the last are lone runners with Settings patched to the cell."""
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import episodes, st
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    monkeypatch.setattr(episodes, "EGO_START_ARC", 180.0)
    cells = st.grid_search_cells()[::4]
    assert len(cells) == 72
    out = episodes.grid_search_st(1, seed=3, traffic="default", cells=cells, ctx=gpu_ctx, max_ticks=12)
    stats = out["stats"]
    assert len(out["cells"]) == 72 and np.array_equal(stats["solver_group"], np.arange(72)) and np.array_equal(stats["traffic_group"], np.arange(72))
    for c in (0, 64, 71):
        snap = pkg.Settings.snapshot()
        pkg.apply_overrides(cells[c])
        lone = episodes.run_episodes(1, controller="st", ctx=gpu_ctx, kmax=16, max_ticks=12, traffic=[dict(episodes.TRAFFIC_TYPES["default"], seed=3)])
        pkg.Settings.restore(snap)
        for key, col in lone.items():
            if key != "traffic_group":
                assert np.array_equal(np.asarray(stats[key])[c:c + 1], np.asarray(col), equal_nan=True), (c, key)
    assert len({tuple(stats["ego4"][c]) for c in range(72)}) > 1, "the cells must not all drive alike"


def test_refusals_leave_the_context_usable(gpu_ctx, case):
    from rl_mpc_lanemerging_amd import _capi, episodes, st

    def refused(word, fn, *args, **kw):
        with pytest.raises(_capi.StmpcError) as e:
            fn(*args, **kw)
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    p0 = case["table"][0]
    for field in ("ds", "j_max", "comb_min_dist"):
        q = _capi.Params.from_buffer_copy(bytes(p0))
        setattr(q, field, getattr(q, field) * 1.5)
        refused(field, st.solve_arrays_groups, [p0, q], NPG, *(a[:2 * NPG] for a in case["batch"]), ctx=gpu_ctx)
    refused("G must be", st.solve_arrays_groups, _capi.ParamsTable([]), NPG, *case["five"], ctx=gpu_ctx)
    refused("G * n_per_group", st.solve_arrays_groups, case["table"], NPG - 1, *case["batch"], ctx=gpu_ctx)
    with pytest.raises(ValueError):
        episodes.EpisodeRunner(4, controller="combined", ctx=gpu_ctx, solver=[CELLS[0], CELLS[1]])
    _group_lone_oracle(gpu_ctx, case)
