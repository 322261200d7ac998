"""golden_combined_cells.npz / golden_combined_cells_b.npz (tests/golden/make_golden_combined_cells.py): the reference's do_combined_control in
the 13 cells of its grid search (base A) and in 10 cells with LIMIT_DQN_SPEED on, CHECK_ROLLOUT_CRASH on and off (base B).

Two things are checked here, without a GPU: that the committed fixtures cover what the GPU tests rely on, and that the CPU twin
(stmpc_testlib.combined_twin: the decision tree on the oracle's predictor and solver) reproduces every cell bit for bit.  The twin is the layer
in between: where tests/test_combined_cells.py disagrees with the fixture and this module does not, the device side is wrong; where both
disagree alike, the restatement is.  Every comparison is equality."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from stmpc_testlib import apply_cell as _apply_cell, combined_cells as _combined_cells, combined_twin as _combined_twin, stub_policy

N, N_BOOK, CELLS = 240, 64, 23


def _fixture():
    g = load_golden("golden_combined_cells.npz")
    return g, _combined_cells(g)


def test_fixture_shapes_and_settings():
    g, cells = _fixture()
    assert len(cells) == CELLS and [c["base"] for c in cells] == [0] * 13 + [1] * 10
    assert g["ego"].shape == (N, 5) and g["other_x"].shape == g["other_v"].shape == (N, 8) and g["k_count"].shape == (N,)
    for q in ("reason", "takeover", "crash_predicted", "rollout_steps", "selected_speed"):
        assert g[q].shape == (CELLS, N), q
    assert g["selected_speed"].dtype == np.float64 and g["hist"].dtype == np.float64
    assert g["test_ego4"].shape == (CELLS, N_BOOK, 4) and g["test_ox"].shape == g["test_ov"].shape == (CELLS, N_BOOK, 8)
    assert g["test_fallback"].shape == (CELLS, N_BOOK) and g["hist_off"].shape == (CELLS * N_BOOK + 1,) and g["hist_off"][-1] == len(g["hist"])
    # the history of a row has its rollout's steps and the start state's s
    assert np.array_equal(np.diff(g["hist_off"]).reshape(CELLS, N_BOOK), g["rollout_steps"][:, :N_BOOK] + 1)
    assert list(g["flags"]) == [1, 0, 1, 0] and dict(zip(g["setting_keys"], g["setting_vals"]))["DESIRED_SPEED"] == 30.0
    # base A is the reference's grid search, cell for cell; base B crosses five cells with the crash check
    grid = json.load(open(os.path.join(GOLDEN, "combined_grid.json")))
    assert [{k: c[k] for k in grid["keys"]} for c in cells[:13]] == grid["cells"]
    assert all(c["CHECK_ROLLOUT_CRASH"] and not c["LIMIT_DQN_SPEED"] and c["DESIRED_SPEED"] == 30.0 for c in cells[:13])
    lpt = [(c["ROLLOUT_LENGTH"], c["ST_TEST_ROLLOUTS"], c["TEST_ROLLOUT_STATE"]) for c in cells[13:]]
    assert lpt == [(3, 2, True), (5, 5, True), (10, 2, False), (1, 2, True), (12, 3, True)] * 2
    assert [c["CHECK_ROLLOUT_CRASH"] for c in cells[13:]] == [True] * 5 + [False] * 5
    assert all(c["LIMIT_DQN_SPEED"] and c["DESIRED_SPEED"] == 16.0 for c in cells[13:])
    assert np.array_equal(g["takeover"], (g["reason"] != 0).astype(np.int32))


def test_fixture_covers_every_reason_and_edge():
    g, cells = _fixture()
    reason = g["reason"]
    base = np.array([c["base"] for c in cells])
    check = np.array([c["CHECK_ROLLOUT_CRASH"] for c in cells])
    R = np.array([c["ROLLOUT_LENGTH"] for c in cells])
    T = np.array([c["ST_TEST_ROLLOUTS"] for c in cells])
    for r in range(4):
        assert (reason == r).sum() >= 20, r
    assert reason.min() == 0 and reason.max() == 3
    for c in np.nonzero(base == 1)[0]:
        assert (reason[c] == 2).sum() >= 50, c
    for c in range(CELLS):
        assert (reason[c] == 1).sum() >= 3 if check[c] else not (reason[c] == 1).any(), c
    # the reason priority: a predicted crash that is not checked falls through to the too-fast test (1 -> 2) or the probe (1 -> 3)
    changed = set()
    for c in range(13, 18):
        changed |= {(int(a), int(b)) for a, b in zip(reason[c], reason[c + 5]) if a != b}
    assert (1, 2) in changed and (1, 3) in changed
    # rollouts the STOP_X break ended, and probe states taken by the fallback of dqn.py:142-143
    assert ((g["rollout_steps"] < R[:, None]) & (g["crash_predicted"] == 0)).sum() >= 5
    assert g["test_fallback"].sum(axis=1).max() >= 5
    assert np.array_equal(g["test_fallback"], (g["rollout_steps"][:, :N_BOOK] < T[:, None]).astype(np.int32))
    b = load_golden("golden_combined_cells_b.npz")
    assert b["b_reason"].shape == (6, 120) and int(b["n"]) == 120
    assert b["part_vals"].tolist() == [[1, 2, 0], [1, 2, 1], [3, 2, 0], [3, 2, 1], [10, 2, 0], [10, 2, 1]]
    for p in range(6):
        assert (b["b_reason"][p] == 0).sum() >= 5 and (b["b_reason"][p] == 4).sum() >= 5, p
    assert np.array_equal(b["b_last_rl"], np.tile((np.arange(120) % 3 != 1).astype(np.int32), (6, 1)))
    assert np.array_equal(b["b_takeover"], (b["b_reason"] != 0).astype(np.int32))
    assert np.isfinite(b["b_speed"][b["b_reason"] == 4]).all() and np.isnan(b["b_speed"][b["b_reason"] != 4]).all()
    size = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ("golden_combined_cells.npz", "golden_combined_cells_b.npz"))
    assert size < 480 * 1024


def twin_mismatches(g, c, twin):
    """The quantities of cell ``c`` in which a twin result differs from the fixture (none: [])."""
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    bad = [q for q in ("reason", "takeover", "crash_predicted", "rollout_steps") if not np.array_equal(twin[q], g[q][c])]
    if not np.array_equal(i64(twin["selected_speed"]), i64(g["selected_speed"][c])):
        bad.append("selected_speed")
    off = g["hist_off"][c * N_BOOK:(c + 1) * N_BOOK + 1]
    for i in range(N_BOOK):
        if not np.array_equal(i64(twin["rollout_s"][i]), i64(g["hist"][off[i]:off[i + 1]])):
            bad.append("rollout_s[%d]" % i)
        t, k = twin["test_states"][i], int(g["k_count"][i])
        same = (np.array_equal(i64([t.ego_x, t.ego_y, t.ego_v, t.ego_a]), i64(g["test_ego4"][c, i])) and t.k == k
                and np.array_equal(i64(t.xs[:k]), i64(g["test_ox"][c, i, :k])) and np.array_equal(i64(t.vs[:k]), i64(g["test_ov"][c, i, :k])))
        if not same:
            bad.append("test_state[%d]" % i)
    if not np.array_equal(twin["test_fallback"][:N_BOOK], g["test_fallback"][c]):
        bad.append("test_fallback")
    return bad


@pytest.mark.parametrize("c", range(CELLS))
def test_twin_reproduces_the_reference_in_every_cell(restore_settings, c):
    g, cells = _fixture()
    S = _apply_cell(g, cells[c]).Settings
    twin = _combined_twin(S, (g["ego"], g["k_count"], g["other_x"], g["other_v"]), lambda i, step, state: stub_policy(state))
    assert twin_mismatches(g, c, twin) == [], cells[c]
    if c == 14:          # the comparison bites: one reason flipped, or one bit of one selected speed, and it reports it
        for q, row, flip in (("reason", 7, lambda a: a ^ 1), ("selected_speed", 200, lambda a: (a.view(np.int64) ^ 1).view(np.float64))):
            h = dict(g, **{q: g[q].copy()})
            h[q][c, row:row + 1] = flip(h[q][c, row:row + 1])
            assert twin_mismatches(h, c, twin) == [q]
