"""The suite's own structure: no test module imports another (what two of them share is in stmpc_testlib.py, learner_testlib.py, discrete_testlib.py,
nstep_testlib.py or env_testlib.py), the helpers that were once copied from module to module are defined in no test module again, and the shared
comparators and env helpers still bite."""
import ast
import glob
import os

import numpy as np

from discrete_testlib import NAMES, Q_SLOTS, assert_same as discrete_assert_same
from env_testlib import episodes_of, hash01, log_rows
from learner_testlib import FLOOR, bits64, bits_equal, check_4x
from stmpc_testlib import REPO, bits, same

SHARED_ONLY = {"_capi", "_rel_err", "_check_4x", "_record", "_flat", "_hash01", "_log_rows", "_episodes",
               # the discrete agents' helpers (discrete_testlib.py, and episode_settings of stmpc_testlib.py).  Not listed: _same_slots -- test_td3_pop.py has
               # one of its own over the continuous learners' tensors, with another signature; _rows and _dev -- test_reward_groups.py and test_vec_env.py
               # use the names for other things
               "_snapshot", "_stats_row", "_assert_same", "_stub_env", "_feed", "_fill", "_pad_mask", "_pads_are_zero", "_twins", "_minibatch_host", "_widen",
               "_plain_policy", "_episode_settings", "_stream", "_states", "_features", "_act", "_transitions", "_expected_values_host"}


def test_no_test_module_imports_another_or_redefines_a_shared_helper():
    paths = sorted(glob.glob(os.path.join(REPO, "tests", "*.py")))
    assert len(paths) > 50
    for path in paths:
        name = os.path.basename(path)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            modules = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            for module in modules:
                assert not module.split(".")[-1].startswith("test_"), "%s:%d imports %s" % (name, node.lineno, module)
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and name.startswith("test_"):
                assert node.name not in SHARED_ONLY, "%s:%d defines %s" % (name, node.lineno, node.name)


def test_bit_comparisons_tell_signed_zeros_apart_and_accept_equal_nans():
    nan = np.float32(np.nan)
    for dtype in (np.float32, np.float64):
        zero, minus, nans = np.array([0.0, 1.0], dtype), np.array([-0.0, 1.0], dtype), np.array([np.nan, 1.0], dtype)
        assert np.array_equal(zero, minus) and not np.array_equal(bits(zero), bits(minus)) and not same(zero, minus)
        assert not np.array_equal(nans, nans) and np.array_equal(bits(nans), bits(nans.copy())) and same(nans, nans.copy())
        assert not np.array_equal(bits64(zero), bits64(minus)) and np.array_equal(bits64(nans), bits64(nans.copy()))
    a = {"q": {"w": np.array([0.0, nan], np.float32)}}
    assert bits_equal(a, {"q": {"w": np.array([0.0, nan], np.float32)}}, ("q",), ("w",))
    assert not bits_equal(a, {"q": {"w": np.array([-0.0, nan], np.float32)}}, ("q",), ("w",))


def test_discrete_assert_same_passes_on_equal_snapshots_and_fails_on_any_single_difference():
    """Two hand-made discrete snapshots (four slots x four tensors, beta_pow float32 [2], counters int64 [8], a ring, a four-entry statistics row): equal
    ones pass; one bit of one tensor, beta_pow, one counter, one ring entry, one statistics entry or the sign of a zero in a tensor fails."""
    import copy

    import pytest

    def snap():
        rng = np.random.default_rng(3)
        t = lambda *sh: rng.normal(size=sh).astype(np.float32)
        params = {slot: {"w0": t(4, 3), "b0": t(4), "w1": t(2, 4), "b1": t(2)} for slot in Q_SLOTS}
        params["q_m"]["b1"][0] = 0.0
        params["beta_pow"] = np.array([0.81, 0.998], np.float32)
        return {"params": params, "counters": np.arange(8, dtype=np.int64), "ring": t(5, 6), "stats": [0.5, -1.25, 5.0, 2.0]}

    def one_bit(a, i):
        a.view(np.uint32).reshape(-1)[i] ^= 1

    a = snap()
    assert set(a["params"]) == set(Q_SLOTS) | {"beta_pow"} and all(tuple(a["params"][s]) == NAMES for s in Q_SLOTS)
    discrete_assert_same(a, snap(), "equal")
    discrete_assert_same(a, copy.deepcopy(a), "a copy")
    changes = {"one bit of one tensor": lambda b: one_bit(b["params"]["q_v"]["w1"], 5), "beta_pow": lambda b: one_bit(b["params"]["beta_pow"], 1),
               "one counter": lambda b: b["counters"].__setitem__(6, 7), "one ring entry": lambda b: one_bit(b["ring"], 29),
               "one stats entry": lambda b: b["stats"].__setitem__(1, float(np.nextafter(-1.25, 0))),
               "+0.0 vs -0.0": lambda b: b["params"]["q_m"]["b1"].__setitem__(0, -0.0)}
    for what, change in changes.items():
        b = snap()
        change(b)
        with pytest.raises(AssertionError):
            discrete_assert_same(a, b, what)
        with pytest.raises(AssertionError):
            discrete_assert_same(b, a, what)
    assert a["params"]["q_m"]["b1"][0] == -0.0                      # (equal as numbers: only a comparison of bits tells the two zeros apart)


def test_check_4x_passes_at_its_bound_and_fails_just_above_it():
    """Against f64 = 1 the errors are the distances themselves; 1 + k / 1024 is exact, and so are the differences."""
    f64 = np.array([1.0, -0.5])
    at = lambda e: np.array([1.0 + e, -0.5])
    e32 = 2.0 ** -10                                              # 4 x e32 governs
    assert 4 * e32 > FLOOR
    ratios = {}
    assert check_4x("at the bound", at(4 * e32), at(e32), f64, ratios) and not check_4x("above it", at(4 * e32 + 2.0 ** -40), at(e32), f64, ratios)
    assert set(ratios) == {"at the bound", "above it"} and ratios["at the bound"] == {"device": 4 * e32, "float32_twin": e32, "ratio": 4.0}
    assert FLOOR == 8 * 2.0 ** -23                                 # the floor governs: an exact float32 twin
    assert check_4x("at the floor", at(FLOOR), f64, f64) and not check_4x("above the floor", at(FLOOR + 2.0 ** -40), f64, f64)
    assert check_4x("floor, small twin error", at(FLOOR), at(FLOOR / 8), f64) and not check_4x("floor, small twin error", at(FLOOR * 1.001), at(FLOOR / 8), f64)


def test_hash01_at_four_literal_pairs():
    """The values the env tests' copies of it gave before they became one: exact, every operation is on integers but the last division by 2^53."""
    want = {(0, 0): "0x1.c4415072f63b9p-1", (1, 0): "0x1.e87d761ce519bp-1", (95, 50): "0x1.4ae3b978a7500p-8", (71, 30): "0x1.de140a44df3c0p-4"}
    for (e, tick), value in want.items():
        assert hash01(e, tick) == float.fromhex(value), (e, tick)
    assert hash01(0, 0) == 0.8833108082136426


def test_episodes_of_cuts_a_hand_made_run_with_and_without_extra_keys():
    """2 rows x 5 ticks: row 0 ends an episode at tick 2 and another at tick 4 (the run's end), row 1 none.  obs[s, e] = 10 e + s + 1, obs0[e] = 10 e."""
    step, row = np.mgrid[0:5, 0:2]
    done = np.zeros((5, 2), bool)
    done[2, 0] = done[4, 0] = True
    run = {"obs0": np.array([0.0, 10.0]), "obs": 10.0 * row + step + 1, "done": done, "final_observation": 100.0 + step + 0 * row,
           "final_stats": 200.0 + step + 0 * row, "ticks": step + 0 * row, "reward": -1.0 * step + 0 * row, "terminated": done, "truncated": ~done,
           "takeover": step % 2 == 0}
    eps = episodes_of(run, 2)
    assert sorted(eps) == [(0, 0), (0, 1)]
    first, second = eps[(0, 0)], eps[(0, 1)]
    assert set(first) == {"start", "obs", "final_observation", "final_stats", "ticks", "end_step", "reward", "terminated", "truncated"}
    assert first["start"] == 0.0 and first["obs"].tolist() == [1.0, 2.0] and first["final_observation"] == 102.0 and first["final_stats"] == 202.0
    assert first["ticks"].tolist() == [0, 1] and first["end_step"] == 2 and first["reward"].tolist() == [0.0, -1.0, -2.0]
    assert first["terminated"].tolist() == [False, False, True] and first["truncated"].tolist() == [True, True, False]
    # the next episode starts from the observation the step that ended the first one returned
    assert second["start"] == 3.0 and second["obs"].tolist() == [4.0] and second["end_step"] == 4 and second["reward"].tolist() == [-3.0, -4.0]
    assert second["final_observation"] == 104.0 and second["ticks"].tolist() == [3]
    assert episodes_of(run, 1).keys() == eps.keys()                # (n: the rows looked at)
    extra = episodes_of(run, 2, ("takeover",))
    assert set(extra[(0, 0)]) == set(first) | {"takeover"} and extra[(0, 0)]["takeover"].tolist() == [True, False, True]
    assert extra[(0, 1)]["takeover"].tolist() == [False, True]
    assert all(np.array_equal(extra[key][k], eps[key][k]) for key in eps for k in eps[key])


def test_log_rows_keys_by_env_and_episode_and_ignores_the_traffic_type():
    log = {"env": np.array([3, 0]), "episode": np.array([1, 0]), "ticks": np.array([40, 45]), "episode_return": np.array([-1.5, 2.25]),
           "traffic_type": np.array([2, 1])}
    rows = log_rows(log)
    assert set(rows) == {(3, 1), (0, 0)}
    # the columns in sorted order: env, episode, episode_return, ticks
    assert rows[(3, 1)] == np.array([3, 1, -1.5, 40], np.float64).tobytes() and rows[(0, 0)] == np.array([0, 0, 2.25, 45], np.float64).tobytes()
    assert log_rows(dict(log, traffic_type=np.array([0, 0]))) == rows and log_rows({k: v for k, v in log.items() if k != "traffic_type"}) == rows
    assert log_rows(dict(log, ticks=np.array([41, 45])))[(3, 1)] != rows[(3, 1)]
