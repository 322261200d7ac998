"""The suite's own structure: no test module imports another (what two of them share is in stmpc_testlib.py or learner_testlib.py), the helpers that
were once copied from module to module are defined in no test module again, and the shared comparators still bite."""
import ast
import glob
import os

import numpy as np

from learner_testlib import FLOOR, bits64, bits_equal, check_4x
from stmpc_testlib import REPO, bits, same

SHARED_ONLY = {"_capi", "_rel_err", "_check_4x", "_record"}


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
