#!/usr/bin/env python3
"""The cells of the reference's combined-controller grid search, as a fixture (tests/golden/combined_grid.json).

Needs a checkout of the reference.  What runs is the reference's own ``main.do_grid_search_combined`` (main.py:62-81), unmodified, with
``main.do_task`` replaced by a recorder of the three settings the search writes: the fixture is the list of cells the search would have run,
in its order -- settings only.  Libraries the reference imports that are absent here (its RL library, gym, SUMO's TraCI, cvxopt, tensorboard)
are inert stand-ins, as in make_golden_combined_real.py: nothing of them is called on this path.

Re-run:  python tests/golden/make_combined_grid.py <reference checkout>
"""
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("ROLLOUT_LENGTH", "ST_TEST_ROLLOUTS", "TEST_ROLLOUT_STATE")


class _InertMeta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Inert

    def __getitem__(cls, key):
        return _Inert

    def __setitem__(cls, key, value):
        pass


class _Inert(metaclass=_InertMeta):
    """Stands for any class, function or object of an absent library: subclassable, callable, never does anything."""

    def __init__(self, *a, **kw):
        pass

    def __call__(self, *a, **kw):
        return _Inert()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Inert

    def __getitem__(self, key):
        return _Inert

    def __setitem__(self, key, value):
        pass


ABSENT = ("all", "gym", "traci", "sumolib", "cvxopt", "st_cy")      # st_cy: the reference's Cython extension, not built for this


class _InertFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Last on sys.meta_path: a module of an absent library that nobody else can find becomes an inert package."""

    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] not in ABSENT:
            return None
        return importlib.machinery.ModuleSpec(fullname, self, is_package=True)

    def create_module(self, spec):
        m = types.ModuleType(spec.name)
        m.__path__ = []
        m.__getattr__ = lambda name: _Inert if not name.startswith("__") else (_ for _ in ()).throw(AttributeError(name))
        return m

    def exec_module(self, module):
        pass


def main(ref):
    os.environ.setdefault("SUMO_HOME", ref)
    os.environ["MPLBACKEND"] = "Agg"
    sys.path.insert(0, ref)
    sys.meta_path.append(_InertFinder())
    tb = types.ModuleType("torch.utils.tensorboard")          # (as make_golden_combined_real.py)
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    import main as ref_main                                   # the reference's
    from config import Settings
    cells = []
    ref_main.do_task = lambda: cells.append({k: getattr(Settings, k) for k in KEYS})
    ref_main.do_grid_search_combined()
    out = {"source": "main.do_grid_search_combined (main.py:62-81), do_task replaced by a recorder", "keys": list(KEYS),
           "cells": [{k: (bool(c[k]) if isinstance(c[k], bool) else int(c[k])) for k in KEYS} for c in cells]}
    with open(os.path.join(HERE, "combined_grid.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%d cells" % len(cells))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
