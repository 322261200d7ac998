"""CPU-only: which translation units build.py compiles again, from made-up modification times (nothing is compiled, no file is touched)."""
import rl_mpc_lanemerging_amd as pkg

build = pkg.build
UNITS = ["stmpc_solver", "stmpc_env", "stmpc_learner", build.CORE_UNIT]
HOST, KERNELS, ENV_K, DDPG_K, STMPC_H = "csrc/stmpc_host.hpp", "csrc/stmpc_kernels.hpp", "csrc/stmpc_env_kernels.hpp", "csrc/stmpc_ddpg_kernels.hpp", "include/stmpc.h"
# (a made-up include graph: the learner does not see stmpc_kernels.hpp here, so that "every unit that includes it" is not "every unit")
DEPS = {
    "stmpc_solver": ["csrc/stmpc_solver.hip", HOST, KERNELS, STMPC_H],
    "stmpc_env": ["csrc/stmpc_env.hip", HOST, KERNELS, ENV_K, STMPC_H],
    "stmpc_learner": ["csrc/stmpc_learner.hip", DDPG_K, STMPC_H],
    build.CORE_UNIT: ["csrc/stmpc.hip", HOST, STMPC_H],
}
BUILT = 100.0                                   # every object's modification time; every source is older


def _stale(edited=(), objects=None):
    mtimes = {f: 50.0 for fs in DEPS.values() for f in fs}
    mtimes.update({f: 200.0 for f in edited})
    return build.stale_units(DEPS, mtimes, objects or {u: BUILT for u in UNITS})


def test_stale_units_from_modification_times():
    assert _stale() == []                                                                   # nothing edited: nothing is compiled
    assert sorted(_stale(["csrc/stmpc_env.hip"])) == sorted(["stmpc_env", build.CORE_UNIT])        # the env unit, and the core for its src= stamp
    assert sorted(_stale([KERNELS])) == sorted(["stmpc_solver", "stmpc_env", build.CORE_UNIT])      # every unit that includes it (+ the core), not the learner
    assert sorted(_stale([STMPC_H])) == sorted(UNITS)                                               # the public header: everything
    # a unit without an object, or whose file list is not known, is compiled (and the core with it)
    assert sorted(_stale(objects={**{u: BUILT for u in UNITS}, "stmpc_learner": None})) == sorted(["stmpc_learner", build.CORE_UNIT])
    assert sorted(build.stale_units({**DEPS, "stmpc_env": None}, {f: 50.0 for fs in DEPS.values() for f in fs}, {u: BUILT for u in UNITS})) == \
        sorted(["stmpc_env", build.CORE_UNIT])


def test_every_unit_has_a_source_and_the_core_is_one_of_them():
    import os
    assert build.CORE_UNIT in build.UNITS and len(set(build.UNITS)) == len(build.UNITS)
    assert sorted(u + ".hip" for u in build.UNITS) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
