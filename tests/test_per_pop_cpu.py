"""Prioritised replay for the DDPG / TD3 populations (``DDPGPopulation(per=)``, ``TD3Population(per=)``, csrc/stmpc_per_pop_kernels.hpp, stmpc_pop_per_* of
include/stmpc.h): CPU part.

  * header, library and binding agree on the two new entries and their argument counts; the ABI is still 8 and no cfg struct grew;
  * both entries refuse NULL before they touch a device;
  * ``per=`` is validated before the env is looked at.
The GPU part is test_per_pop.py.
"""
import ctypes

import pytest

from stmpc_testlib import capi as _capi, header_prototypes, header_text

ENTRIES = {"stmpc_pop_per_enable_ddpg", "stmpc_pop_per_enable_td3"}


def test_header_library_and_binding_agree_on_population_prioritised_replay():
    capi = _capi()
    lib = capi.load()
    header = header_text(flat=True)
    declared = header_prototypes("stmpc_pop_per_")
    assert set(declared) == ENTRIES == {n for n in capi.EXPORTS if n.startswith("stmpc_pop_per_")}
    for name, args in declared.items():
        fn = getattr(lib, name)                                   # (AttributeError: the library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args.split(",")) == 4, name
        assert fn.argtypes[1]._type_ is capi.PERCfg and fn.argtypes[2]._type_ is ctypes.c_uint8 and fn.argtypes[3] is ctypes.c_int, name
    # the lone entries' closed set did not grow, and neither did a struct: the trees are enabled on the handle
    assert {n for n in capi.EXPORTS if n.startswith("stmpc_per_")} == {"stmpc_per_enable", "stmpc_per_tree_read", "stmpc_per_last_device", "stmpc_per_sample_index"}
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8 and "#define STMPC_ABI_VERSION 8" in header
    assert ctypes.sizeof(capi.PERCfg) == 32 and ctypes.sizeof(capi.DDPGCfg) == 24 + 8 * 13 and ctypes.sizeof(capi.TD3Cfg) == ctypes.sizeof(capi.DDPGCfg) + 24


def test_entries_refuse_null_before_touching_a_device():
    capi = _capi()
    lib = capi.load()
    good = (capi.PERCfg * 2)(*[capi.PERCfg(alpha=0.5, beta=0.0, min_priority=1e-6, max_priority=4.0)] * 2)
    on = (ctypes.c_uint8 * 2)(1, 1)
    for fn in (lib.stmpc_pop_per_enable_ddpg, lib.stmpc_pop_per_enable_td3):
        assert fn(None, good, on, 2) == capi.STMPC_EINVAL
        assert fn(None, None, None, 0) == capi.STMPC_EINVAL


class _Reached(Exception):
    pass


class _Env:
    """An env whose first attribute the constructor asks for says that the argument checks are over."""
    @property
    def continuous(self):
        raise _Reached()


def test_per_argument_is_validated_before_the_env_is_looked_at():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    per = learner.PERConfig(alpha=1.0, beta=0.4)
    for Pop, Cfg in ((learner.DDPGPopulation, learner.DDPGConfig), (learner.TD3Population, learner.TD3Config)):
        cfgs = [Cfg(n_obs=20), Cfg(n_obs=20), Cfg(n_obs=20)]
        for bad in ([per, per], [per] * 4, []):
            with pytest.raises(ValueError, match="per has %d entries, the population 3 members" % len(bad)):
                Pop(None, cfgs, per=bad)
        for bad in ([per, {"alpha": 0.5}, None], [per, 0.5, per], [True, None, None]):
            with pytest.raises(ValueError, match=r"per\[[01]\] is a \w+, not a PERConfig or None"):
                Pop(None, cfgs, per=bad)
        for bad in ({"alpha": 0.5}, 0.5, "per"):
            with pytest.raises(ValueError, match="per must be None, a PERConfig, or a list"):
                Pop(None, cfgs, per=bad)
        # on a member's cfg it stays refused, and the message says where it goes instead
        with pytest.raises(ValueError, match="prioritised.*per= argument"):
            Pop(None, [Cfg(n_obs=20), Cfg(n_obs=20, per=per)])
        with pytest.raises(ValueError, match="prioritised"):
            Pop(None, (Cfg(n_obs=20, per=per), 3), per=per)
        # what is valid gets as far as the env: None, one PERConfig, a list with None in it, a tuple
        for ok in (None, per, [per, None, per], (None, None, per), [None] * 3):
            with pytest.raises(_Reached):
                Pop(_Env(), cfgs, per=ok)
        with pytest.raises(_Reached):
            Pop(_Env(), (Cfg(n_obs=20), 2), per=[None, per])
