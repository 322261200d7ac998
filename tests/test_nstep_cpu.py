"""Multi-step returns, on the CPU: the host twin of the window (learner.nstep_window_host) against an independent formulation from per-env episode
lists, its n = 1 identity, and the configs' checks."""
import ctypes

import numpy as np
import pytest

import nstep_testlib as nt
from stmpc_testlib import capi as _capi, header_entries, header_text

NS = (1, 2, 3, 5, 16)
STATES = [(20, 9), (21, 9), (20, 4), (21, 10)]                      # (capacity, pushes): wrapped and not a multiple of 3; a multiple of 3; partly filled; one push further


def _learner():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    return learner


def test_twin_against_the_episode_lists():
    learner = _learner()
    seen = set()
    for capacity, pushes in STATES:
        rows, cursor, fill = nt.ring_host(pushes, capacity)
        seen.add("full ring" if fill == capacity else "partly filled ring")
        for n in NS:
            want = nt.textbook(pushes, capacity, n)
            assert sorted(want) == list(range(fill))                # every live row, and no other
            for i, (R, disc, last, m, why) in want.items():
                got = learner.nstep_window_host(rows, i, cursor, fill, nt.N_ENVS, n, nt.GAMMA)
                assert (got[0].view(np.uint32), got[1].view(np.uint32), got[2], got[3]) == (R.view(np.uint32), disc.view(np.uint32), last, m), (capacity, pushes, n, i, got, want[i])
                assert got[0].dtype == got[1].dtype == np.float32
                if n > 1:
                    seen.add(why)
                    if nt.wraps(i, last, capacity):
                        seen.add("crosses the wrap")
    assert seen == {"term", "trunc", "newest", "full", "crosses the wrap", "full ring", "partly filled ring"}, seen


def test_the_trajectory_has_the_episodes_it_says():
    done0 = [bool(t[0][0] or t[1][0]) for t in map(nt.step_flags, range(10))]
    assert done0 == [False, True, False, False, False, False, True, True, False, True]
    assert nt.step_flags(6)[1][0] and nt.step_flags(1)[0][0] and nt.step_flags(7)[0][0]     # truncated, terminated, terminated
    assert not any(nt.step_flags(p)[0][1] or nt.step_flags(p)[1][1] for p in range(10))
    assert all(nt.step_flags(p)[0][2] or nt.step_flags(p)[1][2] for p in range(10))


def test_n_1_is_the_one_step_target():
    learner = _learner()
    for capacity, pushes in STATES:
        rows, cursor, fill = nt.ring_host(pushes, capacity)
        for gamma in (0.9, 0.99, 0.999):
            for i in range(fill):
                R, disc, last, m = learner.nstep_window_host(rows, i, cursor, fill, nt.N_ENVS, 1, gamma)
                assert R.view(np.uint32) == rows[i, 64].view(np.uint32) and disc.view(np.uint32) == np.float32(gamma).view(np.uint32) and (last, m) == (i, 1)
    rows[0, 64] = -0.0                                              # the sign of a zero reward survives
    assert learner.nstep_window_host(rows, 0, cursor, fill, nt.N_ENVS, 1, 0.9)[0].view(np.uint32) == np.float32(-0.0).view(np.uint32)


def test_batch_twin_takes_s2_and_mask_from_the_last_row():
    learner = _learner()
    rows, cursor, fill = nt.ring_host(9, 20)
    rows[:, 32:52] = np.arange(20, dtype=np.float32)[:, None]       # s' of ring row i is i
    idx = np.arange(fill)
    for dqn in (False, True):
        b = learner.nstep_batch_host(rows, idx, cursor, fill, nt.N_ENVS, 3, nt.GAMMA, 20, dqn=dqn)
        want = nt.textbook(9, 20, 3)
        assert np.array_equal(b["last"], [want[i][2] for i in idx]) and np.array_equal(b["m"], [want[i][3] for i in idx])
        assert np.array_equal(b["s2"][:, 0], b["last"]) and np.array_equal(b["mask"], rows[b["last"], 65])
        assert np.array_equal(b["r"].view(np.uint32), np.array([want[i][0] for i in idx]).view(np.uint32))
        assert np.array_equal(b["disc"].view(np.uint32), np.array([want[i][1] for i in idx]).view(np.uint32))
        assert np.array_equal(b["s"], rows[idx, :b["s"].shape[1]])


def test_configs_check_and_carry_n_step():
    learner = _learner()
    capi = _capi()
    for Cfg in (learner.DDPGConfig, learner.TD3Config, learner.DQNConfig):
        assert Cfg().n_step == 1
        for bad in (0, -1, 17):
            with pytest.raises(ValueError):
                Cfg(n_step=bad)
        c = Cfg(n_step=16, capacity=48)
        g = c.to_c_nstep(3)
        assert isinstance(g, capi.NStepCfg) and (g.n_step, g.rows_per_push) == (16, 3)
        with pytest.raises(ValueError):
            Cfg(n_step=16, capacity=47).to_c_nstep(3)               # n_step * N > capacity
        with pytest.raises(ValueError):
            Cfg(n_step=2).to_c_nstep(None)                          # no N
        one = Cfg(n_step=1, capacity=2).to_c_nstep(7)
        assert (one.n_step, one.rows_per_push) == (1, 0)
    # the three cfg structs keep their layout: n_step travels in a struct of its own
    assert ctypes.sizeof(capi.NStepCfg) == 8 and [n for n, _ in capi.NStepCfg._fields_] == ["n_step", "rows_per_push"]
    assert capi.NSTEP_MAX == 16 and "#define STMPC_NSTEP_MAX 16" in header_text(flat=True)


def test_header_library_and_binding_agree_on_the_entries():
    capi = _capi()
    lib = capi.load()
    declared = header_entries("stmpc_nstep_") | header_entries("stmpc_pop_nstep_")
    assert declared == {"stmpc_nstep_enable_ddpg", "stmpc_nstep_enable_dqn", "stmpc_nstep_window_ddpg", "stmpc_nstep_window_dqn",
                        "stmpc_pop_nstep_enable_ddpg", "stmpc_pop_nstep_enable_td3", "stmpc_pop_nstep_enable_dqn"}
    assert declared == {n for n in capi.EXPORTS if "nstep" in n}
    for name in declared:
        assert getattr(lib, name).argtypes is not None, name
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8
