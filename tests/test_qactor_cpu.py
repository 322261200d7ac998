"""The DQN policy (``actor.DQNActor``, ``actor.q_policy_host``, the stmpc_qactor_ entries) without a GPU: header, library and binding agree; the
host twin against ``torch.nn.Linear`` + ``argmax`` in float64; first-maximum ties; rows whose Q are all negative; acceleration mode's formula at
both clip edges and inside; the refusals that need no device."""
import ctypes
import types

import numpy as np
import pytest

from discrete_testlib import NETS, NETS_WIDE, Q_WIDE_ROWS, Q_WIDE_VARIANTS, actor_table, q_dyadic_policy, tie_groups, tied_rows
from stmpc_testlib import capi as _capi, header_entries, header_prototypes, header_text

ROWS = 400
SEED = 3                        # test_q_policy_host_against_torch_modules asserts that at least 99 % of this seed's rows have a top-two gap above 1e-9


def _net(rng, n_obs, h1, A):
    from rl_mpc_lanemerging_amd import learner
    return learner.init_q_net(n_obs, h1, A, rng)


def test_header_library_and_binding_agree_on_the_q_actor():
    capi = _capi()
    lib = capi.load()
    declared = header_entries("stmpc_qactor_")
    assert declared == {"stmpc_qactor_" + n for n in ("create", "view_dqn", "destroy", "set_limits", "eval_device")}
    assert declared == {n for n in capi.EXPORTS if n.startswith("stmpc_qactor_")}
    assert header_entries("stmpc_") - {"stmpc_params", "stmpc_stats", "stmpc_ctx"} == set(capi.EXPORTS)
    protos = header_prototypes("stmpc_qactor_")
    assert set(protos) == declared
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == protos[name].count(",") + 1, name
    flat = header_text(flat=True)
    for mode, code in capi.QACTOR_MODES.items():
        assert "#define STMPC_QACTOR_%s %d" % (mode.upper(), code) in flat
    # every entry names the reference's function it stands for
    doc = flat[flat.index("A Q-network as the policy"):flat.index("#define STMPC_QACTOR_JERK")]
    for name in ("create", "view_dqn", "eval_device"):
        at = doc.index("stmpc_qactor_" + name + " ")
        assert "dqn.py:375-380" in doc[at:at + 120], name
    assert "#define STMPC_ABI_VERSION 8" in flat and capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8


@pytest.mark.parametrize("shape", NETS)
def test_q_policy_host_against_torch_modules(shape):
    """Q equals nn.Sequential(Linear, ReLU, Linear) in float64 to 1e-12 relative; the index equals torch.argmax on every row whose top-two gap
    exceeds 1e-9 (at least 99 % of the rows); the jerk is the table's entry."""
    _capi()
    import torch
    from torch import nn
    from rl_mpc_lanemerging_amd import actor
    n_obs, h1, A = shape
    rng = np.random.default_rng(SEED)
    net = _net(rng, n_obs, h1, A)
    feat = rng.normal(0, 1, (ROWS, n_obs)).astype(np.float32)
    table = np.linspace(-3.0, 3.0, A)
    m = nn.Sequential(nn.Linear(n_obs, h1), nn.ReLU(), nn.Linear(h1, A)).double()
    with torch.no_grad():
        for p, k in zip(m.parameters(), ("w0", "b0", "w1", "b1")):
            p.copy_(torch.tensor(net[k], dtype=torch.float64))
        want = m(torch.tensor(feat, dtype=torch.float64))
        want_idx = torch.argmax(want, 1).numpy()
    q, idx, jerk = actor.q_policy_host(net, feat, table, "jerk")
    assert q.dtype == np.float64 and q.shape == (ROWS, A) and idx.shape == (ROWS,) and jerk.dtype == np.float64
    assert np.abs(q - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()
    top = np.sort(want.numpy(), 1)
    clear = top[:, -1] - top[:, -2] > 1e-9
    assert clear.mean() >= 0.99, clear.mean()
    assert np.array_equal(idx[clear], want_idx[clear])
    assert np.array_equal(jerk, table[idx]) and len(set(idx.tolist())) > 1
    q32, idx32, _ = actor.q_policy_host(net, feat, table, "jerk", dtype=np.float32)
    assert q32.dtype == np.float32 and (idx32 == idx).mean() > 0.9


def test_ties_take_the_first_maximum():
    _capi()
    from rl_mpc_lanemerging_amd import actor
    A = 7
    net = {"w0": np.zeros((4, 3), np.float32), "b0": np.ones(4, np.float32), "w1": np.zeros((A, 4), np.float32), "b1": np.array([0, 2, 1, 2, -1, 2, 0], np.float32)}
    q, idx, jerk = actor.q_policy_host(net, np.zeros((5, 3), np.float32), np.arange(A) * 0.5, "jerk")
    assert np.array_equal(q[0], net["b1"].astype(np.float64)) and np.array_equal(idx, np.full(5, 1)) and np.array_equal(jerk, np.full(5, 0.5))
    net["b1"][:] = -3.0                                             # every action ties
    assert np.array_equal(actor.q_policy_host(net, np.zeros((5, 3), np.float32), np.arange(A), "jerk")[1], np.zeros(5, np.int64))


def test_all_negative_rows_never_return_a_pad_index():
    """A = 5 and 20 are padded to 16 and 32 columns on the device, whose pad Q are 0: the twin has no pad, and its index on a row whose Q are all
    negative is a real action's (the GPU suite compares the kernel with it on such rows)."""
    _capi()
    from rl_mpc_lanemerging_amd import actor
    rng = np.random.default_rng(SEED)
    for n_obs, h1, A in NETS:
        net = _net(rng, n_obs, h1, A)
        net["b1"] = net["b1"] - np.float32(10.0)
        q, idx, jerk = actor.q_policy_host(net, rng.normal(0, 1, (64, n_obs)).astype(np.float32), np.arange(A, dtype=np.float64), "jerk")
        assert (q < 0).all() and idx.min() >= 0 and idx.max() < A and np.array_equal(jerk, idx.astype(np.float64))
        assert np.array_equal(q[np.arange(64), idx], q.max(1))


@pytest.mark.parametrize("variant", Q_WIDE_VARIANTS)
@pytest.mark.parametrize("shape", NETS_WIDE)
def test_wide_dyadic_policies_cannot_pass_vacuously(shape, variant):
    """``q_dyadic_policy`` beyond 32 actions, from the float64 twin alone: Q is exact in float32 (the float32 twin equals the float64 one value for
    value), rows with only negative Q and rows without; "ties": every group of ``tie_groups`` holds the maximum on rows where no lower column ties,
    and the twin's index there is the group's lowest column; "lone": columns 32 and A - 1 are the twin's index on rows; the table has A distinct
    values."""
    _capi()
    from rl_mpc_lanemerging_amd import actor
    A = shape[2]
    net, S, states, feat, groups, named = q_dyadic_policy(shape, variant)
    table = actor_table(A)
    q, idx, jerk = actor.q_policy_host(net, feat, table, "jerk")
    q32, idx32, _ = actor.q_policy_host(net, feat, table, "jerk", dtype=np.float32)
    assert feat.shape == (Q_WIDE_ROWS, shape[0]) and np.array_equal(q32.astype(np.float64), q) and np.array_equal(idx32, idx) and np.array_equal(jerk, table[idx])
    allneg = (q < 0).all(1)
    assert allneg.any() and not allneg.all() and len(set(table.tolist())) == A and idx.max() < A
    assert set(groups) == (set(tie_groups(A)) if variant == "ties" else {"32", "A - 1"})
    tied = tied_rows(q, groups)
    print(shape, variant, {k: (tied[k].size, named[k].size) for k in groups}, "all negative", int(allneg.sum()))
    for name, cols in groups.items():
        assert named[name].size >= 1 and (idx[named[name]] == cols[0]).all() and (idx[tied[name]] <= cols[0]).all(), name
        assert all(np.array_equal(net["w1"][c], net["w1"][cols[0]]) and net["b1"][c] == net["b1"][cols[0]] for c in cols)
    if variant == "lone":
        assert (idx == 32).any() and (idx == A - 1).any()


def test_acceleration_mode_formula():
    """jerk = clip((table[a] - ego acceleration) / TICK_LENGTH, MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK): inside, at and beyond both edges."""
    _capi()
    from rl_mpc_lanemerging_amd import actor
    S = types.SimpleNamespace(TICK_LENGTH=0.25, MINIMUM_NEGATIVE_JERK=-4.0, MAXIMUM_POSITIVE_JERK=2.0)
    # one action per row: b1 puts the maximum at column r
    A = 6
    net = {"w0": np.zeros((2, 3), np.float32), "b0": np.zeros(2, np.float32), "w1": np.zeros((A, 2), np.float32), "b1": np.zeros(A, np.float32)}
    table = np.array([-1.5, -1.0, 0.0, 0.25, 0.5, 1.0])
    for a in range(A):
        net["b1"][:] = 0
        net["b1"][a] = 1
        acc = np.array([table[a], table[a] - 0.25, table[a] + 0.5, table[a] - 0.5, table[a] + 1.0, table[a] - 0.75, table[a] + 1.25, 3.0, -3.0])
        q, idx, jerk = actor.q_policy_host(net, np.zeros((acc.size, 3), np.float32), table, "acceleration", ego_acc=acc, S=S)
        assert (idx == a).all()
        raw = (table[a] - acc) / 0.25
        assert np.array_equal(jerk, np.minimum(np.maximum(raw, -4.0), 2.0))
        assert jerk[3] == 2.0 and raw[3] == 2.0 and jerk[4] == -4.0 and raw[4] == -4.0        # exactly at the edges
        assert jerk[5] == 2.0 and raw[5] == 3.0 and jerk[6] == -4.0 and raw[6] == -5.0        # beyond them
        inside = (raw > -4.0) & (raw < 2.0)
        assert inside[:3].all() and np.array_equal(jerk[:3], [0.0, 1.0, -2.0]) and np.array_equal(jerk[inside], raw[inside])
    # jerk mode ignores the acceleration; the package's Settings are the default
    assert np.array_equal(actor.q_policy_host(net, np.zeros((2, 3), np.float32), table, "jerk", ego_acc=np.array([9.0, -9.0]))[2], table[[A - 1, A - 1]])
    from rl_mpc_lanemerging_amd import Settings
    j = actor.q_policy_host(net, np.zeros((1, 3), np.float32), table, "acceleration", ego_acc=np.array([0.75]))[2]
    assert j[0] == min(max((1.0 - 0.75) / Settings.TICK_LENGTH, Settings.MINIMUM_NEGATIVE_JERK), Settings.MAXIMUM_POSITIVE_JERK)


def test_python_side_refusals(tmp_path):
    _capi()
    from rl_mpc_lanemerging_amd import Settings, actor, learner
    net = _net(np.random.default_rng(0), 20, 16, 5)
    feat = np.zeros((3, 20), np.float32)
    with pytest.raises(ValueError, match="mode"):
        actor.q_policy_host(net, feat, np.arange(5.0), "speed")
    with pytest.raises(ValueError, match="action table"):
        actor.q_policy_host(net, feat, np.arange(4.0), "jerk")
    with pytest.raises(ValueError, match="ego_acc"):
        actor.q_policy_host(net, feat, np.arange(5.0), "acceleration")
    fake = types.SimpleNamespace(cfg=learner.DQNConfig(n_obs=20, n_actions=5, h1=16), action_values=np.arange(5.0), handle=None)
    with pytest.raises(ValueError, match="mode"):
        actor.DQNActor.from_learner(fake, 4, None, Settings, mode="speed")
    with pytest.raises(ValueError, match="positive"):
        actor.DQNActor.from_learner(fake, 0, None, Settings)
    fake.action_values = np.array([0.0, 1.0, np.inf, 2.0, 3.0])
    with pytest.raises(ValueError, match="finite"):
        actor.DQNActor.from_learner(fake, 4, None, Settings)
    fake.action_values = np.arange(4.0)
    with pytest.raises(ValueError, match="action table"):
        actor.DQNActor.from_learner(fake, 4, None, Settings)
    fake.action_values, fake.cfg = np.arange(5.0), learner.DQNConfig(n_obs=19, n_actions=5, h1=16)
    with pytest.raises(ValueError, match="inputs"):
        actor.DQNActor.from_learner(fake, 4, None, Settings)
    # a file: the table comes from it unless one is given
    path = tmp_path / "q.npz"
    np.savez(path, **net, action_values=np.arange(5.0))
    with pytest.raises(ValueError, match="action table"):
        actor.DQNActor(path, 4, None, Settings, action_values=np.arange(6.0))
    with pytest.raises(ValueError, match="mode"):
        actor.DQNActor(path, 4, None, Settings, mode="accel")
    # the other consumers: a population keeps refusing what is no DDPG actor; the evaluation names its controllers
    with pytest.raises(ValueError, match="'combined' or 'first_step'"):
        learner.evaluate_dqn(str(path), 4, controller="st")
    assert actor.DQNActor.MODES == ("jerk", "acceleration")


def test_library_refusals_that_need_no_device():
    capi = _capi()
    lib, h = capi.load(), ctypes.c_void_p()
    null = ctypes.c_void_p()
    fcfg = capi.FeaturesCfg.from_settings(__import__("rl_mpc_lanemerging_amd").Settings, time_feature=False)
    fp, dp = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_double)()
    for rc in (lib.stmpc_qactor_create(null, 20, 16, 5, fp, fp, fp, fp, dp, 0, ctypes.byref(h)),
               lib.stmpc_qactor_view_dqn(null, 0, dp, 5, 0, ctypes.byref(h)),
               lib.stmpc_qactor_set_limits(null, 0.2, -1.0, 1.0),
               lib.stmpc_qactor_eval_device(null, null, ctypes.byref(fcfg), 4, 8, 1, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0, 0)):
        assert rc != 0 and b"NULL" in lib.stmpc_last_error()
    lib.stmpc_qactor_destroy(null)                                  # (a NULL handle is nothing to destroy)
