"""The DQN learner without a GPU: header, library and binding agree on the stmpc_dqn_ entries; the host twins (``learner.update_host_dqn``,
``dqn_targets_host``, ``dqn_epsilon``, ``dqn_act_host``) against the reference's own numbers (tests/golden/golden_dqn.npz, written by
make_golden_dqn.py from the reference's ``get_targets`` and its SmoothL1 + Adam step) and against torch autograd; the refusals.

The bound against the golden is the learner tests' rule for a float32 computation against its float64 twin: per tensor, in the max norm,
|golden - twin64| <= max(4 x |twin32 - twin64|, 8 float32 ulps) -- the reference computed in float32, ``update_host_dqn("float32")`` is the yardstick."""
import ctypes
import math
import types

import numpy as np
import pytest

from conftest import load_golden
from discrete_testlib import (WIDE_A, WIDE_DQN_SEEDS, _q64, dqn_exactness_bits, dqn_wide_counts, dqn_wide_counts_ok, dqn_wide_problem, minibatch_host, tie_groups,
                              tied_rows)
from learner_testlib import check_4x as _check_4x
from stmpc_testlib import capi as _capi, header_entries, header_struct_fields as _header_struct_fields, header_text

NAMES = ("w0", "b0", "w1", "b1")


def test_header_library_and_binding_agree_on_the_dqn_learner():
    capi = _capi()
    lib = capi.load()
    declared = header_entries("stmpc_dqn_")
    assert declared == {"stmpc_dqn_" + n for n in ("create", "destroy", "set_params", "get_params", "set_state", "get_state", "push_device", "act_device",
                                                    "update_device", "grads_device", "targets_device", "gather_device", "stats_device", "per_enable",
                                                    "per_tree_read", "per_last_device", "padded_read")}
    assert declared == {n for n in capi.EXPORTS if n.startswith("stmpc_dqn_")}
    all_declared = header_entries("stmpc_") - {"stmpc_params", "stmpc_stats", "stmpc_ctx"}
    assert all_declared == set(capi.EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None and getattr(lib, name).argtypes is not None, name
    flat = header_text(flat=True)
    for name, val in (("STMPC_DQN_Q", 0), ("STMPC_DQN_Q_V", len(capi.DQN_SLOTS) - 1), ("STMPC_DQN_GRAD", capi.DQN_GRAD), ("STMPC_DQN_Q_TARGET", capi.DQN_SLOTS.index("q_target")),
                      ("STMPC_ABI_VERSION", 8)):
        assert "#define %s %d" % (name, val) in flat, name
    assert capi.ABI_VERSION == 8 and lib.stmpc_abi_version() == 8


def test_dqn_cfg_struct_layout_matches_header():
    capi = _capi()
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    want = _header_struct_fields("stmpc_dqn_cfg")
    have = list(capi.DQNCfg._fields_)
    assert [n for n, _ in want] == [n for n, _ in have]
    assert [ctype_of[t] for _, t in want] == [t for _, t in have]
    assert ctypes.sizeof(capi.DQNCfg) == 8 * 4 + 8 + 8 + 6 * 8


def _golden_case():
    from rl_mpc_lanemerging_amd import learner
    g = load_golden("golden_dqn.npz")
    net = {k: g["q_" + k] for k in NAMES}
    params = learner.new_params_dqn(net)
    params["q_target"] = {k: g["t_" + k] for k in NAMES}
    batch = {"s": g["s"], "a": g["a"], "r": g["r"], "s2": g["s2"], "mask": g["mask"]}
    mk = lambda **kw: learner.DQNConfig(n_obs=g["s"].shape[1], n_actions=g["q_b1"].size, h1=g["q_b0"].size, batch=g["s"].shape[0], gamma=float(g["gamma"]),
                                        lr=float(g["lr"]), clip_min=float(g["clip"][0]), clip_max=float(g["clip"][1]), **kw)
    return g, params, batch, mk


def test_update_host_dqn_against_the_reference_golden():
    """Targets under DOUBLE_DQN True / False / with CLIP_TARGETS, the double-DQN argmax indices, q_values, the gradients and the weights after one
    Adam step: the reference's own values against ``update_host_dqn("float64")`` under the module text's bound."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    g, params, batch, mk = _golden_case()
    assert g["s"].shape == (50, 20) and int((g["mask"] == 0).sum()) >= 8
    assert learner.DQNConfig().h1 == g["q_b0"].size == 256 and learner.DQNConfig().batch == 50 and learner.DQNConfig().gamma == float(g["gamma"]) == 0.999
    assert learner.DQNConfig().lr == float(g["lr"]) == 2e-4 and learner.DQNConfig().target_period == 500 and learner.DQNConfig().capacity == 50000
    assert learner.DQNConfig().double and not learner.DQNConfig().clip_targets and learner.DQNConfig().per is None
    ok = True
    for key, kw in (("targets_double", dict(double=True)), ("targets_plain", dict(double=False)), ("targets_clip", dict(double=True, clip_targets=True))):
        t64, t32 = (learner.dqn_targets_host(params, batch, mk(**kw), d) for d in ("float64", "float32"))
        ok &= _check_4x(key, g[key], t32[:, 2], t64[:, 2])
        if key == "targets_double":
            live = g["mask"] > 0
            assert np.array_equal(t64[live, 0].astype(np.int64), g["best"][live]) and (g["best"][~live] == -1).all()
        if key == "targets_clip":                                   # the clip bites, on both sides
            gq = float(g["gamma"]) * t64[:, 1]
            assert (gq[g["mask"] > 0] > g["clip"][1]).any() and (gq[g["mask"] > 0] < g["clip"][0]).any()
    cfg = mk(double=True)
    (p64, i64), (p32, i32) = (learner.update_host_dqn(params, batch, cfg, d) for d in ("float64", "float32"))
    assert (np.abs(i64["td"]) > 1).any() and (np.abs(i64["td"]) < 1).any()      # both branches of the Huber loss
    ok &= _check_4x("q_values", g["q_values"], i32["q_values"], i64["q_values"])
    ok &= _check_4x("loss", g["loss"].reshape(1), np.array([i32["loss"]]), np.array([i64["loss"]]))
    for k in NAMES:
        ok &= _check_4x("grad " + k, g["g_" + k], i32["grad"][k], i64["grad"][k])
        ok &= _check_4x("after " + k, g["after_" + k], p32["q"][k], p64["q"][k])
        assert np.abs(g["after_" + k] - g["q_" + k]).max() > 0.5 * float(g["lr"])       # (the first Adam step moves a weight by about lr)
        assert np.array_equal(p64["q_target"][k], g["t_" + k])      # update 1 of 500: the target stays
    assert ok and p64["updates"] == 1


@pytest.mark.parametrize("double,clip", [(True, False), (False, False), (True, True)])
def test_update_host_dqn_against_torch_autograd(double, clip):
    """The twin's gradient against a second statement with nn.Linear modules, nn.SmoothL1Loss and loss.backward(): random data with rows in the linear
    branch of the Huber loss, importance weights and terminal rows; float64, 1e-12 relative.  Three steps with torch.optim.Adam follow the twin's."""
    _capi()
    import torch
    from torch import nn
    from rl_mpc_lanemerging_amd import learner
    rng = np.random.default_rng(5 + 2 * double + clip)
    n_obs, h1, A, B = 12, 24, 7, 33
    cfg = learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=B, gamma=0.9, lr=1e-3, target_period=2, double=double, clip_targets=clip, clip_min=-0.3,
                            clip_max=0.2)
    params = learner.new_params_dqn(learner.init_q_net(n_obs, h1, A, rng))
    params["q_target"] = learner.init_q_net(n_obs, h1, A, rng)
    mods = []
    for slot in ("q", "q_target"):
        m = nn.Sequential(nn.Linear(n_obs, h1), nn.ReLU(), nn.Linear(h1, A)).double()
        with torch.no_grad():
            for p, k in zip(m.parameters(), NAMES):
                p.copy_(torch.tensor(params[slot][k], dtype=torch.float64))
        mods.append(m)
    q, qt = mods
    opt = torch.optim.Adam(q.parameters(), lr=cfg.lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    for step in range(3):
        batch = {"s": rng.normal(size=(B, n_obs)), "s2": rng.normal(size=(B, n_obs)), "a": rng.integers(0, A, B), "r": rng.normal(size=B) * 2,
                 "mask": (rng.random(B) > 0.25).astype(np.float64)}
        w = rng.uniform(0.2, 1.0, B) if step != 1 else None
        assert (batch["mask"] == 0).any()
        new, info = learner.update_host_dqn(params, batch, cfg, "float64", weights=w)
        assert (np.abs(info["td"]) > 1).any() and (np.abs(info["td"]) < 1).any()
        T = lambda a: torch.tensor(a, dtype=torch.float64)
        with torch.no_grad():
            s2 = T(batch["s2"])
            nxt = torch.gather(qt(s2), 1, torch.argmax(q(s2), 1, keepdim=True)).flatten() if double else qt(s2).max(1)[0]
            gq = cfg.gamma * nxt
            if clip:
                gq = gq.clamp(cfg.clip_min, cfg.clip_max)
            y = T(batch["r"]) + T(batch["mask"]) * gq
        qv = torch.gather(q(T(batch["s"])), 1, torch.tensor(batch["a"])[:, None]).flatten()
        loss = nn.SmoothL1Loss()(qv, y) if w is None else (T(w) * nn.SmoothL1Loss(reduction="none")(qv, y)).mean()
        opt.zero_grad()
        loss.backward()
        assert np.abs(info["targets"][:, 2] - y.numpy()).max() <= 1e-12 * np.abs(y.numpy()).max()
        for p, k in zip(q.parameters(), NAMES):
            assert np.abs(info["grad"][k] - p.grad.numpy()).max() <= 1e-12 * np.abs(p.grad.numpy()).max(), (step, k)
        opt.step()
        if (step + 1) % cfg.target_period == 0:
            qt.load_state_dict(q.state_dict())
        for m, slot in ((q, "q"), (qt, "q_target")):
            for p, k in zip(m.parameters(), NAMES):
                assert np.abs(new[slot][k] - p.detach().numpy()).max() <= 1e-12 * np.abs(p.detach().numpy()).max(), (step, slot, k)
        assert np.array_equal(new["q_target"]["w1"], new["q"]["w1"]) == ((step + 1) % 2 == 0)
        params = new
    assert params["updates"] == 3 and np.allclose(params["beta_pow"], [0.9 ** 3, 0.999 ** 3])


@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("shape", WIDE_A["dqn"])
def test_wide_problems_cannot_pass_vacuously(shape, double):
    """``dqn_wide_problem`` at more than 32 actions, from the host twins alone: the counts the GPU tests rest on (``dqn_wide_counts_ok``: rows per tie
    group, all-negative rows, online != target rows, the clip bounds met and passed), every partial sum below 24 bits, the float32 and the float64
    twin equal value for value (targets, Q(s, a), every gradient), with and without clipping, and ``dqn_targets_host``'s a* the lowest column of
    each tie group."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    c = dqn_wide_counts(shape, double)
    print(shape, "double" if double else "plain", "seed", WIDE_DQN_SEEDS[shape, double], c)
    assert dqn_wide_counts_ok(shape, double, c), c
    n_obs, h1, A, B = shape
    assert B & (B - 1) == 0
    for clip in (True, False):
        cfg, params, replay, extra = dqn_wide_problem(shape, double, clip)
        _, batch = minibatch_host(replay, cfg)
        bits = dqn_exactness_bits(params, batch, cfg)
        assert max(bits.values()) < 24, bits
        (_, i64), (_, i32) = (learner.update_host_dqn(params, batch, cfg, d, grads_only=True) for d in ("float64", "float32"))
        assert i32["targets"].dtype == np.float32 and np.array_equal(i32["targets"].astype(np.float64), i64["targets"])
        assert np.array_equal(i32["q_values"].astype(np.float64), i64["q_values"]) and (np.abs(i64["td"]) > 1).any() and (batch["mask"] == 0).any()
        for k in NAMES:
            assert i32["grad"][k].dtype == np.float32 and np.array_equal(i32["grad"][k].astype(np.float64), i64["grad"][k]) and np.abs(i64["grad"][k]).max() > 0, k
        t = learner.dqn_targets_host(params, batch, cfg)
        for name, rows in tied_rows(_q64(params["q" if double else "q_target"], batch["s2"]), extra["groups"]).items():
            assert rows.size >= 4 and (t[rows, 0] == extra["groups"][name][0]).all(), (name, t[rows, 0])
        stored = set(int(a) for a in batch["a"])
        assert {31, 32, A - 1} <= stored and {a // 16 for a in stored} == set(range((A + 15) // 16))
        assert replay["a"].max() == A + 3 and replay["a"].min() == -2 and 0 <= batch["a"].min() and batch["a"].max() == A - 1
    assert set(tie_groups(A)) >= {"ends", "lanes", "strides"} and tie_groups(A)["strides"][1] - tie_groups(A)["strides"][0] == 32 and (A != 256 or len(tie_groups(A)["triple"]) == 3)


def test_wide_twin_gradient_against_torch_autograd():
    """The twin's gradient at (20, 32, 40, 16) against the second statement with nn.Linear modules, nn.SmoothL1Loss and loss.backward(): float64,
    1e-12 relative, double DQN with and without clipping and plain DQN."""
    _capi()
    import torch
    from torch import nn
    from rl_mpc_lanemerging_amd import learner
    shape = WIDE_A["dqn"][0]
    for double, clip in ((True, False), (False, False), (True, True)):
        cfg, params, replay, _ = dqn_wide_problem(shape, double, clip)
        _, batch = minibatch_host(replay, cfg)
        mods = []
        for slot in ("q", "q_target"):
            m = nn.Sequential(nn.Linear(shape[0], shape[1]), nn.ReLU(), nn.Linear(shape[1], shape[2])).double()
            with torch.no_grad():
                for p, k in zip(m.parameters(), NAMES):
                    p.copy_(torch.tensor(params[slot][k], dtype=torch.float64))
            mods.append(m)
        q, qt = mods
        T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        with torch.no_grad():
            s2 = T(batch["s2"])
            nxt = torch.gather(qt(s2), 1, torch.argmax(q(s2), 1, keepdim=True)).flatten() if double else qt(s2).max(1)[0]
            gq = cfg.gamma * nxt
            if clip:
                gq = gq.clamp(cfg.clip_min, cfg.clip_max)
            y = T(batch["r"]) + T(batch["mask"]) * gq
        qv = torch.gather(q(T(batch["s"])), 1, torch.tensor(batch["a"])[:, None]).flatten()
        nn.SmoothL1Loss()(qv, y).backward()
        _, info = learner.update_host_dqn(params, batch, cfg, "float64", grads_only=True)
        assert np.abs(info["targets"][:, 2] - y.numpy()).max() <= 1e-12 * np.abs(y.numpy()).max()
        for p, k in zip(q.parameters(), NAMES):
            assert np.abs(info["grad"][k] - p.grad.numpy()).max() <= 1e-12 * np.abs(p.grad.numpy()).max(), (double, clip, k)


def test_dqn_act_host_draws_beyond_one_stride():
    """A = 40, 64, 256: every index in range; at A = 40 every action is drawn over 4096 envs at eps = 1."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    for A in (40, 64, 256):
        ex, idx = learner.dqn_act_host(7, 0, 4096, 1.0, A)
        assert ex.all() and idx.min() >= 0 and idx.max() < A and idx.dtype == np.int32
        assert A != 40 or len(set(idx.tolist())) == 40
        exq, idxq = learner.dqn_act_host(7, 0, 256, 0.25, A)
        assert np.array_equal(idxq, idx[:256]) and 0 < exq.sum() < 256


def test_dqn_epsilon_is_the_references_decay():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    for it in (0, 29999, 30000, 300000):
        assert learner.dqn_epsilon(it) == 0.1 + (1.0 - 0.1) * np.exp(-0.25 * np.floor(it / 30000))     # dqn.py:275-276 with config.py's constants
    assert learner.dqn_epsilon(0) == learner.dqn_epsilon(29999) == 1.0 and learner.dqn_epsilon(30000) < 1.0
    assert abs(learner.dqn_epsilon(300000) - (0.1 + 0.9 * math.exp(-2.5))) < 1e-15


def test_dqn_act_host_draws():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    for A in (5, 20, 17):
        ex0, _ = learner.dqn_act_host(7, 0, 200, 0.0, A)
        ex1, idx1 = learner.dqn_act_host(7, 0, 200, 1.0, A)
        assert not ex0.any() and ex1.all() and idx1.min() >= 0 and idx1.max() == A - 1 and len(set(idx1.tolist())) == A
        exq, idxq = learner.dqn_act_host(7, 0, 200, 0.25, A)
        assert 20 < exq.sum() < 80 and np.array_equal(idxq, idx1)   # the index does not depend on eps
        assert not np.array_equal(learner.dqn_act_host(7, 1, 200, 0.25, A)[0], exq)      # the call number is part of the hash
    # u < eps in integer arithmetic: the draw's 24 bits against float32(eps) * 2^24
    h = learner.hash3(7 ^ learner.DQN_STREAM, 0, 3)
    u = (h >> 40) * 2.0 ** -24
    assert learner.dqn_act_host(7, 0, 4, float(np.nextafter(np.float32(u), np.float32(2))), 5)[0][3] and not learner.dqn_act_host(7, 0, 4, u, 5)[0][3]


def test_dqn_refusals():
    _capi()
    from rl_mpc_lanemerging_amd import learner
    with pytest.raises(ValueError, match="discrete"):
        learner.DQNLearner(types.SimpleNamespace(continuous=True, obs_dim=20))
    with pytest.raises(ValueError, match="n_actions"):
        learner.DQNLearner((20, 0))
    with pytest.raises(ValueError, match="n_obs"):
        learner.DQNLearner((32, 5), learner.DQNConfig(n_obs=32))
    with pytest.raises(ValueError, match="target_period"):
        learner.DQNLearner((20, 5), learner.DQNConfig(target_period=0))
    with pytest.raises(ValueError, match="PERConfig"):
        learner.DQNConfig(per=0.5)
    # ... and the library's own, on the host, before any device call
    capi = _capi()
    lib, h = capi.load(), ctypes.c_void_p()
    fake_ctx = ctypes.c_void_p()
    assert lib.stmpc_dqn_create(fake_ctx, ctypes.byref(learner.DQNConfig(n_actions=5).to_c(0)), ctypes.byref(h)) != 0      # NULL context
