"""The dueling head of the C51 learner without a GPU (``learner.C51Config(dueling=True)``): the float64 twin against an independent torch module
with separate value and advantage heads; ``c51_fold_dueling_host``; the head's invariance under a shift of every advantage block; the float32
restatement of the device's combine; the config, the struct and the ``export_q`` key; and the properties of the GPU tests' problems that the twins
alone decide (tests/discrete_testlib.py).  Every test here needs ``C51Config`` to take ``dueling``."""
import ctypes
import types

import numpy as np
import pytest

from discrete_testlib import (C51_DUELING as HEAD, NAMES, PROBLEM_SEEDS as _PROBLEM_SEEDS, SHAPES as _SHAPES, WIDE_A as _WIDE_A, all_negative_rows, astar_rows, dueling_module, minibatch_host,
                              problem_net, random_problem, twins)
from stmpc_testlib import capi as _capi

SHAPES, PROBLEM_SEEDS = _SHAPES["c51_dueling"] + _WIDE_A["c51_dueling"], _PROBLEM_SEEDS["c51_dueling"]      # tests/discrete_testlib.py's tables; the last index is the head's shape of WIDE_A

def _problem(seed, double=True, shape=(12, 24, 4, 11, 33)):
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, K, B = shape
    rng = np.random.default_rng(seed)
    cfg = learner.C51Config(n_obs=n_obs, n_actions=A, h1=h1, batch=B, gamma=0.9, lr=1e-3, double=double, n_atoms=K, v_min=-4.0, v_max=3.0, dueling=True)
    params = learner.new_params_dqn(problem_net(HEAD, shape, rng))
    params["q_target"] = problem_net(HEAD, shape, rng)
    batch = {"s": rng.normal(size=(B, n_obs)), "s2": rng.normal(size=(B, n_obs)), "a": rng.integers(0, A, B), "r": rng.normal(size=B) * 2,
             "mask": (rng.random(B) > 0.25).astype(np.float64)}
    return cfg, params, batch


@pytest.mark.parametrize("double", [True, False])
def test_twin_against_separate_value_and_advantage_heads(double):
    _against_separate_heads(double, (12, 24, 4, 11, 33))


@pytest.mark.parametrize("double", [True, False])
def test_twin_against_separate_value_and_advantage_heads_at_63_actions(double):
    """The same statement at WIDE_A's shape: (A + 1) K = 1024, an odd A in the mean's division."""
    _against_separate_heads(double, _WIDE_A["c51_dueling"][0])


def _against_separate_heads(double, shape):
    """update_host_c51(dueling=True) in float64 against a torch module with a value nn.Linear and an advantage nn.Linear carrying the same weights,
    the projection written the textbook way: loss, row losses, m, p and all four gradients to 1e-12 relative; importance weights on one pass."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    cfg, params, batch = _problem(21 + double, double, shape)
    A, K, B = cfg.n_actions, cfg.n_atoms, cfg.batch
    q, qt = dueling_module(params["q"], A, K), dueling_module(params["q_target"], A, K)
    z = torch.tensor(np.linspace(cfg.v_min, cfg.v_max, K))
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    rel = lambda x, ref: np.abs(np.asarray(x) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max()
    for w in (None, np.random.default_rng(5).uniform(0.2, 1.0, B)):
        _, info = learner.update_host_c51(params, batch, cfg, "float64", weights=w, grads_only=True)
        with torch.no_grad():
            pt = torch.softmax(qt(T(batch["s2"])), -1)
            ev = ((torch.softmax(q(T(batch["s2"])), -1) if double else pt) * z).sum(-1)
            astar = ev.argmax(1)
            pn = pt[torch.arange(B), astar].numpy()
        m = learner.c51_project_scatter_host(pn, batch["r"], batch["mask"], np.full(B, cfg.gamma), cfg)
        logp = torch.log_softmax(q(T(batch["s"])), -1)[torch.arange(B), torch.tensor(batch["a"])]
        rows = -(T(m) * logp).sum(-1)
        q.zero_grad()
        (rows.mean() if w is None else (T(w) * rows).mean()).backward()
        assert np.array_equal(info["targets"][:, 0].astype(np.int64), astar.numpy())
        assert rel(info["dist"][:, 0], m) <= 1e-12 and rel(info["dist"][:, 1], logp.detach().exp().numpy()) <= 1e-12
        assert rel(info["row_loss"], rows.detach().numpy()) <= 1e-12 and abs(info["loss"] - float(rows.detach().mean())) <= 1e-12 * abs(float(rows.detach().mean()))
        want = {"w0": q.trunk.weight.grad, "b0": q.trunk.bias.grad, "w1": torch.cat([q.adv.weight.grad, q.val.weight.grad]),
                "b1": torch.cat([q.adv.bias.grad, q.val.bias.grad])}
        for k in NAMES:
            assert info["grad"][k].shape == params["q"][k].shape and rel(info["grad"][k], want[k].numpy()) <= 1e-12, k
    assert params["q"]["w1"].shape == ((A + 1) * K, cfg.h1)


def test_fold_gives_the_plain_network_with_the_same_logits():
    """c51_fold_dueling_host: the folded plain network's logits equal the dueling network's in float64 to 1e-12, and fed to the PLAIN twin it gives
    the same a*, m and row loss."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    cfg, params, batch = _problem(31)
    A, K = cfg.n_actions, cfg.n_atoms
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    folded = {slot: learner.c51_fold_dueling_host(params[slot], A, K) for slot in ("q", "q_target")}
    for slot in folded:
        assert folded[slot]["w1"].shape == (A * K, cfg.h1) and folded[slot]["w1"].dtype == np.float64
        with torch.no_grad():
            have = learner._c51_logits({k: T(folded[slot][k]) for k in NAMES}, T(batch["s"]), A, K).numpy()
            want = learner._c51_logits({k: T(params[slot][k]) for k in NAMES}, T(batch["s"]), A, K, dueling=True).numpy()
            mod = dueling_module(params[slot], A, K)(T(batch["s"])).numpy()
        assert np.abs(have - want).max() <= 1e-12 * np.abs(want).max() and np.abs(mod - want).max() <= 1e-12 * np.abs(want).max()
    plain_cfg = learner.C51Config(n_obs=cfg.n_obs, n_actions=A, h1=cfg.h1, batch=cfg.batch, gamma=cfg.gamma, lr=cfg.lr, double=cfg.double, n_atoms=K,
                                  v_min=cfg.v_min, v_max=cfg.v_max)
    plain = dict(params, **{slot: folded[slot] for slot in folded})
    plain["q_m"] = plain["q_v"] = {k: np.zeros_like(folded["q"][k]) for k in NAMES}
    _, i_d = learner.update_host_c51(params, batch, cfg, "float64", grads_only=True)
    _, i_p = learner.update_host_c51(plain, batch, plain_cfg, "float64", grads_only=True)
    assert np.array_equal(i_d["targets"][:, 0], i_p["targets"][:, 0])
    assert np.abs(i_d["dist"][:, 0] - i_p["dist"][:, 0]).max() <= 1e-12 and np.abs(i_d["row_loss"] - i_p["row_loss"]).max() <= 1e-12 * np.abs(i_p["row_loss"]).max()


def test_a_shift_of_every_advantage_block_changes_nothing():
    """Adding any c[k] to every advantage block (to its bias) leaves the logits and the loss unchanged; and the gradients of W1 and b1 summed over
    the A advantage blocks are zero to rounding, for every k."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    cfg, params, batch = _problem(41)
    A, K = cfg.n_actions, cfg.n_atoms
    c = np.random.default_rng(7).normal(size=K) * 3
    shifted = {slot: {k: np.array(v, dtype=np.float64) for k, v in params[slot].items()} for slot in ("q", "q_target", "q_m", "q_v")}
    for slot in ("q", "q_target"):
        shifted[slot]["b1"][:A * K] += np.tile(c, A)
    shifted = dict(params, **shifted)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    with torch.no_grad():
        l0 = learner._c51_logits({k: T(params["q"][k]) for k in NAMES}, T(batch["s"]), A, K, dueling=True).numpy()
        l1 = learner._c51_logits({k: T(shifted["q"][k]) for k in NAMES}, T(batch["s"]), A, K, dueling=True).numpy()
    assert np.abs(l1 - l0).max() <= 1e-12 * np.abs(l0).max()
    _, i0 = learner.update_host_c51(params, batch, cfg, "float64", grads_only=True)
    _, i1 = learner.update_host_c51(shifted, batch, cfg, "float64", grads_only=True)
    assert abs(i1["loss"] - i0["loss"]) <= 1e-12 * abs(i0["loss"]) and np.abs(i1["row_loss"] - i0["row_loss"]).max() <= 1e-12 * np.abs(i0["row_loss"]).max()
    gw, gb = i0["grad"]["w1"][:A * K].reshape(A, K, -1), i0["grad"]["b1"][:A * K].reshape(A, K)
    assert np.abs(gw).max() > 0 and np.abs(gw.sum(0)).max() <= 1e-12 * np.abs(gw).max() and np.abs(gb.sum(0)).max() <= 1e-12 * np.abs(gb).max()
    # the value block's gradient is the sum over the advantage blocks of their gradient BEFORE the mean is taken out: g itself, not zero
    assert np.abs(i0["grad"]["b1"][A * K:]).max() > 0


@pytest.mark.parametrize("shape", [(2, 16), (5, 17), (19, 51)])
def test_float32_combine_twin_is_the_statement_rounded_once(shape):
    """c51_dueling_combine_host (the device's operation order: numpy float64 on float32 inputs, rounded once) equals the float64 statement
    V + Adv - mean Adv within one float32 ulp of the largest term."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    A, K = shape
    out = (np.random.default_rng(A * K).normal(size=(64, (A + 1) * K)) * 4).astype(np.float32)
    have = learner.c51_dueling_combine_host(out, A, K)
    assert have.dtype == np.float32 and have.shape == (64, A, K)
    o = out.astype(np.float64).reshape(64, A + 1, K)
    want = o[:, A:] + o[:, :A] - o[:, :A].mean(1, keepdims=True)
    # the terms: V, Adv, the mean and their sum (the one rounding is the sum's: half an ulp of it, which three terms of one size can carry to 3/2 ulp
    # of a single one of them -- so the sum counts among the terms); the ulp is float32's spacing at the largest
    largest = np.maximum(np.maximum(np.maximum(np.abs(o[:, A:]), np.abs(o[:, :A])), np.abs(o[:, :A].mean(1, keepdims=True))), np.abs(want))
    assert (np.abs(have.astype(np.float64) - want) <= np.spacing(largest.astype(np.float32)).astype(np.float64)).all()
    # A = 1 would make every logit the value: the mean takes the one advantage out
    one = learner.c51_dueling_combine_host(out[:, :2 * K], 1, K)
    assert np.array_equal(one[:, 0], out[:, K:2 * K])


def test_config_struct_and_export_key(tmp_path):
    capi = _capi()
    from rl_mpc_lanemerging_amd import learner
    with pytest.raises(ValueError, match=r"\(n_actions \+ 1\) \* n_atoms = 21 \* 51 exceeds the widest layer, 1024"):
        learner.C51Config(n_actions=20, n_atoms=51, dueling=True)
    assert learner.C51Config(n_actions=20, n_atoms=48, dueling=True).n_blocks == 21
    assert learner.C51Config(n_actions=19, n_atoms=51, dueling=True).n_blocks == 20
    with pytest.raises(ValueError, match="exceeds"):
        learner.C51Config(n_actions=20, n_atoms=49, dueling=True)
    with pytest.raises(ValueError, match="exceeds"):
        learner.C51Learner((20, 20), learner.C51Config(n_atoms=51, dueling=True))      # the action count arrives with the dims
    assert learner.C51Config().dueling is False and learner.C51Config(n_actions=5).to_c(0).dueling == 0
    # the struct: the size ABI 8 has, `dueling` where `reserved` was (the last int32, behind n_atoms)
    assert ctypes.sizeof(capi.C51Cfg) == 120 and capi.C51Cfg.dueling.offset == capi.C51Cfg.n_atoms.offset + 4 == 116 and capi.C51Cfg.dueling.size == 4
    c = learner.C51Config(n_actions=5, n_atoms=17, dueling=True).to_c(3)
    assert (c.dueling, c.reserved, c.n_atoms, c.seed) == (1, 1, 17, 3)
    assert "stmpc_dueling_c51actor_create" in capi.EXPORTS and capi.load().stmpc_dueling_c51actor_create.argtypes == capi.load().stmpc_c51actor_create.argtypes
    # export_q writes the key (the learner's own method on a stand-in: no device), and a reader takes a missing key as 0
    net = problem_net(HEAD, (20, 16, 5, 17, 7), np.random.default_rng(0))
    for flag in (True, False):
        stub = types.SimpleNamespace(cfg=learner.C51Config(n_obs=20, n_actions=5, h1=16, n_atoms=17, dueling=flag), action_values=np.arange(5.0), _slot=lambda i: net)
        path = learner.C51Learner.export_q(stub, str(tmp_path / ("q%d.npz" % flag)))
        with np.load(path) as z:
            assert int(z["dueling"]) == int(flag) and int(z["n_atoms"]) == 17 and np.array_equal(z["w1"], net["w1"])
    # a population refuses a mix of heads before it asks for the env's context (the stand-in has none)
    members = [learner.C51Config(n_obs=20, h1=16, batch=7, capacity=200, n_atoms=17, dueling=d) for d in (True, True, False)]
    env = types.SimpleNamespace(n=72, obs_dim=20, continuous=False, action_space={"n": 5})
    with pytest.raises(ValueError, match="member 2 has dueling = False, member 0 has True"):
        learner.C51Population(env, members)


@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_gpu_problems_have_the_rows_the_gpu_tests_need(si, double):
    """The problems of tests/test_c51_dueling.py's distribution test, decided by the twins alone: rows on which every expected value at s' is
    negative and rows on which one is not; at most 10 % of the rows left out of the a* comparison."""
    _capi()
    cfg, params, replay = random_problem(HEAD, SHAPES[si], PROBLEM_SEEDS[si, double], neg_shift=True, double=double)
    _, batch = minibatch_host(replay, cfg)
    i64, i32 = twins(HEAD, params, batch, cfg)
    neg = all_negative_rows(i64)
    assert neg.any() and not neg.all(), int(neg.sum())
    keep, left_out = astar_rows(i64, i32)
    assert left_out <= 0.10, left_out
    assert np.array_equal(i32["targets"][keep, 0], i64["targets"][keep, 0])
    assert (batch["mask"] == 0).any() and (batch["mask"] != 0).any()
