"""The noisy output layer of the C51 learner without a GPU (``learner.C51Config(noisy=NoisyConfig())``): the float64 twin against an independent
torch module with a noisy ``Linear`` (mu and sigma as parameters, given f vectors), plain and dueling; g_sigma = g_mu * outer(f_out, f_in); sigma = 0
is the plain twin; the float32 compose twin; the header, the library and the binding; and every refusal that needs no device.  Every test here
needs ``C51Config`` to take ``noisy``."""
import ctypes
import types

import numpy as np
import pytest

from discrete_testlib import C51, C51_DUELING, NAMES, NoLibrary, problem_net
from stmpc_testlib import capi as _capi, header_entries, header_prototypes

SIGMA = ("sigma", "sigma_target", "sigma_m", "sigma_v")
SNAMES = ("w1", "b1")
ENTRIES = {"stmpc_noisy_c51_enable": 2, "stmpc_noisy_c51_set_params": 4, "stmpc_noisy_c51_get_params": 4, "stmpc_noisy_c51_act_device": 8,
           "stmpc_noisy_c51_debug_read": 4}
POP_ENTRIES = {"stmpc_pop_noisy_c51_enable": 3, "stmpc_pop_noisy_c51_act_device": 9}


def _problem(seed, dueling, double=True, shape=(12, 24, 4, 11, 33), sigma0=0.5):
    """(cfg, params with the sigma slots, batch, f): sigma at sigma0 / sqrt(h1) times a factor per element, so that no two entries agree."""
    from rl_mpc_lanemerging_amd import learner
    head = C51_DUELING if dueling else C51
    n_obs, h1, A, K, B = shape
    W = (A + dueling) * K
    rng = np.random.default_rng(seed)
    cfg = learner.C51Config(n_obs=n_obs, n_actions=A, h1=h1, batch=B, gamma=0.9, lr=1e-3, double=double, n_atoms=K, v_min=-4.0, v_max=3.0, dueling=dueling,
                            noisy=learner.NoisyConfig(sigma0))
    params = learner.new_params_dqn(problem_net(head, shape, rng))
    params["q_target"] = problem_net(head, shape, rng)
    s0 = sigma0 / np.sqrt(h1)
    for slot in SIGMA[:2]:
        params[slot] = {"w1": s0 * rng.uniform(0.5, 1.5, (W, h1)), "b1": s0 * rng.uniform(0.5, 1.5, W)}
    for slot in SIGMA[2:]:
        params[slot] = {"w1": np.zeros((W, h1)), "b1": np.zeros(W)}
    batch = {"s": rng.normal(size=(B, n_obs)), "s2": rng.normal(size=(B, n_obs)), "a": rng.integers(0, A, B), "r": rng.normal(size=B) * 2,
             "mask": (rng.random(B) > 0.25).astype(np.float64)}
    f = {net: learner.c51_noisy_f_host(seed, i, h1, W) for i, net in enumerate(("online", "target"))}
    return cfg, params, batch, f


def _module(mu, sigma, f_in, f_out, A, K, dueling):
    """n_obs -> h1 -> ReLU -> a noisy Linear, written on its own: mu and sigma are Parameters, the f vectors buffers; logits [n][A][K]."""
    import torch

    class NoisyLinear(torch.nn.Module):
        def __init__(self):
            super().__init__()
            T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
            self.mu_w, self.mu_b = torch.nn.Parameter(T(mu["w1"])), torch.nn.Parameter(T(mu["b1"]))
            self.sigma_w, self.sigma_b = torch.nn.Parameter(T(sigma["w1"])), torch.nn.Parameter(T(sigma["b1"]))
            self.register_buffer("f_in", T(f_in)); self.register_buffer("f_out", T(f_out))

        def forward(self, x):
            return torch.nn.functional.linear(x, self.mu_w + self.sigma_w * torch.outer(self.f_out, self.f_in), self.mu_b + self.sigma_b * self.f_out)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.trunk = torch.nn.Linear(mu["w0"].shape[1], mu["w0"].shape[0]).double()
            with torch.no_grad():
                self.trunk.weight.copy_(torch.tensor(np.asarray(mu["w0"], dtype=np.float64))); self.trunk.bias.copy_(torch.tensor(np.asarray(mu["b0"], dtype=np.float64)))
            self.out = NoisyLinear()

        def forward(self, x):
            o = self.out(torch.relu(self.trunk(x)))
            if not dueling:
                return o.reshape(x.shape[0], A, K)
            o = o.reshape(x.shape[0], A + 1, K)
            return o[:, A:] + o[:, :A] - o[:, :A].mean(1, keepdim=True)

    return Net()


@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("dueling", [False, True])
def test_twin_against_a_module_with_a_noisy_linear(dueling, double):
    """update_host_c51_noisy in float64 against the hand-written module, the projection written the textbook way: a*, m, p, the row losses, the loss,
    g_mu (all four tensors) and g_sigma to 1e-12 relative; importance weights on one pass.  And g_sigma == g_mu * outer(f_out, f_in) exactly."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import learner
    cfg, params, batch, f = _problem(51 + double, dueling, double)
    A, K, B = cfg.n_actions, cfg.n_atoms, cfg.batch
    q = _module(params["q"], params["sigma"], *f["online"], A, K, dueling)
    qt = _module(params["q_target"], params["sigma_target"], *f["target"], A, K, dueling)
    z = torch.tensor(np.linspace(cfg.v_min, cfg.v_max, K))
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    rel = lambda x, ref: np.abs(np.asarray(x) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max()
    for w in (None, np.random.default_rng(5).uniform(0.2, 1.0, B)):
        _, info = learner.update_host_c51_noisy(params, batch, cfg, f, "float64", weights=w, grads_only=True)
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
        want = {"w0": q.trunk.weight.grad, "b0": q.trunk.bias.grad, "w1": q.out.mu_w.grad, "b1": q.out.mu_b.grad}
        for k in NAMES:
            assert info["grad"][k].shape == params["q"][k].shape and rel(info["grad"][k], want[k].numpy()) <= 1e-12, k
        assert rel(info["grad_sigma"]["w1"], q.out.sigma_w.grad.numpy()) <= 1e-12 and rel(info["grad_sigma"]["b1"], q.out.sigma_b.grad.numpy()) <= 1e-12
        fi, fo = (np.asarray(x, dtype=np.float64) for x in f["online"])
        assert np.array_equal(info["grad_sigma"]["w1"], info["grad"]["w1"] * (fo[:, None] * fi[None, :])) and np.array_equal(info["grad_sigma"]["b1"], info["grad"]["b1"] * fo)
        assert np.abs(info["grad_sigma"]["w1"]).max() > 0
    # the noise matters: the mean network's loss is another
    _, mean = learner.update_host_c51({k: params[k] for k in ("q", "q_target", "q_m", "q_v", "beta_pow", "updates")}, batch, cfg, "float64", grads_only=True)
    assert abs(mean["loss"] - info["loss"]) > 1e-6


@pytest.mark.parametrize("dueling", [False, True])
def test_sigma_zero_gives_the_plain_twin(dueling):
    """With sigma = 0 the noisy twin returns the plain twin's numbers, both dtypes, gradients and one Adam step with the hard copy; sigma then moves
    only where g_sigma is not zero, and its target follows on the copy."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    cfg, params, batch, f = _problem(61, dueling, sigma0=0.0)
    cfg.target_period = 1
    assert all(not params[s][k].any() for s in SIGMA for k in SNAMES)
    plain = {k: params[k] for k in ("q", "q_target", "q_m", "q_v", "beta_pow", "updates")}
    for dtype in ("float64", "float32"):
        new_n, i_n = learner.update_host_c51_noisy(params, batch, cfg, f, dtype)
        new_p, i_p = learner.update_host_c51(plain, batch, cfg, dtype)
        assert i_n["loss"] == i_p["loss"] and np.array_equal(i_n["dist"], i_p["dist"]) and np.array_equal(i_n["targets"], i_p["targets"])
        assert all(np.array_equal(i_n["grad"][k], i_p["grad"][k]) for k in NAMES)
        assert all(np.array_equal(new_n[s][k], new_p[s][k]) for s in ("q", "q_target", "q_m", "q_v") for k in NAMES)
        assert np.abs(new_n["sigma"]["w1"]).max() > 0 and np.array_equal(new_n["sigma_target"]["w1"], new_n["sigma"]["w1"]) and new_n["updates"] == 1


def test_f_and_compose_twins():
    """c51_noisy_f_host: f(e) = sign(e) sqrt|e| of noise_host's variates, e_in first; draws and streams differ.  c51_noisy_compose_host: float32, the
    float64 statement rounded once -- within half a float32 ulp of it (the inner product is exact in float64, the outer two operations round there:
    2^-53 relative each, far below) --; sigma = 0 gives mu's bits."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    h1, W = 24, 55
    f_in, f_out = learner.c51_noisy_f_host(7, 4, h1, W)
    e = learner.noise_host(7, 4, h1 + W, stream=learner.NOISY_LEARN_STREAM)[2]
    assert f_in.dtype == f_out.dtype == np.float32 and f_in.shape == (h1,) and f_out.shape == (W,)
    assert np.allclose(np.concatenate([f_in, f_out]).astype(np.float64) ** 2, np.abs(e), rtol=1e-6) and np.array_equal(np.sign(np.concatenate([f_in, f_out])), np.sign(e))
    assert not np.array_equal(f_in, learner.c51_noisy_f_host(7, 5, h1, W)[0]) and not np.array_equal(f_in, learner.c51_noisy_f_host(7, 4, h1, W, stream=learner.NOISY_ACT_STREAM)[0])
    assert learner.NOISY_LEARN_STREAM != learner.NOISY_ACT_STREAM and len({learner.NOISY_LEARN_STREAM, learner.NOISY_ACT_STREAM, learner.NOISE_STREAM}) == 3
    g = np.concatenate([np.concatenate(learner.c51_noisy_f_host(9, d, 256, 256)) for d in range(4)]).astype(np.float64)
    assert abs(g.mean()) < 0.06 and abs((g ** 2).mean() - np.sqrt(2 / np.pi)) < 0.05     # E f = 0, E f^2 = E|e| = sqrt(2 / pi)
    rng = np.random.default_rng(3)
    mu = {"w1": rng.normal(size=(W, h1)).astype(np.float32), "b1": rng.normal(size=W).astype(np.float32)}
    sg = {"w1": rng.uniform(0.05, 0.2, (W, h1)).astype(np.float32), "b1": rng.uniform(0.05, 0.2, W).astype(np.float32)}
    have = learner.c51_noisy_compose_host(mu, sg, f_in, f_out)
    d = lambda a: a.astype(np.float64)
    want = {"w1": d(mu["w1"]) + d(sg["w1"]) * np.outer(d(f_out), d(f_in)), "b1": d(mu["b1"]) + d(sg["b1"]) * d(f_out)}
    for k in SNAMES:
        assert have[k].dtype == np.float32 and (np.abs(d(have[k]) - want[k]) <= 0.5 * np.spacing(np.abs(want[k]).astype(np.float32)).astype(np.float64) * (1 + 1e-9)).all()
    zero = learner.c51_noisy_compose_host(mu, {k: np.zeros_like(v) for k, v in sg.items()}, f_in, f_out)
    assert all(np.array_equal(zero[k].view(np.uint32), mu[k].view(np.uint32)) for k in SNAMES)


def test_header_library_and_binding():
    """Exactly the new entries under the new prefix with their argument counts, bound and exported; ABI 8; sizeof(stmpc_c51_cfg) = 120; the closed
    prefix sets have the entries they had."""
    capi = _capi()
    lib = capi.load()
    protos = header_prototypes("stmpc_noisy_")
    pop_protos = header_prototypes("stmpc_pop_noisy_")
    assert set(protos) == set(ENTRIES) == header_entries("stmpc_noisy_") and set(pop_protos) == set(POP_ENTRIES) == header_entries("stmpc_pop_noisy_")
    assert set(ENTRIES) | set(POP_ENTRIES) == {n for n in capi.EXPORTS if "noisy" in n}
    protos = dict(protos, **pop_protos)
    assert lib.stmpc_pop_noisy_c51_act_device.argtypes == lib.stmpc_pop_c51_act_device.argtypes
    for name, n_args in dict(ENTRIES, **POP_ENTRIES).items():
        assert len(protos[name].split(",")) == n_args == len(getattr(lib, name).argtypes), name
    assert lib.stmpc_noisy_c51_act_device.argtypes == lib.stmpc_c51_act_device.argtypes
    assert lib.stmpc_abi_version() == capi.ABI_VERSION == 8 and ctypes.sizeof(capi.C51Cfg) == 120 and ctypes.sizeof(capi.NoisyCfg) == 8
    for prefix, count in (("stmpc_c51_", 22), ("stmpc_c51actor_", 2), ("stmpc_pop_c51_", 12), ("stmpc_nstep_", 4)):
        assert len({n for n in capi.EXPORTS if n.startswith(prefix)}) == count == len(header_prototypes(prefix)), prefix
    assert len({n for n in capi.EXPORTS if n.startswith("stmpc_pop_")}) == len(header_prototypes("stmpc_pop_"))
    assert capi.NOISY_SLOTS == SIGMA and capi.NOISY_F == {"online": 0, "target": 1, "act": 2} and capi.NOISY_DRAWS == 5 < capi.DDPG_NCOUNTERS
    # the library's refusals that need no device: a NULL learner or cfg
    cfg = capi.NoisyCfg(sigma0=0.5)
    buf = (ctypes.c_float * 4)()
    assert lib.stmpc_noisy_c51_enable(None, ctypes.byref(cfg)) != 0 and b"NULL" in lib.stmpc_last_error()
    assert lib.stmpc_noisy_c51_get_params(None, 0, buf, 4) != 0 and lib.stmpc_noisy_c51_set_params(None, 0, buf, 4) != 0
    assert lib.stmpc_noisy_c51_debug_read(None, 0, buf, 4) != 0 and lib.stmpc_noisy_c51_act_device(None, 1, None, 20, 0.0, None, None, None) != 0
    assert lib.stmpc_pop_noisy_c51_enable(None, ctypes.byref(cfg), 1) != 0 and lib.stmpc_pop_noisy_c51_act_device(None, 1, None, 20, None, 0, None, None, None) != 0


def test_python_refusals_touch_no_library(tmp_path):
    """Every refusal of the Python layer, on stand-ins that fail the test when the library is touched."""
    _capi()
    from rl_mpc_lanemerging_amd import learner
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma0"):
            learner.NoisyConfig(bad)
    assert learner.NoisyConfig().sigma0 == 0.5 and learner.NoisyConfig(0).sigma0 == 0.0
    with pytest.raises(ValueError, match="noisy must be None or a NoisyConfig"):
        learner.C51Config(noisy=0.5)
    assert learner.C51Config().noisy is None and learner.C51Config(noisy=learner.NoisyConfig(0.25)).noisy.sigma0 == 0.25
    plain = learner.C51Learner.__new__(learner.C51Learner)
    plain.cfg, plain.ctx, plain.handle = learner.C51Config(n_obs=20, n_actions=5, h1=16, n_atoms=17), NoLibrary(), None
    noisy = learner.C51Learner.__new__(learner.C51Learner)
    noisy.cfg, noisy.ctx, noisy.handle = learner.C51Config(n_obs=20, n_actions=5, h1=16, n_atoms=17, noisy=learner.NoisyConfig()), NoLibrary(), None
    assert not plain.noisy and noisy.noisy
    with pytest.raises(ValueError, match="noisy=True needs a learner with the noisy output layer"):
        plain.act(types.SimpleNamespace(shape=(3, 20)), noisy=True)
    with pytest.raises(ValueError, match="the state is a noisy C51 learner's, this learner has a plain output layer"):
        plain.load_state_dict({"noisy": True, "params": {}})
    with pytest.raises(ValueError, match="the state is a plain C51 learner's, this learner has a noisy output layer"):
        noisy.load_state_dict({"noisy": False, "params": {}})
    # a population takes noisy= itself, all members on or all off: refused before the env's context is asked for (the stand-in has none)
    mk = lambda *noisy: [learner.C51Config(n_obs=20, h1=16, batch=7, capacity=200, n_atoms=17, noisy=n) for n in noisy]
    env = types.SimpleNamespace(n=72, obs_dim=20, continuous=False, action_space={"n": 5})
    with pytest.raises(ValueError, match="member 1's cfg asks for the noisy output layer"):
        learner.C51Population(env, mk(None, learner.NoisyConfig(), None))
    with pytest.raises(ValueError, match="member 2 is plain, member 0 is noisy"):
        learner.C51Population(env, mk(None, None, None), noisy=[learner.NoisyConfig(), learner.NoisyConfig(0), None])
    with pytest.raises(ValueError, match="noisy has 2 entries, the population 3 members"):
        learner.C51Population(env, mk(None, None, None), noisy=[learner.NoisyConfig()] * 2)
    with pytest.raises(ValueError, match=r"noisy\[1\] is a float"):
        learner.C51Population(env, mk(None, None, None), noisy=[learner.NoisyConfig(), 0.5, learner.NoisyConfig()])
    with pytest.raises(ValueError, match="noisy must be None, a NoisyConfig, or a list"):
        learner.C51Population(env, mk(None, None, None), noisy=0.5)
    pop = learner.C51Population.__new__(learner.C51Population)
    pop.noisy_cfgs, pop.ctx, pop.handle = [None, None], NoLibrary(), None
    with pytest.raises(ValueError, match="noisy=True needs a population with the noisy output layer"):
        pop.act(types.SimpleNamespace(shape=(4, 20)), noisy=True)
    # export_q writes the mean network and the key (the learner's own method on a stand-in: no device)
    net = problem_net(C51, (20, 16, 5, 17, 7), np.random.default_rng(0))
    for cfg in (plain.cfg, noisy.cfg):
        stub = types.SimpleNamespace(cfg=cfg, action_values=np.arange(5.0), _slot=lambda i: net)
        with np.load(learner.C51Learner.export_q(stub, str(tmp_path / "q.npz"))) as z:
            assert int(z["noisy"]) == int(cfg.noisy is not None) and np.array_equal(z["w1"], net["w1"]) and int(z["dueling"]) == 0
