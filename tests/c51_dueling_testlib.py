"""What tests/test_c51_dueling_cpu.py and tests/test_c51_dueling.py share: the five network shapes of the dueling head, the problems, the torch
module with separate value and advantage heads that the twin is compared with, and the pad masks.  Plain functions, nothing heavy at import time;
the package is imported inside the functions."""
import numpy as np

from c51_testlib import LEARNER_SEED, NEG_TILT, RING, rows_of
from stmpc_testlib import capi

# (n_obs, h1, A, K, B) -> output width (A + 1) K -> Ap: 48 -> 48 (no pad column, K a multiple of 16, the fewest actions); 102 -> 112 (K < 32 lanes, a
# partial minibatch tile); 132 -> 144 (K just over one lane stride); 1020 -> 1024 (the widest output that fits); 306 -> 320 (the shipped head)
SHAPES = [(20, 16, 2, 16, 5), (20, 16, 5, 17, 7), (12, 32, 3, 33, 16), (20, 48, 19, 51, 33), (20, 256, 5, 51, 64)]
NAMES = ("w0", "b0", "w1", "b1")
Q_SLOTS = ("q", "q_target", "q_m", "q_v")
# generator seed per (shape index, double): the first from 300 on under which the float64 twin alone (a) has rows whose expected values at s' are all
# negative and rows where they are not and (b) leaves at most 10 % of the rows' a* out of the comparison (test_c51_dueling_cpu.py asserts both)
PROBLEM_SEEDS = {(i, d): 300 for i in range(len(SHAPES)) for d in (True, False)}


def width(shape):
    return (shape[2] + 1) * shape[3]


def duel_net(shape, rng, neg_shift=False):
    """A dueling net at nn.Linear scale with a last layer that spreads the logits; ``neg_shift``: the VALUE block's bias tilts every action's
    distribution towards the low atoms (a tilt of the advantage blocks would cancel in the head)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, K, _ = shape
    n = learner.init_c51_net(n_obs, h1, A, K, rng, dueling=True)
    n["w1"] = (n["w1"] * 3).astype(np.float32)
    if neg_shift:
        b1 = n["b1"].reshape(A + 1, K).copy()
        b1[A] -= NEG_TILT * np.linspace(-1, 1, K)
        n["b1"] = b1.reshape(-1).astype(np.float32)
    return n


def duel_problem(shape, seed, neg_shift=False, dueling=True, **kw):
    """(cfg, params, replay) as c51_testlib.random_problem makes them, for a dueling head (the nets have (A + 1) K output rows)."""
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, K, B = shape
    rng = np.random.default_rng(seed)
    sup = dict(v_min=-4.0, v_max=4.0) if neg_shift else dict(v_min=-10.0, v_max=10.0)
    sup.update(kw)
    cfg = learner.C51Config(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=RING, lr=1e-3, n_atoms=K, dueling=dueling, **sup)
    params = learner.new_params_dqn(duel_net(shape, rng, neg_shift))
    params["q_target"] = duel_net(shape, rng, neg_shift)
    replay = {"s": rng.normal(size=(RING, n_obs)).astype(np.float32), "s2": rng.normal(size=(RING, n_obs)).astype(np.float32), "a": rng.integers(0, A, RING),
              "r": rng.normal(size=RING) * 2, "term": rng.random(RING) < 0.2}
    return cfg, params, replay


def minibatch_host(replay, cfg, seed=LEARNER_SEED, update=0):
    from rl_mpc_lanemerging_amd import learner
    rows = rows_of(replay, cfg.n_obs)[learner.sample_indices_host(seed, update, cfg.batch, replay["s"].shape[0])]
    return rows, learner.dqn_batch_from_rows(rows, cfg.n_obs)


def twins(params, batch, cfg, **kw):
    from rl_mpc_lanemerging_amd import learner
    return tuple(learner.update_host_c51(params, batch, cfg, d, grads_only=True, **kw)[1] for d in ("float64", "float32"))


def split_heads(net, A, K):
    """(advantage W [A K][h1], advantage b, value W [K][h1], value b) of a dueling net's output layer."""
    return net["w1"][:A * K], net["b1"][:A * K], net["w1"][A * K:], net["b1"][A * K:]


def dueling_module(net, A, K):
    """An independent statement of the network: a torch module (float64) with a trunk, an advantage nn.Linear and a value nn.Linear carrying
    ``net``'s weights; ``forward`` gives the logits [n][A][K] = V + Adv - mean_a Adv."""
    import torch
    from torch import nn

    class Dueling(nn.Module):
        def __init__(self):
            super().__init__()
            h1, n_in = net["w0"].shape
            self.trunk, self.adv, self.val = nn.Linear(n_in, h1), nn.Linear(h1, A * K), nn.Linear(h1, K)

        def forward(self, x):
            h = torch.relu(self.trunk(x))
            adv, val = self.adv(h).view(-1, A, K), self.val(h).view(-1, 1, K)
            return val + adv - adv.mean(dim=1, keepdim=True)

    m = Dueling().double()
    wa, ba, wv, bv = split_heads(net, A, K)
    with torch.no_grad():
        for p, v in ((m.trunk.weight, net["w0"]), (m.trunk.bias, net["b0"]), (m.adv.weight, wa), (m.adv.bias, ba), (m.val.weight, wv), (m.val.bias, bv)):
            p.copy_(torch.tensor(np.asarray(v), dtype=torch.float64))
    return m


def pad_mask(n_obs, h1, n_out):
    h1p, Ap = (h1 + 15) & ~15, (n_out + 15) & ~15
    m = {"w0": np.ones((h1p, 32), bool), "b0": np.ones(h1p, bool), "w1": np.ones((Ap, h1p), bool), "b1": np.ones(Ap, bool)}
    m["w0"][:h1, :n_obs], m["b0"][:h1], m["w1"][:n_out, :h1], m["b1"][:n_out] = False, False, False, False
    return m
