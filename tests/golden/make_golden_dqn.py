#!/usr/bin/env python3
"""Golden vectors for the DQN learner: the reference's own ``get_targets`` (dqn.py:673-705) under DOUBLE_DQN True and False and once with
CLIP_TARGETS, and one ``SmoothL1Loss`` + ``optim.Adam`` step written as dqn.py:333-342 writes it, on a seeded ``DQN()`` with an independent
target network and 50 ``rl.History`` tuples, 9 of them with ``next_state None``.

Build-container only (needs the reference checkout).  Inert stand-ins as in make_golden_combined.py: traci, cvxopt and
torch.utils.tensorboard -- none is called on this path.  Data only is recorded: the weights before, the batch, the three target vectors,
the double-DQN argmax indices, ``q_values``, the gradients, the weights after and the constants.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import import_reference      # noqa: E402

B, N_END = 50, 9
NAMES = ("w0", "b0", "w1", "b1")


def tensors(net):
    layers = (net.first_hidden_layer.weight, net.first_hidden_layer.bias, net.last_hidden_layer.weight, net.last_hidden_layer.bias)
    return [t.detach().numpy().copy() for t in layers]


def one_training_step(dqn, net, target, sars, S):
    """One step of the reference's trainer on ``sars`` through the reference's own calls -- ``get_targets``, the module's tensor helpers and
    ``forward``, ``nn.SmoothL1Loss`` and ``optim.Adam`` with Settings.LEARNING_RATE, as DQNAgent._train uses them.  ``net`` is stepped in place;
    returns (targets, Q(s, a), loss, the four gradients), numpy."""
    import torch
    adam = torch.optim.Adam(net.parameters(), lr=S.LEARNING_RATE)
    y = dqn.get_targets(sars, net, target, gamma=S.DISCOUNT_FACTOR)
    chosen = net.get_action_tensor_bulk([h.action for h in sars]).reshape((-1, 1))
    adam.zero_grad()
    q_sa = torch.gather(net.forward(net.get_q_tensor_bulk([h.state for h in sars])), 1, chosen).flatten()
    huber = torch.nn.SmoothL1Loss()(q_sa, net.get_target_tensor_bulk(y))
    huber.backward()
    layers = (net.first_hidden_layer, net.last_hidden_layer)
    grads = [t.grad.detach().numpy().copy() for layer in layers for t in (layer.weight, layer.bias)]
    adam.step()
    return y, q_sa.detach().numpy(), float(huber.detach()), grads


def main():
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    S = import_reference()[0]
    import torch
    import dqn                                                  # noqa: E402  (the reference's)
    import rl                                                   # noqa: E402
    S.CUDA = False
    rng = np.random.default_rng(20240)
    n_obs = 4 + (4 if S.USE_ACCELERATION_OF_OTHER_CARS else 3) * (S.CARS_AHEAD + S.CARS_BEHIND)
    scale = np.where(np.arange(n_obs) % 4 == 0, 30.0, np.where(np.arange(n_obs) % 4 == 1, 5.0, 1.0))
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)       # (values a float32 ring row holds exactly)
    s, s2 = f32(rng.normal(size=(B, n_obs)) * scale), f32(rng.normal(size=(B, n_obs)) * scale)
    r = f32(rng.normal(size=B) * 2.0)
    a = rng.integers(0, 5, size=B)
    end = np.zeros(B, dtype=bool)
    end[rng.choice(B, size=N_END, replace=False)] = True
    sars = [rl.History(s[i], None if end[i] else s2[i], int(a[i]), float(r[i])) for i in range(B)]
    live = np.flatnonzero(~end)
    for seed in range(100):                                     # seeded weights whose top two online Q(s') are apart on every row
        torch.manual_seed(seed)
        net, target = dqn.DQN(), dqn.DQN()
        with torch.no_grad():
            top = torch.topk(net.forward(net.get_q_tensor_bulk([s2[i] for i in live])), 2, dim=1)
        if float((top.values[:, 0] - top.values[:, 1]).min()) > 1e-4:
            break
    else:
        raise SystemExit("no seed separates the top two Q values")
    assert float((top.values[:, 0] - top.values[:, 1]).min()) > 1e-4
    best = np.full(B, -1, dtype=np.int64)
    best[live] = top.indices[:, 0].numpy()
    target.eval()
    out = {"seed": np.array(seed), "s": s.astype(np.float32), "s2": s2.astype(np.float32), "a": a.astype(np.int64), "r": r, "mask": (~end).astype(np.float32),
           "best": best, "gamma": np.array(S.DISCOUNT_FACTOR), "lr": np.array(S.LEARNING_RATE)}
    for k, v in zip(NAMES, tensors(net)):
        out["q_" + k] = v
    for k, v in zip(NAMES, tensors(target)):
        out["t_" + k] = v
    S.DOUBLE_DQN, S.CLIP_TARGETS = False, False
    out["targets_plain"] = dqn.get_targets(sars, net, target, gamma=S.DISCOUNT_FACTOR)
    S.DOUBLE_DQN, S.CLIP_TARGETS, S.CLIP_MIN_REWARD, S.CLIP_MAX_REWARD = True, True, -2.0, 2.0
    out["targets_clip"] = dqn.get_targets(sars, net, target, gamma=S.DISCOUNT_FACTOR)
    out["clip"] = np.array([S.CLIP_MIN_REWARD, S.CLIP_MAX_REWARD])
    S.CLIP_TARGETS = False
    y, q_sa, loss, grads = one_training_step(dqn, net, target, sars, S)
    out["targets_double"], out["q_values"], out["loss"] = y, q_sa, np.array(loss)
    assert sum(p.numel() for p in net.parameters()) == sum(v.size for v in grads)      # (the two registered layers are the whole module)
    for k, g, v in zip(NAMES, grads, tensors(net)):
        out["g_" + k], out["after_" + k] = g, v
    np.savez_compressed(os.path.join(HERE, "golden_dqn.npz"), **out)
    print("dqn: seed %d, %d rows (%d terminal), |diff| > 1 on %d rows, loss %.6f" % (
        seed, B, N_END, int((np.abs(out["q_values"] - y) > 1).sum()), float(loss)))


if __name__ == "__main__":
    main()
