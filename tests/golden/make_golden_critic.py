#!/usr/bin/env python3
"""Export the reference's pretrained DDPG critic ``pretrained_models/ddpg_medium1_extended/q.pt`` as raw tensors (data only, no pickle).

Build-container only (needs /root/reference/pretrained_models).  The checkpoint is a ``torch.save``d module of the ``all`` library
(autonomous-learning-library 0.5.3), which is not installed; the classes the pickle names are mapped to inert ``nn.Module`` stand-ins by
the same ``find_class`` override as ``data/make_actor_weights.py`` uses, which is enough to read the tensors:

    model.0  Linear 22 -> 400      (20 observation entries, the time feature, the action)
    model.2  Linear 400 -> 300
    model.4  Linear0 300 -> 1

Writes tests/golden/critic_ddpg_medium1.npz with w0,b0,w1,b1,w2,b2 (float32, as stored).  Used by tests/test_learner.py only, so that the
learner's parity tests run on trained weights of real magnitude.
Re-run:  python tests/golden/make_golden_critic.py
"""
import os
import pickle
import types
import warnings

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "/root/reference/pretrained_models/ddpg_medium1_extended/q.pt"


class _Inert(nn.Module):
    def __init__(self, *a, **k):
        super().__init__()


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except Exception:
            if not module.startswith("all."):
                raise
            return type(name, (_Inert,), {"__module__": module})


def main():
    pm = types.ModuleType("pickle_with_stand_ins")
    pm.Unpickler = _Unpickler
    pm.load = lambda f, **kw: _Unpickler(f, **kw).load()
    pm.__name__ = "pickle"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = torch.load(SRC, pickle_module=pm, weights_only=False, map_location="cpu")
    sd = m.state_dict()
    assert list(sd) == ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "model.4.weight", "model.4.bias"], list(sd)
    assert tuple(sd["model.0.weight"].shape) == (400, 22) and tuple(sd["model.2.weight"].shape) == (300, 400) and tuple(sd["model.4.weight"].shape) == (1, 300)
    out = os.path.join(HERE, "critic_ddpg_medium1.npz")
    np.savez_compressed(out, w0=sd["model.0.weight"].numpy(), b0=sd["model.0.bias"].numpy(), w1=sd["model.2.weight"].numpy(),
                        b1=sd["model.2.bias"].numpy(), w2=sd["model.4.weight"].numpy(), b2=sd["model.4.bias"].numpy())
    print({k: tuple(v.shape) for k, v in sd.items()}, "max|w|", max(float(v.abs().max()) for v in sd.values()), "->", os.path.getsize(out), "B")


if __name__ == "__main__":
    main()
