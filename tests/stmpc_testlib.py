"""Helpers the suite's modules share (plain functions: no fixtures, no hooks).  Import what a module needs, e.g.
``from stmpc_testlib import pkg as _pkg, bits as _bits, same as _same``."""
import contextlib

import numpy as np


def pkg():
    """The package, with its library built if it is not."""
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        pkg.build.build()
    return pkg


def bits(a):
    """A float array as the unsigned integers of its bit patterns (anything else as it is): NaNs and signed zeros compare by their bits."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """Equal shape, dtype and bits."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@contextlib.contextmanager
def settings_of(*groups):
    """The global Settings with the values of one or more groups (a traffic group, a reward group, ...) less their ``seed``: how a lone world or env
    of them is made through the plain entries."""
    p = pkg()
    snap = p.Settings.snapshot()
    for group in groups:
        p.apply_overrides({k: v for k, v in group.items() if k != "seed"})
    try:
        yield
    finally:
        p.Settings.restore(snap)


def linit(m):
    """Small random actor and critic nets (21 / 22 -> 400 -> 300 -> 1) of learner ``m``, from its own generator."""
    from rl_mpc_lanemerging_amd import learner
    rng = np.random.default_rng(100 + m)
    a_net, q_net = learner.init_net(21, 400, 300, rng), learner.init_net(22, 400, 300, rng)
    a_net["w2"] = rng.normal(0, 0.05, (1, 300)).astype(np.float32)
    q_net["w2"] = rng.normal(0, 0.05, (1, 300)).astype(np.float32)
    return {"actor": a_net, "critic": q_net}
