"""Helpers the vector-env test modules share (plain functions, as in stmpc_testlib.py: no fixtures, no hooks, nothing heavy at import time).  Import what
a module needs, e.g. ``from env_testlib import settings as _settings, flat as _flat``.  Pinned on the CPU by test_testlib_cpu.py."""
import numpy as np

from stmpc_testlib import pkg

_M64 = (1 << 64) - 1
GROUP_COLUMNS = ("traffic_type", "traffic_group", "reward_group")       # the columns of an episode log that say whose episode it is, not what happened


def settings():
    """The shielded env tests' Settings: REFERENCE_DEFAULT + COMBINED_MEDIUM_1 + the "default" traffic."""
    p = pkg()
    from rl_mpc_lanemerging_amd import combined_bench, episodes
    p.apply_overrides(p.REFERENCE_DEFAULT)
    p.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    p.apply_overrides(episodes.TRAFFIC_TYPES["default"])
    return p.Settings


def flat(d, prefix=""):
    """A nested dict of arrays as one dict of copies under dotted keys."""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(flat(v, prefix + str(k) + "."))
        else:
            out[prefix + str(k)] = np.asarray(v).copy()
    return out


def hash01(e, tick):
    """A fixed hash of (environment, tick of its episode) in [0, 1): equal episodes receive equal actions whatever else the env has been through."""
    z = (0x9E3779B97F4A7C15 * (e * 1000003 + tick + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 11) / 9007199254740992.0


def episodes_of(run, n, extra_keys=()):
    """{(e, j): the record of finished episode j of row e < n} of a recorded run ([step][row] arrays, ``obs0`` the reset's observations, ``done``): the
    observation it started from, every later observation of it, its final observation and statistics row, and of every tick of it the rewards, the
    flags and ``extra_keys`` (a shield's outputs)."""
    eps = {}
    for e in range(n):
        start, s0, j = run["obs0"][e], 0, 0
        for s in np.flatnonzero(run["done"][:, e]):
            ep = {"start": start, "obs": run["obs"][s0:s, e], "final_observation": run["final_observation"][s, e], "final_stats": run["final_stats"][s, e],
                  "ticks": run["ticks"][s0:s, e], "end_step": int(s)}
            ep.update({k: run[k][s0:s + 1, e] for k in ("reward", "terminated", "truncated") + tuple(extra_keys)})
            eps[(e, j)] = ep
            start, s0, j = run["obs"][s, e], s + 1, j + 1
    return eps


def log_rows(log):
    """{(env, episode): the bytes of that row of a drained episode log}, less ``GROUP_COLUMNS``."""
    cols = [k for k in sorted(log) if k not in GROUP_COLUMNS]
    return {(int(e), int(j)): np.array([log[k][i] for k in cols], dtype=np.float64).tobytes() for i, (e, j) in enumerate(zip(log["env"], log["episode"]))}
