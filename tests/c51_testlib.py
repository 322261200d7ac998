"""What tests/test_c51_cpu.py and tests/test_c51.py share: the four network shapes, the problems (random and dyadic), the projection's edge-case
inputs, and the rule for comparing a*.  Plain functions, nothing heavy at import time; the package is imported inside the functions."""
import numpy as np

from learner_testlib import bound_4x, rel_err
from stmpc_testlib import capi

# (n_obs, h1, A, K, B): A K = 85 -> Ap = 96 (pad columns inside the last tile, K < 32 lanes, padded minibatch rows); K one over the lane count, every
# block straddling 16-column tiles; A K = 1020 -> 1024, the widest allowed, three row tiles; the shipped shape
SHAPES = [(20, 16, 5, 17, 7), (12, 32, 3, 33, 16), (20, 48, 20, 51, 33), (20, 256, 5, 51, 64)]
NAMES = ("w0", "b0", "w1", "b1")
Q_SLOTS = ("q", "q_target", "q_m", "q_v")
RING = 128
LEARNER_SEED = 11
NEG_TILT = 0.3                  # found on the CPU: about half of a ring's rows then have only negative expected values
# generator seed per (shape index, double): the first from 300 on under which the float64 twin alone (a) has rows whose real expected values at s'
# are all negative and rows where they are not and (b) leaves at most 10 % of the rows' a* out of the comparison (test_c51_cpu.py asserts both)
PROBLEM_SEEDS = {(i, d): 300 for i in range(len(SHAPES)) for d in (True, False)}
PROBLEM_SEEDS[1, False] = 301


def random_problem(shape, seed, neg_shift=False, **kw):
    """(cfg, params, replay): nn.Linear-scale nets with a target that differs, RING replay rows.  ``neg_shift``: the support is [-4, 4] and the last
    layer's bias tilts every action's distribution a little towards its low atoms, so that on a part of the rows every real expected value at s'
    is negative (a pad column's logits of 0 would mean the support's centre, 0: above them all)."""
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, K, B = shape
    rng = np.random.default_rng(seed)
    sup = dict(v_min=-4.0, v_max=4.0) if neg_shift else dict(v_min=-10.0, v_max=10.0)
    sup.update(kw)
    cfg = learner.C51Config(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=RING, lr=1e-3, n_atoms=K, **sup)

    def net():
        n = learner.init_c51_net(n_obs, h1, A, K, rng)
        n["w1"] = (n["w1"] * 3).astype(np.float32)                 # logits that spread: distributions away from uniform
        if neg_shift:
            n["b1"] = (n["b1"].reshape(A, K) - NEG_TILT * np.linspace(-1, 1, K)[None, :]).reshape(-1).astype(np.float32)
        return n
    params = learner.new_params_dqn(net())
    params["q_target"] = net()
    replay = {"s": rng.normal(size=(RING, n_obs)).astype(np.float32), "s2": rng.normal(size=(RING, n_obs)).astype(np.float32), "a": rng.integers(0, A, RING),
              "r": rng.normal(size=RING) * 2, "term": rng.random(RING) < 0.2}
    return cfg, params, replay


def rows_of(replay, n_obs):
    """The ring rows the push kernel writes for ``replay`` pushed into an empty ring."""
    c = capi()
    R = replay["s"].shape[0]
    rows = np.zeros((R, c.DDPG_ROW), dtype=np.float32)
    rows[:, :n_obs], rows[:, 32:32 + n_obs] = replay["s"], replay["s2"]
    rows[:, 64], rows[:, 65], rows[:, c.DQN_ACTION_COL] = replay["r"], np.where(replay["term"], 0, 1), replay["a"]
    return rows


def minibatch_host(replay, cfg, seed=LEARNER_SEED, update=0):
    from rl_mpc_lanemerging_amd import learner
    rows = rows_of(replay, cfg.n_obs)[learner.sample_indices_host(seed, update, cfg.batch, replay["s"].shape[0])]
    return rows, learner.dqn_batch_from_rows(rows, cfg.n_obs)


def astar_rows(i64, i32):
    """The rows on which a* is compared: those where the float64 twin's two largest expected values at s' differ by more than the parity bound of
    the expected values (relative to their max norm, as the rule measures them).  Returns (mask [B], the share of rows left out)."""
    ev = i64["ev_next"]
    if ev.shape[1] < 2:
        return np.ones(ev.shape[0], dtype=bool), 0.0
    top = np.sort(ev, axis=1)
    gap = top[:, -1] - top[:, -2]
    keep = gap > bound_4x(rel_err(i32["ev_next"], ev)) * np.abs(ev).max()
    return keep, float(1.0 - keep.mean())


def all_negative_rows(i64):
    return (i64["ev_next"] < 0).all(1)


# ---- the projection's inputs ---------------------------------------------------------------------------------------------------------------------
def dyadic_projection_case(K, n=48, seed=0):
    """(cfg, p [n][K], r, mask, disc) on dyadic grids under which every product and sum of the projection is exact in float32: p multiples of 2^-10
    summing to 1, r multiples of 1/4, disc in {1/2, 3/4, 1}, v_min = -8, v_max = 8 (dz = 16 / (K - 1): 1 at K = 17, 1/2 at K = 33).  The first
    rows are the edge cases: integer b_j, shifts clamped at both ends, terminated rows with the reward on an atom and between two atoms."""
    capi()
    from rl_mpc_lanemerging_amd import learner
    cfg = learner.C51Config(n_obs=4, n_actions=2, h1=16, batch=4, capacity=16, n_atoms=K, v_min=-8.0, v_max=8.0)
    dz = 16.0 / (K - 1)
    rng = np.random.default_rng(700 + K + seed)
    cuts = np.sort(rng.integers(0, 1025, size=(n, K - 1)), axis=1)
    p = np.diff(np.concatenate([np.zeros((n, 1), dtype=np.int64), cuts, np.full((n, 1), 1024)], axis=1), axis=1) / 1024.0
    r = rng.integers(-24, 25, n) / 4.0
    disc = rng.choice([0.5, 0.75, 1.0], n)
    mask = (rng.random(n) > 0.25).astype(np.float64)
    r[0], disc[0], mask[0] = 1.0, 1.0, 1.0                          # every b_j an integer (shift by one or two atoms), the top ones clamped
    r[1], disc[1], mask[1] = 6.0, 1.0, 1.0                          # clamped at v_max
    r[2], disc[2], mask[2] = -6.0, 1.0, 1.0                         # clamped at v_min
    r[3], mask[3] = 2.0, 0.0                                        # terminated, the reward on an atom
    r[4], mask[4] = 2.0 + dz / 4, 0.0                               # terminated, the reward between two atoms
    r[5], mask[5] = 30.0, 0.0                                       # terminated, the reward past v_max
    return cfg, p, r, mask, disc


def projection_edge_cases(cfg, r, mask, disc):
    """Which of the edge cases occur in (r, mask, disc): a dict of booleans."""
    from rl_mpc_lanemerging_amd import learner
    z = learner.c51_support(cfg)
    r, mask, disc = (np.asarray(x, dtype=np.float64) for x in (r, mask, disc))
    dz = (cfg.v_max - cfg.v_min) / (cfg.n_atoms - 1)
    live = mask != 0
    raw = np.where(live[:, None], r[:, None] + disc[:, None] * z[None, :], r[:, None] + 0 * z[None, :])
    b = (np.clip(raw, cfg.v_min, cfg.v_max) - cfg.v_min) / dz
    inside = (raw > cfg.v_min) & (raw < cfg.v_max)
    bt = b[~live, 0]
    return {"integer b_j": bool(((b == np.round(b)) & inside & live[:, None]).any()), "clamped at v_min": bool((raw[live] < cfg.v_min).any()),
            "clamped at v_max": bool((raw[live] > cfg.v_max).any()), "terminated on an atom": bool(((bt == np.round(bt)) & inside[~live, 0]).any()),
            "terminated between atoms": bool((bt != np.round(bt)).any())}
