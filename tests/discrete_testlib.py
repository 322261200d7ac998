"""What the discrete agents' test modules share (DQN, C51, the dueling C51 head; their populations; the Q and C51 policies), each defined once.
Plain functions and constants: no fixtures, no hooks, nothing heavy at import time -- the package is imported, and its library built, inside the
functions.  What the copies differed in is a ``Head`` (DQN, C51, C51_DUELING); a helper that met such a difference takes a head.  Import what a
module needs by the names its bodies use, e.g. ``from discrete_testlib import C51 as HEAD, assert_same as _assert_same, fill as _fill``."""
import types

import numpy as np

from learner_testlib import CAP, N_PER, STEPS, bits64, bound_4x, dev as to_device, rel_err
from stmpc_testlib import actor_settings, actor_states, bits, capi, episode_settings

NAMES = ("w0", "b0", "w1", "b1")
Q_SLOTS = ("q", "q_target", "q_m", "q_v")
RING = 128
LEARNER_SEED = 11
NEG_TILT = 0.3                  # found on the CPU: about half of a ring's rows then have only negative expected values
# what the members of the population tests differ in whatever the head (the head's own part is Head.varied)
GAMMA, LR = (0.999, 0.95, 0.9), (2e-4, 1e-3, 5e-4)
DOUBLE, PERIOD = (True, False, True), (1, 3, 5)
C51_SUPPORTS = ((-10.0, 10.0), (-4.0, 4.0), (-2.0, 6.0))


# ---- the heads -----------------------------------------------------------------------------------------------------------------------------------
class Head:
    """What the DQN, C51 and dueling C51 copies of a helper differed in.  ``name``; ``prefix``: the binding's entry prefix (``<prefix>_pop_size``);
    ``learner``, ``population``, ``config``, ``twin``: the classes and the host twin (resolved when asked for: the package is not imported here);
    ``atoms``: the shape tuple is (n_obs, h1, A, K, B), else (n_obs, h1, A, B); ``dueling``; ``varied(m)``: the settings of its own that member m
    of a population test gets."""

    def __init__(self, name, prefix, learner, population, config, twin, atoms, dueling, varied):
        self.name, self.prefix, self.atoms, self.dueling, self.varied = name, prefix, atoms, dueling, varied
        self._names = dict(learner=learner, population=population, config=config, twin=twin)

    def __getattr__(self, key):
        if key.startswith("_") or key not in self._names:
            raise AttributeError(key)
        capi()
        from rl_mpc_lanemerging_amd import learner
        return getattr(learner, self._names[key])

    def __repr__(self):
        return self.name

    def dims(self, shape):
        """(n_obs, h1, A, K, B) of a shape tuple of this head's layout; K is None without atoms."""
        return tuple(shape) if self.atoms else (shape[0], shape[1], shape[2], None, shape[3])

    def width(self, shape):
        """The network's output width: A, A K or (A + 1) K."""
        _, _, A, K, _ = self.dims(shape)
        return (A + self.dueling) * K if self.atoms else A

    def cfg_width(self, cfg):
        return cfg.n_blocks * cfg.n_atoms if self.atoms else cfg.n_actions

    def net(self, shape, rng):
        """The net builder: init_q_net, or init_c51_net with or without ``dueling``."""
        capi()
        from rl_mpc_lanemerging_amd import learner
        n_obs, h1, A, K, _ = self.dims(shape)
        if not self.atoms:
            return learner.init_q_net(n_obs, h1, A, rng)
        return learner.init_c51_net(n_obs, h1, A, K, rng, dueling=True) if self.dueling else learner.init_c51_net(n_obs, h1, A, K, rng)

    def cfg(self, shape, m, **overrides):
        """Member m's cfg of the population tests: its own gamma, target_period and double and what the head varies; ``overrides`` on top (the
        capacity, n_actions where no env gives it, replay_start, lr, per, ...)."""
        n_obs, h1, A, K, B = self.dims(shape)
        base = dict(n_obs=n_obs, h1=h1, batch=B, gamma=GAMMA[m], target_period=PERIOD[m], double=DOUBLE[m], **self.varied(m))
        if self.atoms:
            base["n_atoms"] = K
        return self.config(**dict(base, **overrides))


def _c51_varied(m):
    return dict(v_min=C51_SUPPORTS[m][0], v_max=C51_SUPPORTS[m][1])


DQN = Head("dqn", "dqn", "DQNLearner", "DQNPopulation", "DQNConfig", "update_host_dqn", False, False,
           lambda m: dict(clip_targets=(False, True, False)[m], clip_min=-2.0, clip_max=1.0))
C51 = Head("c51", "c51", "C51Learner", "C51Population", "C51Config", "update_host_c51", True, False, _c51_varied)
C51_DUELING = Head("c51_dueling", "c51", "C51Learner", "C51Population", "C51Config", "update_host_c51", True, True, lambda m: dict(_c51_varied(m), dueling=True))
HEADS = {h.name: h for h in (DQN, C51, C51_DUELING)}

SHAPES = {
    # (n_obs, h1, A, B): one and two output tiles, an A that crosses a tile with padding, a B that is no multiple of 16 and one that is, the
    # reference's own shape
    "dqn": [(20, 16, 5, 7), (20, 48, 20, 33), (20, 256, 5, 50), (12, 32, 17, 16)],
    # (n_obs, h1, A, K, B): A K = 85 -> Ap = 96 (pad columns inside the last tile, K < 32 lanes, padded minibatch rows); K one over the lane count,
    # every block straddling 16-column tiles; A K = 1020 -> 1024, the widest allowed, three row tiles; the shipped shape
    "c51": [(20, 16, 5, 17, 7), (12, 32, 3, 33, 16), (20, 48, 20, 51, 33), (20, 256, 5, 51, 64)],
    # (n_obs, h1, A, K, B) -> output width (A + 1) K -> Ap: 48 -> 48 (no pad column, K a multiple of 16, the fewest actions); 102 -> 112 (K < 32
    # lanes, a partial minibatch tile); 132 -> 144 (K just over one lane stride); 1020 -> 1024 (the widest output that fits); 306 -> 320 (the
    # shipped head)
    "c51_dueling": [(20, 16, 2, 16, 5), (20, 16, 5, 17, 7), (12, 32, 3, 33, 16), (20, 48, 19, 51, 33), (20, 256, 5, 51, 64)],
}
GRAD_SHAPES = {"dqn": [(20, 16, 5, 8), (20, 48, 20, 32), (20, 256, 5, 64), (12, 32, 17, 16)]}      # SHAPES["dqn"]'s networks at a power-of-two B each
# generator seed per (shape index, double): the first from 300 on under which the float64 twin alone (a) has rows whose real expected values at s'
# are all negative and rows where they are not and (b) leaves at most 10 % of the rows' a* out of the comparison (test_c51_cpu.py and
# test_c51_dueling_cpu.py assert both)
PROBLEM_SEEDS = {name: {(i, d): 300 for i in range(len(SHAPES[name])) for d in (True, False)} for name in ("c51", "c51_dueling")}
PROBLEM_SEEDS["c51"][1, False] = 301


# More than 32 actions: a lane of dqn_argmax owns more than one column, three and more output tiles, stored actions of 32 and more.  Every B is a
# power of two: one table serves the exact targets and the exact gradients.  What each reaches:
#   dqn (20, 32, 40, 16)          Ap = 48: three output tiles, eight pad columns inside the second stride, A no multiple of 16
#   dqn (12, 16, 64, 8)           exactly two strides, no pad column, half a tile of minibatch rows
#   dqn (20, 48, 256, 32)         the most the library admits: sixteen output tiles, eight columns per lane
#   c51 (20, 16, 64, 16, 8)       A K = 1024 out of 64 blocks of half a lane stride each
#   c51_dueling (20, 16, 63, 16, 8)   (A + 1) K = 1024, an odd A in the mean's division
WIDE_A = {"dqn": [(20, 32, 40, 16), (12, 16, 64, 8), (20, 48, 256, 32)], "c51": [(20, 16, 64, 16, 8)], "c51_dueling": [(20, 16, 63, 16, 8)]}
NETS_WIDE = [(20, 32, 40), (20, 48, 256)]             # (n_obs, h1, A) of the Q policies beyond one lane stride
# the C51 modules run SHAPES[name] + WIDE_A[name]: the wide shape's index is len(SHAPES[name]), and its seeds are chosen as PROBLEM_SEEDS' are
PROBLEM_SEEDS["c51"].update({(len(SHAPES["c51"]), True): 301, (len(SHAPES["c51"]), False): 300})
PROBLEM_SEEDS["c51_dueling"].update({(len(SHAPES["c51_dueling"]), True): 302, (len(SHAPES["c51_dueling"]), False): 300})
# generator seed per (shape, double) of ``dqn_wide_problem``: the first from 0 on under which ``dqn_wide_counts`` meets ``dqn_wide_counts_ok``
# (test_dqn_cpu.py asserts it from the float64 twin alone)
WIDE_DQN_SEEDS = {((20, 32, 40, 16), True): 0, ((20, 32, 40, 16), False): 4, ((12, 16, 64, 8), True): 10, ((12, 16, 64, 8), False): 9,
                  ((20, 48, 256, 32), True): 13, ((20, 48, 256, 32), False): 85}
WIDE_ACT_ROWS = 50
WIDE_BONUS = 2.0                # the tie groups' bonus on b1, in units of Q(s')'s spread 0.45 sqrt(h1): found on the CPU (the groups win, and not one alone)


# ---- the DQN learner's exact problems ------------------------------------------------------------------------------------------------------------
def dqn_dyadic_problem(shape, double, clip, seed=0):
    """Weights, observations and rewards on small dyadic grids and gamma = 0.5: every sum of the forward pass is exact in float32 (|Q| < 2^13 in
    units of 2^-9).  b1 is shifted down so that on some rows every real Q(s') is negative (the pad columns' 0 would win a careless argmax)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = shape
    rng = np.random.default_rng(100 + seed)
    grid = lambda lo, hi, den, *sh: rng.integers(lo, hi + 1, size=sh).astype(np.float64) / den
    shift = np.round((1.0 if A <= 5 else 0.7) * 0.45 * np.sqrt(h1) * 8) / 8     # about half of the rows: Q(s') spreads by about 0.45 sqrt(h1)
    net = lambda: {"w0": grid(-4, 4, 8, h1, n_obs).astype(np.float32), "b0": grid(-4, 4, 8, h1).astype(np.float32),
                   "w1": grid(-4, 4, 8, A, h1).astype(np.float32), "b1": (grid(-4, 4, 8, A) - shift).astype(np.float32)}
    params = learner.new_params_dqn(net())
    params["q_target"] = net()
    replay = {"s": grid(-4, 4, 4, RING, n_obs), "s2": grid(-4, 4, 4, RING, n_obs), "a": rng.integers(0, A, RING), "r": grid(-8, 8, 4, RING),
              "term": rng.random(RING) < 0.2}
    cfg = learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=RING, gamma=0.5, double=double, clip_targets=clip, clip_min=-0.5, clip_max=0.25)
    return cfg, params, replay


def tie_groups(A, nested=False):
    """name -> the columns, lowest first, whose rows of W1 and entries of b1 are copies of the lowest's: an exact tie at every input.  (5, 37): one
    lane, two strides; (31, 32): neighbouring lanes across the stride boundary; (0, A - 1); at A = 256 a triple over the first, second and last
    stride.  ``nested``: (5, 37) and (31, 32) are one group of four -- a minibatch of 8 rows cannot give three disjoint groups four rows each; there
    5 wins over 31, 32 and 37, which a lane's own second column or a merge towards the higher index both break."""
    groups = {"ends": (0, A - 1), "lanes": (31, 32), "strides": (5, 37)}
    if nested:
        groups = {"ends": (0, A - 1), "lanes+strides": (5, 31, 32, 37)}
    if A == 256:
        groups["triple"] = (9, 41, 233)
    return groups


def _q64(net, x):
    d = lambda a: np.asarray(a, dtype=np.float64)
    return np.maximum(d(x) @ d(net["w0"]).T + d(net["b0"]), 0) @ d(net["w1"]).T + d(net["b1"])


def tied_rows(q, groups):
    """name -> the rows of q [n][A] on which the group's columns all hold the row's maximum."""
    top = q.max(1)
    return {name: np.flatnonzero((q[:, list(cols)] == top[:, None]).all(1)) for name, cols in groups.items()}


def dqn_wide_problem(shape, double, clip, seed=None):
    """(cfg, params, replay, extra) at a shape of WIDE_A["dqn"]: ``dqn_dyadic_problem``'s grids and gamma = 0.5 with, on top,
      * ``tie_groups``' copied columns in BOTH nets, and a bonus on their b1 in the net the argmax runs on (the online net under double DQN, else the
        target net), so that each group holds the maximum at s' on rows of update 0's minibatch;
      * b1 of both nets shifted down by the median of the minibatch rows' maxima (to a multiple of 1/8, plus 1/16: no maximum is 0), so that about
        half of the rows have only negative Q(s');
      * stored actions set by hand on update 0's rows: pushed as A + 3 and -2 (the ring must hold A - 1 and 0), 31, 32 and one column in every
        output tile not yet reached;
      * clip_min and clip_max set to the second smallest and the second largest gamma * Qt(s', a*) of the live minibatch rows: one row lands exactly
        on each bound and at least one beyond each.
    ``extra``: groups, the minibatch's ring indices, the hand-set (ring row, pushed action, stored action) triples, and observations for acting
    (WIDE_ACT_ROWS rows of the same grid).  The acting problem's groups are never nested: its net is ``acting_net`` (the bonus and the copies in
    the online net, whatever ``double`` is)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, B = shape
    rng = np.random.default_rng(WIDE_DQN_SEEDS[tuple(shape), bool(double)] if seed is None else seed)
    grid = lambda lo, hi, den, *sh: rng.integers(lo, hi + 1, size=sh).astype(np.float64) / den
    net = lambda: {"w0": grid(-4, 4, 8, h1, n_obs).astype(np.float32), "b0": grid(-4, 4, 8, h1).astype(np.float32),
                   "w1": grid(-4, 4, 8, A, h1).astype(np.float32), "b1": grid(-4, 4, 8, A).astype(np.float32)}
    q, qt = net(), net()
    base = {k: v.copy() for k, v in q.items()}
    replay = {"s": grid(-4, 4, 4, RING, n_obs), "s2": grid(-4, 4, 4, RING, n_obs), "a": rng.integers(0, A, RING), "r": grid(-8, 8, 4, RING),
              "term": rng.random(RING) < 0.2}
    act_obs = grid(-4, 4, 4, WIDE_ACT_ROWS, n_obs).astype(np.float32)
    bonus = np.float32(np.round(WIDE_BONUS * 0.45 * np.sqrt(h1) * 8) / 8)

    def tie(n, groups, boost):
        n = {k: v.copy() for k, v in n.items()}
        for cols in groups.values():
            for c in cols[1:]:
                n["w1"][c], n["b1"][c] = n["w1"][cols[0]], n["b1"][cols[0]]
            if boost:
                n["b1"][list(cols)] += bonus
        return n

    def drop(n, x):                                                 # the shift of b1: the median row maximum of n on x, a multiple of 1/8, plus 1/16
        return np.float32(np.round(np.median(_q64(n, x).max(1)) * 8) / 8 + 0.0625)

    def lowered(n, by):
        return dict(n, b1=(n["b1"] - by).astype(np.float32))

    groups = tie_groups(A, nested=B < 12)
    idx = learner.sample_indices_host(LEARNER_SEED, 0, B, RING)
    uniq = list(dict.fromkeys(int(i) for i in idx))
    pushed = [A + 3, -2, 31, 32]
    pushed += [16 * t + 7 for t in range((A + 15) // 16) if t not in {min(max(a, 0), A - 1) // 16 for a in pushed}]
    assert len(uniq) >= len(pushed), (len(uniq), len(pushed))
    hand = [(r, a, min(max(a, 0), A - 1)) for r, a in zip(uniq, pushed)]
    for r, a, _ in hand:
        replay["a"][r] = a
    q, qt = tie(q, groups, double), tie(qt, groups, not double)
    shift = drop(q if double else qt, replay["s2"][idx])
    q, qt = lowered(q, shift), lowered(qt, shift)
    params = learner.new_params_dqn(q)
    params["q_target"] = qt
    mk = lambda lo, hi: learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=RING, gamma=0.5, double=double, clip_targets=clip, clip_min=lo, clip_max=hi)
    batch = learner.dqn_batch_from_rows(rows_of(replay, n_obs, A)[idx], n_obs)
    g = 0.5 * learner.dqn_targets_host(params, batch, mk(-1.0, 1.0), "float64")[:, 1]
    vals = np.unique(g[batch["mask"] > 0])
    if seed is None:
        assert vals.size >= 4, vals                                 # (a committed seed; a seed under search may fail it, and dqn_wide_counts_ok says so)
    lo, hi = (float(vals[1]), float(vals[-2])) if vals.size >= 4 else (-0.5, 0.25)
    acting = tie_groups(A)
    extra = {"groups": groups, "idx": idx, "hand": hand, "act_obs": act_obs, "act_groups": acting, "acting_net": lowered(tie(base, acting, True), drop(tie(base, acting, True), act_obs))}
    return mk(lo, hi), params, replay, extra


def dqn_wide_counts(shape, double, seed=None):
    """What ``dqn_wide_problem`` must produce, counted from the float64 twin alone: rows of update 0's minibatch per tie group (the group holds the
    maximum of the net the argmax runs on), rows whose real Q(s') are all negative and rows where not, rows where the online net's a* is not the
    target net's own argmax, live rows exactly on and beyond each clip bound, rows in the linear branch of the loss, terminated rows, the acting
    observations per tie group, and the widest stage of ``dqn_exactness_bits``."""
    from rl_mpc_lanemerging_amd import learner
    cfg, params, replay, extra = dqn_wide_problem(shape, double, True, seed)
    batch = learner.dqn_batch_from_rows(rows_of(replay, cfg.n_obs, cfg.n_actions)[extra["idx"]], cfg.n_obs)
    qn, qtn = _q64(params["q"], batch["s2"]), _q64(params["q_target"], batch["s2"])
    arg = qn if double else qtn
    _, info = learner.update_host_dqn(params, batch, cfg, "float64", grads_only=True)
    g, live = 0.5 * info["targets"][:, 1], batch["mask"] > 0
    raw = 0.5 * qtn[np.arange(cfg.batch), arg.argmax(1)]
    out = {"tie " + k: int(v.size) for k, v in tied_rows(arg, extra["groups"]).items()}
    out.update({"act " + k: int(v.size) for k, v in tied_rows(_q64(extra["acting_net"], extra["act_obs"]), extra["act_groups"]).items()})
    out.update({"all negative": int((arg < 0).all(1).sum()), "not all negative": int((~(arg < 0).all(1)).sum()),
                "online != target": int((qn.argmax(1) != qtn.argmax(1)).sum()), "on clip_min": int((raw[live] == cfg.clip_min).sum()),
                "on clip_max": int((raw[live] == cfg.clip_max).sum()), "below clip_min": int((raw[live] < cfg.clip_min).sum()),
                "above clip_max": int((raw[live] > cfg.clip_max).sum()), "|td| > 1": int((np.abs(info["td"]) > 1).sum()), "terminated": int((~live).sum()),
                "act all negative": int((_q64(extra["acting_net"], extra["act_obs"]) < 0).all(1).sum()),
                "bits": max(dqn_exactness_bits(params, batch, cfg).values())})
    assert np.array_equal(g, raw)
    return out


def dqn_wide_counts_ok(shape, double, c):
    """The conditions on ``dqn_wide_counts``: at least 4 rows per tie group (at s', of update 0), at (20, 32, 40, 16) at least 4 rows all negative
    and 4 not, under double DQN at least 4 rows where online and target argmax differ, both clip bounds met exactly and passed,
    a row in the loss's linear branch, a terminated row, every group tied on acting observations, and every partial sum below 24 bits."""
    ok = all(v >= 4 for k, v in c.items() if k.startswith("tie ")) and all(v >= 2 for k, v in c.items() if k.startswith("act "))
    if shape[2] == 40:
        ok &= c["all negative"] >= 4 and c["not all negative"] >= 4 and c["act all negative"] >= 4
    if double:
        ok &= c["online != target"] >= 4
    return bool(ok and min(c["on clip_min"], c["on clip_max"], c["below clip_min"], c["above clip_max"], c["|td| > 1"], c["terminated"]) >= 1
                and c["bits"] < 24)


def dqn_exactness_bits(params, batch, cfg):
    """``learner_testlib.exactness_bits``' measure for one DQN update: per stage of the three forward passes (online on s and s', target on s'),
    of y and diff, of the backward pass and of the weight gradients, log2 of (the largest sum of |a| |b| over the summed index) / (the unit every
    product is a multiple of).  Below 24, every partial sum of every summation order is a float32 number."""
    from learner_testlib import frac_bits
    from rl_mpc_lanemerging_amd import learner
    d = lambda a: np.asarray(a, dtype=np.float64)
    bits, B = {}, len(batch["r"])

    def stage(name, a, b, bias=None):                             # a [m][k] @ b [k][n] (+ bias [n])
        a, b = d(a), d(b)
        e = frac_bits(a) + frac_bits(b)
        s = np.abs(a) @ np.abs(b)
        if bias is not None:
            e, s = max(e, frac_bits(bias)), s + np.abs(d(bias))
        bits[name] = float(np.log2(max(s.max(), 2.0 ** -e) * 2.0 ** e))

    hidden = {}
    for name, net, x in (("online s", params["q"], batch["s"]), ("online s'", params["q"], batch["s2"]), ("target s'", params["q_target"], batch["s2"])):
        h = np.maximum(d(x) @ d(net["w0"]).T + d(net["b0"]), 0)
        stage(name + " z1", x, d(net["w0"]).T, net["b0"])
        stage(name + " Q", h, d(net["w1"]).T, net["b1"])
        hidden[name] = h
    _, info = learner.update_host_dqn(params, batch, cfg, "float64", grads_only=True)
    tg, a = info["targets"], np.asarray(batch["a"], dtype=np.int64)
    stage("y", np.stack([d(batch["r"]), cfg.gamma * tg[:, 1], d([cfg.clip_min] * B), d([cfg.clip_max] * B)], 1), np.ones((4, 1)))
    stage("diff", np.stack([info["q_values"], tg[:, 2]], 1), np.ones((2, 1)))
    dz = np.clip(info["td"], -1, 1) / B
    h1 = hidden["online s"]
    dzout = np.zeros((B, cfg.n_actions))
    dzout[np.arange(B), a] = dz
    dz1 = dz[:, None] * d(params["q"]["w1"])[a] * (h1 > 0)
    stage("dZ1", np.abs(dz1).reshape(-1, 1), np.ones((1, 1)))
    for name, left, right in (("dW1", dzout, h1), ("db1", dzout, np.ones((B, 1))), ("dW0", dz1, d(batch["s"])), ("db0", dz1, np.ones((B, 1)))):
        stage(name, left.T, right)
    return bits


# ---- problems and their host twins ---------------------------------------------------------------------------------------------------------------
def problem_net(head, shape, rng, neg_shift=False):
    """The head's net at nn.Linear scale; with atoms the last layer is scaled by 3 (logits that spread: distributions away from uniform).
    ``neg_shift``: the last layer's bias tilts every action's distribution a little towards its low atoms -- the plain head's A blocks, the dueling
    head's VALUE block (a tilt of the advantage blocks would cancel in the head)."""
    n = head.net(shape, rng)
    if head.atoms:
        _, _, A, K, _ = head.dims(shape)
        n["w1"] = (n["w1"] * 3).astype(np.float32)
        if neg_shift:
            b1 = n["b1"].reshape(A + head.dueling, K).astype(np.float64)
            b1[A if head.dueling else slice(None)] -= NEG_TILT * np.linspace(-1, 1, K)
            n["b1"] = b1.reshape(-1).astype(np.float32)
    else:
        assert not neg_shift
    return n


def random_problem(head, shape, seed, neg_shift=False, **kw):
    """(cfg, params, replay): the head's nets with a target that differs, RING replay rows.  ``neg_shift`` (heads with atoms): the support is
    [-4, 4] and the bias tilt of ``problem_net``, so that on a part of the rows every real expected value at s' is negative (a pad column's logits
    of 0 would mean the support's centre, 0: above them all).  The generator's call order is the two nets, then s, s2, a, r, term."""
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A, K, B = head.dims(shape)
    rng = np.random.default_rng(seed)
    base = dict(n_obs=n_obs, n_actions=A, h1=h1, batch=B, capacity=RING, lr=1e-3)
    if head.atoms:
        base.update(n_atoms=K, **(dict(v_min=-4.0, v_max=4.0) if neg_shift else dict(v_min=-10.0, v_max=10.0)))
    if head.dueling:
        base["dueling"] = True
    cfg = head.config(**dict(base, **kw))
    params = learner.new_params_dqn(problem_net(head, shape, rng, neg_shift))
    params["q_target"] = problem_net(head, shape, rng, neg_shift)
    replay = {"s": rng.normal(size=(RING, n_obs)).astype(np.float32), "s2": rng.normal(size=(RING, n_obs)).astype(np.float32), "a": rng.integers(0, A, RING),
              "r": rng.normal(size=RING) * 2, "term": rng.random(RING) < 0.2}
    return cfg, params, replay


def rows_of(replay, n_obs, A=None):
    """The ring rows the push kernel writes for ``replay`` pushed into an empty ring.  ``A``: the action count, where the pushed indices leave
    0 ... A - 1 (the push clamps them)."""
    c = capi()
    R = replay["s"].shape[0]
    rows = np.zeros((R, c.DDPG_ROW), dtype=np.float32)
    rows[:, :n_obs], rows[:, 32:32 + n_obs] = replay["s"], replay["s2"]
    rows[:, 64], rows[:, 65], rows[:, c.DQN_ACTION_COL] = replay["r"], np.where(replay["term"], 0, 1), replay["a"] if A is None else np.clip(replay["a"], 0, A - 1)
    return rows


def minibatch_host(replay, cfg, seed=LEARNER_SEED, update=0):
    from rl_mpc_lanemerging_amd import learner
    rows = rows_of(replay, cfg.n_obs, cfg.n_actions)[learner.sample_indices_host(seed, update, cfg.batch, replay["s"].shape[0])]
    return rows, learner.dqn_batch_from_rows(rows, cfg.n_obs)


def twins(head, params, batch, cfg, **kw):
    """The info dicts of the head's host twin in float64 and in float32, gradients only."""
    return tuple(head.twin(params, batch, cfg, d, grads_only=True, **kw)[1] for d in ("float64", "float32"))


def pad_mask(n_obs, h1, n_out):
    """True at the pad entries of a padded slot {w0 [h1p][32], b0 [h1p], w1 [Ap][h1p], b1 [Ap]}."""
    h1p, Ap = (h1 + 15) & ~15, (n_out + 15) & ~15
    m = {"w0": np.ones((h1p, 32), bool), "b0": np.ones(h1p, bool), "w1": np.ones((Ap, h1p), bool), "b1": np.ones(Ap, bool)}
    m["w0"][:h1, :n_obs], m["b0"][:h1], m["w1"][:n_out, :h1], m["b1"][:n_out] = False, False, False, False
    return m


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


def expected_values_host(net, obs, cfg):
    """{"float64", "float32"}: the expected values [n][A] of a C51 net (plain or dueling, as ``cfg`` says) on ``obs``, from the twins' own logits."""
    import torch
    from rl_mpc_lanemerging_amd import learner
    kw = dict(dueling=True) if cfg.dueling else {}
    ev = {}
    for d in ("float64", "float32"):
        T = lambda a: torch.tensor(np.asarray(a), dtype=getattr(torch, d))
        with torch.no_grad():
            p = torch.softmax(learner._c51_logits({k: T(net[k]) for k in NAMES}, T(obs), cfg.n_actions, cfg.n_atoms, **kw), -1)
            ev[d] = (p * T(learner.c51_support(cfg))).sum(-1).numpy()
    return ev


# ---- the dueling head's independent statement ------------------------------------------------------------------------------------------------------
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


# ---- a lone learner on the device ----------------------------------------------------------------------------------------------------------------
def fill(L, replay, rows=slice(None), chunk=64):
    """Push the replay dict's rows (s, a, r, s2, term and, if there, trunc), ``chunk`` at a time."""
    rep = {k: v[rows] for k, v in replay.items()}
    R = rep["s"].shape[0]
    for o in range(0, R, chunk):
        sl = slice(o, min(R, o + chunk))
        term = rep["term"][sl]
        trunc = rep["trunc"][sl] if "trunc" in rep else np.zeros_like(term)
        L.push(to_device(rep["s"][sl].astype(np.float32)), None, to_device(rep["a"][sl].astype(np.int32)), to_device(rep["r"][sl].astype(np.float64)),
               to_device(rep["s2"][sl].astype(np.float32)), to_device(term), to_device(trunc))


def make_learner(gpu_ctx, head, cfg, params, replay=None, seed=LEARNER_SEED, **kw):
    L = head.learner((cfg.n_obs, cfg.n_actions), cfg, seed=seed, init=params["q"], ctx=gpu_ctx, **kw)
    L.load_state_dict({"params": params, "counters": None})
    if replay is not None:
        fill(L, replay)
    return L


def pads_are_zero(gpu_ctx, head, L, slots, pad, tag):
    """The padded arrays themselves (``<prefix>_padded_read``): every pad entry of every slot is an exact zero, every entry finite."""
    for slot in slots:
        arr = getattr(gpu_ctx, head.prefix + "_padded_read")(L.handle, slot, L.cfg.h1, head.cfg_width(L.cfg))
        for k in NAMES:
            assert arr[k].shape == pad[k].shape and not arr[k][pad[k]].any(), (tag, slot, k, int(np.count_nonzero(arr[k][pad[k]])))
            assert np.isfinite(arr[k]).all()


# ---- snapshots -------------------------------------------------------------------------------------------------------------------------------------
def snapshot(gpu_ctx, head, L, stats):
    sd = L.state_dict()
    return {"params": sd["params"], "counters": sd["counters"], "ring": getattr(gpu_ctx, head.prefix + "_pop_replay_read")(L.handle, 0, L.cfg.capacity),
            "stats": stats}


def stats_row(s, m=None):
    return [float(s[k] if m is None else s[k][m]) for k in ("loss", "mean_q", "fill", "updates")]


def same_slots(a, b, slots=Q_SLOTS):
    return all(np.array_equal(bits(a[s][k]), bits(b[s][k])) for s in slots for k in NAMES)


def assert_same(a, b, label):
    """Two snapshots: all four slots, the beta powers, the counters, the ring and the statistics row, bit for bit."""
    for slot in Q_SLOTS:
        for k in NAMES:
            assert np.array_equal(bits(a["params"][slot][k]), bits(b["params"][slot][k])), (label, slot, k)
    assert np.array_equal(bits(a["params"]["beta_pow"]), bits(b["params"]["beta_pow"])) and a["params"]["beta_pow"].shape == (2,), (label, "beta_pow")
    assert np.array_equal(a["counters"], b["counters"]), (label, a["counters"], b["counters"])
    assert np.array_equal(bits(a["ring"]), bits(b["ring"])), (label, "ring")
    assert np.array_equal(bits64(a["stats"]), bits64(b["stats"])), (label, a["stats"], b["stats"])


# ---- synthetic rings: rows pushed through a stub env -------------------------------------------------------------------------------------------------
def stub_env(gpu_ctx, n, n_obs, A, table=None):
    """What a discrete population asks of an env, without one."""
    return types.SimpleNamespace(n=n, obs_dim=n_obs, continuous=False, ctx=gpu_ctx, action_space={"n": A}, env_id="sumo-jerk-v0",
                                 cfg=types.SimpleNamespace(_actions=list(np.linspace(-4.75, 4.75, A) if table is None else table)))


def feed(L, step, rows=slice(None)):
    L.push(to_device(step["obs"][rows]), None, to_device(step["action"][rows]), to_device(step["reward"][rows]), to_device(step["next_obs"][rows]),
           to_device(step["terminated"][rows]), to_device(step["truncated"][rows]))


def syn_steps(head, shape, P, pushes, n, draw_all=False):
    """``pushes`` whole-env steps of random transitions (numpy) for P members of n rows each, the same for every caller.  ``draw_all``: the first
    P * n rows of a draw of 3 * n, so that member 0's slice does not depend on P (test_c51_pop.py's order; test_dqn_pop.py draws P * n)."""
    n_obs, _, A, _, _ = head.dims(shape)
    rng = np.random.default_rng(77)
    N = (3 if draw_all else P) * n
    steps = [{"obs": rng.normal(size=(N, n_obs)).astype(np.float32), "next_obs": rng.normal(size=(N, n_obs)).astype(np.float32),
              "action": rng.integers(0, A, N).astype(np.int32), "reward": rng.normal(size=N) * 2, "terminated": rng.random(N) < 0.2,
              "truncated": rng.random(N) < 0.1} for _ in range(pushes)]
    return [{k: v[:P * n] for k, v in s.items()} for s in steps]


# ---- a population on a real env next to lone learners on its slices --------------------------------------------------------------------------------
def run_population(gpu_ctx, head, shape, P, *, seeds, eps, replay_start, steps=STEPS, alone=True, **member_overrides):
    """``steps`` steps of act -> env.step -> push -> update(1) of a population of P on one env of P * N_PER and, if ``alone``, of the same learners
    as lone learners on their slices, fed the same transitions.  ``member_overrides``: per-member sequences on top of ``head.cfg``.  Returns the
    members' snapshots (the population's)."""
    import torch
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import vec_env
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    n, A = N_PER, shape[2]
    env = vec_env.MergeVecEnv(P * n, env_id="sumo-jerk-v0" if A == 5 else "sumo-accel-v0", seed=7, ctx=gpu_ctx)
    mk = lambda: [head.cfg(shape, m, capacity=CAP, replay_start=replay_start[m], lr=LR[m], **{k: v[m] for k, v in member_overrides.items()}) for m in range(P)]
    cfgs = mk()
    pop = head.population(env, cfgs, seeds=list(seeds[:P]))
    assert getattr(gpu_ctx, head.prefix + "_pop_size")(pop.handle) == P == len(pop) and all(c.n_actions == A for c in cfgs) and all(c.n_actions == A for c in pop.cfgs)
    assert all(isinstance(pop.member(m), head.learner) and pop.member(m).env_id == env.env_id for m in range(P))
    assert all(np.array_equal(pop.member(m).action_values, np.array(env.cfg._actions, dtype=np.float64)) for m in range(P))
    lone = [head.learner(env, c, seed=seeds[m]) for m, c in enumerate(mk())] if alone else []
    sl = [slice(m * n, (m + 1) * n) for m in range(P)]
    lr, eps = list(LR[:P]), list(eps[:P])
    obs = env.reset()
    for i in range(steps):
        action = pop.act(obs, None, eps=eps).clone()
        assert action.dtype == torch.int32 and action.shape == (P * n,)
        if alone:
            a_lone = torch.cat([lone[m].act(obs[sl[m]], None, eps=eps[m]) for m in range(P)])
            assert torch.equal(action, a_lone), "actions of step %d" % i              # before the env sees them
        nobs, r, term, trunc, info = env.step(action)
        fin = info["final_observation"]
        pop.push(obs, None, action, r, nobs, term, trunc, final_obs=fin)
        pop.update(1, lr=lr)
        for m, L in enumerate(lone):
            L.push(obs[sl[m]], None, action[sl[m]].contiguous(), r[sl[m]], nobs[sl[m]], term[sl[m]], trunc[sl[m]], final_obs=fin[sl[m]])
            L.update(1, lr=lr[m])
        obs = nobs
        # the gate is per member: updates done so far = the pushes after which MORE than replay_start frames were in
        want = [sum(1 for j in range(1, i + 2) if n * j > replay_start[m]) for m in range(P)]
        have = pop.stats()["updates"]
        assert list(have) == want, (i, list(have), want)
    torch.cuda.synchronize()
    env.check_error()
    ps = pop.stats()
    assert set(ps) == {"loss", "mean_q", "fill", "updates"} and all(len(v) == P for v in ps.values())
    assert pop.stats_device().shape == (P, 4) and pop.stats_device().dtype == torch.float64
    snaps = [snapshot(gpu_ctx, head, pop.member(m), stats_row(ps, m)) for m in range(P)]
    for m, L in enumerate(lone):
        assert_same(snaps[m], snapshot(gpu_ctx, head, L, stats_row(L.stats())), "member %d vs alone" % m)
    gpu_ctx.check_error()
    return snaps


def assert_population_run(snaps, period=PERIOD):
    """What the three members' snapshots of ``run_population`` over STEPS steps with replay_start (0, 48, CAP - 1) and eps (0, > 0, > 0) must show."""
    n = N_PER
    for m in range(3):
        c = snaps[m]["counters"]
        assert (c[0], c[1], c[4]) == ((n * STEPS) % CAP, CAP, n * STEPS)              # every ring wrapped
    assert [int(s["counters"][2]) for s in snaps] == [12, 10, 4] == [int(s["params"]["updates"]) for s in snaps]
    assert [int(s["counters"][3]) for s in snaps] == [0, 12, 12]                      # eps = 0 is no exploring call: member 0's acting counter stays
    for m, s in enumerate(snaps):                                   # the hard copy follows the member's own count and period
        synced = all(np.array_equal(bits(s["params"]["q_target"][k]), bits(s["params"]["q"][k])) for k in NAMES)
        assert synced == (int(s["counters"][2]) % period[m] == 0), (m, synced)
        assert np.isfinite(s["stats"]).all() and all(np.isfinite(s["params"][slot][k]).all() for slot in Q_SLOTS for k in NAMES)
        assert all(np.abs(s["params"]["q_m"][k]).max() > 0 for k in NAMES), m
    assert not np.array_equal(snaps[0]["ring"], snaps[1]["ring"]) and not np.array_equal(snaps[0]["params"]["q"]["w1"], snaps[2]["params"]["q"]["w1"])
    # Adam stepped once per update: the beta powers, float32 running products of 0.9, say so
    assert [round(float(np.log(s["params"]["beta_pow"][0]) / np.log(np.float32(0.9)))) for s in snaps] == [12, 10, 4]


# ---- the policies (actor.DQNActor, actor.C51Actor, actor.QActorPopulation) ----------------------------------------------------------------------------
NETS = [(20, 16, 5), (20, 48, 20), (20, 256, 5)]      # (n_obs, h1, A) of the Q policies
ROWS = [1, 16, 17, 33]                                # a lone row, a full tile, a tile plus one row, two tiles plus one
JERKS = np.array([-5.0, -2.5, 0.0, 2.5, 5.0])         # JERK_VALUES_DQN
SENTINEL, TAIL = -7.0, 3                              # every output buffer has TAIL rows beyond N, filled with the sentinel
OUT = ("feat", "q", "action", "jerk")
# (n_in, h1, A, K) of the C51 policies: K below, just above and well above one 32-lane pass; A K = 85, 99, 1020, 255 leave pad columns in the last
# 16-column tile
C51_ACTOR_SHAPES = [(20, 16, 5, 17), (20, 32, 3, 33), (20, 48, 20, 51), (20, 256, 5, 51)]
SUPPORT = (-10.0, 10.0)
NEGATIVE_SUPPORT = (-10.0, -1.0)                    # wholly below zero: a pad column's logits of 0 would mean an expected value above every real one
# test_c51actor_cpu.py asserts that under this seed the float64 twin alone keeps at least 99 % of the rows at every shape (top-two gap > 1e-9)
TWIN_SEED = 3
TWIN_ROWS = 400


def dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def policy_states(n):
    """(S, n states as contiguous device tensors: the golden's 72 from the first on, repeated as often as n needs)."""
    import torch
    g, S = actor_settings()
    st = actor_states(g, dev())
    rows = torch.arange(n, device=dev()) % st["k"].shape[0]
    return S, {k: v[rows].contiguous() for k, v in st.items()}


def actor_table(A, m=0, accel=False):
    """Member m's action table (a lone policy is member 0): every member has its own; an acceleration-mode table stays within +-0.1, so that with ego
    accelerations of -20, 0 and +20 a row is clipped at either edge or not at all whatever its action is."""
    if accel:
        return np.linspace(-0.1, 0.1, A) + 0.001 * m
    return (JERKS.copy() if A == 5 else np.linspace(-4.75, 4.75, A)) + 0.125 * m


def q_dyadic_case(shape, n, seed=0):
    """(net, settings, states as numpy) whose every product and partial sum is a float32 number.  Weights: ``dyadic_net``'s value sets (three
    entries of {-1, -1/2, 1/2, 1} per row, biases multiples of 1/2); the state vector is not normalised (NORMALIZE_VECTOR_INPUT False) and every
    state entry is a multiple of 1/4 in [-4, 4]."""
    from learner_testlib import dyadic_net
    n_obs, h1, A = shape
    rng = np.random.default_rng(40 + seed)
    S = types.SimpleNamespace(MAX_SPEED=8.0, SENSOR_RADIUS=16.0, CARS_AHEAD=2, CARS_BEHIND=2, USE_ACCELERATION_OF_OTHER_CARS=True, USE_SPEED_DIFFERENCE=True,
                              NORMALIZE_VECTOR_INPUT=False, TICK_LENGTH=0.25, MINIMUM_NEGATIVE_JERK=-4.0, MAXIMUM_POSITIVE_JERK=2.0)
    net = {k: v for k, v in dyadic_net(rng, n_obs, h1, A, 1.0).items() if k in NAMES}
    quarter = lambda lo, hi, *sh: rng.integers(4 * lo, 4 * hi + 1, sh) / 4.0
    K = 4
    ox = quarter(-4, 4, n, K)
    ox[ox == 0] = 0.25
    states = {"ego4": np.concatenate([np.zeros((n, 1)), quarter(-4, 4, n, 3)], 1),     # (x = 0, y, v, a)
              "k": np.full(n, K, np.int32), "ox": ox, "ov": quarter(-2, 2, n, K),
              "oa": quarter(-2, 2, n, K)}
    return net, S, states


def q_dyadic_features(S, states):
    from rl_mpc_lanemerging_amd import actor
    return np.stack([actor.state_vector_host(S, states["ego4"][i], states["ox"][i], states["ov"][i], states["oa"][i]) for i in range(len(states["k"]))])


def q_dyadic_finish(net, feat, groups=None):
    """From the float64 twin alone: b1 shifted down until about half of the rows have only negative Q, then the tied columns; returns (net, groups:
    name -> columns, lowest first, that hold copies of one row of W1 and entry of b1).  ``groups`` None (up to 32 actions): the action that wins
    most often is copied into the column two further on, {"tie": (j1, j2)} -- the rows it wins hold an exact tie, which the first of the two must
    take.  ``groups`` given (beyond 32 actions): the k-th most frequent winner's row and bias go to every column of group k -- a group of one
    column is a lone winner at that index --, and the winner's own column, unless it is in a group, gets b1 = -64 and never wins again."""
    from rl_mpc_lanemerging_amd import actor
    A = net["b1"].size
    q = actor.q_policy_host(net, feat, np.arange(A), "jerk")[0]
    net["b1"] = (net["b1"] - np.float32(np.round(np.median(q.max(1)) * 2) / 2 + 0.25)).astype(np.float32)      # (a multiple of 1/4: no row's maximum is 0)
    idx = actor.q_policy_host(net, feat, np.arange(A), "jerk")[1]
    if groups is None:
        win = int(np.bincount(idx, minlength=A).argmax())
        other = (win + 2) % A
        net["w1"][other], net["b1"][other] = net["w1"][win], net["b1"][win]
        return net, {"tie": (min(win, other), max(win, other))}
    winners = np.argsort(-np.bincount(idx, minlength=A), kind="stable")[:len(groups)]
    rows = [(net["w1"][w].copy(), net["b1"][w].copy()) for w in winners]
    used = {c for cols in groups.values() for c in cols}
    for w in winners:
        if int(w) not in used:
            net["b1"][w] = -64.0
    for (w1, b1), cols in zip(rows, groups.values()):
        for c in cols:
            net["w1"][c], net["b1"][c] = w1, b1
    return net, groups


Q_WIDE_ROWS = 50
Q_WIDE_VARIANTS = ("ties", "lone")


def q_dyadic_policy(shape, variant=None):
    """(net, S, states, feat, groups, named) of the Q policies' exact test.  Up to 32 actions (``variant`` None): 33 rows and the one tie of
    ``q_dyadic_finish``.  Beyond (NETS_WIDE), Q_WIDE_ROWS rows and ``variant`` "ties": ``tie_groups``' copied columns, each holding the maximum on
    rows; "lone": columns 32 and A - 1 win rows alone.  ``named``: per group the rows on which it holds the maximum and no lower column outside
    it ties by chance -- there the index must be the group's lowest column."""
    from rl_mpc_lanemerging_amd import actor
    A = shape[2]
    net, S, states = q_dyadic_case(shape, 33 if variant is None else Q_WIDE_ROWS)
    feat = q_dyadic_features(S, states)
    groups = None if variant is None else tie_groups(A) if variant == "ties" else {"32": (32,), "A - 1": (A - 1,)}
    net, groups = q_dyadic_finish(net, feat, groups)
    q, idx, _ = actor.q_policy_host(net, feat, np.arange(A), "jerk")
    named = {name: rows[idx[rows] == groups[name][0]] for name, rows in tied_rows(q, groups).items()}
    return net, S, states, feat, groups, named


def widen(P, rows=None):
    """Output buffers with TAIL rows more than the policy evaluates, all sentinel; every output kept."""
    import torch
    rows = (P.n if rows is None else rows) + TAIL
    P.feat = torch.full((rows, P.flen), SENTINEL, dtype=torch.float32, device=dev())
    P.q = torch.full((rows, P.shape[2]), SENTINEL, dtype=torch.float32, device=dev())
    P.action = torch.full((rows,), int(SENTINEL), dtype=torch.int32, device=dev())
    P.jerk = torch.full((rows,), SENTINEL, dtype=torch.float64, device=dev())
    P.keep_features = P.keep_q = True
    return P


def run_policy(P, st, step=1):
    """One evaluation through the policy's call; numpy copies of the n evaluated rows, after the check that the rows beyond them kept the sentinel in
    every output."""
    import torch
    P(step, st["ego4"], st["k"], st["ox"], st["ov"], st["oa"])
    torch.cuda.synchronize()
    out = {k: getattr(P, k).cpu().numpy().copy() for k in OUT}
    for k, v in out.items():
        assert v.shape[0] == P.n + TAIL and (v[P.n:] == SENTINEL).all(), k
    return {k: v[:P.n] for k, v in out.items()}


def policy_features(gpu_ctx, fcfg, st, n, flen):
    import torch
    feat = torch.full((n, flen), SENTINEL, dtype=torch.float32, device=dev())
    gpu_ctx.policy_features_device(fcfg, n, st["ox"].shape[1], 1, st["ego4"].data_ptr(), st["k"].data_ptr(), st["ox"].data_ptr(), st["ov"].data_ptr(),
                                   st["oa"].data_ptr(), 0, feat.data_ptr(), flen, stream())
    return feat


def act_on_features(L, feat):
    """(index int32 [n], Q or expected values float32 [n][A]) of the learner's ``act`` (eps = 0) on input vectors, as numpy."""
    import torch
    q = torch.full((feat.shape[0], L.cfg.n_actions), SENTINEL, dtype=torch.float32, device=dev())
    a = L.act(feat, eps=0.0, debug_q=q)
    torch.cuda.synchronize()
    return a.cpu().numpy().copy(), q.cpu().numpy()


def plain_policy(gpu_ctx, L, S, n):
    """A plain callable with the policy signature from the public entries: features, the learner's act, the table."""
    import torch
    fcfg = capi().FeaturesCfg.from_settings(S, time_feature=False)
    flen = L.cfg.n_obs
    table = torch.as_tensor(L.action_values, device=dev())
    feat = torch.empty(n, flen, dtype=torch.float32, device=dev())

    def policy(step, cur_ego4, k, cur_ox, cur_ov, cur_oa):
        gpu_ctx.policy_features_device(fcfg, n, cur_ox.shape[1], step, cur_ego4.data_ptr(), k.data_ptr(), cur_ox.data_ptr(), cur_ov.data_ptr(), cur_oa.data_ptr(), 0,
                                       feat.data_ptr(), flen, stream())
        return table[L.act(feat, eps=0.0).long()]
    return policy


def transitions(rng, n, n_obs, A):
    """One push of n random transitions, as the learners' ``push`` takes them."""
    t = to_device
    return (t(rng.normal(0, 1, (n, n_obs)).astype(np.float32)), None, t(rng.integers(0, A, n).astype(np.int32)), t(rng.normal(0, 1, n)),
            t(rng.normal(0, 1, (n, n_obs)).astype(np.float32)), t(rng.random(n) < 0.2), t(np.zeros(n, bool)))


# ---- the C51 policy's nets, configs and stand-ins ------------------------------------------------------------------------------------------------------
def c51_actor_net(shape, seed, spread=3.0):
    """nn.Linear-scale tensors n_in -> h1 -> A K with the last layer scaled by ``spread``: distributions away from uniform."""
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_in, h1, A, K = shape
    n = learner.init_c51_net(n_in, h1, A, K, np.random.default_rng(seed))
    n["w1"] = (n["w1"] * spread).astype(np.float32)
    return n


def zero_head(n):
    """The net with a zero last layer: every action's distribution is uniform, every expected value the support's centre -- an exact tie."""
    out = {k: v.copy() for k, v in n.items()}
    out["w1"][:], out["b1"][:] = 0, 0
    return out


def c51_actor_config(shape, support=SUPPORT, **kw):
    capi()
    from rl_mpc_lanemerging_amd import learner
    n_in, h1, A, K = shape
    kw = {**dict(batch=16, capacity=64, lr=1e-2), **kw}
    return learner.C51Config(n_obs=n_in, n_actions=A, h1=h1, n_atoms=K, v_min=support[0], v_max=support[1], **kw)


def export_file(path, n, shape, support=SUPPORT, action_values=None):
    """A file as ``C51Learner.export_q`` writes it."""
    with open(path, "wb") as fh:
        np.savez(fh, **{k: n[k] for k in NAMES}, action_values=actor_table(shape[2]) if action_values is None else action_values, n_atoms=np.int64(shape[3]),
                 v_min=np.float64(support[0]), v_max=np.float64(support[1]))
    return str(path)


class NoLibrary:
    """A context stand-in whose every attribute access fails the test: the refusals are made before any library call."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def c51_learner_stub(shape):
    """What ``actor._is_dqn_learner`` took for a DQN learner on the parent commit: ``export_q``, ``handle`` and a cfg with the DQN fields -- of a C51."""
    return types.SimpleNamespace(cfg=c51_actor_config(shape), action_values=actor_table(shape[2]), handle=NoLibrary(), export_q=lambda path: path, env_id=None,
                                 ctx=NoLibrary())


def c51_actor_stub(shape):
    capi()
    from rl_mpc_lanemerging_amd import actor
    a = actor.C51Actor.__new__(actor.C51Actor)
    a.handle, a.shape, a.ctx = None, shape[:3], NoLibrary()
    return a


# ---- one step of QCombinedShieldVecEnv from the public entries ---------------------------------------------------------------------------------
def compose_first_step(env_id, policy_of, act, n, seed, kmax, settings):
    """The env's first step after reset made from the public entries on a context of its own: stmpc_sim_init_device, stmpc_sim_view_device, the host
    twin of the first action, stmpc_rollout_step_device (step 1) + the policy's call and stmpc_rollout_step_device (steps 2 ... L),
    stmpc_combined_decide_device, the action handling's command, stmpc_sim_step_device, stmpc_policy_features_device and stmpc_env_reward_device on
    the wide view (the construction of tests/test_qshield_env.py's ``_compose`` for a step from the reset's world, where every row is in its
    episode 0).  ``policy_of(ctx)`` builds the rollout policy of ``n`` rows.  Returns obs0 and, per row, takeover, reason, executed_jerk, obs,
    reward, term, trunc, and the rolled-out ego rows."""
    import torch
    from rl_mpc_lanemerging_amd import _capi, combined, episodes, rewards, vec_env
    S = settings()
    ctx = _capi.Context(-1)
    policy = policy_of(ctx)
    params = _capi.Params.from_settings(S)
    ccfg = combined.control_cfgs([{}], sparse_control=False)[0]
    L = max(int(ccfg.rollout_length), 1)
    cfg = episodes.sim_cfg(seed, float(S.MAX_EPISODE_LENGTH))
    ecfg = vec_env.env_cfg(env_id, "Continuous", autoreset=False)
    fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=False)
    dev = lambda a, dtype=None: torch.as_tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")
    WIDE = 32
    feat, rew = z(n, 20, dtype=torch.float32), z(n)
    tick = float(S.TICK_LENGTH)
    a_min, a_max = float(S.MAX_NEGATIVE_ACCELERATION), float(S.MAX_POSITIVE_ACCELERATION)

    def view(K):
        b = (z(n, 5), z(n, dtype=torch.int32), z(n, K), z(n, K), z(n, K))
        ctx.sim_view(cfg, n, K, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), b[4].data_ptr())
        return b

    def features(b):
        e4 = b[0][:, :4].contiguous()
        assert int(b[1].max()) < WIDE
        ctx.policy_features_device(fcfg, n, WIDE, 1, e4.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), b[4].data_ptr(), 0, feat.data_ptr(), 20)
        return e4, feat.cpu().numpy().copy()

    ctx.sim_init(cfg, n)
    out = {"obs0": features(view(WIDE))[1]}
    b = view(kmax)
    e5 = b[0].cpu().numpy()
    fa, bad = vec_env.q_first_action_host(env_id, act, e5[:, 3], S)
    assert not bad.any()
    first = dev(fa, torch.float64)
    cur4, cox, cov, coa = b[0][:, :4].clone().contiguous(), b[2].clone(), b[3].clone(), b[4].clone()
    for step in range(1, L + 1):
        a = first if step == 1 else policy(step, cur4, b[1], cox, cov, coa)
        ctx.rollout_step_device(params, ccfg, n, kmax, step, b[0].data_ptr(), cur4.data_ptr(), b[1].data_ptr(), cox.data_ptr(), cov.data_ptr(), coa.data_ptr(), a.data_ptr())
    take_d, reason_d, speed_d = z(n, dtype=torch.int32), z(n, dtype=torch.int32), z(n)
    ctx.combined_decide_device(params, ccfg, n, kmax, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), cur4.data_ptr(), cox.data_ptr(), cov.data_ptr(),
                               first.data_ptr(), 0, take_d.data_ptr(), reason_d.data_ptr(), speed_d.data_ptr())
    take, speed = take_d.cpu().numpy() != 0, speed_d.cpu().numpy().copy()
    handled = [rewards.handle_action(env_id, float(e5[i, 2]), float(e5[i, 3]), 0.0, int(act[i])) for i in range(n)]
    cmd, pj, inv = (np.array([h[i] for h in handled]) for i in range(3))
    out.update(takeover=take, reason=reason_d.cpu().numpy().copy(), rolled=cur4.cpu().numpy().copy(),
               executed_jerk=np.where(take, (np.clip((speed - e5[:, 2]) / tick, a_min, a_max) - 0.0) / tick, pj))
    d_speed = dev(np.where(take, speed, cmd))
    ctx.sim_step(params, cfg, n, d_speed.data_ptr())
    status, _, _, ego4 = ctx.sim_read(n)
    wide = view(WIDE)
    e4, f = features(wide)
    crashed, arrived = status == 2, status == 1
    jerk = np.where(crashed | arrived, out["executed_jerk"], (ego4[:, 3] - 0.0) / tick)
    d_jerk, d_cr, d_ar = dev(jerk), dev(crashed.astype(np.int32)), dev(arrived.astype(np.int32))
    ctx.env_reward(ecfg, n, WIDE, e4.data_ptr(), wide[1].data_ptr(), wide[2].data_ptr(), d_jerk.data_ptr(), d_cr.data_ptr(), d_ar.data_ptr(), rew.data_ptr())
    out.update(obs=f, reward=rew.cpu().numpy().copy() + inv, term=crashed | arrived, trunc=status == 3, status=status)
    ctx.check_error()
    ctx.close()
    return out
