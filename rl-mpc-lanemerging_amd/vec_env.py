"""Batched on-device RL training environment for the merge world: the reference's gym environments (merge_gym.py: ``sumo-jerk-continuous-v0``
= ContinuousJerkEnv, ``sumo-jerk-v0`` = JerkEnv, ``sumo-accel-v0`` = AccelerationEnv) with the rewards of ``dqn.get_reward_function``
(dqn.py:449-563, rl.py:168-174), for ``n`` environments of the SUMO-free world (episodes.py) stepped in lock-step on one GPU.

``MergeVecEnv`` follows the call shape of a gym / gymnasium vector env (neither is imported): ``reset() -> obs``,
``step(action) -> obs, reward, terminated, truncated, info``, all torch device tensors; ``step`` never synchronises with the host
(one exception, by request: ``shield_sparse=True``, see ``MergeVecEnv``).
Finished environments start their next episode in the same step (``autoreset``); ``info["final_observation"]`` / ``info["final_stats"]``
hold what the finished episode returned in the rows where ``terminated | truncated``.  ``drain_episode_stats()`` is the one sync point.

Differences from the reference, by design: the reset state is the world's start state (the traffic in its stationary state, the ego at the
ramp's start), not the reference's 20 s warm-up plus one tick (merge_gym.py:142-150) -- as ``episodes.EpisodeRunner`` starts; the observation
has no TimeFeature input (that wraps the agent, not the env: ddpg.py:41); the world is a restatement, not SUMO, so
whole-episode outcomes are not the reference's, while rewards, actions and observations are pinned to it.
"""
import functools
import weakref

import numpy as np

from . import _capi, episodes, groups
from .config import Settings

ENV_IDS = {"sumo-jerk-continuous-v0": _capi.ENV_CONTINUOUS_JERK, "sumo-jerk-v0": _capi.ENV_JERK, "sumo-accel-v0": _capi.ENV_ACCELERATION}
REWARD_IDS = {"Continuous": _capi.REWARD_CONTINUOUS, "Slotted": _capi.REWARD_SLOTTED, "Slotted Jerk": _capi.REWARD_SLOTTED_JERK, "ST": _capi.REWARD_ST}
_M64 = 0xFFFFFFFFFFFFFFFF
_owners = weakref.WeakKeyDictionary()       # context -> the MergeVecEnv whose world it holds (a context holds one world)


def episode_seed(seed, episode):
    """Seed of episode ``episode`` of an environment in a run seeded ``seed`` (``stmpc_env_episode_seed``; 0: the seed itself)."""
    if episode == 0:
        return int(seed) & _M64
    return groups.splitmix64((int(seed) + 0x9E3779B97F4A7C15 * int(episode)) & _M64)


def traffic_mix_cum(weights):
    """The cumulative weights of a traffic mix as ``stmpc_traffic_mix_env_reset_device`` forms them: the running sum of ``w / sum(w)`` in fp64, left to
    right, and exactly 1.0 from the last type of positive weight on -- so ``cum[-1] == 1.0`` and a type of weight 0 is never drawn, wherever it stands.
    A list of floats.  ValueError unless there are 1 ... ``TRAFFIC_MIX_MAX`` weights, each finite and >= 0, with a positive (finite) sum."""
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError("mix_weights must be a sequence of numbers, not %r" % (weights,))
    if not 1 <= len(w) <= _capi.TRAFFIC_MIX_MAX:
        raise ValueError("a traffic mix has 1 ... %d weights, not %d" % (_capi.TRAFFIC_MIX_MAX, len(w)))
    total, last = 0.0, -1
    for t, x in enumerate(w):
        if not (x >= 0.0 and x != float("inf")):
            raise ValueError("mix_weights must be finite and not negative, not %r (type %d)" % (x, t))
        total += x                               # (an explicit loop: the built-in sum() of floats is compensated, the C entry's is not)
        if x > 0.0:
            last = t
    if not (total > 0.0 and total != float("inf")):
        raise ValueError("mix_weights must have a positive, finite sum")
    cum, run = [], 0.0
    for t, x in enumerate(w):
        run += x / total
        cum.append(1.0 if t >= last else run)
    return cum


def traffic_mix_draw(mix_seed, env, episode, cum):
    """The traffic type of episode ``episode`` of environment ``env`` in a mix seeded ``mix_seed`` (``stmpc_traffic_mix_draw`` and the kernels, in
    Python integers): the first t with ``u < cum[t]``, u = the world's ``uniform01(mix_seed, env, ctr=episode)`` -- splitmix64 of
    ``mix_seed + gamma * (env * (2**32 + 1) + episode + 1)``, its top 53 bits over 2**53."""
    z = groups.splitmix64((int(mix_seed) + 0x9E3779B97F4A7C15 * (int(env) * 0x100000001 + (int(episode) & 0xFFFFFFFF) + 1)) & _M64)
    u = (z >> 11) * (1.0 / 9007199254740992.0)
    t = 0
    while t < len(cum) - 1 and not u < cum[t]:
        t += 1
    return t


def env_cfg(env_id=None, reward=None, autoreset=True, S=Settings, log_capacity=0):
    """``stmpc_env_cfg`` for ``env_id`` / ``reward`` (default: Settings.GYM_ENVIRONMENT / Settings.REWARD_FUNCTION); ValueError for unknown names."""
    env_id = S.GYM_ENVIRONMENT if env_id is None else env_id
    reward = S.REWARD_FUNCTION if reward is None else reward
    if env_id not in ENV_IDS:
        raise ValueError("Invalid gym environment {} (one of {})".format(env_id, ", ".join(ENV_IDS)))
    if reward not in REWARD_IDS:
        raise ValueError("Invalid reward function {} specified in settings.".format(reward))        # dqn.get_reward_function, dqn.py:460
    table = None
    if env_id == "sumo-jerk-v0":
        table = [S.JERK_VALUES_DQN[i] for i in range(len(S.JERK_VALUES_DQN))]
    elif env_id == "sumo-accel-v0":
        table = [S.ACCELERATION_VALUES_DQN[i] for i in range(len(S.ACCELERATION_VALUES_DQN))]
    return _capi.EnvCfg.from_settings(S, ENV_IDS[env_id], REWARD_IDS[reward], table, autoreset, log_capacity)


#: what a reward group may set: ``REWARD_FUNCTION`` and these ``Settings`` names -> the ``stmpc_env_cfg`` fields that may differ between reward groups
REWARD_GROUP_KEYS = {"CRASH_REWARD": "crash_reward", "SUCCESS_REWARD": "success_reward", "TIME_REWARD": "time_reward", "WT_SMOOTH": "wt_smooth",
                     "WT_SAFE": "wt_safe", "WT_EFFICIENT": "wt_efficient", "ALT_V_WEIGHT": "alt_v_weight", "ALT_A_WEIGHT": "alt_a_weight",
                     "ALT_J_WEIGHT": "alt_j_weight", "ALT_D_WEIGHT": "alt_d_weight", "MIN_FOLLOW_DISTANCE": "min_follow_distance",
                     "DESIRED_SPEED": "desired_speed", "INVALID_ACTION_PENALTY": "invalid_action_penalty"}


def reward_cfgs(rewards, env_id=None, autoreset=True, S=Settings, log_capacity=0):
    """One ``stmpc_env_cfg`` per reward group (a ``_capi.EnvCfgTable`` for the ``stmpc_reward_groups_*`` entries): ``rewards`` is a list of
    dicts, each setting ``REWARD_FUNCTION`` and any of ``REWARD_GROUP_KEYS`` over ``S`` (the global ``Settings``, which is read and never
    written) -- what the reference's configs/*.json override per run (dqn.py:449-460, merge_gym.py:25).  Everything else -- the env, its action
    table, the tick, the limits, autoreset, the log, the observation -- is ``S``'s for every group.  ValueError for any other key, an unknown
    reward function, an empty list and more than ``ENV_REWARD_GROUPS_MAX`` groups."""
    rewards = list(rewards)
    groups.within(len(rewards), _capi.ENV_REWARD_GROUPS_MAX, "rewards")
    table = []
    for group in rewards:
        if not isinstance(group, dict):
            raise ValueError("a reward group is a dict of settings, not %r" % (group,))
        unknown = [k for k in group if k != "REWARD_FUNCTION" and k not in REWARD_GROUP_KEYS]
        if unknown:
            raise ValueError("a reward group may set REWARD_FUNCTION, %s, not %s" % (", ".join(REWARD_GROUP_KEYS), ", ".join(map(str, unknown))))
        c = env_cfg(env_id, group.get("REWARD_FUNCTION"), autoreset, S, log_capacity)
        for key, value in group.items():
            if key != "REWARD_FUNCTION":
                setattr(c, REWARD_GROUP_KEYS[key], float(value))
        table.append(c)
    return _capi.EnvCfgTable(table)


def reward_settings(group, S=Settings):
    """``S`` overlaid with one reward group's dict: a class to hand to the ``rewards.py`` twins as ``S=``."""
    return type("RewardGroupSettings", (S,), dict(group))


def observation_bounds(S=Settings):
    """(low, high) of JerkEnv's observation space, merge_gym.py:41-79."""
    n_cars = S.CARS_AHEAD + S.CARS_BEHIND
    dim = (4 if S.USE_ACCELERATION_OF_OTHER_CARS else 3) * n_cars + 4
    lows, highs = np.zeros(dim), np.zeros(dim)
    if S.NORMALIZE_VECTOR_INPUT:
        lows -= 1
        highs += 1
    else:
        for i in range(n_cars):
            if S.USE_ACCELERATION_OF_OTHER_CARS:
                lows[4 * i:4 * i + 4] = (-9, -S.MAX_SPEED, -300, 0)
                highs[4 * i:4 * i + 4] = (6, S.MAX_SPEED + 1E-5, 300, 1)
            else:
                lows[3 * i:3 * i + 3] = (-S.MAX_SPEED, -300, 0)
                highs[3 * i:3 * i + 3] = (S.MAX_SPEED + 1E-5, 300, 1)
        lows[-4:] = (0, S.MAX_NEGATIVE_ACCELERATION - 1E-5, -250, -10)
        highs[-4:] = (S.MAX_SPEED + 1E-5, S.MAX_POSITIVE_ACCELERATION + 1E-5, 250, 100)
    return lows, highs


#: (shield, group axis) -> the ``_capi.Context`` methods that reset and step that env: the shapes the C entries serve (``env_entries`` reads it)
_ENTRIES = {
    (None, "lone"): ("env_reset", "env_step"),
    (None, "traffic"): ("env_reset_groups", "env_step_groups"),
    (None, "rewards"): ("env_reset_reward_groups", "env_step_reward_groups"),
    (None, "mix"): ("traffic_mix_env_reset", "traffic_mix_env_step"),
    ("first_step", "lone"): ("shield_env_reset", "shield_env_step"),
    ("first_step", "traffic"): ("shield_env_reset_groups", "shield_env_step_groups"),
    ("first_step", "rewards"): ("shield_env_reset_reward_groups", "shield_env_step_reward_groups"),
    ("first_step", "mix"): ("shield_traffic_mix_env_reset", "shield_traffic_mix_env_step"),
    ("combined", "lone"): ("cshield_env_reset", "cshield_env_step"),
}
#: entry -> the env attributes that are its leading arguments, in the method's order: what stands before ``d_obs`` of a reset and ``d_action`` of a step
_LEAD = {
    "env_reset": "params sim_cfg cfg n", "env_step": "params sim_cfg cfg n",
    "env_reset_groups": "params sim_cfgs n_per_group cfg", "env_step_groups": "params cfg n",
    "env_reset_reward_groups": "params _world n_per_group reward_cfgs n_per_reward_group", "env_step_reward_groups": "params cfg n",
    "traffic_mix_env_reset": "params mix_cfgs mix_weights mix_seed cfg n", "traffic_mix_env_step": "params cfg n",
    "shield_env_reset": "params sim_cfg cfg shield_cfg n", "shield_env_step": "params sim_cfg cfg shield_cfg n",
    "shield_env_reset_groups": "params sim_cfgs n_per_group cfg shield_cfg takeover_penalties", "shield_env_step_groups": "params cfg shield_cfg n",
    "shield_env_reset_reward_groups": "params _world n_per_group reward_cfgs n_per_reward_group shield_cfg takeover_penalties",
    "shield_env_step_reward_groups": "params cfg shield_cfg n",
    "shield_traffic_mix_env_reset": "params mix_cfgs mix_weights mix_seed cfg shield_cfg n", "shield_traffic_mix_env_step": "params cfg shield_cfg n",
    "cshield_env_reset": "params sim_cfg cfg shield_cfg _actor n", "cshield_env_step": "params sim_cfg cfg shield_cfg _actor n",
}
#: the discrete env behind the combined shield with a Q-network in the rollout (``QCombinedShieldVecEnv``): a class of its own with entries of its own,
#: bound by that class -- ``env_entries`` and ``_LEAD`` describe the shapes ``MergeVecEnv``'s arguments can express and stay as they are
_Q_ENTRIES = ("qshield_env_reset", "qshield_env_step")
_Q_LEAD = {name: "params sim_cfg cfg shield_cfg _qactor _qpop _n_per_member n" for name in _Q_ENTRIES}
_MIX_ALONE = ("a traffic mix with traffic groups, reward groups or a shield is out of scope: the mixed step serves one ungrouped world "
              "under one reward, unshielded")


def env_entries(shield=None, has_mix=False, R=0, G=0):
    """(reset, step): the names of the ``_capi.Context`` methods that serve an env behind ``shield`` (None, "first_step" or "combined") with a traffic
    mix or not, ``R`` reward groups and ``G`` traffic groups (0: none).  A pure table: no device, no torch, no context.  ValueError for the shapes no
    entry serves: an unknown shield, a mix together with groups, R != G where both are given, anything but the lone world behind the combined shield."""
    if shield not in (None, "first_step", "combined"):
        raise ValueError("unknown shield %r (None, 'first_step' or 'combined')" % (shield,))
    if has_mix and (R or G):
        raise ValueError(_MIX_ALONE)
    if R and G and R != G:
        raise ValueError("the env has %d traffic groups and %d reward groups: cell c pairs traffic c with reward c, so they must coincide" % (G, R))
    axis = "mix" if has_mix else "rewards" if R else "traffic" if G else "lone"
    if (shield, axis) not in _ENTRIES:
        raise ValueError("traffic groups, reward groups and a traffic mix behind the combined shield are out of scope: it serves one ungrouped world")
    return _ENTRIES[(shield, axis)]


def _shield_args(takeover_penalty, shield_kmax, count=None):
    """The checked ``takeover_penalty`` / ``shield_kmax`` of a shielded env: the penalties as a list of floats.  ``count`` None: one number (a Python or
    numpy number, a 0-d array or tensor); else one number or one per group of ``count`` groups.  ValueError unless each is finite and >= 0 and
    ``shield_kmax`` is 1 ... ``KMAX_LIMIT``."""
    try:
        penalties = [float(takeover_penalty)] if count is None else [float(x) for x in np.asarray(takeover_penalty, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError("takeover_penalty must be a number%s, not %r" % ("" if count is None else " or one number per group", takeover_penalty))
    if len(penalties) not in (1, count):
        raise ValueError("takeover_penalty has %d values for %d groups: one number, or one per group" % (len(penalties), count))
    if not all(np.isfinite(x) and x >= 0 for x in penalties):
        raise ValueError("takeover_penalty must be finite and not negative, not %r" % (takeover_penalty,))
    if not 1 <= int(shield_kmax) <= _capi.KMAX_LIMIT:
        raise ValueError("shield_kmax must be 1 ... %d (the solver's vehicles per state), not %r" % (_capi.KMAX_LIMIT, shield_kmax))
    return penalties


def _mix_args(seed, traffic_mix, mix_weights, mix_seed, alone):
    """The checked traffic mix of an env: None without ``traffic_mix``, else (types, their cfgs, weights, cumulative weights, mix seed).  ``alone``:
    whether the env has nothing the mix does not go with.  Every ValueError of the mix's arguments; touches no device."""
    if traffic_mix is None:
        if mix_weights is not None or mix_seed is not None:
            raise ValueError("mix_weights and mix_seed belong to a traffic_mix: none was given")
        return None
    if not alone:
        raise ValueError(_MIX_ALONE)
    mix = list(traffic_mix)
    mix_cfgs = episodes.traffic_mix_cfgs(mix, seed, float(Settings.MAX_EPISODE_LENGTH))
    weights = [1.0] * len(mix) if mix_weights is None else list(mix_weights)
    if len(weights) != len(mix):
        raise ValueError("mix_weights has %d entries for %d traffic types" % (len(weights), len(mix)))
    cum = traffic_mix_cum(weights)
    return mix, mix_cfgs, [float(w) for w in weights], cum, episode_seed(seed, 2 ** 31 - 1) if mix_seed is None else int(mix_seed) & _M64


def _summary_by(rows, owner, count):
    """One dict per part p < ``count`` for the drained episodes ``rows`` with ``owner == p``: ``episodes`` (their number), the ``merged``, ``crashed``
    and ``timed_out`` shares, ``mean_ticks`` and ``mean_return`` (NaN for a part without episodes)."""
    out = []
    for p in range(count):
        m = owner == p
        k = int(m.sum())
        mean = lambda col: float(np.mean(np.asarray(rows[col], dtype=np.float64)[m])) if k else float("nan")
        out.append({"episodes": k, "merged": mean("merged"), "crashed": mean("crashed"), "timed_out": mean("timed_out"), "mean_ticks": mean("ticks"),
                    "mean_return": mean("episode_return")})
    return out


class MergeVecEnv:
    """``n`` merge environments on the device.  ``env_id``: "sumo-jerk-continuous-v0" (actions: fp64 jerks [n], not clipped to the Box, as the
    reference does not clip them), "sumo-jerk-v0" or "sumo-accel-v0" (actions: int indices [n]); ``reward``: "Continuous", "Slotted",
    "Slotted Jerk" or "ST".  Settings are read at construction (Settings.MAX_EPISODE_LENGTH, the traffic, the reward weights, ...).
    ``ctx``: the ``_capi.Context`` that holds the world (default: a context of its own).  A context holds one world: a second env reset on it,
    or an ``EpisodeRunner`` started on it, ends this one -- its next ``step`` raises instead of stepping the other's world.
    Kernels run on the current torch stream of the call.

    Which C entries reset and step an env follows from its shape alone -- its shield, whether it has a traffic mix, its reward and traffic groups --
    by the table ``env_entries``; every class below checks its own arguments and then hands the shape to ``_setup``, which binds the two entries once.

    ``traffic``: None, or a list as ``episodes.sim_cfgs`` takes: ``G = len(traffic)`` traffic groups of ``n / G`` consecutive environments
    (``stmpc_env_reset_groups_device`` / ``stmpc_env_step_groups_device``, the launches of an ungrouped env), group g bit-identical -- through
    every autoreset -- to a lone ``MergeVecEnv`` of ``n / G`` environments with that traffic and group g's seed (``episodes.sim_cfgs``).

    ``rewards``: None, or a list as ``reward_cfgs`` takes: ``R = len(rewards)`` reward groups of ``n / R`` consecutive environments, each rewarded
    under its own reward function and weights (``stmpc_reward_groups_env_reset_device`` / ``stmpc_reward_groups_env_step_device``, the three
    launches of a lone env) -- the reward-shaping sweep the reference runs as one ``TRAIN_DDPG`` per config.  Rows
    ``[r * n / R, (r + 1) * n / R)`` are bit-identical -- through every autoreset -- to those rows of the lone ``MergeVecEnv`` made with group r's
    values in the Settings.  With ``traffic`` too the counts must coincide (cell c pairs traffic c with reward c) and group r is the lone env of
    ``n / R`` environments with that traffic and that reward; without it the world is one world of ``n`` environments whatever the rewards (pass
    ``traffic=[t] * R`` for R copies of one lone world under R rewards: common random numbers).  ``reward`` is then ignored;
    ``reward_names`` lists the groups' functions.  A ``learner.DDPGPopulation`` of R members trains member m under reward m, and
    ``learner.evaluate_members`` / ``episodes.summary_by_member`` compare the resulting policies on one common report.

    ``shield``: None (every action is executed as it is: today's env on every path) or "first_step": every step runs behind the first-step shield,
    ``st.do_conditional_st_based_on_first_step`` (st.py:805-814, ``first_step.py``), on the device (``stmpc_shield_env_reset_device`` /
    ``stmpc_shield_env_step_device``) -- the closed loop ``episodes.EpisodeRunner(controller="first_step")`` deploys a policy in.  The action is a
    proposal: where one predictor step with it crashes, or no feasible path is left after it, ``st.do_st_control``'s speed is executed instead, and
    ``info`` tells the learner: ``takeover`` (bool [n]), ``reason`` (int32 [n], ``first_step.REASON_*``), ``executed_jerk`` (fp64 [n]: the projected jerk
    of what was executed), ``executed_action`` (the continuous env only: the action where it stood, else ``executed_jerk`` clipped to the Box) and
    ``takeover_ticks`` (int32 [n]: takeovers of the environment's current episode up to this tick; the finished episode's where ``terminated |
    truncated``).  ``takeover_penalty`` (>= 0) is added to the reward as ``takeover_penalty * TICK_LENGTH`` on a takeover tick; ``shield_kmax``: the row
    stride of the planner's view the shield sees (``EpisodeRunner``'s ``kmax``; 1 ... 32, the solver's limit).  ``shield_sparse=False`` solves the controller for every environment and
    keeps ``step`` free of host synchronisation; ``shield_sparse=True`` solves it for the taken-over ones only, and ``step`` then DOES synchronise: one
    integer, their number, crosses to the host every step.  Same outputs either way.  ``shield_counts()`` reads the shield's totals.  Refused
    with a ValueError here: a shield together with ``traffic`` or ``rewards`` groups -- that env is a class of its own, ``GroupedShieldVecEnv``.

    ``traffic_mix`` (with ``mix_weights``, ``mix_seed``; keyword-only): every episode draws its own traffic type -- the call then returns a
    ``TrafficMixVecEnv``, see there."""

    SHIELDS = ("first_step",)

    def __new__(cls, *args, **kwargs):
        # ``MergeVecEnv(..., traffic_mix=[...], mix_weights=None, mix_seed=None)`` makes a ``TrafficMixVecEnv``, whose constructor takes these three
        # keyword-only arguments after this class's own (which stay as they are)
        if cls is MergeVecEnv and any(k in kwargs for k in ("traffic_mix", "mix_weights", "mix_seed")):
            return object.__new__(TrafficMixVecEnv)
        return object.__new__(cls)

    def __init__(self, n, env_id=None, seed=0, reward=None, autoreset=True, ctx=None, log_capacity=0, traffic=None, rewards=None, shield=None,
                 shield_sparse=False, takeover_penalty=0.0, shield_kmax=32):
        shield_cfg = self._own_shield_cfg(shield, traffic, rewards, shield_sparse, takeover_penalty, shield_kmax)
        self._setup(n, env_id, seed, reward, autoreset, ctx, log_capacity, traffic, rewards, None, shield, shield_cfg)

    @classmethod
    def _own_shield_cfg(cls, shield, traffic, rewards, shield_sparse, takeover_penalty, shield_kmax):
        """The ``ShieldEnvCfg`` of ``MergeVecEnv(shield=...)`` (None without a shield), after this class's refusals: the lone world only."""
        if shield is None:
            return None
        if shield not in cls.SHIELDS:
            raise ValueError("unknown shield %r (None or one of %s)" % (shield, ", ".join(cls.SHIELDS)))
        if traffic is not None or rewards is not None:
            raise ValueError("a shielded env with traffic or reward groups is out of scope: the shielded step serves one ungrouped world under one reward")
        penalty, = _shield_args(takeover_penalty, shield_kmax)
        return _capi.ShieldEnvCfg.from_settings(Settings, shield_sparse, penalty, shield_kmax)

    def _setup(self, n, env_id, seed, reward, autoreset, ctx, log_capacity, traffic=None, rewards=None, mix=None, shield=None, shield_cfg=None, entries=None):
        """What every constructor ends in, after its own checks: the env's settings and world (the remaining ValueErrors, all before the first device
        call), its context and tensors, the shield's outputs (``shield``: None, "first_step" or "combined", with its ``shield_cfg``), the mix's (``mix``:
        what ``_mix_args`` returns) and the env's two entries, bound once (``entries``: a class's own pair instead of ``env_entries``'; a class sets the
        attributes of ``_LEAD`` that only its entries take, such as the combined shield's policy, before it calls this)."""
        self.shield, self.shield_cfg = shield, shield_cfg
        self.env_id = Settings.GYM_ENVIRONMENT if env_id is None else env_id
        self.reward_name = Settings.REWARD_FUNCTION if reward is None else reward
        self.cfg = env_cfg(self.env_id, self.reward_name, autoreset, Settings, log_capacity)         # (raises ValueError first)
        self.n, self.seed, self.autoreset = int(n), int(seed), bool(autoreset)
        if self.n < 1:
            raise ValueError("n must be positive")
        self.traffic = list(traffic) if traffic is not None else None
        self.G, self.n_per_group = episodes._check_traffic(self.n, self.traffic, None) if self.traffic is not None else (0, 0)
        self.sim_cfgs = episodes.sim_cfgs(self.traffic, seed, float(Settings.MAX_EPISODE_LENGTH)) if self.traffic is not None else None
        self.rewards = [dict(r) for r in rewards] if rewards is not None else None
        self.reward_cfgs = reward_cfgs(self.rewards, self.env_id, autoreset, Settings, log_capacity) if self.rewards is not None else None
        self.R = len(self.rewards) if self.rewards is not None else 0
        if self.R and self.n % self.R:
            raise ValueError("n = %d environments do not divide into %d reward groups of equal size" % (self.n, self.R))
        self.n_per_reward_group = self.n // self.R if self.R else 0
        table_entries = env_entries(shield, mix is not None, self.R, self.G)       # (ValueError unless R and G coincide)
        entries = table_entries if entries is None else entries
        self.reward_names = [r.get("REWARD_FUNCTION", Settings.REWARD_FUNCTION) for r in self.rewards] if self.R else [self.reward_name]
        if self.R:
            self.cfg = self.reward_cfgs[0]                   # (the shared fields: what the step entry reads of it)
        self.traffic_mix = None
        if mix is not None:
            self.traffic_mix, self.mix_cfgs, self.mix_weights, self.mix_cum, self.mix_seed = mix
            self.T = len(self.traffic_mix)
        import torch
        self.torch = torch
        self.ctx = ctx if ctx is not None else _capi.Context(-1)
        self.params = _capi.Params.from_settings(Settings)
        self.sim_cfg = self.sim_cfgs[0] if self.sim_cfgs is not None else episodes.sim_cfg(seed, float(Settings.MAX_EPISODE_LENGTH))
        self._world = self.sim_cfgs if self.sim_cfgs is not None else self.sim_cfg       # (what a reward-groups reset takes: the table, or the one cfg)
        self.log_capacity = int(log_capacity) if log_capacity else 16 * self.n
        self.obs_dim = (4 if Settings.USE_ACCELERATION_OF_OTHER_CARS else 3) * (Settings.CARS_AHEAD + Settings.CARS_BEHIND) + 4
        self.observation_low, self.observation_high = observation_bounds(Settings)
        self.continuous = self.env_id == "sumo-jerk-continuous-v0"
        if self.continuous:             # spaces.Box(MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK, shape=(1,)), merge_gym.py:222-224
            self.action_space = {"type": "Box", "low": float(Settings.MINIMUM_NEGATIVE_JERK), "high": float(Settings.MAXIMUM_POSITIVE_JERK), "shape": (1,)}
        else:                           # spaces.Discrete(len(...)), merge_gym.py:80,190
            self.action_space = {"type": "Discrete", "n": int(self.cfg.n_action_values)}
        dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
        self._obs = [z(self.n, self.obs_dim, dtype=torch.float32) for _ in range(2)]      # double-buffered: a learner may keep the previous step's tensor
        self._final_obs = z(self.n, self.obs_dim, dtype=torch.float32)
        self._reward, self._final_stats = z(self.n), z(self.n, _capi.ENV_NSTAT)
        self._term, self._trunc = z(self.n, dtype=torch.bool), z(self.n, dtype=torch.bool)
        self._cur = 0
        self._ticks = z(self.n, dtype=torch.int32)
        self._reset_done = False
        # what a step writes besides the observation, in the entries' order, and what ``info`` shows of it: the same tensors at every step
        out = [self._reward, self._term, self._trunc, self._final_obs, self._final_stats]
        self._info = {"final_observation": self._final_obs, "final_stats": self._final_stats, "episode_return": self._final_stats[:, _capi.ENV_NSTAT - 1],
                      "status": self._final_stats[:, _capi.SIM_NACC]}
        reset_tail = []
        if shield is not None:
            self._takeover, self._reason = z(self.n, dtype=torch.bool), z(self.n, dtype=torch.int32)
            self._exec_jerk, self._takeover_ticks = z(self.n), z(self.n, dtype=torch.int32)
            self._exec_action = z(self.n) if self.continuous else None
            out += [self._takeover, self._reason, self._exec_jerk] + ([self._exec_action] if entries != _Q_ENTRIES else []) + [self._takeover_ticks]
            self._info.update(takeover=self._takeover, reason=self._reason, executed_jerk=self._exec_jerk, takeover_ticks=self._takeover_ticks)
            if self._exec_action is not None:
                self._info["executed_action"] = self._exec_action
        if mix is not None:
            self._type, self._final_type = z(self.n, dtype=torch.int32), z(self.n, dtype=torch.int32)
            out += [self._type, self._final_type]
            reset_tail = [self._type]
            self._info.update(traffic_type=self._type, final_traffic_type=self._final_type)
        self._bind(entries, reset_tail, out)

    def _bind(self, entries, reset_tail, step_out):
        """The env's reset and step entry, bound once: the ``Context`` method, its leading arguments (``_LEAD``) and the pointers that follow the per-call
        ones.  ``reset()`` calls ``entry(*lead, d_obs, obs_stride, *tail, stream)`` and ``step()`` ``entry(*lead, d_action, d_obs, obs_stride, *out, stream)``,
        ``lead`` held by a ``functools.partial`` and ``out`` being the step's outputs from the reward on, then the shield's, then the mix's types (None: a
        NULL pointer).  ``_setup`` is its only caller, and every constructor calls ``_setup`` once."""
        if hasattr(self, "_step"):
            raise RuntimeError("an env binds its entries once")
        lead = lambda name: (_LEAD[name] if name in _LEAD else _Q_LEAD[name]).split()
        bound = lambda name: functools.partial(getattr(self.ctx, name), *(getattr(self, a) for a in lead(name)))
        ptrs = lambda tensors: tuple(t.data_ptr() if t is not None else 0 for t in tensors)
        self._reset, self._reset_tail = bound(entries[0]), ptrs(reset_tail)
        self._step, self._step_out = bound(entries[1]), ptrs(step_out)

    def reset(self):
        """Every environment back to episode 0 (``stmpc_env_reset_device``, or the reset entry of the env's traffic groups, reward groups, mix or shield):
        the observations of the start states [n][obs_dim] float32."""
        self._cur = 0
        obs = self._obs[0]
        self._reset(obs.data_ptr(), self.obs_dim, *self._reset_tail, self._stream())
        _owners[self.ctx] = self
        self._reset_done = True
        return obs

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    @property
    def episode_ticks(self):
        """Ticks of each environment's current episode, int32 [n] on the device (0 right after a reset; e.g. a TimeFeature input: 0.001 x this).
        One device-to-device copy of the world's counter on the current stream; the tensor is overwritten by the next read."""
        self.ctx.env_episode_ticks(self.n, self._ticks.data_ptr(), self._stream())
        return self._ticks

    def _action_tensor(self, action):
        torch = self.torch
        want = torch.float64 if self.continuous else torch.int32
        a = torch.as_tensor(action, device=self.device)
        if a.dtype != want:
            a = a.to(want)
        a = a.reshape(self.n)
        return a if a.is_contiguous() else a.contiguous()

    def step(self, action):
        """One tick of every environment; no host synchronisation (but with ``shield_sparse=True``).  Returns (obs, reward, terminated, truncated, info) as device tensors;
        info: final_observation [n][obs_dim], final_stats [n][15] (world statistics as episodes.EpisodeRunner reads them, status, ticks, return),
        episode_return [n] (= final_stats[:, 14]) and status [n] (= final_stats[:, 12]) -- valid where terminated | truncated.  A shielded env adds
        takeover, reason, executed_jerk, executed_action (continuous env) and takeover_ticks, valid in every row, an env with a traffic mix
        traffic_type and final_traffic_type (see the classes).  The dict is the call's own; its tensors are the same at every step."""
        if not self._reset_done:
            raise RuntimeError("call reset() before step()")
        if _owners.get(self.ctx) is not self:
            raise RuntimeError("another MergeVecEnv was reset on this env's context since its own reset(): a context holds one world")
        a = self._action_tensor(action)
        self._cur ^= 1
        obs = self._obs[self._cur]
        self._step(a.data_ptr(), obs.data_ptr(), self.obs_dim, *self._step_out, self._stream())
        self._last_action = a                                # (kept alive until the kernels have read it)
        return obs, self._reward, self._term, self._trunc, dict(self._info)

    def shield_counts(self, reset=False):
        """(states decided, states taken over, controller solves) of the shield on this env's context since the last reset of the counts
        (``stmpc_first_step_counts``: finished environments of a run without autoreset are decided too, and count); synchronises."""
        if self.shield_cfg is None:
            raise RuntimeError("this env has no shield")
        return self.ctx.first_step_counts(reset)

    def check_error(self):
        """Raise what the kernels flagged (an action index out of range); synchronises."""
        self.ctx.check_error()

    def drain_episode_stats(self):
        """The episodes finished since the last drain (or reset), as the columns of ``episodes.EpisodeRunner.result()`` plus ``env``,
        ``episode``, ``episode_return``, ``traffic_group`` (``env // n_per_group``; 0 without traffic groups) and ``reward_group``
        (``env // n_per_reward_group``; 0 without reward groups), ordered by (env, episode).  Synchronises; raises if device-side errors were flagged, and
        RuntimeError if more episodes finished than the log holds (``log_capacity``, default 16 n: drain more often)."""
        rows, dropped = self.ctx.env_drain(self.log_capacity)
        self.ctx.check_error()
        if dropped:
            raise RuntimeError("%d finished episodes were dropped: drain_episode_stats() more often or raise log_capacity" % dropped)
        order = np.lexsort((rows[:, _capi.ENV_NSTAT + 1], rows[:, _capi.ENV_NSTAT]))
        rows = rows[order]
        out = episodes.stats_columns(rows[:, _capi.SIM_NACC].astype(np.int32), rows[:, _capi.SIM_NACC + 1].astype(np.int32), rows[:, :_capi.SIM_NACC],
                                     Settings.TICK_LENGTH)
        out["episode_return"] = rows[:, _capi.ENV_NSTAT - 1]
        out["env"] = rows[:, _capi.ENV_NSTAT].astype(np.int64)
        out["episode"] = rows[:, _capi.ENV_NSTAT + 1].astype(np.int64)
        out["traffic_group"] = out["env"] // self.n_per_group if self.sim_cfgs is not None else np.zeros(len(rows), dtype=np.int64)
        out["reward_group"] = out["env"] // self.n_per_reward_group if self.R else np.zeros(len(rows), dtype=np.int64)
        return out


class TrafficMixVecEnv(MergeVecEnv):
    """``MergeVecEnv`` whose every episode draws its own traffic type: domain randomisation at the episode boundary, the autoreset included, on the
    device (``stmpc_traffic_mix_env_reset_device`` / ``stmpc_traffic_mix_env_step_device``, the three launches of a lone env).  Made by
    ``MergeVecEnv(..., traffic_mix=..., mix_weights=..., mix_seed=...)`` as well as by its own name; with ``traffic_mix=None`` it is the plain env.

    ``traffic_mix``: a list as ``episodes.traffic_settings`` takes -- names of ``episodes.TRAFFIC_TYPES`` or dicts of BASE_TRAFFIC_INTERVAL,
    OTHER_CAR_SPEED and optionally VARY_TRAFFIC_START_TIMES; 1 ... ``_capi.TRAFFIC_MIX_MAX`` types; a ``seed`` key is a ValueError (one world, one
    seed).  ``mix_weights``: one number per type, each finite and >= 0 with a positive sum (default: uniform).  ``mix_seed``: default
    ``episode_seed(seed, 2**31 - 1)``, so that the type draws are not the world's draws.

    The world is one ungrouped world of ``n`` environments.  Episode j of environment e runs under type ``traffic_mix_draw(mix_seed, e, j, mix_cum)``
    and is, bit for bit, episode j of row e of the lone ``MergeVecEnv(n, traffic=[that type], seed=seed)`` when it receives the same actions: the draw
    takes nothing from the world's draw counter.  The finishing episode's reward, final observation, statistics and log row are its own type's; the
    observation returned for the row is the next episode's start state under the type drawn for it.  ``step`` adds ``info["traffic_type"]`` (int32 [n]:
    the type of the episode the row is in after the step) and ``info["final_traffic_type"]`` (where ``terminated | truncated``: the type of the
    episode that ended; elsewhere the current type), device tensors, no host synchronisation.  ``traffic_type`` reads the current types,
    ``drain_episode_stats`` adds a ``traffic_type`` column (``traffic_of_log``), ``summary_by_traffic`` condenses it per type.
    ``learner.train_ddpg`` and ``learner.DDPGPopulation`` train on it as on any env.  Out of scope, refused with a ValueError before any device call:
    a mix together with ``traffic`` groups, ``rewards`` groups or a ``shield`` (the shielded mix is a ``GroupedShieldVecEnv``).  This class checks the
    mix's arguments; the mix's tensors, its ``info`` keys and its entries are the base class's (``_setup``)."""

    def __init__(self, n, env_id=None, seed=0, reward=None, autoreset=True, ctx=None, log_capacity=0, traffic=None, rewards=None, shield=None,
                 shield_sparse=False, takeover_penalty=0.0, shield_kmax=32, *, traffic_mix=None, mix_weights=None, mix_seed=None):
        mix = _mix_args(seed, traffic_mix, mix_weights, mix_seed, alone=traffic is None and rewards is None and shield is None)      # (before any device call)
        shield_cfg = self._own_shield_cfg(shield, traffic, rewards, shield_sparse, takeover_penalty, shield_kmax)
        self._setup(n, env_id, seed, reward, autoreset, ctx, log_capacity, traffic, rewards, mix, shield, shield_cfg)

    @property
    def traffic_type(self):
        """The traffic type of the episode each environment is in, int32 [n] on the device (the tensor of ``info["traffic_type"]``)."""
        self._need_mix()
        return self._type

    def _need_mix(self):
        if self.traffic_mix is None:
            raise RuntimeError("this env has no traffic mix")

    def traffic_of_log(self, rows):
        """The traffic type of each drained episode (``rows``: what ``drain_episode_stats`` returns, or any dict with ``env`` and ``episode``
        columns), int64 [len]: host arithmetic on the two columns through ``traffic_mix_draw`` -- the log has no column for it."""
        self._need_mix()
        return np.array([traffic_mix_draw(self.mix_seed, int(e), int(j), self.mix_cum) for e, j in zip(rows["env"], rows["episode"])], dtype=np.int64)

    def summary_by_traffic(self, rows):
        """One dict per traffic type for drained episodes ``rows``: ``episodes`` (their number), the ``merged``, ``crashed`` and ``timed_out`` shares,
        ``mean_ticks`` and ``mean_return`` (NaN for a type without episodes)."""
        return _summary_by(rows, self.traffic_of_log(rows), self.T)

    def drain_episode_stats(self):
        out = super().drain_episode_stats()
        if self.traffic_mix is not None:
            out["traffic_type"] = self.traffic_of_log(out)
        return out


class _CombinedShieldEnv(MergeVecEnv):
    """What the two envs behind the combined controller share, whichever policy proposes in the rollout: the checks of the env id and of where the policy
    lives, the ``control`` overlay, the shield's cfg and ``shield_counts``.  ``noun`` is what the messages call the policy."""

    @staticmethod
    def _served_env_id(env_id, served, refusal):
        """The env id (default: the Settings'), which must be one of ``served``: ``refusal % env_id`` otherwise."""
        env_id = Settings.GYM_ENVIRONMENT if env_id is None else env_id
        if env_id not in ENV_IDS:
            raise ValueError("Invalid gym environment {} (one of {})".format(env_id, ", ".join(ENV_IDS)))
        if env_id not in served:
            raise ValueError(refusal % (env_id,))
        return env_id

    @staticmethod
    def _placed(n, policy, ctx, kinds, wanted, noun, rows=""):
        """``policy`` is a live hip-engine instance of ``kinds`` (``wanted`` names them) with the env's ``n`` rows (``rows``: how they split) on ``ctx``."""
        if not isinstance(policy, kinds) or getattr(policy, "engine", None) != "hip" or getattr(policy, "handle", None) is None:
            raise ValueError("policy must be a hip-engine %s, not %r" % (wanted, policy))
        if int(n) < 1 or policy.n != int(n):
            raise ValueError("%s was built for %d rows%s, the env has n = %r" % (noun, policy.n, rows, n))
        if ctx is not None and policy.ctx is not ctx:
            raise ValueError("%s lives on another context than the env's: build it on ctx (or leave ctx=None to take %s's)" % (noun, noun))

    def _combined_setup(self, cfg_cls, n, policy, env_id, seed, reward, autoreset, log_capacity, shield_sparse, takeover_penalty, shield_kmax, control,
                        entries=None, **cfg_args):
        """The checked shield arguments and ``control`` overlay, the shield's cfg (``cfg_cls.from_settings`` with the policy's features and ``cfg_args``),
        then ``_setup`` on the policy's context."""
        from . import combined
        penalty, = _shield_args(takeover_penalty, shield_kmax)
        self.control = dict(control) if control is not None else {}
        combined.control_cfgs([self.control])                               # (ValueError for a key that is no setting of do_combined_control)
        cfg = cfg_cls.from_settings(combined._Overlay(Settings, self.control), shield_sparse, penalty, shield_kmax, features=policy.fcfg, **cfg_args)
        if cfg.cc.remember_last_choice:
            raise ValueError("REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED is out of scope behind the combined shield: the env keeps no takeover history")
        self.policy = policy
        self._setup(n, env_id, seed, reward, autoreset, policy.ctx, log_capacity, shield="combined", shield_cfg=cfg, entries=entries)

    def shield_counts(self, reset=False):
        """(states decided, controller solves run for them) on this env's context since the last reset of the counts (``stmpc_combined_counts``:
        finished environments of a run without autoreset are decided too, and count; equal unless ``shield_sparse``)."""
        return self.ctx.combined_counts(reset)


class CombinedShieldVecEnv(_CombinedShieldEnv):
    """``MergeVecEnv`` whose every step runs behind the combined RL + ST controller, ``dqn.RLAgent.do_combined_control`` (dqn.py:117-200) -- the
    controller the reference deploys and evaluates (``EVALUATE_COMBINED_DDPG``, ``episodes.EpisodeRunner(controller="combined")``) -- on the device
    (``stmpc_cshield_env_reset_device`` / ``stmpc_cshield_env_step_device``), so that a policy trains in the closed loop it is deployed in.  A class of
    its own: ``MergeVecEnv(shield=...)`` stays the first-step shield's.

    The action handed to ``step`` is the controller's first action (the reference's ``agent.get_control(state)``); rollout steps 2 ... ROLLOUT_LENGTH ask
    ``policy`` on the device, the feasibility probe and the decision rules choose between the action and ``st.do_st_control``, and ``info`` reports what
    was executed with the first-step shield's keys: ``takeover``, ``reason`` (``combined.REASON_*``), ``executed_jerk``, ``executed_action``,
    ``takeover_ticks``.  ``env.shield == "combined"``, so ``learner.train_ddpg`` runs on it as on a shielded env, ``executed_actions=True`` included.

    ``policy``: a lone hip-engine ``actor.DDPGActor`` of ``n`` rows on the env's context (``ctx`` defaults to the actor's): pretrained, or
    ``DDPGActor.from_learner(learner, n, ctx, S, target=...)`` -- a zero-copy view, so the rollouts of a step queued after ``learner.update`` on the same
    stream see the updated weights: the learner's own current actor does the rollouts.  The env keeps it alive; its ``evals`` are not used.
    ``rollout_time``: what the actor's time feature reads at rollout step s >= 2.  "env": ``(episode ticks + s - 1) * time_scale``, the value
    ``learner.act`` would give that many ticks later; "deployed": a running count of all policy evaluations of the episode, the reference's
    ``TimeFeature`` under ``do_combined_control`` (``rollout_evals`` reads the count the next proposal is evaluated at).
    ``control``: a dict of ``combined.CONTROL_KEYS`` overlaid on ``Settings``, as ``combined.control_cfgs`` takes one cell.
    ``shield_sparse``, ``takeover_penalty``, ``shield_kmax``: as ``MergeVecEnv`` takes them.  ``shield_counts()`` reads ``(decisions, controller solves)``.

    Refused with a ValueError before any device call: a discrete env id, ``REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED`` true (the env keeps no
    takeover history), an ``actor.ActorPopulation`` or anything else that is no hip-engine ``DDPGActor``, an actor of another ``n`` or context, and a
    bad ``rollout_time``, ``takeover_penalty`` or ``shield_kmax``.  Out of scope: traffic groups, reward groups and the traffic mix behind this shield
    (``env_entries`` has no entry for them)."""

    def __init__(self, n, policy, env_id=None, seed=0, reward=None, autoreset=True, ctx=None, log_capacity=0, *, rollout_time="env", shield_sparse=False,
                 takeover_penalty=0.0, shield_kmax=32, control=None):
        from . import actor as _actor
        env_id_ = self._served_env_id(env_id, ("sumo-jerk-continuous-v0",),
                                      "the combined shield serves 'sumo-jerk-continuous-v0' only (the rollout policy is a continuous actor), not %r")
        if isinstance(policy, _actor.ActorPopulation):
            raise ValueError("an ActorPopulation behind the combined shield is out of scope: policy is one actor.DDPGActor")
        self._placed(n, policy, ctx, _actor.DDPGActor, "actor.DDPGActor (pretrained, or DDPGActor.from_learner)", "the actor")
        if rollout_time not in _capi.CShieldEnvCfg.ROLLOUT_TIMES:
            raise ValueError("rollout_time must be 'env' or 'deployed', not %r" % (rollout_time,))
        self.rollout_time, self._actor = rollout_time, policy.handle
        self._combined_setup(_capi.CShieldEnvCfg, n, policy, env_id_, seed, reward, autoreset, log_capacity, shield_sparse, takeover_penalty, shield_kmax,
                             control, rollout_time=rollout_time)
        self._evals = self.torch.zeros(self.n, dtype=self.torch.int32, device=self.device)

    @property
    def rollout_evals(self):
        """The count the next step's proposal is evaluated at, int32 [n] on the device (``stmpc_cshield_env_evals_device``): the episode's ticks under
        ``rollout_time="env"``, the episode's policy evaluations so far under "deployed" -- the ``evals`` to hand to an actor that proposes the action."""
        self.ctx.cshield_env_evals(self.n, self._evals.data_ptr(), self._stream())
        return self._evals


def q_first_action_host(env_id, index, ego_acc, S=Settings):
    """The host twin of ``k_qshield_env_pre``'s first action in numpy fp64, operation for operation: the jerk rollout step 1 of
    ``QCombinedShieldVecEnv`` applies for the action indices ``index`` [n] on states whose view has the ego accelerations ``ego_acc`` [n] -- the
    table's entry on "sumo-jerk-v0"; ``clip((table[a] - ego_acc) / TICK_LENGTH, MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK)`` on "sumo-accel-v0"
    (``actor.q_policy_host``'s rule); 0.0 for an index out of range.  Returns (first_action fp64 [n], out_of_range bool [n])."""
    if env_id not in QCombinedShieldVecEnv.MODE_OF:
        raise ValueError("a discrete env id ('sumo-jerk-v0' or 'sumo-accel-v0'), not %r" % (env_id,))
    values = S.JERK_VALUES_DQN if env_id == "sumo-jerk-v0" else S.ACCELERATION_VALUES_DQN
    table = np.array([values[i] for i in range(len(values))], dtype=np.float64)              # (index order, as env_cfg reads it)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    bad = (index < 0) | (index >= table.size)
    value = table[np.where(bad, 0, index)]
    if env_id == "sumo-accel-v0":
        value = (value - np.asarray(ego_acc, dtype=np.float64).reshape(-1)) / float(S.TICK_LENGTH)
        lo, hi = float(S.MINIMUM_NEGATIVE_JERK), float(S.MAXIMUM_POSITIVE_JERK)
        value = np.where(value < lo, lo, np.where(value > hi, hi, value))
    return np.where(bad, 0.0, value), bad


class QCombinedShieldVecEnv(_CombinedShieldEnv):
    """A DISCRETE ``MergeVecEnv`` ("sumo-jerk-v0", "sumo-accel-v0") whose every step runs behind the combined RL + ST controller,
    ``dqn.RLAgent.do_combined_control`` (dqn.py:117-200) as ``DQNAgent`` inherits it, with a Q-network (``DQNAgent.get_control``, dqn.py:375-380)
    proposing rollout steps 2 ... ROLLOUT_LENGTH on the device (``stmpc_qshield_env_reset_device`` / ``stmpc_qshield_env_step_device``): a DQN learner
    trains in the closed loop ``evaluate_dqn`` and ``EpisodeRunner(controller="combined")`` deploy it in.  A class of its own:
    ``CombinedShieldVecEnv`` stays the continuous env's and keeps refusing the discrete ids.

    The action INDEX handed to ``step`` is the controller's first action: its jerk is the table's entry ("sumo-jerk-v0") or, on "sumo-accel-v0",
    ``clip((table[a] - ego acceleration) / TICK_LENGTH, MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK)`` -- what ``policy`` itself returns for that index
    on that state.  ``info`` has ``takeover``, ``reason`` (``combined.REASON_*``), ``executed_jerk`` and ``takeover_ticks``, and no ``executed_action``: a
    takeover's speed is no table entry, so the index is not rewritten (as on the first-step-shielded discrete env).  ``env.shield == "combined"``:
    ``learner.train_dqn`` runs on it as on a shielded env.  There is no time feature, hence no ``rollout_time`` and no ``rollout_evals``.

    ``policy``: a hip-engine ``actor.DQNActor`` of ``n`` rows on the env's context (``ctx`` defaults to the policy's) -- an ``export_q`` file, or
    ``DQNActor.from_learner(learner, n, ctx, S, target=...)``, a zero-copy view, so a step queued after ``learner.update`` on the same stream rolls out
    with the updated weights; or an ``actor.C51Actor``, its subclass for a categorical network (a ``C51Learner.export_q`` file, or
    ``C51Actor.from_learner``, which sees ``C51Learner.update`` the same way) -- or an ``actor.QActorPopulation`` (or its subclass for categorical policies, ``actor.C51ActorPopulation``) with ``P * n_per_member == n``: member m proposes for rows ``[m * n_per_member, (m + 1)
    * n_per_member)`` of the one world.  Its mode and action table must be the env's ("jerk" with JERK_VALUES_DQN, "acceleration" with
    ACCELERATION_VALUES_DQN, byte for byte).  The env keeps it alive.
    ``control``, ``shield_sparse``, ``takeover_penalty``, ``shield_kmax``: as ``CombinedShieldVecEnv`` takes them; ``shield_counts()`` reads
    ``(decisions, controller solves)``.

    Refused with a ValueError before any device call: a continuous or unknown env id, an ``actor.DDPGActor``, an ``actor.ActorPopulation`` or anything
    else that is no hip-engine ``DQNActor`` / ``QActorPopulation``, a mode or table that is not the env's, another ``n`` or context,
    ``REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED`` true, a bad ``takeover_penalty`` or ``shield_kmax``.  Out of scope: traffic groups, reward groups
    and the traffic mix behind this shield."""

    MODE_OF = {"sumo-jerk-v0": "jerk", "sumo-accel-v0": "acceleration"}

    def __init__(self, n, policy, env_id=None, seed=0, reward=None, autoreset=True, ctx=None, log_capacity=0, *, shield_sparse=False, takeover_penalty=0.0,
                 shield_kmax=32, control=None):
        from . import actor as _actor
        env_id_ = self._served_env_id(env_id, self.MODE_OF, "the combined shield behind a Q-network serves 'sumo-jerk-v0' and 'sumo-accel-v0', not %r: the "
                                                            "continuous env's is CombinedShieldVecEnv")
        if isinstance(policy, (_actor.DDPGActor, _actor.ActorPopulation)):
            raise ValueError("a DDPGActor or an ActorPopulation proposes continuous jerks: policy is an actor.DQNActor, an actor.C51Actor or an actor.QActorPopulation "
                             "(the continuous env's class is CombinedShieldVecEnv)")
        pop = isinstance(policy, _actor.QActorPopulation)
        self._placed(n, policy, ctx, (_actor.DQNActor, _actor.QActorPopulation),
                     "actor.DQNActor (an export_q file, or DQNActor.from_learner), actor.C51Actor (likewise, of a C51Learner) or an actor.QActorPopulation", "the policy",
                     " (P = %d members x n_per_member = %d)" % (policy.P, policy.n_per_member) if pop else "")
        table = np.ascontiguousarray(env_cfg(env_id_, reward, autoreset, Settings, log_capacity)._actions, dtype=np.float64)     # (ValueError for an unknown reward)
        for m, a in enumerate(policy.members if pop else [policy]):
            who = "member %d" % m if pop else "the policy"
            if a.mode != self.MODE_OF[env_id_]:
                raise ValueError("%s is in %r mode, %r needs %r" % (who, a.mode, env_id_, self.MODE_OF[env_id_]))
            if np.asarray(a.action_values, dtype=np.float64).tobytes() != table.tobytes():
                raise ValueError("the action table of %s is not the env's (%s of the Settings, byte for byte)"
                                 % (who, "JERK_VALUES_DQN" if env_id_ == "sumo-jerk-v0" else "ACCELERATION_VALUES_DQN"))
        self._qactor, self._qpop, self._n_per_member = (None, policy.handle, policy.n_per_member) if pop else (policy.handle, None, 0)
        self._combined_setup(_capi.QShieldEnvCfg, n, policy, env_id_, seed, reward, autoreset, log_capacity, shield_sparse, takeover_penalty, shield_kmax,
                             control, entries=_Q_ENTRIES)


class GroupedShieldVecEnv(TrafficMixVecEnv):
    """The first-step shield of ``MergeVecEnv(shield="first_step")`` in front of the env's group axes: ``traffic`` groups, ``rewards`` groups (on an
    ungrouped world, or with as many traffic groups) or a ``traffic_mix`` -- the per-traffic-type training matrix, a reward-shaping sweep or a
    mixed-traffic policy trained in the closed loop of ``st.do_conditional_st_based_on_first_step`` (st.py:805-814), on the device
    (``stmpc_shield_traffic_groups_env_reset_device``, ``stmpc_shield_reward_groups_env_reset_device``, ``stmpc_shield_traffic_mix_env_reset_device`` and their
    step entries: the launches of the lone shielded step).  A class of its own: ``MergeVecEnv`` keeps refusing a shield together with groups or a mix.
    It checks its own arguments and hands the shape (the shield with groups or a mix) to the base class's ``_setup``: nothing of it rests on what its
    parents' constructors do.

    ``traffic``, ``rewards``, ``traffic_mix`` / ``mix_weights`` / ``mix_seed``: as ``MergeVecEnv`` and ``TrafficMixVecEnv`` take them; at least one
    of the three must be given, and the mix goes with neither kind of groups (ValueError).  ``takeover_penalty``: one number for every group, or one per
    group (G, or R without traffic groups; the mix takes one number); each finite and >= 0.  ``shield_sparse``, ``shield_kmax``: as ``MergeVecEnv``.

    The rows of group g are bit-identical -- through every autoreset -- to the lone ``MergeVecEnv(n / G, shield="first_step")`` made with group g's
    traffic, reward settings and takeover penalty; an episode of the shielded mix is the lone shielded env's episode of the drawn type.  ``step``'s
    ``info`` has the shielded env's keys (``takeover``, ``reason``, ``executed_jerk``, ``executed_action`` for the continuous env, ``takeover_ticks``)
    and, with a mix, ``traffic_type`` / ``final_traffic_type``.  ``env.shield == "first_step"``: ``learner.train_ddpg`` runs on it as on the lone
    shielded env, ``executed_actions=True`` included, and a ``learner.DDPGPopulation`` of one member per group trains member m behind the shield on
    group m.  ``takeover_share()`` and ``summary_by_group(rows)`` report per group (per traffic type for the mix)."""

    def __init__(self, n, env_id=None, seed=0, reward=None, autoreset=True, ctx=None, log_capacity=0, *, traffic=None, rewards=None, traffic_mix=None,
                 mix_weights=None, mix_seed=None, shield_sparse=False, takeover_penalty=0.0, shield_kmax=32):
        if traffic is None and rewards is None and traffic_mix is None:                   # (every check before any device call)
            raise ValueError("a GroupedShieldVecEnv needs traffic groups, reward groups or a traffic_mix: the lone shielded env is MergeVecEnv(shield='first_step')")
        traffic = list(traffic) if traffic is not None else None
        rewards = list(rewards) if rewards is not None else None
        self.takeover_penalties = _shield_args(takeover_penalty, shield_kmax, len(traffic) if traffic is not None else len(rewards) if rewards is not None else 1)
        mix = _mix_args(seed, traffic_mix, mix_weights, mix_seed, alone=traffic is None and rewards is None)
        # (the cfg's own penalty is what the lone shielded step reads; the grouped step reads the reset's table)
        shield_cfg = _capi.ShieldEnvCfg.from_settings(Settings, shield_sparse, self.takeover_penalties[0], shield_kmax)
        self._setup(n, env_id, seed, reward, autoreset, ctx, log_capacity, traffic, rewards, mix, "first_step", shield_cfg)
        torch = self.torch
        self.n_groups = self.T if mix is not None else self.R or self.G
        # the group a row's tick counts for: fixed, or (None) the type the tick ran under, info["final_traffic_type"]
        self._group_of_row = None if mix is not None else torch.arange(self.n, device=self.device) // (self.n // self.n_groups)
        self._taken = torch.zeros(self.n_groups, dtype=torch.int64, device=self.device)
        self._lived = torch.zeros(self.n_groups, dtype=torch.int64, device=self.device)
        self._alive = torch.ones(self.n, dtype=torch.bool, device=self.device)

    def reset(self):
        obs = super().reset()
        self._taken.zero_(), self._lived.zero_(), self._alive.fill_(True)
        return obs

    def step(self, action):
        out = super().step(action)
        group = self._group_of_row if self._group_of_row is not None else self._final_type.to(self.torch.int64)
        self._taken.index_add_(0, group, self._takeover.to(self.torch.int64))         # (device sums: no host synchronisation)
        self._lived.index_add_(0, group, self._alive.to(self.torch.int64))
        if not self.autoreset:
            self._alive &= ~(out[2] | out[3])                    # (a finished environment idles: not a live tick)
        return out

    def takeover_share(self):
        """Per group (per traffic type for the mix): the share of the live ticks since ``reset()`` on which the shield overruled the action, a list of
        floats (NaN for a type no tick ran under); synchronises."""
        taken, lived = self._taken.cpu().numpy(), self._lived.cpu().numpy()
        return [float(t) / float(l) if l else float("nan") for t, l in zip(taken, lived)]

    def summary_by_group(self, rows):
        """One dict per group for drained episodes ``rows`` (``drain_episode_stats``): ``episodes``, the ``merged``, ``crashed`` and ``timed_out``
        shares, ``mean_ticks``, ``mean_return`` (NaN for a group without episodes) and ``takeover_share`` (of the group's live ticks since ``reset()``).
        The groups are the reward groups, else the traffic groups, else the mix's traffic types."""
        if self.traffic_mix is not None:
            out = self.summary_by_traffic(rows)
        else:
            out = _summary_by(rows, np.asarray(rows["env"], dtype=np.int64) // (self.n // self.n_groups), self.n_groups)
        for d, share in zip(out, self.takeover_share()):
            d["takeover_share"] = share
        return out
