"""The reference's pretrained DDPG actor as the combined controller's policy (BASELINE configs[2]: ``configs/combined_medium_1.json``
-> ``MODEL_NAME runs/ddpg_medium1_extended``), evaluated on the GPU for N states at once.

``DDPGAgent.get_control`` (ddpg.py:83-87) is, per state:

    vector = dqn.get_state_vector_from_base_state(state)        dqn.py:389-446: 20 doubles
    state  = env._make_state(vector, False)                     the RL library's gym wrapper: cast to float32
    action = TimeFeature(GreedyAgent(policy)).eval(state)       ddpg.py:40-41: 21st input = 0.001 x evaluations so far; the network;
                                                                DeterministicPolicyNetwork: tanh(.) * 5 + 0

Here the network is 21 -> 400 -> ReLU -> 300 -> ReLU -> 1 with the tensors of the reference's ``pretrained_models/ddpg_*_extended/policy.pt``
(exported as data by ``data/make_actor_weights.py`` next to this file, into ``data/``), float32 like the reference's, squash ``tanh * tanh_scale + tanh_mean``, in
two interchangeable engines:

* ``engine="hip"`` (default): ONE launch per evaluation, ``k_actor_eval`` (``stmpc_actor_eval_device``): state vector, both hidden layers on
  the matrix cores (``v_mfma_f32_16x16x4_f32``, weights pre-packed in lane order), output layer and squash; activations stay in LDS;
* ``engine="torch"``: the input vectors from ``k_policy_features`` (``stmpc_policy_features_device``), the network on PyTorch-ROCm (three
  rocBLAS GEMMs + elementwise kernels) -- BASELINE configs[2]'s literal wording, and the float32 reference the fused kernel is tested against.

Parity: the 20 state-vector entries and the network's weights are the reference's own (pinned by ``golden_combined_real.npz``); the
float32 cast and the TimeFeature input restate ``autonomous-learning-library`` 0.5.3 (requirements.txt:10), which is absent from the
reference checkout -- parity unpinned for those two steps, and the suite's ``test_actor.py`` measures how much the decisions depend on them.

``DQNActor`` is the same for the reference's second agent, ``DQNAgent.get_control`` (dqn.py:375-380): state vector (no time feature) -> Q ->
``argmax`` -> the action table, one launch (``k_qactor_eval``), from a ``learner.DQNLearner`` where it lies or from its exported file.
``QActorPopulation`` is ``ActorPopulation`` for such policies (``k_qactor_eval_pop``: P Q-networks, one launch; ``C51ActorPopulation`` is its
subclass for categorical policies, ``k_c51actor_eval_pop``), and ``population_of`` picks
between the two from the members' kind.  ``C51Actor`` is ``DQNActor`` for a ``learner.C51Learner``'s categorical network (``k_c51actor_eval``: the
expected values of the return distributions in Q's place); ``C51ActorPopulation`` is the population that takes it.
"""
import os

import numpy as np

from . import _capi
from .config import Settings

ACTOR_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")      # package data: the reference's pretrained_models/*/policy.pt as tensors
#: MODEL_NAME of the shipped evaluation configs -> exported tensor file (configs/combined_<traffic>_1.json:4)
PRETRAINED = ("low1", "medium1", "default1", "moderate1", "fast1")


def weights_path(name):
    """``name``: "medium1", "ddpg_medium1", "runs/ddpg_medium1_extended" (a config's MODEL_NAME) or a path to an .npz file."""
    if os.path.exists(name):
        return name
    short = os.path.basename(name)
    if short.startswith("ddpg_"):
        short = short[5:]
    if short.endswith("_extended"):
        short = short[:-9]
    path = os.path.join(ACTOR_DIR, "actor_ddpg_%s.npz" % short)
    if not os.path.exists(path):
        raise FileNotFoundError("no exported actor for %r (have: %s); data/make_actor_weights.py writes them" % (name, ", ".join(PRETRAINED)))
    return path


def load_weights(name):
    with np.load(weights_path(name)) as z:
        w = {k: np.array(z[k]) for k in ("w0", "b0", "w1", "b1", "w2", "b2")}
        w["tanh_scale"], w["tanh_mean"] = float(z["tanh_scale"]), float(z["tanh_mean"])
    assert w["w0"].shape[0] == w["b0"].shape[0] == w["w1"].shape[1] and w["w1"].shape[0] == w["w2"].shape[1] and w["w2"].shape[0] == 1
    return w


def state_vector_host(S, ego4, xs, vs, accs, evaluations=None):
    """Host twin of ``k_policy_features`` for ONE state (numpy, same operations): dqn.get_state_vector_from_base_state, the float32 cast and,
    if ``evaluations`` is given, the TimeFeature input.  Used by the CPU suite; the product path is the kernel."""
    fc = _capi.FeaturesCfg.from_settings(S, time_feature=evaluations is not None)
    tw = 4 if fc.use_acceleration else 3
    out = np.zeros((fc.cars_ahead + fc.cars_behind) * tw + 4 + (1 if fc.time_feature else 0), dtype=np.float32)
    ex, ey, ev, ea = (float(q) for q in ego4)

    def put(slot, i):
        t = []
        if fc.use_acceleration:
            t.append(accs[i] / 9.0 if fc.normalize else accs[i])
        dv = vs[i] - ev if fc.use_speed_difference else vs[i]
        t.append(dv / fc.max_speed if fc.normalize else dv)
        dx = xs[i] - ex
        t.append(dx / fc.sensor_radius if fc.normalize else dx)
        t.append(1.0)
        out[slot * tw:(slot + 1) * tw] = np.array(t, dtype=np.float64).astype(np.float32)
    front = [i for i in range(len(xs)) if xs[i] > ex][::-1][:fc.cars_ahead]
    back = [i for i in range(len(xs)) if not xs[i] > ex][:fc.cars_behind]
    for s_, i in enumerate(front):
        put(s_, i)
    for s_, i in enumerate(back):
        put(fc.cars_ahead + s_, i)
    base = (fc.cars_ahead + fc.cars_behind) * tw
    ego = [ev / fc.max_speed, ea / 9.0, ex / 300.0, ey / 100.0] if fc.normalize else [ev, ea, ex, ey]
    out[base:base + 4] = np.array(ego, dtype=np.float64).astype(np.float32)
    if fc.time_feature:
        out[base + 4] = np.float32(fc.time_scale) * np.float32(evaluations)
    return out


class DDPGActor:
    """``policy(step, cur_ego4, k, cur_ox, cur_ov, cur_oa) -> jerk[N]`` for ``combined.decide_batch_device``.

    Holds the per-episode evaluation counters of the reference's TimeFeature wrapper (``evals``, int32 [N] on the device;
    ``reset(mask)`` zeroes them where an episode ends, as ``end_episode_callback`` does, ddpg.py:89-90).
    ``engine``: "hip" (one fused launch) or "torch" (see the module text).  ``dtype`` (torch engine only): torch.float32 evaluates the network
    as the reference does; torch.float64 is offered for sensitivity measurements.  ``time_feature=False`` feeds 0 as the 21st input (the
    sensitivity test's other arm; the evaluation counters still run)."""

    def __init__(self, name, n, ctx, S, device=None, dtype=None, time_feature=True, engine="hip"):
        import torch
        self.torch = torch
        self.name = name
        self.ctx = ctx
        self.n = int(n)
        if engine not in ("hip", "torch"):
            raise ValueError("engine must be 'hip' or 'torch'")
        if dtype is not None and dtype != torch.float32 and engine == "hip":
            engine = "torch"                      # the fused kernel is float32 only
        self.engine = engine
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.dtype = dtype or torch.float32
        w = load_weights(name)
        t = lambda a: torch.as_tensor(a, device=dev).to(self.dtype)
        self.w0t, self.b0 = t(w["w0"]).t().contiguous(), t(w["b0"])
        self.w1t, self.b1 = t(w["w1"]).t().contiguous(), t(w["b1"])
        self.w2t, self.b2 = t(w["w2"]).t().contiguous(), t(w["b2"])
        self.scale, self.mean = w["tanh_scale"], w["tanh_mean"]
        self.fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=True)
        if not time_feature:
            self.fcfg.time_scale = 0.0            # the input reads 0 x evaluations
        self.flen = (self.fcfg.cars_ahead + self.fcfg.cars_behind) * (4 if self.fcfg.use_acceleration else 3) + 5
        if self.flen != self.w0t.shape[0]:
            raise ValueError("the actor takes %d inputs, the state vector of these settings has %d" % (self.w0t.shape[0], self.flen))
        self.evals = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.feat = torch.empty(self.n, self.flen, dtype=torch.float32, device=dev)
        self.jerk = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.keep_features = False                # hip engine: also write the input vectors to ``self.feat`` (parity checks)
        self.shape = (int(w["w0"].shape[1]), int(w["w0"].shape[0]), int(w["w1"].shape[0]))      # n_in, h1, h2
        self.handle = ctx.actor_create(w) if engine == "hip" else None

    @classmethod
    def from_learner(cls, learner, n, ctx, S, target=False, time_feature=True):
        """A zero-copy VIEW of a ``learner.DDPGLearner``'s online (``target=True``: target) actor (``stmpc_actor_view_ddpg``; hip engine only):
        the learner keeps both packed for the kernel after every update, so nothing is exported, written or uploaded, and an evaluation queued
        after an update on the same stream sees the updated weights (across streams the order is the caller's).  The arithmetic is the fused
        kernel's float32 chain, as for the learner's exported file.  The view holds the learner, so the learner cannot be collected first."""
        import torch
        self = cls.__new__(cls)
        self.torch, self.ctx, self.n, self.engine, self.dtype = torch, ctx, int(n), "hip", torch.float32
        self.learner, self.target = learner, bool(target)
        self.name = "view of %r (%s actor)" % (learner, "target" if target else "online")
        c = learner.cfg
        self.scale, self.mean, self.shape = c.tanh_scale, c.tanh_mean, (c.n_obs + 1, c.h1, c.h2)
        self._buffers(S, time_feature, learner.device)
        self.handle = ctx.actor_view_ddpg(learner.handle, target)
        return self

    def _buffers(self, S, time_feature, dev):
        torch = self.torch
        self.fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=True)
        if not time_feature:
            self.fcfg.time_scale = 0.0
        self.flen = (self.fcfg.cars_ahead + self.fcfg.cars_behind) * (4 if self.fcfg.use_acceleration else 3) + 5
        if self.flen != self.shape[0]:
            raise ValueError("the actor takes %d inputs, the state vector of these settings has %d" % (self.shape[0], self.flen))
        self.evals = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.feat = torch.empty(self.n, self.flen, dtype=torch.float32, device=dev)
        self.jerk = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.keep_features = False

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                self.ctx.actor_destroy(self.handle)
            except Exception:
                pass
            self.handle = None

    def reset(self, mask=None):
        if mask is None:
            self.evals.zero_()
        else:
            self.evals.masked_fill_(mask, 0)

    def _check_rows(self, cur_ego4, k, cur_ox, cur_ov, cur_oa):
        # the kernels are launched for self.n states and write self.jerk / self.feat / self.evals of that length
        _check_rows(self.n, cur_ego4, k, cur_ox, cur_ov, cur_oa)

    def features(self, step, cur_ego4, k, cur_ox, cur_ov, cur_oa, stream=None):
        torch = self.torch
        self._check_rows(cur_ego4, k, cur_ox, cur_ov, cur_oa)
        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.ctx.policy_features_device(self.fcfg, self.n, cur_ox.shape[1], step, cur_ego4.data_ptr(), k.data_ptr(), cur_ox.data_ptr(), cur_ov.data_ptr(),
                                        cur_oa.data_ptr() if cur_oa is not None else 0, self.evals.data_ptr(), self.feat.data_ptr(), self.flen, stream)
        return self.feat

    def forward(self, feat):
        torch = self.torch
        x = feat.to(self.dtype)
        h = torch.relu(torch.addmm(self.b0, x, self.w0t))
        h = torch.relu(torch.addmm(self.b1, h, self.w1t))
        return torch.tanh(torch.addmm(self.b2, h, self.w2t)).squeeze(1) * self.scale + self.mean

    def __call__(self, step, cur_ego4, k, cur_ox, cur_ov, cur_oa):
        if self.engine == "hip":
            self._check_rows(cur_ego4, k, cur_ox, cur_ov, cur_oa)
            stream = self.torch.cuda.current_stream().cuda_stream
            self.ctx.actor_eval_device(self.handle, self.fcfg, self.n, cur_ox.shape[1], step, cur_ego4.data_ptr(), k.data_ptr(), cur_ox.data_ptr(),
                                       cur_ov.data_ptr(), cur_oa.data_ptr() if cur_oa is not None else 0, self.evals.data_ptr(),
                                       self.feat.data_ptr() if self.keep_features else 0, self.flen, self.jerk.data_ptr(), stream)
            return self.jerk
        with self.torch.no_grad():
            feat = self.features(step, cur_ego4, k, cur_ox, cur_ov, cur_oa)
            return self.forward(feat).to(self.torch.float64)


def _check_rows(n, cur_ego4, k, cur_ox, cur_ov, cur_oa):
    for name, t_ in (("cur_ego4", cur_ego4), ("k", k), ("cur_ox", cur_ox), ("cur_ov", cur_ov), ("cur_oa", cur_oa)):
        if t_ is not None and t_.shape[0] != n:
            raise ValueError("%s has %d rows, this actor was built for %d states" % (name, t_.shape[0], n))


class ActorPopulation:
    """P actors, each on its own slice of one batch, evaluated in ONE launch (``k_actor_eval_pop``, csrc/stmpc_actor_pop_kernels.hpp): the
    reference's per-model ``EVALUATE_COMBINED_DDPG`` runs (``DDPGAgent.load`` + ``get_control`` for the MODEL_NAME of each
    ``configs/combined_<traffic>_{1,2,3}.json``) side by side, and the evaluation ``train_ddpg_all_with_lr_drop`` ends with, for every member
    of a trained population at once.

    ``members``: a list whose items are shipped names or ``.npz`` paths, ``learner.DDPGLearner``s (a zero-copy view each, see
    ``DDPGActor.from_learner``) or existing hip-engine ``DDPGActor``s; or a ``learner.DDPGPopulation`` (one view per member).  The members share the
    network's shape; the squash may differ.  Member m evaluates rows [m * n_per_member, (m + 1) * n_per_member) and is bit-identical to a lone
    ``DDPGActor`` on that slice.  Same call signature as ``DDPGActor``: ``combined.decide_batch_device`` and ``episodes.EpisodeRunner`` take it as
    they are (the runner then reports per member).  In a runner the members face different environments of one world: identically distributed
    episodes, not common random numbers."""

    def __init__(self, members, n_per_member, ctx, S, time_feature=True):
        import torch
        self.torch, self.ctx = torch, ctx
        if hasattr(members, "member") and hasattr(members, "P"):                 # a learner.DDPGPopulation
            members = [members.member(m) for m in range(members.P)]
        members = list(members)
        if not 1 <= len(members) <= _capi.DDPG_POP_MAX:
            raise ValueError("a population has 1 ... %d members, not %d" % (_capi.DDPG_POP_MAX, len(members)))
        self.P, self.n_per_member = len(members), int(n_per_member)
        if self.n_per_member < 1:
            raise ValueError("n_per_member must be positive")
        self.n = self.P * self.n_per_member
        self.members = []
        for item in members:
            if isinstance(item, DDPGActor):
                if item.engine != "hip":
                    raise ValueError("a population evaluates hip-engine actors, not %r" % (item.engine,))
                a = item
            elif isinstance(item, (str, os.PathLike)):
                a = DDPGActor(os.fspath(item), 1, ctx, S, time_feature=time_feature)      # (its own row buffers stay unused: the population has them)
            elif hasattr(item, "export_actor") and hasattr(item, "handle"):     # a learner.DDPGLearner
                a = DDPGActor.from_learner(item, 1, ctx, S, time_feature=time_feature)
            else:
                raise ValueError("a member is a shipped name, an .npz path, a DDPGLearner or a DDPGActor, not %r" % (item,))
            self.members.append(a)
        pad = lambda sh: (sh[0], (sh[1] + 15) & ~15, (sh[2] + 15) & ~15)
        for m, a in enumerate(self.members):
            if pad(a.shape) != pad(self.members[0].shape):
                raise ValueError("member %d is %d -> %d -> %d -> 1, member 0 is %d -> %d -> %d -> 1: one launch needs one shape" % ((m,) + a.shape + self.members[0].shape))
        dev = torch.device("cuda", torch.cuda.current_device())
        self.fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=True)
        if not time_feature:
            self.fcfg.time_scale = 0.0
        self.flen = self.members[0].flen
        self.evals = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.feat = torch.empty(self.n, self.flen, dtype=torch.float32, device=dev)
        self.jerk = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.keep_features = False
        self.handle = ctx.actor_pop_create([a.handle for a in self.members])

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                self.ctx.actor_pop_destroy(self.handle)
            except Exception:
                pass
            self.handle = None

    def reset(self, mask=None):
        if mask is None:
            self.evals.zero_()
        else:
            self.evals.masked_fill_(mask, 0)

    def __call__(self, step, cur_ego4, k, cur_ox, cur_ov, cur_oa):
        _check_rows(self.n, cur_ego4, k, cur_ox, cur_ov, cur_oa)
        stream = self.torch.cuda.current_stream().cuda_stream
        self.ctx.actor_pop_eval_device(self.handle, self.fcfg, self.n_per_member, cur_ox.shape[1], step, cur_ego4.data_ptr(), k.data_ptr(), cur_ox.data_ptr(),
                                       cur_ov.data_ptr(), cur_oa.data_ptr() if cur_oa is not None else 0, self.evals.data_ptr(),
                                       self.feat.data_ptr() if self.keep_features else 0, self.flen, self.jerk.data_ptr(), stream)
        return self.jerk


class DQNActor:
    """The reference's second agent as a policy: ``DQNAgent.get_control`` (dqn.py:375-380) -- state vector -> Q -> ``argmax`` ->
    ``JERK_VALUES_DQN[a]`` -- for ``n`` states in ONE launch (``k_qactor_eval``, csrc/stmpc_qactor_kernels.hpp), with ``DDPGActor``'s call:
    ``policy(step, cur_ego4, k, cur_ox, cur_ov, cur_oa) -> jerk[n]`` (fp64, on the device), so ``combined.decide_batch_device`` and
    ``episodes.EpisodeRunner(controller="combined" | "first_step")`` take it as they are.

    ``source``: a file written by ``learner.DQNLearner.export_q`` (w0, b0, w1, b1, action_values); ``action_values`` replaces the file's table.
    ``mode``: "jerk" (the table holds jerks: sumo-jerk-v0) or "acceleration" (it holds accelerations: sumo-accel-v0; the jerk is then
    ``clip((table[a] - ego acceleration) / TICK_LENGTH, MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK)`` in fp64 -- ``AccelerationEnv._do_action``'s
    projected jerk before its speed clamp, with the state's own acceleration for the env's previous one.  The reference has no evaluator for that
    env: the rule is this project's; ``q_policy_host`` is its host twin).  The constants are read from ``S`` when the actor is built.

    The network has no time feature: ``reset`` does nothing.  ``.action`` (int32 [n]) is filled by every call; ``keep_features`` / ``keep_q`` fill
    ``.feat`` (float32 [n][n_in]) and ``.q`` (float32 [n][A]) too.  Q, the index and the jerk are bit for bit what ``DQNLearner.act`` gives on the
    same input vectors: the kernel runs the learner's own forward pass and argmax."""

    MODES = tuple(_capi.QACTOR_MODES)

    def __init__(self, source, n, ctx, S, mode="jerk", action_values=None):
        with np.load(os.fspath(source)) as z:
            if "n_atoms" in z.files:
                raise ValueError("%s holds a categorical (C51) network (it has n_atoms): load it with C51Actor" % os.fspath(source))
            net = {k: np.array(z[k], dtype=np.float32) for k in ("w0", "b0", "w1", "b1")}
            table = np.array(z["action_values"], dtype=np.float64) if action_values is None else action_values
        self._setup(n, ctx, S, mode, table, (int(net["w0"].shape[1]), int(net["w0"].shape[0]), int(net["w1"].shape[0])))
        self.name, self.learner, self.target = os.fspath(source), None, False
        self.handle = ctx.qactor_create(net, self.action_values, _capi.QACTOR_MODES[self.mode])
        self._limits(S)

    @classmethod
    def from_learner(cls, learner, n, ctx, S, target=False, mode=None):
        """A zero-copy VIEW of a ``learner.DQNLearner``'s online (``target=True``: target) Q-network (``stmpc_qactor_view_dqn``): the learner keeps
        both packed for the kernel after every update, so nothing is exported or uploaded, and an evaluation queued after an update on the same
        stream sees the update.  The table is ``learner.action_values``; ``mode`` defaults to the kind of env the learner was built from
        ("acceleration" for sumo-accel-v0, else -- and without an env -- "jerk").  Evaluating changes nothing of the learner's.  The view holds
        the learner, so the learner cannot be collected first."""
        if _is_c51_learner(learner):
            raise ValueError("%r is a C51Learner: its handle is no DQN learner's; build the view with C51Actor.from_learner" % (learner,))
        return cls._view(learner, n, ctx, S, target, mode, lambda self: ctx.qactor_view_dqn(learner.handle, self.action_values, self.target, _capi.QACTOR_MODES[self.mode]))

    @classmethod
    def _view(cls, learner, n, ctx, S, target, mode, make_handle):
        self = cls.__new__(cls)
        if mode is None:
            mode = "acceleration" if getattr(learner, "env_id", None) == "sumo-accel-v0" else "jerk"
        c = learner.cfg
        self._setup(n, ctx, S, mode, learner.action_values, (c.n_obs, c.h1, c.n_actions))
        self.learner, self.target = learner, bool(target)
        self.name = "view of %r (%s network)" % (learner, "target" if target else "online")
        self.handle = make_handle(self)
        self._limits(S)
        return self

    def _setup(self, n, ctx, S, mode, table, shape):
        import torch
        self.handle = None
        self.torch, self.ctx, self.n, self.engine, self.dtype, self.shape = torch, ctx, int(n), "hip", torch.float32, shape
        if self.n < 1:
            raise ValueError("n must be positive")
        if mode not in _capi.QACTOR_MODES:
            raise ValueError("mode must be one of %s, not %r" % (", ".join(map(repr, _capi.QACTOR_MODES)), mode))
        self.mode = mode
        self.action_values = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
        if self.action_values.size != shape[2]:
            raise ValueError("the action table has %d entries, the network %d actions" % (self.action_values.size, shape[2]))
        if not np.isfinite(self.action_values).all():
            raise ValueError("the action table has entries that are not finite")
        self.fcfg = _capi.FeaturesCfg.from_settings(S, time_feature=False)
        self.flen = (self.fcfg.cars_ahead + self.fcfg.cars_behind) * (4 if self.fcfg.use_acceleration else 3) + 4
        if self.flen != shape[0]:
            raise ValueError("the Q-network takes %d inputs, the state vector of these settings has %d" % (shape[0], self.flen))
        dev = torch.device("cuda", torch.cuda.current_device())
        self.feat = torch.empty(self.n, self.flen, dtype=torch.float32, device=dev)
        self.q = torch.empty(self.n, shape[2], dtype=torch.float32, device=dev)
        self.action = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.jerk = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.keep_features = self.keep_q = False

    def _limits(self, S):
        self.limits = (float(S.TICK_LENGTH), float(S.MINIMUM_NEGATIVE_JERK), float(S.MAXIMUM_POSITIVE_JERK))
        if self.mode == "acceleration":
            self.ctx.qactor_set_limits(self.handle, *self.limits)

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                self.ctx.qactor_destroy(self.handle)
            except Exception:
                pass
            self.handle = None

    def reset(self, mask=None):
        """Nothing: there are no per-episode evaluation counters without a time feature."""

    def __call__(self, step, cur_ego4, k, cur_ox, cur_ov, cur_oa):
        _check_rows(self.n, cur_ego4, k, cur_ox, cur_ov, cur_oa)
        stream = self.torch.cuda.current_stream().cuda_stream
        self.ctx.qactor_eval_device(self.handle, self.fcfg, self.n, cur_ox.shape[1], step, cur_ego4.data_ptr(), k.data_ptr(), cur_ox.data_ptr(), cur_ov.data_ptr(),
                                    cur_oa.data_ptr() if cur_oa is not None else 0, self.feat.data_ptr() if self.keep_features else 0, self.flen,
                                    self.action.data_ptr(), self.q.data_ptr() if self.keep_q else 0, self.jerk.data_ptr(), stream)
        return self.jerk


class C51Actor(DQNActor):
    """``DQNActor`` for a categorical (C51) network -- the distributional head of the reference's third agent (rainbow.py) doing
    ``DQNAgent.get_control``'s job (dqn.py:375-380): state vector -> logits -> E[Z(s, a)] of every action -> first maximum -> the action table, for
    ``n`` states in ONE launch (``k_c51actor_eval``, csrc/stmpc_c51actor_kernels.hpp).  A subclass: whatever takes a ``DQNActor`` --
    ``combined.decide_batch_device``, ``episodes.EpisodeRunner``, ``learner.evaluate_dqn``, ``vec_env.QCombinedShieldVecEnv`` -- takes it.

    ``source``: a file written by ``learner.C51Learner.export_q`` (w0, b0, w1 [A * n_atoms][h1], b1, action_values, n_atoms, v_min, v_max, dueling).
    ``dueling`` = 1: w1 and b1 have (A + 1) * n_atoms rows, the value block last, and the logits are the dueling head's
    (``stmpc_dueling_c51actor_create``); a file without the key has the plain head.  ``.dueling`` says which.
    ``.shape`` is (n_in, h1, A); ``.n_atoms``, ``.v_min``, ``.v_max`` the head's support; ``.q`` (with ``keep_q``) holds the expected values,
    float32 [n][A].  ``mode``, the call, ``reset``, ``keep_features`` and ``keep_q`` are ``DQNActor``'s.  The expected values, the index and the jerk
    are bit for bit what ``C51Learner.act`` gives on the same input vectors; ``c51_policy_host`` is the host twin.  ``QActorPopulation`` refuses a
    C51 policy: C51 policies share a population of their own, ``C51ActorPopulation``."""

    def __init__(self, source, n, ctx, S, mode="jerk", action_values=None):
        with np.load(os.fspath(source)) as z:
            if "n_atoms" not in z.files:
                raise ValueError("%s has no n_atoms: it is not a C51Learner.export_q file (a DQNLearner's file goes to DQNActor)" % os.fspath(source))
            net = {k: np.array(z[k], dtype=np.float32) for k in ("w0", "b0", "w1", "b1")}
            table = np.array(z["action_values"], dtype=np.float64) if action_values is None else action_values
            self.n_atoms, self.v_min, self.v_max = int(z["n_atoms"]), float(z["v_min"]), float(z["v_max"])
            self.dueling = bool(int(z["dueling"])) if "dueling" in z.files else False
        A, rest = divmod(int(net["w1"].shape[0]), self.n_atoms) if self.n_atoms >= 1 else (0, 1)
        if rest or A < 1:
            raise ValueError("the last layer has %d rows, no multiple of n_atoms = %d" % (net["w1"].shape[0], self.n_atoms))
        if self.dueling:
            A -= 1                                                  # (the value block)
            if A < 1:
                raise ValueError("a dueling head has the value block and at least one advantage block; the last layer has %d rows" % net["w1"].shape[0])
        self._setup(n, ctx, S, mode, table, (int(net["w0"].shape[1]), int(net["w0"].shape[0]), A))
        self.name, self.learner, self.target = os.fspath(source), None, False
        self.handle = ctx.c51actor_create(net, self.action_values, self.n_atoms, self.v_min, self.v_max, _capi.QACTOR_MODES[self.mode], dueling=self.dueling)
        self._limits(S)

    @classmethod
    def from_learner(cls, learner, n, ctx, S, target=False, mode=None):
        """``DQNActor.from_learner`` for a ``learner.C51Learner``: a zero-copy VIEW of its online (``target=True``: target) logits network
        (``stmpc_c51actor_view``), live across updates on the same stream; evaluating changes nothing of the learner's."""
        if not _is_c51_learner(learner):
            raise ValueError("%r is no C51Learner (DQNActor.from_learner views a DQNLearner)" % (learner,))
        c = learner.cfg

        def make_handle(self):
            self.n_atoms, self.v_min, self.v_max, self.dueling = int(c.n_atoms), float(c.v_min), float(c.v_max), bool(getattr(c, "dueling", False))
            return ctx.c51actor_view(learner.handle, self.action_values, self.target, _capi.QACTOR_MODES[self.mode])
        return cls._view(learner, n, ctx, S, target, mode, make_handle)


def _is_c51_learner(item):
    return hasattr(item, "handle") and hasattr(getattr(item, "cfg", None), "n_atoms")      # a learner.C51Learner: its handle is a stmpc_c51's


def _is_dqn_learner(item):
    # a learner.DQNLearner (learner.py imports this module); a C51Learner has the same methods, and a handle of another type
    return hasattr(item, "export_q") and hasattr(item, "handle") and not _is_c51_learner(item)


def _is_c51_file(item):
    if not isinstance(item, (str, os.PathLike)) or not os.path.isfile(os.fspath(item)):
        return False
    try:
        with np.load(os.fspath(item)) as z:
            return "n_atoms" in getattr(z, "files", ())
    except Exception:
        return False


def refuse_c51_members(items, who):
    """ValueError if a member of ``items`` is a C51 policy (a ``C51Actor``, a ``learner.C51Learner``, a ``C51Learner.export_q`` file): one launch of a
    population needs one head.  Reads the items alone: nothing is built and the library is not called."""
    bad = [m for m, item in enumerate(items) if isinstance(item, C51Actor) or _is_c51_learner(item) or _is_c51_file(item)]
    if bad:
        raise ValueError("%s: members %s are categorical (C51) policies, and a population of C51 policies does not exist (one launch needs one head); "
                         "evaluate a C51 policy alone, with learner.evaluate_dqn or a C51Actor -- or C51 policies together, in a population of their own: "
                         "actor.C51ActorPopulation, learner.evaluate_c51_members" % (who, ", ".join(map(str, bad))))


def _is_q_member(item):
    return isinstance(item, DQNActor) or _is_dqn_learner(item)


class QActorPopulation:
    """P Q-networks, each on its own slice of one batch, evaluated in ONE launch (``k_qactor_eval_pop``, csrc/stmpc_qactor_pop_kernels.hpp):
    ``ActorPopulation`` for ``DQNActor``s -- the reference's run-by-run comparisons of its DQN agent (double against plain targets, clipped against
    unclipped, the freeze period, prioritised against uniform replay, seeds, traffic types; ``DQNAgent.get_control``, dqn.py:375-380) side by side.

    ``members``: a list whose items are files written by ``learner.DQNLearner.export_q`` (jerk mode, the file's table), ``learner.DQNLearner``s (a
    zero-copy view of the online network each, see ``DQNActor.from_learner``) or existing ``DQNActor``s (file actors or views, online or target,
    either mode); or a ``learner.DQNPopulation`` (one view of ``member(m)`` each).  The members share n_in, the hidden width padded to a multiple of
    16 and the action count; table, mode, limits and online / target may differ.  Member m evaluates rows [m * n_per_member, (m + 1) *
    n_per_member) and is bit-identical to a lone ``DQNActor`` on that slice.  A view is live: an evaluation queued after an update on the same
    stream sees it.  ``DDPGActor``'s call signature: ``combined.decide_batch_device`` and ``episodes.EpisodeRunner`` take it as they are (the
    runner then reports per member).  ``.jerk`` (fp64 [n]) and ``.action`` (int32 [n]) are filled by every call; ``keep_features`` / ``keep_q`` fill
    ``.feat`` (float32 [n][n_in]) and ``.q`` (float32 [n][A]) too.  There is no time feature: ``reset`` does nothing."""

    def _take(self, members, n_per_member, refuse=None):
        """What both kinds of population begin with: a learner population as its members, ``refuse`` on the list, the counts (``P``,
        ``n_per_member``, ``n``).  Returns the list."""
        if hasattr(members, "member") and hasattr(members, "P"):                 # a learner.DQNPopulation (C51Population)
            members = [members.member(m) for m in range(members.P)]
        members = list(members)
        if refuse is not None:
            refuse(members)
        if not 1 <= len(members) <= _capi.DDPG_POP_MAX:
            raise ValueError("a population has 1 ... %d members, not %d" % (_capi.DDPG_POP_MAX, len(members)))
        self.P, self.n_per_member = len(members), int(n_per_member)
        if self.n_per_member < 1:
            raise ValueError("n_per_member must be positive")
        self.n = self.P * self.n_per_member
        return members

    def _build(self, members, ctx, S, shape, actor_cls, is_learner, create):
        """... and end with, once kinds and shapes were checked: a one-row ``actor_cls`` per member that is not one yet, the row buffers, the handle
        ``create`` makes of the members' handles."""
        import torch
        self.torch, self.ctx, self.engine, self.dtype, self.shape = torch, ctx, "hip", torch.float32, shape
        self.members = []
        for item in members:
            if isinstance(item, actor_cls):
                a = item
            elif is_learner(item):
                a = actor_cls.from_learner(item, 1, ctx, S)             # (its own row buffers stay unused: the population has them)
            else:
                a = actor_cls(item, 1, ctx, S)
            self.members.append(a)
        self.fcfg, self.flen = self.members[0].fcfg, self.members[0].flen
        dev = torch.device("cuda", torch.cuda.current_device())
        self.feat = torch.empty(self.n, self.flen, dtype=torch.float32, device=dev)
        self.q = torch.empty(self.n, self.shape[2], dtype=torch.float32, device=dev)
        self.action = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.jerk = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.keep_features = self.keep_q = False
        self.handle = create([a.handle for a in self.members])

    def __init__(self, members, n_per_member, ctx, S):
        members = self._take(members, n_per_member, lambda items: refuse_c51_members(items, "QActorPopulation"))
        # kinds and shapes first, from the host's data alone: nothing is built for a list that will be refused
        shapes = []
        for item in members:
            if isinstance(item, DQNActor):
                shapes.append(tuple(item.shape))
            elif _is_dqn_learner(item):
                shapes.append((item.cfg.n_obs, item.cfg.h1, item.cfg.n_actions))
            elif isinstance(item, (str, os.PathLike)):
                with np.load(os.fspath(item)) as z:
                    shapes.append((int(z["w0"].shape[1]), int(z["w0"].shape[0]), int(z["w1"].shape[0])))
            else:
                raise ValueError("a member is an export_q file, a DQNLearner or a DQNActor, not %r" % (item,))
        pad = lambda sh: (sh[0], (sh[1] + 15) & ~15, sh[2])
        for m, sh in enumerate(shapes):
            if pad(sh) != pad(shapes[0]):
                raise ValueError("member %d is %d -> %d -> %d, member 0 is %d -> %d -> %d: one launch needs one shape" % ((m,) + sh + shapes[0]))
        self._build(members, ctx, S, shapes[0], DQNActor, _is_dqn_learner, lambda handles: ctx.qactor_pop_create(handles))

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                self.ctx.qactor_pop_destroy(self.handle)
            except Exception:
                pass
            self.handle = None

    def reset(self, mask=None):
        """Nothing: there are no per-episode evaluation counters without a time feature."""

    def __call__(self, step, cur_ego4, k, cur_ox, cur_ov, cur_oa):
        _check_rows(self.n, cur_ego4, k, cur_ox, cur_ov, cur_oa)
        stream = self.torch.cuda.current_stream().cuda_stream
        self.ctx.qactor_pop_eval_device(self.handle, self.fcfg, self.n_per_member, cur_ox.shape[1], step, cur_ego4.data_ptr(), k.data_ptr(), cur_ox.data_ptr(),
                                        cur_ov.data_ptr(), cur_oa.data_ptr() if cur_oa is not None else 0, self.feat.data_ptr() if self.keep_features else 0,
                                        self.flen, self.action.data_ptr(), self.q.data_ptr() if self.keep_q else 0, self.jerk.data_ptr(), stream)
        return self.jerk


def _is_c51_member(item):
    return isinstance(item, C51Actor) or _is_c51_learner(item) or _is_c51_file(item)


def all_c51(items):
    """True when ``items`` is not empty and every item is a C51 policy (a ``C51Actor``, a ``learner.C51Learner``, a ``C51Learner.export_q`` file):
    what ``C51ActorPopulation`` takes.  Reads the items alone."""
    items = list(items)
    return bool(items) and all(_is_c51_member(item) for item in items)


class C51ActorPopulation(QActorPopulation):
    """``QActorPopulation`` for categorical (C51) policies: P logits networks, each with its own support and on its own slice of one batch,
    evaluated in ONE launch (``k_c51actor_eval_pop``, csrc/stmpc_c51actor_pop_kernels.hpp; ``stmpc_pop_c51actor_create``).  A subclass: whatever
    takes a ``QActorPopulation`` -- ``combined.decide_batch_device``, ``episodes.EpisodeRunner``, ``vec_env.QCombinedShieldVecEnv`` -- takes it, and
    ``__call__``, ``reset``, ``keep_features`` / ``keep_q``, ``P``, ``n_per_member`` and ``n`` are the parent's.

    ``members``: a list whose items are files written by ``learner.C51Learner.export_q`` (jerk mode, the file's table), ``learner.C51Learner``s (a
    zero-copy view of the online network each, see ``C51Actor.from_learner``) or existing ``C51Actor``s (file actors or views, online or target,
    either mode); or a ``learner.C51Population`` (one view of ``member(m)`` each).  The members share n_in, the hidden width padded to a multiple of
    16, the action count, ``n_atoms`` and the head (dueling or not); support, table, mode, limits and online / target may differ.  Kinds and shapes
    are checked from host data before anything is built or the library is called; a DQN member is refused (``QActorPopulation`` is theirs).
    Member m evaluates rows [m * n_per_member, (m + 1) * n_per_member) and is bit-identical to a lone ``C51Actor`` on that slice; its arithmetic
    on the host is ``c51_policy_host`` on that slice.  A view is live, and a view of a noisy learner evaluates the mean weights, as ``C51Actor``
    does.  ``.q`` (with ``keep_q``) holds the expected values, float32 [n][A]; ``.shape`` is (n_in, h1, A) of member 0, ``.n_atoms`` and
    ``.dueling`` the common head."""

    def __init__(self, members, n_per_member, ctx, S):
        members = self._take(members, n_per_member)
        # kinds and shapes first, from the host's data alone: nothing is built for a list that will be refused.  (n_in, h1, A, n_atoms, dueling)
        shapes = []
        for m, item in enumerate(members):
            if isinstance(item, C51Actor):
                shapes.append(tuple(item.shape) + (int(item.n_atoms), bool(item.dueling)))
            elif _is_c51_learner(item):
                c = item.cfg
                shapes.append((c.n_obs, c.h1, c.n_actions, int(c.n_atoms), bool(getattr(c, "dueling", False))))
            elif _is_c51_file(item):
                with np.load(os.fspath(item)) as z:
                    K, duel = int(z["n_atoms"]), bool(int(z["dueling"])) if "dueling" in z.files else False
                    rows = int(z["w1"].shape[0])
                    if K < 1 or rows % K or rows // K - duel < 1:
                        raise ValueError("member %d: the last layer has %d rows, not %s blocks of n_atoms = %d" % (m, rows, "a value block and advantage" if duel else "whole", K))
                    shapes.append((int(z["w0"].shape[1]), int(z["w0"].shape[0]), rows // K - duel, K, duel))
            elif _is_q_member(item) or (isinstance(item, (str, os.PathLike)) and os.path.isfile(os.fspath(item))):
                raise ValueError("member %d is a Q-network (a DQNActor, a DQNLearner or a DQNLearner.export_q file), not a categorical (C51) policy: one launch needs "
                                 "one head; Q-networks share a population of their own, actor.QActorPopulation" % m)
            else:
                raise ValueError("a member is a C51Learner.export_q file, a C51Learner or a C51Actor, not %r" % (item,))
        pad = lambda sh: (sh[0], (sh[1] + 15) & ~15) + sh[2:]
        text = lambda sh: "%d -> %d -> %d x %d atoms%s" % (sh[:4] + (" (dueling)" if sh[4] else "",))
        for m, sh in enumerate(shapes):
            if pad(sh) != pad(shapes[0]):
                raise ValueError("member %d is %s, member 0 is %s: one launch needs one shape and one head" % (m, text(sh), text(shapes[0])))
        self.n_atoms, self.dueling = shapes[0][3], shapes[0][4]
        self._build(members, ctx, S, shapes[0][:3], C51Actor, _is_c51_learner, lambda handles: ctx.c51actor_pop_create(handles))


def population_of(members, n_per_member, ctx, S, **kw):
    """The population for ``members``: a ``QActorPopulation`` when every member is a ``DQNActor`` or a ``learner.DQNLearner`` (a
    ``learner.DQNPopulation`` counts as its members), an ``ActorPopulation`` (with ``kw``) when none is -- names and paths stay DDPG actors, as they
    always were -- and a ValueError for a mix: one launch evaluates one kind of network."""
    items = members
    if hasattr(members, "member") and hasattr(members, "P"):
        items = [members.member(m) for m in range(members.P)]
    items = list(items)
    refuse_c51_members(items, "population_of")
    q = [_is_q_member(item) for item in items]
    if items and all(q):
        return QActorPopulation(items, n_per_member, ctx, S)
    if any(q):
        raise ValueError("members %s are Q-networks and the others are not: DDPG and DQN members do not share a population"
                         % ", ".join(str(m) for m, is_q in enumerate(q) if is_q))
    return ActorPopulation(members, n_per_member, ctx, S, **kw)


def q_policy_host(net, feat, action_values, mode, ego_acc=None, S=Settings, dtype=np.float64):
    """The host twin of ``DQNActor`` in numpy (CPU suite), for input vectors ``feat`` [n][n_in] and a net {w0, b0, w1, b1}: (Q [n][A] in
    ``dtype``, the first maximum's index int64 [n], the jerk fp64 [n]).  ``mode`` "acceleration" needs ``ego_acc`` [n] (the states' ego
    accelerations, fp64) and reads TICK_LENGTH, MINIMUM_NEGATIVE_JERK and MAXIMUM_POSITIVE_JERK of ``S`` (default: the package's Settings)."""
    if mode not in _capi.QACTOR_MODES:
        raise ValueError("mode must be one of %s, not %r" % (", ".join(map(repr, _capi.QACTOR_MODES)), mode))
    f = lambda a: np.asarray(a, dtype=dtype)
    q = np.maximum(f(feat) @ f(net["w0"]).T + f(net["b0"]), 0) @ f(net["w1"]).T + f(net["b1"])
    table = np.asarray(action_values, dtype=np.float64).reshape(-1)
    if table.size != q.shape[1]:
        raise ValueError("the action table has %d entries, the network %d actions" % (table.size, q.shape[1]))
    idx, jerk = _first_maximum_jerk(q, table, mode, ego_acc, S)
    return q, idx, jerk


def _first_maximum_jerk(q, table, mode, ego_acc, S):
    """What ``q_policy_host`` and ``c51_policy_host`` share: the first maximum's index of every row of ``q`` and the jerk it stands for."""
    idx = np.argmax(q, axis=1)                                      # (numpy's argmax returns the first maximum, like torch's)
    jerk = table[idx]
    if mode == "acceleration":
        if ego_acc is None:
            raise ValueError("acceleration mode needs the states' ego accelerations (ego_acc)")
        jerk = np.clip((jerk - np.asarray(ego_acc, dtype=np.float64)) / float(S.TICK_LENGTH), float(S.MINIMUM_NEGATIVE_JERK), float(S.MAXIMUM_POSITIVE_JERK))
    return idx, jerk


def c51_policy_host(net, feat, action_values, mode, n_atoms, v_min, v_max, ego_acc=None, S=Settings, dtype=np.float64):
    """The host twin of ``C51Actor`` in numpy (CPU suite), for input vectors ``feat`` [n][n_in] and a net {w0, b0, w1 [A * n_atoms][h1], b1}: (the
    expected values E[Z(s, a)] [n][A] in ``dtype``, the first maximum's index int64 [n], the jerk fp64 [n]).  Action a's logits are the outputs
    a * n_atoms ... (a + 1) * n_atoms - 1; their softmax (the maximum subtracted) weights the support ``learner.c51_support`` forms.  ``mode``,
    ``ego_acc`` and ``S`` are ``q_policy_host``'s, and so is the acceleration rule."""
    import types
    from .learner import c51_support                                # (learner.py imports this module)
    if mode not in _capi.QACTOR_MODES:
        raise ValueError("mode must be one of %s, not %r" % (", ".join(map(repr, _capi.QACTOR_MODES)), mode))
    n_atoms = int(n_atoms)
    if n_atoms < 2 or not (np.isfinite(v_min) and np.isfinite(v_max) and v_max > v_min):
        raise ValueError("C51 needs n_atoms >= 2 and a finite support with v_max > v_min")
    f = lambda a: np.asarray(a, dtype=dtype)
    logits = np.maximum(f(feat) @ f(net["w0"]).T + f(net["b0"]), 0) @ f(net["w1"]).T + f(net["b1"])
    table = np.asarray(action_values, dtype=np.float64).reshape(-1)
    if table.size * n_atoms != logits.shape[1]:
        raise ValueError("the action table has %d entries, the network %d outputs = %g actions of %d atoms" % (table.size, logits.shape[1], logits.shape[1] / n_atoms, n_atoms))
    z = c51_support(types.SimpleNamespace(n_atoms=n_atoms, v_min=float(v_min), v_max=float(v_max)), dtype)
    x = logits.reshape(logits.shape[0], table.size, n_atoms)
    w = np.exp(x - x.max(axis=2, keepdims=True))
    q = (w * z).sum(axis=2) / w.sum(axis=2)
    idx, jerk = _first_maximum_jerk(q, table, mode, ego_acc, S)
    return q, idx, jerk


def forward_host(w, feat, dtype=np.float32):
    """The network on the host in numpy (CPU suite): feat [n, 21] -> jerk [n]."""
    x = np.asarray(feat, dtype=dtype)
    h = np.maximum(x @ w["w0"].T.astype(dtype) + w["b0"].astype(dtype), 0)
    h = np.maximum(h @ w["w1"].T.astype(dtype) + w["b1"].astype(dtype), 0)
    y = h @ w["w2"].T.astype(dtype) + w["b2"].astype(dtype)
    return np.tanh(y[:, 0]) * dtype(w["tanh_scale"]) + dtype(w["tanh_mean"])
