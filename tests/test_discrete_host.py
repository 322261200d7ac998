"""The discrete learners' host path (csrc/stmpc_learner.hip: stmpc_dqn_*, stmpc_c51_*, stmpc_pop_dqn_*, stmpc_pop_c51_*): what the C entries
refuse, for both heads from one table, with the message compared for equality.  test_dqn.py, test_c51.py and their population suites pin every
entry on its normal path bit for bit; this module pins the other side: which check fires, in which order, with which words.

Every case is a refusal in front of any launch (or the N == 0 early return): nothing here runs a kernel beyond what create itself does.  The shape
is the smallest one, n_obs 4, h1 16, 3 actions, batch 8, capacity 64 and 5 atoms.  One check cannot fire there: "network too wide for one
workgroup's LDS" needs a tile of more than 159 KB, which no DQN shape inside the other limits has (the widest is 136 KB) and of the C51 shapes only
those near h1 1024 with 1024 logits of one action; that C51 case is in the table at its own shape.
"""
import ctypes as C

import pytest

from stmpc_testlib import capi as _capi

pytestmark = pytest.mark.gpu

SHAPE = dict(n_obs=4, h1=16, n_actions=3, batch=8, capacity=64, target_period=10, double_dqn=1, clip_targets=0, replay_start=0, seed=3, gamma=0.99, beta1=0.9,
             beta2=0.999, eps=1e-8, clip_min=-20.0, clip_max=10.0)
SUPPORT = dict(v_min=-10.0, v_max=10.0, n_atoms=5)
INF, NAN = float("inf"), float("nan")

# what differs between the heads: the cfg, the entries' names, the head's name in two messages, and the entries a borrowed member is sent to
HEADS = {
    "dqn": dict(name="DQN", lone="stmpc_dqn_", pop="stmpc_pop_dqn_", nstep="stmpc_nstep_enable_dqn", extra={},
                per_on_pop="stmpc_pop_dqn_per_enable", nstep_on_pop="stmpc_pop_nstep_enable_dqn"),
    "c51": dict(name="C51", lone="stmpc_c51_", pop="stmpc_pop_c51_", nstep="stmpc_c51_multi_step_enable", extra=SUPPORT,
                per_on_pop="stmpc_pop_c51_per_enable", nstep_on_pop="stmpc_pop_c51_multi_step_enable"),
}

N_ACTIONS = "n_actions must be in 1 ... 256"
SHAPE_MSG = "%s network shape out of range (n_obs <= 31, hidden width <= 1024)"
BATCH = "batch must be in 1 ... 8192"
PERIOD = "target_period must be at least 1"
CAPACITY = "capacity must be positive and replay_start below it"
CONSTANTS = "%s constants out of range"
# the checks both heads make, in the order create makes them: (the fields that are wrong, the message; %s: the head's name)
SHARED_CREATE = [
    (dict(n_actions=0), N_ACTIONS), (dict(n_actions=257), N_ACTIONS),
    (dict(n_obs=0), SHAPE_MSG), (dict(n_obs=32), SHAPE_MSG), (dict(h1=0), SHAPE_MSG), (dict(h1=1025), SHAPE_MSG),
    (dict(batch=0), BATCH), (dict(batch=8193), BATCH),
    (dict(target_period=0), PERIOD),
    (dict(capacity=0), CAPACITY), (dict(replay_start=-1), CAPACITY), (dict(replay_start=64), CAPACITY),
    (dict(gamma=-0.5), CONSTANTS), (dict(gamma=INF), CONSTANTS), (dict(gamma=NAN), CONSTANTS), (dict(beta1=1.0), CONSTANTS), (dict(beta1=-0.1), CONSTANTS),
    (dict(beta2=1.0), CONSTANTS), (dict(beta2=NAN), CONSTANTS), (dict(eps=0.0), CONSTANTS),
]
SUPPORT_MSG = "the support needs finite v_min < v_max"
HEAD_CREATE = {
    "dqn": [(dict(clip_targets=1, clip_min=1.0, clip_max=0.0), CONSTANTS), (dict(clip_targets=1, clip_min=NAN), CONSTANTS),
            # two faults: n_actions is looked at before the shape, the batch before the target period
            (dict(n_actions=0, n_obs=0), N_ACTIONS), (dict(batch=0, target_period=0), BATCH)],
    "c51": [(dict(n_atoms=1), "n_atoms must be at least 2"), (dict(n_atoms=342), "n_actions * n_atoms = 1026 exceeds 1024"),
            (dict(v_min=10.0, v_max=10.0), SUPPORT_MSG), (dict(v_min=-INF), SUPPORT_MSG), (dict(v_max=NAN), SUPPORT_MSG),
            (dict(n_actions=1, n_atoms=1024, h1=1024), "C51 network too wide for one workgroup's LDS"),
            # two faults: the head's own checks come between n_actions and the shape
            (dict(n_atoms=1, n_obs=0), "n_atoms must be at least 2"), (dict(n_actions=0, n_atoms=1), N_ACTIONS), (dict(v_max=-20.0, batch=0), SUPPORT_MSG)],
}
CREATE_CASES = [(head, odd, msg) for head in HEADS for odd, msg in SHARED_CREATE + HEAD_CREATE[head]]


class _Head:
    """One head's entries on the loaded library, a lone learner and a population of two at SHAPE."""

    def __init__(self, kind, ctx):
        capi = _capi()
        self.kind, self.capi, self.lib, self.ctx, self.d = kind, capi, capi.load(), ctx, HEADS[kind]
        self.Cfg = {"dqn": capi.DQNCfg, "c51": capi.C51Cfg}[kind]
        self.learner, self.population = C.c_void_p(), C.c_void_p()
        assert self.lone("create")(ctx._h, C.byref(self.cfg()), C.byref(self.learner)) == 0, self.last()
        cfgs = (self.Cfg * 2)(self.cfg(seed=1), self.cfg(seed=2, gamma=0.9))
        assert self.pop("create")(ctx._h, cfgs, 2, C.byref(self.population)) == 0, self.last()

    def close(self):
        self.pop("destroy")(self.population)
        self.lone("destroy")(self.learner)

    def cfg(self, **odd):
        return self.Cfg(**dict(dict(SHAPE, **self.d["extra"]), **odd))

    def lone(self, tail):
        return getattr(self.lib, self.d["lone"] + tail)

    def pop(self, tail):
        return getattr(self.lib, self.d["pop"] + tail)

    def last(self):
        return self.lib.stmpc_last_error().decode()

    def refused(self, rc, msg):
        assert rc == self.capi.STMPC_EINVAL and self.last() == msg, (rc, self.last(), msg)


@pytest.fixture(scope="module")
def heads(gpu_ctx):
    made = {kind: _Head(kind, gpu_ctx) for kind in HEADS}
    yield made
    for h in made.values():
        h.close()


@pytest.mark.parametrize("kind,odd,msg", CREATE_CASES)
def test_create_refuses_with_the_first_fault(heads, kind, odd, msg):
    h = heads[kind]
    out = C.c_void_p(1)
    h.refused(h.lone("create")(h.ctx._h, C.byref(h.cfg(**odd)), C.byref(out)), msg % h.d["name"] if "%s" in msg else msg)
    assert not out.value                                            # (create clears it before the first check)


@pytest.mark.parametrize("kind", list(HEADS))
def test_push_and_act_refuse_before_any_launch(heads, kind):
    h = heads[kind]
    t, push, act = h.learner, h.lone("push_device"), h.lone("act_device")
    big = "N exceeds the replay capacity, or obs_stride is shorter than the observation"
    h.refused(push(None, 1, *[None] * 3, 4, *[None] * 5), "learner is NULL")
    h.refused(push(t, 65, *[None] * 3, 4, *[None] * 5), big)
    h.refused(push(t, -1, *[None] * 3, 4, *[None] * 5), big)
    h.refused(push(t, 8, *[None] * 3, 3, *[None] * 5), big)
    assert push(t, 0, *[None] * 3, 4, *[None] * 5) == 0             # nothing to push: the return comes before the pointers are looked at
    h.refused(push(t, 8, *[None] * 3, 4, *[None] * 5), "NULL device pointer")
    short = "N negative, or obs_stride shorter than the observation"
    h.refused(act(None, 1, None, 4, 0.0, None, None, None), "learner is NULL")
    h.refused(act(t, -1, None, 4, 0.0, None, None, None), short)
    h.refused(act(t, 8, None, 3, 0.0, None, None, None), short)
    for eps in (-0.1, 1.5, NAN):
        h.refused(act(t, 8, None, 4, eps, None, None, None), "eps must be in 0 ... 1")
    h.refused(act(t, 0, None, 4, 2.0, None, None, None), "eps must be in 0 ... 1")      # eps is checked even when there is nothing to act on
    assert act(t, 0, None, 4, 0.5, None, None, None) == 0
    h.refused(act(t, 8, None, 4, 0.5, None, None, None), "NULL device pointer")
    # the counters say that nothing ran: no row pushed, no exploring call counted
    cn, bp = (C.c_int64 * 8)(), (C.c_float * 2)()
    assert h.lone("get_state")(t, cn, bp) == 0 and list(cn) == [0] * 8


@pytest.mark.parametrize("kind", list(HEADS))
def test_parameter_entries_refuse_a_wrong_slot_and_a_wrong_count(heads, kind):
    h = heads[kind]
    t, n_out = h.learner, 3 * (5 if kind == "c51" else 1)
    count = (4 + 1) * 16 + (16 + 1) * n_out
    buf = (C.c_float * (count + 1))()
    slot, length = "NULL argument or slot out of range", "count is not the length of this slot"
    for entry in (h.lone("set_params"), h.lone("get_params")):
        h.refused(entry(None, 0, buf, count), slot)
        h.refused(entry(t, 0, None, count), slot)
        h.refused(entry(t, 4, buf, count), slot)
        h.refused(entry(t, -1, buf, count), slot)
        h.refused(entry(t, 0, buf, count + 1), length)
        h.refused(entry(t, 3, buf, count - 1), length)
    assert h.lone("get_params")(t, 0, buf, count) == 0
    padded = 33 * 16 + (16 + 1) * 16                                # h1p = 16, Ap = 16 for both heads' widths (3 and 15)
    big = (C.c_float * (padded + 1))()
    h.refused(h.lone("padded_read")(t, 5, big, padded), slot)
    h.refused(h.lone("padded_read")(t, -1, big, padded), slot)
    h.refused(h.lone("padded_read")(None, 0, big, padded), slot)
    h.refused(h.lone("padded_read")(t, 4, big, padded + 1), "count is not the length of a padded slot")
    assert h.lone("padded_read")(t, 4, big, padded) == 0


@pytest.mark.parametrize("kind", list(HEADS))
def test_a_borrowed_member_names_the_populations_entry(heads, kind):
    h = heads[kind]
    member = C.c_void_p(h.pop("member")(h.population, 1))
    assert member.value and h.pop("size")(h.population) == 2
    per = h.capi.PERCfg(alpha=0.5, beta=0.4, min_priority=1e-6, max_priority=4.0)
    h.refused(h.lone("per_enable")(member, C.byref(per)),
              "this learner is a member of a population: prioritised replay is enabled on the population (%s)" % h.d["per_on_pop"])
    bad = h.capi.PERCfg(alpha=0.5, beta=0.4, min_priority=0.0, max_priority=4.0)
    h.refused(h.lone("per_enable")(member, C.byref(bad)),              # the cfg is looked at first, on a member too
              "prioritised replay needs min_priority > 0, max_priority >= min_priority, alpha >= 0 and beta >= 0, all finite")
    nstep = h.capi.NStepCfg(n_step=3, rows_per_push=8)
    h.refused(getattr(h.lib, h.d["nstep"])(member, C.byref(nstep)), "this learner is a member of a population: n_step is set on the population (%s)" % h.d["nstep_on_pop"])
    h.refused(h.pop("member")(h.population, 2) or h.capi.STMPC_EINVAL, "population is NULL, or no such member")


@pytest.mark.parametrize("kind", list(HEADS))
def test_population_entries_refuse_tables_of_the_wrong_length(heads, kind):
    h = heads[kind]
    p, dbl = h.population, lambda *v: (C.c_double * len(v))(*v)
    act, update = h.pop("act_device"), h.pop("update_device")
    rows = "n_per_member must be in 1 ... capacity, and obs_stride at least the observation's width"
    h.refused(act(None, 8, None, 4, dbl(0.1, 0.1), 2, None, None, None), "population is NULL")
    h.refused(act(p, 0, None, 4, dbl(0.1, 0.1), 2, None, None, None), rows)
    h.refused(act(p, 65, None, 4, dbl(0.1, 0.1), 2, None, None, None), rows)
    h.refused(act(p, 8, None, 3, dbl(0.1, 0.1), 2, None, None, None), rows)
    h.refused(act(p, 8, None, 4, None, 2, None, None, None), "NULL argument")
    h.refused(act(p, 8, None, 4, dbl(0.1), 1, None, None, None), "the eps array has 1 entries, the population 2 members")
    h.refused(act(p, 8, None, 4, dbl(0.1, 0.1, 0.1), 3, None, None, None), "the eps array has 3 entries, the population 2 members")
    h.refused(act(p, 8, None, 4, dbl(0.5, 1.5), 2, None, None, None), "member 1's eps must be in 0 ... 1")
    h.refused(act(p, 8, None, 4, dbl(NAN, 1.5), 2, None, None, None), "member 0's eps must be in 0 ... 1")
    h.refused(act(p, 8, None, 4, dbl(0.5, 0.0), 2, None, None, None), "NULL device pointer")
    push = h.pop("push_device")
    h.refused(push(None, 8, *[None] * 3, 4, *[None] * 5), "population is NULL")
    h.refused(push(p, 65, *[None] * 3, 4, *[None] * 5), rows)
    h.refused(push(p, 8, *[None] * 3, 4, *[None] * 5), "NULL device pointer")
    h.refused(update(None, 1, dbl(1e-3, 1e-3), 2, None), "NULL argument")
    h.refused(update(p, 1, None, 2, None), "NULL argument")
    h.refused(update(p, 1, dbl(1e-3), 1, None), "the learning-rate arrays have 1 entries, the population 2 members")
    h.refused(update(p, 1, dbl(1e-3, 1e-3, 1e-3), 3, None), "the learning-rate arrays have 3 entries, the population 2 members")
    h.refused(update(p, -1, dbl(1e-3, 1e-3), 2, None), "n_updates is negative")
    h.refused(update(p, 1, dbl(1e-3, -1e-3), 2, None), "a member's learning rate is negative")
    h.refused(h.pop("stats_device")(p, None, None), "NULL argument")
    per = (h.capi.PERCfg * 2)()
    h.refused(h.pop("per_enable")(p, per, (C.c_uint8 * 3)(), 3), "cfgs and enabled have 3 entries, the population 2 members")
    h.refused(getattr(h.lib, h.d["nstep_on_pop"])(p, (h.capi.NStepCfg * 1)(), 1), "cfgs has 1 entries, the population 2 members")


@pytest.mark.parametrize("kind", list(HEADS))
def test_population_create_hands_back_an_invalid_members_error(heads, kind):
    h = heads[kind]
    out = C.c_void_p(1)
    # the members agree in what a population shares, so the population's own checks pass; member 1's create then refuses its cfg, and the
    # population made so far -- member 0 with it -- is destroyed
    cfgs = (h.Cfg * 2)(h.cfg(seed=1), h.cfg(seed=2, target_period=0))
    h.refused(h.pop("create")(h.ctx._h, cfgs, 2, C.byref(out)), PERIOD)
    assert not out.value
    cfgs = (h.Cfg * 3)(h.cfg(), h.cfg(), h.cfg(gamma=-1.0))
    h.refused(h.pop("create")(h.ctx._h, cfgs, 3, C.byref(out)), CONSTANTS % h.d["name"])
    assert not out.value
    shared = "n_obs, h1, n_actions, %sbatch and capacity" % ("n_atoms, " if kind == "c51" else "")
    cfgs = (h.Cfg * 2)(h.cfg(), h.cfg(batch=9))
    h.refused(h.pop("create")(h.ctx._h, cfgs, 2, C.byref(out)), "the members of a population share %s (member 1 differs from member 0)" % shared)
