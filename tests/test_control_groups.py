"""Controller groups on the GPU (csrc/stmpc_cc_groups_kernels.hpp; stmpc_combined_groups_* / stmpc_rollout_step_groups_device /
stmpc_combined_decide_groups_device of include/stmpc.h; combined.ControlGroups, the ``control`` argument of episodes.EpisodeRunner).

The contract: group g of a grouped batch is, bit for bit, the lone batch of n_per_group states under cfgs[g] -- decisions, commands, the rolled-out
states, the rollout bookkeeping and the policy's evaluation counters.  Every comparison here is ``np.array_equal`` on the raw bits, against LONE
``decide_batch_device`` calls through the plain entries, each in a context of its own.  The shape is the smallest that can go wrong: the shipped
21-400-300-1 actor ``medium1``, Kmax = 16, 24 states per group (no multiple of the 64-lane workgroup nor of the actor's 16-row tile: every group has
masked lanes, and a workgroup that spanned groups would mix cfgs from row 24 on).  No tolerance anywhere.

The states are 24 of golden_combined_real.npz.  Its first 24 are all plain rollouts the policy keeps (5 evaluations, reason 0), so the rows are
chosen by what the reference recorded for them: IDX[0:5] rollouts that end after ONE step (a crash predicted at step 1), IDX[5:10] states whose
rolled-out state the feasibility probe rejects, IDX[10:14] crashes predicted at steps 2-4, IDX[14:24] the fixture's first ten.

What is compared of the bookkeeping is what a rollout writes: rollout_s up to hist_len (at most the group's own R + 1 columns of the Rmax + 1),
test_ego4 / test_ox / test_ov where have_test is set and a vehicle exists.  The rest of those arrays is memory no kernel wrote, in either run.
"""
import numpy as np
import pytest

from conftest import load_golden
from stmpc_testlib import apply_settings as _apply_settings, bits as _bits, same as _same

NPG, KMAX = 24, 16
IDX = [90, 128, 131, 165, 241, 101, 108, 144, 187, 202, 123, 167, 291, 297, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
GROUPS = [
    {"ROLLOUT_LENGTH": 3, "ST_TEST_ROLLOUTS": 2, "TEST_ROLLOUT_STATE": True},
    {"ROLLOUT_LENGTH": 5, "ST_TEST_ROLLOUTS": 5, "TEST_ROLLOUT_STATE": True},
    {"ROLLOUT_LENGTH": 10, "ST_TEST_ROLLOUTS": 2, "TEST_ROLLOUT_STATE": False},
    {"ROLLOUT_LENGTH": 1, "ST_TEST_ROLLOUTS": 2, "TEST_ROLLOUT_STATE": True},       # the probe state falls back to the last rolled-out state
    {"ROLLOUT_LENGTH": 5, "ST_TEST_ROLLOUTS": 2, "TEST_ROLLOUT_STATE": True, "TEST_ST_STRICTLY_BETTER": True, "REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED": True},
]
LAST_RL = (np.arange(NPG) % 3 != 0).astype(np.int32)          # mixed: the remember-last branch is taken for every third row
DECISION = ("takeover", "reason", "speed", "first_action", "cur_ego4", "cur_ox", "cur_ov", "cur_oa", "evals")
ROLLOUT = ("live", "hist_len", "crash_pred", "sel_speed", "rollout_s", "have_test", "test_ego4", "test_ox", "test_ov", "probe_crash")
CONTROLLER = ("st_speed", "fine", "fine_len")
_cache, _ctxs = {}, {}


def _pkg():
    g = load_golden("golden_combined_real.npz")
    pkg = _apply_settings(g)
    if pkg.build.needs_build():
        pkg.build.build()
    return g, pkg


def _lone_ctx(i):
    """A context of its own for the lone run of group i (kept for the session: later tests reuse it, whatever it holds)."""
    from rl_mpc_lanemerging_amd import _capi
    if i not in _ctxs:
        _ctxs[i] = _capi.Context(-1)
    return _ctxs[i]


def _run(ctx, control, grouped, sparse=False, ticks=1):
    """``ticks`` consecutive decisions of the 24 states (once per group) under ``control``: through the grouped entries, or -- one group only --
    through the plain ones.  Returns one dict of host arrays per tick."""
    import torch
    from rl_mpc_lanemerging_amd import _capi, actor, combined
    g, pkg = _pkg()
    S = pkg.Settings
    dev = torch.device("cuda", torch.cuda.current_device())
    cfgs = combined.control_cfgs(control, sparse_control=sparse)
    C = len(cfgs)
    assert grouped or C == 1
    cfg = combined.ControlGroups(cfgs, NPG) if grouped else cfgs[0]
    n = C * NPG
    pad = lambda a: np.concatenate([a[IDX], np.zeros((NPG, KMAX - a.shape[1]))], axis=1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(np.concatenate([a] * C, axis=0)), device=dev)
    d_ego, d_k, d_ox, d_ov, d_oa = t(g["ego"][IDX]), t(g["k_count"][IDX]), t(pad(g["other_x"])), t(pad(g["other_v"])), t(pad(g["other_a"]))
    d_last = t(LAST_RL)
    params = _capi.Params.from_settings(S)
    pol = actor.DDPGActor(str(g["actor"]), n, ctx, S, dev)
    pol.evals.copy_(t(g["evals0"][IDX]))
    R = max(max(int(c.rollout_length), 1) for c in cfgs)
    k = np.concatenate([g["k_count"][IDX]] * C)
    outs = []
    for _ in range(ticks):
        d = combined.decide_batch_device(ctx, params, cfg, d_ego, d_k, d_ox, d_ov, pol, d_last, torch.cuda.current_stream().cuda_stream, d_oa=d_oa)
        torch.cuda.synchronize()
        ctx.check_error()
        out = {q: d[q].cpu().numpy() for q in DECISION if q != "evals"}
        out["evals"] = pol.evals.cpu().numpy()
        out.update(ctx.combined_read_state(n, KMAX, R))
        # what no kernel wrote is not compared
        col = np.arange(R + 1)[None, :]
        out["rollout_s"] = np.where(col < out["hist_len"][:, None], out["rollout_s"], 0.0)
        have = out["have_test"].astype(bool)
        out["test_ego4"] = np.where(have[:, None], out["test_ego4"], 0.0)
        veh = have[:, None] & (np.arange(KMAX)[None, :] < k[:, None])
        out["test_ox"], out["test_ov"] = np.where(veh, out["test_ox"], 0.0), np.where(veh, out["test_ov"], 0.0)
        outs.append(out)
    return outs


def _lone(i, control, sparse=False, ticks=1):
    key = ("lone", i, repr(control), sparse, ticks)
    if key not in _cache:
        _cache[key] = _run(_lone_ctx(i), [control], grouped=False, sparse=sparse, ticks=ticks)
    return _cache[key]


def _assert_group(got, g, lone, label, keys=DECISION + ROLLOUT + CONTROLLER):
    sl = slice(g * NPG, (g + 1) * NPG)
    for q in keys:
        a, b = got[q][sl], lone[q]
        if q == "rollout_s":                                         # the group's own R + 1 columns of the run's Rmax + 1; nothing beyond them
            assert not a[:, b.shape[1]:].any(), (label, "group %d" % g, "rollout_s beyond the group's length")
            a = a[:, :b.shape[1]]
        assert _same(a, b), (label, "group %d" % g, q)


# ---- 1. decide level ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_every_group_decides_as_its_lone_batch(gpu_ctx, restore_settings):
    got = _run(gpu_ctx, GROUPS, grouped=True)[0]
    lones = [_lone(i, c)[0] for i, c in enumerate(GROUPS)]
    # the lone results make the comparison mean something
    for i in (0, 3):
        assert lones[i]["live"].any(), "group %d: no row is still live after its last step" % i
    assert any((lones[i]["reason"] != lones[j]["reason"]).any() for i in range(5) for j in range(i)), "no row's reason differs between two groups"
    assert any((l["have_test"] == 0).any() for l in lones) and (lones[0]["have_test"] == 0).any() and not lones[3]["have_test"].any()
    assert (lones[0]["hist_len"] == 2).any(), "no rollout ended after one step"
    assert [l["rollout_s"].shape[1] for l in lones] == [4, 6, 11, 2, 6] and got["rollout_s"].shape[1] == 11
    print("reasons per group:", [np.bincount(l["reason"], minlength=5).tolist() for l in lones])
    for i in range(5):
        _assert_group(got, i, lones[i], "decide")
    # live keeps its meaning: rows of the short groups are still live, and were not asked again
    assert got["live"][:NPG].any() and got["live"][3 * NPG:4 * NPG].any()


# ---- 2. two consecutive ticks: the ask mask ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_evaluation_counters_over_two_ticks(gpu_ctx, restore_settings):
    """A row of a short group that is live after its last step must not be asked again: its time feature would be one evaluation ahead in every
    later tick.  The second decision is fed by the first's counters."""
    got = _run(gpu_ctx, GROUPS, grouped=True, ticks=2)
    g, _ = _pkg()
    for i, c in enumerate(GROUPS):
        lone = _lone(i, c, ticks=2)
        sl = slice(i * NPG, (i + 1) * NPG)
        for t in range(2):
            assert _same(got[t]["evals"][sl], lone[t]["evals"]), (i, t)
        _assert_group(got[1], i, lone[1], "second tick")
        # every state is asked once, none more often than its group's R in a tick
        for per_tick in (lone[1]["evals"] - lone[0]["evals"], lone[0]["evals"] - g["evals0"][IDX]):
            assert per_tick.min() >= 1 and per_tick.max() <= c["ROLLOUT_LENGTH"], (i, per_tick)
    assert (got[0]["evals"][:NPG] < got[0]["evals"][2 * NPG:3 * NPG]).any()                   # (the groups do count differently)


# ---- 3. sparse against dense ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_sparse_and_dense_controller_solves_agree(gpu_ctx, restore_settings):
    gpu_ctx.combined_counts(reset=True)
    dense = _run(gpu_ctx, GROUPS[:4], grouped=True, sparse=False)[0]
    assert gpu_ctx.combined_counts(reset=True) == (4 * NPG, 4 * NPG)
    sparse = _run(gpu_ctx, GROUPS[:4], grouped=True, sparse=True)[0]
    decisions, solves = gpu_ctx.combined_counts(reset=True)
    assert decisions == 4 * NPG and 0 < solves < decisions
    for q in DECISION + ROLLOUT:
        assert _same(sparse[q], dense[q]), q
    assert np.isnan(sparse["st_speed"]).sum() == decisions - solves and not np.isnan(dense["st_speed"]).any()
    for i in range(4):
        _assert_group(sparse, i, _lone(i, GROUPS[i], sparse=True)[0], "sparse")
    # one strictly-better group makes the whole run dense, and still every group's
    both = _run(gpu_ctx, GROUPS, grouped=True, sparse=True)[0]
    assert gpu_ctx.combined_counts(reset=True) == (5 * NPG, 5 * NPG)
    for i in range(5):
        _assert_group(both, i, _lone(i, GROUPS[i], sparse=True)[0], "sparse, dense through group 4", keys=DECISION + ROLLOUT)
    _assert_group(both, 4, _lone(4, GROUPS[4], sparse=True)[0], "group 4")


# ---- 4. C = 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,sparse", [(0, False), (0, True), (4, False)])
def test_gpu_one_group_is_the_plain_entries(gpu_ctx, restore_settings, which, sparse):
    plain = _run(gpu_ctx, [GROUPS[which]], grouped=False, sparse=sparse, ticks=2)
    one = _run(gpu_ctx, [GROUPS[which]], grouped=True, sparse=sparse, ticks=2)
    for t in range(2):
        _assert_group(one[t], 0, plain[t], "C = 1, tick %d" % t)


# ---- 5. independence between groups -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_groups_are_independent(gpu_ctx, restore_settings):
    a = _run(gpu_ctx, GROUPS[:3], grouped=True)[0]
    other = {"ROLLOUT_LENGTH": 12, "ST_TEST_ROLLOUTS": 3, "TEST_ROLLOUT_STATE": True, "LIMIT_DQN_SPEED": True, "CHECK_ROLLOUT_CRASH": False}
    b = _run(gpu_ctx, [GROUPS[0], other, GROUPS[2]], grouped=True)[0]          # (Rmax, and with it the stride of rollout_s, changes too)
    assert a["rollout_s"].shape[1] == 11 and b["rollout_s"].shape[1] == 13
    for g in (0, 2):
        sl = slice(g * NPG, (g + 1) * NPG)
        for q in DECISION + ROLLOUT + CONTROLLER:
            x, y = a[q][sl], b[q][sl]
            if q == "rollout_s":
                assert not y[:, 11:].any()
                y = y[:, :11]
            assert _same(x, y), (g, q)
    assert not _same(a["reason"][NPG:2 * NPG], b["reason"][NPG:2 * NPG]) or not _same(a["evals"][NPG:2 * NPG], b["evals"][NPG:2 * NPG])


# ---- 6. runner --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_runner_cells_equal_lone_runners(gpu_ctx, restore_settings):
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import actor, combined_bench, episodes, report
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    S = pkg.Settings
    TICKS, C = 40, 3
    cells = GROUPS[:3]
    tr = dict(episodes.TRAFFIC_TYPES["medium"], seed=41)                       # the same traffic draws in every cell
    rec = lambda: report.RecorderConfig(depth=8)
    pop = actor.ActorPopulation(["medium1"] * C, NPG, gpu_ctx, S)
    got = episodes.run_episodes(C * NPG, controller="combined", policy=pop, ctx=gpu_ctx, kmax=KMAX, max_ticks=TICKS, record=rec(), traffic=[tr] * C, control=cells)
    gpu_ctx.check_error()
    assert np.array_equal(got["control_group"], np.arange(C * NPG) // NPG) and got["ticks"].max() == TICKS
    lones = []
    for c in range(C):
        lone = episodes.run_episodes(NPG, controller="combined", policy=actor.ActorPopulation(["medium1"], NPG, gpu_ctx, S), ctx=gpu_ctx, kmax=KMAX,
                                     max_ticks=TICKS, record=rec(), traffic=[tr], control=[cells[c]])
        gpu_ctx.check_error()
        lones.append(lone)
        sl = slice(c * NPG, (c + 1) * NPG)
        cols = [k for k in lone if k not in ("report", "control_group", "traffic_group", "member")]
        assert "ego4" in cols and "percent_st" in cols
        for k in cols:
            assert _same(got[k][sl], lone[k]), (c, k)
        a, b = got["report"]._rec, lone["report"]._rec
        for k in ("ring", "length", "status"):
            assert _same(a[k][sl], b[k]), (c, k)
        assert _same(np.ascontiguousarray(a["acc_env"][:, sl]), b["acc_env"]), (c, "acc_env")
    by = episodes.summary_by_control(got, C)
    for c in range(C):
        want = episodes.summary(lones[c])
        for k, v in want.items():
            assert _same(np.float64(by[c][k]), np.float64(v)), (c, k)
    # the cells were told apart: same traffic draws, so any difference is the controller's
    cols = [k for k in lones[0] if k not in ("report", "control_group", "traffic_group", "member")]
    assert any(not _same(lones[i][k], lones[j][k]) for i in range(C) for j in range(i) for k in cols)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refusals_change_nothing(restore_settings):
    import torch
    from rl_mpc_lanemerging_amd import _capi, combined
    g, pkg = _pkg()
    S = pkg.Settings
    ctx = _lone_ctx("refusals")
    ctx.combined_groups_clear()
    params = _capi.Params.from_settings(S)
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 2 * NPG
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    ego5, k, ox, ov, oa, act = z(n, 5), z(n, dtype=torch.int32), z(n, KMAX), z(n, KMAX), z(n, KMAX), z(n)
    ego4, take, reason, speed = z(n, 4), z(n, dtype=torch.int32), z(n, dtype=torch.int32), z(n)
    step = lambda N, s, K=KMAX: ctx.rollout_step_groups_device(params, N, K, s, ego5.data_ptr(), ego4.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(),
                                                               oa.data_ptr(), act.data_ptr())
    decide = lambda N: ctx.combined_decide_groups_device(params, N, KMAX, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), ego4.data_ptr(), ox.data_ptr(),
                                                         ov.data_ptr(), act.data_ptr(), 0, take.data_ptr(), reason.data_ptr(), speed.data_ptr())

    def refused(call, match):
        with pytest.raises(_capi.StmpcError, match=match) as e:
            call()
        assert e.value.code == _capi.STMPC_EINVAL

    two = combined.control_cfgs(GROUPS[:2])
    before = _run(ctx, GROUPS[:2], grouped=True)[0]            # a valid grouped decision; sets the table
    ctx.combined_groups_clear()
    # no table set
    refused(lambda: step(n, 1), "no controller groups")
    refused(lambda: decide(n), "no controller groups")
    # tables that are refused leave the context without one
    for field, val in (("tick_length", 0.1), ("stop_x", 1.0), ("sparse_control", 1)):
        bad = combined.control_cfgs(GROUPS[:2])
        setattr(bad[1], field, val)
        refused(lambda: ctx.combined_groups_set(params, bad, NPG), "must share %s .*group 1" % field)
    bad = combined.control_cfgs(GROUPS[:2])
    bad[1].rollout_length = _capi_rollout_limit() + 1
    refused(lambda: ctx.combined_groups_set(params, bad, NPG), "STMPC_ROLLOUT_LIMIT")
    refused(lambda: ctx.combined_groups_set(params, two * 33, NPG), "1 ... STMPC_SIM_GROUPS_MAX")
    refused(lambda: ctx.combined_groups_set(params, [], NPG), "1 ... STMPC_SIM_GROUPS_MAX")
    refused(lambda: ctx.combined_groups_set(params, two, 0), "n_per_group must be positive")
    refused(lambda: step(n, 1), "no controller groups")
    ctx.combined_groups_set(params, two, NPG)
    # a refused table leaves the one that is set
    refused(lambda: ctx.combined_groups_set(params, bad, NPG), "STMPC_ROLLOUT_LIMIT")
    # N that is not C * n_per_group
    refused(lambda: step(n + 1, 1), "C \\* n_per_group")
    refused(lambda: step(NPG, 1), "C \\* n_per_group")
    refused(lambda: decide(NPG), "C \\* n_per_group")
    # step > 1 / decide without a grouped rollout of this shape
    refused(lambda: step(n, 2), "does not continue the grouped rollout")
    refused(lambda: decide(n), "no grouped rollout of this shape")
    plain = two[0]
    ctx.rollout_step_device(params, plain, n, KMAX, 1, ego5.data_ptr(), ego4.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr(), act.data_ptr())
    refused(lambda: step(n, 2), "does not continue the grouped rollout")
    refused(lambda: decide(n), "no grouped rollout of this shape")               # a grouped decide after a plain rollout
    step(n, 1)
    refused(lambda: step(n, 2, K=8), "does not continue the grouped rollout")     # another Kmax
    refused(lambda: ctx.rollout_step_device(params, plain, n, KMAX, 2, ego5.data_ptr(), ego4.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), oa.data_ptr(),
                                            act.data_ptr()), "does not continue the rollout")
    refused(lambda: ctx.combined_decide_device(params, plain, n, KMAX, ego5.data_ptr(), k.data_ptr(), ox.data_ptr(), ov.data_ptr(), ego4.data_ptr(), ox.data_ptr(),
                                               ov.data_ptr(), act.data_ptr(), 0, take.data_ptr(), reason.data_ptr(), speed.data_ptr()),
            "no rollout of this shape")                                           # a plain decide after a grouped rollout
    torch.cuda.synchronize()
    ctx.check_error()
    # nothing was launched by a refused call: the outputs of the refused decides are untouched ...
    assert not take.any() and not reason.any() and not speed.any()
    # ... and a following valid call gives what it gave before
    after = _run(ctx, GROUPS[:2], grouped=True)[0]
    for q in DECISION + ROLLOUT + CONTROLLER:
        assert _same(after[q], before[q]), q


def _capi_rollout_limit():
    import os
    import re
    from conftest import REPO
    return int(re.search(r"#define STMPC_ROLLOUT_LIMIT (\d+)", open(os.path.join(REPO, "include", "stmpc.h")).read()).group(1))
