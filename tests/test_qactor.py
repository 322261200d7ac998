"""The DQN policy on the GPU (``actor.DQNActor``, ``k_qactor_eval`` of csrc/stmpc_qactor_kernels.hpp): the fused launch against the public entries it
replaces -- ``stmpc_policy_features_device`` (no time feature), ``DQNLearner.act`` (eps = 0), the action table -- bit for bit, and against
``actor.q_policy_host`` value for value on dyadic data.  Networks (n_obs, h1, A) = (20, 16, 5), (20, 48, 20), (20, 256, 5); row counts 1, 16, 17,
33 (a lone row, a full tile, a tile plus one row, two tiles plus one); states of ``golden_combined_real.npz`` with 16 vehicle slots.  No tolerance
anywhere: the kernel runs the learner's own forward pass and argmax.

Not covered: the refusal of a context on another device than the policy's (the check is ``stmpc_actor_eval_device``'s; one device here)."""
import ctypes
import types

import numpy as np
import pytest

from discrete_testlib import (JERKS, NAMES, NETS, NETS_WIDE, Q_WIDE_VARIANTS, ROWS, SENTINEL, q_dyadic_policy as _dyadic_policy, tied_rows as _tied_rows, act_on_features as _act, actor_table as _table, dev as _dev, episode_settings as _episode_settings,
                              plain_policy as _plain_policy, policy_features as _features, policy_states as _states, run_policy as _run, stream as _stream,
                              transitions as _transitions, widen as _widen)
from stmpc_testlib import ACTOR_KMAX, capi as _capi, same


def _trained(gpu_ctx, shape, seed=5, table=None, target_period=4, updates=1):
    """A learner whose online and target networks differ: 32 random transitions, then ``updates`` updates (< target_period: no hard copy)."""
    from rl_mpc_lanemerging_amd import learner
    n_obs, h1, A = shape
    cfg = learner.DQNConfig(n_obs=n_obs, n_actions=A, h1=h1, batch=16, capacity=64, target_period=target_period, lr=1e-2)
    L = learner.DQNLearner((n_obs, A), cfg, seed=seed, ctx=gpu_ctx)
    L.action_values = _table(A) if table is None else np.asarray(table, dtype=np.float64)
    L.push(*_transitions(np.random.default_rng(seed), 32, n_obs, A))
    if updates:
        L.update(updates)
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("shape", NETS)
def test_gpu_fused_launch_equals_features_act_and_table(shape, n, gpu_ctx, restore_settings, tmp_path):
    """A view of the online network, a view of the target network and a file actor of the exported online network: .feat is
    stmpc_policy_features_device's output, .action and .q are learner.act's on those rows (the target's: of a second learner loaded with the
    target slot), jerk = action_values[action]; the rows beyond n keep their sentinel."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor, learner
    S, st = _states(n)
    L = _trained(gpu_ctx, shape)
    params = L.state_dict()["params"]
    assert params["updates"] == 1 and not np.array_equal(params["q"]["w1"], params["q_target"]["w1"])
    L_target = learner.DQNLearner((shape[0], shape[2]), L.cfg, seed=1, init=params["q_target"], ctx=gpu_ctx)
    path = L.export_q(str(tmp_path / "q.npz"))
    table = L.action_values
    fcfg = capi.FeaturesCfg.from_settings(S, time_feature=False)
    feat = _features(gpu_ctx, fcfg, st, n, shape[0])
    want_feat = feat.cpu().numpy()
    assert not (want_feat == SENTINEL).any()
    for label, P, ref in (("online view", actor.DQNActor.from_learner(L, n, gpu_ctx, S), L), ("target view", actor.DQNActor.from_learner(L, n, gpu_ctx, S, target=True), L_target),
                          ("file", actor.DQNActor(path, n, gpu_ctx, S), L)):
        assert P.mode == "jerk" and P.shape == shape and np.array_equal(P.action_values, table), label
        got = _run(_widen(P), st)
        a, q = _act(ref, feat)
        assert same(got["feat"], want_feat), label
        assert same(got["q"], q), (label, int((got["q"] != q).sum()))
        assert same(got["action"], a) and a.min() >= 0 and a.max() < shape[2], label
        assert same(got["jerk"], table[a]), label
        P.reset()
        P.reset(torch.ones(n, dtype=torch.bool, device=_dev()))
    gpu_ctx.check_error()


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_gpu_acceleration_mode_equals_the_numpy_formula(n, gpu_ctx, restore_settings):
    """(20, 48, 20) behind an env of sumo-accel-v0: the default mode is "acceleration", and the jerk is clip((table[a] - ego acceleration) /
    TICK_LENGTH, MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK) of the same fp64 inputs, exactly.  The states' accelerations cycle through -20, 0 and
    +20 and the table stays within +-0.1, so whatever the actions are, rows are clipped at either edge and rows are not."""
    _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    S, st = _states(n)
    st["ego4"][:, 3] = st["ego4"].new_tensor([-20.0, 0.0, 20.0]).repeat(n // 3 + 1)[:n]
    n_obs, h1, A = NETS[1]
    table = np.linspace(-0.1, 0.1, A)
    env = types.SimpleNamespace(continuous=False, obs_dim=n_obs, action_space={"n": A}, cfg=types.SimpleNamespace(_actions=table), ctx=gpu_ctx, env_id="sumo-accel-v0")
    L = learner.DQNLearner(env, learner.DQNConfig(n_obs=n_obs, h1=h1, batch=16, capacity=64), seed=9)
    assert L.env_id == "sumo-accel-v0" and np.array_equal(L.action_values, table)
    assert learner.DQNLearner((n_obs, A), learner.DQNConfig(n_obs=n_obs, h1=h1, batch=16, capacity=64), ctx=gpu_ctx).env_id is None
    P = actor.DQNActor.from_learner(L, n, gpu_ctx, S)
    assert P.mode == "acceleration"
    got = _run(_widen(P), st)
    acc = st["ego4"][:, 3].cpu().numpy()
    raw = (table[got["action"]] - acc) / S.TICK_LENGTH
    want = np.clip(raw, S.MINIMUM_NEGATIVE_JERK, S.MAXIMUM_POSITIVE_JERK)
    assert same(got["jerk"], want)
    assert same(got["jerk"], actor.q_policy_host(L.state_dict()["params"]["q"], got["feat"], table, "acceleration", ego_acc=acc, S=S)[2])
    assert (got["jerk"] == S.MAXIMUM_POSITIVE_JERK).any()
    if n >= 3:
        assert (got["jerk"] == S.MINIMUM_NEGATIVE_JERK).any() and (np.abs(got["jerk"]) <= 0.5).any()
    # the same learner under "jerk": the table's entries themselves
    J = actor.DQNActor.from_learner(L, n, gpu_ctx, S, mode="jerk")
    gotj = _run(_widen(J), st)
    assert same(gotj["action"], got["action"]) and same(gotj["jerk"], table[got["action"]])
    gpu_ctx.check_error()


# ---- dyadic data: Q against the float64 twin, value for value ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", NETS + NETS_WIDE)
def test_gpu_dyadic_q_equals_the_float64_twin(shape, gpu_ctx, restore_settings, tmp_path):
    """.q equals q_policy_host in float64 value for value, .action its first-maximum index and .jerk the table's entry, for a view and for a file
    actor, on rows of which some have only negative Q (a pad column's 0 must not win) and some hold an exact tie (the first column wins).  The
    problems are discrete_testlib.q_dyadic_policy's.  Up to 32 actions: 33 rows, one tied pair.  Beyond (NETS_WIDE; a lane of the argmax owns
    several columns), 50 rows, an action table of A distinct values and two problems: "ties" -- (5, 37), (31, 32), (0, A - 1), at A = 256
    (9, 41, 233) each hold the maximum on rows, and there the index is the group's lowest column, group by group --, and "lone" -- columns 32 and
    A - 1 win rows alone, and the jerk there is the table's entry, or in acceleration mode the clipped difference quotient of the table's entry."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor, learner
    A, wide = shape[2], shape in NETS_WIDE
    for variant in Q_WIDE_VARIANTS if wide else (None,):
        net, S, states, feat, groups, named = _dyadic_policy(shape, variant)
        n = feat.shape[0]
        table = _table(A)
        q, idx, jerk = actor.q_policy_host(net, feat, table, "jerk")
        allneg = (q < 0).all(1)
        assert allneg.any() and not allneg.all() and len(set(table.tolist())) == A
        assert np.array_equal(q.astype(np.float32).astype(np.float64), q)
        for name, rows in _tied_rows(q, groups).items():
            print("%s %s: %s holds the maximum on %d rows, %d of them named" % (shape, variant, name, rows.size, named[name].size))
            assert named[name].size >= 1 and (idx[rows] <= groups[name][0]).all(), name
        if not wide:                                                # (the one pair: the rows it wins, not every row, and its first column on all of them)
            tie = _tied_rows(q, groups)["tie"]
            assert 0 < tie.size < n and (idx[tie] == groups["tie"][0]).all()
        L = learner.DQNLearner((shape[0], A), learner.DQNConfig(n_obs=shape[0], n_actions=A, h1=shape[1], batch=16, capacity=64), init=net, ctx=gpu_ctx)
        L.action_values = table
        st = {k: torch.as_tensor(np.ascontiguousarray(v), device=_dev()) for k, v in states.items()}
        path = L.export_q(str(tmp_path / ("q%s.npz" % (variant or ""))))
        for label, P in (("view", actor.DQNActor.from_learner(L, n, gpu_ctx, S)), ("file", actor.DQNActor(path, n, gpu_ctx, S))):
            got = _run(_widen(P), st)
            assert same(got["feat"], feat), label
            assert np.array_equal(got["q"].astype(np.float64), q), (label, int((got["q"].astype(np.float64) != q).sum()))
            for name, rows in named.items():
                assert (got["action"][rows] == groups[name][0]).all(), (label, variant, "index on the rows where %s holds the maximum" % name, got["action"][rows].tolist())
            assert np.array_equal(got["action"], idx) and same(got["jerk"], jerk), label
        if variant == "lone":
            small = np.linspace(-0.1, 0.1, A)
            L.action_values = small
            acc = states["ego4"][:, 3]
            want = actor.q_policy_host(net, feat, small, "acceleration", ego_acc=acc, S=S)
            got = _run(_widen(actor.DQNActor.from_learner(L, n, gpu_ctx, S, mode="acceleration")), st)
            assert np.array_equal(got["action"], want[1]) and same(got["jerk"], want[2])
            assert same(got["jerk"], np.clip((small[idx] - acc) / S.TICK_LENGTH, S.MINIMUM_NEGATIVE_JERK, S.MAXIMUM_POSITIVE_JERK))
            for c in (32, A - 1):
                assert (idx == c).any() and np.array_equal(got["action"] == c, idx == c)
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_view_is_live_and_leaves_the_learner_alone(gpu_ctx, restore_settings):
    """Evaluate, update(3), evaluate again on the same object: the second result is learner.act's of the updated network, and the learner's state
    (all four slots, Adam's beta powers, every counter -- the exploring-call counter among them) equals, bit for bit, that of a twin with the
    same pushes and updates and no evaluation."""
    _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor
    shape, n = NETS[2], 17
    S, st = _states(n)
    L, twin = (_trained(gpu_ctx, shape, seed=3, target_period=2, updates=0) for _ in range(2))
    obs = torch.zeros(8, shape[0], dtype=torch.float32, device=_dev())
    for x in (L, twin):
        x.act(obs, eps=1.0)                                         # one exploring call: the counter the evaluations must not advance
    P = _widen(actor.DQNActor.from_learner(L, n, gpu_ctx, S))
    first = _run(P, st)
    L.update(3)
    twin.update(3)
    second = _run(P, st)
    _run(_widen(actor.DQNActor.from_learner(L, n, gpu_ctx, S, target=True)), st)
    a, b = L.state_dict(), twin.state_dict()
    assert a["params"]["updates"] == 3 and a["counters"][3] == 1 and np.array_equal(a["counters"], b["counters"])
    assert same(a["params"]["beta_pow"], b["params"]["beta_pow"])
    for slot in _capi().DQN_SLOTS:
        for k in NAMES:
            assert same(a["params"][slot][k], b["params"][slot][k]), (slot, k)
    assert same(L.minibatch(), twin.minibatch())                    # (the workspace is not part of the state; the next update's rows are)
    act, q = _act(twin, P.feat[:n])
    assert same(second["q"], q) and same(second["action"], act) and same(second["jerk"], L.action_values[act])
    assert same(second["feat"], first["feat"]) and not np.array_equal(second["q"], first["q"])
    gpu_ctx.check_error()


@pytest.mark.gpu
def test_gpu_drop_in_for_the_combined_controller(gpu_ctx, restore_settings):
    """combined.decide_batch_device with a DQNActor returns what it returns with the plain callable, bit for bit."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor, combined
    n = 33
    S, st = _states(n)
    L = _trained(gpu_ctx, NETS[2])
    params, cfg = capi.Params.from_settings(S), capi.CombinedCfg.from_settings(S)
    assert cfg.rollout_length > 1
    out = []
    for policy in (actor.DQNActor.from_learner(L, n, gpu_ctx, S), _plain_policy(gpu_ctx, L, S, n)):
        d = combined.decide_batch_device(gpu_ctx, params, cfg, st["ego5"], st["k"], st["ox"], st["ov"], policy, None, _stream(), d_oa=st["oa"])
        torch.cuda.synchronize()
        gpu_ctx.check_error()
        out.append({k: v.cpu().numpy().copy() for k, v in d.items()})
    assert set(out[0]) == set(out[1]) and len(out[0]) == 8
    for k in out[0]:
        assert same(out[0][k], out[1][k]), k
    assert set(np.unique(out[0]["first_action"])) <= set(JERKS)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["combined", "first_step"])
def test_gpu_drop_in_for_the_episode_runner(controller, gpu_ctx, restore_settings):
    """EpisodeRunner(32, controller, policy) gives identical result() columns after 8 ticks with a DQNActor and with the plain callable."""
    _capi()
    from rl_mpc_lanemerging_amd import actor, episodes
    S = _episode_settings()
    n = 32
    L = _trained(gpu_ctx, NETS[2])
    res = []
    for policy in (actor.DQNActor.from_learner(L, n, gpu_ctx, S), _plain_policy(gpu_ctx, L, S, n)):
        r = episodes.EpisodeRunner(n, seed=4, controller=controller, policy=policy, ctx=gpu_ctx, kmax=ACTOR_KMAX)
        for _ in range(8):
            r.tick()
        res.append(r.result())
    assert set(res[0]) == set(res[1]) and "percent_st" in res[0]
    for k in res[0]:
        assert same(res[0][k], res[1][k]), k
    assert r.ticks_done == 8 and res[0]["ticks"].max() >= 1


@pytest.mark.gpu
def test_gpu_evaluate_dqn(gpu_ctx, restore_settings, tmp_path):
    """32 episodes of 2 s behind a freshly initialised learner (a view, a context of the evaluation's own), and behind its exported file under the
    first-step shield: run_episodes' columns."""
    _capi()
    from rl_mpc_lanemerging_amd import actor, learner
    _episode_settings()
    L = learner.DQNLearner((20, 5), learner.DQNConfig(batch=16, capacity=64), seed=2, ctx=gpu_ctx)
    L.action_values = JERKS.copy()
    keys = {"crashed", "merged", "timed_out", "mean_speed", "max_speed", "mean_abs_jerk", "closest_distance", "mean_closest_distance", "time_taken", "ticks",
            "status", "time_to_merge", "mean_disruption", "max_disruption", "total_disruption", "disruption_time", "ego4", "percent_st"}
    out = learner.evaluate_dqn(L, 32, seed=1, kmax=ACTOR_KMAX, max_episode_length=2.0)
    assert set(out) == keys and out["ticks"].shape == (32,) and out["ticks"].max() <= 10 and (out["status"] != 0).all()
    path = L.export_q(str(tmp_path / "q.npz"))
    out = learner.evaluate_dqn(path, 32, seed=1, kmax=ACTOR_KMAX, max_episode_length=2.0, controller="first_step")
    assert set(out) == keys and (out["status"] != 0).all()
    with pytest.raises(ValueError, match="built for 16"):
        learner.evaluate_dqn(actor.DQNActor.from_learner(L, 16, gpu_ctx, _episode_settings()), 32)


@pytest.mark.gpu
def test_gpu_library_refusals(gpu_ctx, restore_settings):
    """Every refusal of the stmpc_qactor_ entries is STMPC_EINVAL with a message, made before anything is launched: the outputs keep their sentinel."""
    capi = _capi()
    import torch
    from rl_mpc_lanemerging_amd import actor
    lib = capi.load()
    n = 17
    S, st = _states(n)
    L = _trained(gpu_ctx, NETS[0])
    table = L.action_values
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    h = ctypes.c_void_p()

    def refused(rc, word):
        msg = lib.stmpc_last_error().decode()
        assert rc == capi.STMPC_EINVAL and word in msg, (rc, word, msg)
        assert not h.value                                          # no handle came back

    net = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in L.state_dict()["params"]["q"].items()}
    create = lambda A=5, w0=fp(net["w0"]), tab=table, mode=0, n_in=20, ctx=gpu_ctx._h: lib.stmpc_qactor_create(
        ctx, n_in, 16, A, w0, fp(net["b0"]), fp(net["w1"]), fp(net["b1"]), dp(np.ascontiguousarray(tab, dtype=np.float64)), mode, ctypes.byref(h))
    refused(create(ctx=ctypes.c_void_p()), "NULL")
    refused(create(w0=ctypes.POINTER(ctypes.c_float)()), "NULL")
    refused(create(mode=2), "mode")
    refused(create(tab=[0.0, 1.0, float("nan"), 2.0, 3.0]), "finite")
    refused(create(A=0), "n_actions")
    refused(create(n_in=32), "shape")
    view = lambda learner=L.handle, target=0, tab=table, A=5, mode=0: lib.stmpc_qactor_view_dqn(learner, target, dp(np.ascontiguousarray(tab, dtype=np.float64)), A, mode,
                                                                                                 ctypes.byref(h))
    refused(view(learner=ctypes.c_void_p()), "NULL")
    refused(view(target=2), "target")
    refused(view(mode=-1), "mode")
    refused(view(tab=table[:4], A=4), "4 entries")
    refused(view(tab=[0.0, 1.0, float("inf"), 2.0, 3.0]), "finite")
    assert lib.stmpc_qactor_view_dqn(L.handle, 0, ctypes.POINTER(ctypes.c_double)(), 5, 0, ctypes.byref(h)) == capi.STMPC_EINVAL
    # set_limits, and the evaluation that needs them
    A = actor.DQNActor.from_learner(L, n, gpu_ctx, S, mode="acceleration")
    for bad in ((0.0, -1.0, 1.0), (0.2, 1.0, -1.0), (0.2, float("nan"), 1.0), (float("inf"), -1.0, 1.0)):
        assert lib.stmpc_qactor_set_limits(A.handle, *bad) == capi.STMPC_EINVAL and "finite" in lib.stmpc_last_error().decode()
    raw = gpu_ctx.qactor_view_dqn(L.handle, table, mode=capi.QACTOR_MODES["acceleration"])
    P = _widen(actor.DQNActor.from_learner(L, n, gpu_ctx, S))
    fcfg = P.fcfg
    args = lambda **kw: {**dict(handle=P.handle, fcfg=fcfg, N=n, Kmax=ACTOR_KMAX, step=1, d_cur_ego4=st["ego4"].data_ptr(), d_k=st["k"].data_ptr(),
                                d_cur_ox=st["ox"].data_ptr(), d_cur_ov=st["ov"].data_ptr(), d_cur_oa=st["oa"].data_ptr(), d_feat=P.feat.data_ptr(), feat_stride=P.flen,
                                d_action=P.action.data_ptr(), d_q=P.q.data_ptr(), d_jerk=P.jerk.data_ptr(), stream=_stream()), **kw}
    timed = capi.FeaturesCfg.from_settings(S, time_feature=True)
    wide = capi.FeaturesCfg.from_settings(S, time_feature=False)
    wide.cars_ahead += 1
    for kw, word in ((dict(handle=raw), "set_limits"), (dict(N=0), "positive"), (dict(N=-3), "positive"), (dict(fcfg=timed), "time feature"), (dict(fcfg=wide), "input width"),
                     (dict(feat_stride=P.flen - 1), "feat_stride"), (dict(d_jerk=0), "NULL"), (dict(d_cur_ego4=0), "NULL"), (dict(d_k=0), "NULL"), (dict(d_cur_ox=0), "NULL"),
                     (dict(handle=None), "NULL"), (dict(step=0), "step"), (dict(Kmax=33), "Kmax")):
        with pytest.raises(capi.StmpcError) as err:
            gpu_ctx.qactor_eval_device(**args(**kw))
        assert err.value.code == capi.STMPC_EINVAL and word in str(err.value), (kw, str(err.value))
    with pytest.raises(capi.StmpcError, match="rollout"):          # step 2 asks for the context's rollout, and a new context has none
        capi.Context(-1).qactor_eval_device(**args(step=2))
    assert lib.stmpc_qactor_eval_device(gpu_ctx._h, P.handle, None, n, ACTOR_KMAX, 1, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0, 0) == capi.STMPC_EINVAL
    torch.cuda.synchronize()
    for t in (P.feat, P.q, P.action, P.jerk):
        assert (t == SENTINEL).all()                                # nothing ran
    gpu_ctx.qactor_eval_device(**args())                            # ... and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert not (P.jerk[:n] == SENTINEL).any() and (P.jerk[n:] == SENTINEL).all()
    gpu_ctx.qactor_destroy(raw)
    gpu_ctx.check_error()
