#!/usr/bin/env python3
"""Golden vectors for the combined RL+ST controller (dqn.RLAgent.do_combined_control, dqn.py:117-200) in every settings cell the project
runs it under, generated from the reference itself with the stand-in policy of make_golden_combined.py.

Build-container only; same rules and the same inert stand-ins as make_golden_combined.py.  Writes

  golden_combined_cells.npz    240 states decided in 23 cells:
      base A  configs/combined_medium_1.json, DESIRED_SPEED 30, CHECK_ROLLOUT_CRASH on, LIMIT_DQN_SPEED off: the 13 cells of
              main.do_grid_search_combined (ROLLOUT_LENGTH x ST_TEST_ROLLOUTS x TEST_ROLLOUT_STATE);
      base B  DESIRED_SPEED 16, LIMIT_DQN_SPEED on: five (ROLLOUT_LENGTH, ST_TEST_ROLLOUTS, TEST_ROLLOUT_STATE) x CHECK_ROLLOUT_CRASH on / off.
      Per cell and state: reason, takeover, crash_predicted, rollout_steps, selected_speed; for the first 64 states also the rollout history
      (ragged: hist / hist_off) and the probe state (test_ego4 / test_ox / test_ov, test_fallback: set by dqn.py:142-143, not inside the loop).
  golden_combined_cells_b.npz  the TEST_ST_STRICTLY_BETTER branch on the first 120 states at three rollout lengths of base A, each with
      REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED off and on (st.finer_fit's cvxopt call replaced by oracle/ff_oracle, as in make_golden_combined.py).

How the numbers are taken: do_combined_control runs unmodified.  Recording wrappers sit on the two functions its rollout loop calls once per
step, control.get_ego_speed_from_jerk (called by nothing else on this path) and HighwayState.predict_step_with_ego (the probe and the solver
call it too, but only after the loop): the first len(speeds) predictor calls are the loop's steps.  The history is the reference's
control.get_ego_s of those states; the probe state is the state after step ST_TEST_ROLLOUTS, else the last one, and it is checked against the
object the reference hands to st.test_guaranteed_crash_from_state whenever it gets that far.

Re-run:  python tests/golden/make_golden_combined_cells.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import import_reference, REF                           # noqa: E402
from make_golden_combined import CODES, agent_class                     # noqa: E402

N, N_BOOK, N_B, KMAX = 240, 64, 120, 8
CELL_KEYS = ("ROLLOUT_LENGTH", "ST_TEST_ROLLOUTS", "TEST_ROLLOUT_STATE", "CHECK_ROLLOUT_CRASH", "LIMIT_DQN_SPEED", "DESIRED_SPEED")
BASE_B = [(3, 2, True), (5, 5, True), (10, 2, False), (1, 2, True), (12, 3, True)]
PARTS_B = [(1, 2), (3, 2), (10, 2)]


def cells(pkg):
    from rl_mpc_lanemerging_amd import combined
    out = [dict(c, base=0, CHECK_ROLLOUT_CRASH=True, LIMIT_DQN_SPEED=False, DESIRED_SPEED=30.0) for c in combined.grid_search_cells()]
    for check in (True, False):
        for R, T, P in BASE_B:
            out.append(dict(base=1, ROLLOUT_LENGTH=R, ST_TEST_ROLLOUTS=T, TEST_ROLLOUT_STATE=P, CHECK_ROLLOUT_CRASH=check, LIMIT_DQN_SPEED=True,
                            DESIRED_SPEED=16.0))
    return out


def main():
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    S, control, prediction, st, st_cy = import_reference()
    import dqn                                                  # noqa: E402  (the reference's)
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import synth
    S.load_from_file(os.path.join(REF, "configs", "combined_medium_1.json"))
    for k_, v_ in pkg.REFERENCE_DEFAULT.items():
        setattr(S, k_, v_)
    S.DESIRED_SPEED, S.CHECK_ROLLOUT_CRASH, S.LIMIT_DQN_SPEED = 30.0, True, False
    Agent = agent_class(dqn)

    calls, msgs, speeds, steps, probed = {}, [], [], [], []
    dqn.print = lambda *a, **kw: msgs.append(str(a[0]))
    st.do_st_control = lambda state: calls.setdefault("st", True) and "ST"
    control.set_ego_jerk = lambda jerk: calls.setdefault("rl", jerk) and "RL"
    speed_from_jerk = control.get_ego_speed_from_jerk

    def rec_speed(v, a, j):
        r = speed_from_jerk(v, a, j); speeds.append(float(r)); return r
    control.get_ego_speed_from_jerk = rec_speed                 # dqn.py:135 looks it up as control.<name> at call time
    predict = prediction.HighwayState.predict_step_with_ego

    def rec_predict(self, *a, **kw):
        r = predict(self, *a, **kw); steps.append(r); return r
    prediction.HighwayState.predict_step_with_ego = rec_predict
    probe = st.test_guaranteed_crash_from_state

    def rec_probe(state):
        probed.append(state); return probe(state)
    st.test_guaranteed_crash_from_state = rec_probe             # dqn.py:152 looks it up as st.<name>

    ego, k, ox, ov = synth.generate_states(N, k=6, kmax=KMAX, seed=31, vary_k=True, dt=0.2, blocked_quota=0.02)
    ego[:, 0] = np.random.default_rng(5).uniform(-120.0, 40.0, N)
    ego[:, 1] = synth.road_y(ego[:, 0])
    n = N

    def state_of(i):
        kk = int(k[i])
        return prediction.HighwayState((float(ego[i, 0]), float(ego[i, 1])), float(ego[i, 2]), float(ego[i, 3]),
                                       [float(x) for x in ox[i, :kk]], [float(x) for x in ov[i, :kk]], [0.0] * kk)
    for i in range(n):
        ego[i, 4] = control.get_ego_s(state_of(i).ego_position)

    table = cells(pkg)
    C = len(table)
    assert C == 23
    out = {q: np.zeros((C, n), np.int32) for q in ("reason", "takeover", "crash_predicted", "rollout_steps")}
    out["selected_speed"] = np.zeros((C, n))
    out["test_ego4"], out["test_ox"], out["test_ov"] = np.zeros((C, N_BOOK, 4)), np.zeros((C, N_BOOK, KMAX)), np.zeros((C, N_BOOK, KMAX))
    out["test_fallback"] = np.zeros((C, N_BOOK), np.int32)
    hist, hist_off = [], [0]
    for c, cell in enumerate(table):
        for key in CELL_KEYS:
            setattr(S, key, cell[key])
        for i in range(n):
            state = state_of(i)
            agent = Agent()
            calls.clear(); msgs.clear(); speeds.clear(); steps.clear(); probed.clear()
            agent.do_combined_control(state)
            out["reason"][c, i] = CODES[msgs[0]] if msgs else 0
            assert len(agent.takeover_history) == 1 and ("st" in calls) == agent.takeover_history[0] == (out["reason"][c, i] != 0)
            out["takeover"][c, i] = int(agent.takeover_history[0])
            m = len(speeds)                                     # the loop's steps: one speed and one predictor call each
            assert 1 <= m <= cell["ROLLOUT_LENGTH"] and len(steps) >= m
            out["rollout_steps"][c, i] = m
            out["selected_speed"][c, i] = speeds[-1]
            out["crash_predicted"][c, i] = int(bool(steps[m - 1][1]))
            assert not any(cr for _, cr in steps[:m - 1])      # a predicted crash ends the loop
            fallback = m < cell["ST_TEST_ROLLOUTS"]
            test_state = steps[m - 1][0] if fallback else steps[cell["ST_TEST_ROLLOUTS"] - 1][0]
            if probed:
                assert probed[0] is test_state                  # the very object the reference probes
            assert bool(probed) == (out["reason"][c, i] in (0, 3) and cell["TEST_ROLLOUT_STATE"])
            assert m == cell["ROLLOUT_LENGTH"] or steps[m - 1][1] or steps[m - 1][0].ego_position[0] > S.STOP_X
            if i < N_BOOK:
                hist.extend([control.get_ego_s(state.ego_position)] + [control.get_ego_s(s.ego_position) for s, _ in steps[:m]])
                hist_off.append(len(hist))
                out["test_ego4"][c, i] = (test_state.ego_position[0], test_state.ego_position[1], test_state.ego_speed, test_state.ego_acceleration)
                out["test_ox"][c, i, :k[i]] = test_state.other_xs
                out["test_ov"][c, i, :k[i]] = test_state.other_speeds
                out["test_fallback"][c, i] = int(fallback)
        print("cell %2d %s: reasons %s, fallback rows %d, short rollouts without a crash %d" % (
            c, {q: cell[q] for q in CELL_KEYS[:4]}, np.bincount(out["reason"][c], minlength=4).tolist(), int(out["test_fallback"][c].sum()),
            int(((out["rollout_steps"][c] < cell["ROLLOUT_LENGTH"]) & (out["crash_predicted"][c] == 0)).sum())))
    for key, val in (("DESIRED_SPEED", 30.0), ("CHECK_ROLLOUT_CRASH", True), ("LIMIT_DQN_SPEED", False), ("ROLLOUT_LENGTH", 5), ("ST_TEST_ROLLOUTS", 5),
                     ("TEST_ROLLOUT_STATE", True)):
        setattr(S, key, val)                                    # base A at the config's own cell again

    # the coverage the suite relies on (tests/test_combined_cells_cpu.py asserts it again on the committed file)
    base = np.array([cell["base"] for cell in table])
    check = np.array([cell["CHECK_ROLLOUT_CRASH"] for cell in table])
    R = np.array([cell["ROLLOUT_LENGTH"] for cell in table])
    reason = out["reason"]
    assert all((reason == r).sum() >= 20 for r in range(4))
    assert all((reason[c] == 2).sum() >= 50 for c in np.nonzero(base == 1)[0])
    assert all((reason[c] == 1).sum() >= 3 for c in np.nonzero(check)[0]) and not (reason[~check] == 1).any()
    changed = set()
    for c in range(13, 18):                                     # base B: cell c has the check on, cell c + 5 has it off
        assert [table[c][q] for q in CELL_KEYS[:3]] == [table[c + 5][q] for q in CELL_KEYS[:3]] and check[c] and not check[c + 5]
        changed |= {(int(a), int(b)) for a, b in zip(reason[c], reason[c + 5]) if a != b}
    assert (1, 2) in changed and (1, 3) in changed, changed
    assert ((out["rollout_steps"] < R[:, None]) & (out["crash_predicted"] == 0)).sum() >= 5
    assert out["test_fallback"].sum(axis=1).max() >= 5

    keys = ["ROLLOUT_LENGTH", "ST_TEST_ROLLOUTS", "COMBINATION_MIN_DISTANCE", "STOP_X", "TICK_LENGTH", "DESIRED_SPEED"]
    np.savez_compressed(os.path.join(HERE, "golden_combined_cells.npz"), ego=ego, k_count=k, other_x=ox, other_v=ov,
                        hist=np.array(hist), hist_off=np.array(hist_off, np.int32), cell_keys=np.array(CELL_KEYS),
                        cell_vals=np.array([[float(cell[q]) for q in CELL_KEYS] for cell in table]), cell_base=base.astype(np.int32),
                        setting_keys=np.array(keys), setting_vals=np.array([float(getattr(S, q)) for q in keys]),
                        flags=np.array([int(S.CHECK_ROLLOUT_CRASH), int(S.LIMIT_DQN_SPEED), int(S.TEST_ROLLOUT_STATE), int(S.TEST_ST_STRICTLY_BETTER)]),
                        **out)

    # ---- part b: TEST_ST_STRICTLY_BETTER at other rollout lengths
    from oracle import ff_oracle as ff
    FS = ff.settings(S.MAX_SPEED, S.MAX_POSITIVE_ACCELERATION, S.MAX_NEGATIVE_ACCELERATION, S.MAXIMUM_POSITIVE_JERK,
                     S.MINIMUM_NEGATIVE_JERK, S.CAR_LENGTH)

    def finer_fit(s_sequence, delta_t, coarse_delta_t, start_speed, start_acceleration, before_after_cars=None):
        return ff.finer_fit(np.asarray(s_sequence, dtype=np.float64), delta_t, coarse_delta_t, start_speed, start_acceleration, FS,
                            before_after_cars)[0]
    st.finer_fit = finer_fit
    S.TEST_ST_STRICTLY_BETTER = True
    sent = []
    control.set_ego_speed = lambda v: sent.append(float(v))
    parts = [(R_, T_, remember) for R_, T_ in PARTS_B for remember in (False, True)]
    P = len(parts)
    b_reason, b_takeover = np.zeros((P, N_B), np.int32), np.zeros((P, N_B), np.int32)
    b_speed, b_last_rl = np.full((P, N_B), np.nan), np.ones((P, N_B), np.int32)
    for p, (R_, T_, remember) in enumerate(parts):
        S.ROLLOUT_LENGTH, S.ST_TEST_ROLLOUTS, S.REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED = R_, T_, remember
        for i in range(N_B):
            agent = Agent()
            if i % 3 == 1:
                agent.takeover_history.append(True)             # previous tick was an ST takeover
                b_last_rl[p, i] = 0
            calls.clear(); msgs.clear(); sent.clear()
            agent.do_combined_control(state_of(i))
            b_takeover[p, i] = int(agent.takeover_history[-1])
            if "st" in calls:                                   # crash / rollout-probe takeovers: do_st_control(start_state)
                b_reason[p, i] = CODES[msgs[0]]
            elif sent:                                          # ST path chosen by the comparison
                b_reason[p, i] = 4
                b_speed[p, i] = sent[0]
            assert b_takeover[p, i] == int(b_reason[p, i] != 0)
        print("part b %d (R %d, T %d, remember %d): reasons %s" % (p, R_, T_, remember, np.bincount(b_reason[p], minlength=5).tolist()))
        assert (b_reason[p] == 0).sum() >= 5 and (b_reason[p] == 4).sum() >= 5
    np.savez_compressed(os.path.join(HERE, "golden_combined_cells_b.npz"), n=np.array(N_B), part_keys=np.array(["ROLLOUT_LENGTH", "ST_TEST_ROLLOUTS", "REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED"]),
                        part_vals=np.array([[int(x) for x in part] for part in parts], np.int32), b_reason=b_reason, b_takeover=b_takeover, b_speed=b_speed,
                        b_last_rl=b_last_rl)
    sizes = [os.path.getsize(os.path.join(HERE, f)) for f in ("golden_combined_cells.npz", "golden_combined_cells_b.npz")]
    print("sizes: %d + %d = %d bytes" % (sizes[0], sizes[1], sum(sizes)))
    assert sum(sizes) < 480 * 1024


if __name__ == "__main__":
    main()
