#!/usr/bin/env python3
"""Golden vectors for the first-step shield controller: the reference's own ``st.do_conditional_st_based_on_first_step`` (st.py:805-814),
unmodified, under configs/combined_medium_1.json.

Build-container only (needs /root/reference).  The reference is imported as make_golden_combined_real.py imports it (inert ``traci`` / ``cvxopt``
stand-ins).  For every (state, start_speed) pair the reference's function is called once; what it computes on the way is recorded through
wrappers around the two functions it calls -- ``HighwayState.predict_step_with_ego(start_speed, delta_t=TICK_LENGTH)`` (the next state's arrays
and ``crashed``) and ``st.test_guaranteed_crash_from_state(next_state)`` (``crash_guaranteed``) -- together with the branch it takes.
``st.do_st_control`` and ``control.set_ego_speed`` are recorders: the taken-over speed passes through cvxopt, which the image lacks, so the suite
compares it with this project's own ``st_control`` instead.

Inputs: the first N_STATES start states of golden_combined_real.npz, each with three proposed speeds -- ``control.get_ego_speed_from_jerk`` of its
recorded first action, of jerk -5 and of jerk +5 --, then, only if a branch were still short, merge-zone states of ``synth.generate_states`` in
blocks of 60 until the counts hold.  The file is refused unless at least 20 pairs have ``crashed``, 20 have ``crash_guaranteed`` and not
``crashed``, and 100 have neither.

Counts of the committed file: 1620 pairs = 720 from the 240 states of golden_combined_real.npz + 900 from 300 added merge-zone states (the combined
goldens alone were short of a branch); crashed 59, crash_guaranteed and not crashed 23, neither 1538 (COUNTS below: a re-run must reproduce them).
Re-run:  python tests/golden/make_golden_first_step.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import import_reference, REF      # noqa: E402

N_STATES = 240
NEED = {"crashed": 20, "guaranteed": 20, "neither": 100}
#: (crashed, crash_guaranteed and not crashed, neither) of the committed file
COUNTS = (59, 23, 1538)
JERKS = (-5.0, 5.0)


def main():
    S, control, prediction, st, st_cy = import_reference()
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import synth
    S.load_from_file(os.path.join(REF, "configs", "combined_medium_1.json"))
    for k_, v_ in pkg.REFERENCE_DEFAULT.items():
        setattr(S, k_, v_)
    g = dict(np.load(os.path.join(HERE, "golden_combined_real.npz"), allow_pickle=False))
    K = g["other_x"].shape[1]

    seen = {}
    real_predict = prediction.HighwayState.predict_step_with_ego
    real_test = st.test_guaranteed_crash_from_state

    def predict(self, selected_speed, delta_t, min_crash_distance=5):
        if "next" in seen:                  # (the solver's own traffic prediction, st.py:42-43, comes through here too)
            return real_predict(self, selected_speed, delta_t, min_crash_distance)
        assert delta_t == S.TICK_LENGTH and min_crash_distance == 5
        seen["next"], seen["crashed"] = real_predict(self, selected_speed, delta_t, min_crash_distance)
        return seen["next"], seen["crashed"]

    def test(state):
        assert state is seen["next"]
        seen["guaranteed"] = real_test(state)
        return seen["guaranteed"]

    prediction.HighwayState.predict_step_with_ego = predict
    st.test_guaranteed_crash_from_state = test
    st.do_st_control = lambda state: seen.setdefault("st", True) and "ST"
    control.set_ego_speed = lambda speed: seen.setdefault("set", speed)
    st.print = lambda *a, **kw: None

    rows = []

    def run(ego4, kk, xs, vs, accs, jerk):
        speed = control.get_ego_speed_from_jerk(float(ego4[2]), float(ego4[3]), float(jerk))
        state = prediction.HighwayState((float(ego4[0]), float(ego4[1])), float(ego4[2]), float(ego4[3]), [float(x) for x in xs[:kk]],
                                        [float(v) for v in vs[:kk]], [float(a) for a in accs[:kk]])
        seen.clear()
        out = st.do_conditional_st_based_on_first_step(state, speed)
        nxt, crashed, guaranteed = seen["next"], bool(seen["crashed"]), bool(seen["guaranteed"])
        took = "st" in seen
        assert took == (crashed or guaranteed) and (out == "ST") == took and (took or seen["set"] == speed)
        pad = lambda v: np.concatenate([np.asarray(v, dtype=np.float64), np.zeros(K - kk)])
        rows.append(dict(ego=np.array([ego4[0], ego4[1], ego4[2], ego4[3], control.get_ego_s(state.ego_position)], dtype=np.float64), k_count=kk,
                         other_x=pad(xs[:kk]), other_v=pad(vs[:kk]), other_a=pad(accs[:kk]), jerk=float(jerk), start_speed=float(speed),
                         next_ego=np.array([nxt.ego_position[0], nxt.ego_position[1], nxt.ego_speed, nxt.ego_acceleration,
                                            control.get_ego_s(nxt.ego_position)], dtype=np.float64),
                         next_other_x=pad(nxt.other_xs), next_other_v=pad(nxt.other_speeds), crashed=int(crashed), crash_guaranteed=int(guaranteed),
                         branch=1 if crashed else (2 if guaranteed else 0)))

    def counts():
        cr = sum(r["crashed"] for r in rows)
        gu = sum(1 for r in rows if r["crash_guaranteed"] and not r["crashed"])
        return {"crashed": cr, "guaranteed": gu, "neither": sum(1 for r in rows if not r["crashed"] and not r["crash_guaranteed"])}

    for i in range(N_STATES):
        for jerk in (float(g["jerks"][i, 0]),) + JERKS:
            run(g["ego"][i], int(g["k_count"][i]), g["other_x"][i], g["other_v"][i], g["other_a"][i], jerk)
    n_real = len(rows)
    added, block = 0, 0
    while any(counts()[q] < NEED[q] for q in NEED) and added < 600:
        ego, kc, ox, ov = synth.generate_states(60, k=6, kmax=K, seed=900 + block, vary_k=True, dt=0.2, blocked_quota=0.0)
        rng = np.random.default_rng(950 + block)
        ego[:, 0] = rng.uniform(-45.0, 20.0, 60)                       # the merge zone and just past it: where a step can crash
        ego[:, 1] = synth.road_y(ego[:, 0])
        ego[:, 2] = np.clip(rng.normal(12.0, 4.0, 60), 0.5, 24.0)
        ego[:, 3] = np.clip(rng.normal(0.0, 1.0, 60), -3.0, 3.0)
        for i in range(60):
            for jerk in (0.0,) + JERKS:
                run(ego[i], int(kc[i]), ox[i], ov[i], np.zeros(K), jerk)
        added += 60
        block += 1
    c = counts()
    short = [q for q in NEED if c[q] < NEED[q]]
    if short:
        raise SystemExit("refusing to write the fixture: branches %s are short (%s, need %s)" % (short, c, NEED))
    if COUNTS is not None:
        assert (c["crashed"], c["guaranteed"], c["neither"]) == COUNTS, (c, COUNTS)
    col = lambda name, dtype=np.float64: np.array([r[name] for r in rows], dtype=dtype)
    keys = ["TICK_LENGTH", "COMBINATION_MIN_DISTANCE", "CAR_LENGTH", "T_DISCRETIZATION", "S_DISCRETIZATION", "FUTURE_T", "FUTURE_S"]
    np.savez_compressed(os.path.join(HERE, "golden_first_step.npz"), ego=col("ego"), k_count=col("k_count", np.int32), other_x=col("other_x"),
                        other_v=col("other_v"), other_a=col("other_a"), jerk=col("jerk"), start_speed=col("start_speed"), next_ego=col("next_ego"),
                        next_other_x=col("next_other_x"), next_other_v=col("next_other_v"), crashed=col("crashed", np.int32),
                        crash_guaranteed=col("crash_guaranteed", np.int32), branch=col("branch", np.int32), n_from_combined_real=np.array(n_real),
                        setting_keys=np.array(keys), setting_vals=np.array([float(getattr(S, q)) for q in keys]))
    print("first step: %d pairs (%d from golden_combined_real.npz, %d synthetic states added): crashed %d, crash_guaranteed and not crashed %d, neither %d"
          % (len(rows), n_real, added, c["crashed"], c["guaranteed"], c["neither"]))


if __name__ == "__main__":
    main()
