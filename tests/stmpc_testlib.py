"""Helpers the suite's modules share (plain functions: no fixtures, no hooks, nothing heavy at import time).  Import what a module needs, e.g.
``from stmpc_testlib import pkg as _pkg, bits as _bits, same as _same``.  What only the learner tests share is in learner_testlib.py; no test
module imports another (test_testlib_cpu.py)."""
import contextlib
import json
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    """The package, with its library built if it is not."""
    import rl_mpc_lanemerging_amd as pkg
    if pkg.build.needs_build():
        pkg.build.build()
    return pkg


def capi():
    """The binding (rl_mpc_lanemerging_amd._capi), with its library built if it is not."""
    pkg()
    from rl_mpc_lanemerging_amd import _capi
    return _capi


def bits(a):
    """A float array as the unsigned integers of its bit patterns (anything else as it is): NaNs and signed zeros compare by their bits."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """Equal shape, dtype and bits."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@contextlib.contextmanager
def settings_of(*groups):
    """The global Settings with the values of one or more groups (a traffic group, a reward group, ...) less their ``seed``: how a lone world or env
    of them is made through the plain entries."""
    p = pkg()
    snap = p.Settings.snapshot()
    for group in groups:
        p.apply_overrides({k: v for k, v in group.items() if k != "seed"})
    try:
        yield
    finally:
        p.Settings.restore(snap)


def linit(m):
    """Small random actor and critic nets (21 / 22 -> 400 -> 300 -> 1) of learner ``m``, from its own generator."""
    from rl_mpc_lanemerging_amd import learner
    rng = np.random.default_rng(100 + m)
    a_net, q_net = learner.init_net(21, 400, 300, rng), learner.init_net(22, 400, 300, rng)
    a_net["w2"] = rng.normal(0, 0.05, (1, 300)).astype(np.float32)
    q_net["w2"] = rng.normal(0, 0.05, (1, 300)).astype(np.float32)
    return {"actor": a_net, "critic": q_net}


def build_plan_checker(directory):
    """tests/solve_plan_check.cpp (the solver's launch plan, host code only) compiled into ``directory``; the program's path."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), "solve_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "rl-mpc-lanemerging_amd", "csrc"),
                    os.path.join(REPO, "tests", "solve_plan_check.cpp"), "-o", exe], check=True)
    return exe


def plan_args(p, H):
    """The plan checker's arguments for one parameter set (a dict of stmpc_params' fields): H and DevP's fields as make_devp derives them."""
    dt = (0.0 + p["dt"]) - 0.0
    assert H == int(math.ceil((p["future_t"] + p["dt"]) / p["dt"]))
    args = [H, p["future_s"], p["ds"], dt, dt * dt, math.pow(dt, 3.0), p["v_w"], p["a_w"], p["j_w"], p["v_des"], p["v_max"], p["a_min"], p["a_max"], p["j_min"], p["j_max"]]
    return [repr(float(a)) if isinstance(a, float) else str(a) for a in args]


def plan_of(exe, inputs):
    """The checker's output lines for one solve call: ``inputs`` as profiles/solver/launch_plan_parent.json records them (device shape, N, Kmax,
    grouped, fastdiv_proven, H, params, knobs); the knobs go through the environment."""
    args = [str(inputs[k]) for k in ("num_cu", "lds_per_block", "N", "Kmax")] + [str(int(inputs["grouped"])), str(int(inputs["fastdiv_proven"]))]
    env = {k: v for k, v in os.environ.items() if not k.startswith("STMPC_")}
    env.update(inputs["knobs"])
    out = subprocess.run([exe] + args + plan_args(inputs["params"][0], inputs["H"]), env=env, check=True, capture_output=True, text=True).stdout
    return out.splitlines()


def fastdiv_proven(dt):
    """What solve_device finds for a time step: dt, dt^2 and dt^3 pass fastdiv_ok (a significand that is not all ones, restated here) and the
    library's fastdiv2_ok."""
    from rl_mpc_lanemerging_amd import _capi
    dt = (0.0 + dt) - 0.0

    def fastdiv_ok(d):
        return 1e-100 < d < 1e100 and struct.unpack("<Q", struct.pack("<d", d))[0] & 0xFFFFFFFFFFFFF != 0xFFFFFFFFFFFFF
    return all(fastdiv_ok(d) and _capi.fastdiv2_check(d)[0] for d in (dt, dt * dt, math.pow(dt, 3.0)))


def record_json(path, key, value):
    """Merge one entry into the JSON file ``path`` (evidence under profiles/; the assertions are in the tests)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


# ---- include/stmpc.h ---------------------------------------------------------------------------------------------------------------------------
def header_text(flat=False):
    """include/stmpc.h; ``flat``: with every run of white space made one blank."""
    header = open(os.path.join(REPO, "include", "stmpc.h")).read()
    return " ".join(header.split()) if flat else header


def header_entries(prefix):
    """The names ``prefix``... that the header follows with an opening parenthesis (its functions; a struct named in a cast would count too)."""
    return {n for n in re.findall(r"\b(stmpc_[a-z_0-9]+)\s*\(", header_text()) if n.startswith(prefix)}


def header_prototypes(prefix):
    """name -> argument list (as text) of the prototypes ``prefix``...(...); of the header.  Stricter than ``header_entries``: only what ends
    in ");" counts, which is why both exist."""
    return {name: args for name, args in re.findall(r"\b(%s[a-z_0-9]+)\s*\(([^)]*)\)\s*;" % re.escape(prefix), header_text(flat=True))}


def header_struct_fields(name):
    """Field names and C types of `typedef struct <name> { ... } <name>;` in include/stmpc.h, in order (comments stripped)."""
    header = header_text()
    body = header[header.index("typedef struct %s {" % name) + len("typedef struct %s {" % name):header.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        if stmt.startswith("const "):
            stmt = stmt[6:]
        ctype, rest = stmt.split(" ", 1)
        for n in rest.split(","):
            n = n.strip()
            out.append((n.lstrip("*"), ctype + " *" if n.startswith("*") else ctype))
    return out


# ---- the solver and the combined controller against their goldens ----------------------------------------------------------------------------------
def check_solve(res, ref, H):
    """A solve's integer outputs, cost and path distances equal the reference's, bit for bit (NaNs at the same places)."""
    assert np.array_equal(res["best_t"], ref["best_t"])
    assert np.array_equal(res["path_idx"], ref["path_idx"])
    assert np.array_equal(res["cost"], ref["cost"])
    assert np.array_equal(res["crash"], ref["crash"])
    assert np.array_equal(np.isnan(res["path_dist"]), np.isnan(ref["path_dist"]))
    m = ~np.isnan(ref["path_dist"])
    assert np.array_equal(res["path_dist"][m], ref["path_dist"][m])


def apply_settings(g):
    """The Settings a combined-controller golden ``g`` was generated with; returns the package."""
    import rl_mpc_lanemerging_amd as pkg
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    for key, val in zip(g["setting_keys"], g["setting_vals"]):
        setattr(pkg.Settings, str(key), int(val) if str(key) in ("ROLLOUT_LENGTH", "ST_TEST_ROLLOUTS", "STOP_X") else float(val))
    pkg.Settings.CHECK_ROLLOUT_CRASH, pkg.Settings.LIMIT_DQN_SPEED, pkg.Settings.TEST_ROLLOUT_STATE, \
        pkg.Settings.TEST_ST_STRICTLY_BETTER = [bool(x) for x in g["flags"]]
    return pkg


def combined_cells(g):
    """The cell table of golden_combined_cells.npz as one dict per cell: ``base`` (0: A, 1: B) and the settings of the cell under their names."""
    kinds = {"ROLLOUT_LENGTH": int, "ST_TEST_ROLLOUTS": int, "DESIRED_SPEED": float}
    return [dict({str(key): kinds.get(str(key), bool)(val) for key, val in zip(g["cell_keys"], row)}, base=int(base))
            for row, base in zip(g["cell_vals"], g["cell_base"])]


def apply_cell(g, cell):
    """The Settings of one cell of golden_combined_cells.npz (or one part of golden_combined_cells_b.npz: any dict of settings; ``base`` is no
    setting): the fixture's own, then the cell's.  Returns the package."""
    pkg = apply_settings(g)
    pkg.apply_overrides({key: val for key, val in cell.items() if key != "base"})
    return pkg


def golden_states(g, n=None):
    """The first ``n`` start states of a combined-controller golden as HighwayStates (vehicles cruising: accelerations 0)."""
    from rl_mpc_lanemerging_amd.prediction import HighwayState
    out = []
    for i in range(g["ego"].shape[0] if n is None else n):
        k = int(g["k_count"][i])
        out.append(HighwayState((float(g["ego"][i, 0]), float(g["ego"][i, 1])), float(g["ego"][i, 2]), float(g["ego"][i, 3]),
                                [float(x) for x in g["other_x"][i, :k]], [float(x) for x in g["other_v"][i, :k]], [0.0] * k))
    return out


def stub_policy(state):
    """The stand-in policy of the combined-controller goldens: the arithmetic of tests/golden/make_golden_combined.py::stub_policy, operation for operation."""
    gap = 100.0
    for x in state.other_xs:
        d = x - state.ego_position[0]
        if 0.0 <= d < gap:
            gap = d
    j = 0.4 * (18.0 - state.ego_speed) - 0.8 * state.ego_acceleration - 25.0 / (gap + 5.0) + 1.0
    return max(-5.0, min(5.0, j))


class TwinState:
    """An oracle state under the attribute names a policy reads (``other_accelerations``: the oracle's predictor does not return them)."""

    def __init__(self, st_, xs, vs):
        self.ego_position = (st_.ego_x, st_.ego_y); self.ego_speed = st_.ego_v; self.ego_acceleration = st_.ego_a
        self.other_xs = xs; self.other_speeds = vs


def combined_twin(S, states, policy, nthreads=8):
    """The decision tree of dqn.RLAgent.do_combined_control (dqn.py:117-155) restated on the CPU oracle: its predictor rolls the policy's
    jerks out, its solver probes the rolled-out state.  This is the layer between the reference's recorded decisions and the GPU's: a mismatch
    of the GPU that this twin does not share is the kernels' or the host path's.

    ``S``: the settings (ROLLOUT_LENGTH, ST_TEST_ROLLOUTS, TICK_LENGTH, COMBINATION_MIN_DISTANCE, STOP_X, CHECK_ROLLOUT_CRASH, LIMIT_DQN_SPEED with
    DESIRED_SPEED, TEST_ROLLOUT_STATE, and what the solver reads).  ``states``: (ego[n, >= 4], k_count[n], other_x[n, K], other_v[n, K]).
    ``policy(i, step, state) -> jerk``: asked once per rollout step of state i (step from 1), on a ``TwinState``.

    Returns ``reason`` (0 policy, 1 crash predicted, 2 too fast, 3 probe), ``takeover``, ``crash_predicted``, ``rollout_steps``,
    ``selected_speed`` (of the last step), ``rollout_s`` (one list per state, the start state's s first), ``test_states`` (oracle states: after
    step ST_TEST_ROLLOUTS, else the last rolled-out one) and ``test_fallback`` (which of the two)."""
    from rl_mpc_lanemerging_amd import _capi
    from rl_mpc_lanemerging_amd.combined import get_ego_speed_from_jerk
    from oracle import st_oracle as orc
    ego, k_count, other_x, other_v = states
    op = orc.OrcParams.from_dict(_capi.Params.from_settings(S).as_dict())
    n, K = ego.shape[0], other_x.shape[1]
    reason, crash_predicted, steps = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    selected, fallback = np.zeros(n), np.zeros(n, np.int32)
    rollout_s, test_states, probe = [], [], []
    for i in range(n):
        k = int(k_count[i])
        st_ = orc.make_state(*ego[i, :4], other_x[i, :k], other_v[i, :k])
        hist = [orc.ego_s(st_.ego_x, st_.ego_y)]
        crash, test_state, j, sel = False, None, 0, 0.0
        while not (crash or j >= max(S.ROLLOUT_LENGTH, 1)):                    # dqn.py:129-141
            j += 1
            xs, vs = orc.state_lists(st_)
            sel = get_ego_speed_from_jerk(st_.ego_v, st_.ego_a, policy(i, j, TwinState(st_, xs, vs)))
            st_, crash = orc.predict_with_ego(op, st_, sel, S.TICK_LENGTH, S.COMBINATION_MIN_DISTANCE)
            if j == S.ST_TEST_ROLLOUTS:
                test_state = st_
            hist.append(orc.ego_s(st_.ego_x, st_.ego_y))
            if st_.ego_x > S.STOP_X:
                break
        if test_state is None:                                                 # dqn.py:142-143
            test_state, fallback[i] = st_, 1
        crash_predicted[i], steps[i], selected[i] = crash, j, sel
        rollout_s.append(hist)
        test_states.append(test_state)
        if S.CHECK_ROLLOUT_CRASH and crash:                                    # dqn.py:144-155: the first that holds
            reason[i] = 1
        elif S.LIMIT_DQN_SPEED and sel > S.DESIRED_SPEED:
            reason[i] = 2
        elif S.TEST_ROLLOUT_STATE:
            probe.append(i)
    if probe:
        ts = [test_states[i] for i in probe]
        p_ego = np.array([[t.ego_x, t.ego_y, t.ego_v, t.ego_a, orc.ego_s(t.ego_x, t.ego_y)] for t in ts])
        p_k = np.array([t.k for t in ts], dtype=np.int32)
        p_ox, p_ov = np.zeros((len(ts), K)), np.zeros((len(ts), K))
        for r, t in enumerate(ts):
            p_ox[r, :t.k], p_ov[r, :t.k] = orc.state_lists(t)
        res = orc.solve_batch(op, p_ego, p_k, p_ox, p_ov, solver="layered", nthreads=nthreads)
        reason[np.array(probe)[res["crash"] != 0]] = 3
    return {"reason": reason, "takeover": (reason != 0).astype(np.int32), "crash_predicted": crash_predicted, "rollout_steps": steps,
            "selected_speed": selected, "rollout_s": rollout_s, "test_states": test_states, "test_fallback": fallback}


# ---- actor populations (test_actor_pop.py; the learner tests evaluate views of their learners' actors through the same steps) ------------------
ACTOR_P, ACTOR_N_PER, ACTOR_KMAX = 3, 24, 16
ACTOR_N = ACTOR_P * ACTOR_N_PER


def actor_settings():
    from conftest import load_golden
    g = load_golden("golden_combined_real.npz")
    return g, apply_settings(g).Settings


def episode_settings():
    """The settings of the episode tests: the reference's defaults under the combined controller's medium-1 overrides and traffic."""
    import rl_mpc_lanemerging_amd as pkg
    from rl_mpc_lanemerging_amd import combined_bench
    pkg.apply_overrides(pkg.REFERENCE_DEFAULT)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1)
    pkg.apply_overrides(combined_bench.COMBINED_MEDIUM_1_TRAFFIC)
    return pkg.Settings


def actor_states(g, dev, same=False):
    """72 states of the golden, vehicle slots padded from 8 to Kmax = 16: per member 18 of its first states and, spread over both tiles of the
    member's slice, 6 whose rollout the reference ended after the first step (so that step 2 meets rows that are no longer live).
    ``same``: member 0's 24 states, three times."""
    import torch
    P, N_PER, N, KMAX = ACTOR_P, ACTOR_N_PER, ACTOR_N, ACTOR_KMAX
    short = np.nonzero(g["n_evals"] == 1)[0]
    assert len(short) >= 6 * P
    rows = np.arange(N)
    for m in range(P):
        rows[m * N_PER + np.array([3, 9, 15, 16, 20, 23])] = short[6 * m:6 * m + 6]
    if same:
        rows = np.tile(rows[:N_PER], P)
    pad = lambda a: np.concatenate([a[rows], np.zeros((N, KMAX - a.shape[1]))], axis=1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return {"ego5": t(g["ego"][rows]), "ego4": t(g["ego"][rows][:, :4]), "k": t(g["k_count"][rows]), "ox": t(pad(g["other_x"])), "ov": t(pad(g["other_v"])),
            "oa": t(pad(g["other_a"])), "evals0": t(g["evals0"][rows])}


def actor_two_steps(ctx, S, policy, st, rows):
    """Evaluate ``policy`` on ``rows`` of the states at step 1, roll those rows out one step with its jerks, evaluate at step 2 (only the rows whose
    rollout goes on are evaluated then).  Returns the policy's jerk, input vectors and counters after each step, as numpy."""
    import torch
    from rl_mpc_lanemerging_amd import _capi
    params, ccfg = _capi.Params.from_settings(S), _capi.CombinedCfg.from_settings(S)
    cur = {k: st[k][rows].clone().contiguous() for k in ("ego4", "ox", "ov", "oa")}
    ego5, k = st["ego5"][rows].contiguous(), st["k"][rows].contiguous()
    n = ego5.shape[0]
    policy.keep_features = True
    policy.evals.copy_(st["evals0"][rows])
    policy.feat.fill_(-7.0)
    policy.jerk.fill_(-7.0)
    out = []
    for step in (1, 2):
        jerk = policy(step, cur["ego4"], k, cur["ox"], cur["ov"], cur["oa"])
        torch.cuda.synchronize()
        out.append({"jerk": jerk.cpu().numpy().copy(), "feat": policy.feat.cpu().numpy().copy(), "evals": policy.evals.cpu().numpy().copy()})
        if step == 1:
            ctx.rollout_step_device(params, ccfg, n, ACTOR_KMAX, 1, ego5.data_ptr(), cur["ego4"].data_ptr(), k.data_ptr(), cur["ox"].data_ptr(), cur["ov"].data_ptr(),
                                    cur["oa"].data_ptr(), jerk.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ctx.check_error()
    return out


def actor_eval(ctx, S, policy, st):
    return actor_two_steps(ctx, S, policy, st, slice(0, ACTOR_N_PER))


def assert_steps_equal(got, want, label):
    for step, (a, b) in enumerate(zip(got, want), 1):
        for key in ("jerk", "feat", "evals"):
            assert same(a[key], b[key]), (label, "step", step, key)


def slice_steps(steps, sl):
    return [{k: v[sl] for k, v in s.items()} for s in steps]
