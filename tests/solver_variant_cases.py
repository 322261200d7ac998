"""The solver's k_solve variants, case by case: one table read by the CPU audit (tests/test_solver_variants_cpu.py: which kernels each case launches,
from the pure launch plan) and by the GPU tests (tests/test_solver_variants.py: every case of CASES bit for bit against the oracle, and the statistics
that prove the intended window saw an episode).  A plain module: no fixtures, no hooks.

A case is a dict:
  name      its id
  knobs     the STMPC_* environment it runs under
  lattice   a key of LATTICES (Settings overrides on top of REFERENCE_DEFAULT with CRASH_MIN_S = 20, as the golden files were made), plus
  settings  further overrides of its own
  batch     a key of BATCHES: a golden file's states, or synth.generate_states arguments
  N, Kmax   the batch's shape (grouped: N = groups x the batch)
  groups    None (a lone solve), or the cells of a grouped solve; every group receives the whole batch
  expect    conditions on ctx.stats() after the solve, (counter, comparison, value): they prove that the window the case is about was handed work
  exercises kernels the case is there for: names as tests/solve_plan_check.cpp prints them; the audit looks each up in the case's plan
  test      None for a case tests/test_solver_variants.py runs; for a setting the GPU suite already runs, the test that does ("covered elsewhere":
            the audit counts its kernels, nothing runs it twice)

The plan is computed for DEVICE, an MI355X's shape (profiles/solver/launch_plan_parent.json).  STMPC_WAVES_PER_CU=4 makes the first window's grid one
workgroup per compute unit (256), so 600 states are more than the grid (the side launch) and more than twice it (task splitting)."""
import os

import numpy as np

DEVICE = {"num_cu": 256, "lds_per_block": 163840}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

H40A21 = {"T_DISCRETIZATION": 0.30, "FUTURE_T": 11.7, "S_DISCRETIZATION": 0.05, "FUTURE_S": 360.0, "MAX_POSITIVE_ACCELERATION": 5.2,
          "MAX_NEGATIVE_ACCELERATION": -6.0, "MINIMUM_NEGATIVE_JERK": -35.0, "MAXIMUM_POSITIVE_JERK": 35.0}      # = SYNTHETIC_H40A21's lattice (checked by the audit)
LATTICES = {
    "ref": {},                                                                                      # H = 18, S = 3001, fan-out 9
    "ref_h20": {"FUTURE_T": 5.6},                                                                   # the last horizon whose staged table fits 4096 B
    "ref_h21": {"FUTURE_T": 5.9},                                                                   # the first that does not
    "h40a21": H40A21,                                                                               # H = 40, S = 7201, fan-out 21 (the benchmark's)
    "ref_a21": {"MAX_POSITIVE_ACCELERATION": 5.2, "MINIMUM_NEGATIVE_JERK": -35.0, "MAXIMUM_POSITIVE_JERK": 35.0},   # the reference's cells under the wide fan: its
                                                                                                    # second window covers every cell and is the last tier
    "hbm": {"S_DISCRETIZATION": 0.0125, "FUTURE_S": 375.0, "FUTURE_T": 7.8, "T_DISCRETIZATION": 0.2},   # H = 40, S = 30001: no LDS window covers it
}
BATCHES = {
    "golden_default": {"golden": "golden_default.npz"},
    "ref_k8": {"synth": dict(n=384, k=8, kmax=8, seed=808)},                  # exactly k = kmax = 8: every slot of the staged table is a vehicle
    "ref_k9": {"synth": dict(n=192, k=9, kmax=9, seed=809)},                  # one vehicle more than the staged table holds
    "ref_k0": {"synth": dict(n=192, k=0, kmax=0, seed=800)},                  # Kmax = 0: no vehicle arrays at all
    "ref_192": {"synth": dict(n=192, k=6, kmax=8, seed=6192)},
    "ref_384": {"synth": dict(n=384, k=6, kmax=8, seed=6384)},
    "h40_600": {"synth": dict(n=600, k=6, kmax=8, seed=6100)},
    "h40_150": {"synth": dict(n=150, k=6, kmax=8, seed=6150)},                # x 4 groups = 600
    "hbm_12": {"synth": dict(n=12, k=6, kmax=8, seed=12, vary_k=True, dt=0.2)},
}

# Four cells that differ strongly; 1 and 3 share (v_w, a_w, j_w) and with it one guide table
CELLS4 = [{"V_WEIGHT": 0.0, "D_WEIGHT": 0.0, "MIN_ALLOWED_DISTANCE": 0, "CRASH_MIN_S": 10},
          {"V_WEIGHT": 0.5, "D_WEIGHT": 10.0, "MIN_ALLOWED_DISTANCE": 8, "CRASH_MIN_S": 20},
          {"V_WEIGHT": 10.0, "D_WEIGHT": 10.0, "MIN_ALLOWED_DISTANCE": 0, "CRASH_MIN_S": 15},
          {"V_WEIGHT": 0.5, "D_WEIGHT": 0.0, "MIN_ALLOWED_DISTANCE": 8, "CRASH_MIN_S": 10}]
CELLS2 = [CELLS4[0], CELLS4[1]]

# Knobs left out on purpose, with the reason
EXCLUDED_KNOBS = {"STMPC_CU_RESERVE": "needs CU-masked streams; an experiment stmpc_create clears on most contexts"}

W4 = {"STMPC_WAVES_PER_CU": "4"}
NARROW_BAND = "60"       # a band so narrow that a tenth of the bounds fall below the answer (test_retry_bound_from_the_last_layer_is_exact): retries occur
# Which STMPC_PEN_CELLS the penalty-buffer case runs with: "512,512", or "256,256" had that batch shown hbm_tier == 0 (no lower: the lattice's
# largest step is 248 cells).  On an MI355X "512,512" sends 75 of the 600 episodes there (profiles/solver/variant_cases_stats.json, case pen_cells).
PEN_CELLS_USED = "512,512"


def batch_shape(batch):
    """(N, Kmax) of a batch."""
    spec = BATCHES[batch]
    if "golden" in spec:
        with np.load(os.path.join(GOLDEN, spec["golden"]), allow_pickle=False) as g:
            return int(g["ego"].shape[0]), int(g["other_x"].shape[1])
    s = spec["synth"]
    return s["n"], s["kmax"]


def variant(use_lds, fastdiv, kt, fanmax, s1gen, res, nwx, grouped=False):
    """A k_solve instantiation's name, as the plan checker prints it."""
    b = lambda x: "true" if x else "false"
    return "%sk_solve<%s, false, %s, %d, %d, %s, %d, %d>" % ("grouped::" if grouped else "", b(use_lds), b(fastdiv), kt, fanmax, b(s1gen), res, nwx)


def _case(name, knobs, lattice, batch, expect=(), settings=None, groups=None, exercises=(), shape=None, test=None):
    n, kmax = shape or batch_shape(batch)
    return {"name": name, "knobs": dict(knobs), "lattice": lattice, "settings": dict(settings or {}), "batch": batch, "N": n * (len(groups) if groups else 1),
            "Kmax": kmax, "groups": [dict(c) for c in groups] if groups else None, "expect": list(expect), "exercises": list(exercises), "test": test}


OVERFLOWS = [("fallback", ">", 0)]
TO_HBM = [("fallback", ">", 0), ("hbm_tier", ">", 0)]
WIDE = [("fallback", ">", 0), ("hbm_tier", "==", 0), ("guided", ">", 0), ("pool_exhausted", "==", 0)]      # the benchmark lattice under automatic windows


def _own_cases():
    out = []
    # ---- staged vehicle table (KT = 8), the reference's lattice -------------------------------------------------------------------------------
    for fd in (1, 0):
        for batch in ("golden_default", "ref_k8"):
            kn = {"STMPC_STAGE_TAB": "1", "STMPC_FASTDIV": str(fd)}
            out.append(_case("stage_%s_fd%d" % (batch, fd), kn, "ref", batch, exercises=[variant(1, fd, 8, 9, 0, 0, 4)]))
            # small windows: the staged second window (general shape) gets the first's overflow, the HBM tier the second's
            out.append(_case("stage_%s_fd%d_tiers" % (batch, fd), dict(kn, STMPC_TIERS="256,512"), "ref", batch, TO_HBM,
                             exercises=[variant(1, fd, 8, 9, 0, 0, 8), variant(0, fd, 0, 9, 1, 0, 8)]))
    # the staged kernel as the last tier (the general lattice form next to the table)
    out.append(_case("stage_last_window", {"STMPC_STAGE_TAB": "1", "STMPC_TIERS": "256,4096"}, "ref", "golden_default", OVERFLOWS, exercises=[variant(1, 1, 8, 9, 1, 0, 8)]))
    out.append(_case("stage_last_window_fd0", {"STMPC_STAGE_TAB": "1", "STMPC_TIERS": "256,4096", "STMPC_FASTDIV": "0"}, "ref", "golden_default", OVERFLOWS,
                     exercises=[variant(1, 0, 8, 9, 1, 0, 8)]))
    out.append(_case("stage_h20", {"STMPC_STAGE_TAB": "1"}, "ref_h20", "ref_k8", exercises=[variant(1, 1, 8, 9, 0, 0, 4)]))
    out.append(_case("stage_h20_tiers", {"STMPC_STAGE_TAB": "1", "STMPC_TIERS": "256,512"}, "ref_h20", "ref_k8", TO_HBM, exercises=[variant(1, 1, 8, 9, 0, 0, 8)]))
    out.append(_case("stage_h21_unstaged", {"STMPC_STAGE_TAB": "1"}, "ref_h21", "ref_k8", exercises=[variant(1, 1, 0, 9, 0, 0, 4)]))
    out.append(_case("stage_kmax9_unstaged", {"STMPC_STAGE_TAB": "1"}, "ref", "ref_k9", exercises=[variant(1, 1, 0, 9, 0, 0, 4)]))
    out.append(_case("stage_kmax0", {"STMPC_STAGE_TAB": "1"}, "ref", "ref_k0", exercises=[variant(1, 1, 8, 9, 0, 0, 4)]))
    # ---- the unstaged small-fan kernels under ordinary division, and the last LDS window with work ----------------------------------------------------
    out.append(_case("ref_fd0", {"STMPC_FASTDIV": "0"}, "ref", "golden_default", exercises=[variant(1, 0, 0, 9, 0, 0, 4)]))
    out.append(_case("ref_last_window_fd0", {"STMPC_FASTDIV": "0", "STMPC_TIERS": "256,4096"}, "ref", "golden_default", OVERFLOWS, exercises=[variant(1, 0, 0, 9, 1, 0, 8)]))
    # ---- the wide fan where the second window is the last tier (no HBM tier behind it): resumed and restarted searches in the general lattice form ----
    for fd in (1, 0):
        kn = {"STMPC_TIERS": "512,4096", "STMPC_FASTDIV": str(fd)}
        out.append(_case("a21_last_window_fd%d" % fd, kn, "ref_a21", "ref_384", OVERFLOWS + [("guided", ">", 0)], exercises=[variant(1, fd, 0, 8, 0, 1, 8), variant(1, fd, 0, 8, 1, 2, 8)]))
        out.append(_case("a21_last_window_fd%d_noresume" % fd, dict(kn, STMPC_RESUME="0"), "ref_a21", "ref_384", OVERFLOWS, exercises=[variant(1, fd, 0, 8, 1, 0, 8)]))
        out.append(_case("groups_a21_last_window_fd%d" % fd, kn, "ref_a21", "ref_192", OVERFLOWS, groups=CELLS2, exercises=[variant(1, fd, 0, 8, 1, 0, 8, True)]))
        out.append(_case("groups_ref_last_window_fd%d" % fd, {"STMPC_TIERS": "256,4096", "STMPC_FASTDIV": str(fd)}, "ref", "ref_192", OVERFLOWS, groups=CELLS2,
                         exercises=[variant(1, fd, 0, 9, 1, 0, 8, True)]))
    out.append(_case("groups_ref_fd0", {"STMPC_FASTDIV": "0"}, "ref", "ref_192", groups=CELLS2, exercises=[variant(1, 0, 0, 9, 0, 0, 4, True)]))
    # ---- the benchmark lattice under ordinary division: standard shapes, small windows, without resume ---------------------------------------------------
    out.append(_case("wide_fd0", dict(W4, STMPC_FASTDIV="0"), "h40a21", "h40_600", WIDE, exercises=[variant(1, 0, 0, 8, 0, 1, 4), variant(1, 0, 0, 24, 0, 2, 88)]))
    out.append(_case("wide_fd0_noresume", dict(W4, STMPC_FASTDIV="0", STMPC_RESUME="0"), "h40a21", "h40_600", WIDE, exercises=[variant(1, 0, 0, 8, 0, 0, 4), variant(1, 0, 0, 8, 0, 0, 8)]))
    out.append(_case("wide_fd0_tiers", dict(W4, STMPC_FASTDIV="0", STMPC_TIERS="512,2048"), "h40a21", "h40_600", TO_HBM,
                     exercises=[variant(1, 0, 0, 8, 0, 1, 8), variant(1, 0, 0, 8, 0, 2, 8), variant(0, 0, 0, 8, 1, 0, 8)]))
    # ---- grouped solve on the wide-fan lattice, the cells in both orders ---------------------------------------------------------------------------
    for tag, cells in (("", CELLS4), ("_rev", CELLS4[::-1])):
        out.append(_case("groups_wide" + tag, W4, "h40a21", "h40_150", WIDE[:3], groups=cells,
                         exercises=[variant(1, 1, 0, 8, 0, 0, 4, True), variant(1, 1, 0, 8, 0, 0, 8, True)]))
        out.append(_case("groups_wide_tiers" + tag, dict(W4, STMPC_TIERS="512,2048"), "h40a21", "h40_150", TO_HBM + [("guided", ">", 0)], groups=cells,
                         exercises=[variant(1, 1, 0, 8, 0, 0, 8, True), variant(0, 0, 0, 8, 1, 0, 8, True)]))
        out.append(_case("groups_wide_fd0" + tag, dict(W4, STMPC_FASTDIV="0"), "h40a21", "h40_150", WIDE[:3], groups=cells,
                         exercises=[variant(1, 0, 0, 8, 0, 0, 4, True), variant(1, 0, 0, 8, 0, 0, 8, True)]))
    # no guide table can be built for this lattice (more than 254 cells per step): every group's offset falls back to 0 and the guided attempt is off
    out.append(_case("groups_no_guide_table", {"STMPC_PRUNE": "1"}, "hbm", "hbm_12", [("hbm_tier", ">", 0), ("guided", "==", 0)], groups=CELLS2,
                     exercises=[variant(0, 0, 0, 9, 1, 0, 8, True)]))
    # ---- a round whose 64 sources' targets exceed the penalty buffer: the only way to the HBM tier under a window that covers every cell -----------
    out.append(_case("pen_cells", dict(W4, STMPC_PEN_CELLS=PEN_CELLS_USED), "h40a21", "h40_600", TO_HBM, exercises=[variant(0, 1, 0, 8, 1, 0, 8)]))
    # ---- waves per workgroup: the first window in the full-width list-search shape ------------------------------------------------------------------
    for nw, tag, second in (("8", "8", variant(1, 1, 0, 24, 0, 2, 88)), ("8,4", "8_4", variant(1, 1, 0, 8, 0, 2, 8))):
        out.append(_case("nw%s" % tag, dict(W4, STMPC_NW=nw), "h40a21", "h40_600", WIDE, exercises=[variant(1, 1, 0, 8, 0, 1, 8), second]))
        out.append(_case("nw%s_noresume" % tag, dict(W4, STMPC_NW=nw, STMPC_RESUME="0"), "h40a21", "h40_600", WIDE, exercises=[variant(1, 1, 0, 8, 0, 0, 8)]))
    # ---- the remaining knobs: each only trades speed ----------------------------------------------------------------------------------------------
    retry = {"STMPC_RETRY": "1.0001,1.0002,1.0003", "STMPC_BAND": NARROW_BAND}
    RETRIES = WIDE + [("retries", ">", 0)]
    for name, kn, expect in [
            ("split0", {"STMPC_SPLIT": "0"}, WIDE),
            ("prio0", {"STMPC_PRIO": "0"}, WIDE), ("prio1", {"STMPC_PRIO": "1"}, WIDE),
            ("prio_mode1", {"STMPC_PRIO_MODE": "1"}, WIDE), ("prio_mode2", {"STMPC_PRIO_MODE": "2"}, WIDE), ("prio_mode3", {"STMPC_PRIO_MODE": "3"}, WIDE),
            ("retry_small_steps", retry, RETRIES),
            ("retry_move1", {"STMPC_RETRY_MOVE": "1"}, WIDE), ("retry_move2", dict(retry, STMPC_RETRY_MOVE="2"), RETRIES),
            ("retire_64_at75", {"STMPC_RETIRE_CUS": "64", "STMPC_RETIRE_AT": "75"}, WIDE), ("retire_64_at200", {"STMPC_RETIRE_CUS": "64", "STMPC_RETIRE_AT": "200"}, WIDE),
            ("side_grid1", {"STMPC_SIDE_GRID": "1"}, WIDE),
            ("bp16", {"STMPC_BP16": "1"}, WIDE),
            # (bounds half as tight again: half the batch overflows the first window, more than the checkpoint pool's 256 entries -- no pool condition)
            ("bound_infl", {"STMPC_BOUND_INFL": "1.5"}, WIDE[:3]),
            ("band2_mult1", {"STMPC_BAND2_MULT": "1"}, WIDE), ("band2_mult40", {"STMPC_BAND2_MULT": "40"}, WIDE),
            ("lds_headroom", {"STMPC_LDS_HEADROOM": "8192"}, WIDE)]:
        out.append(_case(name, dict(W4, **kn), "h40a21", "h40_600", expect, exercises=[variant(1, 1, 0, 8, 0, 1, 4), variant(1, 1, 0, 24, 0, 2, 88)]))
    return out


# ---- the settings the GPU suite already runs: knobs, lattice, batch shape and the test ------------------------------------------------------------
GOLDEN_LATTICE = {"golden_default.npz": "ref", "golden_uncertainty.npz": "ref", "golden_h40a21.npz": "h40a21", "golden_h40a21_unc.npz": "h40a21"}   # (uncertainty: not read by the plan)
LIMITS = {"H=64": (dict(T_DISCRETIZATION=0.1, FUTURE_T=6.3), 256, 8), "S=60001": (dict(S_DISCRETIZATION=0.005, FUTURE_S=300.0, FUTURE_T=3.0), 48, 4),
          "K=32": (dict(), 256, 32), "S=30001,H=40": (LATTICES["hbm"], 24, 8), "H=2": (dict(FUTURE_T=0.3), 128, 8), "S=4": (dict(FUTURE_S=0.1), 64, 8)}
OTHER_SETS = [(dict(MAX_POSITIVE_ACCELERATION=5.2, MINIMUM_NEGATIVE_JERK=-35.0, MAXIMUM_POSITIVE_JERK=35.0), 8),
              (dict(FUTURE_T=2.0, T_DISCRETIZATION=0.5, S_DISCRETIZATION=0.1, FUTURE_S=60.0), 16),
              (dict(S_DISCRETIZATION=0.025, FUTURE_S=100.0, FUTURE_T=3.0), 4),
              (dict(MAX_SPEED=12, DESIRED_SPEED=10.0, V_WEIGHT=0.0, A_WEIGHT=0.0, J_WEIGHT=0.0), 8)]
FAILING_DT = 0.3500034505541218      # test_fastdiv2.FAILING_D


def _elsewhere_cases():
    out = []
    par, grp = "test_gpu_parity::", "test_solver_groups::"

    def add(test, knobs, lattice, n, kmax, expect=(), settings=None, groups=None):
        out.append(_case("elsewhere%03d" % len(out), knobs, lattice, None, expect, settings, groups, shape=(n, kmax), test=test))

    def goldens(test, knobs, files=tuple(GOLDEN_LATTICE)):
        for f in files:
            with np.load(os.path.join(GOLDEN, f), allow_pickle=False) as g:
                add(test, knobs, GOLDEN_LATTICE[f], int(g["ego"].shape[0]), int(g["other_x"].shape[1]))

    goldens(par + "test_batch_matches_reference_golden", {})
    for prune, band in (("0", "0"), ("1", "0"), ("1", "3"), ("1", "100000"), ("2", "0"), ("1", "nodense")):
        kn = {"STMPC_PRUNE": "1" if prune == "2" else prune}
        kn.update({"STMPC_TWO_PHASE": "1"} if prune == "2" else {})
        kn.update({"STMPC_BAND_DENSE": "0"} if band == "nodense" else ({"STMPC_BAND": band} if band != "0" else {}))
        goldens(par + "test_bounded_search_is_exact", kn)
    for last_infl, band in (("1", "450"), ("1.005", "450"), ("1.5", "450"), ("1.005", "60"), ("4", "900")):
        kn = {"STMPC_LAST_INFL": last_infl, "STMPC_BAND": band}
        add(par + "test_retry_bound_from_the_last_layer_is_exact", kn, "h40a21", 1536, 8, [("retries", ">", 0)])
        goldens(par + "test_retry_bound_from_the_last_layer_is_exact", kn)
    for tube, dense in (("0", "1"), ("8", "1"), ("96", "1"), ("96", "0"), ("127", "1"), ("4000", "1")):
        goldens(par + "test_guided_bounding_attempt_is_exact", {"STMPC_TUBE": tube, "STMPC_TUBE_DENSE": dense})
    # (STMPC_FORCE_GENERAL: every episode is routed to the last tier -- all of them "fall back", whatever the windows)
    goldens(par + "test_general_lattice_form_routing", {"STMPC_FORCE_GENERAL": "1"}, ("golden_default.npz", "golden_h40a21.npz"))
    for tiers in ("64", "256,512", "512,2048", "64,128,256"):
        for fd in ("1", "0"):
            add(par + "test_window_overflow_falls_back_exactly", {"STMPC_TIERS": tiers, "STMPC_FASTDIV": fd}, "ref", 320, 8, TO_HBM if tiers == "64" else OVERFLOWS)
    for kmax in (6, 8, 1, 20):
        add(par + "test_batch_matches_oracle_seeded", {}, "ref", 512, kmax)
    add(par + "test_h40a21_matches_oracle_seeded", {}, "h40a21", 192, 8)
    for over, kmax in OTHER_SETS:
        add(par + "test_other_parameter_sets_match_oracle", {}, "ref", 384, kmax, settings=over)
    for n in (8192, 257):
        add(par + "test_config4_shard_properties", {}, "h40a21", n, 8)
    for n in (4096, 129):
        add(par + "test_full_size_batch_properties", {}, "h40a21", n, 8)
    add(par + "test_fused_action_cost_rows_and_one_8192_shard", {}, "h40a21", 8192, 8)
    for overlap, resume, pool in (("1", "1", ""), ("0", "1", ""), ("1", "0", ""), ("0", "0", ""), ("1", "1", "7"), ("0", "1", "1")):
        kn = {"STMPC_OVERLAP": overlap, "STMPC_RESUME": resume}
        kn.update({"STMPC_POOL": pool} if pool else {})
        add(par + "test_concurrent_overflow_launch_is_exact", kn, "h40a21", 1400, 8, OVERFLOWS)
    for name, (over, n, kmax) in LIMITS.items():
        add(par + "test_limits_of_the_interface", {}, "ref", n, kmax, [("hbm_tier", ">", 0)] if name == "S=30001,H=40" else (), settings=over)
    for n in (2600, 1, 1025, 2047, 2049, 300, 1024):
        add(par + "test_batch_sizes_around_the_scheduling_thresholds", {}, "h40a21", n, 8)
    for cap in ("0", "20", "300", "100000"):
        goldens(par + "test_band_cap_never_changes_results", {"STMPC_PRUNE": "1", "STMPC_BAND_CAP": cap})
    for gsh, heavy in (("0", "0"), ("1", "0"), ("3", "1"), ("4", "1")):
        kn = {"STMPC_GSH": gsh, "STMPC_HEAVY_FIRST": heavy}
        goldens(par + "test_lane_mapping_and_task_order_never_change_results", kn)
        add(par + "test_lane_mapping_and_task_order_never_change_results", kn, "h40a21", 2300, 8)
    add(par + "test_narrow_lattice_side_launch_follows_the_previous_batch", {}, "ref", 1400, 8)
    add(par + "test_narrow_lattice_side_launch_follows_the_previous_batch", {"STMPC_FORCE_GENERAL": "1"}, "ref", 1400, 8)
    add("test_fastdiv2::test_gpu_solver_with_a_dt_that_fails_the_check", {}, "h40a21", 600, 8,
        settings={"T_DISCRETIZATION": FAILING_DT, "FUTURE_T": 23 * FAILING_DT + 1e-9, "FUTURE_S": 300.0})
    cells = [{}] * 4          # (the plan reads no field the cells may set, but for the band, which chooses no kernel)
    add(grp + "test_group_equals_lone_equals_oracle", {}, "ref", 5, 8, groups=cells)
    for fd in ("1", "0"):
        add(grp + "test_group_equals_lone_with_first_window_overflow", {"STMPC_TIERS": "256,512", "STMPC_FASTDIV": fd}, "ref", 5, 8, OVERFLOWS, groups=cells)
    add(grp + "test_overflow_with_the_side_launch", {"STMPC_TIERS": "256,512", "STMPC_OVERLAP": "1", "STMPC_WAVES_PER_CU": "4"}, "ref", 320, 8, OVERFLOWS, groups=cells)
    add(grp + "test_one_group_and_288_groups", {}, "ref", 37, 8, groups=[{}])
    add(grp + "test_one_group_and_288_groups", {}, "ref", 1, 8, groups=[{}] * 288)
    return out


CASES = _own_cases()                        # what tests/test_solver_variants.py runs
ELSEWHERE = _elsewhere_cases()              # what other GPU tests run already
ALL = CASES + ELSEWHERE
assert len({c["name"] for c in ALL}) == len(ALL)
