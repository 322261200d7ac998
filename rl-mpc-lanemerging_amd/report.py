"""The reference's full evaluation report for the batched episodes: what ``control.evaluate_control`` + ``stats.StatsAggregator`` print,
plot and dump, from the on-device flight recorder (``stmpc_rec_*``, csrc/stmpc_rec_kernels.hpp).

* the per-episode columns and the three ``_merged`` columns (stats.py:54-74), their means and standard errors
  (``get_stat_averages(report_stds=True)``, stats.py:145-158) and the report row (``get_stat_report_row_dict``, stats.py:160-190);
* the position-binned profiles: ``counts`` / ``jerks`` / ``speeds`` over ``bins`` (stats.py:33-52, printed by ``print_stats``) and the share of
  ticks the ST solver took over per bin (``RLAgent.plot_st_proportion``, dqn.py:215-226, fed by ``combined_stats_callback``, dqn.py:101-115);
* the crash dump (``save_state_on_crash``, stats.py:75-77; TASK "ST" = ``st.evaluate_st_and_dump_crash``, st.py:822-824): the last recorded
  states of every environment, and ``replay`` in the role of ``st.replay_crash`` (st.py:827-847).

``bin_profiles_host`` and ``report_host`` are host twins written in the reference's own operation order; the test suite pins them to the
reference's unmodified ``stats.py`` (recorded outputs, golden_stats.npz) and the device recorder to them.

The recorder follows ONE episode per environment (``episodes.EpisodeRunner``).  ``vec_env.MergeVecEnv``'s autoreset starts further episodes
inside the step kernel; recording those is out of scope.
"""
import numpy as np

from . import _capi
from .config import Settings

DEFAULT_BINS = np.arange(-220, 61, 20)          # StatsAggregator.bins (stats.py:33) = default_bins of plot_st_proportion (dqn.py:216)
# get_stats()'s keys (stats.py:91-110) without the two wall-clock lists, then the combined controller's custom stat (dqn.py:115)
STAT_NAMES = ("crashed", "merged", "mean_speed", "max_speed", "mean_abs_jerk", "closest_distance", "mean_closest_distance", "mean_abs_jerk_merged",
              "closest_distance_merged", "mean_closest_distance_merged", "mean_disruption", "max_disruption", "total_disruption", "disruption_time",
              "time_taken", "time_to_merge")
PERCENT_ST = "percent st solver"


class RecorderConfig:
    """``depth``: records kept per environment (1 ... 64: the run-up to its end); ``bins``: the bin edges of the position profiles (at most 32)."""

    def __init__(self, depth=32, bins=DEFAULT_BINS):
        self.depth = int(depth)
        self.bins = np.ascontiguousarray(bins, dtype=np.float64).reshape(-1)


class Recorder:
    """The device recorder of one world (``stmpc_rec``): ``tick`` between the controller and ``sim_step``, ``read`` at the end."""

    def __init__(self, ctx, n, kmax, config, tick_length):
        self.ctx, self.n, self.kmax, self.config = ctx, int(n), int(kmax), config
        self._h = ctx.rec_create(self.n, self.kmax, config.depth, tick_length, config.bins)

    def tick(self, n, kmax, d_ego5, d_k, d_ox, d_ov, d_oa, d_cmd, d_takeover=None, stream=0):
        ptr = lambda t: t.data_ptr() if t is not None else 0
        self.ctx.rec_tick(self._h, n, kmax, ptr(d_ego5), ptr(d_k), ptr(d_ox), ptr(d_ov), ptr(d_oa), ptr(d_cmd), ptr(d_takeover), stream)

    def reset(self, stream=0):
        self.ctx.rec_reset(self._h, stream)

    def reduce(self, d_out=None, stream=0):
        self.ctx.rec_reduce(self._h, d_out.data_ptr() if d_out is not None else 0, stream)

    def read(self, want_ring=True):
        """Host copies (synchronises): ``ring``, ``length``, ``acc_env``, ``acc_reduced``, ``status`` plus ``bins`` and ``kmax``."""
        out = self.ctx.rec_read(self._h, self.n, self.kmax, self.config.depth, self.config.bins.size, want_ring)
        out["bins"], out["kmax"] = self.config.bins.copy(), self.kmax
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.ctx.rec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host twins (the suite's yardsticks) ----------------------------------------------------------------------------------------------------
def bin_profiles_host(xs, jerks, speeds, takeovers, edges, out=None):
    """One episode's contribution to the position profiles, in the reference's own order: ``np.histogram`` for ``counts`` (stats.py:45-46) and for
    the takeover positions (dqn.py:217-218), the running ``while`` loop for ``jerks`` / ``speeds`` (stats.py:47-52).  ``out`` (a dict of the four
    arrays, as returned) is added to in place -- the reference keeps one running array over all episodes, and the order of the additions is part
    of the result's bits.  Where the reference's loop would run off ``bins`` (x beyond the last edge: an IndexError there) the tick is dropped."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = len(edges) - 1
    if out is None:
        out = {q: np.zeros(nb) for q in ("counts", "takeover_counts", "jerks", "speeds")}
    xs = [float(x) for x in xs]
    hist, _ = np.histogram(xs, edges)
    out["counts"] += hist
    if takeovers is not None:
        hist_st, _ = np.histogram([x for x, t in zip(xs, takeovers) if t], edges)
        out["takeover_counts"] += hist_st
    current_bin = 0
    for i, x in enumerate(xs):
        while current_bin < nb and x > edges[current_bin + 1]:
            current_bin += 1
        if current_bin >= nb:
            break
        out["jerks"][current_bin] += abs(jerks[i])
        out["speeds"][current_bin] += abs(speeds[i])
    return out


def report_host(per_episode_histories, edges=DEFAULT_BINS, tick_length=None):
    """The aggregate lists and profiles as ``StatsAggregator.add_episode_stats`` builds them (stats.py:43-85) from ``control.run_episode``'s
    ``episode_stats`` dicts (``position_history``, ``speed_history``, ``jerk_history``, ``closest_vehicle_history``, ``disruption_history``,
    ``crashed``, ``merged``, ``simulation_time_taken``; optionally ``takeover_history`` for ``combined_stats_callback``, dqn.py:101-115).
    Returns ``{"lists": get_stats() without the clock columns, "counts", "jerks", "speeds", "takeover_counts", "bins"}``."""
    tick_length = Settings.TICK_LENGTH if tick_length is None else tick_length
    lists = {name: [] for name in STAT_NAMES}
    prof = None
    for ep in per_episode_histories:
        xs = [pos[0] for pos in ep["position_history"]]
        take = ep.get("takeover_history")
        prof = bin_profiles_host(xs, ep["jerk_history"], ep["speed_history"], take, edges, prof)
        lists["crashed"].append(ep["crashed"])
        lists["merged"].append(ep["merged"])
        lists["time_taken"].append(ep["simulation_time_taken"])
        lists["mean_speed"].append(np.mean(ep["speed_history"]))
        lists["max_speed"].append(np.max(ep["speed_history"]))
        lists["mean_abs_jerk"].append(np.mean(np.abs(ep["jerk_history"])))
        if len(ep["closest_vehicle_history"]) > 0:
            lists["closest_distance"].append(min(ep["closest_vehicle_history"]))
            lists["mean_closest_distance"].append(np.mean(ep["closest_vehicle_history"]))
        if len(ep["disruption_history"]) > 0:
            lists["mean_disruption"].append(np.mean(ep["disruption_history"]))
            lists["max_disruption"].append(np.max(ep["disruption_history"]))
            lists["total_disruption"].append(np.sum(ep["disruption_history"]) * tick_length)
            lists["disruption_time"].append(np.count_nonzero(ep["disruption_history"]) * tick_length)
        if ep["merged"]:
            lists["time_to_merge"].append(ep["simulation_time_taken"])
            lists["closest_distance_merged"].append(min(ep["closest_vehicle_history"]))
            lists["mean_closest_distance_merged"].append(np.mean(ep["closest_vehicle_history"]))
            lists["mean_abs_jerk_merged"].append(np.mean(np.abs(ep["jerk_history"])))
        if take is not None:
            lists.setdefault(PERCENT_ST, []).append(sum(1 for t in take[:len(xs)] if t) / max(len(xs), 1))
    if prof is None:
        prof = bin_profiles_host([], [], [], None, edges)
    return {"lists": lists, "counts": prof["counts"], "jerks": prof["jerks"], "speeds": prof["speeds"], "takeover_counts": prof["takeover_counts"],
            "bins": np.asarray(edges, dtype=np.float64)}


def columns_from_histories(per_episode_histories, tick_length=None):
    """The per-episode columns ``episodes.stats_columns`` returns (NaN where the reference appends nothing), from ``episode_stats`` dicts."""
    tick_length = Settings.TICK_LENGTH if tick_length is None else tick_length
    eps = list(per_episode_histories)
    col = lambda f: np.array([f(ep) for ep in eps], dtype=np.float64)
    some = lambda key, f: col(lambda ep: f(ep[key]) if len(ep[key]) > 0 else np.nan)
    out = {"crashed": col(lambda ep: bool(ep["crashed"])), "merged": col(lambda ep: bool(ep["merged"])),
           "mean_speed": col(lambda ep: np.mean(ep["speed_history"])), "max_speed": col(lambda ep: np.max(ep["speed_history"])),
           "mean_abs_jerk": col(lambda ep: np.mean(np.abs(ep["jerk_history"]))),
           "closest_distance": some("closest_vehicle_history", min), "mean_closest_distance": some("closest_vehicle_history", np.mean),
           "mean_disruption": some("disruption_history", np.mean), "max_disruption": some("disruption_history", np.max),
           "total_disruption": some("disruption_history", lambda h: np.sum(h) * tick_length),
           "disruption_time": some("disruption_history", lambda h: np.count_nonzero(h) * tick_length),
           "time_taken": col(lambda ep: ep["simulation_time_taken"])}
    out["time_to_merge"] = np.where(out["merged"] != 0, out["time_taken"], np.nan)
    if eps and all(ep.get("takeover_history") is not None for ep in eps):
        out["percent_st"] = col(lambda ep: sum(1 for t in ep["takeover_history"][:len(ep["position_history"])] if t) / max(len(ep["position_history"]), 1))
    return out


def reduce_rows_host(acc, threads=256):
    """Host twin of ``k_rec_reduce`` for ``acc`` [rows][n]: per row, ``threads`` partial sums (environment e goes to partial e % threads, in index
    order), then the fixed halving tree.  The order depends on n alone, so this gives the bits the device's reduction has for n environments."""
    acc = np.asarray(acc, dtype=np.float64)
    rows, n = acc.shape
    part = np.zeros((rows, threads))
    for e0 in range(0, n, threads):
        chunk = acc[:, e0:e0 + threads]
        part[:, :chunk.shape[1]] += chunk
    w = threads // 2
    while w > 0:
        part[:, :w] += part[:, w:2 * w]
        w //= 2
    return part[:, 0].copy()


def sem(values):
    """``scipy.stats.sem`` in numpy: std(ddof=1) / sqrt(n) (NaN for fewer than two values, as scipy returns)."""
    a = np.asarray(values, dtype=np.float64)
    if a.size < 2:
        return float("nan")
    return float(np.std(a, ddof=1) / np.sqrt(a.size))


class Trace(list):
    """The recorded states of one environment in tick order: dicts of ``tick``, ``ego5`` (x, y, v, a, s), ``k``, ``other_x`` / ``other_v`` /
    ``other_a`` (``k`` entries each), ``cmd`` (the commanded speed), ``takeover``, ``jerk``; ``env``, ``status`` and ``kmax`` as attributes."""
    env, status, kmax = -1, 0, 0


class Report:
    """Built by ``EpisodeRunner.result()`` (``out["report"]``) from the per-episode columns and the recorder's host copies, or by
    ``Report.from_histories`` from ``episode_stats`` dicts."""

    def __init__(self, columns, profiles, recorded=None):
        self.columns = {k: np.asarray(v) for k, v in columns.items()}
        self._profiles = profiles                   # counts, jerks, speeds, takeover_counts, bins
        self._rec = recorded                        # Recorder.read(), or None
        self.traffic = None                         # the traffic group this report's episodes ran on (by_group / by_member), or None: the global Settings'

    @classmethod
    def from_result(cls, result, recorded):
        """``result``: the dict of ``EpisodeRunner.result()``; ``recorded``: ``Recorder.read()``."""
        nb = len(recorded["bins"]) - 1
        red = recorded["acc_reduced"]
        q = lambda name: red[_capi.REC_QUANTITIES.index(name) * nb:(_capi.REC_QUANTITIES.index(name) + 1) * nb].copy()
        prof = {"counts": q("count"), "takeover_counts": q("takeover_count"), "jerks": q("sum_abs_jerk"), "speeds": q("sum_abs_speed"), "bins": recorded["bins"].copy()}
        cols = {k: v for k, v in result.items() if k not in ("ego4", "report")}
        return cls(cols, prof, recorded)

    def by_group(self, G, traffic):
        """G ``Report``s, group g's from environments [g * n / G, (g + 1) * n / G) of a run with traffic groups (``by_member``'s split), each with
        the TRAFFIC_DESCRIPTION of its own group in ``row()``.  ``traffic``: the G groups as the runner took them."""
        if traffic is None or len(traffic) != G:
            raise ValueError("by_group needs the run's %d traffic groups" % G)
        return self.by_member(G, traffic)

    def by_member(self, P, traffic=None):
        """P ``Report``s, member m's from environments [m * n / P, (m + 1) * n / P): its columns, rings and per-environment accumulators, and the
        profiles summed from the latter in the order the recorder's own reduction has for that many environments (``reduce_rows_host``) -- what a
        recorder of the member's environments alone would hold.  For a run whose policy was an ``actor.ActorPopulation`` of P members
        (the reference: one report row per evaluated model, experiment_data/saved_data.csv).  ``P = 1``: this report itself.
        ``traffic``: None, or the P traffic groups the members ran on (``episodes.traffic_settings`` entries): part m's ``row()`` then describes
        traffic m instead of the global ``Settings``'."""
        from . import episodes
        r = self._need_recorded()
        n = len(r["status"])
        if P < 1 or n % P:
            raise ValueError("%d environments do not split into %d members" % (n, P))
        if traffic is not None and len(traffic) != P:
            raise ValueError("%d traffic groups for %d parts" % (len(traffic), P))
        groups = [episodes.traffic_settings(t) for t in traffic] if traffic is not None else None
        if P == 1:
            if groups is None:
                return [self]
            one = Report(self.columns, self._profiles, self._rec)
            one.traffic = groups[0]
            return [one]
        npm, nb, out = n // P, len(r["bins"]) - 1, []
        for m in range(P):
            sl = slice(m * npm, (m + 1) * npm)
            acc = np.ascontiguousarray(r["acc_env"][:, sl])
            rec = {"ring": r["ring"][sl].copy() if r["ring"] is not None else None, "length": r["length"][sl].copy(), "acc_env": acc,
                   "acc_reduced": reduce_rows_host(acc), "status": r["status"][sl].copy(), "bins": r["bins"].copy(), "kmax": r["kmax"]}
            out.append(Report.from_result({k: v[sl] for k, v in self.columns.items()}, rec))
            if groups is not None:
                out[-1].traffic = groups[m]
        return out

    @classmethod
    def from_histories(cls, per_episode_histories, edges=DEFAULT_BINS, tick_length=None):
        eps = list(per_episode_histories)
        h = report_host(eps, edges, tick_length)
        return cls(columns_from_histories(eps, tick_length), {k: h[k] for k in ("counts", "jerks", "speeds", "takeover_counts", "bins")})

    # -- the aggregate lists, stats.py:54-74 ----------------------------------------------------------------------------------------------------
    def lists(self):
        """``StatsAggregator.get_stats()`` (without the clock columns): per stat the values of the episodes the reference appends one for --
        every episode, or those with at least one sample (``closest_distance``, the disruption columns), or the merged ones (``time_to_merge``
        and the ``_merged`` columns, stats.py:70-74)."""
        c = self.columns
        merged = c["merged"] != 0
        have = lambda name: ~np.isnan(c[name])
        out = {}
        for name in ("crashed", "merged", "mean_speed", "max_speed", "mean_abs_jerk", "time_taken"):
            out[name] = c[name]
        for name in ("closest_distance", "mean_closest_distance", "mean_disruption", "max_disruption", "total_disruption", "disruption_time"):
            out[name] = c[name][have(name)]          # the reference's quirk: episodes without a sample are skipped, not counted as NaN
        out["time_to_merge"] = c["time_taken"][merged]
        out["mean_abs_jerk_merged"] = c["mean_abs_jerk"][merged]
        # (a merged episode without a closest-vehicle sample makes the reference's min() raise; it cannot merge without passing CRASH_MIN_S)
        out["closest_distance_merged"] = c["closest_distance"][merged & have("closest_distance")]
        out["mean_closest_distance_merged"] = c["mean_closest_distance"][merged & have("mean_closest_distance")]
        out = {name: out[name] for name in STAT_NAMES}
        if "percent_st" in c:
            out[PERCENT_ST] = c["percent_st"]
        return out

    def merged_columns(self):
        """The three ``_merged`` columns per episode (NaN for episodes that did not merge)."""
        c = self.columns
        merged = c["merged"] != 0
        return {name + "_merged": np.where(merged, c[name], np.nan) for name in ("mean_abs_jerk", "closest_distance", "mean_closest_distance")}

    def averages(self):
        return {name: (float(np.mean(v)) if len(v) else float("nan")) for name, v in self.lists().items()}

    def stds(self):
        """Standard errors of the means, as ``get_stat_averages(report_stds=True)`` reports them (``scipy.stats.sem``)."""
        return {name: sem(v) for name, v in self.lists().items()}

    def row(self):
        """The report row in ``get_stat_report_row_dict``'s column naming: ``<stat>`` and ``<stat>_std``, then ST_DESCRIPTION and
        TRAFFIC_DESCRIPTION.  It has no TIME stamp and no ``clock_time_*`` columns: those are wall-clock readings of the reference's host loop,
        not reproducible and without a counterpart in a batched run.  The exported Settings are left to the caller."""
        avg, std = self.averages(), self.stds()
        cols = {}
        for name in avg:
            cols[name] = avg[name]
            cols[name + "_std"] = std[name]
        S = Settings
        t = self.traffic or {}
        g = lambda name, default: t[name] if name in t else getattr(S, name, default)
        cols["ST_DESCRIPTION"] = "st-{}-{}-{}-{}-{}-{}-{}-{}".format(S.V_WEIGHT, S.A_WEIGHT, S.J_WEIGHT, S.A_WEIGHT, S.MIN_ALLOWED_DISTANCE, S.CRASH_MIN_S,
                                                                     S.START_UNCERTAINTY, S.UNCERTAINTY_PER_SECOND)
        cols["TRAFFIC_DESCRIPTION"] = "uniform-{}-{}-{}".format(g("OTHER_CAR_SPEED", 7.0), g("BASE_TRAFFIC_INTERVAL", 1.2),
                                                                "varying" if g("VARY_TRAFFIC_START_TIMES", True) else "constant")
        return cols

    # -- the position profiles, stats.py:119-123 / dqn.py:217-219 ---------------------------------------------------------------------------------
    def profiles(self):
        """``counts``, ``avg_jerks = jerks / counts``, ``avg_speeds``, ``st_proportion = takeover_counts / counts`` (NaN in empty bins, as the
        reference's division gives) and ``bins``."""
        p = self._profiles
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"bins": p["bins"], "counts": p["counts"], "jerks": p["jerks"], "speeds": p["speeds"], "takeover_counts": p["takeover_counts"],
                    "avg_jerks": p["jerks"] / p["counts"], "avg_speeds": p["speeds"] / p["counts"], "st_proportion": p["takeover_counts"] / p["counts"]}

    def percent_st(self):
        """Per environment, from the recorder's own totals: ticks taken over / recorded ticks (dqn.py:113)."""
        acc = self._need_recorded()["acc_env"]
        return acc[-2] / np.maximum(acc[-1], 1.0)

    # -- the crash dump -----------------------------------------------------------------------------------------------------------------------------
    def _need_recorded(self):
        if self._rec is None:
            raise ValueError("this Report was not built from a recorder")
        return self._rec

    def traces(self, status=None):
        """The recorded run-up (the last ``min(ticks, depth)`` states before control) of every environment, or of those that ended with
        ``status`` (1 merged, 2 crashed, 3 out of time, 0 still running; a collection selects several)."""
        r = self._need_recorded()
        if r["ring"] is None:
            raise ValueError("the recorder was read without its rings")
        K = r["kmax"]
        want = None if status is None else set(np.atleast_1d(status).tolist())
        out = []
        for e in range(len(r["status"])):
            if want is not None and int(r["status"][e]) not in want:
                continue
            tr = Trace()
            tr.env, tr.status, tr.kmax = e, int(r["status"][e]), K
            for rec in r["ring"][e, :r["length"][e]]:
                k = int(rec[6])
                veh = rec[_capi.REC_HDR:]
                tr.append({"tick": int(rec[0]), "ego5": rec[1:6].copy(), "k": k, "other_x": veh[:k].copy(), "other_v": veh[K:K + k].copy(),
                           "other_a": veh[2 * K:2 * K + k].copy(), "cmd": float(rec[7]), "takeover": bool(rec[8]), "jerk": float(rec[9])})
            out.append(tr)
        return out

    def crashed_traces(self):
        """What the reference pickles into crashed_state_history.pkl (stats.py:75-77), for every crashed environment."""
        return self.traces(status=2)


def replay(trace, ctx=None):
    """The role of ``st.replay_crash`` (st.py:827-847): re-solve every recorded state of one trace -- as ONE batch through
    ``st_control_batch_device`` with the current Settings.  Returns ``path_idx`` [L][H], ``best_t``, ``cost``, ``speed`` (the commanded speeds:
    for a trace recorded under ``controller="st"`` with the same Settings they equal the recorded ``cmd`` bit for bit), ``fine``, ``fine_len``."""
    import torch
    ctx = ctx or _capi.default_context()
    L = len(trace)
    if L == 0:
        raise ValueError("empty trace")
    K = max(int(getattr(trace, "kmax", 0)), max(s["k"] for s in trace), 1)
    ego5, k, ox, ov = np.zeros((L, 5)), np.zeros(L, np.int32), np.zeros((L, K)), np.zeros((L, K))
    for i, s in enumerate(trace):
        ego5[i], k[i] = s["ego5"], s["k"]
        ox[i, :s["k"]], ov[i, :s["k"]] = s["other_x"], s["other_v"]
    params = _capi.Params.from_settings(Settings)
    H = _capi.num_t(params)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.as_tensor(a, device=dev)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    d_ego5, d_k, d_ox, d_ov = t(ego5), t(k), t(ox), t(ov)
    d_path, d_bt, d_cost, d_speed, d_fine, d_fl = z(L, H, dtype=torch.int32), z(L, dtype=torch.int32), z(L), z(L), z(L, _capi.QP_NMAX), z(L, dtype=torch.int32)
    ctx.st_control_batch_device(params, Settings.TICK_LENGTH, L, K, d_ego5.data_ptr(), d_k.data_ptr(), d_ox.data_ptr(), d_ov.data_ptr(), d_path.data_ptr(),
                                d_bt.data_ptr(), d_cost.data_ptr(), d_speed.data_ptr(), d_fine.data_ptr(), d_fl.data_ptr(), 0)
    torch.cuda.synchronize()
    ctx.check_error()
    return {"path_idx": d_path.cpu().numpy(), "best_t": d_bt.cpu().numpy(), "cost": d_cost.cpu().numpy(), "speed": d_speed.cpu().numpy(),
            "fine": d_fine.cpu().numpy(), "fine_len": d_fl.cpu().numpy()}
