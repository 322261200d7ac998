"""ctypes binding of the C-ABI declared in ``include/stmpc.h``.

This is the whole Python<->native boundary: plain pointers and sizes.  There is no CPU
fallback -- if ``libstmpc.so`` is missing the import of this module raises, and if no GPU
is visible ``Context()`` raises ``StmpcError(STMPC_ENODEV)``.
"""
import ctypes as C
import functools
import os

import numpy as np

from . import build as _build

STMPC_OK, STMPC_EINVAL, STMPC_ENODEV, STMPC_EHIP, STMPC_ENOMEM, STMPC_EINTERNAL = 0, -1, -2, -3, -4, -5
KMAX_LIMIT, H_LIMIT, S_LIMIT = 32, 64, 65000      # STMPC_KMAX_LIMIT, ...


class StmpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("stmpc error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    """``stmpc_params`` (include/stmpc.h)."""
    _fields_ = [(n, C.c_double) for n in (
        "future_s", "ds", "dt", "future_t", "start_unc", "unc_per_s",
        "d_w", "v_w", "a_w", "j_w", "v_des", "v_max", "a_min", "a_max", "j_min", "j_max", "min_allowed",
        "car_length", "crash_min_s", "max_pred_decel", "follow_gap", "react_thr", "crash_thr", "comb_min_dist")]

    @classmethod
    def from_settings(cls, S):
        """Read the flags exactly where the reference reads them (st.py:727-746, 37, 46, 800;
        prediction.py:11-12, 85-86)."""
        return cls(
            future_s=S.FUTURE_S, ds=S.S_DISCRETIZATION, dt=S.T_DISCRETIZATION, future_t=S.FUTURE_T,
            start_unc=S.START_UNCERTAINTY, unc_per_s=S.UNCERTAINTY_PER_SECOND,
            d_w=S.D_WEIGHT, v_w=S.V_WEIGHT, a_w=S.A_WEIGHT, j_w=S.J_WEIGHT, v_des=S.DESIRED_SPEED,
            v_max=S.MAX_SPEED, a_min=S.MAX_NEGATIVE_ACCELERATION, a_max=S.MAX_POSITIVE_ACCELERATION,
            j_min=S.MINIMUM_NEGATIVE_JERK, j_max=S.MAXIMUM_POSITIVE_JERK, min_allowed=S.MIN_ALLOWED_DISTANCE,
            car_length=S.CAR_LENGTH, crash_min_s=S.CRASH_MIN_S, max_pred_decel=S.MAX_PREDICTED_DECELERATION,
            follow_gap=30.0, react_thr=8.0, crash_thr=11.0, comb_min_dist=S.COMBINATION_MIN_DISTANCE)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CfgTable:
    """A contiguous ctypes array ``ELEM[G]`` for the group entries, from a sequence of ``ELEM``.  With ``COPY`` the rows are private copies and
    indexing gives the copies; without it the caller's objects are kept alive (with the arrays they point to) and indexing gives them back."""
    ELEM, COPY = None, False

    def __init__(self, rows):
        E = self.ELEM
        self.rows = [E.from_buffer_copy(bytes(r)) for r in rows] if self.COPY else list(rows)
        self.array = (E * max(len(self.rows), 1))()
        for i, r in enumerate(self.rows):
            C.memmove(C.byref(self.array, i * C.sizeof(E)), C.byref(r), C.sizeof(E))

    @classmethod
    def of(cls, x):
        """``x`` itself if it is such a table already, else a table of the sequence ``x``."""
        return x if isinstance(x, cls) else cls(x)

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return self.rows[i]

    def __iter__(self):
        return iter(self.rows)


class ParamsTable(CfgTable):
    """A contiguous ``stmpc_params[G]`` for the solver-group entries, from a sequence of ``Params`` (copied); indexing gives the copies."""
    ELEM, COPY = Params, True
    params = property(lambda self: self.rows)


class Stats(C.Structure):
    _fields_ = [("episodes", C.c_int64), ("fast_path", C.c_int64), ("fallback", C.c_int64), ("hbm_tier", C.c_int64),
                ("retries", C.c_int64), ("nodes_exact", C.c_int64), ("nodes_bound", C.c_int64),
                ("solve_ms", C.c_double), ("dp_kernel_ms", C.c_double), ("guided", C.c_int64), ("resume_refused", C.c_int64), ("pool_exhausted", C.c_int64)]


class CombinedCfg(C.Structure):
    """``stmpc_combined_cfg`` (include/stmpc.h): the flags of dqn.RLAgent.do_combined_control."""
    _fields_ = [("tick_length", C.c_double), ("stop_x", C.c_double), ("rollout_length", C.c_int32), ("st_test_rollouts", C.c_int32),
                ("check_rollout_crash", C.c_int32), ("limit_dqn_speed", C.c_int32), ("test_rollout_state", C.c_int32),
                ("test_st_strictly_better", C.c_int32), ("remember_last_choice", C.c_int32), ("sparse_control", C.c_int32)]

    @classmethod
    def from_settings(cls, S, sparse_control=False):
        """``sparse_control`` (not a reference flag): False (the C-level default: a zeroed field) keeps ``stmpc_combined_decide_device`` fully asynchronous
        -- nothing leaves the GPU, the call can be captured in a hipGraph -- and solves st.do_st_control for every state; True solves it only for
        the states whose decision calls it, as the reference does, at the price of one host round trip per decide call (the count of those
        states).  ``EpisodeRunner`` and the benchmarks ask for it explicitly."""
        return cls(sparse_control=int(bool(sparse_control)), tick_length=S.TICK_LENGTH, stop_x=S.STOP_X, rollout_length=int(S.ROLLOUT_LENGTH), st_test_rollouts=int(S.ST_TEST_ROLLOUTS),
                   check_rollout_crash=int(bool(S.CHECK_ROLLOUT_CRASH)), limit_dqn_speed=int(bool(getattr(S, "LIMIT_DQN_SPEED", False))),
                   test_rollout_state=int(bool(S.TEST_ROLLOUT_STATE)), test_st_strictly_better=int(bool(getattr(S, "TEST_ST_STRICTLY_BETTER", False))),
                   remember_last_choice=int(bool(getattr(S, "REMEMBER_LAST_CHOICE_FOR_SWITCHING_COMBINED", False))))


class CombinedCfgTable(CfgTable):
    """A contiguous ``stmpc_combined_cfg[C]`` for ``stmpc_combined_groups_set``, from a sequence of ``CombinedCfg``; indexing gives the caller's objects."""
    ELEM = CombinedCfg


class FirstStepCfg(C.Structure):
    """``stmpc_first_step_cfg`` (include/stmpc.h): what st.do_conditional_st_based_on_first_step (st.py:805-814) reads besides the solver's settings."""
    _fields_ = [("tick_length", C.c_double), ("min_crash_distance", C.c_double), ("sparse_control", C.c_int)]

    #: the default of HighwayState.predict_step_with_ego's min_crash_distance (prediction.py:46): st.py:806 passes none
    MIN_CRASH_DISTANCE = 5.0

    @classmethod
    def from_settings(cls, S, sparse_control=False):
        """``sparse_control`` as ``CombinedCfg.from_settings`` takes it: False keeps ``stmpc_first_step_device`` asynchronous and solves the controller
        for every state, True only for the taken-over ones at the price of one host round trip."""
        return cls(tick_length=S.TICK_LENGTH, min_crash_distance=cls.MIN_CRASH_DISTANCE, sparse_control=int(bool(sparse_control)))


class ShieldEnvCfg(C.Structure):
    """``stmpc_shield_env_cfg`` (include/stmpc.h): the first-step shield of the shielded vector environment, the takeover penalty and the row stride
    of the planner's view handed to the shield."""
    _fields_ = [("fs", FirstStepCfg), ("takeover_penalty", C.c_double), ("kmax", C.c_int32), ("reserved0", C.c_int32)]

    @classmethod
    def from_settings(cls, S, sparse_control=False, takeover_penalty=0.0, kmax=32):
        return cls(fs=FirstStepCfg.from_settings(S, sparse_control=sparse_control), takeover_penalty=float(takeover_penalty), kmax=int(kmax))


class FeaturesCfg(C.Structure):
    """``stmpc_policy_features_cfg`` (include/stmpc.h): the flags of dqn.get_state_vector_from_base_state (+ the TimeFeature input of ddpg.py:41)."""
    _fields_ = [("max_speed", C.c_double), ("sensor_radius", C.c_double), ("time_scale", C.c_double), ("cars_ahead", C.c_int32), ("cars_behind", C.c_int32),
                ("use_acceleration", C.c_int32), ("use_speed_difference", C.c_int32), ("normalize", C.c_int32), ("time_feature", C.c_int32)]

    @classmethod
    def from_settings(cls, S, time_feature=True):
        g = lambda name, default: getattr(S, name, default)             # the reference's defaults (config.py:35,48-49,136-139)
        return cls(max_speed=float(S.MAX_SPEED), sensor_radius=float(g("SENSOR_RADIUS", 125)), time_scale=0.001, cars_ahead=int(g("CARS_AHEAD", 2)),
                   cars_behind=int(g("CARS_BEHIND", 2)), use_acceleration=int(bool(g("USE_ACCELERATION_OF_OTHER_CARS", True))),
                   use_speed_difference=int(bool(g("USE_SPEED_DIFFERENCE", True))), normalize=int(bool(g("NORMALIZE_VECTOR_INPUT", True))),
                   time_feature=int(bool(time_feature)))


def _combined_shield_fields(S, sparse_control, takeover_penalty, kmax, features, time_feature):
    """The fields ``stmpc_cshield_env_cfg`` and ``stmpc_qshield_env_cfg`` share (``features`` None: the Settings' with ``time_feature``)."""
    f = FeaturesCfg.from_buffer_copy(features) if features is not None else FeaturesCfg.from_settings(S, time_feature=time_feature)
    return dict(cc=CombinedCfg.from_settings(S, sparse_control=sparse_control), features=f, takeover_penalty=float(takeover_penalty), kmax=int(kmax))


class CShieldEnvCfg(C.Structure):
    """``stmpc_cshield_env_cfg`` (include/stmpc.h): the combined controller behind the vector environment -- its flags, the rollout actor's input, the
    takeover penalty, the row stride of the planner's view and the rule of the rollout's time counter."""
    _fields_ = [("cc", CombinedCfg), ("features", FeaturesCfg), ("takeover_penalty", C.c_double), ("kmax", C.c_int32), ("rollout_time", C.c_int32)]

    ROLLOUT_TIMES = {"env": 0, "deployed": 1}

    @classmethod
    def from_settings(cls, S, sparse_control=False, takeover_penalty=0.0, kmax=32, rollout_time="env", features=None):
        """``S``: the ``Settings`` (or an overlay of them) ``do_combined_control`` reads; ``features``: the rollout actor's ``FeaturesCfg`` (default:
        ``FeaturesCfg.from_settings(S)``, the time feature on); ``rollout_time``: "env" or "deployed" (ValueError otherwise)."""
        if rollout_time not in cls.ROLLOUT_TIMES:
            raise ValueError("rollout_time must be one of %s, not %r" % (", ".join(map(repr, cls.ROLLOUT_TIMES)), rollout_time))
        return cls(rollout_time=cls.ROLLOUT_TIMES[rollout_time], **_combined_shield_fields(S, sparse_control, takeover_penalty, kmax, features, True))


class QShieldEnvCfg(C.Structure):
    """``stmpc_qshield_env_cfg`` (include/stmpc.h): the combined controller behind a discrete vector environment with a Q-network in the rollout -- its
    flags, the Q-network's input (no time feature), the takeover penalty and the row stride of the planner's view.  ``stmpc_cshield_env_cfg`` without
    the rollout's time counter."""
    _fields_ = [("cc", CombinedCfg), ("features", FeaturesCfg), ("takeover_penalty", C.c_double), ("kmax", C.c_int32), ("reserved0", C.c_int32)]

    @classmethod
    def from_settings(cls, S, sparse_control=False, takeover_penalty=0.0, kmax=32, features=None):
        """``S``: the ``Settings`` (or an overlay of them) ``do_combined_control`` reads; ``features``: the Q-actor's ``FeaturesCfg`` (default:
        ``FeaturesCfg.from_settings(S, time_feature=False)``)."""
        return cls(**_combined_shield_fields(S, sparse_control, takeover_penalty, kmax, features, False))


class SimCfg(C.Structure):
    """``stmpc_sim_cfg`` (include/stmpc.h): scenario constants of the batched SUMO-free episode runner."""
    _fields_ = [("tick_length", C.c_double), ("other_car_speed", C.c_double), ("base_traffic_interval", C.c_double), ("spawn_x", C.c_double),
                ("despawn_x", C.c_double), ("ego_start_x", C.c_double), ("ego_start_y", C.c_double), ("arrive_x", C.c_double),
                ("sensor_radius", C.c_double), ("start_speed", C.c_double), ("start_speed_std", C.c_double), ("min_start_speed", C.c_double),
                ("max_start_speed", C.c_double), ("veh_accel", C.c_double), ("veh_decel", C.c_double), ("veh_min_gap", C.c_double), ("veh_tau", C.c_double),
                ("veh_emergency_decel", C.c_double), ("veh_length", C.c_double), ("veh_width", C.c_double), ("speed_dev", C.c_double),
                ("vary_traffic_start_times", C.c_int32), ("randomize_start_speed", C.c_int32),
                ("max_ticks", C.c_int32), ("yield_overlap", C.c_int32), ("seed", C.c_uint64),
                ("ego_route_xy", C.POINTER(C.c_double)), ("ego_route_n", C.c_int32), ("reserved0", C.c_int32),
                ("disruption_min_s", C.c_double)]

    def set_route(self, xy):
        """``xy``: [n][2] polyline of the ego's lane centre line (x strictly increasing), or None for the planner's straight lines.
        The array is kept alive by this object; ``stmpc_sim_init_device`` copies it to the device."""
        if xy is None:
            self._route = None
            self.ego_route_xy, self.ego_route_n = None, 0
        else:
            self._route = np.ascontiguousarray(xy, dtype=np.float64)
            assert self._route.ndim == 2 and self._route.shape[1] == 2
            self.ego_route_xy = self._route.ctypes.data_as(C.POINTER(C.c_double))
            self.ego_route_n = int(self._route.shape[0])
        return self


class SimCfgTable(CfgTable):
    """A contiguous ``stmpc_sim_cfg[G]`` for the traffic-group entries, from a sequence of ``SimCfg`` (kept alive with their routes); indexing gives
    the caller's ``SimCfg`` objects."""
    ELEM = SimCfg
    cfgs = property(lambda self: self.rows)


class EnvCfg(C.Structure):
    """``stmpc_env_cfg`` (include/stmpc.h): action mode, reward function and the reference's reward / action settings (merge_gym.py, dqn.py:449-563)."""
    _fields_ = [("action_mode", C.c_int32), ("reward_function", C.c_int32), ("tick_length", C.c_double), ("crash_reward", C.c_double),
                ("success_reward", C.c_double), ("time_reward", C.c_double), ("wt_smooth", C.c_double), ("wt_safe", C.c_double), ("wt_efficient", C.c_double),
                ("alt_v_weight", C.c_double), ("alt_a_weight", C.c_double), ("alt_j_weight", C.c_double), ("alt_d_weight", C.c_double),
                ("min_follow_distance", C.c_double), ("desired_speed", C.c_double), ("car_length", C.c_double), ("invalid_action_penalty", C.c_double),
                ("minimum_negative_jerk", C.c_double), ("maximum_positive_jerk", C.c_double), ("max_negative_acceleration", C.c_double),
                ("max_positive_acceleration", C.c_double), ("max_speed", C.c_double), ("action_values", C.POINTER(C.c_double)), ("n_action_values", C.c_int32),
                ("autoreset", C.c_int32), ("log_capacity", C.c_int32), ("reserved0", C.c_int32), ("features", C.POINTER(FeaturesCfg))]

    @classmethod
    def from_settings(cls, S, action_mode, reward_function, action_values=None, autoreset=True, log_capacity=0):
        """``action_mode`` / ``reward_function``: the STMPC_ENV_* / STMPC_REWARD_* codes; ``action_values``: the discrete action table in index order.
        The arrays it points to are kept alive by this object."""
        c = cls(action_mode=int(action_mode), reward_function=int(reward_function), tick_length=S.TICK_LENGTH, crash_reward=S.CRASH_REWARD,
                success_reward=S.SUCCESS_REWARD, time_reward=S.TIME_REWARD, wt_smooth=S.WT_SMOOTH, wt_safe=S.WT_SAFE, wt_efficient=S.WT_EFFICIENT,
                alt_v_weight=S.ALT_V_WEIGHT, alt_a_weight=S.ALT_A_WEIGHT, alt_j_weight=S.ALT_J_WEIGHT, alt_d_weight=S.ALT_D_WEIGHT,
                min_follow_distance=S.MIN_FOLLOW_DISTANCE, desired_speed=S.DESIRED_SPEED, car_length=S.CAR_LENGTH,
                invalid_action_penalty=S.INVALID_ACTION_PENALTY, minimum_negative_jerk=S.MINIMUM_NEGATIVE_JERK, maximum_positive_jerk=S.MAXIMUM_POSITIVE_JERK,
                max_negative_acceleration=S.MAX_NEGATIVE_ACCELERATION, max_positive_acceleration=S.MAX_POSITIVE_ACCELERATION, max_speed=S.MAX_SPEED,
                autoreset=int(bool(autoreset)), log_capacity=int(log_capacity))
        c._features = FeaturesCfg.from_settings(S, time_feature=False)
        c.features = C.pointer(c._features)
        if action_values is not None:
            c._actions = np.ascontiguousarray(action_values, dtype=np.float64)
            c.action_values = c._actions.ctypes.data_as(C.POINTER(C.c_double))
            c.n_action_values = int(c._actions.size)
        return c


class EnvCfgTable(CfgTable):
    """A contiguous ``stmpc_env_cfg[R]`` for the reward-group entries, from a sequence of ``EnvCfg`` (kept alive with their action tables and
    feature cfgs); indexing gives the caller's ``EnvCfg`` objects."""
    ELEM = EnvCfg
    cfgs = property(lambda self: self.rows)


class DDPGCfg(C.Structure):
    """``stmpc_ddpg_cfg`` (include/stmpc.h): shapes, replay size and the constants of the DDPG update (defaults: the ``all`` preset's)."""
    _fields_ = [("n_obs", C.c_int32), ("h1", C.c_int32), ("h2", C.c_int32), ("batch", C.c_int32), ("capacity", C.c_int32), ("reserved0", C.c_int32),
                ("replay_start", C.c_int64), ("seed", C.c_uint64), ("gamma", C.c_double), ("tau", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("time_scale", C.c_double), ("tanh_scale", C.c_double), ("tanh_mean", C.c_double), ("noise_std", C.c_double),
                ("action_low", C.c_double), ("action_high", C.c_double)]


class TD3Cfg(C.Structure):
    """``stmpc_td3_cfg`` (include/stmpc.h): the DDPG cfg plus the smoothing noise (absolute) and the delay of the actor and the targets."""
    _fields_ = [("base", DDPGCfg), ("target_noise_std", C.c_double), ("noise_clip", C.c_double), ("policy_delay", C.c_int32), ("reserved0", C.c_int32)]


class PERCfg(C.Structure):
    """``stmpc_per_cfg`` (include/stmpc.h): the constants of prioritised replay (defaults: the reference's config.py)."""
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("min_priority", C.c_double), ("max_priority", C.c_double)]


class NStepCfg(C.Structure):
    """``stmpc_nstep_cfg`` (include/stmpc.h): the length of the multi-step return's window and the rows of every push."""
    _fields_ = [("n_step", C.c_int32), ("rows_per_push", C.c_int32)]


class DQNCfg(C.Structure):
    """``stmpc_dqn_cfg`` (include/stmpc.h): the Q-network's shape, the replay size and the constants of the DQN update (defaults: the reference's config.py)."""
    _fields_ = [("n_obs", C.c_int32), ("h1", C.c_int32), ("n_actions", C.c_int32), ("batch", C.c_int32), ("capacity", C.c_int32), ("target_period", C.c_int32),
                ("double_dqn", C.c_int32), ("clip_targets", C.c_int32), ("replay_start", C.c_int64), ("seed", C.c_uint64), ("gamma", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("clip_min", C.c_double), ("clip_max", C.c_double)]


class C51Cfg(C.Structure):
    """``stmpc_c51_cfg`` (include/stmpc.h): ``stmpc_dqn_cfg``'s fields, then the support's ends, the atom count of the categorical head and
    ``dueling`` (0 / 1: the dueling head).  ``reserved`` is that field under the name it had while it had to be 0."""
    _fields_ = list(DQNCfg._fields_) + [("v_min", C.c_double), ("v_max", C.c_double), ("n_atoms", C.c_int32), ("dueling", C.c_int32)]
    reserved = property(lambda self: self.dueling, lambda self, value: setattr(self, "dueling", value))


class NoisyCfg(C.Structure):
    """``stmpc_noisy_cfg`` (include/stmpc.h): the noisy output layer's initial sigma is ``sigma0 / sqrt(h1)``."""
    _fields_ = [("sigma0", C.c_double)]


class ProfileTotals(C.Structure):
    _fields_ = [("launches", C.c_int64), ("episodes", C.c_int64), ("solve_ms", C.c_double), ("dp_kernel_ms", C.c_double)]


_lib = None

EXPORTS = (
    "stmpc_backend_info", "stmpc_last_error", "stmpc_create", "stmpc_destroy", "stmpc_ego_s", "stmpc_num_s",
    "stmpc_num_t", "stmpc_path_mean_abs_jerk", "stmpc_solve_batch_device", "stmpc_solve_batch", "stmpc_get_stats",
    "stmpc_solve_grid", "stmpc_build_grid", "stmpc_predict_batch", "stmpc_probe_arith", "stmpc_profile",
    "stmpc_finer_fit_batch", "stmpc_st_control_batch", "stmpc_st_control_batch_device",
    "stmpc_rollout_step_device", "stmpc_combined_decide_device", "stmpc_combined_read_state", "stmpc_solve_grid_no_jerk",
    "stmpc_sim_init_device", "stmpc_sim_view_device", "stmpc_sim_step_device", "stmpc_sim_read", "stmpc_fastdiv2_check",
    "stmpc_abi_version", "stmpc_check_error", "stmpc_predict_batch_acc", "stmpc_sim_status_device",
    "stmpc_policy_features_device", "stmpc_policy_features_len", "stmpc_combined_counts", "stmpc_solve_batch_device_ac",
    "stmpc_actor_create", "stmpc_actor_destroy", "stmpc_actor_eval_device",
    "stmpc_actor_view_ddpg", "stmpc_actor_pop_create", "stmpc_actor_pop_destroy", "stmpc_actor_pop_size", "stmpc_actor_pop_eval_device",
    "stmpc_env_reset_device", "stmpc_env_step_device", "stmpc_env_reward_device", "stmpc_env_drain", "stmpc_env_episode_seed",
    "stmpc_env_episode_ticks_device",
    "stmpc_sim_init_groups_device", "stmpc_sim_step_groups_device", "stmpc_sim_groups", "stmpc_env_reset_groups_device", "stmpc_env_step_groups_device",
    "stmpc_ddpg_create", "stmpc_ddpg_destroy", "stmpc_ddpg_set_params", "stmpc_ddpg_get_params", "stmpc_ddpg_set_state", "stmpc_ddpg_get_state",
    "stmpc_ddpg_push_device", "stmpc_ddpg_act_device", "stmpc_ddpg_update_device", "stmpc_ddpg_grads_device", "stmpc_ddpg_stats_device",
    "stmpc_ddpg_replay_read", "stmpc_ddpg_gather_device", "stmpc_ddpg_sample_index", "stmpc_ddpg_noise",
    "stmpc_ddpg_pop_create", "stmpc_ddpg_pop_destroy", "stmpc_ddpg_pop_size", "stmpc_ddpg_pop_member", "stmpc_ddpg_pop_act_device",
    "stmpc_ddpg_pop_push_device", "stmpc_ddpg_pop_update_device", "stmpc_ddpg_pop_stats_device",
    "stmpc_td3_create", "stmpc_td3_destroy", "stmpc_td3_base", "stmpc_td3_set_params", "stmpc_td3_get_params", "stmpc_td3_set_state", "stmpc_td3_get_state",
    "stmpc_td3_update_device", "stmpc_td3_grads_device", "stmpc_td3_targets_device", "stmpc_td3_stats_device", "stmpc_td3_noise",
    "stmpc_pop_td3_create", "stmpc_pop_td3_destroy", "stmpc_pop_td3_size", "stmpc_pop_td3_member", "stmpc_pop_td3_act_device",
    "stmpc_pop_td3_push_device", "stmpc_pop_td3_update_device", "stmpc_pop_td3_stats_device",
    "stmpc_per_enable", "stmpc_per_tree_read", "stmpc_per_last_device", "stmpc_per_sample_index",
    "stmpc_pop_per_enable_ddpg", "stmpc_pop_per_enable_td3",
    "stmpc_dqn_create", "stmpc_dqn_destroy", "stmpc_dqn_set_params", "stmpc_dqn_get_params", "stmpc_dqn_set_state", "stmpc_dqn_get_state",
    "stmpc_dqn_push_device", "stmpc_dqn_act_device", "stmpc_dqn_update_device", "stmpc_dqn_grads_device", "stmpc_dqn_targets_device",
    "stmpc_dqn_gather_device", "stmpc_dqn_stats_device", "stmpc_dqn_per_enable", "stmpc_dqn_per_tree_read", "stmpc_dqn_per_last_device",
    "stmpc_dqn_padded_read",
    "stmpc_c51_create", "stmpc_c51_destroy", "stmpc_c51_set_params", "stmpc_c51_get_params", "stmpc_c51_set_state", "stmpc_c51_get_state",
    "stmpc_c51_push_device", "stmpc_c51_act_device", "stmpc_c51_update_device", "stmpc_c51_grads_device", "stmpc_c51_targets_device",
    "stmpc_c51_dist_device", "stmpc_c51_project_device", "stmpc_c51_gather_device", "stmpc_c51_stats_device", "stmpc_c51_per_enable",
    "stmpc_c51_per_tree_read", "stmpc_c51_per_last_device", "stmpc_c51_multi_step_enable", "stmpc_c51_replay_read", "stmpc_c51_dzout_read", "stmpc_c51_padded_read",
    "stmpc_noisy_c51_enable", "stmpc_noisy_c51_set_params", "stmpc_noisy_c51_get_params", "stmpc_noisy_c51_act_device", "stmpc_noisy_c51_debug_read",
    "stmpc_pop_noisy_c51_enable", "stmpc_pop_noisy_c51_act_device",
    "stmpc_pop_dqn_create", "stmpc_pop_dqn_destroy", "stmpc_pop_dqn_size", "stmpc_pop_dqn_member", "stmpc_pop_dqn_act_device",
    "stmpc_pop_dqn_push_device", "stmpc_pop_dqn_update_device", "stmpc_pop_dqn_stats_device", "stmpc_pop_dqn_per_enable", "stmpc_pop_dqn_replay_read",
    "stmpc_pop_c51_create", "stmpc_pop_c51_destroy", "stmpc_pop_c51_size", "stmpc_pop_c51_member", "stmpc_pop_c51_act_device",
    "stmpc_pop_c51_push_device", "stmpc_pop_c51_update_device", "stmpc_pop_c51_stats_device", "stmpc_pop_c51_per_enable",
    "stmpc_pop_c51_multi_step_enable", "stmpc_pop_c51_replay_read", "stmpc_pop_c51_multi_step_window",
    "stmpc_nstep_enable_ddpg", "stmpc_nstep_enable_dqn", "stmpc_pop_nstep_enable_ddpg", "stmpc_pop_nstep_enable_td3", "stmpc_pop_nstep_enable_dqn",
    "stmpc_nstep_window_ddpg", "stmpc_nstep_window_dqn",
    "stmpc_qactor_create", "stmpc_qactor_view_dqn", "stmpc_qactor_destroy", "stmpc_qactor_set_limits", "stmpc_qactor_eval_device",
    "stmpc_pop_qactor_create", "stmpc_pop_qactor_destroy", "stmpc_pop_qactor_size", "stmpc_pop_qactor_eval_device",
    "stmpc_c51actor_create", "stmpc_c51actor_view", "stmpc_dueling_c51actor_create", "stmpc_pop_c51actor_create",
    "stmpc_combined_groups_set", "stmpc_combined_groups_clear", "stmpc_rollout_step_groups_device", "stmpc_combined_decide_groups_device",
    "stmpc_rec_create", "stmpc_rec_destroy", "stmpc_rec_reset", "stmpc_rec_tick_device", "stmpc_rec_reduce_device", "stmpc_rec_read",
    "stmpc_first_step_device", "stmpc_first_step", "stmpc_first_step_counts", "stmpc_speed_from_jerk_device",
    "stmpc_solve_batch_groups_device", "stmpc_solve_batch_groups", "stmpc_st_control_groups_device", "stmpc_solver_groups_sim_step_device",
    "stmpc_solver_groups_sim_init_device",
    "stmpc_reward_groups_env_reset_device", "stmpc_reward_groups_env_step_device", "stmpc_reward_groups_env_reward_device", "stmpc_reward_groups_split",
    "stmpc_shield_env_reset_device", "stmpc_shield_env_step_device",
    "stmpc_traffic_mix_env_reset_device", "stmpc_traffic_mix_env_step_device", "stmpc_traffic_mix_draw",
    "stmpc_cshield_env_reset_device", "stmpc_cshield_env_step_device", "stmpc_cshield_env_evals_device",
    "stmpc_qshield_env_reset_device", "stmpc_qshield_env_step_device",
    "stmpc_shield_traffic_groups_env_reset_device", "stmpc_shield_traffic_groups_env_step_device",
    "stmpc_shield_reward_groups_env_reset_device", "stmpc_shield_reward_groups_env_step_device",
    "stmpc_shield_traffic_mix_env_reset_device", "stmpc_shield_traffic_mix_env_step_device",
)
SIM_NACC = 12        # STMPC_SIM_NACC
ENV_CONTINUOUS_JERK, ENV_JERK, ENV_ACCELERATION = 0, 1, 2                                 # STMPC_ENV_*
REWARD_CONTINUOUS, REWARD_SLOTTED, REWARD_SLOTTED_JERK, REWARD_ST = 0, 1, 2, 3             # STMPC_REWARD_*
ENV_NSTAT, ENV_LOG_COLS = 15, 17      # STMPC_ENV_NSTAT, STMPC_ENV_LOG_COLS
DDPG_ROW, DDPG_NCOUNTERS = 68, 8      # STMPC_DDPG_ROW, STMPC_DDPG_NCOUNTERS
DDPG_POP_MAX = 64                     # STMPC_DDPG_POP_MAX
TD3_POP_MAX = 64                      # STMPC_TD3_POP_MAX
DQN_POP_MAX = 64                      # STMPC_DQN_POP_MAX
C51_POP_MAX = 64                      # STMPC_C51_POP_MAX
SIM_GROUPS_MAX = 64                   # STMPC_SIM_GROUPS_MAX
SOLVER_GROUPS_MAX = 512               # STMPC_SOLVER_GROUPS_MAX
ENV_REWARD_GROUPS_MAX = 64            # STMPC_ENV_REWARD_GROUPS_MAX
TRAFFIC_MIX_MAX = 64                  # STMPC_TRAFFIC_MIX_MAX
TD3_SLOTS = ("critic2", "critic2_target", "critic2_m", "critic2_v")     # STMPC_TD3_CRITIC2 ... STMPC_TD3_CRITIC2_V
DQN_SLOTS = ("q", "q_target", "q_m", "q_v")     # STMPC_DQN_Q ... STMPC_DQN_Q_V
DQN_GRAD = 4                          # STMPC_DQN_GRAD: the gradient, for dqn_padded_read
C51_SLOTS = DQN_SLOTS                 # STMPC_C51_Q ... STMPC_C51_Q_V
C51_GRAD = 4                          # STMPC_C51_GRAD: the gradient, for c51_padded_read
C51_MAX_LOGITS = 1024                 # STMPC_C51_MAX_LOGITS
NOISY_SLOTS = ("sigma", "sigma_target", "sigma_m", "sigma_v")      # STMPC_NOISY_SIGMA ... STMPC_NOISY_SIGMA_V
NOISY_F = {"online": 0, "target": 1, "act": 2}                      # STMPC_NOISY_F_ONLINE ...; + 3: STMPC_NOISY_WEFF_*, + 6: STMPC_NOISY_WEFF_PADDED_*
NOISY_DRAWS = 5                       # the counters' slot of a noisy C51 learner's acting draws
NSTEP_MAX = 16                        # STMPC_NSTEP_MAX
DONE_COL = 67                         # the replay row's done column (terminated || truncated) on a learner with n_step > 1
DQN_ACTION_COL = 66                   # the replay row's action column of a DQN learner
QACTOR_MODES = {"jerk": 0, "acceleration": 1}      # STMPC_QACTOR_JERK, STMPC_QACTOR_ACCELERATION
DDPG_SLOTS = ("actor", "actor_target", "actor_m", "actor_v", "critic", "critic_target", "critic_m", "critic_v")     # STMPC_DDPG_ACTOR ... STMPC_DDPG_CRITIC_V
REC_HDR, REC_NQ, REC_MAX_DEPTH, REC_MAX_EDGES = 10, 4, 64, 32      # STMPC_REC_HDR, STMPC_REC_NQ, STMPC_REC_MAX_DEPTH, STMPC_REC_MAX_EDGES
REC_COLUMNS = ("tick", "x", "y", "v", "a", "s", "k", "cmd", "takeover", "jerk")      # the first STMPC_REC_HDR columns of a record
REC_QUANTITIES = ("count", "takeover_count", "sum_abs_jerk", "sum_abs_speed")        # the STMPC_REC_NQ binned quantities, in row order
ABI_VERSION = 8     # STMPC_ABI_VERSION of include/stmpc.h this binding was written against

QP_NMAX = 64        # STMPC_QP_NMAX
QP_MAXITERS = 10    # STMPC_QP_MAXITERS (solvers.options['maxiters'], st.py:17)


def lib_path():
    # STMPC_LIB selects another build of the same ABI (A/B measurements of kernel variants)
    return os.environ.get("STMPC_LIB") or _build.LIB_PATH


def load():
    """Load ``libstmpc.so`` (must have been built in-tree: ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and must be the first to load it, otherwise the
    # system copy this library links against initialises the device and torch then reports "No HIP GPUs are available"
    # (and device pointers could not be shared).  With torch imported first the loader resolves this library's
    # libamdhip64 dependency to the copy torch already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(this package has no CPU fallback)" % path)
    lib = C.CDLL(path)
    have = lib.stmpc_abi_version() if hasattr(lib, "stmpc_abi_version") else 0
    if have != ABI_VERSION:
        raise ImportError("%s implements ABI %d, this binding expects %d: rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)"
                          % (path, have, ABI_VERSION))
    dp, ip, u8p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
    pp = C.POINTER(Params)
    lib.stmpc_backend_info.restype = C.c_char_p
    lib.stmpc_last_error.restype = C.c_char_p
    lib.stmpc_create.argtypes = [C.POINTER(vp), C.c_int]
    lib.stmpc_destroy.argtypes = [vp]
    lib.stmpc_destroy.restype = None
    lib.stmpc_ego_s.argtypes = [C.c_double, C.c_double]
    lib.stmpc_ego_s.restype = C.c_double
    lib.stmpc_num_s.argtypes = [pp, C.c_double]
    lib.stmpc_num_t.argtypes = [pp]
    lib.stmpc_path_mean_abs_jerk.argtypes = [dp, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.stmpc_path_mean_abs_jerk.restype = C.c_double
    lib.stmpc_fastdiv2_check.argtypes = [C.c_double, C.POINTER(C.c_double)]
    lib.stmpc_solve_batch_device.argtypes = [vp, pp, C.c_int, C.c_int] + [vp] * 9 + [vp]
    lib.stmpc_solve_batch_device_ac.argtypes = [vp, pp, C.c_int, C.c_int] + [vp] * 10 + [vp]
    lib.stmpc_solve_batch.argtypes = [vp, pp, C.c_int, C.c_int, dp, ip, dp, dp, ip, ip, dp, dp, ip]
    lib.stmpc_get_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.stmpc_solve_batch_groups_device.argtypes = [vp, pp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 10 + [vp]
    lib.stmpc_solve_batch_groups.argtypes = [vp, pp, C.c_int, C.c_int, C.c_int, C.c_int, dp, ip, dp, dp, ip, ip, dp, dp, ip, dp]
    lib.stmpc_st_control_groups_device.argtypes = [vp, pp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int] + [vp] * 10 + [vp]
    lib.stmpc_solver_groups_sim_step_device.argtypes = [vp, pp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.stmpc_solver_groups_sim_init_device.argtypes = [vp, C.POINTER(SimCfg), C.c_int, C.c_int, vp]
    lib.stmpc_solve_grid.argtypes = [vp, u8p, dp, C.c_int, dp, C.c_int, C.c_double, C.c_double, dp] + [C.c_double] * 11 + [dp]
    lib.stmpc_solve_grid_no_jerk.argtypes = [vp, C.c_int, u8p, dp, C.c_int, dp, C.c_int, C.c_double, dp, dp]
    lib.stmpc_build_grid.argtypes = [vp, pp, dp, C.c_int, dp, dp, u8p, dp, dp, dp]
    lib.stmpc_predict_batch.argtypes = [vp, pp, C.c_int, C.c_int, C.c_int, dp, ip, dp, dp, dp, C.c_double, C.c_double,
                                        dp, dp, dp, ip]
    lib.stmpc_predict_batch_acc.argtypes = [vp, pp, C.c_int, C.c_int, C.c_int, dp, ip, dp, dp, dp, C.c_double, C.c_double,
                                            dp, dp, dp, ip, dp]
    lib.stmpc_check_error.argtypes = [vp]
    lib.stmpc_sim_status_device.argtypes = [vp, C.c_int, vp, vp]
    cp = C.POINTER(CombinedCfg)
    lib.stmpc_rollout_step_device.argtypes = [vp, pp, cp, C.c_int, C.c_int, C.c_int] + [vp] * 7 + [vp]
    lib.stmpc_combined_decide_device.argtypes = [vp, pp, cp, C.c_int, C.c_int] + [vp] * 12 + [vp]
    lib.stmpc_combined_groups_set.argtypes = [vp, pp, cp, C.c_int, C.c_int]
    lib.stmpc_combined_groups_clear.argtypes = [vp]
    lib.stmpc_rollout_step_groups_device.argtypes = [vp, pp, C.c_int, C.c_int, C.c_int] + [vp] * 7 + [vp]
    lib.stmpc_combined_decide_groups_device.argtypes = [vp, pp, C.c_int, C.c_int] + [vp] * 12 + [vp]
    sp = C.POINTER(SimCfg)
    lib.stmpc_policy_features_len.argtypes = [C.POINTER(FeaturesCfg)]
    lib.stmpc_policy_features_device.argtypes = [vp, C.POINTER(FeaturesCfg), C.c_int, C.c_int, C.c_int] + [vp] * 7 + [C.c_int, vp]
    fp = C.POINTER(C.c_float)
    lib.stmpc_actor_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, C.c_double, C.c_double, C.POINTER(vp)]
    lib.stmpc_actor_destroy.argtypes = [vp]
    lib.stmpc_actor_destroy.restype = None
    lib.stmpc_actor_eval_device.argtypes = [vp, vp, C.POINTER(FeaturesCfg), C.c_int, C.c_int, C.c_int] + [vp] * 7 + [C.c_int, vp, vp]
    lib.stmpc_combined_counts.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
    lib.stmpc_sim_init_device.argtypes = [vp, sp, C.c_int, vp]
    lib.stmpc_sim_view_device.argtypes = [vp, sp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.stmpc_sim_step_device.argtypes = [vp, pp, sp, C.c_int, vp, vp]
    lib.stmpc_sim_read.argtypes = [vp, C.c_int, ip, ip, dp, dp]
    lib.stmpc_combined_read_state.argtypes = [vp, C.c_int, ip, ip, ip, dp, dp, ip, dp, dp, dp, ip, dp, dp, ip]
    lib.stmpc_probe_arith.argtypes = [vp, C.c_int, dp, dp, dp, C.c_int]
    lib.stmpc_profile.argtypes = [vp, C.c_int, C.POINTER(ProfileTotals)]
    lib.stmpc_finer_fit_batch.argtypes = [vp, pp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, dp, ip, dp, dp, dp,
                                          C.c_int, dp, ip, ip]
    lib.stmpc_st_control_batch.argtypes = [vp, pp, C.c_double, C.c_int, C.c_int, dp, ip, dp, dp, dp, ip, ip, dp, dp, ip]
    ep = C.POINTER(EnvCfg)
    lib.stmpc_env_reset_device.argtypes = [vp, pp, sp, ep, C.c_int, vp, C.c_int, vp]
    lib.stmpc_env_step_device.argtypes = [vp, pp, sp, ep, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.stmpc_env_reward_device.argtypes = [vp, ep, C.c_int, C.c_int] + [vp] * 9 + [vp]
    lib.stmpc_env_drain.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.stmpc_env_episode_ticks_device.argtypes = [vp, C.c_int, vp, vp]
    lib.stmpc_sim_init_groups_device.argtypes = [vp, sp, C.c_int, C.c_int, vp]
    lib.stmpc_sim_step_groups_device.argtypes = [vp, pp, C.c_int, vp, vp]
    lib.stmpc_sim_groups.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.stmpc_env_reset_groups_device.argtypes = [vp, pp, sp, C.c_int, C.c_int, ep, vp, C.c_int, vp]
    lib.stmpc_env_step_groups_device.argtypes = [vp, pp, ep, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.stmpc_reward_groups_env_reset_device.argtypes = [vp, pp, sp, C.c_int, C.c_int, ep, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.stmpc_reward_groups_env_step_device.argtypes = [vp, pp, ep, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.stmpc_reward_groups_env_reward_device.argtypes = [vp, ep, C.c_int, C.c_int] + [vp] * 9 + [vp]
    lib.stmpc_reward_groups_split.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.stmpc_env_episode_seed.argtypes = [C.c_uint64, C.c_uint32]
    lib.stmpc_env_episode_seed.restype = C.c_uint64
    lib.stmpc_st_control_batch_device.argtypes = [vp, pp, C.c_double, C.c_int, C.c_int] + [vp] * 10 + [vp]
    i64p, u32p = C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    lib.stmpc_ddpg_create.argtypes = [vp, C.POINTER(DDPGCfg), C.POINTER(vp)]
    lib.stmpc_ddpg_destroy.argtypes = [vp]
    lib.stmpc_ddpg_destroy.restype = None
    lib.stmpc_ddpg_set_params.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_ddpg_get_params.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_ddpg_set_state.argtypes = [vp, i64p, fp]
    lib.stmpc_ddpg_get_state.argtypes = [vp, i64p, fp]
    lib.stmpc_ddpg_push_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 6 + [vp]
    lib.stmpc_ddpg_act_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    lib.stmpc_ddpg_update_device.argtypes = [vp, C.c_int, C.c_double, C.c_double, vp]
    lib.stmpc_ddpg_grads_device.argtypes = [vp, vp, vp, vp]
    lib.stmpc_ddpg_stats_device.argtypes = [vp, vp, vp]
    lib.stmpc_ddpg_replay_read.argtypes = [vp, C.c_int64, C.c_int64, fp]
    lib.stmpc_ddpg_gather_device.argtypes = [vp, vp, vp]
    lib.stmpc_ddpg_sample_index.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64]
    lib.stmpc_ddpg_sample_index.restype = C.c_uint64
    lib.stmpc_ddpg_noise.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, u32p, u32p]
    lib.stmpc_ddpg_noise.restype = C.c_double
    lib.stmpc_ddpg_pop_create.argtypes = [vp, C.POINTER(DDPGCfg), C.c_int, C.POINTER(vp)]
    lib.stmpc_ddpg_pop_destroy.argtypes = [vp]
    lib.stmpc_ddpg_pop_destroy.restype = None
    lib.stmpc_ddpg_pop_size.argtypes = [vp]
    lib.stmpc_ddpg_pop_member.argtypes = [vp, C.c_int]
    lib.stmpc_ddpg_pop_member.restype = vp
    lib.stmpc_ddpg_pop_act_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    lib.stmpc_ddpg_pop_push_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 6 + [vp]
    lib.stmpc_ddpg_pop_update_device.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, vp]
    lib.stmpc_ddpg_pop_stats_device.argtypes = [vp, vp, vp]
    lib.stmpc_td3_create.argtypes = [vp, C.POINTER(TD3Cfg), C.POINTER(vp)]
    lib.stmpc_td3_destroy.argtypes = [vp]
    lib.stmpc_td3_destroy.restype = None
    lib.stmpc_td3_base.argtypes = [vp]
    lib.stmpc_td3_base.restype = vp
    lib.stmpc_td3_set_params.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_td3_get_params.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_td3_set_state.argtypes = [vp, fp]
    lib.stmpc_td3_get_state.argtypes = [vp, fp]
    lib.stmpc_td3_update_device.argtypes = [vp, C.c_int, C.c_double, C.c_double, vp]
    lib.stmpc_td3_grads_device.argtypes = [vp, vp, vp, vp, vp]
    lib.stmpc_td3_targets_device.argtypes = [vp, vp, vp]
    lib.stmpc_td3_stats_device.argtypes = [vp, vp, vp]
    lib.stmpc_td3_noise.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, u32p, u32p]
    lib.stmpc_td3_noise.restype = C.c_double
    lib.stmpc_pop_td3_create.argtypes = [vp, C.POINTER(TD3Cfg), C.c_int, C.POINTER(vp)]
    lib.stmpc_pop_td3_destroy.argtypes = [vp]
    lib.stmpc_pop_td3_destroy.restype = None
    lib.stmpc_pop_td3_size.argtypes = [vp]
    lib.stmpc_pop_td3_member.argtypes = [vp, C.c_int]
    lib.stmpc_pop_td3_member.restype = vp
    lib.stmpc_pop_td3_act_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    lib.stmpc_pop_td3_push_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 6 + [vp]
    lib.stmpc_pop_td3_update_device.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, vp]
    lib.stmpc_pop_td3_stats_device.argtypes = [vp, vp, vp]
    lib.stmpc_per_enable.argtypes = [vp, C.POINTER(PERCfg)]
    lib.stmpc_per_tree_read.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(C.c_double)]
    lib.stmpc_per_last_device.argtypes = [vp, vp, vp, vp, vp]
    lib.stmpc_per_sample_index.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint32]
    lib.stmpc_per_sample_index.restype = C.c_int64
    lib.stmpc_pop_per_enable_ddpg.argtypes = [vp, C.POINTER(PERCfg), C.POINTER(C.c_uint8), C.c_int]
    lib.stmpc_pop_per_enable_td3.argtypes = [vp, C.POINTER(PERCfg), C.POINTER(C.c_uint8), C.c_int]
    lib.stmpc_dqn_create.argtypes = [vp, C.POINTER(DQNCfg), C.POINTER(vp)]
    lib.stmpc_dqn_destroy.argtypes = [vp]
    lib.stmpc_dqn_destroy.restype = None
    lib.stmpc_dqn_set_params.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_dqn_get_params.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_dqn_set_state.argtypes = [vp, i64p, fp]
    lib.stmpc_dqn_get_state.argtypes = [vp, i64p, fp]
    lib.stmpc_dqn_push_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 4 + [vp]
    lib.stmpc_dqn_act_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double, vp, vp, vp]
    lib.stmpc_dqn_update_device.argtypes = [vp, C.c_int, C.c_double, vp]
    lib.stmpc_dqn_grads_device.argtypes = [vp, vp, vp]
    lib.stmpc_dqn_targets_device.argtypes = [vp, vp, vp]
    lib.stmpc_dqn_gather_device.argtypes = [vp, vp, vp]
    lib.stmpc_dqn_stats_device.argtypes = [vp, vp, vp]
    lib.stmpc_dqn_per_enable.argtypes = [vp, C.POINTER(PERCfg)]
    lib.stmpc_dqn_per_tree_read.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(C.c_double)]
    lib.stmpc_dqn_per_last_device.argtypes = [vp, vp, vp, vp, vp]
    lib.stmpc_dqn_padded_read.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_c51_create.argtypes = [vp, C.POINTER(C51Cfg), C.POINTER(vp)]
    lib.stmpc_c51_destroy.argtypes = [vp]
    lib.stmpc_c51_destroy.restype = None
    for name in ("set_params", "get_params", "set_state", "get_state", "push_device", "act_device", "update_device", "grads_device", "targets_device",
                 "gather_device", "stats_device", "per_enable", "per_tree_read", "per_last_device", "padded_read"):       # the DQN learner's signatures
        getattr(lib, "stmpc_c51_" + name).argtypes = list(getattr(lib, "stmpc_dqn_" + name).argtypes)
    lib.stmpc_c51_dist_device.argtypes = [vp, vp, vp, vp]
    lib.stmpc_c51_project_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.stmpc_c51_multi_step_enable.argtypes = [vp, C.POINTER(NStepCfg)]
    lib.stmpc_c51_replay_read.argtypes = [vp, C.c_int64, C.c_int64, fp]
    lib.stmpc_c51_dzout_read.argtypes = [vp, fp, C.c_int64]
    lib.stmpc_noisy_c51_enable.argtypes = [vp, C.POINTER(NoisyCfg)]
    lib.stmpc_noisy_c51_set_params.argtypes = list(lib.stmpc_c51_set_params.argtypes)
    lib.stmpc_noisy_c51_get_params.argtypes = list(lib.stmpc_c51_get_params.argtypes)
    lib.stmpc_noisy_c51_act_device.argtypes = list(lib.stmpc_c51_act_device.argtypes)
    lib.stmpc_noisy_c51_debug_read.argtypes = [vp, C.c_int, fp, C.c_int64]
    lib.stmpc_pop_noisy_c51_enable.argtypes = [vp, C.POINTER(NoisyCfg), C.c_int]
    lib.stmpc_pop_noisy_c51_act_device.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_double), C.c_int, vp, vp, vp]
    lib.stmpc_pop_dqn_create.argtypes = [vp, C.POINTER(DQNCfg), C.c_int, C.POINTER(vp)]
    lib.stmpc_pop_dqn_destroy.argtypes = [vp]
    lib.stmpc_pop_dqn_destroy.restype = None
    lib.stmpc_pop_dqn_size.argtypes = [vp]
    lib.stmpc_pop_dqn_member.argtypes = [vp, C.c_int]
    lib.stmpc_pop_dqn_member.restype = vp
    lib.stmpc_pop_dqn_act_device.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_double), C.c_int, vp, vp, vp]
    lib.stmpc_pop_dqn_push_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 4 + [vp]
    lib.stmpc_pop_dqn_update_device.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_int, vp]
    lib.stmpc_pop_dqn_stats_device.argtypes = [vp, vp, vp]
    lib.stmpc_pop_dqn_per_enable.argtypes = [vp, C.POINTER(PERCfg), C.POINTER(C.c_uint8), C.c_int]
    lib.stmpc_pop_dqn_replay_read.argtypes = [vp, C.c_int64, C.c_int64, fp]
    lib.stmpc_pop_c51_create.argtypes = [vp, C.POINTER(C51Cfg), C.c_int, C.POINTER(vp)]
    lib.stmpc_pop_c51_destroy.argtypes = [vp]
    lib.stmpc_pop_c51_destroy.restype = None
    lib.stmpc_pop_c51_size.argtypes = [vp]
    lib.stmpc_pop_c51_member.argtypes = [vp, C.c_int]
    lib.stmpc_pop_c51_member.restype = vp
    lib.stmpc_pop_c51_act_device.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_double), C.c_int, vp, vp, vp]
    lib.stmpc_pop_c51_push_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 4 + [vp]
    lib.stmpc_pop_c51_update_device.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_int, vp]
    lib.stmpc_pop_c51_stats_device.argtypes = [vp, vp, vp]
    lib.stmpc_pop_c51_per_enable.argtypes = [vp, C.POINTER(PERCfg), C.POINTER(C.c_uint8), C.c_int]
    lib.stmpc_pop_c51_multi_step_enable.argtypes = [vp, C.POINTER(NStepCfg), C.c_int]
    lib.stmpc_pop_c51_replay_read.argtypes = [vp, C.c_int64, C.c_int64, fp]
    lib.stmpc_pop_c51_multi_step_window.argtypes = [vp, i64p, C.c_int, dp]
    for name in ("stmpc_nstep_enable_ddpg", "stmpc_nstep_enable_dqn"):
        getattr(lib, name).argtypes = [vp, C.POINTER(NStepCfg)]
    for name in ("stmpc_pop_nstep_enable_ddpg", "stmpc_pop_nstep_enable_td3", "stmpc_pop_nstep_enable_dqn"):
        getattr(lib, name).argtypes = [vp, C.POINTER(NStepCfg), C.c_int]
    for name in ("stmpc_nstep_window_ddpg", "stmpc_nstep_window_dqn"):
        getattr(lib, name).argtypes = [vp, i64p, C.c_int, dp]
    lib.stmpc_qactor_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, dp, C.c_int, C.POINTER(vp)]
    lib.stmpc_qactor_view_dqn.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.stmpc_c51actor_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, fp, fp, fp, fp, dp, C.c_int, C.POINTER(vp)]
    lib.stmpc_dueling_c51actor_create.argtypes = list(lib.stmpc_c51actor_create.argtypes)
    lib.stmpc_c51actor_view.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.stmpc_qactor_destroy.argtypes = [vp]
    lib.stmpc_qactor_destroy.restype = None
    lib.stmpc_qactor_set_limits.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    lib.stmpc_qactor_eval_device.argtypes = [vp, vp, C.POINTER(FeaturesCfg), C.c_int, C.c_int, C.c_int] + [vp] * 6 + [C.c_int, vp, vp, vp, vp]
    lib.stmpc_pop_qactor_create.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp)]
    lib.stmpc_pop_qactor_destroy.argtypes = [vp]
    lib.stmpc_pop_qactor_destroy.restype = None
    lib.stmpc_pop_qactor_size.argtypes = [vp]
    lib.stmpc_pop_qactor_eval_device.argtypes = list(lib.stmpc_qactor_eval_device.argtypes)
    lib.stmpc_pop_c51actor_create.argtypes = list(lib.stmpc_pop_qactor_create.argtypes)
    lib.stmpc_actor_view_ddpg.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.stmpc_actor_pop_create.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp)]
    lib.stmpc_actor_pop_destroy.argtypes = [vp]
    lib.stmpc_actor_pop_destroy.restype = None
    lib.stmpc_actor_pop_size.argtypes = [vp]
    lib.stmpc_actor_pop_eval_device.argtypes = [vp, vp, C.POINTER(FeaturesCfg), C.c_int, C.c_int, C.c_int] + [vp] * 7 + [C.c_int, vp, vp]
    lib.stmpc_rec_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, dp, C.c_int, C.POINTER(vp)]
    lib.stmpc_rec_destroy.argtypes = [vp]
    lib.stmpc_rec_destroy.restype = None
    lib.stmpc_rec_reset.argtypes = [vp, vp]
    lib.stmpc_rec_tick_device.argtypes = [vp, C.c_int, C.c_int] + [vp] * 7 + [vp]
    lib.stmpc_rec_reduce_device.argtypes = [vp, vp, vp]
    lib.stmpc_rec_read.argtypes = [vp, dp, ip, dp, dp, ip]
    fsp = C.POINTER(FirstStepCfg)
    lib.stmpc_first_step_device.argtypes = [vp, pp, fsp, C.c_int, C.c_int] + [vp] * 9 + [vp]
    lib.stmpc_first_step.argtypes = [vp, pp, fsp, C.c_int, C.c_int, dp, ip, dp, dp, dp, dp, ip, ip, ip, ip, dp, dp, dp]
    lib.stmpc_first_step_counts.argtypes = [vp, i64p, i64p, i64p, C.c_int]
    lib.stmpc_speed_from_jerk_device.argtypes = [vp, pp, C.c_double, C.c_int, vp, vp, vp, vp]
    shp = C.POINTER(ShieldEnvCfg)
    lib.stmpc_shield_env_reset_device.argtypes = [vp, pp, sp, ep, shp, C.c_int, vp, C.c_int, vp]
    lib.stmpc_shield_env_step_device.argtypes = [vp, pp, sp, ep, shp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.stmpc_traffic_mix_env_reset_device.argtypes = [vp, pp, sp, C.c_int, dp, C.c_uint64, ep, C.c_int, vp, C.c_int, vp, vp]
    lib.stmpc_traffic_mix_env_step_device.argtypes = [vp, pp, ep, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.stmpc_traffic_mix_draw.argtypes = [C.c_uint64, C.c_int, C.c_uint32, dp, C.c_int]
    csp = C.POINTER(CShieldEnvCfg)
    lib.stmpc_cshield_env_reset_device.argtypes = [vp, pp, sp, ep, csp, vp, C.c_int, vp, C.c_int, vp]
    lib.stmpc_cshield_env_step_device.argtypes = [vp, pp, sp, ep, csp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.stmpc_cshield_env_evals_device.argtypes = [vp, C.c_int, vp, vp]
    qsp = C.POINTER(QShieldEnvCfg)
    lib.stmpc_qshield_env_reset_device.argtypes = [vp, pp, sp, ep, qsp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.stmpc_qshield_env_step_device.argtypes = [vp, pp, sp, ep, qsp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int] + [vp] * 10
    shield_step = [vp, pp, ep, shp, C.c_int, vp, vp, C.c_int] + [vp] * 10         # ctx ... N, d_action, d_obs, obs_stride, the step's and the shield's outputs
    lib.stmpc_shield_traffic_groups_env_reset_device.argtypes = [vp, pp, sp, C.c_int, C.c_int, ep, shp, dp, C.c_int, vp, C.c_int, vp]
    lib.stmpc_shield_traffic_groups_env_step_device.argtypes = shield_step + [vp]
    lib.stmpc_shield_reward_groups_env_reset_device.argtypes = [vp, pp, sp, C.c_int, C.c_int, ep, C.c_int, C.c_int, shp, dp, C.c_int, vp, C.c_int, vp]
    lib.stmpc_shield_reward_groups_env_step_device.argtypes = shield_step + [vp]
    lib.stmpc_shield_traffic_mix_env_reset_device.argtypes = [vp, pp, sp, C.c_int, dp, C.c_uint64, ep, shp, C.c_int, vp, C.c_int, vp, vp]
    lib.stmpc_shield_traffic_mix_env_step_device.argtypes = shield_step + [vp, vp, vp]
    _lib = lib
    return lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _u8ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _batch_states(ego, k_count, other_x, other_v):
    """Host batch entries' states as contiguous arrays: ``(ego[N,5], k_count[N], other_x[N,Kmax], other_v[N,Kmax], N, Kmax)``, Kmax from ``other_x``."""
    ego = np.ascontiguousarray(ego, dtype=np.float64)
    k_count = np.ascontiguousarray(k_count, dtype=np.int32)
    N = ego.shape[0]
    if ego.ndim != 2 or ego.shape[1] != 5:
        raise ValueError("ego must be [N,5] (x, y, v, a, start_s)")
    other_x = np.ascontiguousarray(other_x, dtype=np.float64)
    other_v = np.ascontiguousarray(other_v, dtype=np.float64)
    Kmax = other_x.shape[1] if other_x.ndim == 2 else (other_x.size // N if N else 0)
    return ego, k_count, other_x.reshape(N, Kmax), other_v.reshape(N, Kmax), N, Kmax


def ego_s(x, y):
    """control.get_ego_s evaluated by the library's host helper (same libm as CPython)."""
    return load().stmpc_ego_s(float(x), float(y))


def num_s(params, start_s):
    return load().stmpc_num_s(C.byref(params), float(start_s))


def num_t(params):
    return load().stmpc_num_t(C.byref(params))


def path_mean_abs_jerk(seq, v0, a0, dt):
    return load().stmpc_path_mean_abs_jerk(_dptr(seq), int(seq.size), float(v0), float(a0), float(dt))


def fastdiv2_check(d):
    """(ok, zl): whether the solver may form x / d as fma(x, RN(1/d), x * zl) -- the check it applies to dt, dt**2, dt**3."""
    zl = C.c_double(0.0)
    ok = load().stmpc_fastdiv2_check(float(d), C.byref(zl))
    return bool(ok), zl.value


def ddpg_sample_index(seed, update, row, fill):
    """``stmpc_ddpg_sample_index``: the ring row minibatch row ``row`` of update ``update`` reads (host only)."""
    return int(load().stmpc_ddpg_sample_index(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(update)), C.c_uint32(int(row)), C.c_uint64(int(fill))))


def ddpg_noise(seed, call, row):
    """``stmpc_ddpg_noise``: (standard normal in fp64, draw 1, draw 2) of row ``row`` in noisy acting call ``call`` (host only)."""
    u1, u2 = C.c_uint32(0), C.c_uint32(0)
    g = load().stmpc_ddpg_noise(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(call)), C.c_uint32(int(row)), C.byref(u1), C.byref(u2))
    return float(g), int(u1.value), int(u2.value)


def per_sample_index(tree, leaves, fill, seed, update, row):
    """``stmpc_per_sample_index``: the ring row minibatch row ``row`` of update ``update`` reads from the sum tree ``tree`` (fp64 [2 * leaves - 1]; host only)."""
    tree = np.ascontiguousarray(tree, dtype=np.float64)
    assert tree.size == 2 * int(leaves) - 1
    return int(load().stmpc_per_sample_index(tree.ctypes.data_as(C.POINTER(C.c_double)), int(leaves), int(fill), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                             C.c_uint64(int(update)), C.c_uint32(int(row))))


def td3_noise(seed, update, row):
    """``stmpc_td3_noise``: (standard normal in fp64, draw 1, draw 2) of minibatch row ``row`` of update ``update``'s target smoothing (host only)."""
    u1, u2 = C.c_uint32(0), C.c_uint32(0)
    g = load().stmpc_td3_noise(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(update)), C.c_uint32(int(row)), C.byref(u1), C.byref(u2))
    return float(g), int(u1.value), int(u2.value)


def env_episode_seed(seed, episode):
    """``stmpc_env_episode_seed``: the seed episode ``episode`` of an environment starts from (host only)."""
    return int(load().stmpc_env_episode_seed(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(episode))))


def traffic_mix_draw(mix_seed, env, episode, cum):
    """``stmpc_traffic_mix_draw``: the traffic type of episode ``episode`` of environment ``env`` under the cumulative weights ``cum`` (host only)."""
    cum = np.ascontiguousarray(cum, dtype=np.float64)
    return int(load().stmpc_traffic_mix_draw(C.c_uint64(int(mix_seed) & 0xFFFFFFFFFFFFFFFF), int(env), C.c_uint32(int(episode)), _dptr(cum), int(cum.size)))


def backend_info():
    return load().stmpc_backend_info().decode()


def library_source_hash():
    """sha256[:16] of the sources the loaded library was built from (``build.source_hash`` at build time), or "unknown"."""
    info = backend_info()
    return info.rsplit("src=", 1)[1].strip() if "src=" in info else "unknown"


class Context:
    """One HIP device + its scratch (``stmpc_ctx``)."""

    def __init__(self, device=-1):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.stmpc_create(C.byref(h), int(device))
        if rc != 0:
            raise StmpcError(rc, self._lib.stmpc_last_error().decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.stmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise StmpcError(rc, self._lib.stmpc_last_error().decode())

    # -- batched solve, host numpy arrays --------------------------------------------------
    def solve_batch(self, params, ego, k_count, other_x, other_v, want_dist=True):
        ego, k_count, other_x, other_v, N, Kmax = _batch_states(ego, k_count, other_x, other_v)
        H = num_t(params)
        path = np.empty((N, H), dtype=np.int32)
        best_t = np.empty(N, dtype=np.int32)
        cost = np.empty(N, dtype=np.float64)
        pdist = np.empty((N, H), dtype=np.float64) if want_dist else None
        crash = np.empty(N, dtype=np.int32) if want_dist else None
        self._chk(self._lib.stmpc_solve_batch(self._h, C.byref(params), N, Kmax, _dptr(ego), _iptr(k_count),
                                              _dptr(other_x) if Kmax else None, _dptr(other_v) if Kmax else None,
                                              _iptr(path), _iptr(best_t), _dptr(cost), _dptr(pdist), _iptr(crash)))
        return path, best_t, cost, pdist, crash

    # -- batched solve, device pointers (ints), asynchronous ---------------------------------
    def solve_batch_device(self, params, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_pd=0, d_crash=0,
                           stream=0, d_action_cost=0):
        """``d_action_cost``: optional fp64 [N][2] device buffer the solver fills with (first-step cell, cost) -- the fused row of the multi-GPU gather."""
        self._chk(self._lib.stmpc_solve_batch_device_ac(self._h, C.byref(params), int(N), int(Kmax), d_ego, d_k, d_ox,
                                                        d_ov, d_path, d_bt, d_cost, d_pd or None, d_crash or None,
                                                        d_action_cost or None, stream or None))

    # -- st.finer_fit, batched (host arrays) ------------------------------------------------------
    def finer_fit_batch(self, params, delta_t, coarse_delta_t, s_seq, lengths, v0, a0, bac=None, maxiters=QP_MAXITERS):
        """Returns ``(out[N, QP_NMAX], out_len[N], iters[N])``; see ``stmpc_finer_fit_batch`` in include/stmpc.h."""
        s_seq = np.ascontiguousarray(s_seq, dtype=np.float64)
        if s_seq.ndim != 2:
            raise ValueError("s_seq must be [N, Hs]")
        N, Hs = s_seq.shape
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        v0 = np.ascontiguousarray(v0, dtype=np.float64)
        a0 = np.ascontiguousarray(a0, dtype=np.float64)
        if bac is not None:
            bac = np.ascontiguousarray(bac, dtype=np.float64).reshape(N, 4)
        out = np.zeros((N, QP_NMAX), dtype=np.float64)
        out_len = np.zeros(N, dtype=np.int32)
        iters = np.zeros(N, dtype=np.int32)
        self._chk(self._lib.stmpc_finer_fit_batch(self._h, C.byref(params), float(delta_t), float(coarse_delta_t),
                                                  int(maxiters), N, Hs, _dptr(s_seq), _iptr(lengths), _dptr(v0), _dptr(a0),
                                                  _dptr(bac), QP_NMAX, _dptr(out), _iptr(out_len), _iptr(iters)))
        return out, out_len, iters

    # -- st.do_st_control, batched (host arrays) ---------------------------------------------------
    def st_control_batch(self, params, tick_length, ego, k_count, other_x, other_v, want_paths=False):
        """Returns a dict: ``speed[N]``, ``best_t[N]`` and, with ``want_paths``, ``path_idx``, ``cost``, ``fine``, ``fine_len``."""
        ego, k_count, other_x, other_v, N, Kmax = _batch_states(ego, k_count, other_x, other_v)
        H = num_t(params)
        speed = np.zeros(N, dtype=np.float64)
        best_t = np.zeros(N, dtype=np.int32)
        path = np.empty((N, H), dtype=np.int32) if want_paths else None
        cost = np.empty(N, dtype=np.float64) if want_paths else None
        fine = np.zeros((N, QP_NMAX), dtype=np.float64) if want_paths else None
        fine_len = np.zeros(N, dtype=np.int32) if want_paths else None
        self._chk(self._lib.stmpc_st_control_batch(self._h, C.byref(params), float(tick_length), N, Kmax, _dptr(ego),
                                                   _iptr(k_count), _dptr(other_x) if Kmax else None,
                                                   _dptr(other_v) if Kmax else None, _dptr(speed), _iptr(best_t),
                                                   _iptr(path), _dptr(cost), _dptr(fine), _iptr(fine_len)))
        res = {"speed": speed, "best_t": best_t}
        if want_paths:
            res.update(path_idx=path, cost=cost, fine=fine, fine_len=fine_len)
        return res

    def st_control_batch_device(self, params, tick_length, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_speed,
                                d_fine=0, d_fine_len=0, stream=0):
        self._chk(self._lib.stmpc_st_control_batch_device(self._h, C.byref(params), float(tick_length), int(N), int(Kmax),
                                                          d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_speed,
                                                          d_fine or None, d_fine_len or None, stream or None))

    # -- solver groups (main.py:43-59): G parameter sets in the launches of one batch ------------------
    def solve_batch_groups(self, groups, n_per_group, ego, k_count, other_x, other_v):
        """``stmpc_solve_batch_groups``: state i is solved under ``groups[i // n_per_group]`` (a ``ParamsTable`` or a sequence of ``Params``).
        Returns a dict with ``path_idx``, ``best_t``, ``cost``, ``path_dist``, ``crash`` and ``action_cost[N, 2]``."""
        t = ParamsTable.of(groups)
        ego, k_count, other_x, other_v, N, Kmax = _batch_states(ego, k_count, other_x, other_v)
        H = max(num_t(t.array[0]), 1) if len(t) else 1        # (an empty or unusable table is refused by the library, not here)
        path, best_t, cost = np.empty((N, H), dtype=np.int32), np.empty(N, dtype=np.int32), np.empty(N, dtype=np.float64)
        pdist, crash, ac = np.empty((N, H), dtype=np.float64), np.empty(N, dtype=np.int32), np.empty((N, 2), dtype=np.float64)
        self._chk(self._lib.stmpc_solve_batch_groups(self._h, t.array, len(t), int(n_per_group), N, Kmax, _dptr(ego), _iptr(k_count),
                                                     _dptr(other_x) if Kmax else None, _dptr(other_v) if Kmax else None,
                                                     _iptr(path), _iptr(best_t), _dptr(cost), _dptr(pdist), _iptr(crash), _dptr(ac)))
        return {"path_idx": path, "best_t": best_t, "cost": cost, "path_dist": pdist, "crash": crash, "action_cost": ac}

    def solve_batch_groups_device(self, groups, n_per_group, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_pd=0, d_crash=0, d_action_cost=0, stream=0):
        t = ParamsTable.of(groups)
        self._chk(self._lib.stmpc_solve_batch_groups_device(self._h, t.array, len(t), int(n_per_group), int(N), int(Kmax), d_ego, d_k, d_ox, d_ov, d_path,
                                                            d_bt, d_cost, d_pd or None, d_crash or None, d_action_cost or None, stream or None))

    def st_control_groups_device(self, groups, n_per_group, tick_length, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_speed, d_fine=0,
                                 d_fine_len=0, stream=0):
        t = ParamsTable.of(groups)
        self._chk(self._lib.stmpc_st_control_groups_device(self._h, t.array, len(t), int(n_per_group), float(tick_length), int(N), int(Kmax), d_ego, d_k,
                                                           d_ox, d_ov, d_path, d_bt, d_cost, d_speed, d_fine or None, d_fine_len or None, stream or None))

    def sim_init_solver_groups(self, cfgs, n_per_group, stream=0):
        """``stmpc_solver_groups_sim_init_device``: ``sim_init_groups`` for up to ``SOLVER_GROUPS_MAX`` cells, one traffic group per cell."""
        t = SimCfgTable.of(cfgs)
        self._chk(self._lib.stmpc_solver_groups_sim_init_device(self._h, t.array, len(t), int(n_per_group), stream))

    def sim_step_solver_groups(self, groups, n_per_group, N, d_cmd_speed, stream=0):
        """``stmpc_solver_groups_sim_step_device``: the grouped world step with traffic group g's closest-distance gate at ``groups[g].crash_min_s``."""
        t = ParamsTable.of(groups)
        self._chk(self._lib.stmpc_solver_groups_sim_step_device(self._h, t.array, len(t), int(n_per_group), int(N), d_cmd_speed, stream))

    def profile_begin(self):
        self._chk(self._lib.stmpc_profile(self._h, 1, None))

    def profile_end(self):
        t = ProfileTotals()
        self._chk(self._lib.stmpc_profile(self._h, 0, C.byref(t)))
        return {n: getattr(t, n) for n, _ in ProfileTotals._fields_}

    def stats(self):
        s = Stats()
        self._chk(self._lib.stmpc_get_stats(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in Stats._fields_}

    # -- st_cy.solve_s_t_path_fast semantics -------------------------------------------------------
    def solve_grid(self, obstacles, s_values, t_values, v0, a0, distances, tunables11):
        ob = np.ascontiguousarray(obstacles).view(np.uint8) if obstacles.dtype == np.bool_ else \
            np.ascontiguousarray(obstacles, dtype=np.uint8)
        sv = np.ascontiguousarray(s_values, dtype=np.float64)
        tv = np.ascontiguousarray(t_values, dtype=np.float64)
        di = np.ascontiguousarray(distances, dtype=np.float64)
        H, S = tv.shape[0], sv.shape[0]
        if ob.shape != (H, S) or di.shape != (H, S):
            raise ValueError("obstacles/distances must be [num_t, num_s]")
        out = np.empty(H, dtype=np.float64)
        self._chk(self._lib.stmpc_solve_grid(self._h, _u8ptr(ob), _dptr(sv), S, _dptr(tv), H, float(v0), float(a0),
                                             _dptr(di), *[float(x) for x in tunables11], _dptr(out)))
        return out

    def solve_grid_no_jerk(self, variant, obstacles, s_values, t_values, v0, distances):
        """variant 0 = st_cy.solve_s_t_path_no_jerk_fast, 1 = st_cy.solve_s_t_path_no_jerk_djikstra."""
        ob = np.ascontiguousarray(obstacles).view(np.uint8)
        sv = np.ascontiguousarray(s_values, dtype=np.float64)
        tv = np.ascontiguousarray(t_values, dtype=np.float64)
        di = np.ascontiguousarray(distances, dtype=np.float64)
        if ob.shape != (tv.size, sv.size) or di.shape != ob.shape:
            raise ValueError("obstacles / distances must be [num_t, num_s]")
        seq = np.zeros(tv.size)
        self._chk(self._lib.stmpc_solve_grid_no_jerk(self._h, int(variant), _u8ptr(ob), _dptr(sv), sv.size, _dptr(tv), tv.size, float(v0), _dptr(di), _dptr(seq)))
        return seq

    def build_grid(self, params, state5, other_x, other_v):
        state5 = np.ascontiguousarray(state5, dtype=np.float64)
        ox = np.ascontiguousarray(other_x, dtype=np.float64)
        ov = np.ascontiguousarray(other_v, dtype=np.float64)
        k = ox.shape[0]
        H, S = num_t(params), num_s(params, state5[4])
        ob = np.empty((H, S), dtype=np.uint8)
        di = np.empty((H, S), dtype=np.float64)
        sv = np.empty(S, dtype=np.float64)
        tv = np.empty(H, dtype=np.float64)
        self._chk(self._lib.stmpc_build_grid(self._h, C.byref(params), _dptr(state5), k, _dptr(ox) if k else None,
                                             _dptr(ov) if k else None, _u8ptr(ob), _dptr(di), _dptr(sv), _dptr(tv)))
        return ob.view(np.bool_), sv, tv, di

    def predict_batch(self, params, mode, ego4, k_count, other_x, other_v, selected_speed, dt, min_crash_distance, want_acc=False):
        ego4 = np.ascontiguousarray(ego4, dtype=np.float64)
        N = ego4.shape[0]
        k_count = np.ascontiguousarray(k_count, dtype=np.int32)
        other_x = np.ascontiguousarray(other_x, dtype=np.float64).reshape(N, -1)
        other_v = np.ascontiguousarray(other_v, dtype=np.float64).reshape(N, -1)
        Kmax = other_x.shape[1]
        sel = np.ascontiguousarray(selected_speed, dtype=np.float64) if selected_speed is not None else None
        eo = np.empty_like(ego4)
        xo = np.array(other_x, copy=True)
        vo = np.array(other_v, copy=True)
        cr = np.empty(N, dtype=np.int32)
        ao = np.zeros_like(other_x) if want_acc else None
        args = (self._h, C.byref(params), int(mode), N, Kmax, _dptr(ego4), _iptr(k_count), _dptr(other_x) if Kmax else None,
                _dptr(other_v) if Kmax else None, _dptr(sel), float(dt), float(min_crash_distance), _dptr(eo),
                _dptr(xo) if Kmax else None, _dptr(vo) if Kmax else None, _iptr(cr))
        if want_acc:
            self._chk(self._lib.stmpc_predict_batch_acc(*args, _dptr(ao) if Kmax else None))
        else:
            self._chk(self._lib.stmpc_predict_batch(*args))
        if want_acc:
            return eo, xo, vo, cr, ao
        return eo, xo, vo, cr

    # -- combined controller (device pointers; see include/stmpc.h) ------------------------------
    def rollout_step_device(self, params, cfg, N, Kmax, step, d_ego5_start, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_action, stream=0):
        self._chk(self._lib.stmpc_rollout_step_device(self._h, C.byref(params), C.byref(cfg), int(N), int(Kmax), int(step), d_ego5_start, d_cur_ego4,
                                                      d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_action, stream))

    def combined_decide_device(self, params, cfg, N, Kmax, d_ego5_start, d_k, d_ox_start, d_ov_start, d_cur_ego4, d_cur_ox, d_cur_ov,
                               d_first_action, d_last_choice_rl, d_takeover, d_reason, d_speed, stream=0):
        self._chk(self._lib.stmpc_combined_decide_device(self._h, C.byref(params), C.byref(cfg), int(N), int(Kmax), d_ego5_start, d_k, d_ox_start,
                                                         d_ov_start, d_cur_ego4, d_cur_ox, d_cur_ov, d_first_action, d_last_choice_rl,
                                                         d_takeover, d_reason, d_speed, stream))

    # -- controller groups (stmpc_combined_groups_*; see include/stmpc.h) --
    def combined_groups_set(self, params, cfgs, n_per_group):
        """``stmpc_combined_groups_set``: ``cfgs`` is a sequence of ``CombinedCfg``, one per controller group."""
        t = CombinedCfgTable.of(cfgs)
        self._control_groups_key = None       # (combined.ControlGroups.ensure_set's note of the table the context holds)
        self._chk(self._lib.stmpc_combined_groups_set(self._h, C.byref(params), t.array, len(t), int(n_per_group)))

    def combined_groups_clear(self):
        self._control_groups_key = None
        self._chk(self._lib.stmpc_combined_groups_clear(self._h))

    def rollout_step_groups_device(self, params, N, Kmax, step, d_ego5_start, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_action, stream=0):
        self._chk(self._lib.stmpc_rollout_step_groups_device(self._h, C.byref(params), int(N), int(Kmax), int(step), d_ego5_start, d_cur_ego4,
                                                             d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_action, stream))

    def combined_decide_groups_device(self, params, N, Kmax, d_ego5_start, d_k, d_ox_start, d_ov_start, d_cur_ego4, d_cur_ox, d_cur_ov,
                                      d_first_action, d_last_choice_rl, d_takeover, d_reason, d_speed, stream=0):
        self._chk(self._lib.stmpc_combined_decide_groups_device(self._h, C.byref(params), int(N), int(Kmax), d_ego5_start, d_k, d_ox_start,
                                                                d_ov_start, d_cur_ego4, d_cur_ox, d_cur_ov, d_first_action, d_last_choice_rl,
                                                                d_takeover, d_reason, d_speed, stream))

    def policy_features_device(self, fcfg, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_evals, d_feat, feat_stride, stream=0):
        """The policy's float32 input vectors (dqn.get_state_vector_from_base_state + TimeFeature) into ``d_feat`` [N][feat_stride]."""
        self._chk(self._lib.stmpc_policy_features_device(self._h, C.byref(fcfg), int(N), int(Kmax), int(step), d_cur_ego4, d_k, d_cur_ox, d_cur_ov,
                                                         d_cur_oa, d_evals, d_feat, int(feat_stride), stream))

    def actor_create(self, w):
        """Pack and upload a policy network (dict of numpy float32 arrays w0, b0, w1, b1, w2, b2 as torch stores them + tanh_scale, tanh_mean);
        returns an opaque handle for ``actor_eval_device`` / ``actor_destroy``."""
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        w0, b0, w1, b1, w2, b2 = f32(w["w0"]), f32(w["b0"]), f32(w["w1"]), f32(w["b1"]), f32(w["w2"]).reshape(-1), f32(w["b2"]).reshape(-1)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        self._chk(self._lib.stmpc_actor_create(self._h, int(w0.shape[1]), int(w0.shape[0]), int(w1.shape[0]), fp(w0), fp(b0), fp(w1), fp(b1), fp(w2), fp(b2),
                                               float(w["tanh_scale"]), float(w["tanh_mean"]), C.byref(h)))
        return h

    def actor_destroy(self, handle):
        self._lib.stmpc_actor_destroy(handle)

    def actor_eval_device(self, handle, fcfg, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_evals, d_feat, feat_stride, d_jerk, stream=0):
        """One launch: state vectors + the packed network -> proposed jerk [N] fp64 (``stmpc_actor_eval_device``)."""
        self._chk(self._lib.stmpc_actor_eval_device(self._h, handle, C.byref(fcfg), int(N), int(Kmax), int(step), d_cur_ego4, d_k, d_cur_ox, d_cur_ov,
                                                    d_cur_oa, d_evals, d_feat, int(feat_stride), d_jerk, stream))

    # -- actors from learners, and a population of actors (stmpc_actor_view_ddpg, stmpc_actor_pop_*) -------------
    def actor_view_ddpg(self, learner_handle, target=False):
        """A borrowed actor aliasing the learner's online (or target) actor: no copy; ``actor_destroy`` it before the learner goes."""
        h = C.c_void_p()
        self._chk(self._lib.stmpc_actor_view_ddpg(learner_handle, int(bool(target)), C.byref(h)))
        return h

    def actor_pop_create(self, handles):
        """``handles``: a sequence of actor handles (created or views); the library checks the member count and that the shapes are common."""
        arr = (C.c_void_p * len(handles))(*handles)
        h = C.c_void_p()
        self._chk(self._lib.stmpc_actor_pop_create(self._h, arr, len(handles), C.byref(h)))
        return h

    def actor_pop_destroy(self, handle):
        self._lib.stmpc_actor_pop_destroy(handle)

    def actor_pop_size(self, handle):
        return int(self._lib.stmpc_actor_pop_size(handle))

    def actor_pop_eval_device(self, handle, fcfg, n_per_member, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_evals, d_feat, feat_stride, d_jerk,
                              stream=0):
        """One launch for all members, member m on rows [m * n_per_member, (m + 1) * n_per_member) (``stmpc_actor_pop_eval_device``)."""
        self._chk(self._lib.stmpc_actor_pop_eval_device(self._h, handle, C.byref(fcfg), int(n_per_member), int(Kmax), int(step), d_cur_ego4, d_k, d_cur_ox,
                                                        d_cur_ov, d_cur_oa, d_evals, d_feat, int(feat_stride), d_jerk, stream))

    def combined_counts(self, reset=False):
        """(decisions taken, controller solves run for them) since the last reset."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.stmpc_combined_counts(self._h, C.byref(a), C.byref(b), int(bool(reset))))
        return int(a.value), int(b.value)

    # -- first-step shield controller (stmpc_first_step*; see include/stmpc.h) ------------------------------
    def first_step_device(self, params, cfg, N, Kmax, d_ego5, d_k, d_ox, d_ov, d_oa, d_start_speed, d_cmd_speed, d_takeover, d_reason, stream=0):
        self._chk(self._lib.stmpc_first_step_device(self._h, C.byref(params), C.byref(cfg), int(N), int(Kmax), d_ego5, d_k, d_ox, d_ov, d_oa or None,
                                                    d_start_speed, d_cmd_speed, d_takeover, d_reason, stream or None))

    def first_step(self, params, cfg, ego, k_count, other_x, other_v, start_speed, want_state=True):
        """``stmpc_first_step`` on host arrays.  Returns a dict: ``cmd_speed``, ``takeover``, ``reason`` and, with ``want_state``, ``crashed``,
        ``crash_guaranteed`` (the probe's verdict for every state) and the predicted state ``next_ego`` [N][5], ``next_other_x``, ``next_other_v``."""
        ego, k_count, other_x, other_v, N, Kmax = _batch_states(ego, k_count, other_x, other_v)
        start_speed = np.ascontiguousarray(start_speed, dtype=np.float64).reshape(-1)
        if start_speed.size != N:
            raise ValueError("start_speed has %d entries for %d states" % (start_speed.size, N))
        out = {"cmd_speed": np.zeros(N), "takeover": np.zeros(N, np.int32), "reason": np.zeros(N, np.int32)}
        ext = {"crashed": np.zeros(N, np.int32), "crash_guaranteed": np.zeros(N, np.int32), "next_ego": np.zeros((N, 5)), "next_other_x": np.zeros((N, Kmax)),
               "next_other_v": np.zeros((N, Kmax))} if want_state else {}
        self._chk(self._lib.stmpc_first_step(self._h, C.byref(params), C.byref(cfg), N, Kmax, _dptr(ego), _iptr(k_count), _dptr(other_x) if Kmax else None,
                                             _dptr(other_v) if Kmax else None, _dptr(start_speed), _dptr(out["cmd_speed"]), _iptr(out["takeover"]),
                                             _iptr(out["reason"]), _iptr(ext.get("crashed")), _iptr(ext.get("crash_guaranteed")), _dptr(ext.get("next_ego")),
                                             _dptr(ext.get("next_other_x")) if Kmax else None, _dptr(ext.get("next_other_v")) if Kmax else None))
        out.update(ext)
        return out

    def first_step_counts(self, reset=False):
        """(states decided, states taken over, controller solves run for them) since the last reset; synchronises."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.stmpc_first_step_counts(self._h, C.byref(a), C.byref(b), C.byref(c), int(bool(reset))))
        return int(a.value), int(b.value), int(c.value)

    def speed_from_jerk_device(self, params, tick_length, N, d_ego5, d_jerk, d_speed, stream=0):
        """control.get_ego_speed_from_jerk for N states on the device (``stmpc_speed_from_jerk_device``)."""
        self._chk(self._lib.stmpc_speed_from_jerk_device(self._h, C.byref(params), float(tick_length), int(N), d_ego5, d_jerk, d_speed, stream or None))

    # -- batched episode simulator --------------------------------------------------------------
    def sim_init(self, cfg, N, stream=0):
        self._chk(self._lib.stmpc_sim_init_device(self._h, C.byref(cfg), int(N), stream))

    def sim_view(self, cfg, N, Kmax, d_ego5, d_k, d_ox, d_ov, d_oa=0, stream=0):
        self._chk(self._lib.stmpc_sim_view_device(self._h, C.byref(cfg), int(N), int(Kmax), d_ego5, d_k, d_ox, d_ov, d_oa, stream))

    def sim_step(self, params, cfg, N, d_cmd_speed, stream=0):
        self._chk(self._lib.stmpc_sim_step_device(self._h, C.byref(params), C.byref(cfg), int(N), d_cmd_speed, stream))

    def sim_init_groups(self, cfgs, n_per_group, stream=0):
        """``stmpc_sim_init_groups_device``: ``cfgs`` is a ``SimCfgTable`` (or a sequence of ``SimCfg``), one per traffic group."""
        t = SimCfgTable.of(cfgs)
        self._chk(self._lib.stmpc_sim_init_groups_device(self._h, t.array, len(t), int(n_per_group), stream))

    def sim_step_groups(self, params, N, d_cmd_speed, stream=0):
        self._chk(self._lib.stmpc_sim_step_groups_device(self._h, C.byref(params), int(N), d_cmd_speed, stream))

    def sim_groups(self):
        """(G, n_per_group) of the context's world; (0, 0) for an ungrouped one."""
        g, n = C.c_int(0), C.c_int(0)
        self._chk(self._lib.stmpc_sim_groups(self._h, C.byref(g), C.byref(n)))
        return g.value, n.value

    def sim_status_device(self, N, d_status, stream=0):
        """Environment status words into a device int32 array (asynchronous): 0 running, 1 arrived, 2 crashed, 3 out of time."""
        self._chk(self._lib.stmpc_sim_status_device(self._h, int(N), d_status, stream))

    # -- what the learner families' methods below share: each piece of marshalling once ------------------------
    def _new_handle(self, entry, *args):
        """``entry(ctx, *args, &handle)``: the new handle."""
        h = C.c_void_p()
        self._chk(entry(self._h, *args, C.byref(h)))
        return h

    def _borrowed(self, h):
        """A handle another object owns (a population's member, a TD3 learner's base) as a ``c_void_p``; NULL is ``STMPC_EINVAL``."""
        if not h:
            self._chk(STMPC_EINVAL)
        return C.c_void_p(h)

    def _slot_in(self, entry, handle, slot, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        self._chk(entry(handle, int(slot), flat.ctypes.data_as(C.POINTER(C.c_float)), int(flat.size)))

    def _slot_out(self, entry, handle, slot, count):
        flat = np.empty(int(count), dtype=np.float32)
        self._chk(entry(handle, int(slot), flat.ctypes.data_as(C.POINTER(C.c_float)), int(flat.size)))
        return flat

    def _rows_out(self, entry, handle, first, count):
        """``count`` rows from row ``first`` of a learner's ring, float32 [count][DDPG_ROW]; synchronises."""
        rows = np.zeros((int(count), DDPG_ROW), dtype=np.float32)
        self._chk(entry(handle, int(first), int(count), rows.ctypes.data_as(C.POINTER(C.c_float))))
        return rows

    def _tree_out(self, entry, handle, first, count):
        """``count`` nodes from node ``first`` of a learner's sum tree, float64; synchronises."""
        nodes = np.empty(int(count), dtype=np.float64)
        self._chk(entry(handle, int(first), int(count), nodes.ctypes.data_as(C.POINTER(C.c_double))))
        return nodes

    @staticmethod
    def _table(elem, cfgs):
        """The contiguous ``elem[len(cfgs)]`` a population's entry takes, from a sequence of ``elem``."""
        return (elem * len(cfgs))(*cfgs)

    # -- DDPG learner (stmpc_ddpg_*): the handle belongs to this context's device ------------------------
    def ddpg_create(self, cfg):
        return self._new_handle(self._lib.stmpc_ddpg_create, C.byref(cfg))

    def ddpg_destroy(self, handle):
        self._lib.stmpc_ddpg_destroy(handle)

    def ddpg_set_params(self, handle, slot, flat):
        self._slot_in(self._lib.stmpc_ddpg_set_params, handle, slot, flat)

    def ddpg_get_params(self, handle, slot, count):
        return self._slot_out(self._lib.stmpc_ddpg_get_params, handle, slot, count)

    def ddpg_set_state(self, handle, counters, beta_pow):
        cn = np.ascontiguousarray(counters, dtype=np.int64)
        bp = np.ascontiguousarray(beta_pow, dtype=np.float32)
        assert cn.size == DDPG_NCOUNTERS and bp.size == 4
        self._chk(self._lib.stmpc_ddpg_set_state(handle, cn.ctypes.data_as(C.POINTER(C.c_int64)), bp.ctypes.data_as(C.POINTER(C.c_float))))

    def ddpg_get_state(self, handle):
        """(counters int64 [8]: cursor, fill, updates, noisy acting calls, frames, ...; Adam's beta powers float32 [4]); synchronises."""
        cn, bp = np.zeros(DDPG_NCOUNTERS, dtype=np.int64), np.zeros(4, dtype=np.float32)
        self._chk(self._lib.stmpc_ddpg_get_state(handle, cn.ctypes.data_as(C.POINTER(C.c_int64)), bp.ctypes.data_as(C.POINTER(C.c_float))))
        return cn, bp

    def ddpg_push(self, handle, N, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks, d_action, d_reward, d_terminated, d_truncated, stream=0):
        self._chk(self._lib.stmpc_ddpg_push_device(handle, int(N), d_obs, d_next_obs, d_final_obs, int(obs_stride), d_ticks, d_next_ticks, d_action, d_reward,
                                                   d_terminated, d_truncated, stream))

    def ddpg_act(self, handle, N, d_obs, obs_stride, d_ticks, noise, d_action, d_debug=0, stream=0):
        self._chk(self._lib.stmpc_ddpg_act_device(handle, int(N), d_obs, int(obs_stride), d_ticks, int(bool(noise)), d_action, d_debug, stream))

    def ddpg_update(self, handle, n_updates, lr_q, lr_pi, stream=0):
        self._chk(self._lib.stmpc_ddpg_update_device(handle, int(n_updates), float(lr_q), float(lr_pi), stream))

    def ddpg_grads(self, handle, d_grad_actor, d_grad_critic, stream=0):
        self._chk(self._lib.stmpc_ddpg_grads_device(handle, d_grad_actor, d_grad_critic, stream))

    def ddpg_stats(self, handle, d_out, stream=0):
        self._chk(self._lib.stmpc_ddpg_stats_device(handle, d_out, stream))

    def ddpg_replay_read(self, handle, first, count):
        return self._rows_out(self._lib.stmpc_ddpg_replay_read, handle, first, count)

    def ddpg_gather(self, handle, d_rows, stream=0):
        self._chk(self._lib.stmpc_ddpg_gather_device(handle, d_rows, stream))

    # -- prioritised replay (stmpc_per_*) on a lone learner's handle (a TD3 learner: its base) ------------------------
    def per_enable(self, handle, cfg):
        self._chk(self._lib.stmpc_per_enable(handle, C.byref(cfg)))

    def per_tree_read(self, handle, first, count):
        return self._tree_out(self._lib.stmpc_per_tree_read, handle, first, count)

    def per_last(self, handle, d_idx, d_td, d_weight, stream=0):
        self._chk(self._lib.stmpc_per_last_device(handle, d_idx, d_td, d_weight, stream))

    # -- the discrete learners (stmpc_dqn_*, stmpc_c51_*): the DQN agent and the categorical one; the handle belongs to this context's device.  The
    # entries both have are written once with the ``kind`` ("dqn" or "c51") in front and bound as ``dqn_<name>`` and ``c51_<name>`` below the class
    def _q(self, kind, name):
        return getattr(self._lib, "stmpc_%s_%s" % (kind, name))

    def _q_create(self, kind, cfg):
        return self._new_handle(self._q(kind, "create"), C.byref(cfg))

    def _q_destroy(self, kind, handle):
        self._q(kind, "destroy")(handle)

    def _q_set_params(self, kind, handle, slot, flat):
        self._slot_in(self._q(kind, "set_params"), handle, slot, flat)

    def _q_get_params(self, kind, handle, slot, count):
        return self._slot_out(self._q(kind, "get_params"), handle, slot, count)

    def _q_set_state(self, kind, handle, counters, beta_pow):
        cn = np.ascontiguousarray(counters, dtype=np.int64)
        bp = np.ascontiguousarray(beta_pow, dtype=np.float32)
        assert cn.size == DDPG_NCOUNTERS and bp.size == 2
        self._chk(self._q(kind, "set_state")(handle, cn.ctypes.data_as(C.POINTER(C.c_int64)), bp.ctypes.data_as(C.POINTER(C.c_float))))

    def _q_get_state(self, kind, handle):
        """(counters int64 [8]: cursor, fill, updates, exploring acting calls, frames, ...; Adam's beta powers float32 [2]); synchronises."""
        cn, bp = np.zeros(DDPG_NCOUNTERS, dtype=np.int64), np.zeros(2, dtype=np.float32)
        self._chk(self._q(kind, "get_state")(handle, cn.ctypes.data_as(C.POINTER(C.c_int64)), bp.ctypes.data_as(C.POINTER(C.c_float))))
        return cn, bp

    def _q_push(self, kind, handle, N, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated, d_truncated, stream=0):
        self._chk(self._q(kind, "push_device")(handle, int(N), d_obs, d_next_obs, d_final_obs, int(obs_stride), d_action, d_reward, d_terminated, d_truncated, stream))

    def _q_act(self, kind, handle, N, d_obs, obs_stride, eps, d_action, d_debug_q=0, stream=0):
        self._chk(self._q(kind, "act_device")(handle, int(N), d_obs, int(obs_stride), float(eps), d_action, d_debug_q, stream))

    def _q_update(self, kind, handle, n_updates, lr, stream=0):
        self._chk(self._q(kind, "update_device")(handle, int(n_updates), float(lr), stream))

    def _q_grads(self, kind, handle, d_grad, stream=0):
        self._chk(self._q(kind, "grads_device")(handle, d_grad, stream))

    def _q_targets(self, kind, handle, d_out, stream=0):
        self._chk(self._q(kind, "targets_device")(handle, d_out, stream))

    def _q_gather(self, kind, handle, d_rows, stream=0):
        self._chk(self._q(kind, "gather_device")(handle, d_rows, stream))

    def _q_stats(self, kind, handle, d_out, stream=0):
        self._chk(self._q(kind, "stats_device")(handle, d_out, stream))

    def _q_per_enable(self, kind, handle, cfg):
        self._chk(self._q(kind, "per_enable")(handle, C.byref(cfg)))

    def _q_per_tree_read(self, kind, handle, first, count):
        return self._tree_out(self._q(kind, "per_tree_read"), handle, first, count)

    def _q_per_last(self, kind, handle, d_idx, d_td, d_weight, stream=0):
        self._chk(self._q(kind, "per_last_device")(handle, d_idx, d_td, d_weight, stream))

    def _q_padded_read(self, kind, handle, slot, h1, n_out):
        """Debug: a slot (0 ... 3, or ``DQN_GRAD`` / ``C51_GRAD``) in the library's padded layout as {w0 [h1p][32], b0 [h1p], w1 [Ap][h1p], b1 [Ap]};
        ``n_out``: the network's output width, n_actions of DQN and n_actions * n_atoms of C51; synchronises."""
        h1p, Ap = (int(h1) + 15) & ~15, (int(n_out) + 15) & ~15
        flat = self._slot_out(self._q(kind, "padded_read"), handle, slot, 33 * h1p + (h1p + 1) * Ap)
        o = np.cumsum([0, 32 * h1p, h1p, Ap * h1p, Ap])
        return {"w0": flat[o[0]:o[1]].reshape(h1p, 32), "b0": flat[o[1]:o[2]], "w1": flat[o[2]:o[3]].reshape(Ap, h1p), "b1": flat[o[3]:o[4]]}

    # -- what the C51 learner has on top: the distribution's debug entries ----
    def c51_dist(self, handle, d_dist, d_out=0, stream=0):
        self._chk(self._lib.stmpc_c51_dist_device(handle, d_dist, d_out, stream))

    def c51_project(self, handle, n, d_p, d_reward, d_mask, d_disc, d_m, stream=0):
        self._chk(self._lib.stmpc_c51_project_device(handle, int(n), d_p, d_reward, d_mask, d_disc, d_m, stream))

    def c51_replay_read(self, handle, first, count):
        """Debug: ``count`` rows from row ``first`` of a C51 learner's ring, float32 [count][DDPG_ROW]; synchronises."""
        return self._rows_out(self._lib.stmpc_c51_replay_read, handle, first, count)

    def c51_dzout_read(self, handle, batch, n_logits):
        """Debug: the output layer's gradient of the last pass, float32 [Bp][Ap] (``batch`` rounded up to 16, ``n_logits`` to 16); synchronises."""
        out = np.zeros((((int(batch) + 15) & ~15), ((int(n_logits) + 15) & ~15)), dtype=np.float32)
        self._chk(self._lib.stmpc_c51_dzout_read(handle, out.ctypes.data_as(C.POINTER(C.c_float)), int(out.size)))
        return out

    # -- the noisy output layer of a C51 learner (stmpc_noisy_c51_*) ----
    def noisy_c51_enable(self, handle, sigma0):
        self._chk(self._lib.stmpc_noisy_c51_enable(handle, C.byref(NoisyCfg(sigma0=float(sigma0)))))

    def noisy_c51_set_params(self, handle, slot, flat):
        self._slot_in(self._lib.stmpc_noisy_c51_set_params, handle, slot, flat)

    def noisy_c51_get_params(self, handle, slot, count):
        return self._slot_out(self._lib.stmpc_noisy_c51_get_params, handle, slot, count)

    def noisy_c51_act(self, handle, N, d_obs, obs_stride, eps, d_action, d_debug_q=0, stream=0):
        self._chk(self._lib.stmpc_noisy_c51_act_device(handle, int(N), d_obs, int(obs_stride), float(eps), d_action, d_debug_q, stream))

    def noisy_c51_debug_read(self, handle, what, count):
        """Debug: quantity ``what`` (STMPC_NOISY_F_* / _WEFF_* / _WEFF_PADDED_*) as float32 [count]; synchronises."""
        return self._slot_out(self._lib.stmpc_noisy_c51_debug_read, handle, what, count)

    def c51_pop_noisy_enable(self, handle, sigma0s):
        """``sigma0s``: one value per member (``stmpc_pop_noisy_c51_enable``)."""
        self._chk(self._lib.stmpc_pop_noisy_c51_enable(handle, self._table(NoisyCfg, [NoisyCfg(sigma0=float(s)) for s in sigma0s]), len(sigma0s)))

    def c51_pop_noisy_act(self, handle, n_per_member, d_obs, obs_stride, eps, d_action, d_debug_q=0, stream=0):
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        self._chk(self._lib.stmpc_pop_noisy_c51_act_device(handle, int(n_per_member), d_obs, int(obs_stride), eps.ctypes.data_as(C.POINTER(C.c_double)), int(eps.size),
                                                           d_action, d_debug_q, stream))

    # -- populations (stmpc_ddpg_pop_*, stmpc_pop_td3_*, stmpc_pop_dqn_*, stmpc_pop_c51_*): P learners, one launch per kernel.  Written once with the
    # ``kind`` in front, as the discrete learners' are, and bound as ``<kind>_pop_<name>`` below the class: the six methods every population has, then
    # what only the discrete kinds have in this form (``_q_pop_*``); ``act`` / ``push`` / ``update`` of the continuous kinds: ``_continuous_pop_steps``.
    _POPS = {       # kind: (the entries' prefix, the entry of per_enable, the cfg struct)
        "ddpg": ("stmpc_ddpg_pop_", "stmpc_pop_per_enable_ddpg", DDPGCfg), "td3": ("stmpc_pop_td3_", "stmpc_pop_per_enable_td3", TD3Cfg),
        "dqn": ("stmpc_pop_dqn_", "stmpc_pop_dqn_per_enable", DQNCfg), "c51": ("stmpc_pop_c51_", "stmpc_pop_c51_per_enable", C51Cfg)}

    def _pop(self, kind, name):
        return getattr(self._lib, self._POPS[kind][0] + name)

    def _pop_create(self, kind, cfgs):
        """``cfgs``: a sequence of the kind's cfg struct; the library checks the member count and that the launch shapes (a C51 population's n_atoms
        included) are common."""
        return self._new_handle(self._pop(kind, "create"), self._table(self._POPS[kind][2], cfgs), len(cfgs))

    def _pop_destroy(self, kind, handle):
        self._pop(kind, "destroy")(handle)

    def _pop_size(self, kind, handle):
        return int(self._pop(kind, "size")(handle))

    def _pop_member(self, kind, handle, m):
        """The m-th member as a borrowed handle of the lone learner's kind (``stmpc_ddpg``, ``stmpc_td3``, ...) for its methods above (never destroy it)."""
        return self._borrowed(self._pop(kind, "member")(handle, int(m)))

    def _pop_stats(self, kind, handle, d_out, stream=0):
        self._chk(self._pop(kind, "stats_device")(handle, d_out, stream))

    def _pop_per_enable(self, kind, handle, cfgs):
        """Prioritised replay, once per population, on empty rings.  ``cfgs``: one ``PERCfg`` or None per member; a None member keeps sampling uniformly."""
        on = (C.c_uint8 * len(cfgs))(*[int(c is not None) for c in cfgs])
        self._chk(getattr(self._lib, self._POPS[kind][1])(handle, self._table(PERCfg, [c if c is not None else PERCfg() for c in cfgs]), on, len(cfgs)))

    def _q_pop_act(self, kind, handle, n_per_member, d_obs, obs_stride, eps, d_action, d_debug_q=0, stream=0):
        """``eps``: one value per member (the library checks the length and the range)."""
        e = np.ascontiguousarray(eps, dtype=np.float64).reshape(-1)
        self._chk(self._pop(kind, "act_device")(handle, int(n_per_member), d_obs, int(obs_stride), _dptr(e), int(e.size), d_action, d_debug_q, stream))

    def _q_pop_push(self, kind, handle, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_action, d_reward, d_terminated, d_truncated, stream=0):
        self._chk(self._pop(kind, "push_device")(handle, int(n_per_member), d_obs, d_next_obs, d_final_obs, int(obs_stride), d_action, d_reward, d_terminated,
                                                 d_truncated, stream))

    def _q_pop_update(self, kind, handle, n_updates, lr, stream=0):
        """``lr``: one learning rate per member (the library checks the length)."""
        lr = np.ascontiguousarray(lr, dtype=np.float64).reshape(-1)
        self._chk(self._pop(kind, "update_device")(handle, int(n_updates), _dptr(lr), int(lr.size), stream))

    def _q_pop_replay_read(self, kind, learner_handle, first, count):
        """Debug: ``count`` rows from row ``first`` of a learner's ring (a borrowed member's or a lone learner's), float32 [count][DDPG_ROW]; synchronises."""
        return self._rows_out(self._pop(kind, "replay_read"), learner_handle, first, count)

    # -- multi-step returns: once per learner / population, on empty rings.  The stmpc_nstep_ and stmpc_pop_nstep_ prefixes are closed sets, so the
    # C51 learner's entries carry ``multi_step`` in their own prefixes; a lone TD3 learner is its base, kind "ddpg"
    _NSTEP = {      # kind: the entries of (nstep_enable, pop_nstep_enable, nstep_window)
        "ddpg": ("stmpc_nstep_enable_ddpg", "stmpc_pop_nstep_enable_ddpg", "stmpc_nstep_window_ddpg"),
        "td3": (None, "stmpc_pop_nstep_enable_td3", None),
        "dqn": ("stmpc_nstep_enable_dqn", "stmpc_pop_nstep_enable_dqn", "stmpc_nstep_window_dqn"),
        "c51": ("stmpc_c51_multi_step_enable", "stmpc_pop_c51_multi_step_enable", "stmpc_pop_c51_multi_step_window")}

    def _nstep(self, kind, which):
        name = self._NSTEP[kind][which]
        if name is None:
            raise ValueError("a lone TD3 learner's ring is its base's: its multi-step entries are the kind \"ddpg\"'s, on the base handle")
        return getattr(self._lib, name)

    def nstep_enable(self, kind, handle, cfg):
        self._chk(self._nstep(kind, 0)(handle, C.byref(cfg)))

    def pop_nstep_enable(self, kind, handle, cfgs):
        """``cfgs``: one ``NStepCfg`` per member."""
        self._chk(self._nstep(kind, 1)(handle, self._table(NStepCfg, cfgs), len(cfgs)))

    def nstep_window(self, kind, handle, idx):
        """Debug: float64 [len(idx)][4] = R, disc, the ring row of the window's last transition, m of the ring rows ``idx`` of a learner's handle (a
        borrowed member's or a lone learner's); synchronises."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = np.zeros((idx.size, 4), dtype=np.float64)
        self._chk(self._nstep(kind, 2)(handle, idx.ctypes.data_as(C.POINTER(C.c_int64)), int(idx.size), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def c51_pop_multi_step_enable(self, handle, cfgs):
        return self.pop_nstep_enable("c51", handle, cfgs)

    def c51_pop_multi_step_window(self, learner_handle, idx):
        return self.nstep_window("c51", learner_handle, idx)

    # -- a Q-network as a policy (stmpc_qactor_*): DQNAgent.get_control, dqn.py:375-380 ------------------------
    def qactor_create(self, net, action_values, mode=0):
        """Pack and upload a Q-network (dict of numpy float32 arrays w0, b0, w1, b1 as torch stores them) with its action table (fp64 [A]);
        ``mode``: a ``QACTOR_MODES`` code.  Returns an opaque handle for ``qactor_eval_device`` / ``qactor_destroy``."""
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        w0, b0, w1, b1 = f32(net["w0"]), f32(net["b0"]).reshape(-1), f32(net["w1"]), f32(net["b1"]).reshape(-1)
        if w0.ndim != 2 or w1.ndim != 2 or b0.size != w0.shape[0] or w1.shape[1] != w0.shape[0] or b1.size != w1.shape[0]:
            raise ValueError("the net's tensors are not w0 [h1][n_in], b0 [h1], w1 [A][h1], b1 [A]")
        table = np.ascontiguousarray(action_values, dtype=np.float64).reshape(-1)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        self._chk(self._lib.stmpc_qactor_create(self._h, int(w0.shape[1]), int(w0.shape[0]), int(table.size), fp(w0), fp(b0), fp(w1), fp(b1),
                                                table.ctypes.data_as(C.POINTER(C.c_double)), int(mode), C.byref(h)))
        return h

    def qactor_view_dqn(self, learner_handle, action_values, target=False, mode=0):
        """A borrowed policy aliasing the DQN learner's online (or target) network: no copy; ``qactor_destroy`` it before the learner goes."""
        table = np.ascontiguousarray(action_values, dtype=np.float64).reshape(-1)
        h = C.c_void_p()
        self._chk(self._lib.stmpc_qactor_view_dqn(learner_handle, int(bool(target)), table.ctypes.data_as(C.POINTER(C.c_double)), int(table.size), int(mode), C.byref(h)))
        return h

    def c51actor_create(self, net, action_values, n_atoms, v_min, v_max, mode=0, dueling=False):
        """``qactor_create`` for a categorical (C51) network: w1 [A * n_atoms][h1], b1 [A * n_atoms] as ``C51Learner.export_q`` writes them, with the
        support's ``n_atoms``, ``v_min``, ``v_max`` (``stmpc_c51actor_create``).  ``dueling``: the net has (A + 1) * n_atoms output rows, the value
        block last (``stmpc_dueling_c51actor_create``).  The handle is a Q-actor's: ``qactor_eval_device``, ``qactor_set_limits`` and
        ``qactor_destroy`` take it."""
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        w0, b0, w1, b1 = f32(net["w0"]), f32(net["b0"]).reshape(-1), f32(net["w1"]), f32(net["b1"]).reshape(-1)
        table = np.ascontiguousarray(action_values, dtype=np.float64).reshape(-1)
        if (w0.ndim != 2 or w1.ndim != 2 or b0.size != w0.shape[0] or w1.shape[1] != w0.shape[0] or b1.size != w1.shape[0]
                or w1.shape[0] != (table.size + (1 if dueling else 0)) * int(n_atoms)):
            raise ValueError("the net's tensors are not w0 [h1][n_in], b0 [h1], w1 [%s * n_atoms][h1], b1 [%s * n_atoms]" % (("(A + 1)",) * 2 if dueling else ("A",) * 2))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        create = self._lib.stmpc_dueling_c51actor_create if dueling else self._lib.stmpc_c51actor_create
        self._chk(create(self._h, int(w0.shape[1]), int(w0.shape[0]), int(table.size), int(n_atoms), float(v_min), float(v_max), fp(w0), fp(b0), fp(w1), fp(b1),
                         table.ctypes.data_as(C.POINTER(C.c_double)), int(mode), C.byref(h)))
        return h

    def c51actor_view(self, learner_handle, action_values, target=False, mode=0):
        """A borrowed policy aliasing the C51 learner's online (or target) logits network: no copy; ``qactor_destroy`` it before the learner goes."""
        table = np.ascontiguousarray(action_values, dtype=np.float64).reshape(-1)
        h = C.c_void_p()
        self._chk(self._lib.stmpc_c51actor_view(learner_handle, int(bool(target)), table.ctypes.data_as(C.POINTER(C.c_double)), int(table.size), int(mode), C.byref(h)))
        return h

    def qactor_destroy(self, handle):
        self._lib.stmpc_qactor_destroy(handle)

    def qactor_set_limits(self, handle, tick_length, minimum_negative_jerk, maximum_positive_jerk):
        """Acceleration mode's constants (Settings.TICK_LENGTH, MINIMUM_NEGATIVE_JERK, MAXIMUM_POSITIVE_JERK)."""
        self._chk(self._lib.stmpc_qactor_set_limits(handle, float(tick_length), float(minimum_negative_jerk), float(maximum_positive_jerk)))

    def qactor_eval_device(self, handle, fcfg, N, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_feat, feat_stride, d_action, d_q, d_jerk, stream=0):
        """One launch: state vectors + Q-network + first argmax + action table -> jerk [N] fp64 (``stmpc_qactor_eval_device``)."""
        self._chk(self._lib.stmpc_qactor_eval_device(self._h, handle, C.byref(fcfg), int(N), int(Kmax), int(step), d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa,
                                                     d_feat, int(feat_stride), d_action, d_q, d_jerk, stream))

    # -- a population of Q-networks as policies (stmpc_pop_qactor_*) ------------------------
    def qactor_pop_create(self, handles):
        """``handles``: a sequence of Q-actor handles (created or views); the library checks the member count, the common shape and that every
        acceleration-mode member has its limits.  The members must outlive the population."""
        arr = (C.c_void_p * len(handles))(*handles)
        h = C.c_void_p()
        self._chk(self._lib.stmpc_pop_qactor_create(self._h, arr, len(handles), C.byref(h)))
        return h

    def c51actor_pop_create(self, handles):
        """``qactor_pop_create`` for categorical (C51) Q-actor handles (``c51actor_create`` or ``c51actor_view``; ``stmpc_pop_c51actor_create``): they
        share n_in, the padded hidden width, n_actions, n_atoms and the head; the support may differ.  The handle is a Q-actor population's:
        ``qactor_pop_destroy``, ``qactor_pop_size``, ``qactor_pop_eval_device`` and the ``qshield_env_*`` entries take it."""
        arr = (C.c_void_p * len(handles))(*handles)
        h = C.c_void_p()
        self._chk(self._lib.stmpc_pop_c51actor_create(self._h, arr, len(handles), C.byref(h)))
        return h

    def qactor_pop_destroy(self, handle):
        self._lib.stmpc_pop_qactor_destroy(handle)

    def qactor_pop_size(self, handle):
        return int(self._lib.stmpc_pop_qactor_size(handle))

    def qactor_pop_eval_device(self, handle, fcfg, n_per_member, Kmax, step, d_cur_ego4, d_k, d_cur_ox, d_cur_ov, d_cur_oa, d_feat, feat_stride, d_action, d_q,
                               d_jerk, stream=0):
        """One launch for all members, member m on rows [m * n_per_member, (m + 1) * n_per_member) (``stmpc_pop_qactor_eval_device``)."""
        self._chk(self._lib.stmpc_pop_qactor_eval_device(self._h, handle, C.byref(fcfg), int(n_per_member), int(Kmax), int(step), d_cur_ego4, d_k, d_cur_ox,
                                                         d_cur_ov, d_cur_oa, d_feat, int(feat_stride), d_action, d_q, d_jerk, stream))

    # -- TD3 learner (stmpc_td3_*): a DDPG learner as base plus critic 2 ------------------------
    def td3_create(self, cfg):
        return self._new_handle(self._lib.stmpc_td3_create, C.byref(cfg))

    def td3_destroy(self, handle):
        self._lib.stmpc_td3_destroy(handle)

    def td3_base(self, handle):
        """The base as a borrowed ``stmpc_ddpg`` handle for the ``ddpg_*`` methods above (never ``ddpg_destroy`` it)."""
        return self._borrowed(self._lib.stmpc_td3_base(handle))

    def td3_set_params(self, handle, slot, flat):
        self._slot_in(self._lib.stmpc_td3_set_params, handle, slot, flat)

    def td3_get_params(self, handle, slot, count):
        return self._slot_out(self._lib.stmpc_td3_get_params, handle, slot, count)

    def td3_set_state(self, handle, beta_pow2):
        bp = np.ascontiguousarray(beta_pow2, dtype=np.float32)
        assert bp.size == 2
        self._chk(self._lib.stmpc_td3_set_state(handle, bp.ctypes.data_as(C.POINTER(C.c_float))))

    def td3_get_state(self, handle):
        """Critic 2's beta powers float32 [2]; synchronises."""
        bp = np.zeros(2, dtype=np.float32)
        self._chk(self._lib.stmpc_td3_get_state(handle, bp.ctypes.data_as(C.POINTER(C.c_float))))
        return bp

    def td3_update(self, handle, n_updates, lr_q, lr_pi, stream=0):
        self._chk(self._lib.stmpc_td3_update_device(handle, int(n_updates), float(lr_q), float(lr_pi), stream))

    def td3_grads(self, handle, d_grad_actor, d_grad_critic1, d_grad_critic2, stream=0):
        self._chk(self._lib.stmpc_td3_grads_device(handle, d_grad_actor, d_grad_critic1, d_grad_critic2, stream))

    def td3_targets(self, handle, d_out, stream=0):
        self._chk(self._lib.stmpc_td3_targets_device(handle, d_out, stream))

    def td3_stats(self, handle, d_out, stream=0):
        self._chk(self._lib.stmpc_td3_stats_device(handle, d_out, stream))

    # -- episode flight recorder (stmpc_rec_*): the handle follows this context's world ------------------------
    def rec_create(self, N, Kmax, depth, tick_length, edges):
        """A recorder of ``depth`` records per environment with the given bin edges for this context's world (``stmpc_rec_create``)."""
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        h = C.c_void_p()
        self._chk(self._lib.stmpc_rec_create(self._h, int(N), int(Kmax), int(depth), float(tick_length), _dptr(edges), int(edges.size), C.byref(h)))
        return h

    def rec_destroy(self, handle):
        self._lib.stmpc_rec_destroy(handle)

    def rec_reset(self, handle, stream=0):
        self._chk(self._lib.stmpc_rec_reset(handle, stream))

    def rec_tick(self, handle, N, Kmax, d_ego5, d_k, d_ox, d_ov, d_oa, d_cmd_speed, d_takeover=0, stream=0):
        """One record + the bin accumulators for every running environment; between the controller and ``sim_step`` (asynchronous)."""
        self._chk(self._lib.stmpc_rec_tick_device(handle, int(N), int(Kmax), d_ego5, d_k, d_ox, d_ov, d_oa or None, d_cmd_speed, d_takeover or None, stream))

    def rec_reduce(self, handle, d_out=0, stream=0):
        self._chk(self._lib.stmpc_rec_reduce_device(handle, d_out or None, stream))

    def rec_read(self, handle, N, Kmax, depth, n_edges, want_ring=True):
        """Host copies (synchronises): dict of ``ring`` [N][depth][REC_HDR + 3 Kmax] in chronological order, ``length`` [N], ``acc_env``
        [REC_NQ * (n_edges - 1) + 2][N], ``acc_reduced`` and the world's ``status`` [N]."""
        rows = REC_NQ * (int(n_edges) - 1) + 2
        out = {"ring": np.zeros((N, depth, REC_HDR + 3 * Kmax)) if want_ring else None, "length": np.zeros(N, np.int32), "acc_env": np.zeros((rows, N)),
               "acc_reduced": np.zeros(rows), "status": np.zeros(N, np.int32)}
        self._chk(self._lib.stmpc_rec_read(handle, _dptr(out["ring"]), _iptr(out["length"]), _dptr(out["acc_env"]), _dptr(out["acc_reduced"]), _iptr(out["status"])))
        return out

    # -- vector environment (stmpc_env_*) ---------------------------------------------------------------
    def env_reset(self, params, sim_cfg, env_cfg, N, d_obs, obs_stride, stream=0):
        self._chk(self._lib.stmpc_env_reset_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), int(N), d_obs, int(obs_stride), stream))

    def env_step(self, params, sim_cfg, env_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs=0, d_final_stats=0, stream=0):
        self._chk(self._lib.stmpc_env_step_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), int(N), d_action, d_obs, int(obs_stride),
                                                  d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, stream))

    def env_reset_groups(self, params, cfgs, n_per_group, env_cfg, d_obs, obs_stride, stream=0):
        t = SimCfgTable.of(cfgs)
        self._chk(self._lib.stmpc_env_reset_groups_device(self._h, C.byref(params), t.array, len(t), int(n_per_group), C.byref(env_cfg), d_obs, int(obs_stride), stream))

    def env_step_groups(self, params, env_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs=0, d_final_stats=0, stream=0):
        self._chk(self._lib.stmpc_env_step_groups_device(self._h, C.byref(params), C.byref(env_cfg), int(N), d_action, d_obs, int(obs_stride), d_reward, d_terminated,
                                                         d_truncated, d_final_obs, d_final_stats, stream))

    # -- shielded vector environment (stmpc_shield_env_*; see include/stmpc.h) -------------------------------
    def shield_env_reset(self, params, sim_cfg, env_cfg, shield_cfg, N, d_obs, obs_stride, stream=0):
        self._chk(self._lib.stmpc_shield_env_reset_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), C.byref(shield_cfg), int(N), d_obs,
                                                          int(obs_stride), stream))

    def shield_env_step(self, params, sim_cfg, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs,
                        d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks, stream=0):
        """``stmpc_shield_env_step_device``; ``d_executed_action``: 0 for a discrete env."""
        self._chk(self._lib.stmpc_shield_env_step_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), C.byref(shield_cfg), int(N), d_action,
                                                         d_obs, int(obs_stride), d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, d_takeover,
                                                         d_reason, d_executed_jerk, d_executed_action or None, d_takeover_ticks, stream))

    # -- vector environment behind the combined controller (stmpc_cshield_env_*; see include/stmpc.h) --------------
    def cshield_env_reset(self, params, sim_cfg, env_cfg, shield_cfg, actor, N, d_obs, obs_stride, stream=0):
        """``stmpc_cshield_env_reset_device``; ``actor``: an actor handle (``actor_create`` or ``actor_view_ddpg``)."""
        self._chk(self._lib.stmpc_cshield_env_reset_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), C.byref(shield_cfg), actor, int(N), d_obs,
                                                           int(obs_stride), stream))

    def cshield_env_step(self, params, sim_cfg, env_cfg, shield_cfg, actor, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs,
                         d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks, stream=0):
        """``stmpc_cshield_env_step_device``; ``d_executed_action`` may be 0."""
        self._chk(self._lib.stmpc_cshield_env_step_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), C.byref(shield_cfg), actor, int(N), d_action,
                                                          d_obs, int(obs_stride), d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats, d_takeover,
                                                          d_reason, d_executed_jerk, d_executed_action or None, d_takeover_ticks, stream))

    # -- discrete vector environment behind the combined controller, a Q-network in the rollout (stmpc_qshield_env_*; see include/stmpc.h) --------
    def qshield_env_reset(self, params, sim_cfg, env_cfg, shield_cfg, qactor, qactor_pop, n_per_member, N, d_obs, obs_stride, stream=0):
        """``stmpc_qshield_env_reset_device``; exactly one of ``qactor`` (a ``qactor_create`` / ``qactor_view_dqn`` handle, ``n_per_member`` 0) and
        ``qactor_pop`` (a ``pop_qactor_create`` handle) is given, the other None."""
        self._chk(self._lib.stmpc_qshield_env_reset_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), C.byref(shield_cfg), qactor, qactor_pop,
                                                           int(n_per_member), int(N), d_obs, int(obs_stride), stream))

    def qshield_env_step(self, params, sim_cfg, env_cfg, shield_cfg, qactor, qactor_pop, n_per_member, N, d_action, d_obs, obs_stride, d_reward, d_terminated,
                         d_truncated, d_final_obs, d_final_stats, d_takeover, d_reason, d_executed_jerk, d_takeover_ticks, stream=0):
        """``stmpc_qshield_env_step_device``: no ``d_executed_action`` (a discrete index is not rewritten)."""
        self._chk(self._lib.stmpc_qshield_env_step_device(self._h, C.byref(params), C.byref(sim_cfg), C.byref(env_cfg), C.byref(shield_cfg), qactor, qactor_pop,
                                                          int(n_per_member), int(N), d_action, d_obs, int(obs_stride), d_reward, d_terminated, d_truncated,
                                                          d_final_obs, d_final_stats, d_takeover, d_reason, d_executed_jerk, d_takeover_ticks, stream))

    def cshield_env_evals(self, N, d_evals, stream=0):
        """``stmpc_cshield_env_evals_device``: the count the next step's proposal is evaluated at, int32 [N] on the device."""
        self._chk(self._lib.stmpc_cshield_env_evals_device(self._h, int(N), d_evals, stream))

    # -- first-step shield on traffic groups, reward groups and the traffic mix (stmpc_shield_*groups* / stmpc_shield_traffic_mix_*; see include/stmpc.h) ----
    @staticmethod
    def _penalties(takeover_penalties):
        """(pointer, P, the array kept alive) of a reset's ``takeover_penalties``: None -> (NULL, 0, None), the shield cfg's penalty for every group."""
        if takeover_penalties is None:
            return None, 0, None
        w = np.ascontiguousarray(takeover_penalties, dtype=np.float64).reshape(-1)
        return _dptr(w), int(w.size), w

    @staticmethod
    def _sims(sim_cfgs):
        """(pointer, G) of a reward-groups reset's world: one ``SimCfg`` (an ungrouped world: G = 0) or a ``SimCfgTable`` / sequence (the array owns its
        memory; what its rows point to is the caller's, alive for the call)."""
        if isinstance(sim_cfgs, SimCfg):
            return C.byref(sim_cfgs), 0
        t = SimCfgTable.of(sim_cfgs)
        return t.array, len(t)

    @staticmethod
    def _mix(sim_cfgs, weights):
        """(table, weights as fp64 [T]) of a traffic-mix reset: ValueError unless there is one weight per traffic type."""
        t = SimCfgTable.of(sim_cfgs)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != len(t):
            raise ValueError("%d weights for %d traffic types" % (w.size, len(t)))
        return t, w

    def shield_env_reset_groups(self, params, cfgs, n_per_group, env_cfg, shield_cfg, takeover_penalties, d_obs, obs_stride, stream=0):
        """``stmpc_shield_traffic_groups_env_reset_device``; ``takeover_penalties``: None, or 1 or G numbers."""
        t = SimCfgTable.of(cfgs)
        ptr, P, keep = self._penalties(takeover_penalties)
        self._chk(self._lib.stmpc_shield_traffic_groups_env_reset_device(self._h, C.byref(params), t.array, len(t), int(n_per_group), C.byref(env_cfg), C.byref(shield_cfg),
                                                                 ptr, P, d_obs, int(obs_stride), stream))

    def shield_env_reset_reward_groups(self, params, sim_cfgs, n_per_traffic_group, env_cfgs, n_per_reward_group, shield_cfg, takeover_penalties, d_obs,
                                       obs_stride, stream=0):
        """``stmpc_shield_reward_groups_env_reset_device``; ``sim_cfgs`` and ``env_cfgs`` as ``env_reset_reward_groups`` takes them."""
        e = EnvCfgTable.of(env_cfgs)
        sims, G = self._sims(sim_cfgs)
        ptr, P, keep = self._penalties(takeover_penalties)
        self._chk(self._lib.stmpc_shield_reward_groups_env_reset_device(self._h, C.byref(params), sims, G, int(n_per_traffic_group), e.array, len(e),
                                                                        int(n_per_reward_group), C.byref(shield_cfg), ptr, P, d_obs, int(obs_stride), stream))

    def shield_traffic_mix_env_reset(self, params, sim_cfgs, weights, mix_seed, env_cfg, shield_cfg, N, d_obs, obs_stride, d_traffic_type=0, stream=0):
        """``stmpc_shield_traffic_mix_env_reset_device``; ``sim_cfgs`` and ``weights`` as ``traffic_mix_env_reset`` takes them."""
        t, w = self._mix(sim_cfgs, weights)
        self._chk(self._lib.stmpc_shield_traffic_mix_env_reset_device(self._h, C.byref(params), t.array, len(t), _dptr(w), C.c_uint64(int(mix_seed) & 0xFFFFFFFFFFFFFFFF),
                                                                      C.byref(env_cfg), C.byref(shield_cfg), int(N), d_obs, int(obs_stride), d_traffic_type or None,
                                                                      stream))

    def _shield_groups_step(self, entry, params, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs,
                            d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks, *tail):
        self._chk(entry(self._h, C.byref(params), C.byref(env_cfg), C.byref(shield_cfg), int(N), d_action, d_obs, int(obs_stride), d_reward, d_terminated,
                        d_truncated, d_final_obs, d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action or None, d_takeover_ticks, *tail))

    def shield_env_step_groups(self, params, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs,
                               d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks, stream=0):
        """``stmpc_shield_traffic_groups_env_step_device``; ``d_executed_action``: 0 for a discrete env."""
        self._shield_groups_step(self._lib.stmpc_shield_traffic_groups_env_step_device, params, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward,
                                 d_terminated, d_truncated, d_final_obs, d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action,
                                 d_takeover_ticks, stream)

    def shield_env_step_reward_groups(self, params, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs,
                                      d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks, stream=0):
        """``stmpc_shield_reward_groups_env_step_device``."""
        self._shield_groups_step(self._lib.stmpc_shield_reward_groups_env_step_device, params, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward,
                                 d_terminated, d_truncated, d_final_obs, d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action,
                                 d_takeover_ticks, stream)

    def shield_traffic_mix_env_step(self, params, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs,
                                    d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action, d_takeover_ticks, d_traffic_type,
                                    d_final_traffic_type, stream=0):
        """``stmpc_shield_traffic_mix_env_step_device``."""
        self._shield_groups_step(self._lib.stmpc_shield_traffic_mix_env_step_device, params, env_cfg, shield_cfg, N, d_action, d_obs, obs_stride, d_reward,
                                 d_terminated, d_truncated, d_final_obs, d_final_stats, d_takeover, d_reason, d_executed_jerk, d_executed_action,
                                 d_takeover_ticks, d_traffic_type, d_final_traffic_type, stream)

    # -- traffic mix (stmpc_traffic_mix_*; see include/stmpc.h) ---------------------------------------------------
    def traffic_mix_env_reset(self, params, sim_cfgs, weights, mix_seed, env_cfg, N, d_obs, obs_stride, d_traffic_type=0, stream=0):
        """``stmpc_traffic_mix_env_reset_device``: ``sim_cfgs`` is a ``SimCfgTable`` (or a sequence of ``SimCfg``), one per traffic type, ``weights``
        one number per type."""
        t, w = self._mix(sim_cfgs, weights)
        self._chk(self._lib.stmpc_traffic_mix_env_reset_device(self._h, C.byref(params), t.array, len(t), _dptr(w), C.c_uint64(int(mix_seed) & 0xFFFFFFFFFFFFFFFF),
                                                               C.byref(env_cfg), int(N), d_obs, int(obs_stride), d_traffic_type or None, stream))

    def traffic_mix_env_step(self, params, env_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs, d_final_stats,
                             d_traffic_type, d_final_traffic_type, stream=0):
        self._chk(self._lib.stmpc_traffic_mix_env_step_device(self._h, C.byref(params), C.byref(env_cfg), int(N), d_action, d_obs, int(obs_stride), d_reward,
                                                              d_terminated, d_truncated, d_final_obs, d_final_stats, d_traffic_type, d_final_traffic_type, stream))

    def env_reward(self, env_cfg, N, Kmax, d_ego4, d_k, d_ox, d_jerk, d_crashed=0, d_arrived=0, d_reward=0, stream=0):
        self._chk(self._lib.stmpc_env_reward_device(self._h, C.byref(env_cfg), int(N), int(Kmax), d_ego4, d_k, d_ox, 0, 0, d_jerk, d_crashed, d_arrived,
                                                    d_reward, stream))

    def env_reset_reward_groups(self, params, sim_cfgs, n_per_traffic_group, env_cfgs, n_per_reward_group, d_obs, obs_stride, stream=0):
        """``stmpc_reward_groups_env_reset_device``: ``env_cfgs`` is an ``EnvCfgTable`` (or a sequence of ``EnvCfg``), one per reward group;
        ``sim_cfgs`` is one ``SimCfg`` (an ungrouped world, ``n_per_traffic_group`` unused) or a ``SimCfgTable`` / sequence (traffic groups)."""
        e = EnvCfgTable.of(env_cfgs)
        sims, G = self._sims(sim_cfgs)
        self._chk(self._lib.stmpc_reward_groups_env_reset_device(self._h, C.byref(params), sims, G, int(n_per_traffic_group), e.array, len(e),
                                                                 int(n_per_reward_group), d_obs, int(obs_stride), stream))

    def env_step_reward_groups(self, params, env_cfg, N, d_action, d_obs, obs_stride, d_reward, d_terminated, d_truncated, d_final_obs=0, d_final_stats=0,
                               stream=0):
        self._chk(self._lib.stmpc_reward_groups_env_step_device(self._h, C.byref(params), C.byref(env_cfg), int(N), d_action, d_obs, int(obs_stride), d_reward,
                                                                d_terminated, d_truncated, d_final_obs, d_final_stats, stream))

    def env_reward_reward_groups(self, env_cfg, N, Kmax, d_ego4, d_k, d_ox, d_jerk, d_crashed=0, d_arrived=0, d_reward=0, stream=0):
        """``stmpc_reward_groups_env_reward_device``: state e is rewarded under reward group ``e // n_per_reward_group`` of the context's env."""
        self._chk(self._lib.stmpc_reward_groups_env_reward_device(self._h, C.byref(env_cfg), int(N), int(Kmax), d_ego4, d_k, d_ox, 0, 0, d_jerk, d_crashed,
                                                                  d_arrived, d_reward, stream))

    def env_reward_groups(self):
        """(R, n_per_reward_group) of the context's env; (0, 0) without reward groups."""
        r, n = C.c_int(0), C.c_int(0)
        self._chk(self._lib.stmpc_reward_groups_split(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def env_episode_ticks(self, N, d_ticks, stream=0):
        """Ticks of each environment's current episode into a device int32 [N] array (asynchronous)."""
        self._chk(self._lib.stmpc_env_episode_ticks_device(self._h, int(N), d_ticks, stream))

    def env_drain(self, capacity):
        """(rows [n][ENV_LOG_COLS], dropped): the episodes finished since the last drain (synchronises)."""
        rows = np.zeros((max(int(capacity), 1), ENV_LOG_COLS))
        n, dropped = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.stmpc_env_drain(self._h, int(capacity), _dptr(rows), C.byref(n), C.byref(dropped)))
        return rows[:n.value], int(dropped.value)

    def check_error(self):
        """Synchronise and raise what kernels of earlier (asynchronous) calls on this context flagged; see ``stmpc_check_error``."""
        self._chk(self._lib.stmpc_check_error(self._h))

    def sim_read(self, N):
        status, ticks = np.zeros(N, np.int32), np.zeros(N, np.int32)
        acc, ego4 = np.zeros((N, SIM_NACC)), np.zeros((N, 4))
        self._chk(self._lib.stmpc_sim_read(self._h, int(N), _iptr(status), _iptr(ticks), _dptr(acc), _dptr(ego4)))
        return status, ticks, acc, ego4

    def combined_read_state(self, N, Kmax, rollout_length, after_decide=True):
        """Host copies of the rollout bookkeeping (and, after the decision, of the probe / controller results)."""
        K = max(int(Kmax), 1)
        R1 = max(int(rollout_length), 1) + 1
        out = {"live": np.zeros(N, np.int32), "hist_len": np.zeros(N, np.int32), "crash_pred": np.zeros(N, np.int32),
               "sel_speed": np.zeros(N), "rollout_s": np.zeros((N, R1)), "have_test": np.zeros(N, np.int32),
               "test_ego4": np.zeros((N, 4)), "test_ox": np.zeros((N, K)), "test_ov": np.zeros((N, K))}
        extra = {"probe_crash": np.zeros(N, np.int32), "st_speed": np.zeros(N), "fine": np.zeros((N, QP_NMAX)), "fine_len": np.zeros(N, np.int32)} if after_decide else {}
        self._chk(self._lib.stmpc_combined_read_state(self._h, int(N), _iptr(out["live"]), _iptr(out["hist_len"]), _iptr(out["crash_pred"]), _dptr(out["sel_speed"]),
                                                      _dptr(out["rollout_s"]), _iptr(out["have_test"]), _dptr(out["test_ego4"]), _dptr(out["test_ox"]), _dptr(out["test_ov"]),
                                                      _iptr(extra.get("probe_crash")), _dptr(extra.get("st_speed")), _dptr(extra.get("fine")), _iptr(extra.get("fine_len"))))
        out.update(extra)
        return out

    def probe_arith(self, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
        out = np.empty_like(a)
        self._chk(self._lib.stmpc_probe_arith(self._h, int(op), _dptr(a), _dptr(b), _dptr(out), a.size))
        return out


# Context.dqn_<name> / c51_<name>: the discrete learners' shared methods with their kind; Context.<kind>_pop_<name>: the populations' likewise
for _kind in ("dqn", "c51"):
    for _name in ("create", "destroy", "set_params", "get_params", "set_state", "get_state", "push", "act", "update", "grads", "targets", "gather", "stats",
                  "per_enable", "per_tree_read", "per_last", "padded_read"):
        setattr(Context, "%s_%s" % (_kind, _name), functools.partialmethod(getattr(Context, "_q_" + _name), _kind))
for _kind in Context._POPS:
    for _name in ("create", "destroy", "size", "member", "stats", "per_enable"):
        setattr(Context, "%s_pop_%s" % (_kind, _name), functools.partialmethod(getattr(Context, "_pop_" + _name), _kind))
for _kind in ("dqn", "c51"):
    for _name in ("act", "push", "update", "replay_read"):
        setattr(Context, "%s_pop_%s" % (_kind, _name), functools.partialmethod(getattr(Context, "_q_pop_" + _name), _kind))


def _continuous_pop_steps(prefix):
    """``act``, ``push`` and ``update`` of a continuous population whose entries begin with ``prefix``.  They are the three calls of every training
    step, so each is a plain method that knows its entry, with no ``partialmethod`` hop and no table lookup per call: bound through the table like the
    other six, the population's loop step at P = 4 fell outside the parent's spread (profiles/learner/python_layer_refactor_bench.json, ``first_binding``)."""
    act_entry, push_entry, update_entry = prefix + "act_device", prefix + "push_device", prefix + "update_device"

    def act(self, handle, n_per_member, d_obs, obs_stride, d_ticks, noise, d_action, d_debug=0, stream=0):
        self._chk(getattr(self._lib, act_entry)(handle, int(n_per_member), d_obs, int(obs_stride), d_ticks, int(bool(noise)), d_action, d_debug, stream))

    def push(self, handle, n_per_member, d_obs, d_next_obs, d_final_obs, obs_stride, d_ticks, d_next_ticks, d_action, d_reward, d_terminated, d_truncated,
             stream=0):
        self._chk(getattr(self._lib, push_entry)(handle, int(n_per_member), d_obs, d_next_obs, d_final_obs, int(obs_stride), d_ticks, d_next_ticks, d_action,
                                                 d_reward, d_terminated, d_truncated, stream))

    def update(self, handle, n_updates, lr_q, lr_pi, stream=0):
        """``lr_q`` / ``lr_pi``: one learning rate per member (the library checks the lengths)."""
        lq, lp = np.ascontiguousarray(lr_q, dtype=np.float64).reshape(-1), np.ascontiguousarray(lr_pi, dtype=np.float64).reshape(-1)
        if lq.size != lp.size:
            raise ValueError("lr_q has %d entries, lr_pi %d" % (lq.size, lp.size))
        self._chk(getattr(self._lib, update_entry)(handle, int(n_updates), _dptr(lq), _dptr(lp), int(lq.size), stream))
    return {"act": act, "push": push, "update": update}


for _kind in ("ddpg", "td3"):
    for _name, _method in _continuous_pop_steps(Context._POPS[_kind][0]).items():
        setattr(Context, "%s_pop_%s" % (_kind, _name), _method)

_default_ctx = None


def default_context():
    """Process-wide context on the current HIP device (created on first use)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(-1)
    return _default_ctx
