"""Host twins of the reference's gym-environment arithmetic: the four reward functions ``dqn.get_reward_function`` picks (dqn.py:449-563,
rl.py:168-174) and the action handling of the three environments of merge_gym.py (83-100, 193-227).

Plain Python in the reference's operation order: they are pinned to golden vectors recorded from the reference's own functions
(golden_env.npz) and serve as checkers of the kernels in csrc/stmpc_env_kernels.hpp.  One difference is selectable: the reference
squares with ``x ** 2``, a libm ``pow`` call that glibc >= 2.28 does not round correctly (about 0.1 % of arguments land one ulp off ``x * x``);
the kernels square with the correctly rounded ``x * x``.  ``square=pow2`` (the default) is the reference, ``square=mul2`` the kernels.
"""
import math

from . import control
from .config import Settings


def pow2(x):
    return x ** 2


def mul2(x):
    return x * x


def closest_cars(ego_x, other_xs, other_speeds=None, other_accelerations=None):
    """HighwayState.get_closest_cars, prediction.py:162-182: (car_front, car_behind) in the list order of ``other_xs`` (front to back)."""
    index_behind = -1
    index_front = -1
    last_index = -1
    for other_index, x in enumerate(other_xs):
        if x < ego_x:
            index_behind = other_index
            break
        last_index = other_index
    if last_index != -1:
        index_front = last_index
    sp = other_speeds if other_speeds is not None else [0.0] * len(other_xs)
    ac = other_accelerations if other_accelerations is not None else [0.0] * len(other_xs)
    car_front = (other_xs[index_front], sp[index_front], ac[index_front]) if index_front != -1 else None
    car_behind = (other_xs[index_behind], sp[index_behind], ac[index_behind]) if index_behind != -1 else None
    return car_front, car_behind


def continuous_reward(ego_position, ego_speed, ego_acceleration, other_xs, jerk, crashed, arrived, S=Settings, square=pow2):
    """dqn.continuous_reward, dqn.py:463-505."""
    absolute_metric = 0
    safety_metric = 0
    efficiency_metric = 0
    smoothness_metric = 0
    if crashed:
        absolute_metric = -10
    elif arrived:
        absolute_metric = 10
    else:
        smoothness_metric = - abs(jerk) * S.TICK_LENGTH
        car_ahead, car_behind = closest_cars(ego_position[0], other_xs)
        ego_x, ego_y = ego_position
        ego_s = control.get_ego_s(ego_position)
        if ego_s > 0:
            front_distance = car_ahead[0] - ego_x - S.CAR_LENGTH if car_ahead is not None else math.inf
            back_distance = ego_x - car_behind[0] - S.CAR_LENGTH if car_behind is not None else math.inf
            min_distance = min(front_distance, back_distance)
            if min_distance < S.MIN_FOLLOW_DISTANCE:
                safety_metric = -1
            elif min_distance == math.inf:
                safety_metric = 0
            elif math.isnan(min_distance):
                safety_metric = 0
            else:
                safety_metric = -1 / min_distance
            safety_metric *= S.TICK_LENGTH
        efficiency_metric = -S.TICK_LENGTH * abs(ego_speed - S.DESIRED_SPEED)
    return S.WT_SMOOTH * smoothness_metric + S.WT_SAFE * safety_metric + S.WT_EFFICIENT * efficiency_metric + absolute_metric


def st_reward(ego_position, ego_speed, ego_acceleration, other_xs, jerk, crashed, arrived, S=Settings, square=pow2):
    """dqn.st_reward, dqn.py:508-554."""
    absolute_metric = 0
    speed_metric = 0
    acceleration_metric = 0
    jerk_metric = 0
    distance_metric = 0
    if crashed:
        absolute_metric = -10
    elif arrived:
        absolute_metric = 10
    else:
        jerk_metric = -square(jerk) * S.TICK_LENGTH
        car_ahead, car_behind = closest_cars(ego_position[0], other_xs)
        ego_x, ego_y = ego_position
        ego_s = control.get_ego_s(ego_position)
        speed_metric = -S.TICK_LENGTH * square(ego_speed - S.DESIRED_SPEED)
        acceleration_metric = -S.TICK_LENGTH * square(ego_acceleration)
        if ego_s > 0:
            front_distance = car_ahead[0] - ego_x - S.CAR_LENGTH if car_ahead is not None else math.inf
            back_distance = ego_x - car_behind[0] - S.CAR_LENGTH if car_behind is not None else math.inf
            min_distance = min(front_distance, back_distance)
            if min_distance < S.MIN_FOLLOW_DISTANCE:
                distance_metric = -2 / max(min_distance, 1)
            elif min_distance == math.inf:
                distance_metric = 0
            elif math.isnan(min_distance):
                distance_metric = 0
            else:
                distance_metric = -1 / min_distance
            distance_metric *= S.TICK_LENGTH
    return S.ALT_A_WEIGHT * acceleration_metric + S.ALT_D_WEIGHT * distance_metric + \
        S.ALT_J_WEIGHT * jerk_metric + S.ALT_V_WEIGHT * speed_metric + absolute_metric


def slotted_reward(ego_position, ego_speed, ego_acceleration, other_xs, jerk, crashed, arrived, S=Settings, square=pow2):
    """rl.slotted_reward, rl.py:168-174."""
    if crashed:
        return S.CRASH_REWARD
    elif arrived:
        return S.SUCCESS_REWARD
    else:
        return S.TIME_REWARD * S.TICK_LENGTH


def slotted_reward_with_jerk(ego_position, ego_speed, ego_acceleration, other_xs, jerk, crashed, arrived, S=Settings, square=pow2):
    """dqn.slotted_reward_with_jerk, dqn.py:557-563."""
    if crashed:
        return S.CRASH_REWARD
    elif arrived:
        return S.SUCCESS_REWARD
    else:
        return S.TIME_REWARD * S.TICK_LENGTH - S.ALT_J_WEIGHT * square(jerk) * S.TICK_LENGTH


REWARD_FUNCTIONS = {"Continuous": continuous_reward, "Slotted": slotted_reward, "Slotted Jerk": slotted_reward_with_jerk, "ST": st_reward}


def get_reward_function(name=None):
    """dqn.get_reward_function, dqn.py:449-460: ValueError for an unknown name."""
    name = Settings.REWARD_FUNCTION if name is None else name
    if name not in REWARD_FUNCTIONS:
        raise ValueError("Invalid reward function {} specified in settings.".format(name))
    return REWARD_FUNCTIONS[name]


def ego_speed_from_jerk(current_speed, current_acceleration, jerk, S=Settings):
    """control.get_ego_speed_from_jerk, control.py:160-171."""
    new_acceleration = current_acceleration + jerk * S.TICK_LENGTH
    if new_acceleration > S.MAX_POSITIVE_ACCELERATION:
        new_acceleration = S.MAX_POSITIVE_ACCELERATION
    if new_acceleration < S.MAX_NEGATIVE_ACCELERATION:
        new_acceleration = S.MAX_NEGATIVE_ACCELERATION
    new_speed = current_speed + new_acceleration * S.TICK_LENGTH
    if new_speed > S.MAX_SPEED:
        new_speed = S.MAX_SPEED
    if new_speed < 0:
        new_speed = 0
    return new_speed


def _clip(x, lo, hi):
    return min(max(x, lo), hi)              # np.clip of a scalar


def handle_jerk(speed, acceleration, previous_acceleration, selected_jerk, S=Settings):
    """JerkEnv._handle_jerk + control.set_ego_jerk (merge_gym.py:83-96, control.py:174-179) -> (commanded speed, projected jerk, invalid-action
    reward).  ``speed`` / ``acceleration``: the ego's state now (previous_state.ego_speed and what TraCI reports are the same state here)."""
    penalty = S.INVALID_ACTION_PENALTY
    projected_acceleration = previous_acceleration + selected_jerk * S.TICK_LENGTH
    projected_speed = speed + projected_acceleration * S.TICK_LENGTH
    if projected_acceleration > S.MAX_POSITIVE_ACCELERATION or projected_acceleration < S.MAX_NEGATIVE_ACCELERATION:
        invalid_action_reward = penalty * S.TICK_LENGTH
        projected_acceleration = _clip(projected_acceleration, S.MAX_NEGATIVE_ACCELERATION, S.MAX_POSITIVE_ACCELERATION)
    elif projected_speed > S.MAX_SPEED or projected_speed < 0:
        invalid_action_reward = penalty * S.TICK_LENGTH
        projected_speed = _clip(projected_speed, 0, S.MAX_SPEED)
        projected_acceleration = (projected_speed - speed) / S.TICK_LENGTH
    else:
        invalid_action_reward = 0
    projected_jerk = (projected_acceleration - previous_acceleration) / S.TICK_LENGTH
    return ego_speed_from_jerk(speed, acceleration, selected_jerk, S), projected_jerk, invalid_action_reward


def handle_acceleration(speed, acceleration, previous_acceleration, selected_acceleration, S=Settings):
    """AccelerationEnv._do_action, merge_gym.py:193-214 -> (commanded speed, projected jerk, invalid-action reward)."""
    penalty = S.INVALID_ACTION_PENALTY
    projected_acceleration = selected_acceleration
    projected_speed = speed + projected_acceleration * S.TICK_LENGTH
    projected_jerk = (projected_acceleration - previous_acceleration) / S.TICK_LENGTH
    if projected_jerk > S.MAXIMUM_POSITIVE_JERK:
        return ego_speed_from_jerk(speed, acceleration, S.MAXIMUM_POSITIVE_JERK, S), S.MAXIMUM_POSITIVE_JERK, penalty * S.TICK_LENGTH
    elif projected_jerk < S.MINIMUM_NEGATIVE_JERK:
        return ego_speed_from_jerk(speed, acceleration, S.MINIMUM_NEGATIVE_JERK, S), S.MINIMUM_NEGATIVE_JERK, penalty * S.TICK_LENGTH
    elif projected_speed > S.MAX_SPEED or projected_speed < 0:
        projected_speed = _clip(projected_speed, 0, S.MAX_SPEED)
        projected_acceleration = (projected_speed - speed) / S.TICK_LENGTH
        projected_jerk = (projected_acceleration - previous_acceleration) / S.TICK_LENGTH
        return projected_speed, projected_jerk, penalty * S.TICK_LENGTH
    return projected_speed, projected_jerk, 0


def handle_action(env_id, speed, acceleration, previous_acceleration, action, S=Settings):
    """The action handling of env ``env_id`` (merge_gym.py:98-100, 193-227): a jerk for the continuous env, an index for the discrete ones."""
    if env_id == "sumo-jerk-continuous-v0":
        return handle_jerk(speed, acceleration, previous_acceleration, action, S)
    if env_id == "sumo-jerk-v0":
        return handle_jerk(speed, acceleration, previous_acceleration, S.JERK_VALUES_DQN[action], S)
    if env_id == "sumo-accel-v0":
        return handle_acceleration(speed, acceleration, previous_acceleration, S.ACCELERATION_VALUES_DQN[action], S)
    raise ValueError("unknown gym environment %r" % (env_id,))
