"""The pieces every group axis shares (groups.split / coincide / summary_by / splitmix64, _capi.CfgTable): the exact messages and values the axes
produced while each carried its own copy, as literals.  No GPU."""
import numpy as np
import pytest

from stmpc_testlib import pkg as _pkg


def _msg(fn, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    return str(e.value)


class _Pop:
    P, n_per_member, n = 2, 6, 12


def test_split_messages_and_values():
    _pkg()
    from rl_mpc_lanemerging_amd import episodes, groups
    assert groups.split(12, 3, 64, "traffic") == (3, 4) and groups.split(3, 3, 64, "traffic") == (3, 1)
    assert groups.split(288, 288, 512, "solver") == (288, 1) and groups.split(12, 3, 64, "control", "controller") == (3, 4)
    assert _msg(groups.split, 12, 0, 64, "traffic") == "traffic must name 1 ... 64 groups, not 0"
    assert _msg(groups.split, 2, 65, 64, "control", "controller") == "control must name 1 ... 64 groups, not 65"        # (the count before the split)
    assert _msg(groups.split, 12, 513, 512, "solver") == "solver must name 1 ... 512 groups, not 513"
    assert _msg(groups.split, 10, 3, 64, "traffic") == "n = 10 environments do not split into 3 traffic groups of equal size"
    assert _msg(groups.split, 2, 3, 64, "control", "controller") == "n = 2 environments do not split into 3 controller groups of equal size"
    assert _msg(groups.split, 13, 3, 512, "solver") == "n = 13 environments do not split into 3 solver groups of equal size"
    assert groups.within(64, 64, "rewards") == 64
    assert _msg(groups.within, 65, 64, "traffic_mix", "traffic types") == "traffic_mix must name 1 ... 64 traffic types, not 65"
    # the three axes' checks are compositions of them
    assert episodes._check_traffic(12, ["low"] * 3, None) == (3, 4) and episodes._check_control(12, [{}] * 3, ["low"] * 3, None) == (3, 4)
    assert episodes._check_solver(12, [{}] * 3, ["low"] * 3, "st") == (3, 4)
    assert _msg(episodes._check_traffic, 12, [], None) == "traffic must name 1 ... 64 groups, not 0"
    assert _msg(episodes._check_traffic, 12, ["low"] * 65, None, 512) == "n = 12 environments do not split into 65 traffic groups of equal size"
    assert _msg(episodes._check_control, 2, [{}] * 3, None, None) == "n = 2 environments do not split into 3 controller groups of equal size"
    assert _msg(episodes._check_solver, 13, [{}] * 3, None, "st") == "n = 13 environments do not split into 3 solver groups of equal size"
    assert _msg(episodes.traffic_mix_cfgs, ["low"] * 65) == "traffic_mix must name 1 ... 64 traffic types, not 65"


def test_coincide_messages_and_order():
    _pkg()
    from rl_mpc_lanemerging_amd import episodes, groups
    assert groups.coincide("control", 3, 4) is None and groups.coincide("control", 2, 6, ["low", "fast"], _Pop) is None
    assert groups.coincide("traffic", 3, 4, policy=object()) is None                       # (a lone policy has no members to pair)
    traffic_msg = "the traffic has 2 groups, the control 3: cell c pairs traffic c with control c, so they must coincide"
    assert _msg(groups.coincide, "control", 3, 4, ["low", "fast"]) == traffic_msg
    assert _msg(groups.coincide, "control", 3, 4, ["low", "fast"], _Pop) == traffic_msg                          # (the traffic before the population)
    assert _msg(groups.coincide, "solver", 3, 4, ["low", "fast"]) == "the traffic has 2 groups, the solver 3: cell c pairs traffic c with solver c, so they must coincide"
    pop_msg = "the population has 2 members of 6 environments, the %s 3 groups of 4: cell c pairs member c with %s c, so they must coincide"
    assert _msg(groups.coincide, "traffic", 3, 4, policy=_Pop) == pop_msg % ("traffic", "traffic")
    assert _msg(groups.coincide, "control", 3, 4, None, _Pop) == pop_msg % ("control", "control")
    assert _msg(groups.coincide, "traffic", 2, 4, policy=_Pop) == ("the population has 2 members of 6 environments, the traffic 2 groups of 4: "
                                                                   "cell c pairs member c with traffic c, so they must coincide")
    assert _msg(episodes._check_traffic, 12, ["low"] * 3, _Pop) == pop_msg % ("traffic", "traffic")
    assert _msg(episodes._check_control, 12, [{}] * 3, ["low"] * 2, _Pop) == traffic_msg
    assert _msg(episodes._check_control, 12, [{}] * 3, None, _Pop) == pop_msg % ("control", "control")
    assert _msg(episodes._check_solver, 12, [{}] * 3, ["low"] * 2, "st") == "the traffic has 2 groups, the solver 3: cell c pairs traffic c with solver c, so they must coincide"
    assert _msg(episodes._check_solver, 12, [{}] * 3, None, "combined") == "solver groups are settings of the ST controller, not of 'combined'"


@pytest.mark.parametrize("name,noun", [("summary_by_member", "members"), ("summary_by_group", "traffic groups"), ("summary_by_control", "controller groups"),
                                       ("summary_by_solver", "solver groups")])
def test_summary_by(name, noun):
    _pkg()
    from rl_mpc_lanemerging_amd import episodes, groups
    stats = {"status": np.zeros(6), "mean_speed": np.arange(6.0), "report": object(), "member": np.arange(6)}
    fn = getattr(episodes, name)
    assert fn(stats, 3) == [{"mean_speed": 0.5}, {"mean_speed": 2.5}, {"mean_speed": 4.5}] == groups.summary_by(stats, 3, noun)
    assert fn(stats, 1) == [episodes.summary(stats)] == [{"mean_speed": 2.5}]
    assert _msg(fn, stats, 4) == "6 environments do not split into 4 %s" % noun
    assert _msg(fn, stats, 0) == "6 environments do not split into 0 %s" % noun


def test_cfg_tables():
    _pkg()
    import ctypes as C
    from rl_mpc_lanemerging_amd import _capi as capi
    # ParamsTable copies its rows
    a, b = capi.Params(ds=0.05, d_w=1.0), capi.Params(ds=0.1, d_w=2.0)
    t = capi.ParamsTable([a, b])
    assert isinstance(t, capi.CfgTable) and len(t) == 2 and [p.ds for p in t] == [0.05, 0.1] and t[1].d_w == 2.0 and t.params is t.rows
    assert t[0] is not a and isinstance(t[0], capi.Params) and isinstance(t.array, capi.Params * 2)
    a.ds = 9.0
    assert t[0].ds == 0.05 and t.array[0].ds == 0.05 and bytes(t.array[1]) == bytes(b)
    assert capi.ParamsTable.of(t) is t and isinstance(capi.ParamsTable.of([a]), capi.ParamsTable) and len(capi.ParamsTable.of((a,))) == 1
    # the other two keep the caller's objects (alive, with what they point to) and hand them back
    route = np.array([[0.0, 0.0], [1.0, 0.5], [2.0, 0.5]])
    s0, s1 = capi.SimCfg(tick_length=0.2, seed=3).set_route(route), capi.SimCfg(tick_length=0.2, seed=4)
    st = capi.SimCfgTable([s0, s1])
    assert isinstance(st, capi.CfgTable) and len(st) == 2 and st[0] is s0 and list(st) == [s0, s1] and st.cfgs is st.rows and st.cfgs[:1] == [s0]
    assert isinstance(st.array, capi.SimCfg * 2) and bytes(st.array[0]) == bytes(s0) and st.array[1].seed == 4
    assert C.addressof(st.array[0].ego_route_xy.contents) == s0._route.ctypes.data and st.array[0].ego_route_n == 3
    s1.seed = 8                                                  # (the array is the table's own: filled once, at construction)
    assert st[1].seed == 8 and st.array[1].seed == 4
    assert capi.SimCfgTable.of(st) is st and capi.SimCfgTable.of([s0])[0] is s0
    e0 = capi.EnvCfg(action_mode=1, reward_function=2, crash_reward=-10.0)
    e0._actions = np.array([-1.0, 0.0, 1.0])
    e0.action_values, e0.n_action_values = e0._actions.ctypes.data_as(C.POINTER(C.c_double)), 3
    e1 = capi.EnvCfg(action_mode=1, reward_function=0)
    et = capi.EnvCfgTable([e0, e1])
    assert isinstance(et, capi.CfgTable) and len(et) == 2 and et[0] is e0 and list(et) == [e0, e1] and et.cfgs is et.rows
    assert isinstance(et.array, capi.EnvCfg * 2) and bytes(et.array[0]) == bytes(e0) and [et.array[0].action_values[i] for i in range(3)] == [-1.0, 0.0, 1.0]
    assert capi.EnvCfgTable.of(et) is et and capi.EnvCfgTable.of([e1])[0] is e1
    # a table is of its own class only; an empty one still has an array to point at
    assert not isinstance(st, capi.ParamsTable) and not isinstance(t, capi.SimCfgTable) and not isinstance(et, capi.SimCfgTable)
    for cls in (capi.ParamsTable, capi.SimCfgTable, capi.EnvCfgTable):
        empty = cls([])
        assert len(empty) == 0 and list(empty) == [] and len(empty.array) == 1


def test_splitmix64_and_the_seeds_drawn_with_it():
    _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, groups, learner, vec_env
    assert [groups.splitmix64(z) for z in (0, 1, 0x9E3779B97F4A7C15, 2 ** 64 - 1)] == [0x0, 0x5692161D100B05E5, 0xE220A8397B1DCDAF, 0xB4D055FCF2CBBD7B]
    assert learner.hash3(5, 3, 7) == 0x3B8CE72583150241
    cases = ((7, 1), (7, 2), (2 ** 64 - 1, 3), (123456789, 4000000000))
    assert [vec_env.episode_seed(s, e) for s, e in cases] == [0x63CBE1E459320DD7, 0x44C3CD7F43C661C, 0x382FF84CB27281E9, 0x3306FBA541FB23C4]
    for s in (0, 5, 2 ** 63 + 1, 2 ** 64 - 1):
        assert vec_env.episode_seed(s, 0) == s == capi.env_episode_seed(s, 0)
    for s, e in cases + ((0, 1), (2 ** 63 + 1, 65536)):
        assert vec_env.episode_seed(s, e) == capi.env_episode_seed(s, e)


def test_traffic_mix_draw_with_zero_weights():
    _pkg()
    from rl_mpc_lanemerging_amd import _capi as capi, vec_env
    want = {(1, 0, 2): ([0.3333333333333333, 0.3333333333333333, 1.0], [2, 2, 0, 2, 0, 0, 2, 0, 2, 2, 2, 2, 2, 0, 2, 0, 2, 0, 0, 2, 2, 0, 2, 0]),
            (1, 2, 0): ([0.3333333333333333, 1.0, 1.0], [1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0])}
    for weights, (cum, draws) in want.items():
        assert vec_env.traffic_mix_cum(weights) == cum
        cells = [(env, ep) for env in range(4) for ep in range(6)]
        assert [vec_env.traffic_mix_draw(9, env, ep, cum) for env, ep in cells] == draws == [capi.traffic_mix_draw(9, env, ep, cum) for env, ep in cells]
        for seed, env, ep in ((0, 0, 0), (2 ** 64 - 1, 1000, 2 ** 32 - 1), (12345, 95, 70000)):
            t = vec_env.traffic_mix_draw(seed, env, ep, cum)
            assert t == capi.traffic_mix_draw(seed, env, ep, cum) and weights[t] > 0            # (a type of weight 0 is never drawn, wherever it stands)
