"""The dynamic-window controller of the unicycle robot (cn_dwa_predict, cn_scripted_dwa, the policy 'dwa').

The controller is this project's definition (include/crowdnav.h); policy_factory.dwa_predict restates it on Python
floats and is what the device is compared with. The device's sin / cos may differ from the C library's in the last
bit, so costs are compared to rtol 1e-9 on `sharp` candidates (none of the walk's comparisons c_k < 0, g_k < r within
1e-9 of equality) and choices where the host's best two costs differ by more than 1e-6; everything between device
paths (cn_robot_act against cn_dwa_predict, rollouts against the eager loop) is compared bit for bit."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config, make_cn_config, make_varied_cn_configs
from crowdnav_dsrnn_amd.policy_factory import DWA_DEFAULTS, DWA_GRID, ScriptedRobot, dwa_params, dwa_predict
from tests import rollout_noise_ref as ref_noise

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
DEV = "cuda:0"
OBS = ("robot_node", "temporal_edges", "spatial_edges")
RECORDS = ("reward", "done", "event", "info", "ep_return", "ep_len")
ROWS = ("actions",) + OBS + RECORDS
GRID32 = np.array(DWA_GRID, np.float64).astype(np.float32)


def _config(N=5, kin="unicycle", dwa=True, time_limit=2, policy="srnn", rng="mt19937"):
    c = clone_config(Config())
    c.sim.human_num = N
    c.robot.policy = policy
    c.robot.scripted_dwa = dwa
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.env.rng = rng
    if time_limit is not None:
        c.env.time_limit = time_limit
    return c


def _self(px=0.0, py=0.0, r=0.3, gx=5.0, gy=0.0, vpref=1.0, theta=0.0):
    return np.array([[px, py, 0.0, 0.0, r, gx, gy, vpref, theta]])


# ---- CPU: the host restatement's known answers ---------------------------------------------------
def test_grid_is_the_steps_clip_range_and_never_below_the_freeze_threshold():
    g = np.array(DWA_GRID)
    assert len(g) == 8 and g[0] == -0.1 and g[7] == 0.1 and (np.diff(g) > 0).all()
    assert g.tolist() == [(0.1 * (2 * k - 7)) / 7 for k in range(8)]
    assert (np.abs(g) >= 0.1 / 7 - 1e-15).all() and (np.abs(GRID32) >= 1e-4).all()   # all 64 dtheta: 8 values
    assert (np.abs(GRID32) <= np.float32(0.1)).all()                                 # the step's clip is a no-op
    a, ch, co = dwa_predict(_self(), [0.0], np.zeros((1, 0, 5)), 0.25)
    assert a.dtype == np.float32 and a.shape == (1, 2) and ch.dtype == np.int32 and co.shape == (1, 64)


def test_no_humans_goal_ahead_accelerates_with_the_smallest_turn():
    a, ch, co = dwa_predict(_self(gx=5.0), [0.0], np.zeros((1, 0, 5)), 0.25)
    assert a[0, 0] == np.float32(0.1) and abs(a[0, 1]) == GRID32[4] and ch[0] >> 3 == 7 and (ch[0] & 7) in (3, 4)
    assert co[0].min() == co[0, ch[0]] and np.isfinite(co).all()


def test_goal_behind_turns_as_hard_as_it_can():
    """At v = 0.5 every candidate moves forwards (v1 in [0.4, 0.6]), so the only way to lose less ground is to turn.
    (From rest the grid holds reversing candidates, and the controller backs up towards a goal behind it.)"""
    for v in (0.5, 1.0):
        a, ch, co = dwa_predict(_self(gx=-5.0), [v], np.zeros((1, 0, 5)), 0.25)
        assert abs(a[0, 1]) == np.float32(0.1) and a[0, 0] == np.float32(-0.1), (v, a)
    a, ch, co = dwa_predict(_self(gx=-5.0), [0.0], np.zeros((1, 0, 5)), 0.25)
    assert a[0, 0] == np.float32(-0.1) and abs(a[0, 1]) == GRID32[4]      # backs up, straight


def test_a_human_on_the_straight_arc_at_step_two_is_avoided():
    """v = 2 clipped to v_pref = 1 at time_step 1: every candidate advances 1 m per step, the straight ones are at
    (2, ~0.03) after two steps, where a human of radius 0.05 stands (robot radius 0.1: no contact at step 1, 1 m
    away). The hardest turn passes 0.2 m beside it."""
    H = 8
    hum = np.array([[[2.0, 0.0, 0.0, 0.0, 0.05]]])
    a, ch, co, d = dwa_predict(_self(r=0.1, gx=10.0), [2.0], hum, 1.0, {"horizon": H}, detail=True)
    straight = [8 * k + b for k in range(8) for b in (3, 4)]
    assert (d["hit"][0, straight] == H - 1).all()
    assert d["hit"][0, ch[0]] == 0 and (ch[0] & 7) in (0, 7)
    assert co[0, ch[0]] < 100.0 and co[0, straight].min() >= 100.0 * (H - 1)   # w_col = 100 per step left


def test_goal_within_reach_at_the_first_step_ends_the_walk():
    """H = 1, goal 0.5 m ahead, radius 0.3, v = 0.9: the first step covers 0.2 m (dv = -0.1: 0.3000x m short of the
    goal, not inside) to 0.25 m; gterm is 0 exactly for the candidates whose first position is within the radius."""
    s = _self(gx=0.5, r=0.3)
    a, ch, co, d = dwa_predict(s, [0.9], np.zeros((1, 0, 5)), 0.25, {"horizon": 1}, detail=True)
    inside = np.zeros(64, bool)
    for c in range(64):
        dv, dth = DWA_GRID[c >> 3], DWA_GRID[c & 7]
        R = min(max(0.9 + dv, -1.0), 1.0) / (dth / 0.25)
        x, y = R * math.sin(dth), R - R * math.cos(dth)
        inside[c] = math.hypot(x - 0.5, y) < 0.3
    assert inside.any() and not inside.all() and not inside[:8].any()
    assert (d["gterm"][0, inside] == 0).all() and (d["gterm"][0, ~inside] >= 0.3).all()
    assert (co[0, inside] == 0).all() and inside[ch[0]]
    # with a longer horizon the slow candidates reach it at step 2 and stop there as well
    d8 = dwa_predict(s, [0.9], np.zeros((1, 0, 5)), 0.25, {"horizon": 8}, detail=True)[3]
    assert (d8["gterm"][0] == 0).all()


def test_parameter_rule():
    assert dwa_params() == DWA_DEFAULTS and dwa_params(True) == DWA_DEFAULTS
    assert dwa_params({"horizon": 12})["horizon"] == 12 and dwa_params({"horizon": 12})["w_col"] == DWA_DEFAULTS["w_col"]
    for bad in ({"horizon": 0}, {"horizon": 17}, {"d_safe": 0.0}, {"d_safe": -1.0}, {"w_goal": float("nan")},
                {"w_clear": float("inf")}, {"w_col": float("-inf")}, {"d_safe": float("inf")}, {"horizons": 3}):
        with pytest.raises(ValueError):
            dwa_params(bad)


# ---- CPU: config plumbing and the ABI ------------------------------------------------------------
class _VenvStub:
    """What ScriptedRobot reads before it touches the engine (no GPU behind it)."""

    num_envs = 8
    obs_mode = "srnn"

    def __init__(self, config):
        self.config = config

    def __getattr__(self, name):
        raise AssertionError("the check must come before the engine is touched (%s)" % name)


def test_scripted_robot_takes_dwa_only_on_a_unicycle_config_with_the_optin():
    assert Config().robot.scripted_dwa is None and "dwa" in ScriptedRobot.NAMES
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(_VenvStub(_config(kin="holonomic")), "dwa")
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(_VenvStub(_config(dwa=None)), "dwa")
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot.check_rollout(_VenvStub(_config(dwa=None)), "dwa")
    c = _config()
    c.robot.scripted_unicycle = False                      # (no tracking law involved)
    a = ScriptedRobot(_VenvStub(c), "dwa")
    assert a.name == "dwa" and a.base.human_num == 5
    ScriptedRobot.check_rollout(_VenvStub(_config(dwa={"horizon": 6})), "dwa")
    cv = _config()
    cv.sim.human_nums = [3, 5]
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(_VenvStub(cv), "dwa")
    cv.sim.human_nums_scripted = True
    ScriptedRobot(_VenvStub(cv), "dwa")
    # the opt-in does not open the other controllers on a unicycle config
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(_VenvStub(_config()), "orca")


def test_header_binding_and_export_list_agree_on_the_two_functions():
    from crowdnav_dsrnn_amd import _lib, build
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    txt = open(os.path.join(REPO, "include", "crowdnav.h")).read()
    want = {"cn_dwa_predict": ["void*", "int64_t", "int", "constdouble*", "constdouble*", "constdouble*", "double",
                               "constcn_dwa_params*", "float*", "int32_t*", "double*"],
            "cn_scripted_dwa": ["cn_engine*", "constcn_dwa_params*"]}
    build.build()
    L = _lib.lib()
    for fn, types in want.items():
        m = re.search(r"^int %s\((.*?)\);" % fn, txt, re.S | re.M)
        assert m, "include/crowdnav.h does not declare %s" % fn
        params = [p.strip() for p in m.group(1).split(",")]
        assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == types
        assert fn in _lib.EXPORTED
        assert hasattr(L, fn) and len(getattr(L, fn).argtypes) == len(params)
    body = re.search(r"typedef struct cn_dwa_params \{(.*?)\} cn_dwa_params;", txt, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in abi.DwaParams._fields_] == ["horizon"] + [k for k in DWA_DEFAULTS if k != "horizon"]
    assert ctypes.sizeof(abi.DwaParams) == 40              # int32 + padding, four doubles
    assert re.search(r"^#define CN_ROBOT_DWA 2$", txt, re.M) and abi.ROBOT_DWA == 2
    assert CrowdNavEngine.ROBOT_POLICIES == {"orca": 0, "social_force": 1, "dwa": 2}
    # argument checks that launch nothing
    p = abi.DwaParams(**DWA_DEFAULTS)
    assert L.cn_scripted_dwa(None, ctypes.byref(p)) == EINVAL and b"null engine" in L.cn_last_error()
    assert L.cn_dwa_predict(None, 0, 0, 16, 16, None, 0.25, ctypes.byref(p), 16, None, None) == EINVAL
    assert L.cn_dwa_predict(None, 4, 0, 16, 16, None, 0.25, None, 16, None, None) == EINVAL
    assert L.cn_dwa_predict(None, 4, 65, 16, 16, 16, 0.25, ctypes.byref(p), 16, None, None) == EINVAL
    assert L.cn_dwa_predict(None, 4, 2, 16, 16, None, 0.25, ctypes.byref(p), 16, None, None) == EINVAL
    for k, v in (("horizon", 0), ("horizon", 17), ("d_safe", 0.0), ("w_goal", float("nan")), ("w_col", float("inf"))):
        q = abi.DwaParams(**dict(DWA_DEFAULTS, **{k: v}))
        assert L.cn_dwa_predict(None, 4, 0, 16, 16, None, 0.25, ctypes.byref(q), 16, None, None) == EINVAL, (k, v)
        assert b"cn_dwa_predict" in L.cn_last_error()


# ---- GPU -----------------------------------------------------------------------------------------
def _engine(c, E, dwa=True, **kw):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    return CrowdNavEngine(make_cn_config(c, num_envs=E, nenv=kw.pop("nenv", E), phase="train", **kw), DEV,
                          scripted_dwa=dwa)


def _random_states(rs, n, M):
    """Positions and goals in +-6, speeds in +-1, radii 0.2 .. 0.5, headings in [0, 2 pi), v_pref 1."""
    s = np.zeros((n, 9))
    s[:, 0:2] = rs.uniform(-6, 6, (n, 2))
    s[:, 2:4] = rs.uniform(-1, 1, (n, 2))
    s[:, 4] = rs.uniform(0.2, 0.5, n)
    s[:, 5:7] = rs.uniform(-6, 6, (n, 2))
    s[:, 7] = 1.0
    s[:, 8] = rs.uniform(0, 2 * np.pi, n)
    v = rs.uniform(-1, 1, n)
    o = np.zeros((n, M, 5))
    o[:, :, 0:2] = rs.uniform(-6, 6, (n, M, 2))
    o[:, :, 2:4] = rs.uniform(-1, 1, (n, M, 2))
    o[:, :, 4] = rs.uniform(0.2, 0.5, (n, M))
    # half of the humans near the robot's path, so that collisions and the clearance term take part
    near = rs.rand(n, M) < 0.5
    o[:, :, 0:2] = np.where(near[..., None], s[:, None, 0:2] + rs.uniform(-1.5, 1.5, (n, M, 2)), o[:, :, 0:2])
    return s, v, o


def _device_predict(eng, s, v, o, params):
    import torch

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)   # noqa: E731
    act, ch, co = eng.dwa_predict(t(s), t(v), t(o), 0.25, params)
    torch.cuda.synchronize()
    return act.cpu().numpy(), ch.cpu().numpy(), co.cpu().numpy()


@pytest.fixture(scope="module")
def any_engine():
    eng = _engine(_config(5), 8)
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 8, 16])
def test_gpu_predict_equals_the_host_restatement(any_engine, H):
    """n in {1, 5, 67} (a lone wave, a workgroup and a wave, 16 workgroups and 3 waves) x M in {0, 1, 5, 11}."""
    params = {"horizon": H}
    rs = np.random.RandomState(20261020 + H)
    total = nonsharp = decided = hits = reached = 0
    for n in (1, 5, 67):
        for M in (0, 1, 5, 11):
            s, v, o = _random_states(rs, n, M)
            act_h, ch_h, co_h, d = dwa_predict(s, v, o, 0.25, params, detail=True)
            sharp = d["sharp"]
            total += sharp.size
            nonsharp += int((~sharp).sum())
            assert nonsharp * 10000 <= total, (n, M, nonsharp, total)   # at most 1 in 10,000, on the host's values
            act, ch, co = _device_predict(any_engine, s, v, o, params)
            err = np.abs(co - co_h) / np.maximum(np.abs(co_h), 1e-300)
            print("H %d n %d M %d: max rel cost error on sharp candidates %.3g" % (H, n, M, err[sharp].max()))
            assert np.isclose(co[sharp], co_h[sharp], rtol=1e-9, atol=0.0).all(), (n, M)
            best = co_h.min(axis=1)
            picked = co_h[np.arange(n), ch]
            assert (picked <= best + 1e-9 * (1 + np.abs(best))).all(), (n, M)
            second = np.sort(co_h, axis=1)[:, 1]
            clear = second - best > 1e-6
            assert (ch[clear] == ch_h[clear]).all(), (n, M)
            decided += int(clear.sum())
            assert ch.dtype == np.int32 and ((ch >= 0) & (ch < 64)).all()
            want = np.stack([GRID32[ch >> 3], GRID32[ch & 7]], axis=1)
            assert act.dtype == np.float32 and act.tobytes() == want.tobytes(), (n, M)
            hits += int((d["hit"] > 0).sum())
            reached += int((d["gterm"] == 0).sum())
    assert decided >= 0.9 * 73 * 4 and hits > 100, (decided, hits, reached)   # the cases hold what they were built for
    assert H == 1 or reached > 0, reached


@pytest.mark.gpu
def test_gpu_ties_go_to_the_lowest_candidate(any_engine):
    """w_goal = 0: without humans, and with humans farther than d_safe from every arc, all 64 costs are exactly 0, so
    the choice is candidate 0; two envs mirrored about the heading (goal dead ahead) behave alike. With w_goal back
    on, a mirror pair of candidates whose costs are bitwise equal on the device resolves to the lower index."""
    s = np.concatenate([_self(theta=0.0, gx=4.0), _self(theta=0.0, gx=4.0)])
    v = np.array([0.3, 0.3])
    far = np.array([[[0.0, 5.0, 0.0, 0.0, 0.3], [3.0, -6.0, 0.0, 0.0, 0.3]],
                    [[0.0, -5.0, 0.0, 0.0, 0.3], [3.0, 6.0, 0.0, 0.0, 0.3]]])        # env 1 = env 0 mirrored in y
    for o in (np.zeros((2, 0, 5)), far):
        act, ch, co = _device_predict(any_engine, s, v, o, {"w_goal": 0.0})
        assert (co == 0).all() and (ch == 0).all()
        assert act.tobytes() == np.array([[GRID32[0], GRID32[0]]] * 2, np.float32).tobytes()
        assert (dwa_predict(s, v, o, 0.25, {"w_goal": 0.0})[1] == 0).all()
    act, ch, co = _device_predict(any_engine, s, v, far, None)
    for e in range(2):
        ties = np.nonzero(co[e] == co[e].min())[0]
        assert ch[e] == ties[0], (e, ch[e], ties)


def _state_arrays(sv):
    s = np.stack([sv.r_px, sv.r_py, sv.r_vx, sv.r_vy, sv.r_radius, sv.r_gx, sv.r_gy, sv.r_vpref, sv.r_theta], axis=1)
    o = np.stack([sv.b_px, sv.b_py, sv.b_vx, sv.b_vy, sv.b_r], axis=2)
    return np.ascontiguousarray(s, np.float64), np.array(sv.r_dv, np.float64), np.ascontiguousarray(o, np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 11])
@pytest.mark.parametrize("E", [8, 67])
def test_gpu_robot_act_equals_predict_on_the_same_state(E, N):
    """After a reset (r_dv = 0) and after 3 steps of the controller's own actions (r_dv != 0, humans seen): bit for bit.
    The engine has no cn_scripted_unicycle: the controller needs no tracking law."""
    import torch

    c = _config(N, time_limit=None)
    eng = _engine(c, E, nenv=131)
    eng.reset()
    moving = 0
    for where in ("reset", "after 3 steps"):
        s, v, o = _state_arrays(eng.get_state())
        want = _device_predict(eng, s, v, o, None)[0]
        got = eng.robot_act("dwa")
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (E, N, where)
        assert np.isin(got, GRID32).all()
        if where == "reset":
            assert (v == 0).all()
            for _ in range(3):
                eng.step(eng.robot_act("dwa"))
        else:
            moving = int((v != 0).sum())
    assert moving > E // 2, moving
    eng.close()


@pytest.mark.gpu
def test_gpu_mixed_engine_rows_land_at_their_envs():
    import torch

    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    NUMS, E = [3, 5], 10
    c = _config(5, time_limit=None)
    c.sim.human_nums, c.sim.human_nums_scripted = list(NUMS), True
    cfgs, eg = make_varied_cn_configs(c, NUMS, E, phase="train", seed=7, rng="mt19937")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=True, scripted_dwa=True)
    mixed.reset()
    for where in range(2):
        got = torch.full((E, 2), 7.0, device=DEV)
        mixed.robot_act("dwa", out=got)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        seen = np.zeros(E, bool)
        for rows, sv in mixed.get_state():
            s, v, o = _state_arrays(sv)
            assert o.shape[1] == NUMS[int(rows[0]) % 2]
            want = _device_predict(mixed, s, v, o, None)[0]
            assert got[rows].tobytes() == want.tobytes(), (where, rows)
            seen[rows] = True
        assert seen.all()
        for _ in range(3):
            mixed.step(mixed.robot_act("dwa"))
    mixed.close()


@pytest.mark.gpu
def test_gpu_error_codes():
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    L = _lib.lib()
    E = 8
    out = torch.zeros((E, 2), device=DEV)
    good = abi.DwaParams(**DWA_DEFAULTS)
    eng = _engine(_config(5), E, dwa=None)
    eng.reset()
    assert L.cn_robot_act(eng._h, None, 2, out.data_ptr()) == EINVAL                # before the opt-in: as ever
    with pytest.raises(RuntimeError):
        eng.rollout("dwa", 2)
    for k, v in (("horizon", 0), ("horizon", 17), ("horizon", -3), ("d_safe", 0.0), ("d_safe", -0.5),
                 ("d_safe", float("nan")), ("w_goal", float("nan")), ("w_clear", float("inf")),
                 ("w_col", float("-inf"))):
        bad = abi.DwaParams(**dict(DWA_DEFAULTS, **{k: v}))
        assert L.cn_scripted_dwa(eng._h, ctypes.byref(bad)) == EINVAL, (k, v)
        assert b"cn_scripted_dwa" in L.cn_last_error()
        assert L.cn_robot_act(eng._h, None, 2, out.data_ptr()) == EINVAL            # a refused opt-in enables nothing
    assert L.cn_scripted_dwa(eng._h, ctypes.byref(good)) == 0
    assert L.cn_robot_act(eng._h, None, 2, out.data_ptr()) == 0
    assert L.cn_robot_act(eng._h, None, 2, None) == EINVAL
    assert L.cn_robot_act(eng._h, None, 3, out.data_ptr()) == EINVAL
    # policies 0 and 1 keep their own rule: this unicycle engine has no cn_scripted_unicycle
    assert L.cn_robot_act(eng._h, None, 0, out.data_ptr()) == EUNSUPPORTED and b"holonomic" in L.cn_last_error()
    assert L.cn_robot_act(eng._h, None, 1, out.data_ptr()) == EUNSUPPORTED
    assert L.cn_scripted_dwa(eng._h, None) == 0
    assert L.cn_robot_act(eng._h, None, 2, out.data_ptr()) == EINVAL                # after cn_scripted_dwa(eng, NULL)
    with pytest.raises(RuntimeError):
        eng.robot_act("dwa")
    eng.close()
    holo = CrowdNavEngine(make_cn_config(_config(5, kin="holonomic", dwa=None), num_envs=E), DEV)
    assert L.cn_scripted_dwa(holo._h, ctypes.byref(good)) == EUNSUPPORTED and b"unicycle" in L.cn_last_error()
    assert L.cn_robot_act(holo._h, None, 2, out.data_ptr()) == EINVAL
    assert L.cn_scripted_dwa(holo._h, None) == 0
    holo.close()
    # a mixed engine needs cn_mixed_scripted as for the other controllers
    c = _config(5)
    c.sim.human_nums, c.sim.human_nums_scripted = [3, 5], True
    cfgs, eg = make_varied_cn_configs(c, [3, 5], E, phase="train", seed=7, rng="mt19937")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=False, scripted_dwa=True)
    assert L.cn_robot_act(mixed._h, None, 2, out.data_ptr()) == EUNSUPPORTED and b"mixed" in L.cn_last_error()
    mixed.close()
    # the env refuses the opt-in on a holonomic config before it builds an engine
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    with pytest.raises(UnsupportedConfig):
        CrowdNavVecEnv(_config(5, kin="holonomic"), E, 0, DEV, allow_early_resets=True, nenv=E, phase="train")


def _blob(eng):
    return np.asarray(eng.get_state().blob).view(np.uint8).copy()


def _pairs(c, E, T, noise=None):
    """The eager loop robot_act -> step after cn_reset, every row cloned; with `noise` (sigma, seed, step0) the step
    takes the host restatement's perturbed action."""
    import torch

    eng = _engine(c, E)
    eng.reset()
    rows = {k: [] for k in ROWS + (("executed",) if noise else ())}
    for t in range(T):
        a = eng.robot_act("dwa").clone()
        x = a
        if noise:
            sigma, seed, step0 = noise
            x = torch.from_numpy(ref_noise.perturb(a.cpu().numpy()[None], sigma, seed, step0 + t, 0)[0]).to(DEV)
            rows["executed"].append(x)
        obs, rew, done, ev, info, epr, epl = eng.step(x)
        rows["actions"].append(a)
        for k in OBS:
            rows[k].append(obs[k].clone())
        for k, val in zip(RECORDS, (rew, done, ev, info, epr, epl)):
            rows[k].append(val.clone())
    torch.cuda.synchronize()
    out = {k: torch.stack(val).cpu().numpy() for k, val in rows.items()}
    out["state"] = _blob(eng)
    eng.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
def test_gpu_rollout_equals_the_eager_loop(noisy):
    """E = 13, T = 6 at time_limit 1 s (4 steps): every env resets inside the rollout. Launch pairs, or with noise
    triples (the perturbation between the two), on every step."""
    import torch

    from crowdnav_dsrnn_amd.engine import RolloutNoise

    E, T = 13, 6
    c = _config(5, time_limit=1)
    noise = (0.03, 7, 11) if noisy else None
    ref = _pairs(c, E, T, noise)
    eng = _engine(c, E)
    eng.reset()
    out = eng.rollout("dwa", T, **({"noise": RolloutNoise(*noise)} if noisy else {}))
    torch.cuda.synchronize()
    assert out["num_launches"] == (3 if noisy else 2) * T
    for k in ROWS + (("executed",) if noisy else ()):
        assert out[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    assert _blob(eng).tobytes() == ref["state"].tobytes()
    assert ref["done"].all(axis=0).any() or ref["done"].sum() >= E
    assert np.isin(ref["actions"], GRID32).all()
    if noisy:
        assert not np.isin(ref["executed"], GRID32).all()
    eng.close()


@pytest.mark.gpu
def test_gpu_lidar_rollout_equals_the_eager_triple():
    """A unicycle 'convgru' env with lidar.live, 16 beams, E = 8, T = 6: rollout's `lidar` and `actions` rows are
    robot_act -> step_device's of a twin; per step the controller, the step and the row copy, then one scan."""
    import torch

    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    E, T = 8, 6

    def make():
        c = _config(5, policy="convgru", time_limit=1)
        c.lidar.enable, c.lidar.live = True, True
        c.lidar.cfg = dict(c.lidar.cfg, num_beams=16)
        envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
        envs.reset()
        return envs

    a, b = make(), make()
    out = ScriptedRobot(a, "dwa").rollout(T)
    assert out["lidar"].shape == (T, E, 1, 7 + 16)
    assert out["num_launches"] == 3 * T + 1
    for t in range(T):
        act = b.robot_act("dwa").clone()
        o, rew, done, *_ = b.step_device(act)
        assert torch.equal(act, out["actions"][t]), t
        assert torch.equal(o, out["lidar"][t]), t
        assert torch.equal(done, out["done"][t]) and torch.equal(rew, out["reward"][t]), t
    assert bool(out["done"].any())
    assert _blob(a.engine).tobytes() == _blob(b.engine).tobytes()
    a.close()
    b.close()


class _Log:
    def info(self, msg):
        pass


def _rates(name):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.evaluation import evaluate, evaluate_scripted

    E = 100
    c = clone_config(Config())
    c.action_space.kinematics = "unicycle"
    c.robot.scripted_unicycle = name != "dwa"
    c.robot.scripted_dwa = True if name == "dwa" else None
    assert c.env.test_size == 500 and c.sim.human_num == 5
    envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="test")
    evaluate_scripted(name, envs, E, DEV, c, _Log(), keep_traces=False, verbose=False)
    envs.close()
    last = evaluate.last
    return last["success_rate"], last["collision_rate"], last["timeout_rate"]


@pytest.mark.gpu
def test_gpu_dwa_beats_orca_through_the_tracking_law_on_the_default_unicycle_test_episodes():
    """The 500 default test episodes (5 humans, the four default scenarios) on the unicycle robot: the dynamic window at
    DWA_DEFAULTS against ORCA behind the tracking law (config.robot.scripted_unicycle). The success rate must be
    higher by three standard errors of the difference of two rates over 500 episodes each, and the timeout rate
    lower."""
    so, co, to = _rates("orca")
    sd, cd, td = _rates("dwa")
    se = math.sqrt(so * (1 - so) / 500 + sd * (1 - sd) / 500)
    print("orca: success %.3f collision %.3f timeout %.3f; dwa: success %.3f collision %.3f timeout %.3f; "
          "difference %.3f, 3 se %.3f" % (so, co, to, sd, cd, td, sd - so, 3 * se))
    assert sd - so >= 3 * se, (sd, so, 3 * se)
    assert td < to, (td, to)


@pytest.mark.gpu
def test_gpu_behaviour_cloning_takes_the_dwa_expert():
    """16 unicycle envs x 8 steps, two updates: finite losses, and the stored labels are the rollout's `actions` rows
    (grid points of the action space) while the executed actions carry the noise."""
    import torch

    from crowdnav_dsrnn_amd.engine import RolloutNoise
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import BehaviourCloning
    from tests.helpers import make_policy

    E, N, T = 16, 5, 8
    c = _config(N, time_limit=1.5)
    c.training.num_processes, c.ppo.num_steps, c.ppo.num_mini_batch = E, T, 1
    envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
    pol = make_policy(N, E=E, T=T, device=DEV)
    pol.train()
    bc = BehaviourCloning(c, envs, pol, expert="dwa", sigma=0.03, seed=11, lr=1e-3, num_mini_batch=1, value_coef=0.5)
    twin = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
    twin.reset()
    expert = ScriptedRobot(twin, "dwa")
    for k in range(2):
        stats = bc.update()
        assert math.isfinite(stats["nll"]) and math.isfinite(stats["value_loss"]), stats
        want = expert.rollout(T, noise=RolloutNoise(0.03, 11, k * T))
        assert torch.equal(bc.rollouts.actions.reshape(T, E, 2), want["actions"]), k
        assert torch.equal(bc.last["executed"], want["executed"]), k
        lab = bc.rollouts.actions.cpu().numpy()
        assert np.isin(lab, GRID32).all() and float((want["executed"] - want["actions"]).abs().max()) > 0.01
    assert math.isfinite(float(bc.chunk_nll()))
    envs.close()
    twin.close()
    with pytest.raises(UnsupportedConfig):      # the check comes before the GPU: a config without the opt-in
        BehaviourCloning(_config(N, dwa=None), _VenvStub(_config(N, dwa=None)), pol, expert="dwa")
