"""Scripted robot baselines on the device (cn_robot_act, CrowdNavEngine.robot_act, policy_factory.ScriptedRobot).

cn_robot_act is DEFINED as a composition of functions the suite already pins against the reference
(tests/test_policy_factory.py, tests/test_orca_known_answers.py): for every env, what a fresh
policy_factory['orca' | 'social_force'] object predicts from JointState(robot FullState, the N belief humans
(b_px, b_py, b_vx, b_vy, b_r) in index order), rounded to float32. The GPU tests build that composition on the
host -- get_state(), fresh policy objects, predict_batch, np.float32 -- and compare int32 bit patterns: the
kernels run the same device functions under -ffp-contract=off, so any difference is a bug, not rounding."""
import ctypes
import os
import re

import numpy as np
import pytest

from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config, make_cn_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orca", "social_force")


def _config(N, fov=2.0, kin="holonomic"):
    c = clone_config(Config())
    c.sim.human_num = N
    c.robot.FOV = fov
    c.action_space.kinematics = kin
    return c


# ---- CPU ----------------------------------------------------------------------------------------
def test_header_binding_and_export_list_agree_on_cn_robot_act():
    from crowdnav_dsrnn_amd import _lib, build

    txt = open(os.path.join(REPO, "include", "crowdnav.h")).read()
    m = re.search(r"^int cn_robot_act\((.*?)\);", txt, re.S | re.M)
    assert m, "include/crowdnav.h does not declare cn_robot_act"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == ["cn_engine*", "void*", "int", "float*"]
    assert re.search(r"^#define CN_ROBOT_ORCA 0$", txt, re.M) and re.search(r"^#define CN_ROBOT_SOCIAL_FORCE 1$", txt, re.M)
    assert "cn_robot_act" in _lib.EXPORTED
    build.build()
    L = _lib.lib()
    assert hasattr(L, "cn_robot_act") and len(L.cn_robot_act.argtypes) == len(params)
    assert L.cn_robot_act(None, None, 0, None) == -1          # a null engine is CN_EINVAL, before any launch
    assert b"null engine" in L.cn_last_error()


class _VenvStub:
    """What ScriptedRobot reads at construction: the env's config (no GPU behind it)."""

    def __init__(self, config):
        self.config = config

    def robot_act(self, name):
        raise AssertionError("construction must not touch the engine")


def test_scripted_robot_rejects_unicycle_and_unknown_names_without_a_gpu():
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(_VenvStub(_config(5, kin="unicycle")), "orca")
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(_VenvStub(_config(5)), "cadrl")
    for name in NAMES:
        a = ScriptedRobot(_VenvStub(_config(7)), name)
        assert a.base.human_num == 7 and a.name == name


# ---- GPU ----------------------------------------------------------------------------------------
def host_actions(sv, config, name):
    """The reference composition: fresh policy objects on the state's robot and belief rows -> predict_batch ->
    float32 (E, 2)."""
    from crowdnav_dsrnn_amd import policy_factory as PF

    pols, states = [], []
    for e in range(sv.E):
        fs = PF.FullState(sv.r_px[e], sv.r_py[e], sv.r_vx[e], sv.r_vy[e], sv.r_radius[e], sv.r_gx[e], sv.r_gy[e],
                          sv.r_vpref[e], sv.r_theta[e])
        hs = [PF.ObservableState(sv.b_px[e, k], sv.b_py[e, k], sv.b_vx[e, k], sv.b_vy[e, k], sv.b_r[e, k])
              for k in range(sv.N)]
        pols.append(PF.policy_factory[name](config))
        states.append(PF.JointState(fs, hs))
    acts = PF.predict_batch(pols, states)
    return np.array([[a.vx, a.vy] for a in acts], np.float64).astype(np.float32)


def _device_actions(eng, name):
    import torch

    a = eng.robot_act(name)
    torch.cuda.synchronize()
    return a.cpu().numpy()


def _assert_bits(got, want, where):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    g, w = got.view(np.int32), want.view(np.int32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (where, "%d of %d words differ" % (len(bad), g.size), bad[:4].tolist(),
                           got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.gpu
@pytest.mark.parametrize("E", [37, 1])
@pytest.mark.parametrize("N", [1, 5, 9, 10, 31])
def test_gpu_robot_act_equals_host_composition_bit_for_bit(N, E):
    """After reset and after each of 12 steps driven by the controller's own actions: robot_act == the host
    composition, both policies, every env. N = 9 is the quad path's last size (A = 10, all three line slots per
    lane), N = 10 the smallest kd tree, N = 31 the engine's maximum; N = 5 runs with a robot FOV of pi, so that
    belief rows of unseen humans occur."""
    _closed_loop_bits(_config(N, fov=1.0 if N == 5 else 2.0), N, E)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 12])
def test_gpu_robot_act_equals_host_composition_at_tuned_parameters(N):
    """The same check away from the default parameters: ORCA neighbor_dist 3 / safety_space 0.3 / time_horizon 2,
    social force A 3.5 / B 0.6 / KI 2.5, time_step 0.1. cn_robot_act reads them from the engine's cn_config, the
    host composition from the Python Config, so a default baked into either side shows. N = 5 is the quad path
    (robot FOV pi), N = 12 the kd tree, where neighbor_dist 3 cuts the neighbour set."""
    c = _config(N, fov=1.0 if N == 5 else 2.0)
    c.orca.neighbor_dist, c.orca.safety_space, c.orca.time_horizon = 3, 0.3, 2
    c.sf.A, c.sf.B, c.sf.KI = 3.5, 0.6, 2.5
    c.env.time_step = 0.1
    _closed_loop_bits(c, N, 37)


def _closed_loop_bits(c, N, E):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(make_cn_config(c, num_envs=E, nenv=37), "cuda:0")
    unseen = moved = 0
    for drive in NAMES:
        eng.reset()
        for t in range(13):
            sv = eng.get_state()
            unseen += int((sv.b_px != sv.h_px).sum())
            for name in NAMES:
                got = _device_actions(eng, name)
                _assert_bits(got, host_actions(sv, c, name), (N, E, drive, t, name))
                moved += int((got != 0).any())
            if t < 12:
                eng.step(eng.robot_act(drive))
    assert moved == 2 * 13 * 2
    if N == 5:
        assert unseen > 0, "a robot FOV of pi should leave humans unseen"
    eng.close()


def _crafted(eng, cfg):
    """Five envs from a reset state: 0 a belief human inside the combined radius (RVO2's 1/timeStep branch),
    1 a ring at 0.7 m all heading for the robot (linearProgram2 fails, linearProgram3 runs), 2 the robot within
    0.5 m of its goal (unnormalised preferred velocity), 3 every human at the never-seen belief (15, 15) and the
    robot at (0, -4) bound for (0, 4) (no neighbours), 4 left as reset."""
    eng.reset()
    sv = eng.get_state()
    N = sv.N
    sv.b_px[0, 0], sv.b_py[0, 0] = sv.r_px[0] + 0.3, sv.r_py[0]
    sv.b_vx[0, 0], sv.b_vy[0, 0] = -0.5, 0.1
    ang = 2 * np.pi * np.arange(N) / N
    sv.b_px[1], sv.b_py[1] = sv.r_px[1] + 0.7 * np.cos(ang), sv.r_py[1] + 0.7 * np.sin(ang)
    sv.b_vx[1], sv.b_vy[1] = -np.cos(ang), -np.sin(ang)
    sv.r_gx[2], sv.r_gy[2] = sv.r_px[2] + 0.3, sv.r_py[2] + 0.2
    sv.b_px[3], sv.b_py[3], sv.b_vx[3], sv.b_vy[3] = 15.0, 15.0, 0.0, 0.0
    sv.r_px[3], sv.r_py[3], sv.r_gx[3], sv.r_gy[3], sv.r_vx[3], sv.r_vy[3] = 0.0, -4.0, 0.0, 4.0, 0.0, 0.0
    eng.set_state(sv)
    return eng.get_state()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [9, 12])
def test_gpu_robot_act_crafted_states(N):
    import torch

    from crowdnav_dsrnn_amd import _lib, policy_factory as PF
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    c = _config(N)
    eng = CrowdNavEngine(make_cn_config(c, num_envs=5), "cuda:0")
    sv = _crafted(eng, c)
    got = {}
    for name in NAMES:
        got[name] = _device_actions(eng, name)
        _assert_bits(got[name], host_actions(sv, c, name), (N, name))
    # the no-neighbour env: the preferred velocity (0, 8) / 8 itself, inside the speed disc
    assert got["orca"][3].tolist() == [0.0, 1.0]
    assert np.hypot(sv.r_gx[2] - sv.r_px[2], sv.r_gy[2] - sv.r_py[2]) < 0.5
    # linearProgram3 was reached: cn_orca_predict's (fail_at, line count) of the same frames
    frames = []
    for e in range(sv.E):
        fs = PF.FullState(sv.r_px[e], sv.r_py[e], sv.r_vx[e], sv.r_vy[e], sv.r_radius[e], sv.r_gx[e], sv.r_gy[e],
                          sv.r_vpref[e], sv.r_theta[e])
        hs = [PF.ObservableState(sv.b_px[e, k], sv.b_py[e, k], sv.b_vx[e, k], sv.b_vy[e, k], sv.b_r[e, k])
              for k in range(N)]
        frames.append(PF.ORCA(c)._frame(PF.JointState(fs, hs)))
    ag = torch.from_numpy(np.stack([f[0] for f in frames])).to("cuda:0")
    sf = torch.from_numpy(np.stack([f[1] for f in frames])).to("cuda:0")
    res = torch.zeros((sv.E, 4), dtype=torch.float32, device="cuda:0")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().cn_orca_predict(st, sv.E, N + 1, ag.data_ptr(), sf.data_ptr(), float(c.orca.neighbor_dist),
                                          float(c.orca.time_horizon), float(c.env.time_step), res.data_ptr()))
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    _assert_bits(np.ascontiguousarray(r[:, :2]), got["orca"], (N, "cn_orca_predict"))
    fail_at, cnt = r[:, 2], r[:, 3]
    print("N=%d fail_at %s line counts %s" % (N, fail_at.tolist(), cnt.tolist()))
    assert (fail_at < cnt).any(), (fail_at, cnt)
    assert cnt[1] == N and cnt[3] == 0 and cnt[0] >= 1
    eng.close()


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


class _HostScripted:
    """The eager loop's actor: every action comes from the host composition on the engine's state."""

    def __init__(self, venv, name):
        self.venv, self.name = venv, name
        self.base = type("B", (), {"human_num": int(venv.config.sim.human_num)})()

    def act(self, obs, hxs, masks, deterministic=False):
        import torch

        a = host_actions(self.venv.engine.get_state(), self.venv.config, self.name)
        return None, torch.from_numpy(a).to(self.venv.engine.device), None, hxs


def _closed_loop(name, host):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.evaluation import evaluate
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    E = 8
    c = _config(5)
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.env.test_size = E
    envs = CrowdNavVecEnv(c, E, c.env.seed, "cuda:0", allow_early_resets=True, nenv=E, phase="test")
    actor = _HostScripted(envs, name) if host else ScriptedRobot(envs, name)
    log = _Log()
    evaluate(actor, None, envs, E, "cuda:0", c, log, verbose=False)
    return log.lines, evaluate.last["records"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_evaluate_runs_a_scripted_baseline(name):
    """evaluate() unchanged with ScriptedRobot as the actor (8 envs, 8 circle-crossing test episodes): every
    episode ends, two runs log the same, and the per-episode records are those of an eager loop fed by the host
    composition."""
    from crowdnav_dsrnn_amd import abi

    l1, r1 = _closed_loop(name, False)
    l2, r2 = _closed_loop(name, False)
    lh, rh = _closed_loop(name, True)
    assert l1 == l2 and l1 == lh
    assert np.isin(r1["event"], (abi.EV_REACHGOAL, abi.EV_COLLISION, abi.EV_TIMEOUT)).all(), r1["event"]
    assert (r1["done"] == 1).all() and (r1["steps"] > 0).all()
    print(name, "events", r1["event"].tolist(), "steps", r1["steps"].tolist())
    for k in r1:
        assert r1[k].tobytes() == r2[k].tobytes(), k
        assert r1[k].tobytes() == rh[k].tobytes(), k


@pytest.mark.gpu
def test_gpu_robot_act_graph_capture():
    """8 x (robot_act -> step) captured in one HIP graph (engine in graph mode): kernel nodes only, and the state
    blob after the replay is byte-identical to an eager engine's after the same 8 closed-loop steps."""
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    E, T = 64, 8
    c = _config(5)
    blobs = []
    for graph in (False, True):
        eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
        eng.reset()
        eng.step(eng.robot_act("orca"))     # one eager step before the capture, as RolloutTrainer's warm-up
        if graph:
            eng.set_graph_mode(True)
            gr = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(gr):
                for t in range(T):
                    eng.step(eng.robot_act(NAMES[t & 1]))
            counts = _lib.graph_node_counts(gr.raw_cuda_graph())
            assert counts.get("memset", 0) == 0 and counts["kernel"] == counts["total"] == 2 * T, counts
            eng.set_graph_mode(False)       # (recorded, not run: the device sequence is unchanged)
            eng.set_graph_mode(True)
            gr.replay()
            torch.cuda.synchronize()
            eng.set_graph_mode(False)
        else:
            for t in range(T):
                eng.step(eng.robot_act(NAMES[t & 1]))
        torch.cuda.synchronize()
        blobs.append(np.array(eng.get_state().blob, copy=True))
        eng.close()
    assert blobs[0].tobytes() == blobs[1].tobytes()


@pytest.mark.gpu
def test_gpu_robot_act_error_codes():
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.config import make_mixed_cn_configs
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    L = _lib.lib()
    out = torch.zeros((8, 2), device="cuda:0")
    EINVAL, EUNSUPPORTED = -1, -2
    uni = CrowdNavEngine(make_cn_config(_config(5, kin="unicycle"), num_envs=8), "cuda:0")
    assert L.cn_robot_act(uni._h, None, 0, out.data_ptr()) == EUNSUPPORTED
    assert b"holonomic" in L.cn_last_error()
    with pytest.raises(RuntimeError):
        uni.robot_act("orca")
    uni.close()
    sc = ["parallel_traffic", "perpendicular_traffic"]
    ca, cb = _config(5), _config(3)
    ca.sim.train_val_sim = ca.sim.test_sim = cb.sim.train_val_sim = cb.sim.test_sim = sc
    cfgs, eg = make_mixed_cn_configs({sc[0]: ca, sc[1]: cb}, sc, 8)
    mixed = CrowdNavEngine.mixed(cfgs, eg, "cuda:0")
    assert L.cn_robot_act(mixed._h, None, 1, out.data_ptr()) == EUNSUPPORTED
    assert b"mixed" in L.cn_last_error()
    mixed.close()
    eng = CrowdNavEngine(make_cn_config(_config(5), num_envs=8), "cuda:0")
    eng.reset()
    assert L.cn_robot_act(eng._h, None, 2, out.data_ptr()) == EINVAL
    assert L.cn_robot_act(eng._h, None, -1, out.data_ptr()) == EINVAL
    assert L.cn_robot_act(eng._h, None, 0, None) == EINVAL
    with pytest.raises(ValueError):
        eng.robot_act("cadrl")
    with pytest.raises(ValueError):
        eng.robot_act("orca", out=torch.zeros((8, 3), device="cuda:0"))
    mine = eng.robot_act("orca", out=out)
    assert mine is out and torch.equal(eng.robot_act("orca"), out) and eng.robot_act("orca") is eng.robot_actions
    eng.close()
