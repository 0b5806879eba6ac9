"""Live LiDAR mode (cn_lidar_scan, config.lidar.live): the scan of the CURRENT state — all humans and the
walls, heading along the robot's velocity — at every reset and step, vs the reference.

tests/golden/lidar_live/direct_*.npz: direct LidarSensor.sensor_spin calls; lidar_live/roll_*.npz: the
reference CrowdSimDict stepped with random actions, the rel_distances its step() computed and discards
(tools/gen_lidar_live_golden.py). Every case carries an `unstable` mask (beams that move by more than 1e-6
when the inputs move by 1e-10: angular edges, samples on a disc's rim); at most 0.5 % of a file.
Tolerances: the numpy restatement (tests/lidar_live_ref.py) runs the reference's float64 arithmetic on the
same libm: 1e-12 on stable beams. The GPU's trigonometry may differ in the last ulp (~1e-16 in an end point,
/ max_range), the observation is float32 (6e-8): 1e-6 on every stable beam, none excepted; the robot part
is exact."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import lidar_live_ref as R


def _files(pattern):   # in their own folder: test_lidar.py's lidar_*.npz glob must not pick them up
    return sorted("lidar_live/" + os.path.basename(p) for p in glob.glob(os.path.join(H.GOLDEN, "lidar_live", pattern)))


DIRECT, ROLL = _files("direct_*.npz"), _files("roll_*.npz")
CAP = 0.005
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(name):
    d = H.load(name)
    out = []
    for i in range(int(d["cases"])):
        k = "c%d_" % i
        out.append(dict(sensor=d[k + "sensor"], heading=float(d[k + "heading"]), xyr=d[k + "xyr"],
                        half_world=float(d[k + "half_world"]), beams=int(d[k + "beams"]),
                        max_range=float(d[k + "max_range"]), robot_radius=float(d[k + "robot_radius"]),
                        rel_dist=d[k + "rel_dist"], unstable=d[k + "unstable"], tag="%s#%d %s" % (name, i, d[k + "tag"])))
    return out


def _roll_kw(d):
    return dict(beams=int(d["meta_num_beams"]), max_range=float(d["meta_max_range"]),
                robot_radius=float(d["meta_lidar_robot_radius"]))


# ---- CPU ----------------------------------------------------------------------------------------
def test_fixture_files_present():
    assert len(DIRECT) == 3 and len(ROLL) == 2, (DIRECT, ROLL)


@pytest.mark.parametrize("name", DIRECT)
def test_restatement_vs_reference_direct(name):
    cases = _cases(name)
    assert {len(c["xyr"]) for c in cases} >= ({1, 5, 10, 31} if "edge" not in name else {1})
    total = bad = 0
    for c in cases:
        got = R.scan(c["sensor"], c["heading"], c["xyr"], c["beams"], c["max_range"], c["robot_radius"], c["half_world"])
        err = np.abs(got - c["rel_dist"])
        assert (err[~c["unstable"]] <= 1e-12).all(), (c["tag"], err.max(), np.flatnonzero(err > 1e-12)[:8])
        total += got.size
        bad += int(c["unstable"].sum())
    assert bad / total <= CAP


@pytest.mark.parametrize("name", ROLL)
def test_restatement_vs_reference_roll(name):
    d = H.load(name)
    kw = _roll_kw(d)
    cfg = H.cn_config_from_meta(d)
    total = bad = 0
    for t in range(int(d["steps"])):
        sv = H.state_from(d, "t%d_post_" % t, cfg)
        # the reference's heading: np.arctan2 of the robot's velocity — a float32 one while the velocity holds
        # np.float32 values (its last ulp depends on the host's math library); within 2 float32 ulps of the
        # float64 arctangent of the state, which is what cn_lidar_scan takes
        head = d["t%d_heading" % t]
        assert (np.abs(np.arctan2(sv.r_vy, sv.r_vx) - head) <= 2 * np.spacing(np.float32(np.pi))).all()
        for e in range(sv.E):
            got = R.scan((sv.r_px[e], sv.r_py[e]), head[e], np.stack([sv.h_px[e], sv.h_py[e], sv.h_r[e]], 1),
                         half_world=cfg.square_width / 2, **kw)
            un = d["t%d_unstable" % t][e]
            err = np.abs(got - d["t%d_rel_dist" % t][e])
            assert (err[~un] <= 1e-12).all(), (t, e, err.max())
            total += got.size
            bad += int(un.sum())
    assert bad / total <= CAP


def test_header_binding_and_export_list_agree_on_cn_lidar_scan():
    from crowdnav_dsrnn_amd import _lib, abi, build

    txt = open(os.path.join(REPO, "include", "crowdnav.h")).read()
    m = re.search(r"^int cn_lidar_scan\((.*?)\);", txt, re.S | re.M)
    assert m, "include/crowdnav.h does not declare cn_lidar_scan"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == \
        ["cn_engine*", "void*", "int", "double", "double", "float*"]
    assert "cn_lidar_scan" in _lib.EXPORTED
    build.build()
    L = _lib.lib()
    assert len(L.cn_lidar_scan.argtypes) == len(params)
    # the argument checks of cn_lidar_obs, before any launch: a null engine is CN_EINVAL (-1)
    assert L.cn_lidar_scan(None, None, 180, 5.0, 0.3, None) == -1
    assert b"null engine" in L.cn_last_error()
    assert {n for n, _, _ in abi.STATE_FIELDS} >= {"r_px", "r_py", "r_vx", "r_vy", "h_px", "h_py", "h_r"}   # what it reads


def test_config_default_is_parity_mode():
    from crowdnav_dsrnn_amd.config import Config, clone_config

    assert Config().lidar.live is False
    assert clone_config(Config()).lidar.live is False


# ---- GPU ----------------------------------------------------------------------------------------
def _live_cfg(N, E, half_world=10.0, kin="holonomic"):
    from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config

    c = clone_config(Config())
    c.sim.human_num = N
    c.sim.square_width = 2 * half_world
    c.action_space.kinematics = kin
    return make_cn_config(c, num_envs=E)


@pytest.fixture(scope="module")
def engines():
    """Engines shared by the tests of this module, by (E, N, half_world)."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    pool = {}

    def get(E, N, half_world=10.0):
        key = (E, N, half_world)
        if key not in pool:
            cfg = _live_cfg(N, E, half_world)
            pool[key] = (CrowdNavEngine(cfg, "cuda:0"), cfg)
        return pool[key]

    yield get
    for eng, _ in pool.values():
        eng.close()


def _state_of(cases, cfg):
    """A StateView holding one direct case per env; the heading is carried by the robot's velocity."""
    from crowdnav_dsrnn_amd import abi

    sv = abi.StateView(None, cfg.num_envs, cfg.human_num, cfg.robot_visible)
    for e, c in enumerate(cases):
        sv.r_px[e], sv.r_py[e] = c["sensor"]
        sv.r_vx[e], sv.r_vy[e] = np.cos(c["heading"]), np.sin(c["heading"])
        sv.r_radius[e], sv.r_vpref[e] = 0.3, 1.0
        sv.r_gx[e], sv.r_gy[e], sv.r_theta[e] = 3.5 - e, -2.0 + e, -1.0 + 0.7 * e   # clipped both ways
        sv.h_px[e], sv.h_py[e], sv.h_r[e] = c["xyr"][:, 0], c["xyr"][:, 1], c["xyr"][:, 2]
    return sv


def _scan(eng, sv, beams, max_range, robot_radius):
    eng.set_state(sv)
    out = torch.full((eng.E, 1, 7 + beams), -1.0, device="cuda:0")
    eng.lidar_scan(out, beams, max_range, robot_radius)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_rows(got, sv, rel_dist, unstable, max_range, where):
    np.testing.assert_array_equal(got[:, 0, :7], R.robot_part(sv, max_range), err_msg=str(where))
    err = np.abs(got[:, 0, 7:].astype(np.float64) - R.to_obs(rel_dist))
    print(where, "max err on stable beams %.3g, unstable %d" % (err[~unstable].max(), int(unstable.sum())))
    assert (err[~unstable] <= 1e-6).all(), (where, err[~unstable].max(), np.argwhere((err > 1e-6) & ~unstable)[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("name", DIRECT)
def test_gpu_scan_vs_reference_direct(name, E, engines):
    groups = {}
    for c in _cases(name):
        groups.setdefault((len(c["xyr"]), c["beams"], c["max_range"], c["robot_radius"], c["half_world"]), []).append(c)
    for (N, beams, max_range, rr, half), cs in groups.items():
        eng, cfg = engines(E, N, half)
        if E > 1:   # E different cases side by side (wrapping round a short group)
            packs = [[cs[(i + j) % len(cs)] for j in range(E)] for i in range(0, len(cs), E)]
        else:
            packs = [[c] for c in cs]
        for pack in packs:
            sv = _state_of(pack, cfg)
            got = _scan(eng, sv, beams, max_range, rr)
            _check_rows(got, sv, np.stack([c["rel_dist"] for c in pack]), np.stack([c["unstable"] for c in pack]),
                        max_range, [c["tag"] for c in pack])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROLL)
def test_gpu_scan_vs_reference_roll(name):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    d = H.load(name)
    kw = _roll_kw(d)
    cfg = H.cn_config_from_meta(d)
    eng = CrowdNavEngine(cfg, "cuda:0")
    for t in range(int(d["steps"])):
        sv = H.state_from(d, "t%d_post_" % t, cfg)     # teacher-forced: the reference's post-step state
        got = _scan(eng, sv, **kw)
        _check_rows(got, sv, d["t%d_rel_dist" % t], d["t%d_unstable" % t], kw["max_range"], (name, t))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("E,N,beams,max_range", [(67, 31, 180, 5.0), (67, 31, 65, 11.0), (3, 1, 180, 5.0),
                                                 (3, 1, 65, 11.0)])
def test_gpu_scan_vs_restatement_random_states(E, N, beams, max_range, engines):
    from crowdnav_dsrnn_amd import abi

    eng, cfg = engines(E, N)
    rng = np.random.RandomState(100 * E + beams)
    sv = abi.StateView(None, E, N, cfg.robot_visible)
    sv.r_px[:], sv.r_py[:] = rng.uniform(-8.5, 8.5, E), rng.uniform(-8.5, 8.5, E)
    sv.r_vx[:], sv.r_vy[:] = rng.normal(0, 0.7, E), rng.normal(0, 0.7, E)
    sv.r_vx[0] = sv.r_vy[0] = 0.0                       # heading 0, as right after a reset
    sv.r_radius[:], sv.r_vpref[:] = 0.3, 1.0
    sv.r_gx[:], sv.r_gy[:], sv.r_theta[:] = rng.uniform(-6, 6, E), rng.uniform(-6, 6, E), rng.uniform(-3, 3, E)
    ang, dist = rng.uniform(0, 2 * np.pi, (E, N)), rng.uniform(0.4, 7.0, (E, N))
    sv.h_px[:], sv.h_py[:] = sv.r_px[:, None] + dist * np.cos(ang), sv.r_py[:, None] + dist * np.sin(ang)
    sv.h_r[:] = rng.uniform(0.2, 0.5, (E, N))
    rr, half = 0.3, cfg.square_width / 2
    want = np.zeros((E, beams))
    un = np.zeros((E, beams), bool)
    for e in range(E):
        args = ((sv.r_px[e], sv.r_py[e]), np.arctan2(sv.r_vy[e], sv.r_vx[e]),
                np.stack([sv.h_px[e], sv.h_py[e], sv.h_r[e]], 1))
        fn = lambda s, h, x: R.scan(s, float(h), x, beams, max_range, rr, half)  # noqa: E731
        want[e] = fn(*args)
        un[e] = R.unstable_mask(fn, args, rng)
    assert un.mean() <= CAP, un.mean()
    got = _scan(eng, sv, beams, max_range, rr)
    _check_rows(got, sv, want, un, max_range, (E, N, beams))
    assert (want < 1.0).mean() > 0.05       # the crowd (or a wall) is in sight


def _convgru_config(live, kin="holonomic", N=5):
    from crowdnav_dsrnn_amd.config import Config, clone_config

    c = clone_config(Config())
    c.robot.policy = "convgru"
    c.lidar.enable = True
    c.lidar.live = live
    c.sim.circle_radius = 6.0
    c.sim.human_num = N
    c.action_space.kinematics = kin
    return c


@pytest.mark.gpu
def test_gpu_vecenv_live_scan_every_step():
    """lidar.live: every reset / step observation is the scan of the state it returns — done envs show their
    new episode — and the scan moves on steps without a reset."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    E = 64
    c = _convgru_config(True)
    envs = CrowdNavVecEnv(c, E, 0, "cuda:0")
    assert tuple(envs.observation_space.shape) == (1, 187)
    probe = CrowdNavEngine(envs.cn_cfg, "cuda:0")
    kw = dict(beams=180, max_range=5.0, robot_radius=float(c.lidar.cfg["robot_radius"]))
    o = envs.reset()
    assert o.shape == (E, 1, 187)
    sv = envs.engine.get_state()
    np.testing.assert_array_equal(o.cpu().numpy(), _scan(probe, sv, **kw))
    assert bool((o[:, 0, 7:] != 0).any(1).all())     # no empty scan held over: the crowd is in sight at once
    # and the reset scan is the reference's semantics at heading 0
    want = R.state_scans(sv, half_world=envs.cn_cfg.square_width / 2, **kw)
    assert (np.abs(o[:, 0, 7:].cpu().numpy() - R.to_obs(want)) > 1e-6).mean() <= CAP
    g = torch.Generator(device="cuda:0").manual_seed(3)
    prev, moved, dones = o[:, 0, 7:].clone(), 0, 0
    for _ in range(30):
        a = torch.randn(E, 2, device="cuda:0", generator=g)
        o, r, done, *_ = envs.step_device(a)
        cur, done = o.clone(), done.bool().clone()
        np.testing.assert_array_equal(cur.cpu().numpy(), _scan(probe, envs.engine.get_state(), **kw))
        moved += int((cur[:, 0, 7:] != prev).any(1)[~done].sum())
        dones += int(done.sum())
        prev = cur[:, 0, 7:]
    assert moved > 20 * E and dones > 0, (moved, dones)
    probe.close()
    envs.close()


@pytest.mark.gpu
def test_gpu_vecenv_live_off_is_todays_observation():
    """lidar.live off (the default, and live without lidar.enable): bit for bit what cn_lidar_obs gives —
    the held per-episode scan of the last human."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    E = 64
    c = _convgru_config(False)
    envs = CrowdNavVecEnv(c, E, 0, "cuda:0")
    eng = CrowdNavEngine(envs.cn_cfg, "cuda:0")
    kw = dict(enable=True, beams=180, max_range=5.0, robot_radius=float(c.lidar.cfg["robot_radius"]))
    out = torch.zeros((E, 1, 187), device="cuda:0")
    lid = torch.zeros((E, 180), device="cuda:0")
    eng.reset()
    eng.lidar_obs(out, lid, None, **kw)
    assert torch.equal(envs.reset(), out)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    for _ in range(30):
        a = torch.randn(E, 2, device="cuda:0", generator=g)
        o = envs.step_device(a)[0]
        done = eng.step(a)[2]
        eng.lidar_obs(out, lid, done, **kw)
        assert torch.equal(o, out)
    eng.close()
    envs.close()
    c = _convgru_config(True)
    c.lidar.enable = False          # live needs the LiDAR switched on
    envs = CrowdNavVecEnv(c, 8, 0, "cuda:0")
    envs.reset()
    o = envs.step_device(torch.zeros(8, 2, device="cuda:0"))[0]
    assert bool((o[:, 0, 7:] == 0).all())
    envs.close()


@pytest.mark.gpu
def test_gpu_live_step_graph_replay_equals_eager():
    """A HIP graph of 8 live step_device calls (single-stream capture, engine in graph mode) replayed once
    equals 8 eager calls: cn_lidar_scan launches without host synchronisation or allocation."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    E, T = 64, 8
    g = torch.Generator(device="cuda:0").manual_seed(9)
    acts = torch.randn((T + 1, E, 2), generator=g, device="cuda:0").contiguous()
    res = []
    for graph in (False, True):
        envs = CrowdNavVecEnv(_convgru_config(True), E, 0, "cuda:0")
        envs.reset()
        envs.step_device(acts[0])        # one eager step before the capture, as RolloutTrainer's warm-up
        rec = torch.zeros((T, E, 1, 187), device="cuda:0")
        if graph:
            buf = acts[1:].clone()
            envs.engine.set_graph_mode(True)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for t in range(T):
                    rec[t].copy_(envs.step_device(buf[t])[0])
            envs.engine.set_graph_mode(False)   # (recorded, not run: the device sequence is unchanged)
            envs.engine.set_graph_mode(True)
            gr.replay()
            torch.cuda.synchronize()
            envs.engine.set_graph_mode(False)
        else:
            for t in range(T):
                rec[t].copy_(envs.step_device(acts[1 + t])[0])
        torch.cuda.synchronize()
        res.append(rec.cpu().numpy())
        envs.close()
    assert (res[0][1:, :, 0, 7:] != res[0][:-1, :, 0, 7:]).any()
    np.testing.assert_array_equal(res[0], res[1])


@pytest.mark.gpu
def test_gpu_live_rollout_trainer_graph_equals_eager():
    """RolloutTrainer in live mode, 16 envs, 2 updates (the second rollout is the captured HIP graph): finite
    losses, and the observations the graph rollout stored equal those of eager live steps of a fresh VecEnv
    driven by the same actions. (Two ConvGRU trainers are not compared with each other: the convolution
    library may pick other algorithms from one run to the next, which moves the actions in the last bits.)"""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import PPO
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer
    from crowdnav_dsrnn_amd.policy import Policy

    c = _convgru_config(True)
    c.ppo.num_steps = 8
    c.ppo.num_mini_batch = 2
    c.ppo.epoch = 2
    torch.manual_seed(0)
    envs = CrowdNavVecEnv(c, 16, 0, "cuda:0")
    pol = Policy(envs.observation_space, envs.action_space, base="convgru", base_kwargs=c).to("cuda:0")
    agent = PPO(pol, 0.2, c.ppo.epoch, c.ppo.num_mini_batch, 0.5, 0.0, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    tr = RolloutTrainer(c, envs, pol, agent, deterministic=True, graphs=True)
    obs0 = tr.rollouts.obs[0].clone()
    stored = []
    for u in range(2):
        st = tr.update()
        assert all(np.isfinite([st["value_loss"], st["action_loss"], st["dist_entropy"]])), st
        assert (tr._graph is not None) == (u == 1)
        stored.append((tr.rollouts.obs.clone(), tr.rollouts.actions.clone()))
    envs.close()
    eager = CrowdNavVecEnv(c, 16, 0, "cuda:0")
    assert torch.equal(eager.reset(), obs0)
    for u, (obs, actions) in enumerate(stored):
        assert bool((obs[1:, :, 0, 7:] != obs[:-1, :, 0, 7:]).any())
        for t in range(c.ppo.num_steps):
            o = eager.step_device(actions[t])[0]
            assert torch.equal(o, obs[t + 1]), "update %d step %d" % (u, t)
    eager.close()
