"""The scripted controllers on the unicycle robot (cn_scripted_unicycle, config.robot.scripted_unicycle).

The tracking law between a controller's velocity and the step's (dv, dtheta) action is this project's definition
(the reference has no scripted unicycle robot): tests/unicycle_track_ref.py restates it from the formulas in
include/crowdnav.h on Python floats. robot_act is compared with that restatement applied to the holonomic answer of
the same state (tests/test_robot_act.py::host_actions); every rollout comparison is exact, against the eager loop
robot_act -> step on a twin engine, as in tests/test_rollout.py. time_limit 2 s at time_step 0.25 makes every env
reset every few steps."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config, make_cn_config, make_varied_cn_configs
from tests import rollout_noise_ref as ref_noise
from tests import unicycle_track_ref as ref_track

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orca", "social_force")
OBS = ("robot_node", "temporal_edges", "spatial_edges")
RECORDS = ("reward", "done", "event", "info", "ep_return", "ep_len")
ROWS = ("actions",) + OBS + RECORDS
EINVAL, EUNSUPPORTED = -1, -2
DEV = "cuda:0"
ULP = float(np.spacing(np.float32(0.1)))   # 7.45e-9: one float32 ulp at the action limit
LIM = np.float32(0.1)


def _config(N, kin="unicycle", rng="mt19937", time_limit=2, optin=True, policy="srnn"):
    c = clone_config(Config())
    c.sim.human_num = N
    c.robot.policy = policy
    c.robot.scripted_unicycle = optin
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.env.rng = rng
    if time_limit is not None:
        c.env.time_limit = time_limit
    return c


# ---- CPU ----------------------------------------------------------------------------------------
def test_header_binding_and_export_list_agree_on_cn_scripted_unicycle():
    from crowdnav_dsrnn_amd import _lib, build

    txt = open(os.path.join(REPO, "include", "crowdnav.h")).read()
    m = re.search(r"^int cn_scripted_unicycle\((.*?)\);", txt, re.S | re.M)
    assert m, "include/crowdnav.h does not declare cn_scripted_unicycle"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == ["cn_engine*", "int"]
    assert "cn_scripted_unicycle" in _lib.EXPORTED
    build.build()
    L = _lib.lib()
    assert hasattr(L, "cn_scripted_unicycle") and len(L.cn_scripted_unicycle.argtypes) == len(params)
    assert L.cn_scripted_unicycle(None, 1) == EINVAL and b"null engine" in L.cn_last_error()


class _VenvStub:
    """What ScriptedRobot reads before it touches the engine (no GPU behind it)."""

    num_envs = 8
    obs_mode = "srnn"

    def __init__(self, config):
        self.config = config

    def __getattr__(self, name):
        raise AssertionError("the check must come before the engine is touched (%s)" % name)


def test_scripted_robot_takes_a_unicycle_env_only_with_the_optin():
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    assert Config().robot.scripted_unicycle is False
    for name in NAMES:
        with pytest.raises(UnsupportedConfig):
            ScriptedRobot(_VenvStub(_config(5, optin=False)), name)
        with pytest.raises(UnsupportedConfig):
            ScriptedRobot.check_rollout(_VenvStub(_config(5, optin=False)), name)
        a = ScriptedRobot(_VenvStub(_config(7)), name)
        assert a.base.human_num == 7 and a.name == name
        ScriptedRobot.check_rollout(_VenvStub(_config(7)), name)
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(_VenvStub(_config(5)), "cadrl")


def _law_rows():
    """10 000 rows (float32 velocity, float64 theta and v): random ones, then the law's corners -- s == 0, |delta|
    below the turn limit, delta next to +-pi (both sides of the cut), v at +-v_pref."""
    rs = np.random.RandomState(20241020)
    n = 10000
    u = (rs.normal(0, 0.6, (n, 2))).astype(np.float32)
    theta = rs.uniform(0, 2 * np.pi, n)
    theta[::2] = theta[::2].astype(np.float32)            # (the step stores a float32 heading)
    v = rs.uniform(-1, 1, n).astype(np.float32).astype(np.float64)
    psi = np.arctan2(u[:, 1].astype(np.float64), u[:, 0].astype(np.float64))
    u[0:200] = 0.0                                         # s == 0 (also -0.0 components)
    u[100:200, 0] = -0.0
    theta[200:1200] = psi[200:1200] + rs.uniform(-0.1, 0.1, 1000)            # |delta| < 0.1: no saturation of a1
    theta[1200:2200] = psi[1200:2200] + np.pi + rs.uniform(-1e-3, 1e-3, 1000)   # delta near +-pi
    theta[2200:2300] = psi[2200:2300] + np.pi                                 # ... and as near as rounding puts it
    theta[2300:2400] = psi[2300:2400] - np.pi
    theta[2400:2600] = psi[2400:2600] + rs.choice([-0.1, 0.1], 200)           # at the turn limit
    v[2600:3100] = 1.0
    v[3100:3600] = -1.0
    v[3600:3800] = 0.0
    return u, theta, v


def test_host_unicycle_track_equals_the_restatement_bit_for_bit():
    from crowdnav_dsrnn_amd.policy_factory import unicycle_track

    u, theta, v = _law_rows()
    want, delta = ref_track.track(u, theta, v)
    got = unicycle_track(u, theta, v)
    assert got.dtype == np.float32 and got.shape == (len(u), 2)
    assert got.view(np.int32).tolist() == want.view(np.int32).tolist()
    # the rows hold what they were built for
    assert np.isnan(delta[:200]).all() and (want[:200, 1] == 0).all()
    assert (np.abs(delta[200:1200]) < 0.1 + 1e-12).all() and (np.abs(want[200:1200, 1]) < LIM).sum() > 900
    assert (np.pi - np.abs(delta[1200:2400]) < 1.1e-3).all()
    assert (delta[1200:2400] > 0).any() and (delta[1200:2400] < 0).any()
    assert (np.abs(want) <= LIM).all()
    for k in range(2):
        assert (np.abs(want[:, k]) == LIM).any() and (np.abs(want[:, k]) < LIM).any()
    slow = np.hypot(u[2600:3100, 0].astype(np.float64), u[2600:3100, 1].astype(np.float64)) <= 1.0
    assert slow.sum() > 100 and (want[2600:3100, 0][slow] <= 0).all()    # at v = v_pref: target <= s <= v
    assert (want[3100:3600, 0] == LIM).all()                             # at v = -v_pref: never backwards, target >= 0
    # a (..., 2) batch and a single row give the same rows
    assert unicycle_track(u[:6].reshape(2, 3, 2), theta[:6].reshape(2, 3), v[:6].reshape(2, 3)).tobytes() == got[:6].tobytes()
    assert unicycle_track(u[777], theta[777], v[777]).tobytes() == got[777].tobytes()


@pytest.mark.parametrize("kind", NAMES)
def test_the_law_closed_over_the_integrator_reaches_the_desired_velocity(kind):
    """A desired velocity held fixed towards a goal -- ORCA's free-space answer, the unit vector times v_pref = 1, and
    social force's from rest, KI * v_pref * time_step = 0.25 along it -- with the step's integrator (float32, as
    cn_step: v <- clip(v + a0, -v_pref, v_pref), theta <- (theta + a1) mod 2 pi): |delta| < 1e-6 and |v - s| < 1e-6
    within 40 steps, from headings up to pi away and from rest, full speed ahead and full speed in reverse. A sanity
    check of the definition: the worst case turns pi at 0.1 per step (32 steps) while the speed settles."""
    goal = np.array([3.0, -4.0])
    d = goal / np.linalg.norm(goal)
    u = (d * (1.0 if kind == "orca" else 0.25)).astype(np.float32)
    s = math.sqrt(float(u[0]) ** 2 + float(u[1]) ** 2)
    psi = math.atan2(float(u[1]), float(u[0]))
    two_pi = np.float32(2 * np.pi)
    for off in (0.0, 0.05, -1.0, 2.0, math.pi - 0.01, -(math.pi - 1e-9), math.pi):
        for v0 in (0.0, 1.0, -1.0):
            theta, v = np.float32(np.mod(psi + off, 2 * np.pi)), np.float32(v0)
            for _ in range(40):
                a0, a1, _d = ref_track.track_one(u[0], u[1], theta, v)
                a0, a1 = np.float32(a0), np.float32(a1)
                v = np.float32(min(max(np.float32(v + a0), np.float32(-1)), np.float32(1)))
                theta = np.float32(np.mod(np.float32(theta + a1), two_pi))
            delta = math.remainder(psi - float(theta), 2 * math.pi)
            assert abs(delta) < 1e-6 and abs(float(v) - s) < 1e-6, (kind, off, v0, delta, float(v), s)


# ---- GPU ----------------------------------------------------------------------------------------
def _engine(c, E, chunk=None, optin=True, **kw):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(make_cn_config(c, num_envs=E, nenv=kw.pop("nenv", E), phase="train", **kw), DEV,
                         scripted_unicycle=optin)
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    return eng


def _blob(eng):
    return np.asarray(eng.get_state().blob).view(np.uint8).copy()


def _host(out, keys=ROWS):
    import torch

    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in keys if out.get(k) is not None}


def _same_rows(got, ref, what, keys=ROWS):
    for k in keys:
        g, r = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            bad = np.argwhere(g.view(np.uint8).reshape(g.shape[0], -1) != r.view(np.uint8).reshape(r.shape[0], -1))
            raise AssertionError("%s: %s differs first at step %d (%d bytes in all)" % (what, k, bad[0][0], len(bad)))


def _pairs(c, E, name, T, noise=None):
    """The reference: the eager loop robot_act -> step after cn_reset, every row cloned; with `noise` (sigma, seed,
    step0) the step takes the host restatement's perturbed action and the rows gain 'executed'."""
    import torch

    eng = _engine(c, E)
    eng.reset()
    rows = {k: [] for k in ROWS + (("executed",) if noise else ())}
    for t in range(T):
        a = eng.robot_act(name).clone()
        x = a
        if noise:
            sigma, seed, step0 = noise
            x = torch.from_numpy(ref_noise.perturb(a.cpu().numpy()[None], sigma, seed, step0 + t, 0)[0]).to(DEV)
            rows["executed"].append(x)
        obs, rew, done, ev, info, epr, epl = eng.step(x)
        rows["actions"].append(a)
        for k in OBS:
            rows[k].append(obs[k].clone())
        for k, v in zip(RECORDS, (rew, done, ev, info, epr, epl)):
            rows[k].append(v.clone())
    torch.cuda.synchronize()
    out = {k: torch.stack(v).cpu().numpy() for k, v in rows.items()}
    out["state"] = _blob(eng)
    eng.close()
    return out


_REF = {}


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _rollout(c, E, name, T, chunk=None, **kw):
    eng = _engine(c, E, chunk=chunk)
    eng.reset()
    out = eng.rollout(name, T, **kw)
    got = _host(out, ROWS + ("executed",))
    got["state"] = _blob(eng)
    eng.close()
    return got, out["num_launches"]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 12])
def test_gpu_robot_act_equals_the_law_on_the_holonomic_answer(N):
    """E = 19: at N = 5 (the quad controller) the second 16-env workgroup holds three quads; N = 12 is the kd
    controller. Both controllers, after reset (r_dv = 0, the reset's float64 heading) and after 25 steps of the
    controller's own actions (r_dv != 0, a float32 heading). (ux, uy): the host composition of tests/test_robot_act.py
    on the state's rows, i.e. the holonomic answer. Both sides round a float64 value of magnitude <= 0.1 once to
    float32 and ocml differs from libm by ulps of float64, so a component may differ by one float32 ulp at 0.1."""
    from tests.test_robot_act import host_actions

    import torch

    E = 19
    c = _config(N, time_limit=None)
    eng = _engine(c, E, nenv=37)
    seen = {(k, s): 0 for k in range(2) for s in (True, False)}
    moving = 0
    for name in NAMES:
        eng.reset()
        for where in ("reset", "after 25 steps"):
            sv = eng.get_state()
            u = host_actions(sv, c, name)
            theta, v = np.array(sv.r_theta, np.float64), np.array(sv.r_dv, np.float64)
            want, delta = ref_track.track(u, theta, v)
            got = eng.robot_act(name)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            print(N, name, where, "max |got - want| / ulp:", np.abs(got.astype(np.float64) - want).max() / ULP,
                  "min pi - |delta|:", np.nanmin(np.pi - np.abs(delta)))
            assert not (np.pi - np.abs(delta) < 1e-9).any(), "a row at the cut of delta: change the seed"
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ULP).all(), (N, name, where)
            assert (np.abs(got) <= LIM).all()
            for k in range(2):
                seen[(k, True)] += int((np.abs(got[:, k]) == LIM).sum())
                seen[(k, False)] += int((np.abs(got[:, k]) < LIM).sum())
            if where == "reset":
                assert (v == 0).all()
                for _ in range(25):
                    eng.step(eng.robot_act(name))
            else:
                moving += int((v != 0).sum())
                assert (theta == theta.astype(np.float32)).all()
    assert moving > E and all(n > 0 for n in seen.values()), (moving, seen)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 4])
@pytest.mark.parametrize("N", [1, 5, 9])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fused_rollout_equals_pairs(name, rng, N, chunk):
    """tests/test_rollout.py's test of the same name on the unicycle engine: E = 13 (partial workgroups), T = 37 = the
    first step after cn_reset (a pair) + a full default chunk + a remainder."""
    E, T = 13, 37
    c = _config(N, rng=rng)
    ref = _ref(("fused", name, rng, N), lambda: _pairs(c, E, name, T))
    got, nl = _rollout(c, E, name, T, chunk=chunk)
    C = 32 if chunk is None else chunk
    assert nl == 2 + math.ceil((T - 1) / C), nl
    _same_rows(got, ref, "%s %s N=%d chunk %s" % (name, rng, N, chunk))
    assert got["state"].tobytes() == ref["state"].tobytes()
    done_steps = np.nonzero(ref["done"].any(axis=1))[0]
    last_of_launch = {0} | {min(1 + k * C + C - 1, T - 1) for k in range(math.ceil((T - 1) / C))}
    assert any(int(t) not in last_of_launch for t in done_steps), done_steps
    assert ref["done"].sum(axis=0).min() >= 3, ref["done"].sum(axis=0)   # several resets per env
    assert (np.abs(ref["actions"]) <= LIM).all() and np.abs(ref["actions"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case,N", [("orca at N + 1 = 11: pairs", 10), ("kd-tree step path", 12)])
def test_gpu_rollout_as_launch_pairs_gives_the_same_rows(case, N):
    E, T = 13, 37
    c = _config(N)
    ref = _pairs(c, E, "orca", T)
    got, nl = _rollout(c, E, "orca", T)
    assert nl == 2 * T, (case, nl)
    _same_rows(got, ref, case)
    assert got["state"].tobytes() == ref["state"].tobytes(), case
    assert ref["done"].sum(axis=0).min() >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 4])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_noisy_rollout_keeps_clean_labels_and_steps_the_perturbed_action(name, rng, chunk):
    """sigma = 0.03 in action units at N = 5: the `actions` rows are the clean labels of the eager loop whose step
    takes the perturbed action, `executed` - `actions` is the restatement's noise, and `executed` leaves [-0.1, 0.1]
    in some rows, so the step's clip of the action works."""
    from crowdnav_dsrnn_amd.engine import RolloutNoise

    E, T, N = 13, 37, 5
    sigma, seed, step0 = 0.03, 7, 11
    c = _config(N, rng=rng)
    ref = _ref(("noisy", name, rng), lambda: _pairs(c, E, name, T, noise=(sigma, seed, step0)))
    got, nl = _rollout(c, E, name, T, chunk=chunk, noise=RolloutNoise(sigma, seed, step0))
    C = 32 if chunk is None else chunk
    assert nl == 3 + 1 + math.ceil((T - 1) / C), nl      # a launch triple, the noise block, the fused launches
    _same_rows(got, ref, "noisy %s %s chunk %s" % (name, rng, chunk), ROWS + ("executed",))
    assert got["state"].tobytes() == ref["state"].tobytes()
    assert got["executed"].tobytes() == ref_noise.perturb(got["actions"], sigma, seed, step0, 0).tobytes()
    assert (np.abs(got["actions"]) <= LIM).all()
    assert (got["executed"] > LIM).any() and (got["executed"] < -LIM).any()
    assert ref["done"].sum(axis=0).min() >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_lidar_rows_equal_the_eager_triple(name):
    """A plain unicycle 'convgru' env with lidar.live, 16 beams, E = 8, T = 6 (a pair, then a recording launch of 5
    steps): rollout's `lidar` and `actions` rows are robot_act -> step_device's of a twin, and so is the state."""
    import torch

    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    E, T = 8, 6

    def make():
        c = _config(5, policy="convgru")
        c.lidar.enable, c.lidar.live = True, True
        c.lidar.cfg = dict(c.lidar.cfg, num_beams=16)
        envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
        envs.reset()
        return envs

    a, b = make(), make()
    out = a.rollout(name, T)
    assert out["lidar"].shape == (T, E, 1, 7 + 16)
    assert out["num_launches"] == 3 + 1 + 1 + 1      # a launch triple, the row block, one recording launch, the scan
    for t in range(T):
        act = b.robot_act(name).clone()
        o, rew, done, *_ = b.step_device(act)
        assert torch.equal(act, out["actions"][t]), t
        assert torch.equal(o, out["lidar"][t]), t
        assert torch.equal(done, out["done"][t]) and torch.equal(rew, out["reward"][t]), t
    assert (out["actions"].abs() <= float(LIM)).all() and out["actions"].abs().max() > 0
    assert _blob(a.engine).tobytes() == _blob(b.engine).tobytes()
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_mixed_engine_rows_equal_plain_unicycle_engines(name):
    """human_nums = [3, 5] with both opt-ins, E = 10, T = 37: every env's rollout rows are those of the plain unicycle
    one-env engine of its count (env_offset r of nenv E) -- tests/test_varied_scripted.py's comparison."""
    import torch

    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    NUMS, E, T, SEED = [3, 5], 10, 37, 7
    c = _config(5)
    c.sim.human_nums, c.sim.human_nums_scripted = list(NUMS), True
    cfgs, eg = make_varied_cn_configs(c, NUMS, E, phase="train", seed=SEED, rng="mt19937")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=True, scripted_unicycle=True)
    mixed.reset()
    got = mixed.rollout(name, T)
    assert int(got["done"].long().sum(0).min()) >= 3
    for r in range(E):
        n = NUMS[r % 2]
        cp = _config(n)
        p = CrowdNavEngine(make_cn_config(cp, num_envs=1, env_offset=r, nenv=E, phase="train", seed=SEED, rng="mt19937"),
                           DEV, scripted_unicycle=True)
        p.reset()
        want = p.rollout(name, T)
        for k in ("actions", "robot_node", "temporal_edges") + RECORDS:
            x, y = got[k][:, r], want[k][:, 0]
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (r, k)
        assert torch.equal(got["spatial_edges"][:, r, :n], want["spatial_edges"][:, 0]), r
        p.close()
    assert float(got["actions"].abs().max()) <= float(LIM)
    mixed.close()


@pytest.mark.gpu
def test_gpu_refusals_without_the_optin_are_unchanged():
    """Without cn_scripted_unicycle the four entry points refuse a unicycle engine with the texts they always had,
    a refusal launches nothing (the next step equals a twin's), and switching the opt-in off restores the refusal."""
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine, RolloutNoise

    L = _lib.lib()
    E, T = 8, 4
    lidar = dict(beams=16, max_range=5.0, robot_radius=0.3)
    c = _config(5)

    def refused(eng, text):
        calls = [lambda: eng.robot_act("orca"), lambda: eng.rollout("orca", T),
                 lambda: eng.rollout("social_force", T, noise=RolloutNoise(0.03, 1, 0))]
        if eng.groups is None:
            calls.append(lambda: eng.rollout("orca", T, lidar=lidar))
        for fn in calls:
            with pytest.raises(RuntimeError) as ei:
                fn()
            assert "error %d" % EUNSUPPORTED in str(ei.value) and text in str(ei.value), str(ei.value)

    eng, twin = _engine(c, E, optin=False), _engine(c, E, optin=False)
    eng.reset()
    twin.reset()
    before = _blob(eng)
    refused(eng, "holonomic")
    assert _blob(eng).tobytes() == before.tobytes()
    a = torch.from_numpy(np.random.RandomState(1).uniform(-0.1, 0.1, (E, 2)).astype(np.float32)).to(DEV)
    x, y = eng.step(a), twin.step(a)
    assert all(torch.equal(p, q) for p, q in zip(x[1:3], y[1:3])) and _blob(eng).tobytes() == _blob(twin).tobytes()
    eng.scripted_unicycle(True)
    assert float(eng.robot_act("orca").abs().max()) <= float(LIM)
    assert eng.rollout("orca", T)["num_launches"] > 0
    eng.scripted_unicycle(False)
    refused(eng, "holonomic")
    eng.close()
    twin.close()
    # a unicycle mixed engine: served by cn_mixed_scripted alone it still refuses
    cm = _config(5)
    cm.sim.human_nums, cm.sim.human_nums_scripted = [3, 5], True
    cfgs, eg = make_varied_cn_configs(cm, [3, 5], E, phase="train", seed=7, rng="mt19937")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=True)
    mixed.reset()
    refused(mixed, "unicycle mixed engine")
    mixed.scripted_unicycle(True)
    assert mixed.rollout("orca", T)["num_launches"] > 0
    mixed.scripted_unicycle(False)
    refused(mixed, "unicycle mixed engine")
    mixed.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_holonomic_engine_is_untouched_by_the_optin(name):
    E, T = 13, 37
    c = _config(5, kin="holonomic")
    rows = []
    for optin in (False, True):
        eng = _engine(c, E, optin=optin)
        eng.reset()
        out = eng.rollout(name, T)
        got = _host(out)
        got["state"] = _blob(eng)
        rows.append((got, out["num_launches"]))
        eng.close()
    assert rows[0][1] == rows[1][1] == 2 + 2
    _same_rows(rows[1][0], rows[0][0], "holonomic with the opt-in")
    assert rows[0][0]["state"].tobytes() == rows[1][0]["state"].tobytes()
    assert np.abs(rows[0][0]["actions"]).max() > 0.5      # velocities, not unicycle actions


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def _evaluation(name, scripted):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.evaluation import evaluate, evaluate_scripted
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    E = 12
    c = _config(5, time_limit=10)
    c.env.test_size = 24
    envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="test")
    log = _Log()
    if scripted:
        ret = evaluate_scripted(name, envs, E, DEV, c, log, verbose=False)
    else:
        ret = evaluate(ScriptedRobot(envs, name), None, envs, E, DEV, c, log, verbose=False)
    envs.close()
    return log.lines, evaluate.last["records"], ret


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_evaluate_scripted_equals_evaluate_on_unicycle_envs(name):
    """24 test episodes on 12 unicycle envs (time_limit 10 s: 40 steps): the records, the logged lines and the
    returned lists of evaluate_scripted are those of evaluate() driven by ScriptedRobot.act step by step."""
    l0, r0, ret0 = _evaluation(name, False)
    l1, r1, ret1 = _evaluation(name, True)
    assert l0 == l1
    assert sorted(r0) == sorted(r1) and (r0["done"] == 1).all() and len(r0["done"]) == 24
    for k in r0:
        assert r0[k].tobytes() == r1[k].tobytes(), k
    assert ret0 == ret1


@pytest.mark.gpu
def test_gpu_cloning_lowers_the_nll_of_a_fixed_chunk_on_unicycle_envs():
    """BehaviourCloning on 16 unicycle envs x 8 steps (sigma 0.03 in action units): 30 updates on one stored chunk
    lower its negative log-likelihood; the labels are unicycle actions."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import BehaviourCloning
    from tests.helpers import make_policy

    E, N, T = 16, 5, 8
    c = _config(N, time_limit=1.5)
    c.training.num_processes, c.ppo.num_steps, c.ppo.num_mini_batch = E, T, 1
    envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
    pol = make_policy(N, E=E, T=T, device=DEV)
    pol.train()
    bc = BehaviourCloning(c, envs, pol, expert="orca", sigma=0.03, seed=11, lr=1e-3, num_mini_batch=1, value_coef=0.0)
    out = bc.collect()
    assert float(bc.rollouts.actions.abs().max()) <= float(LIM) and out["done"].any()
    assert float((out["executed"] - bc.rollouts.actions).abs().max()) > 0.01
    nll0 = float(bc.chunk_nll())
    bc.fit(30)
    nll1 = float(bc.chunk_nll())
    print("nll before %.6f, after 30 updates %.6f" % (nll0, nll1))
    assert np.isfinite(nll0) and np.isfinite(nll1) and nll1 < nll0, (nll0, nll1)
    envs.close()
