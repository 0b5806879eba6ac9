"""Closed-loop scripted rollouts (cn_rollout, CrowdNavEngine.rollout, ScriptedRobot.rollout, evaluate_scripted).

cn_rollout is DEFINED as the pair sequence cn_robot_act -> cn_step for t = 0..T-1 with every step's outputs kept
at row t. The reference of every GPU test is therefore a second engine of the same config and seed driven by an
eager loop of robot_act -> step (both pinned elsewhere in the suite), and the comparison is exact: rows as raw
bytes, the final state blobs byte for byte. The fused path (the controller inside the multi-step launches) runs the
same device functions under -ffp-contract=off, so any difference is a bug, not rounding. `num_launches` shows which
path ran."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config, make_cn_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orca", "social_force")
OBS = ("robot_node", "temporal_edges", "spatial_edges")
RECORDS = ("reward", "done", "event", "info", "ep_return", "ep_len")
ROWS = ("actions",) + OBS + RECORDS
EINVAL, EUNSUPPORTED = -1, -2


def _config(N, fov=2.0, kin="holonomic", rng="mt19937", time_limit=None, visible=False, policy="srnn"):
    c = clone_config(Config())
    c.sim.human_num = N
    c.robot.FOV = fov
    c.robot.visible = visible
    c.robot.policy = policy
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.env.rng = rng
    if time_limit is not None:
        c.env.time_limit = time_limit
    return c


# ---- CPU ----------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(REPO, "include", "crowdnav.h")).read()


def test_header_binding_and_export_list_agree_on_cn_rollout():
    from crowdnav_dsrnn_amd import _lib, build

    txt = _header()
    m = re.search(r"^int cn_rollout\((.*?)\);", txt, re.S | re.M)
    assert m, "include/crowdnav.h does not declare cn_rollout"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == [
        "cn_engine*", "void*", "int", "int", "constcn_rollout_out*", "int32_t*"]
    assert re.search(r"^#define CN_ROLLOUT_OBS_EVERY_STEP 1$", txt, re.M)
    assert _lib.ROLLOUT_OBS_EVERY_STEP == 1
    assert "cn_rollout" in _lib.EXPORTED
    build.build()
    L = _lib.lib()
    assert hasattr(L, "cn_rollout") and len(L.cn_rollout.argtypes) == len(params)
    nl = ctypes.c_int32(7)
    assert L.cn_rollout(None, None, 0, 4, None, ctypes.byref(nl)) == EINVAL   # a null engine, before any launch
    assert nl.value == 0 and b"null engine" in L.cn_last_error()


def test_ctypes_mirror_matches_the_header_struct():
    from crowdnav_dsrnn_amd import _lib

    m = re.search(r"typedef struct cn_rollout_out \{(.*?)\} cn_rollout_out;", _header(), re.S)
    assert m, "include/crowdnav.h does not define cn_rollout_out"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    size = {"int32_t": 4, "int64_t": 8, "float": 4, "double": 8, "uint8_t": 1, "int8_t": 1}
    off, align, names = 0, 1, []
    for f in fields:
        mm = re.match(r"^(\w+)\s*(\*?)\s*(\w+)$", f)
        assert mm, f
        n = ctypes.sizeof(ctypes.c_void_p) if mm.group(2) else size[mm.group(1)]
        off = (off + n - 1) // n * n + n
        align = max(align, n)
        names.append(mm.group(3))
    total = (off + align - 1) // align * align
    assert names == [f[0] for f in _lib.RolloutOut._fields_]
    assert ctypes.sizeof(_lib.RolloutOut) == total == 88
    for (name, ct), f in zip(_lib.RolloutOut._fields_, fields):
        assert (ct is ctypes.c_void_p) == ("*" in f), name


class _VenvStub:
    """What ScriptedRobot / evaluate_scripted read before they touch the engine (no GPU behind it)."""

    num_envs = 8

    def __init__(self, config, obs_mode="srnn"):
        self.config = config
        self.obs_mode = obs_mode

    def __getattr__(self, name):
        raise AssertionError("the check must come before the engine is touched (%s)" % name)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def test_rollout_entry_points_reject_unsupported_configs_without_a_gpu():
    from crowdnav_dsrnn_amd.evaluation import evaluate_scripted
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    good, uni = _config(5), _config(5, kin="unicycle")
    conv = _VenvStub(_config(5, policy="convgru"), obs_mode="convgru")
    robot = ScriptedRobot(_VenvStub(good), "orca")
    robot.venv = _VenvStub(uni)                      # (a config that changed under the actor)
    with pytest.raises(UnsupportedConfig):
        robot.rollout(4)
    robot.venv, robot.name = _VenvStub(good), "cadrl"
    with pytest.raises(UnsupportedConfig):
        robot.rollout(4)
    with pytest.raises(UnsupportedConfig):
        ScriptedRobot(conv, "social_force").rollout(4)
    for venv, name in ((_VenvStub(uni), "orca"), (_VenvStub(good), "cadrl"), (conv, "orca")):
        with pytest.raises(UnsupportedConfig):
            evaluate_scripted(name, venv, 8, "cpu", venv.config, _Log())


# ---- GPU ----------------------------------------------------------------------------------------
def _engine(c, E, chunk=None, budget=None, graph=False):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(make_cn_config(c, num_envs=E, nenv=E, phase="train"), "cuda:0")
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    if budget is not None:
        eng.set_spawn_budget(budget)
    return eng


def _blob(eng):
    return np.asarray(eng.get_state().blob).view(np.uint8).copy()


def _pairs(c, E, name, T, budget=None, warm=0):
    """The reference: an eager loop of robot_act -> step after cn_reset (and `warm` unrecorded pairs), every
    step's outputs cloned into row t; the rows as numpy arrays + the final state blob."""
    import torch

    eng = _engine(c, E, budget=budget)
    eng.reset()
    rows = {k: [] for k in ROWS}
    for t in range(warm + T):
        a = eng.robot_act(name)
        if t >= warm:
            rows["actions"].append(a.clone())
        obs, rew, done, ev, info, epr, epl = eng.step(a)
        if t >= warm:
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


def _host(out):
    import torch

    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ROWS if out.get(k) is not None}


def _same_rows(got, ref, what, keys=ROWS):
    for k in keys:
        g, r = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            bad = np.argwhere(g.view(np.uint8).reshape(g.shape[0], -1) != r.view(np.uint8).reshape(r.shape[0], -1))
            raise AssertionError("%s: %s differs first at step %d (%d bytes in all)" % (what, k, bad[0][0], len(bad)))


def _rollout(c, E, name, T, chunk=None, budget=None, graph=False, warm=0, **kw):
    """A fresh engine from cn_reset (+ `warm` eager pairs), one rollout(T): host rows, launches, state blob."""
    eng = _engine(c, E, chunk=chunk, budget=budget)
    eng.reset()
    for _ in range(warm):
        eng.step(eng.robot_act(name))
    if graph:
        eng.set_graph_mode(True)
    out = eng.rollout(name, T, **kw)
    got = _host(out)
    if graph:
        eng.set_graph_mode(False)
    got["state"] = _blob(eng)
    eng.close()
    return got, out["num_launches"]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 4])
@pytest.mark.parametrize("N", [1, 5, 9])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fused_rollout_equals_pairs(name, rng, N, chunk, visible=False):
    """E = 13 leaves every workgroup partial (16, 12, 7 envs per workgroup at N = 1, 5, 9); T = 37 = the single
    first step after cn_reset (a pair) + a full default chunk of 32 + a remainder of 4. time_limit 2 at time_step
    0.25: every env times out every few steps, so it auto-resets several times inside a launch and the
    controller acts on the new episode in the same launch. `visible` (tests/test_step_matrix.py): robot.visible."""
    E, T = 13, 37
    c = _config(N, rng=rng, time_limit=2, visible=visible)
    ref = _ref(("fused", name, rng, N) + (("visible",) if visible else ()), lambda: _pairs(c, E, name, T))
    got, nl = _rollout(c, E, name, T, chunk=chunk)
    C = 32 if chunk is None else chunk
    assert nl == 2 + math.ceil((T - 1) / C), nl
    _same_rows(got, ref, "%s %s N=%d chunk %s" % (name, rng, N, chunk))
    assert got["state"].tobytes() == ref["state"].tobytes()
    done_steps = np.nonzero(ref["done"].any(axis=1))[0]
    last_of_launch = {0} | {min(1 + k * C + C - 1, T - 1) for k in range(math.ceil((T - 1) / C))}
    assert any(int(t) not in last_of_launch for t in done_steps), done_steps
    assert ref["done"].sum(axis=0).min() >= 3, ref["done"].sum(axis=0)   # several resets per env
    assert np.abs(ref["actions"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("orca", 9), ("social_force", 10)])
def test_gpu_fused_rollout_equals_pairs_on_a_full_grid(name, N):
    """4096 envs: several step workgroups per CU on every XCD, where a controller that read a neighbour's state
    or a store the closing barrier did not order would show. T = 40: a pair, a full chunk and a remainder."""
    E, T = 4096, 40
    c = _config(N, time_limit=2)
    ref = _pairs(c, E, name, T)
    got, nl = _rollout(c, E, name, T)
    assert nl == 2 + 2, nl
    _same_rows(got, ref, "%s N=%d E=%d" % (name, N, E))
    assert got["state"].tobytes() == ref["state"].tobytes()
    assert ref["done"].sum() >= 6 * E


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", ["fov", "visible"])
def test_gpu_rollout_beliefs_and_visible_robot(case, name):
    """N = 5 with a robot FOV of pi: unseen humans become extrapolated belief rows and (15, 15) rows, which the
    controller then acts on. N = 9 with robot.visible: the step's simulators have A = 10 agents (the quad path's
    last size) and so has the robot's."""
    import torch

    E, T = 13, 37
    c = _config(5, fov=1.0, time_limit=4) if case == "fov" else _config(9, visible=True, time_limit=4)
    ref = _ref((case, name), lambda: _pairs(c, E, name, T))
    got, nl = _rollout(c, E, name, T)
    assert nl == 2 + 2, nl
    _same_rows(got, ref, "%s %s" % (case, name))
    assert got["state"].tobytes() == ref["state"].tobytes()
    if case == "fov":   # (15, 15) - robot position: a never-seen human's spatial edge
        rn, se = torch.from_numpy(ref["robot_node"]), torch.from_numpy(ref["spatial_edges"])
        unseen = ((se + rn[:, :, 0:1, 0:2] - 15.0).abs() < 1e-4).all(dim=-1)
        assert unseen.any() and not unseen.all()


@pytest.mark.gpu
@pytest.mark.parametrize("case,N,name,chunk,graph,fused", [
    ("orca at N + 1 = 11: pairs", 10, "orca", None, False, False),
    ("social force at N = 10: fused", 10, "social_force", None, False, True),
    ("chunk 1", 5, "orca", 1, False, False),
    ("graph mode", 5, "social_force", None, True, False),
    ("kd-tree step path, orca", 12, "orca", None, False, False),
    ("kd-tree step path, social force", 12, "social_force", None, False, False),
])
def test_gpu_rollout_fallbacks_give_the_same_rows(case, N, name, chunk, graph, fused):
    E, T = 13, 16
    c = _config(N, time_limit=3)
    ref = _ref(("fallback", N, name), lambda: _pairs(c, E, name, T))
    got, nl = _rollout(c, E, name, T, chunk=chunk, graph=graph)
    assert nl == (2 + 1 if fused else 2 * T), (case, nl)
    _same_rows(got, ref, case)
    assert got["state"].tobytes() == ref["state"].tobytes(), case
    assert ref["done"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_rollout_single_observation_row(name):
    """obs_every_step=False: the engine's own single-row observation buffers hold row T-1 of the per-step record;
    the other outputs are unchanged; NULL optional pointers are accepted; T = 0 and T = 1."""
    import torch

    from crowdnav_dsrnn_amd import _lib

    E, T = 13, 37
    c = _config(5, time_limit=2)
    ref = _ref(("fused", name, "mt19937", 5), lambda: _pairs(c, E, name, T))
    eng = _engine(c, E)
    eng.reset()
    out = eng.rollout(name, T, obs_every_step=False)
    got = _host(out)
    assert out["num_launches"] == 2 + 2
    for k in OBS:
        assert out[k] is getattr(eng, k)
        assert got[k].tobytes() == ref[k][T - 1].tobytes(), k
    _same_rows(got, ref, "single observation row", ("actions",) + RECORDS)
    assert _blob(eng).tobytes() == ref["state"].tobytes()
    eng.close()
    # only the required pointers, and T = 1 (from cn_reset: a pair), then T = 0 and T = 1 again (one fused launch)
    eng = _engine(c, E)
    eng.reset()
    buf = eng.rollout_buffers(1)
    req = {k: buf[k] for k in ("actions",) + OBS}
    o1 = eng.rollout(name, 1, out=req)
    assert o1["num_launches"] == 2 and o1["actions"] is buf["actions"]
    a0 = _host(o1)
    o0 = eng.rollout(name, 0)
    assert o0["num_launches"] == 0 and o0["actions"].shape == (0, E, 2)
    L = _lib.lib()
    ro = _lib.RolloutOut()
    for k in ("actions",) + OBS:
        setattr(ro, k, buf[k].data_ptr())
    ro.flags = 1
    nl = ctypes.c_int32(5)
    assert L.cn_rollout(eng._h, None, 0, 0, ctypes.byref(ro), ctypes.byref(nl)) == 0 and nl.value == 0
    full = {k: v.clone() for k, v in buf.items()}
    o2 = eng.rollout(name, 1, out=full)
    assert o2["num_launches"] == 1
    a1 = _host(o2)
    for k in ("actions",) + OBS:
        assert a0[k][0].tobytes() == ref[k][0].tobytes(), k
    for k in ROWS:
        assert a1[k][0].tobytes() == ref[k][1].tobytes(), k
    with pytest.raises(ValueError):
        eng.rollout(name, 1, out={k: v for k, v in full.items() if k != "spatial_edges"})
    with pytest.raises(ValueError):
        eng.rollout(name, 2, out=full)
    with pytest.raises(ValueError):
        eng.rollout("cadrl", 1)
    torch.cuda.synchronize()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tl", [1, 2])
def test_gpu_rollout_forced_spawn_parking(tl):
    """Spawn budget 1 (every pending spawn parks after each human) with time_limit 1 (every env resets at every
    step) and 2: phase 5 consumes, or draws inline, the spawns of several resets per env inside one launch, and the
    controller acts on each new episode; still the pairs' rows."""
    E, T = 13, 25
    c = _config(5, time_limit=tl)
    ref = _pairs(c, E, "orca", T, budget=1)
    got, nl = _rollout(c, E, "orca", T, budget=1)
    assert nl == 2 + 1, nl
    _same_rows(got, ref, "time_limit %d, budget 1" % tl)
    assert got["state"].tobytes() == ref["state"].tobytes()
    assert ref["done"].sum(axis=0).min() >= (T - 1 if tl == 1 else T // 5)


def _evaluation(name, scripted):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.evaluation import evaluate, evaluate_scripted
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    E = 8
    c = _config(5)
    c.env.test_size = 24
    envs = CrowdNavVecEnv(c, E, c.env.seed, "cuda:0", allow_early_resets=True, nenv=E, phase="test")
    log = _Log()
    if scripted:
        ret = evaluate_scripted(name, envs, E, "cuda:0", c, log, verbose=False)
    else:
        ret = evaluate(ScriptedRobot(envs, name), None, envs, E, "cuda:0", c, log, verbose=False)
    return log.lines, evaluate.last["records"], ret


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_evaluate_scripted_equals_evaluate(name):
    """24 test episodes on 8 envs: the per-episode records, the logged lines and the returned per-step lists of
    evaluate_scripted (whole rollouts) are those of evaluate() driven by ScriptedRobot.act step by step."""
    l0, r0, ret0 = _evaluation(name, False)
    l1, r1, ret1 = _evaluation(name, True)
    assert l0 == l1
    assert sorted(r0) == sorted(r1) and (r0["done"] == 1).all() and len(r0["done"]) == 24
    for k in r0:
        assert r0[k].tobytes() == r1[k].tobytes(), k
    assert ret0 == ret1


@pytest.mark.gpu
@pytest.mark.parametrize("T", [20, 30])
def test_gpu_rollout_profile_window_counts_steps(T):
    """cn_profile(eng, 1, 25) over rollouts of T steps at chunk 8 until the window is full: cn_profile_read reports
    25 steps (not launches); the launch that would straddle the end of the window is split there, and the rows
    are the pairs' all the same."""
    from crowdnav_dsrnn_amd import _lib

    K, E = 25, 13
    c = _config(5, time_limit=3)
    ref = _ref(("profile",), lambda: _pairs(c, E, "orca", 60, warm=1))
    eng = _engine(c, E, chunk=8)
    eng.reset()
    eng.step(eng.robot_act("orca"))   # (the first step after cn_reset is a pair; the window below starts fused)
    L = _lib.lib()
    _lib.check(L.cn_profile(eng._h, 1, K))
    t0, launches = 0, []
    while t0 < K:
        out = eng.rollout("orca", T)
        launches.append(out["num_launches"])
        got = _host(out)
        _same_rows(got, {k: ref[k][t0:t0 + T] for k in ROWS}, "window, steps %d.." % t0)
        t0 += T
    a_ms, b_ms, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    _lib.check(L.cn_profile_read(eng._h, ctypes.byref(a_ms), ctypes.byref(b_ms), ctypes.byref(n)))
    _lib.check(L.cn_profile(eng._h, 0, 0))
    eng.close()
    assert n.value == K and a_ms.value > 0.0
    # T = 20: 8 + 8 + 4, then 5 | 8 + 7; T = 30: 8 + 8 + 8 + 1 | 5
    assert launches == ([3, 3] if T == 20 else [5]), launches


@pytest.mark.gpu
def test_gpu_rollout_error_codes():
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.config import make_mixed_cn_configs
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    L = _lib.lib()
    E, T = 8, 4

    def call(eng, policy, T, ro):
        nl = ctypes.c_int32(9)
        rc = L.cn_rollout(eng._h, None, policy, T, None if ro is None else ctypes.byref(ro), ctypes.byref(nl))
        assert nl.value == 0
        return rc

    def args(N, drop=None):
        bufs = {"actions": torch.zeros((T, E, 2), device="cuda:0"), "robot_node": torch.zeros((T, E, 7), device="cuda:0"),
                "temporal_edges": torch.zeros((T, E, 2), device="cuda:0"),
                "spatial_edges": torch.zeros((T, E, N, 2), device="cuda:0")}
        ro = _lib.RolloutOut()
        for k, v in bufs.items():
            if k != drop:
                setattr(ro, k, v.data_ptr())
        ro.flags = 1
        return ro, bufs

    uni = CrowdNavEngine(make_cn_config(_config(5, kin="unicycle"), num_envs=E), "cuda:0")
    uni.reset()
    ro, keep = args(5)
    assert call(uni, 0, T, ro) == EUNSUPPORTED and b"holonomic" in L.cn_last_error()
    with pytest.raises(RuntimeError):
        uni.rollout("orca", T)
    uni.close()
    sc = ["parallel_traffic", "perpendicular_traffic"]
    ca, cb = _config(5), _config(3)
    ca.sim.train_val_sim = ca.sim.test_sim = cb.sim.train_val_sim = cb.sim.test_sim = sc
    cfgs, eg = make_mixed_cn_configs({sc[0]: ca, sc[1]: cb}, sc, E)
    mixed = CrowdNavEngine.mixed(cfgs, eg, "cuda:0")
    assert call(mixed, 1, T, ro) == EUNSUPPORTED and b"mixed" in L.cn_last_error()
    mixed.close()
    eng = CrowdNavEngine(make_cn_config(_config(5), num_envs=E), "cuda:0")
    eng.reset()
    before = _blob(eng)
    assert call(eng, 2, T, ro) == EINVAL
    assert call(eng, -1, T, ro) == EINVAL
    assert call(eng, 0, -1, ro) == EINVAL
    assert call(eng, 0, T, None) == EINVAL
    for drop in ("actions",) + OBS:
        bad, keep2 = args(5, drop)
        assert call(eng, 0, T, bad) == EINVAL, drop
    assert _blob(eng).tobytes() == before.tobytes()   # nothing was launched
    eng.close()
