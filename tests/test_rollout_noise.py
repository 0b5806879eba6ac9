"""Noise-injected scripted rollouts (cn_rollout_noisy, rollout(..., noise=)).

The executed action is DEFINED as x = a + sigma * n(seed, global env index, step0 + t) with a the clean action of
cn_robot_act (tests/rollout_noise_ref.py restates n and the float32 arithmetic in numpy), and everything else as
cn_rollout's pair sequence with x in place of a. So every GPU comparison is exact: `executed` against the restatement
applied to the recorded `actions`, and the rows and the final state blob against an eager loop
robot_act -> restatement -> step of a second engine of the same config. The fused launches, the launch triples
(chunk 1, graph mode, ORCA at 11 agents) and a call split in two must all give those rows."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_noise_ref as ref_noise  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config, make_cn_config  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS = ("robot_node", "temporal_edges", "spatial_edges")
RECORDS = ("reward", "done", "event", "info", "ep_return", "ep_len")
ROWS = ("actions", "executed") + OBS + RECORDS
EINVAL, EUNSUPPORTED = -1, -2
E, OFFSET, NENV, T, SIGMA, SEED, STEP0 = 13, 3, 20, 37, 0.2, 20240607, 5
CASES = [("orca", 5), ("orca", 9), ("orca", 10), ("social_force", 5)]


def _config(N, kin="holonomic", policy="srnn"):
    c = clone_config(Config())
    c.sim.human_num = N
    c.robot.FOV = 2.0
    c.robot.policy = policy
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.env.time_limit = 2.0
    c.env.time_step = 0.25
    return c


# ---- CPU ----------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(REPO, "include", "crowdnav.h")).read()


def test_header_declares_cn_rollout_noisy_and_its_struct():
    from crowdnav_dsrnn_amd import _lib

    txt = _header()
    m = re.search(r"^int cn_rollout_noisy\((.*?)\);", txt, re.S | re.M)
    assert m, "include/crowdnav.h does not declare cn_rollout_noisy"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == [
        "cn_engine*", "void*", "int", "int", "constcn_rollout_out*", "constcn_rollout_noise*", "int32_t*"]
    m = re.search(r"typedef struct cn_rollout_noise \{(.*?)\} cn_rollout_noise;", txt, re.S)
    assert m, "include/crowdnav.h does not define cn_rollout_noise"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.match(r"^(\w+)\s*(\*?)\s*(\w+)$", f.strip()).groups() for f in body.split(";") if f.strip()]
    assert fields == [("float", "", "sigma"), ("uint32_t", "", "seed"), ("int64_t", "", "step0"),
                      ("float", "*", "executed")]
    assert [f[0] for f in _lib.RolloutNoise._fields_] == [f[2] for f in fields]
    assert ctypes.sizeof(_lib.RolloutNoise) == 24
    assert _lib.RolloutNoise.step0.offset == 8 and _lib.RolloutNoise.executed.offset == 16


def test_export_list_names_cn_rollout_noisy():
    from crowdnav_dsrnn_amd import _lib

    assert "cn_rollout_noisy" in _lib.EXPORTED


def test_built_library_exports_cn_rollout_noisy():
    from crowdnav_dsrnn_amd import _lib, build

    build.build()
    L = _lib.lib()
    assert hasattr(L, "cn_rollout_noisy") and len(L.cn_rollout_noisy.argtypes) == 7


def test_null_engine_is_einval():
    from crowdnav_dsrnn_amd import _lib, build

    build.build()
    L = _lib.lib()
    nl = ctypes.c_int32(7)
    nz = _lib.RolloutNoise(0.2, 1, 0, None)
    assert L.cn_rollout_noisy(None, None, 0, 4, None, ctypes.byref(nz), ctypes.byref(nl)) == EINVAL
    assert nl.value == 0 and b"null engine" in L.cn_last_error()


def test_restatement_reproduces_random123_known_answers():
    """Random123's kat_vectors for philox4x32_10: zeros, all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in ref_noise.philox4x32_10(ctr, key)) == want
    n = ref_noise.unit_noise(0, 0, 0)   # from the first vector: words 0x6627e8d5, 0xe169c58d
    assert n.dtype == np.float32 and n.shape == (2,)
    assert float(n[0]) == 2.0 * (0x6627e8 / 2.0 ** 24) - 1.0 and float(n[1]) == 2.0 * (0xe169c5 / 2.0 ** 24) - 1.0
    big = ref_noise.unit_noise(9, np.arange(4096)[:, None], np.arange(64)[None, :])
    assert big.min() >= -1.0 and big.max() < 1.0 and abs(float(big.mean())) < 0.01
    a = np.full((2, 3, 2), -0.0, np.float32)
    assert ref_noise.perturb(a, 0.5, 1, 0, 0).shape == (2, 3, 2)
    # step0 continues the sequence; the env's global index selects the stream
    whole = ref_noise.perturb(np.zeros((6, 4, 2), np.float32), 0.2, 7, 10, 3)
    assert np.array_equal(whole[2:], ref_noise.perturb(np.zeros((4, 4, 2), np.float32), 0.2, 7, 12, 3))
    assert np.array_equal(whole[:, 1:], ref_noise.perturb(np.zeros((6, 3, 2), np.float32), 0.2, 7, 10, 4))


class _VenvStub:
    """What ScriptedRobot / evaluate_scripted read before they touch the engine (no GPU behind it)."""

    num_envs = 8

    def __init__(self, config, obs_mode="srnn"):
        self.config = config
        self.obs_mode = obs_mode

    def __getattr__(self, name):
        raise AssertionError("the check must come before the engine is touched (%s)" % name)


class _Log:
    def info(self, msg):
        pass


def test_noisy_entry_points_reject_unsupported_configs_without_a_gpu():
    from crowdnav_dsrnn_amd.engine import RolloutNoise
    from crowdnav_dsrnn_amd.evaluation import evaluate_scripted
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    good, uni = _config(5), _config(5, kin="unicycle")
    conv = _VenvStub(_config(5, policy="convgru"), obs_mode="convgru")
    for noise in (RolloutNoise(0.2, seed=1), {"sigma": 0.2, "seed": 1, "step0": 4}):
        robot = ScriptedRobot(_VenvStub(good), "orca")
        robot.venv = _VenvStub(uni)
        with pytest.raises(UnsupportedConfig):
            robot.rollout(4, noise=noise)
        robot.venv, robot.name = _VenvStub(good), "cadrl"
        with pytest.raises(UnsupportedConfig):
            robot.rollout(4, noise=noise)
        with pytest.raises(UnsupportedConfig):
            ScriptedRobot(conv, "social_force").rollout(4, noise=noise)
        for venv, name in ((_VenvStub(uni), "orca"), (_VenvStub(good), "cadrl"), (conv, "orca")):
            with pytest.raises(UnsupportedConfig):
                evaluate_scripted(name, venv, 8, "cpu", venv.config, _Log(), noise=noise)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            RolloutNoise(bad)
    with pytest.raises(ValueError):
        RolloutNoise.of({"sigma": 0.1, "sead": 3})
    assert RolloutNoise.of({"sigma": 0.1, "seed": 3}) == RolloutNoise(0.1, 3, 0) and RolloutNoise.of(None) is None


# ---- GPU ----------------------------------------------------------------------------------------
def _engine(c, chunk=None):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(make_cn_config(c, num_envs=E, env_offset=OFFSET, nenv=NENV, phase="train"), "cuda:0")
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    return eng


def _blob(eng):
    return np.asarray(eng.get_state().blob).view(np.uint8).copy()


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


def _noise(sigma=SIGMA, seed=SEED, step0=STEP0):
    from crowdnav_dsrnn_amd.engine import RolloutNoise

    return RolloutNoise(sigma, seed, step0)


def _rollout(name, N, calls=((T, STEP0),), chunk=None, graph=False, sigma=SIGMA, seed=SEED, noisy=True):
    """A fresh engine from cn_reset, then rollout(Tk, noise at step0 k) per call: host rows (concatenated), the
    launches per call and the state blob."""
    eng = _engine(_config(N), chunk=chunk)
    eng.reset()
    if graph:
        eng.set_graph_mode(True)
    parts, nls = [], []
    for Tk, s0 in calls:
        out = eng.rollout(name, Tk, noise=_noise(sigma, seed, s0)) if noisy else eng.rollout(name, Tk)
        parts.append(_host(out))
        nls.append(out["num_launches"])
    if graph:
        eng.set_graph_mode(False)
    got = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    got["state"] = _blob(eng)
    eng.close()
    return got, nls


def _eager(name, N):
    """The reference: a = robot_act(); x = restatement(a); step(x), every step's outputs cloned into row t."""
    import torch

    eng = _engine(_config(N))
    eng.reset()
    rows = {k: [] for k in ROWS}
    for t in range(T):
        a = eng.robot_act(name).clone()
        x = ref_noise.perturb(a.cpu().numpy()[None], SIGMA, SEED, STEP0 + t, OFFSET)[0]
        xd = torch.from_numpy(x).to("cuda:0")
        obs, rew, done, ev, info, epr, epl = eng.step(xd)
        rows["actions"].append(a)
        rows["executed"].append(xd)
        for k in OBS:
            rows[k].append(obs[k].clone())
        for k, v in zip(RECORDS, (rew, done, ev, info, epr, epl)):
            rows[k].append(v.clone())
    torch.cuda.synchronize()
    out = {k: torch.stack(v).cpu().numpy() for k, v in rows.items()}
    out["state"] = _blob(eng)
    eng.close()
    return out


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _fused(name, N):
    return _cached(("fused", name, N), lambda: _rollout(name, N))


def _launches(name, N, T1, first_after_reset=True):
    """cn_rollout_noisy's launches for T1 steps at the default chunk of 32."""
    if name == "orca" and N + 1 > 10:
        return 3 * T1
    rest = T1 - 1 if first_after_reset else T1
    return (3 if first_after_reset else 0) + (1 + -(-rest // 32) if rest > 0 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", CASES)
def test_gpu_executed_is_the_restatement_of_the_recorded_actions(name, N):
    got, nls = _fused(name, N)
    assert nls == [_launches(name, N, T)], nls
    want = ref_noise.perturb(got["actions"], SIGMA, SEED, STEP0, OFFSET)
    assert got["executed"].dtype == np.float32 and got["executed"].tobytes() == want.tobytes()
    assert np.abs(got["executed"] - got["actions"]).max() > 0.1   # (sigma 0.2: the noise is there)
    # every env times out every 8 steps: auto-resets inside the fused launches
    for b in range(T // 8):
        assert got["done"][8 * b:8 * b + 8].any(), b


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", CASES)
def test_gpu_fused_equals_chunk_one(name, N):
    got, _ = _fused(name, N)
    one, nls = _rollout(name, N, chunk=1)
    assert nls == [3 * T], nls
    _same_rows(got, one, "%s N=%d fused vs chunk 1" % (name, N))
    assert got["state"].tobytes() == one["state"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", CASES)
def test_gpu_rows_equal_the_eager_loop(name, N):
    got, _ = _fused(name, N)
    ref = _eager(name, N)
    _same_rows(got, ref, "%s N=%d vs robot_act -> restatement -> step" % (name, N))
    assert got["state"].tobytes() == ref["state"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", CASES)
def test_gpu_two_calls_continue_the_sequence(name, N):
    got, _ = _fused(name, N)
    two, nls = _rollout(name, N, calls=((20, STEP0), (17, STEP0 + 20)))
    assert nls == [_launches(name, N, 20), _launches(name, N, 17, first_after_reset=False)], nls
    _same_rows(got, two, "%s N=%d one call vs 20 + 17" % (name, N))
    assert got["state"].tobytes() == two["state"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", CASES)
def test_gpu_sigma_zero_is_cn_rollout(name, N):
    clean, _ = _rollout(name, N, noisy=False)
    zero, _ = _rollout(name, N, sigma=0.0)
    _same_rows(zero, clean, "%s N=%d sigma 0 vs cn_rollout" % (name, N), tuple(k for k in ROWS if k != "executed"))
    assert zero["state"].tobytes() == clean["state"].tobytes()
    assert zero["executed"].tobytes() == zero["actions"].tobytes()
    assert "executed" not in clean


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", CASES)
def test_gpu_graph_mode_gives_the_same_rows(name, N):
    got, _ = _fused(name, N)
    gm, nls = _rollout(name, N, graph=True)
    assert nls == [3 * T], nls
    _same_rows(got, gm, "%s N=%d graph mode" % (name, N))
    assert got["state"].tobytes() == gm["state"].tobytes()


@pytest.mark.gpu
def test_gpu_two_seeds_differ_in_executed_only_at_step_zero():
    a, _ = _fused("orca", 5)
    b, _ = _rollout("orca", 5, seed=SEED + 1)
    assert a["actions"][0].tobytes() == b["actions"][0].tobytes()
    assert (a["executed"][0] != b["executed"][0]).all()
    assert a["executed"].tobytes() != b["executed"].tobytes()


@pytest.mark.gpu
def test_gpu_rollout_noisy_error_codes():
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.config import make_mixed_cn_configs
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    L = _lib.lib()
    E8, T4 = 8, 4
    bufs = {"actions": torch.zeros((T4, E8, 2), device="cuda:0"), "robot_node": torch.zeros((T4, E8, 7), device="cuda:0"),
            "temporal_edges": torch.zeros((T4, E8, 2), device="cuda:0"),
            "spatial_edges": torch.zeros((T4, E8, 5, 2), device="cuda:0")}
    executed = torch.zeros((T4, E8, 2), device="cuda:0")
    ro = _lib.RolloutOut()
    for k, v in bufs.items():
        setattr(ro, k, v.data_ptr())
    ro.flags = 1

    def call(eng, sigma, null_noise=False):
        nl = ctypes.c_int32(9)
        nz = _lib.RolloutNoise(sigma, 1, 0, executed.data_ptr())
        rc = L.cn_rollout_noisy(eng._h, None, 0, T4, ctypes.byref(ro), None if null_noise else ctypes.byref(nz),
                                ctypes.byref(nl))
        assert nl.value == 0
        return rc

    def cfg(kin="holonomic", N=5):
        c = _config(N, kin=kin)
        return c

    uni = CrowdNavEngine(make_cn_config(cfg("unicycle"), num_envs=E8), "cuda:0")
    uni.reset()
    before = _blob(uni)
    assert call(uni, 0.2) == EUNSUPPORTED and b"holonomic" in L.cn_last_error()
    assert _blob(uni).tobytes() == before.tobytes()
    uni.close()
    sc = ["parallel_traffic", "perpendicular_traffic"]
    ca, cb = cfg(), cfg(N=3)
    ca.sim.train_val_sim = ca.sim.test_sim = cb.sim.train_val_sim = cb.sim.test_sim = sc
    cfgs, eg = make_mixed_cn_configs({sc[0]: ca, sc[1]: cb}, sc, E8)
    mixed = CrowdNavEngine.mixed(cfgs, eg, "cuda:0")
    mixed.reset()
    mb = [np.asarray(v.blob).view(np.uint8).copy() for _, v in mixed.get_state()]
    assert call(mixed, 0.2) == EUNSUPPORTED and b"mixed" in L.cn_last_error()
    for x, (_, v) in zip(mb, mixed.get_state()):
        assert x.tobytes() == np.asarray(v.blob).view(np.uint8).tobytes()
    mixed.close()
    eng = CrowdNavEngine(make_cn_config(cfg(), num_envs=E8), "cuda:0")
    eng.reset()
    before = _blob(eng)
    for sigma in (-1.0, float("nan"), float("inf")):
        assert call(eng, sigma) == EINVAL, sigma
        assert _blob(eng).tobytes() == before.tobytes(), sigma
    assert call(eng, 0.2, null_noise=True) == EINVAL
    assert _blob(eng).tobytes() == before.tobytes()
    torch.cuda.synchronize()
    assert float(executed.abs().max()) == 0.0 and float(bufs["actions"].abs().max()) == 0.0   # nothing was launched
    eng.close()
