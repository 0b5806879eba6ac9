"""Scripted rollouts that record the visibility mask (cn_rollout_masked, rollout(..., mask=True), the opt-in
config.sim.visible_masks_scripted).

The mask is booleans from one device function shared by cn_visible_mask's kernel and the rollout kernels, and every
other row is a copy of what cn_rollout / cn_rollout_noisy record, so every GPU comparison is exact. The yardstick is
always the existing eager path on a second engine of the same config: robot_act -> (the noise restatement of
tests/rollout_noise_ref.py) -> step -> visible_mask, the blob read at the end. Shapes are tests/test_rollout_noise.py's:
13 envs at env_offset 3 of 20, 37 steps, time_limit 2.0 at time_step 0.25 (every env auto-resets at least four times),
noise sigma 0.2, seed 20240607, step0 5. robot.FOV counts in units of pi."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_noise_ref as ref_noise  # noqa: E402

from crowdnav_dsrnn_amd.config import (Config, UnsupportedConfig, clone_config, make_cn_config,  # noqa: E402
                                       make_varied_cn_configs)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
OBS = ("robot_node", "temporal_edges", "spatial_edges")
RECORDS = ("reward", "done", "event", "info", "ep_return", "ep_len")
ROWS = ("actions", "executed", "visible_masks") + OBS + RECORDS
EINVAL, EUNSUPPORTED = -1, -2
E, OFFSET, NENV, T, SIGMA, SEED, STEP0 = 13, 3, 20, 37, 0.2, 20240607, 5
NUMS = [1, 5, 12]
# name: (controller, humans (None: the mixed engine of NUMS), robot.FOV, kinematics, the rollout's path)
CASES = {
    "orca5": ("orca", 5, 0.5, "holonomic", "fused"),
    "orca9": ("orca", 9, 1.0, "holonomic", "fused"),          # the largest fused ORCA (7 envs per workgroup)
    "sf5": ("social_force", 5, 0.5, "holonomic", "fused"),    # the lane-per-env controller
    "orca10": ("orca", 10, 0.5, "holonomic", "pairs"),        # N + 1 > 10
    "orca12": ("orca", 12, 1.0, "holonomic", "pairs"),        # the kd-tree step path
    "uni5": ("orca", 5, 0.5, "unicycle", "fused"),            # scripted_unicycle: the float32 r_theta heading
    "dwa5": ("dwa", 5, 0.5, "unicycle", "pairs"),             # scripted_dwa
    "full5": ("orca", 5, 2.0, "holonomic", "fused"),          # vis360: all ones bar coincident agents
    "mixed": ("orca", None, 0.5, "holonomic", "mixed"),       # human_nums [1, 5, 12]: a partial workgroup per group
}
PLAIN = [k for k in CASES if k != "mixed"]
FUSED = [k for k, v in CASES.items() if v[4] == "fused"]


def _config(N=5, fov=0.5, kin="holonomic", name="orca", masks=False, scripted=False, rng=None):
    c = clone_config(Config())
    c.sim.human_num = N
    c.robot.FOV = fov
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.env.time_limit = 2.0
    c.env.time_step = 0.25
    if rng is not None:
        c.env.rng = rng
    if kin == "unicycle":
        c.robot.scripted_unicycle = name != "dwa"
        c.robot.scripted_dwa = True if name == "dwa" else None
    c.sim.visible_masks = masks
    c.sim.visible_masks_scripted = scripted
    return c


# ---- CPU ----------------------------------------------------------------------------------------
def test_header_binding_and_export_list_agree_on_cn_rollout_masked():
    from crowdnav_dsrnn_amd import _lib, build

    txt = open(os.path.join(REPO, "include", "crowdnav.h")).read()
    m = re.search(r"^int cn_rollout_masked\((.*?)\);", txt, re.S | re.M)
    assert m, "include/crowdnav.h does not declare cn_rollout_masked"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == [
        "cn_engine*", "void*", "int", "int", "constcn_rollout_out*", "constcn_rollout_noise*", "float*", "int32_t*"]
    assert "cn_rollout_masked" in _lib.EXPORTED
    build.build()
    L = _lib.lib()
    assert hasattr(L, "cn_rollout_masked") and len(L.cn_rollout_masked.argtypes) == len(params)
    nl = ctypes.c_int32(7)
    assert L.cn_rollout_masked(None, None, 0, 4, None, None, None, ctypes.byref(nl)) == EINVAL
    assert nl.value == 0 and b"null engine" in L.cn_last_error()


def test_opt_in_is_off_by_default_and_needs_visible_masks():
    from crowdnav_dsrnn_amd.config import no_visible_masks, visible_masks_scripted

    assert Config().sim.visible_masks_scripted is False
    c = _config()
    assert visible_masks_scripted(c) is False and no_visible_masks(c, "x") is False
    del c.sim.visible_masks_scripted                     # absent counts as off
    assert visible_masks_scripted(c) is False and no_visible_masks(c, "x") is False
    c.sim.visible_masks = True
    with pytest.raises(UnsupportedConfig, match="visible_masks_scripted"):
        no_visible_masks(c, "x")                         # (as before, and the message now names the opt-in)
    c = _config(scripted=True)                           # the opt-in without sim.visible_masks
    for fn in (visible_masks_scripted, lambda cc: no_visible_masks(cc, "x")):
        with pytest.raises(UnsupportedConfig) as ei:
            fn(c)
        assert "visible_masks_scripted" in str(ei.value) and "sim.visible_masks" in str(ei.value)
    c = _config(masks=True, scripted=True)
    assert visible_masks_scripted(c) is True and no_visible_masks(c, "x") is True


def test_config_only_checks_pass_with_both_keys():
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner.imitation import BehaviourCloning
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    c = _config(masks=True, scripted=True)
    venv = types.SimpleNamespace(config=c, obs_mode="srnn")   # (no engine: the checks read the config alone)
    ScriptedRobot.check_rollout(venv, "orca")
    ScriptedRobot.check_rollout(venv, "social_force")
    # BehaviourCloning's checks pass; the first thing it needs after them is the env itself
    with pytest.raises(AttributeError, match="num_envs"):
        BehaviourCloning(c, venv, types.SimpleNamespace(srnn=True), expert="orca")
    bad = _config(scripted=True)
    with pytest.raises(UnsupportedConfig, match="visible_masks_scripted"):
        ScriptedRobot.check_rollout(types.SimpleNamespace(config=bad, obs_mode="srnn"), "orca")
    with pytest.raises(UnsupportedConfig, match="visible_masks_scripted"):
        BehaviourCloning(bad, types.SimpleNamespace(config=bad, obs_mode="srnn"), types.SimpleNamespace(srnn=True))
    with pytest.raises(UnsupportedConfig, match="visible_masks_scripted"):
        CrowdNavVecEnv(bad, 4, 0, "cpu")


# ---- GPU ----------------------------------------------------------------------------------------
def _engine(case, chunk=None, N=None, rng=None):
    """`N`, `rng` (tests/test_step_matrix.py): the plain case at another human count / under another RNG."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    name, n_case, fov, kin, _ = CASES[case]
    assert N is None or n_case is not None
    N = n_case if N is None else N
    if N is None:
        c = _config(max(NUMS), fov, kin, name)
        c.sim.human_nums = list(NUMS)
        cfgs, eg = make_varied_cn_configs(c, NUMS, E, env_offset=OFFSET, nenv=NENV, phase="train")
        eng = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=True)
    else:
        eng = CrowdNavEngine(make_cn_config(_config(N, fov, kin, name, rng=rng), num_envs=E, env_offset=OFFSET, nenv=NENV,
                                            phase="train"), DEV, scripted_unicycle=kin == "unicycle" and name != "dwa",
                             scripted_dwa=True if name == "dwa" else None)
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    return eng


def _blob(eng):
    import torch

    torch.cuda.synchronize()
    st = eng.get_state()
    views = [st] if eng.groups is None else [v for _, v in st]
    return b"".join(np.asarray(v.blob).view(np.uint8).tobytes() for v in views)


def _noise(sigma=SIGMA, step0=STEP0):
    from crowdnav_dsrnn_amd.engine import RolloutNoise

    return RolloutNoise(sigma, SEED, step0)


def _same_rows(got, ref, what, keys=None):
    for k in keys or [k for k in ROWS if k in ref]:
        g, r = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            bad = np.argwhere(g.view(np.uint8).reshape(g.shape[0], -1) != r.view(np.uint8).reshape(r.shape[0], -1))
            raise AssertionError("%s: %s differs first at step %d (%d bytes in all)" % (what, k, bad[0][0], len(bad)))


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _variant(N, rng):
    return () if N is None and rng is None else (N, rng)


def _eager(case, noisy, N=None, rng=None):
    """The reference: a = robot_act(); x = restatement(a) (noisy) or a; step(x); visible_mask() -- every step's
    outputs cloned into row t, the blob at the end. Also the figures of the premises, from this run alone."""
    import torch

    def make():
        name = CASES[case][0]
        eng = _engine(case, N=N, rng=rng)
        eng.reset()
        rows = {k: [] for k in ROWS}
        real = eng.human_mask.cpu().numpy()
        prem = {"stale_exact": 0, "reset_mask": eng.visible_mask().cpu().numpy().copy()}
        for t in range(T):
            a = eng.robot_act(name).clone()
            x = a
            if noisy:
                x = torch.from_numpy(ref_noise.perturb(a.cpu().numpy()[None], SIGMA, SEED, STEP0 + t, OFFSET)[0]).to(DEV)
            obs, rew, done, ev, info, epr, epl = eng.step(x)
            rows["actions"].append(a)
            rows["executed"].append(x.clone())
            rows["visible_masks"].append(eng.visible_mask().clone())
            for k in OBS:
                rows[k].append(obs[k].clone())
            for k, v in zip(RECORDS, (rew, done, ev, info, epr, epl)):
                rows[k].append(v.clone())
            if eng.groups is None:   # invisible slots whose belief is the true state bit for bit
                sv, m = eng.get_state(), rows["visible_masks"][-1].cpu().numpy()
                same = np.ones((E, eng.N), bool)
                for b, h in (("b_px", "h_px"), ("b_py", "h_py"), ("b_vx", "h_vx"), ("b_vy", "h_vy")):
                    same &= (np.asarray(getattr(sv, b)).reshape(E, -1).view(np.uint64)
                             == np.asarray(getattr(sv, h)).reshape(E, -1).view(np.uint64))
                prem["stale_exact"] += int((same & (m == 0.0)).sum())
        torch.cuda.synchronize()
        out = {k: torch.stack(v).cpu().numpy() for k, v in rows.items()}
        out["state"] = _blob(eng)
        eng.close()
        m, done = out["visible_masks"], out["done"].astype(bool)
        prem["resets"] = done.sum(axis=0)
        prem["share"] = float(m[:, real].mean())
        prev = np.concatenate([prem["reset_mask"][None], m[:-1]])
        prem["done_rows_changed"] = int((m != prev).any(axis=2)[done].sum())
        prem["real"] = real
        out["premises"] = prem
        return out

    return _cached(("eager", case, noisy) + _variant(N, rng), make)


def _rollout(case, noisy=True, calls=((T, STEP0),), chunk=None, graph=False, every=True, sigma=SIGMA, mask=True,
             N=None, rng=None):
    """A fresh engine from cn_reset, then one rollout per call (noise continued at step0): host rows (concatenated),
    the launches per call and the state blob. The mask buffer is poisoned first, so an unwritten slot shows."""
    import torch

    name = CASES[case][0]
    eng = _engine(case, chunk=chunk, N=N, rng=rng)
    eng.reset()
    if graph:
        eng.set_graph_mode(True)
    parts, nls = [], []
    for Tk, s0 in calls:
        bufs = eng.rollout_buffers(Tk, obs_every_step=every, executed=noisy, mask=mask)
        if mask:
            bufs["visible_masks"].fill_(7.0)
        out = eng.rollout(name, Tk, obs_every_step=every, out=bufs, noise=_noise(sigma, s0) if noisy else None,
                          mask=mask)
        torch.cuda.synchronize()
        parts.append({k: out[k].cpu().numpy() for k in ROWS if out.get(k) is not None})
        nls.append(out["num_launches"])
    if graph:
        eng.set_graph_mode(False)
    single = () if every else OBS + ("visible_masks",)   # (one row each: the last call's is the last step's)
    got = {k: parts[-1][k] if k in single else np.concatenate([p[k] for p in parts]) for k in parts[0]}
    got["state"] = _blob(eng)
    eng.close()
    return got, nls


def _default(case, noisy, N=None, rng=None):
    return _cached(("rollout", case, noisy) + _variant(N, rng), lambda: _rollout(case, noisy, N=N, rng=rng))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_premises_hold_on_the_eager_run(case, N=None, rng=None):
    """Asserted on the eager reference alone: the shapes exercise what the comparisons below are about."""
    fov = CASES[case][2]
    for noisy in (True, False):
        p = _eager(case, noisy, N, rng)["premises"]
        print(case, "noisy" if noisy else "clean", "resets min", int(p["resets"].min()), "visible share", p["share"],
              "done rows whose mask changed", p["done_rows_changed"], "invisible slots with an exact belief",
              p["stale_exact"])
        assert p["resets"].min() >= 4, p["resets"]
        if fov < 2:
            assert 0.1 < p["share"] < 0.9, p["share"]
            assert p["done_rows_changed"] >= 1               # the reset path wrote some of the rows
            if case != "mixed":
                assert p["stale_exact"] >= 1                 # the mask is not derivable from the observation
        else:
            assert p["share"] > 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [True, False], ids=["noisy", "clean"])
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_rows_equal_the_eager_loop(case, noisy, N=None, rng=None):
    got, _ = _default(case, noisy, N, rng)
    ref = _eager(case, noisy, N, rng)
    assert set(np.unique(got["visible_masks"])) <= {0.0, 1.0}
    keys = [k for k in ROWS if noisy or k != "executed"]
    _same_rows(got, ref, "%s vs robot_act -> step -> visible_mask" % case, keys)
    assert got["state"] == ref["state"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_every_row_cn_rollout_records_is_unchanged(case):
    """The rollout without the mask (cn_rollout_noisy) on a second engine: the same rows, the same blob."""
    got, _ = _default(case, True)
    plain, _ = _cached(("plain", case), lambda: _rollout(case, True, mask=False))
    assert "visible_masks" not in plain
    _same_rows(got, plain, "%s masked vs cn_rollout_noisy" % case, [k for k in ROWS if k != "visible_masks"])
    assert got["state"] == plain["state"]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 5])
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_chunks_give_the_same_rows(case, chunk, N=None, rng=None):
    got, _ = _default(case, True, N, rng)
    other, nls = _rollout(case, True, chunk=chunk, N=N, rng=rng)
    _same_rows(got, other, "%s default chunk vs %d" % (case, chunk))
    assert got["state"] == other["state"]
    if chunk == 1 and case != "mixed":
        assert nls == [4 * T], nls   # robot_act, the perturbation, step, visible_mask


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_two_calls_continue_the_sequence(case):
    got, _ = _default(case, True)
    two, _ = _rollout(case, True, calls=((17, STEP0), (20, STEP0 + 17)))
    _same_rows(got, two, "%s one call vs 17 + 20" % case)
    assert got["state"] == two["state"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLAIN)
def test_gpu_graph_mode_gives_the_same_rows(case):
    got, _ = _default(case, True)
    gm, nls = _rollout(case, True, graph=True)
    assert nls == [4 * T], nls
    _same_rows(got, gm, "%s graph mode" % case)
    assert got["state"] == gm["state"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_single_row_holds_the_last_steps_mask(case):
    got, _ = _default(case, True)
    one, _ = _rollout(case, True, calls=((17, STEP0), (20, STEP0 + 17)), every=False)
    n = got["visible_masks"].shape[-1]
    assert one["visible_masks"].shape == (E, n)
    assert one["visible_masks"].tobytes() == got["visible_masks"][-1].tobytes()
    for k in OBS:
        assert one[k].tobytes() == got[k][-1].tobytes(), k
    _same_rows(got, one, "%s single observation row" % case, ("actions", "executed") + RECORDS)
    assert got["state"] == one["state"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLAIN)
def test_gpu_no_launch_is_added_on_the_fused_path(case):
    """cn_rollout / cn_rollout_noisy at the same arguments on a second engine: on the fused path the launches are
    theirs (the one pair after cn_reset gets its mask launch: + 1 in the first call, + 0 in a call that continues);
    elsewhere theirs plus one per step."""
    fused = CASES[case][4] == "fused"
    calls = ((17, STEP0), (20, STEP0 + 17))
    for noisy in (True, False):
        _, masked = _rollout(case, noisy, calls=calls)
        _, plain = _rollout(case, noisy, calls=calls, mask=False)
        want = [plain[0] + 1, plain[1]] if fused else [plain[0] + 17, plain[1] + 20]
        assert masked == want, (case, noisy, masked, plain)
        if fused:   # 17 steps: the pair and one launch of 16; 20 steps: one launch (the noise block: one more each)
            assert plain == ([3 + 2, 2] if noisy else [2 + 1, 1]), plain


@pytest.mark.gpu
def test_gpu_sigma_zero_is_the_rollout_without_noise():
    clean, n0 = _default("orca5", False)
    zero, n1 = _rollout("orca5", True, sigma=0.0)
    _same_rows(zero, clean, "sigma 0 vs no noise", [k for k in ROWS if k != "executed"])
    assert zero["state"] == clean["state"] and zero["executed"].tobytes() == zero["actions"].tobytes()
    assert n1 == [n0[0] + 1], (n0, n1)   # the copy into `executed`


@pytest.mark.gpu
def test_gpu_mixed_engine_pads_with_zeros_and_equals_plain_engines():
    import torch

    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    got, _ = _default("mixed", True)
    m = got["visible_masks"]
    counts = [NUMS[(OFFSET + r) % len(NUMS)] for r in range(E)]
    assert m.shape == (T, E, max(NUMS)) and sorted(set(counts)) == sorted(NUMS)
    for r in range(E):
        assert (m[:, r, counts[r]:] == 0.0).all(), r      # padded slots: exactly 0 in every row
    name, _, fov, kin, _ = CASES["mixed"]
    for r in range(E):
        p = CrowdNavEngine(make_cn_config(_config(counts[r], fov, kin, name), num_envs=1, env_offset=OFFSET + r,
                                          nenv=NENV, phase="train"), DEV)
        p.reset()
        out = p.rollout(name, T, noise=_noise(), mask=True)
        torch.cuda.synchronize()
        assert out["visible_masks"].cpu().numpy().tobytes() == m[:, r:r + 1, :counts[r]].tobytes(), r
        assert out["actions"].cpu().numpy().tobytes() == got["actions"][:, r:r + 1].tobytes(), r
        assert out["done"].cpu().numpy().tobytes() == got["done"][:, r:r + 1].tobytes(), r
        p.close()


@pytest.mark.gpu
def test_gpu_error_codes():
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    L = _lib.lib()
    E8, T4, N = 8, 4, 5
    bufs = {"actions": torch.zeros((T4, E8, 2), device=DEV), "robot_node": torch.zeros((T4, E8, 7), device=DEV),
            "temporal_edges": torch.zeros((T4, E8, 2), device=DEV),
            "spatial_edges": torch.zeros((T4, E8, N, 2), device=DEV)}
    mask = torch.full((T4, E8, N), 7.0, device=DEV)
    ro = _lib.RolloutOut()
    for k, v in bufs.items():
        setattr(ro, k, v.data_ptr())
    ro.flags = 1

    def call(eng, null_mask=False, sigma=None):
        nl = ctypes.c_int32(9)
        nz = None if sigma is None else ctypes.byref(_lib.RolloutNoise(sigma, 1, 0, None))
        rc = L.cn_rollout_masked(eng._h, None, 0, T4, ctypes.byref(ro), nz, None if null_mask else mask.data_ptr(),
                                 ctypes.byref(nl))
        assert nl.value == 0
        return rc

    eng = CrowdNavEngine(make_cn_config(_config(N), num_envs=E8), DEV)
    eng.reset()
    before = _blob(eng)
    assert call(eng, null_mask=True) == EINVAL and b"mask" in L.cn_last_error()
    for sigma in (-1.0, float("nan"), float("inf")):
        assert call(eng, sigma=sigma) == EINVAL, sigma
    assert _blob(eng) == before
    eng.close()
    uni = CrowdNavEngine(make_cn_config(_config(N, kin="unicycle"), num_envs=E8), DEV)   # without its opt-in
    uni.reset()
    before = _blob(uni)
    assert call(uni) == EUNSUPPORTED and b"holonomic" in L.cn_last_error()
    assert _blob(uni) == before
    uni.close()
    c = _config(N)
    c.sim.human_nums = [3, 5]
    cfgs, eg = make_varied_cn_configs(c, [3, 5], E8, phase="train")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV)                                          # without cn_mixed_scripted
    mixed.reset()
    before = _blob(mixed)
    assert call(mixed) == EUNSUPPORTED and b"mixed" in L.cn_last_error()
    assert _blob(mixed) == before
    mixed.close()
    torch.cuda.synchronize()
    assert float((mask - 7.0).abs().max()) == 0.0 and float(bufs["actions"].abs().max()) == 0.0   # nothing was launched


def _envs(c, n_env, phase="train"):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    return CrowdNavVecEnv(c, n_env, c.env.seed, DEV, allow_early_resets=True, nenv=n_env, phase=phase)


@pytest.mark.gpu
@pytest.mark.parametrize("with_noise", [False, True])
def test_gpu_vecenv_rollout_equals_robot_act_step_device(with_noise):
    import torch

    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    keys, Tv = OBS + ("visible_masks",), 20
    c = _config(masks=True, scripted=True)
    a, b = _envs(c, E), _envs(c, E)
    a.reset()
    b.reset()
    noise = _noise() if with_noise else None
    out = ScriptedRobot(a, "orca").rollout(Tv, noise=noise)
    assert tuple(out["visible_masks"].shape) == (Tv, E, 5)
    seen = 0.0
    for t in range(Tv):
        act = b.robot_act("orca")
        assert torch.equal(act, out["actions"][t]), t
        if with_noise:
            act = torch.from_numpy(ref_noise.perturb(act.cpu().numpy()[None], SIGMA, SEED, STEP0 + t, 0)[0]).to(DEV)
        obs = b.step_device(act)[0]
        for k in keys:
            assert torch.equal(obs[k].reshape(out[k][t].shape), out[k][t]), (k, t)
        seen += float(obs["visible_masks"].mean())
    assert 0.1 < seen / Tv < 0.9
    act = b.robot_act("orca").clone()     # a step after the rollout continues identically
    oa, ob = a.step_device(act), b.step_device(act)
    for k in keys:
        assert torch.equal(oa[0][k], ob[0][k]), k
    for x, y in zip(oa[1:], ob[1:]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # without the opt-in the env refuses as before, and obs_every_step=False keeps one row
    last = a.rollout("orca", 3, obs_every_step=False)
    assert tuple(last["visible_masks"].shape) == (E, 5)
    assert torch.equal(last["visible_masks"], a.engine.visible_mask())
    a.close()
    b.close()
    off = _envs(_config(masks=True), 4)
    with pytest.raises(UnsupportedConfig, match="visible_masks"):
        off.rollout("orca", 3)
    off.close()


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


@pytest.mark.gpu
def test_gpu_behaviour_cloning_records_and_uses_the_mask():
    import torch

    from crowdnav_dsrnn_amd.learner import BehaviourCloning
    from tests.helpers import make_policy

    n_env, Tb = 16, 8
    c = _config(masks=True, scripted=True)
    envs = _envs(c, n_env)
    pol = make_policy(5, E=n_env, T=Tb, device=DEV)
    pol.train()
    bc = BehaviourCloning(c, envs, pol, expert="orca", sigma=0.2, seed=11, num_steps=Tb, num_mini_batch=1)
    eng = envs.engine
    before = eng.get_state()
    reset_mask = eng.visible_mask().clone()
    out = bc.collect()
    r = bc.rollouts
    torch.cuda.synchronize()
    stored = r.obs["visible_masks"].clone()
    assert tuple(stored.shape) == (Tb + 1, n_env, 5) and out["visible_masks"].data_ptr() == r.obs["visible_masks"][1:].data_ptr()
    assert torch.equal(stored[0], reset_mask)
    executed = out["executed"].clone()
    eng.set_state(before)                  # replay the chunk eagerly with the recorded executed actions
    for t in range(Tb):
        eng.step(executed[t].contiguous())
        assert torch.equal(stored[t + 1], eng.visible_mask()), t
    assert 0.1 < float(stored.mean()) < 0.9
    nll = float(bc.chunk_nll())
    r.obs["visible_masks"].fill_(1.0)
    nll_ones = float(bc.chunk_nll())
    r.obs["visible_masks"].copy_(stored)
    print("nll with the recorded mask %.9g, with all ones %.9g" % (nll, nll_ones))
    assert np.isfinite(nll) and np.isfinite(nll_ones) and nll != nll_ones   # the masked attention was used
    st = bc.update()
    assert np.isfinite(st["nll"]) and np.isfinite(st["value_loss"])
    envs.close()


@pytest.mark.gpu
def test_gpu_evaluate_scripted_report_equals_the_plain_envs():
    from crowdnav_dsrnn_amd.evaluation import evaluate, evaluate_scripted

    n_env = 8
    runs = []
    for masks in (True, False):
        c = _config(masks=masks, scripted=masks)
        c.env.test_size = 24
        c.env.time_limit = 30.0   # (long enough for episodes to end in success or collision as well)
        envs = _envs(c, n_env, phase="test")
        log = _Log()
        ret = evaluate_scripted("orca", envs, n_env, DEV, c, log, verbose=False)
        runs.append((log.lines, {k: v.tobytes() for k, v in evaluate.last["records"].items()}, ret))
        envs.close()
    assert runs[0] == runs[1]
    assert len(runs[0][0]) > 0 and evaluate.last["success_rate"] > 0
