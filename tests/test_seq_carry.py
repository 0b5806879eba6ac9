"""Multi-step launches (the SEQ kernels of cn_step_kernel), which compute the info-only values in their last step
only and hand the state from step to step inside one launch, against the same engine at set_seq_chunk(1): the
single-step kernels, which compute everything in every step and which the rest of the suite pins to the oracle.
The nine outputs of the last step and the whole state blob, bit for bit.

The cases are the places where a step of a launch depends on what the step before it left: the belief on the
main path and on the 360-degree fallback, the info columns in the step that stores them, a reset inside a launch
beside envs that go on, the other step paths (social force, norm zones, side preference) and the state at a
launch's end. (They were written for a build that also kept the state in LDS across the steps; that
part was measured slower and is not in the source, the cases hold for any such change.) Every case asserts on the
reference run the condition that makes it a test (a belief that differs from the position, a reset inside a
launch, an info column that is not trivially zero ...): a case whose premise does not hold fails instead of
passing vacuously. The action streams come from a CPU generator, so they are the same on every machine."""
import os
import sys

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (the C5 side-preference scenario definitions)

pytestmark = pytest.mark.gpu

OUTPUTS = ("robot_node", "temporal_edges", "spatial_edges", "reward", "done", "event", "info", "ep_return", "ep_len")


def _cfg(N=10, kin="unicycle", E=13, fov=None, time_limit=None, policy="orca", norm_zones=False, base=None, sims=None):
    c = clone_config(base if base is not None else Config())
    c.sim.human_num = N
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = list(sims or ["circle_crossing"])
    c.humans.policy = policy
    c.reward.norm_zones = norm_zones
    if fov is not None:
        c.robot.FOV = c.humans.FOV = fov
    if time_limit is not None:
        c.env.time_limit = time_limit
    return make_cn_config(c, num_envs=E, nenv=E, phase="train")


def _actions(T, E, kin, seed):
    """unicycle: U[-0.1, 0.1]^2 (the C2 benchmark's); holonomic: N(0, 0.5^2)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kin == "unicycle":
        a = torch.rand((T, E, 2), generator=g) * 0.2 - 0.1
    else:
        a = torch.randn((T, E, 2), generator=g) * 0.5
    return a.to("cuda:0").contiguous()


def _run(cfg, acts, ops, chunk=None, state0=None):
    """A fresh engine from cn_reset (or cn_set_state of `state0`), then `ops`: ("seq", a, b) = one step_seq call
    over acts[a:b]. Returns the nine outputs of the last step, the state blob and its StateView."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(cfg, "cuda:0")
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    if state0 is None:
        eng.reset()
    else:
        eng.set_state(state0)
    for op in ops:
        eng.step_seq(acts[op[1]:op[2]])
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in OUTPUTS}
    sv = eng.get_state()
    out["state"] = np.asarray(sv.blob).view(np.uint8).copy()
    eng.close()
    return out, sv


def _same(got, ref, what):
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s: %s" % (what, k))


def _check(cfg, acts, chunks, premise, what):
    """The chunk-1 reference (its premise asserted), then every chunk length against it."""
    T = acts.shape[0]
    ref, sv = _run(cfg, acts, [("seq", 0, T)], chunk=1)
    premise(ref, sv)
    for chunk in chunks:
        got, _ = _run(cfg, acts, [("seq", 0, T)], chunk=chunk)
        _same(got, ref, "%s, chunk %d" % (what, chunk))
    return ref, sv


def _belief_off(sv):
    """[E, N]: the robot's belief of the human is not the human's position."""
    return (sv.b_px != sv.h_px) | (sv.b_py != sv.h_py)


@pytest.mark.parametrize("kin", ["holonomic", "unicycle"])
def test_belief_carried_on_main_path(kin):
    """Robot and human FOV of pi: the belief fields are loaded in phase 0 and extrapolated for every human outside
    the robot's FOV, step after step. E = 13 leaves a partial last workgroup (6 envs per workgroup)."""
    E, T = 13, 37
    cfg = _cfg(10, kin, E, fov=1.0)

    def premise(ref, sv):
        n = int(_belief_off(sv).sum())
        print("belief != position for %d of %d humans" % (n, E * 10))
        assert n >= E * 10 // 10, n

    _check(cfg, _actions(T, E, kin, 5), (2, 8, 32), premise, "FOV pi, %s" % kin)


def test_belief_fallback_360_inside_a_launch():
    """Default (360-degree) FOV: the belief is read only where the robot cannot see a human at all. A NaN action
    makes one env's robot state NaN from step 4 on, so all its humans take that fallback in every later step: it
    must extrapolate the belief the previous step of the same launch left, not a value from global memory."""
    E, T, bad, t_bad = 13, 20, 7, 4
    cfg = _cfg(10, "holonomic", E)
    acts = _actions(T, E, "holonomic", 9)
    acts[t_bad, bad, :] = float("nan")
    _, sv_mid = _run(cfg, acts, [("seq", 0, t_bad + 1)], chunk=1)

    def premise(ref, sv):
        print("reset_count of env %d: %d after step %d, %d at the end; belief != position for %d of its humans"
              % (bad, sv_mid.reset_count[bad], t_bad, sv.reset_count[bad], int(_belief_off(sv)[bad].sum())))
        assert sv.reset_count[bad] == sv_mid.reset_count[bad]
        assert _belief_off(sv)[bad].all()

    _check(cfg, acts, (8, 32), premise, "NaN action")


@pytest.mark.parametrize("kin", ["unicycle", "holonomic"])
def test_info_columns_where_they_are_emitted(kin):
    """The C2 configuration (and a holonomic variant): the path violation (velocity rectangles and their
    intersection test) and the other info-only values are computed in the launch's last step only, from the state
    the steps before it carried."""
    E, T = 64, 40
    cfg = _cfg(10, kin, E)

    def premise(ref, sv):
        info = ref["info"].reshape(E, abi.INFO_K)
        nv = int((info[:, abi.INFO_PATH_VIOLATION] > 0).sum())
        print("%s: PATH_VIOLATION > 0 in %d of %d envs, min AGG_NAV_TIME %g"
              % (kin, nv, E, info[:, abi.INFO_AGG_NAV_TIME].min()))
        assert nv >= 1
        assert (info[:, abi.INFO_AGG_NAV_TIME] > 0).all()

    _check(cfg, _actions(T, E, kin, 1), (8, 32), premise, "info, %s" % kin)


@pytest.mark.parametrize("tl", [2, 1])
def test_reload_after_reset_beside_carried_envs(tl):
    """time_limit = 2: every env resets every few steps, inside a launch, in its second-to-last and in its last
    step, beside envs that carry their state; time_limit = 1: every env reloads in every step. FOV pi, so the
    reloaded belief is read."""
    E, T = 13, 33
    cfg = _cfg(10, "unicycle", E, fov=1.0, time_limit=tl)

    def premise(ref, sv):
        rc = np.asarray(sv.reset_count).astype(np.int64) - 1   # (reset_count is 1 after cn_reset)
        print("time_limit %d: resets per env %s" % (tl, rc))
        assert (rc >= (T if tl == 1 else (1 + T) // 5)).all(), rc

    _check(cfg, _actions(T, E, "unicycle", 23), (8, 32), premise, "time_limit %d" % tl)


def test_social_force_humans():
    """humans.policy = social_force: the human lanes' own path-violation test and human_post."""
    E, T = 13, 30
    cfg = _cfg(10, "holonomic", E, policy="social_force")

    def premise(ref, sv):
        assert not np.array_equal(sv.h_vx, np.zeros_like(sv.h_vx))

    _check(cfg, _actions(T, E, "holonomic", 2), (8,), premise, "social force")


def test_norm_zones_ladder_after_phase_2():
    """reward.norm_zones: the reward ladder (ep_return, ep_len, potential, gtime) runs after phase 2."""
    E, T = 13, 30
    cfg = _cfg(5, "holonomic", E, norm_zones=True)

    def premise(ref, sv):
        assert (np.asarray(sv.ep_len) > 0).all() or (np.asarray(sv.reset_count) > 1).any()

    _check(cfg, _actions(T, E, "holonomic", 4), (8,), premise, "norm zones")


def test_side_preference_scenario():
    """One side-preference scenario of the C5 workload as a plain engine: 1 human per env, 16 envs per workgroup,
    the side-preference info columns."""
    E, T = 50, 30
    scen = "side_pref_passing"
    cfg = _cfg(1, "holonomic", E, norm_zones=True, base=bench.c5_scenario_configs()[scen], sims=[scen])
    assert cfg.side_preference

    def premise(ref, sv):
        info = ref["info"].reshape(E, abi.INFO_K)
        print("separation: min %g max %g" % (info[:, abi.INFO_SEPARATION].min(), info[:, abi.INFO_SEPARATION].max()))
        assert (info[:, abi.INFO_SEPARATION] > 0).all()

    _check(cfg, _actions(T, E, "holonomic", 6), (8,), premise, "side preference")


def test_state_complete_at_every_launch_end():
    """Two step_seq calls of 5 and 32 steps with the state taken out after the first and put into a fresh engine:
    everything a later launch needs is in global memory when a launch ends."""
    E, T = 13, 37
    cfg = _cfg(10, "unicycle", E, fov=1.0)
    acts = _actions(T, E, "unicycle", 8)
    ref, sv = _run(cfg, acts, [("seq", 0, T)], chunk=1)
    assert _belief_off(sv).any()
    _, mid = _run(cfg, acts, [("seq", 0, 5)])
    got, _ = _run(cfg, acts, [("seq", 5, T)], state0=mid)
    _same(got, ref, "get_state / set_state between two calls")
