"""The CPU oracle (oracle/cpu_ref.c) against golden vectors recorded from the REFERENCE itself
(oracle/gen_golden.py runs the reference's CrowdSimDict through import shims). Pins the oracle
before it is trusted as the GPU checker."""
import glob
import os

import numpy as np
import pytest

from crowdnav_dsrnn_amd import abi
from tests import helpers as H

SPAWN = sorted(os.path.basename(p) for p in glob.glob(os.path.join(H.GOLDEN, "spawn_*.npz")))
ROLL = sorted(os.path.basename(p) for p in glob.glob(os.path.join(H.GOLDEN, "roll_*.npz")))


def test_fixtures_present():
    assert len(SPAWN) >= 24 and len(ROLL) >= 28, (SPAWN, ROLL)


# every config field the *_cfg_* fixtures vary away from its default (oracle/gen_golden.py:config_cases)
CFG_FIELDS = {
    "env__time_step", "env__time_limit", "sim__circle_radius", "sim__square_width", "robot__radius", "robot__v_pref",
    "humans__radius", "humans__v_pref", "env__randomize_attributes", "humans__goal_change_chance",
    "humans__end_goal_change_chance", "reward__success_reward", "reward__collision_penalty",
    "reward__potential_factor", "reward__discomfort_penalty_factor", "reward__discomfort_dist_front",
    "reward__discomfort_dist_back", "orca__neighbor_dist", "orca__safety_space", "orca__time_horizon", "sf__A",
    "sf__B", "sf__KI", "reward__norm_zone_side", "reward__norm_zone_penalty", "social__min_personal_space",
    "social__max_walking_speed", "env__test_size", "env__seed"}


@pytest.mark.parametrize("names", [SPAWN, ROLL], ids=["spawn", "roll"])
def test_config_fixtures_cover_every_varied_field(names):
    """The spawn fixtures and the rollout fixtures each vary every field of CFG_FIELDS, to a value that differs
    from the default Config's, and phase 'test' is recorded: a deleted or re-recorded-at-defaults fixture fails
    here instead of silently narrowing what pins the oracle."""
    from crowdnav_dsrnn_amd.config import Config

    seen, phases = set(), set()
    for name in names:
        d = H.load(name)
        for k, v in H.meta_overrides(d).items():
            sec, fld = k.split("__")
            if v != getattr(getattr(Config, sec), fld):
                seen.add(k)
        phases.add(str(d["meta_phase"]) if "meta_phase" in d else "train")
    assert CFG_FIELDS <= seen, sorted(CFG_FIELDS - seen)
    assert phases == {"train", "test"}, phases


def test_tl7_fixture_times_out():
    """roll_cfg_tl7 (time_limit 7) is there for the Timeout branch at a non-default limit."""
    assert (H.load("roll_cfg_tl7.npz")["event"] == abi.EV_TIMEOUT).sum() >= 4


def test_mt19937_matches_numpy(oracle):
    """numpy legacy RandomState is the reference's RNG (crowd_sim_dict.py:154)."""
    for seed in (0, 1, 2000, 2001, 123456789, 2**32 - 1):
        got = oracle.mt_draw(seed, 1500)
        want = np.random.RandomState(seed).random_sample(1500)
        assert np.array_equal(got, want), seed


@pytest.mark.parametrize("name", SPAWN)
def test_spawn_bit_exact(oracle, name):
    """CrowdSimDict.reset() states and first observations, bit-exact (tolerance 0)."""
    d = H.load(name)
    cfg = H.cn_config_from_meta(d)
    eng = oracle.RefEngine(cfg)
    for k in range(int(d["resets"])):
        pre = H.state_from(d, "k%d_pre_" % k, cfg)
        eng.set_state(pre)
        obs = eng.reset()
        errs = H.compare_state(eng.get_state(), d, "k%d_post_" % k, tol=0.0)
        assert not errs, errs
        for key, ok in (("robot_node", "robot_node"), ("temporal", "temporal_edges"), ("spatial", "spatial_edges")):
            assert np.array_equal(obs[ok].reshape(d["k%d_%s" % (k, key)].shape), d["k%d_%s" % (k, key)]), key


@pytest.mark.parametrize("name", ROLL)
def test_rollout_teacher_forced(oracle, name):
    """Teacher-forced CrowdSimDict.step + VecEnv auto-reset + Monitor: exact events/done/flags/indices,
    1e-5 on positions, rewards and observations (north-star tolerance)."""
    d = H.load(name)
    cfg = H.cn_config_from_meta(d)
    eng = oracle.RefEngine(cfg)
    errs = H.run_teacher_forced(eng, d, cfg, tol=H.POS_TOL)
    assert not errs, "\n".join(errs[:20])


def test_rollouts_cover_every_event():
    seen = set()
    for name in ROLL:
        seen |= set(np.unique(H.load(name)["event"]).tolist())
    assert seen == {abi.EV_NOTHING, abi.EV_DANGER, abi.EV_COLLISION, abi.EV_REACHGOAL, abi.EV_TIMEOUT}, seen
