"""helpers.compare_info / compare_monitor notice what they are there to notice (CPU only: the oracle alone).

Two 20-step oracle rollouts (64 envs): the holonomic side-preference config (N = 1, robot.v_pref = 2.0; odd envs
steer at the human so that some collide with human 0, whose MIN_DIST is inf; env 0 moves at exactly
social.max_walking_speed) and the C3 shape (25 humans, square_crossing, FOV pi: goal-change overflows). Each
mutation below changes a copy of the oracle's own outputs the way a subtly wrong kernel would, and the helper must
name the column; on the untouched copy it must report nothing."""
import numpy as np
import pytest

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config
from tests import helpers as H

E, T = 64, 20
LIMIT = 1.5   # social.max_walking_speed


def _rollout(oracle, shape):
    c = clone_config(Config())
    c.humans.policy = "orca"
    c.action_space.kinematics = "holonomic"
    if shape == "side":
        c.sim.human_num = 1
        c.sim.train_val_sim = c.sim.test_sim = ["side_pref_passing", "side_pref_overtaking", "side_pref_crossing"]
        c.test.side_preference = True
        c.humans.random_goal_changing = c.humans.end_goal_changing = False
        c.sim.circle_radius = 4
        c.robot.v_pref = 2.0
    else:
        c.sim.human_num = 25
        c.sim.train_val_sim = c.sim.test_sim = ["square_crossing"]
        c.robot.FOV = c.humans.FOV = 1.0
    assert c.social.max_walking_speed == LIMIT
    cfg = make_cn_config(c, num_envs=E)
    ref = oracle.RefEngine(cfg)
    ref.reset()
    rng = np.random.RandomState(5)
    rec = {k: [] for k in ("act", "info", "event", "done", "epr", "epl", "ovf_post", "min_dist_ref")}
    for t in range(T):
        pre = ref.get_state()
        a = rng.normal(0, 0.8, (E, 2))
        if shape == "side":
            d = np.stack([pre.h_px[:, 0] - pre.r_px, pre.h_py[:, 0] - pre.r_py], axis=1)
            a[1::2] = 1.2 * d[1::2] / np.linalg.norm(d[1::2], axis=1, keepdims=True)
            a[0] = (LIMIT, 0.0) if t % 2 else (0.0, -LIMIT)
        a = a.astype(np.float32)
        _, _, done, ev, info, epr, epl = ref.step(a)
        for k, v in zip(rec, (a, info, ev, done, epr, epl, np.asarray(ref.get_state().overflow).astype(np.float32),
                              H.min_dist_ref(pre))):
            rec[k].append(np.array(v))
    rec = {k: np.stack(v) for k, v in rec.items()}
    for v in rec.values():
        v.setflags(write=False)
    return cfg, rec


@pytest.fixture(scope="module")
def side(oracle):
    return _rollout(oracle, "side")


@pytest.fixture(scope="module")
def c3(oracle):
    return _rollout(oracle, "c3")


def _report(rec, got):
    """compare_info of every step of a mutated copy `got` against the rollout: the mismatch strings."""
    return [m for t in range(T) for m in H.compare_info(got[t], rec["info"][t], rec["event"][t], where="t=%d " % t)]


def _columns(errs):
    return {m.split("info ")[1].split(":")[0] for m in errs}


@pytest.mark.parametrize("shape", ["side", "c3"])
def test_untouched_copy_is_clean(shape, side, c3):
    _, rec = side if shape == "side" else c3
    assert _report(rec, rec["info"].copy()) == []
    for t in range(T):
        assert H.compare_monitor(rec["epr"][t].copy(), rec["epl"][t].copy(), rec["epr"][t], rec["epl"][t],
                                 rec["done"][t]) == []


@pytest.mark.parametrize("shape", ["side", "c3"])
def test_min_dist_ref_is_the_oracles(shape, side, c3):
    """helpers.min_dist_ref (the fixture path's MIN_DIST on rows where the reference records none) against the
    oracle's column on every row, inf rows included."""
    _, rec = side if shape == "side" else c3
    got, want = rec["info"][:, :, abi.INFO_MIN_DIST].astype(np.float64), rec["min_dist_ref"]
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert np.abs(got[fin] - want[fin]).max() <= H.POS_TOL


def test_side_columns_swapped(side):
    _, rec = side
    live = rec["info"][:, :, abi.INFO_SIDE_LEFT] != rec["info"][:, :, abi.INFO_SIDE_RIGHT]
    assert live.sum() >= 20, int(live.sum())
    got = rec["info"].copy()
    got[:, :, [abi.INFO_SIDE_LEFT, abi.INFO_SIDE_RIGHT]] = got[:, :, [abi.INFO_SIDE_RIGHT, abi.INFO_SIDE_LEFT]]
    errs = _report(rec, got)
    assert _columns(errs) == {"SIDE_LEFT", "SIDE_RIGHT"}, errs[:3]
    assert len(errs) == 2 * int(live.any(axis=1).sum())   # both columns, in every step with a live row


def test_overflow_delayed_by_one_step(c3):
    """The counter read after the step's goal changes / auto-reset instead of before the step."""
    _, rec = c3
    got = rec["info"].copy()
    got[:, :, abi.INFO_OVERFLOW] = rec["ovf_post"]
    moved = rec["ovf_post"] != rec["info"][:, :, abi.INFO_OVERFLOW]
    assert moved.sum() >= 20, int(moved.sum())
    errs = _report(rec, got)
    assert _columns(errs) == {"OVERFLOW"}, errs[:3]
    assert len(errs) == int(moved.any(axis=1).sum())


def test_speed_violation_with_greater_or_equal(side):
    """Env 0 moves at exactly the limit: `>` (crowd_sim.py:1024) does not flag it, `>=` would."""
    _, rec = side
    a = rec["act"]
    on_limit = np.sqrt(a[:, :, 0] * a[:, :, 0] + a[:, :, 1] * a[:, :, 1]) == np.float32(LIMIT)
    assert on_limit[:, 0].all() and on_limit.sum() == T
    assert (rec["info"][:, 0, abi.INFO_SPEED_VIOLATION] == 0).all()
    assert (rec["info"][:, :, abi.INFO_SPEED_VIOLATION] == 1).sum() >= 20   # the column is live both ways
    got = rec["info"].copy()
    got[:, :, abi.INFO_SPEED_VIOLATION][on_limit] = 1.0
    errs = _report(rec, got)
    assert _columns(errs) == {"SPEED_VIOLATION"} and len(errs) == T, errs[:3]


def test_min_dist_inf_made_finite(side):
    _, rec = side
    inf = np.isinf(rec["info"][:, :, abi.INFO_MIN_DIST])
    assert inf.sum() >= 5, int(inf.sum())
    assert (rec["event"][inf] == abi.EV_COLLISION).all()   # N = 1: the only human is in collision
    got = rec["info"].copy()
    got[:, :, abi.INFO_MIN_DIST][inf] = 3.0e38
    errs = _report(rec, got)
    assert _columns(errs) == {"MIN_DIST"} and len(errs) == int(inf.any(axis=1).sum()), errs[:3]
    got = rec["info"].copy()   # and a finite value turned into inf, a NaN on either side
    fin_row = tuple(np.argwhere(~inf)[0])
    got[:, :, abi.INFO_MIN_DIST][fin_row] = np.inf
    assert _columns(_report(rec, got)) == {"MIN_DIST"}
    got[:, :, abi.INFO_MIN_DIST][fin_row] = np.nan
    assert _columns(_report(rec, got)) == {"MIN_DIST"}


def test_min_dist_off_a_danger_row(c3):
    """MIN_DIST is compared on every row: 3e-5 m off on a row that is not Danger."""
    _, rec = c3
    rows = np.argwhere((rec["event"] == abi.EV_NOTHING) & np.isfinite(rec["info"][:, :, abi.INFO_MIN_DIST]))
    assert len(rows)
    got = rec["info"].copy()
    got[:, :, abi.INFO_MIN_DIST][tuple(rows[0])] += 3e-5
    errs = _report(rec, got)
    assert _columns(errs) == {"MIN_DIST"} and len(errs) == 1, errs[:3]


@pytest.mark.parametrize("shape", ["side", "c3"])
def test_jerk_scaled(shape, side, c3):
    _, rec = side if shape == "side" else c3
    got = rec["info"].copy()
    got[:, :, abi.INFO_JERK_COST] *= np.float32(1 + 1e-3)
    # 1e-3 * jerk exceeds atol 1e-4 + rtol 1e-5 * jerk from jerk = 0.102 up
    assert (rec["info"][:, :, abi.INFO_JERK_COST] > 0.11).any(axis=1).all()
    errs = _report(rec, got)
    assert _columns(errs) == {"JERK_COST"} and len(errs) == T, errs[:3]


@pytest.mark.parametrize("shape", ["side", "c3"])
def test_monitor_off_by_one(shape, side, c3):
    _, rec = side if shape == "side" else c3
    assert rec["done"].sum() >= 5, int(rec["done"].sum())
    hits = 0
    for t in range(T):
        if not rec["done"][t].any():
            continue
        e = int(np.nonzero(rec["done"][t])[0][0])
        epl = rec["epl"][t].copy()
        epl[e] += 1
        errs = H.compare_monitor(rec["epr"][t], epl, rec["epr"][t], rec["epl"][t], rec["done"][t])
        assert len(errs) == 1 and "ep_len" in errs[0], errs
        epr = rec["epr"][t].copy()
        epr[e] += 3e-4
        errs = H.compare_monitor(epr, rec["epl"][t], rec["epr"][t], rec["epl"][t], rec["done"][t])
        assert len(errs) == 1 and "ep_return" in errs[0], errs
        keep = np.ones(E, bool)
        keep[e] = False   # a row masked for ep_return still has its ep_len compared
        assert H.compare_monitor(epr, rec["epl"][t], rec["epr"][t], rec["epl"][t], rec["done"][t], keep=keep) == []
        assert len(H.compare_monitor(epr, epl, rec["epr"][t], rec["epl"][t], rec["done"][t], keep=keep)) == 1
        hits += 1
    assert hits


def test_personal_violation_allowance_only_on_the_threshold():
    """Free-running allowance: a PERSONAL_VIOLATION difference passes only where want's MIN_DIST is within
    POS_TOL of min_personal_space, and is counted; without min_personal_space nothing passes."""
    mps = 0.2
    want = np.zeros((3, abi.INFO_K), np.float32)
    want[:, abi.INFO_MIN_DIST] = [mps + 5e-6, mps + 1e-3, np.inf]
    got = want.copy()
    got[:, abi.INFO_PERSONAL_VIOLATION] = 1
    ev = np.zeros(3, np.int8)
    assert "3 of 3" in H.compare_info(got, want, ev)[0]
    tally = {}
    errs = H.compare_info(got, want, ev, min_personal_space=mps, tally=tally)
    assert len(errs) == 1 and "PERSONAL_VIOLATION: 2 of 3" in errs[0], errs
    assert tally == {"rows": 3, "personal_flips": 1}
