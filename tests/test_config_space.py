"""The engine over the numeric config space: every numeric field of cn_config that the step, reset and spawn
kernels read, at a value away from its default, GPU against the CPU oracle (which tests/test_oracle_golden.py
pins to the reference at the same settings through the *_cfg_* fixtures), and the bounded rejection loops at
small max_tries.

Teacher-forced cases use _cfg / _actions / _teacher_forced of tests/test_gpu_parity.py unchanged: 64 envs x 60
steps = 3,840 rows, RandomState(5), done / event / flags exact, 1e-5 on rewards, observations and state, the whole
info row and the Monitor pair. No case can go vacuous: the CPU tests here run the oracle at the varied setting and
at its twin (the same shape with the fields under test back at their defaults) on the same actions and assert a
floor on the rows whose reward / info row differs; each floor is half the count measured on the oracle, which is
quoted next to it."""
import numpy as np
import pytest

from crowdnav_dsrnn_amd import abi
from tests import helpers as H
from tests.test_gpu_parity import _actions, _cfg, _teacher_forced

E, STEPS = 64, 60
SQ = "square_crossing"
TRAFFIC = ("parallel_traffic", "perpendicular_traffic")


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from crowdnav_dsrnn_amd.engine import NumpyEngine

    return NumpyEngine


def _case(kin="holonomic", N=5, policy="orca", scen="circle_crossing", fov=2.0, base=None, over=None, live=None):
    """`over`: the fields under test; `base`: settings the case and its twin share; `live`: {what: count
    measured on the oracle}, what = "reward" / "info" (rows that differ from the twin's), "timeout" (Timeout
    rows) or "done" (episodes ended: resets that move the case counter). The floor is half the count."""
    return dict(kin=kin, N=N, policy=policy, scen=scen, fov=fov, base=base or {}, over=over or {}, live=live or {})


TL4 = {"env__time_limit": 4}
PHILOX = {"env__rng": "philox"}
_SQ31 = {"sim__square_width": 31}
_GOALCHG = {"humans__goal_change_chance": 0.7, "humans__end_goal_change_chance": 0.4}
_TEST_WRAP = {"phase": "test", "env__test_size": 5, "env__seed": 77}
_ORCA_KD = {"orca__neighbor_dist": 3, "orca__safety_space": 0.3, "orca__time_horizon": 8}

# name: case. The first 16 are the settings of the roll_cfg_* / spawn_cfg_* fixtures (robot.radius also alone);
# then the ones the reference cannot record; then three Philox twins.
CASES = {
    "ts01": _case(over={"env__time_step": 0.1}, live={"reward": 3776, "info": 3776}),
    "ts04_uni": _case("unicycle", 6, over={"env__time_step": 0.4}, live={"reward": 3772, "info": 3776}),
    "tl7": _case(N=3, over={"env__time_limit": 7}, live={"reward": 2226, "info": 2165, "timeout": 121}),
    "radius35_uni": _case("unicycle", 5, over={"sim__circle_radius": 3.5}, live={"reward": 3768, "info": 3840}),
    "sq31": _case(N=12, scen=SQ, over=_SQ31, live={"reward": 810, "info": 3840}),
    "rr045": _case(over={"robot__radius": 0.45, "robot__v_pref": 0.7}, live={"reward": 3726, "info": 3840}),
    "robot_radius_alone": _case(over={"robot__radius": 0.45}, live={"reward": 663, "info": 3837}),
    "hum": _case(N=6, over={"humans__radius": 0.22, "humans__v_pref": 1.4, "env__randomize_attributes": False},
                 live={"reward": 1039, "info": 3840}),
    "goalchg": _case(over=_GOALCHG, live={"reward": 208, "info": 2163}),
    "rewards": _case(base={"sim__circle_radius": 4},
                     over={"reward__success_reward": 3.5, "reward__collision_penalty": -7.25,
                           "reward__potential_factor": 0.75, "reward__discomfort_penalty_factor": 1.3},
                     live={"reward": 3739}),
    "disc06": _case(over={"reward__discomfort_dist_front": 0.6, "reward__discomfort_dist_back": 0.6},
                    live={"reward": 494, "info": 1355}),
    "orca": _case(N=9, over={"orca__neighbor_dist": 3, "orca__safety_space": 0.05, "orca__time_horizon": 2},
                  live={"reward": 740, "info": 3695}),
    "sf": _case(N=6, policy="social_force", over={"sf__A": 3.5, "sf__B": 0.6, "sf__KI": 2.5},
                live={"reward": 960, "info": 3774}),
    # all 74 rows come from the penalty: the side alone changes 0 of the 3,840 rows on the oracle, as it must (the
    # reference builds both zones around the robot itself, crowd_sim.py:917-926, and 'rhs' is the mirror image of
    # 'lhs' about the robot's heading, helper.py:262-275, so its disc meets a zone in the same states)
    "nz_rhs": _case(scen=TRAFFIC, base={"reward__norm_zones": True},
                    over={"reward__norm_zone_side": "rhs", "reward__norm_zone_penalty": -1.25}, live={"reward": 74}),
    "social": _case(over={"social__min_personal_space": 0.5, "social__max_walking_speed": 0.7}, live={"info": 2660}),
    "test_wrap": _case(base=TL4, over=_TEST_WRAP, live={"reward": 3450, "info": 3840, "done": 281}),
    "seed_train": _case(base=TL4, over={"env__seed": 123456789}, live={"reward": 3494, "info": 3840}),
    # beyond the recorder: the reference's unbounded rejection never ends at square_width 12, its RVO2 stand-in is
    # too slow at N = 14, its reset raises KeyError in phase 'val' (parity section)
    "sq12_N12": _case(N=12, scen=SQ, over={"sim__square_width": 12}, live={"reward": 1824, "info": 3840}),
    "sq31_N25_kd": _case(N=25, scen=SQ, over=_SQ31, live={"reward": 1224, "info": 3840}),
    "orca_kd_N14": _case(N=14, scen=SQ, over=_ORCA_KD, live={"reward": 785, "info": 3775}),
    "ts04_uni_N10": _case("unicycle", 10, over={"env__time_step": 0.4}, live={"reward": 3771, "info": 3776}),
    "phase_val9": _case("unicycle", 10, base=TL4, over={"phase": "val", "env__val_size": 9},
                        live={"reward": 3251, "info": 3840, "done": 256}),
    "phase_test11_offset": _case(base=TL4, over={"phase": "test", "env__test_size": 11, "env_offset": 37, "nenv": 200},
                                 live={"reward": 3436, "info": 3840, "done": 274}),
    "philox_sq31": _case(N=12, scen=SQ, base=PHILOX, over=_SQ31, live={"reward": 1085, "info": 3840}),
    "philox_goalchg": _case(base=PHILOX, over=_GOALCHG, live={"reward": 259, "info": 2072}),
    "philox_test_wrap": _case(base=dict(TL4, **PHILOX), over=_TEST_WRAP, live={"reward": 3452, "info": 3840, "done": 278}),
}


def _case_cfg(case, twin=False):
    over = dict(case["base"]) if twin else dict(case["base"], **case["over"])
    return _cfg(case["N"], case["kin"], case["scen"], case["policy"], E, case["fov"], **over)


def _oracle_run(oracle, cfg, kin, steps=STEPS, seed=5):
    """The oracle's side of _teacher_forced alone (the GPU follows the oracle there, so the oracle's trajectory
    is this free run): stacked reward [T][E], info [T][E][K], event [T][E], done [T][E], and the final state."""
    ref = oracle.RefEngine(cfg)
    ref.reset()
    rng = np.random.RandomState(seed)
    rew, info, ev, done = [], [], [], []
    for t in range(steps):
        out = ref.step(_actions(rng, cfg, kin, ref.get_state()))
        rew.append(out[1]); info.append(out[4]); ev.append(out[3]); done.append(out[2])
    return np.stack(rew), np.stack(info), np.stack(ev), np.stack(done), ref.get_state()


def _differing_rows(a, b):
    """Rows (step, env) in which two stacked outputs differ in any column (NaN equals NaN)."""
    a, b = a.reshape(a.shape[0], a.shape[1], -1), b.reshape(b.shape[0], b.shape[1], -1)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=2).sum())


def _live_counts(oracle, case):
    rew, info, ev, done, st = _oracle_run(oracle, _case_cfg(case), case["kin"])
    rew0, info0, _, _, _ = _oracle_run(oracle, _case_cfg(case, twin=True), case["kin"])
    assert np.isfinite(rew).all()
    return {"reward": _differing_rows(rew, rew0), "info": _differing_rows(info, info0),
            "timeout": int((ev == abi.EV_TIMEOUT).sum()), "done": int(done.sum())}, done, st


@pytest.mark.parametrize("name", sorted(CASES))
def test_config_case_is_live(oracle, name):
    """CPU: the varied setting changes what the oracle computes. Rows of the 3,840 whose reward / info row differs
    from the twin's run (same actions), Timeout rows and episodes ended, against half of the count measured on
    the oracle (CASES[name]["live"] holds the measured counts). A column left out of a case's `live` does not
    depend on its fields: the reward constants and the norm-zone side / penalty leave the info row alone, the
    social thresholds leave the reward alone."""
    case = CASES[name]
    got, done, st = _live_counts(oracle, case)
    for what, measured in case["live"].items():
        assert measured > 0 and got[what] >= measured // 2, "%s: %s rows = %d, measured %d" % (
            name, what, got[what], measured)
    if "done" in case["live"]:
        # crowd_sim_dict.py:162-164 in closed form: one reset() and one auto-reset per episode ended, each adding
        # nenv modulo the phase's case size (every env wraps: nenv is larger than the size)
        cfg = _case_cfg(case)
        size = cfg.val_size if cfg.phase == abi.PHASES["val"] else cfg.test_size
        assert cfg.nenv > size
        np.testing.assert_array_equal(np.asarray(st.case_counter), (1 + done.sum(axis=0)) * cfg.nenv % size)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_vs_oracle_config_space(gpu, oracle, name):
    """Teacher-forced GPU vs oracle at the setting of CASES[name], with _teacher_forced's own assertions. The
    oracle's outputs there are those of _oracle_run, the run test_config_case_is_live counts."""
    case = CASES[name]
    info, ev = _teacher_forced(gpu, oracle, _case_cfg(case), case["kin"], steps=STEPS)
    _, info2, ev2, _, _ = _oracle_run(oracle, _case_cfg(case), case["kin"])
    assert np.array_equal(ev, ev2) and np.array_equal(info, info2, equal_nan=True)


# ---- bounded rejection: wave_reject2 / wave_reject_discs / goal_reject_crowded at small max_tries ----
def _shape_cfg(shape, max_tries, rng, **over):
    if rng != "mt19937":
        over["env__rng"] = rng
    if shape == "c3":
        cfg = _cfg(25, "holonomic", SQ, E=E, fov=1.0, **over)
    elif shape == "c2":
        cfg = _cfg(10, "unicycle", E=E, **over)
    elif shape == "crowded":
        cfg = _cfg(20, "holonomic", E=E, sim__circle_radius=2.5, **over)
    else:
        cfg = _cfg(12, "holonomic", SQ, E=E, sim__square_width=12, **over)
    cfg.max_tries = max_tries
    return cfg, ("unicycle" if shape == "c2" else "holonomic")


# (shape, max_tries, rng): {1, 3} on the three shapes, both streams at 3; 64 and 65 (one whole 64-try block of a
# wave, and one try into the next) where the default geometries overflow too rarely: square_width 12, N = 12
# (c2 never overflows there); c3 and crowded still overflow in every env at 64 / 65, so they run too.
# Value: envs of the 64 whose overflow counter is non-zero at the end of the oracle's run and, in brackets, the
# overflows counted, measured on the oracle: (60 teacher-forced steps, 12 steps at time_limit 1).
OVF_MEASURED = {
    ("c3", 1, "mt19937"): ("64 (2095)", "64 (1195)"), ("c3", 3, "mt19937"): ("64 (1533)", "64 (1024)"),
    ("c2", 1, "mt19937"): ("64 (409)", "64 (226)"), ("c2", 3, "mt19937"): ("49 (92)", "36 (49)"),
    ("crowded", 1, "mt19937"): ("64 (914)", "64 (882)"), ("crowded", 3, "mt19937"): ("64 (714)", "64 (727)"),
    ("c3", 3, "philox"): ("64 (1576)", "64 (991)"), ("c2", 3, "philox"): ("47 (78)", "36 (49)"),
    ("crowded", 3, "philox"): ("64 (764)", "64 (737)"),
    ("sq12", 64, "mt19937"): ("64 (577)", "64 (278)"), ("sq12", 65, "mt19937"): ("64 (524)", "64 (276)"),
    ("sq12", 65, "philox"): ("63 (504)", "64 (274)"),
    ("c3", 64, "mt19937"): ("64 (988)", "64 (584)"), ("c3", 65, "mt19937"): ("64 (1006)", "64 (567)"),
    ("crowded", 64, "mt19937"): ("64 (478)", "64 (421)"), ("crowded", 65, "mt19937"): ("64 (452)", "64 (414)"),
}
TRIES = sorted(OVF_MEASURED)


def _ovf_envs(st):
    return int((np.asarray(st.overflow) > 0).sum())


@pytest.mark.parametrize("shape,max_tries,rng", TRIES)
def test_small_max_tries_overflows_on_the_oracle(oracle, shape, max_tries, rng):
    """CPU: the condition of the GPU tests below. The oracle gives up (overflow counter non-zero) in at least
    half of the 64 envs, in the 60-step run and in the 12-step run where every env resets at every step; all
    outputs finite. OVF_MEASURED quotes the counts measured: 64 of 64 envs everywhere but the C2 shape at
    max_tries 3 (49 / 36 envs, MT19937; 47 / 36, Philox) and 63 in one Philox run. The crowded shape at
    max_tries 3 also ends 784 of its 3,840 rows in Collision (spawns accepted on top of each other), which
    drives the step kernel's overlapping-pair ORCA branch."""
    cfg, kin = _shape_cfg(shape, max_tries, rng)
    rew, info, _, _, st = _oracle_run(oracle, cfg, kin)
    assert np.isfinite(rew).all() and np.isfinite(info[:, :, abi.INFO_DIST_TO_GOAL]).all()
    assert _ovf_envs(st) >= E // 2, (_ovf_envs(st), OVF_MEASURED[shape, max_tries, rng][0])
    cfg, kin = _shape_cfg(shape, max_tries, rng, env__time_limit=1)
    rew, info, _, done, st = _oracle_run(oracle, cfg, kin, steps=12, seed=23)
    assert np.isfinite(rew).all() and done.all()
    assert _ovf_envs(st) >= E // 2, (_ovf_envs(st), OVF_MEASURED[shape, max_tries, rng][1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,max_tries,rng", TRIES)
def test_gpu_small_max_tries_teacher_forced(gpu, oracle, shape, max_tries, rng):
    """Teacher-forced, 60 steps: goal changes and auto-resets whose rejection loops stop at try max_tries,
    accept the last try and count an overflow; the stream must stand where the oracle's stands (state
    comparison: mt_pos, stream CRC, overflow every step)."""
    cfg, kin = _shape_cfg(shape, max_tries, rng)
    info, _ = _teacher_forced(gpu, oracle, cfg, kin, steps=STEPS)
    assert np.isfinite(info[:, :, abi.INFO_OVERFLOW]).all()


def _every_env_resets(gpu, oracle, cfg, kin, budget):
    """Free-running from reset() at time_limit = 1, 12 steps: done / event and CN_INFO_OVERFLOW exact every step,
    rewards 1e-5; at the end the state within 1e-5 and overflow, mt_pos, case_counter, reset_count and the
    stream CRC exact."""
    ref, g = oracle.RefEngine(cfg), gpu(cfg)
    if budget is not None:
        g.eng.set_spawn_budget(budget)
    ref.reset()
    g.reset()
    rs = np.random.RandomState(23)
    for t in range(12):
        a = _actions(rs, cfg, kin)
        r1, r2 = ref.step(a), g.step(a)
        assert r1[2].all(), "time_limit = 1: every env ends its episode at every step (t=%d)" % t
        np.testing.assert_array_equal(r2[2], r1[2], err_msg="done t=%d" % t)
        np.testing.assert_array_equal(r2[3], r1[3], err_msg="event t=%d" % t)
        np.testing.assert_array_equal(r2[4][:, abi.INFO_OVERFLOW], r1[4][:, abi.INFO_OVERFLOW],
                                      err_msg="CN_INFO_OVERFLOW t=%d" % t)
        np.testing.assert_allclose(r2[1], r1[1], atol=1e-5, rtol=0, err_msg="reward t=%d" % t)
    st, gs = ref.get_state(), g.get_state()
    for n in ("overflow", "mt_pos", "case_counter", "reset_count"):
        np.testing.assert_array_equal(np.asarray(getattr(gs, n)), np.asarray(getattr(st, n)), err_msg=n)
    np.testing.assert_array_equal(H.mt_crc(gs), H.mt_crc(st), err_msg="stream CRC")
    d = {"post_" + n: np.asarray(getattr(st, n)) for n, _, _ in abi.STATE_FIELDS if n != "mt"}
    errs = H.compare_state(gs, d, "post_", tol=1e-5)
    assert not errs, errs[:20]
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [None, 1])
@pytest.mark.parametrize("shape,max_tries,rng", TRIES)
def test_gpu_small_max_tries_every_env_resets(gpu, oracle, shape, max_tries, rng, budget):
    """Every env resets at every step, so physics cannot accumulate (the pattern of
    test_gpu_every_env_resets_every_launch), at the default spawn budget and at a 1-cycle budget (spawns parked
    after every human and resumed): the spawns drawn ahead by the spare waves give up at try max_tries exactly
    where the oracle's sequential loop does (_every_env_resets)."""
    cfg, kin = _shape_cfg(shape, max_tries, rng, env__time_limit=1)
    _every_env_resets(gpu, oracle, cfg, kin, budget)


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [None, 1])
@pytest.mark.parametrize("name", ["test_wrap", "phase_val9", "phase_test11_offset", "philox_test_wrap"])
def test_gpu_case_counter_wraps_in_spawns_drawn_ahead(gpu, oracle, name, budget):
    """The phases with a small case size, free-running with every env resetting at every step: the episode after
    next is keyed from (case_counter + nenv) % case_size by the waves that draw spawns ahead, which teacher
    forcing never consumes (set_state discards them). 12 resets per env wrap the counter 12 times (nenv is larger
    than the case size); its closed form is asserted on the oracle's final state."""
    case = CASES[name]
    over = dict(case["base"], **case["over"])
    over["env__time_limit"] = 1
    cfg = _cfg(case["N"], case["kin"], case["scen"], case["policy"], E, case["fov"], **over)
    st = _every_env_resets(gpu, oracle, cfg, case["kin"], budget)
    size = cfg.val_size if cfg.phase == abi.PHASES["val"] else cfg.test_size
    np.testing.assert_array_equal(np.asarray(st.case_counter), np.full(E, 13 * cfg.nenv % size))
