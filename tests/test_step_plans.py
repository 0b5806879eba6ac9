"""The step kernel at every plan: cn_step_plan(N, robot.visible) derives the whole layout of cn_step_kernel from
the human count N (1..31) and robot.visible -- envs per workgroup (EPB = min(64 // N, 16)), simulator size
(A = N + visible), quad or KdTree neighbour path (A > 10), the LDS carving (the kd path's NH = EPB * N, the
o_hvr / o_hst overlay, rng_waves, rng_stride) and, through the host, the spawn grid. The rest of the suite pins
the step to the CPU oracle at 13 of these 62 plans; this file does it at all of them, with one rule for the other
settings and one batch size.

The rule (so that every plan meets both integrators, both scenarios' spawns and both belief paths): unicycle for
odd N, holonomic for even N; circle_crossing for N <= 20, square_crossing above; robot and human FOV pi when
N % 3 == 0, else 2 pi. E = 37 everywhere: a prime above 2 x 16, so every EPB value leaves a partial last workgroup
behind at least two full ones.

Every comparison is an existing one, imported unchanged with its bars: _teacher_forced and _free_run_exact of
tests/test_gpu_parity.py against the oracle (oracle/cpu_ref.c: scalar C with no N-dependent layout), _run / _same
of tests/test_seq_carry.py for the multi-step launches, and the checks of tests/test_rollout.py and
tests/test_robot_act.py at the human counts they leave out. No case can pass vacuously: the oracle's own runs
(actions do not depend on the GPU, so they are computed once on the CPU and shared) must reset every env several
times, lose sight of humans where the FOV is pi, and meet Danger / Collision rows where the crowd is dense enough;
the CPU test asserts that for every case, the GPU tests again on the run they compared with."""
import numpy as np
import pytest

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, clone_config
from tests import helpers as H
from tests import test_robot_act as RA
from tests import test_rollout as RO
from tests import test_seq_carry as SC
from tests.test_gpu_parity import _actions, _cfg, _free_run_exact, _teacher_forced

E = 37
PLANS = [(N, vis) for N in range(1, 32) for vis in (False, True)]
TF_STEPS, TF_LIMIT = 48, 6          # teacher-forced: 48 steps at time_limit 6
FREE_STEPS, FREE_LIMIT = 40, 2      # free-running: 40 steps at time_limit 2
# Free-running seed of a plan (RandomState of _free_run_exact). A plan gets another seed only where a threshold
# event flipped between two states that agree within 1e-5 (the margin, taken from the oracle's pre-step state,
# goes into the comment of the entry); none has needed it.
FREE_SEED = {}
TERMINAL = (abi.EV_COLLISION, abi.EV_REACHGOAL, abi.EV_TIMEOUT)


def _epb(N):
    return min(64 // N, 16)


def _rule(N):
    return ("unicycle" if N % 2 else "holonomic", "circle_crossing" if N <= 20 else "square_crossing",
            1.0 if N % 3 == 0 else 2.0)


def _plan_cfg(N, vis, time_limit):
    kin, scen, fov = _rule(N)
    return _cfg(N, kin, scen, "orca", E, fov, robot__visible=vis, env__time_limit=time_limit), kin


def _ids(plans):
    return ["N%d%s" % (N, "_visible" if vis else "") for N, vis in plans]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from crowdnav_dsrnn_amd.engine import NumpyEngine

    return NumpyEngine


def _belief_off(sv):
    """Humans of a state whose belief is not their position (the robot does not see them)."""
    return int(((np.asarray(sv.b_px) != np.asarray(sv.h_px)) | (np.asarray(sv.b_py) != np.asarray(sv.h_py))).sum())


# ---- the oracle's side of both comparisons, once per plan ----
_ORACLE = {}


def _tf_recipe(kin):
    return {"bias": 0.05} if kin == "unicycle" else {}


def _oracle_teacher_forced(oracle, N, vis):
    """The oracle's side of _teacher_forced (the GPU follows the oracle there, so this free run is the oracle's
    trajectory): stacked info, event, done, and the humans with belief != position over the post-step states."""
    key = ("tf", N, vis)
    if key not in _ORACLE:
        cfg, kin = _plan_cfg(N, vis, TF_LIMIT)
        ref = oracle.RefEngine(cfg)
        ref.reset()
        rng = np.random.RandomState(5)
        info, ev, done, off = [], [], [], 0
        for t in range(TF_STEPS):
            out = ref.step(_actions(rng, cfg, kin, ref.get_state(), **_tf_recipe(kin)))
            info.append(out[4]); ev.append(out[3]); done.append(out[2])
            off += _belief_off(ref.get_state())
        _ORACLE[key] = dict(info=np.stack(info), event=np.stack(ev), done=np.stack(done), belief_off=off)
    return _ORACLE[key]


def _oracle_free(oracle, N, vis):
    """The oracle's side of _free_run_exact (same RandomState, same recipe): done [T][E], the humans with belief !=
    position over the post-step states and the final reset counts."""
    key = ("free", N, vis)
    if key not in _ORACLE:
        cfg, kin = _plan_cfg(N, vis, FREE_LIMIT)
        ref = oracle.RefEngine(cfg)
        ref.reset()
        rng = np.random.RandomState(FREE_SEED.get((N, vis), 11))
        done, off = [], 0
        for t in range(FREE_STEPS):
            a = (rng.uniform(-0.1, 0.1, (E, 2)) if kin == "unicycle" else rng.normal(0, 0.5, (E, 2))).astype(np.float32)
            done.append(ref.step(a)[2])
            off += _belief_off(ref.get_state())
        _ORACLE[key] = dict(done=np.stack(done), belief_off=off,
                            reset_count=np.asarray(ref.get_state().reset_count).copy())
    return _ORACLE[key]


def _teacher_forced_premises(N, vis, run):
    """Measured on the oracle over the 62 plans: at least 2 resets per env; FOV pi: belief != position in 0.44 to
    0.50 of the human-steps (floor 0.30); holonomic, N >= 4, robot not visible: at least 46 Danger + Collision rows
    of the 1,776 (floor 20). Low-N, unicycle and visible-robot plans have few or none, so no floor there."""
    kin, _, fov = _rule(N)
    resets = run["done"].sum(axis=0)
    assert resets.min() >= 2, resets
    assert np.array_equal(run["done"], np.isin(run["event"], TERMINAL))
    if fov == 1.0:
        frac = run["belief_off"] / float(TF_STEPS * E * N)
        assert frac >= 0.30, frac
    if kin == "holonomic" and N >= 4 and not vis:
        rows = int(np.isin(run["event"], (abi.EV_DANGER, abi.EV_COLLISION)).sum())
        assert rows >= 20, rows


def _free_premises(N, vis, run):
    """Measured on the oracle: at least 4 resets per env within the first 24 steps (time_limit 2), every one an
    auto-reset that takes a spawn drawn ahead or parked; FOV pi: belief != position as above."""
    resets = run["done"][:24].sum(axis=0)
    assert resets.min() >= 4, resets
    np.testing.assert_array_equal(run["reset_count"], 1 + run["done"].sum(axis=0))
    if _rule(N)[2] == 1.0:
        frac = run["belief_off"] / float(FREE_STEPS * E * N)
        assert frac >= 0.30, frac


# ---- 1. CPU ----
def test_table_holds_every_plan_and_leaves_a_partial_workgroup():
    assert len(PLANS) == len(set(PLANS)) == 62
    assert {N for N, _ in PLANS} == set(range(1, 32)) and {v for _, v in PLANS} == {False, True}
    assert sorted({_epb(N) for N, _ in PLANS}) == [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16]
    for N, vis in PLANS:
        assert E % _epb(N) != 0 and E // _epb(N) >= 2, N
        kin, scen, fov = _rule(N)
        cfg, _ = _plan_cfg(N, vis, TF_LIMIT)
        assert (cfg.num_envs, cfg.human_num, bool(cfg.robot_visible)) == (E, N, vis)
    # both values of every rule meet both neighbour paths (A > 10: the KdTree), with and without the robot
    for kd in (False, True):
        for vis in (False, True):
            rules = [_rule(N) for N, v in PLANS if v == vis and (N + vis > 10) == kd]
            assert {r[0] for r in rules} == {"unicycle", "holonomic"} and {r[2] for r in rules} == {1.0, 2.0}, (kd, vis)


@pytest.mark.parametrize("N,vis", PLANS, ids=_ids(PLANS))
def test_oracle_meets_the_premises(oracle, N, vis):
    """CPU: the oracle alone, at the table's settings and recipes, meets what the GPU cases rely on."""
    _teacher_forced_premises(N, vis, _oracle_teacher_forced(oracle, N, vis))
    _free_premises(N, vis, _oracle_free(oracle, N, vis))


# ---- 2. teacher-forced ----
@pytest.mark.gpu
@pytest.mark.parametrize("N,vis", PLANS, ids=_ids(PLANS))
def test_gpu_teacher_forced_every_plan(gpu, oracle, N, vis):
    """_teacher_forced with its own bars (events, done and flags exact; 1e-5 on state, reward and observations; the
    whole info row and the Monitor pair), 48 steps from the oracle's state at time_limit 6."""
    cfg, kin = _plan_cfg(N, vis, TF_LIMIT)
    info, ev = _teacher_forced(gpu, oracle, cfg, kin, steps=TF_STEPS, **_tf_recipe(kin))
    run = _oracle_teacher_forced(oracle, N, vis)
    assert np.array_equal(ev, run["event"]) and np.array_equal(info, run["info"], equal_nan=True)
    _teacher_forced_premises(N, vis, run)


# ---- 3. free-running ----
@pytest.mark.gpu
@pytest.mark.parametrize("N,vis", PLANS, ids=_ids(PLANS))
def test_gpu_free_running_every_plan(gpu, oracle, N, vis):
    """What teacher forcing cannot reach: every auto-reset takes the spawn that the spare workgroups of an earlier
    launch drew, or one that was parked (pend_waves, pend_blocks and rng_stride all follow the plan). The reset
    observations, then _free_run_exact for 40 steps at time_limit 2, then the whole state within 1e-5 with every
    MT19937 stream where the oracle's stands."""
    cfg, kin = _plan_cfg(N, vis, FREE_LIMIT)
    ref, g = oracle.RefEngine(cfg), gpu(cfg)
    o1, o2 = ref.reset(), g.reset()
    for k in o1:
        np.testing.assert_allclose(o2[k], o1[k], atol=1e-6, rtol=0, err_msg=k)
    _free_run_exact(ref, g, cfg, FREE_STEPS, kin, FREE_SEED.get((N, vis), 11))
    rs, gs = ref.get_state(), g.get_state()
    d = {"post_" + n: np.asarray(getattr(rs, n)) for n, _, _ in abi.STATE_FIELDS if n != "mt"}
    d["post_mt_crc"] = H.mt_crc(rs)
    errs = H.compare_state(gs, d, "post_", tol=1e-5)
    assert not errs, errs
    run = _oracle_free(oracle, N, vis)
    np.testing.assert_array_equal(np.asarray(rs.reset_count), run["reset_count"])
    _free_premises(N, vis, run)


# ---- 4. multi-step launches ----
QUAD_PLANS = [(N, False) for N in range(1, 11)] + [(N, True) for N in range(1, 10)]
KD_SEQ_PLANS = [(10, True), (31, True)]


def _seq_case(N, vis, rng=None):
    kin, scen, fov = _rule(N)
    base = clone_config(Config())
    base.robot.visible = vis
    if rng is not None:
        base.env.rng = rng
    return SC._cfg(N, kin, E, fov=fov, time_limit=2, base=base, sims=[scen]), kin


def _seq_check(N, vis, chunks, rng=None):
    """step_seq over T = 37 steps at each chunk length against chunk 1: the nine outputs and the state blob, bit
    for bit; every env resets inside launches, and at FOV pi the carried belief is not the position."""
    T = 37
    cfg, kin = _seq_case(N, vis, rng)
    assert cfg.robot_visible == vis and cfg.human_num == N
    acts = SC._actions(T, E, kin, 100 + N)
    ref, sv = SC._run(cfg, acts, [("seq", 0, T)], chunk=1)
    rc = np.asarray(sv.reset_count).astype(np.int64) - 1
    assert (rc >= (1 + T) // 5).all(), rc
    for chunk in chunks:
        got, _ = SC._run(cfg, acts, [("seq", 0, T)], chunk=chunk)
        SC._same(got, ref, "N=%d visible=%s chunk %d" % (N, vis, chunk))
    return sv


@pytest.mark.gpu
@pytest.mark.parametrize("N,vis", QUAD_PLANS, ids=_ids(QUAD_PLANS))
def test_gpu_multi_step_launches_every_quad_plan(N, vis):
    """The SEQ kernels exist for the quad path (A <= 10): chunks 2, 8 and 32."""
    _seq_check(N, vis, (2, 8, 32))


@pytest.mark.gpu
@pytest.mark.parametrize("N,vis", KD_SEQ_PLANS, ids=_ids(KD_SEQ_PLANS))
def test_gpu_step_seq_falls_back_to_single_steps_on_kd_plans(N, vis):
    """A > 10: the host runs single steps whatever the chunk, so chunk 32 must give chunk 1's bytes."""
    _seq_check(N, vis, (32,))


# ---- 5. scripted rollouts and cn_robot_act ----
ROLLOUT_CASES = [(name, N) for N in (2, 3, 4, 6, 7, 8) for name in RO.NAMES] + [("social_force", 10)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", ROLLOUT_CASES)
def test_gpu_fused_rollout_equals_pairs_other_counts(name, N):
    """test_gpu_fused_rollout_equals_pairs itself (E = 13, T = 37, time_limit 2, MT19937, default chunk: the fused
    launch count, rows and state blob byte for byte, resets inside launches) at the human counts it leaves out:
    16 (N = 2, 3, 4), 10, 9 and 8 envs per workgroup, N = 8 with all 64 human lanes, and N = 10 (6 envs per
    workgroup), which only the social-force controller runs fused."""
    RO.test_gpu_fused_rollout_equals_pairs(name, "mt19937", N, None)


ROBOT_ACT_N = [N for N in range(1, 32) if N not in (1, 5, 9, 10, 31)]


@pytest.mark.gpu
@pytest.mark.parametrize("envs", [E, 1])
@pytest.mark.parametrize("N", ROBOT_ACT_N)
def test_gpu_robot_act_equals_host_composition_other_counts(N, envs):
    """test_gpu_robot_act_equals_host_composition_bit_for_bit itself (its E = 37 and E = 1) at every human count it
    leaves out: with its own 1, 5, 9, 10 and 31 that is every N of 1..31."""
    RA.test_gpu_robot_act_equals_host_composition_bit_for_bit(N, envs)
