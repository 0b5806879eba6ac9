"""Every instantiation of cn_step_kernel at every step plan it can serve.

cn_step_kernel is one template; `step_kernels[]` in csrc/engine/host_engine.h lists its instantiations, keyed
{kd, phx, mix} x {SINGLE, DEVSEQ, SEQ, ROBOT, ROBOT_REC, ROBOT_MASK}, and each runs under whichever of the 62 step
plans cn_step_plan(N, robot.visible) selects. tests/test_step_plans.py pins three of them (single-step MT19937, quad
and kd; multi-step MT19937) at every plan; this file does the same for the others. MATRIX below is the table: one
entry per instantiation with the tests that run it and the plans it serves, and a CPU test holds it against the
header, so that a new template flag or table entry fails until it gets its rows.

Two parts compare with the oracle (oracle/cpu_ref.c: scalar C with no N-dependent layout): A, the Philox single-step
kernels on plain engines, and B, the four single-step kernels of mixed engines against oracle.RefMixedEngine with
every human count in one engine. The others compare bit for bit with a kernel that A, B or tests/test_step_plans.py
has pinned: C graph mode (replay equals eager), D the multi-step Philox kernel (chunks 2, 8, 32 against chunk 1), E
the scripted rollouts (fused equals the eager loop and chunk 1) and F the mixed-group multi-step and rollout kernels
(chunk 32 against chunk 1; rows against plain one-env engines). No tolerance is new: every bar is that of the
imported check. The premises that keep a case from passing vacuously are asserted on the CPU for A and B (the
oracle's own runs) and on the reference run for the others."""
import os
import re
import types

import numpy as np
import pytest

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config, make_varied_cn_configs
from tests import helpers as H
from tests import test_rollout as RO
from tests import test_rollout_lidar as RL
from tests import test_rollout_mask as RM
from tests import test_seq_carry as SC
from tests import test_step_plans as SP
from tests.test_gpu_parity import _actions, _cfg, _free_run_exact
from tests.test_step_plans import (E, FREE_LIMIT, FREE_STEPS, PLANS, QUAD_PLANS, _belief_off, _free_premises, _ids,
                                   _rule)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "crowdnav_dsrnn_amd", "csrc", "engine", "host_engine.h")
DEV = "cuda:0"
RNGS = ("mt19937", "philox")
MODES = ("SINGLE", "DEVSEQ", "SEQ", "ROBOT", "ROBOT_REC", "ROBOT_MASK")
KD_PLANS = [p for p in PLANS if p not in QUAD_PLANS]


# ---- 0. the table ----
def _served(kd, phx, mix, mode):
    """The plans an instantiation serves, or None where the combination does not exist: kd is A = N + visible > 10;
    the multi-step and rollout kernels exist for the quad path only; graph mode and the recording rollout for plain
    engines only."""
    if (kd and mode not in ("SINGLE", "DEVSEQ")) or (mix and mode in ("DEVSEQ", "ROBOT_REC")):
        return None
    return list(KD_PLANS if kd else QUAD_PLANS)


# mode -> mix -> the tests that run those instantiations (both RNGs, quad and kd alike unless told otherwise)
_TESTS = {
    ("SINGLE", False): {False: ("tests/test_step_plans.py::test_gpu_teacher_forced_every_plan",
                                "tests/test_step_plans.py::test_gpu_free_running_every_plan"),
                        True: ("test_gpu_philox_free_running_every_plan",)},
    ("SINGLE", True): ("test_gpu_mixed_teacher_forced_every_count", "test_gpu_mixed_free_running_every_count"),
    ("DEVSEQ", False): ("test_gpu_graph_replay_equals_eager_every_plan",),
    ("SEQ", False): {False: ("tests/test_step_plans.py::test_gpu_multi_step_launches_every_quad_plan",),
                     True: ("test_gpu_multi_step_philox_every_quad_plan",)},
    ("SEQ", True): ("test_gpu_mixed_step_seq_chunk_32_equals_chunk_1",),
    ("ROBOT", False): {False: ("tests/test_step_plans.py::test_gpu_fused_rollout_equals_pairs_other_counts",
                               "tests/test_rollout.py::test_gpu_fused_rollout_equals_pairs",
                               "test_gpu_fused_rollout_visible_quad_plans"),
                       True: ("tests/test_rollout.py::test_gpu_fused_rollout_equals_pairs",
                              "test_gpu_fused_rollout_philox_other_counts",
                              "test_gpu_fused_rollout_visible_quad_plans")},
    ("ROBOT", True): ("test_gpu_mixed_rollout_rows_equal_plain_engines",),
    ("ROBOT_REC", False): ("test_gpu_lidar_rollout_every_count",),
    ("ROBOT_MASK", False): ("test_gpu_masked_rollout_every_count",),
    ("ROBOT_MASK", True): ("test_gpu_mixed_rollout_rows_equal_plain_engines",),
}


def _build_matrix():
    m = {}
    for mode in MODES:
        for mix in (False, True):
            for phx in (False, True):
                for kd in (False, True):
                    plans = _served(kd, phx, mix, mode)
                    if plans is None:
                        continue
                    tests = _TESTS[(mode, mix)]
                    m[(kd, phx, mix, mode)] = dict(tests=tests[phx] if isinstance(tests, dict) else tests, plans=plans)
    return m


MATRIX = _build_matrix()


def _table_entries(path=HEADER):
    """Every STEP_KERNEL(<bool>, <bool>, <bool>, STEP_<MODE>) inside the step_kernels[] initialiser (not the
    #define), in the header's order."""
    txt = open(path).read()
    m = re.search(r"step_kernels\[\]\s*=\s*\{(.*?)\};", txt, re.S)
    assert m, "no step_kernels[] initialiser in %s" % path
    body = re.sub(r"//[^\n]*|/\*.*?\*/", "", m.group(1), flags=re.S)
    found = re.findall(r"STEP_KERNEL\(\s*(true|false)\s*,\s*(true|false)\s*,\s*(true|false)\s*,\s*STEP_(\w+)\s*\)", body)
    assert len(found) == body.count("STEP_KERNEL"), "an entry of step_kernels[] was not understood"
    return [(a == "true", b == "true", c == "true", mode) for a, b, c, mode in found]


def _check_table(path=HEADER):
    entries = _table_entries(path)
    assert len(entries) == len(set(entries)), sorted(e for e in entries if entries.count(e) > 1)
    extra, missing = set(entries) - set(MATRIX), set(MATRIX) - set(entries)
    assert not extra and not missing, "step_kernels[] and MATRIX differ: not in MATRIX %s, not in the header %s" % (
        sorted(extra), sorted(missing))
    return entries


def test_matrix_holds_every_instantiation_of_the_kernel_table():
    entries = _check_table()
    assert len(entries) == 26
    here = globals()
    for key, row in MATRIX.items():
        assert row["tests"], key
        for name in row["tests"]:
            if "::" in name:
                path, fn = name.split("::")
                assert re.search(r"^def %s\(" % fn, open(os.path.join(REPO, path)).read(), re.M), name
            else:
                assert callable(here.get(name)), (key, name)
        assert row["plans"] == _served(*key) and row["plans"], key
        assert all((N + vis > 10) == key[0] for N, vis in row["plans"]), key
    # the plans of the kd and quad instantiations of one (phx, mix, mode) are disjoint, and together all 62 where both exist
    for (kd, phx, mix, mode), row in MATRIX.items():
        if kd:
            assert sorted(row["plans"] + MATRIX[(False, phx, mix, mode)]["plans"]) == sorted(PLANS)
    assert len(QUAD_PLANS) == 19 and len(KD_PLANS) == 43


def test_a_new_table_entry_fails_until_it_has_its_rows(tmp_path):
    """A 27th STEP_KERNEL line in a copy of the header, and a duplicate of an existing one."""
    txt = open(HEADER).read()
    last = "STEP_KERNEL(false, true, true, STEP_ROBOT_MASK)}"
    assert txt.count(last) == 1
    for extra in ("STEP_KERNEL(true, false, false, STEP_SEQ)", "STEP_KERNEL(false, false, false, STEP_SEQ)"):
        p = tmp_path / "host_engine.h"
        p.write_text(txt.replace(last, last[:-1] + ",\n    " + extra + "}"))
        assert len(_table_entries(str(p))) == 27
        with pytest.raises(AssertionError):
            _check_table(str(p))


# ---- shared ----
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from crowdnav_dsrnn_amd.engine import NumpyEngine

    return NumpyEngine


def _plan_cfg(N, vis, time_limit, rng):
    """tests/test_step_plans.py's _plan_cfg (its rule, E = 37) with the RNG chosen."""
    kin, scen, fov = _rule(N)
    return _cfg(N, kin, scen, "orca", E, fov, robot__visible=vis, env__time_limit=time_limit, env__rng=rng), kin


def _end_state_errs(rs, gs):
    d = {"post_" + n: np.asarray(getattr(rs, n)) for n, _, _ in abi.STATE_FIELDS if n != "mt"}
    d["post_mt_crc"] = H.mt_crc(rs)
    return H.compare_state(gs, d, "post_", tol=1e-5)


_ORACLE = {}


# ---- A. Philox single-step kernels vs the oracle's Philox, all 62 plans ----
# Free-running seed of a plan, by the rule of FREE_SEED in tests/test_step_plans.py (another seed only for a threshold
# flip between two states that agree within 1e-5, the oracle's margin in the comment); none has needed it.
PHILOX_FREE_SEED = {}


def _oracle_philox_free(oracle, N, vis):
    """tests/test_step_plans.py's _oracle_free under Philox."""
    key = ("A", N, vis)
    if key not in _ORACLE:
        cfg, kin = _plan_cfg(N, vis, FREE_LIMIT, "philox")
        ref = oracle.RefEngine(cfg)
        ref.reset()
        rng = np.random.RandomState(PHILOX_FREE_SEED.get((N, vis), 11))
        done, off = [], 0
        for t in range(FREE_STEPS):
            a = (rng.uniform(-0.1, 0.1, (E, 2)) if kin == "unicycle" else rng.normal(0, 0.5, (E, 2))).astype(np.float32)
            done.append(ref.step(a)[2])
            off += _belief_off(ref.get_state())
        _ORACLE[key] = dict(done=np.stack(done), belief_off=off,
                            reset_count=np.asarray(ref.get_state().reset_count).copy())
    return _ORACLE[key]


@pytest.mark.parametrize("N,vis", PLANS, ids=_ids(PLANS))
def test_oracle_philox_meets_the_free_running_premises(oracle, N, vis):
    """CPU: at least 4 auto-resets per env in the first 24 steps, belief != position in at least 0.30 of the
    human-steps at FOV pi (_free_premises, unchanged) on the oracle's Philox run."""
    cfg, _ = _plan_cfg(N, vis, FREE_LIMIT, "philox")
    assert cfg.rng_mode == abi.RNG_MODE["philox"]
    _free_premises(N, vis, _oracle_philox_free(oracle, N, vis))


@pytest.mark.gpu
@pytest.mark.parametrize("N,vis", PLANS, ids=_ids(PLANS))
def test_gpu_philox_free_running_every_plan(gpu, oracle, N, vis):
    """tests/test_step_plans.py's test_gpu_free_running_every_plan with env.rng = philox: the reset observations,
    _free_run_exact for 40 steps at time_limit 2, the whole state within 1e-5 with every stream position and key
    where the oracle's stands, reset_count."""
    cfg, kin = _plan_cfg(N, vis, FREE_LIMIT, "philox")
    ref, g = oracle.RefEngine(cfg), gpu(cfg)
    o1, o2 = ref.reset(), g.reset()
    for k in o1:
        np.testing.assert_allclose(o2[k], o1[k], atol=1e-6, rtol=0, err_msg=k)
    _free_run_exact(ref, g, cfg, FREE_STEPS, kin, PHILOX_FREE_SEED.get((N, vis), 11))
    rs, gs = ref.get_state(), g.get_state()
    errs = _end_state_errs(rs, gs)
    assert not errs, errs
    run = _oracle_philox_free(oracle, N, vis)
    np.testing.assert_array_equal(np.asarray(rs.reset_count), run["reset_count"])
    _free_premises(N, vis, run)
    g.eng.close()


# ---- B. mixed-group single-step kernels vs oracle.RefMixedEngine, every human count at once ----
B_NUMS = list(range(1, 32))
B_PER = 37
B_E = B_PER * len(B_NUMS)      # 1147
B_TF_STEPS, B_TF_LIMIT = 48, 6
# (kinematics, robot.visible, rng, scenario). The first four run the four SINGLE mixed kernels under every N, both
# integrators and both robot.visible values; the last two give each RNG the robot.visible value the first four do
# not, so that each of the four kernels meets each of its plans.
B_ENGINES = [("holonomic", False, "mt19937", "circle_crossing"), ("unicycle", True, "philox", "square_crossing"),
             ("holonomic", True, "philox", "circle_crossing"), ("unicycle", False, "mt19937", "square_crossing"),
             ("holonomic", True, "mt19937", "square_crossing"), ("unicycle", False, "philox", "circle_crossing")]
B_IDS = ["%s-%s-%s-%s" % (k[:3], "visible" if v else "hidden", r, s.split("_")[0]) for k, v, r, s in B_ENGINES]


def _b_cfgs(kin, vis, rng, scen, time_limit):
    c = clone_config(Config())
    c.action_space.kinematics = kin
    c.robot.visible = vis
    c.humans.policy = "orca"
    c.env.rng = rng
    c.env.time_limit = time_limit
    c.sim.train_val_sim = c.sim.test_sim = [scen]
    c.sim.human_nums = list(B_NUMS)
    c.sim.human_num = max(B_NUMS)
    return make_varied_cn_configs(c, B_NUMS, B_E, env_offset=0, nenv=B_E, phase="train", seed=5)


def _b_counts():
    return np.array([B_NUMS[r % len(B_NUMS)] for r in range(B_E)], np.int32)


def _b_tf_action(rng, kin):
    """tests/test_step_plans.py's teacher-forced recipe (_actions with bias 0.05 for the unicycle)."""
    return _actions(rng, types.SimpleNamespace(num_envs=B_E), kin, **SP._tf_recipe(kin))


def _b_free_action(rng, kin):
    return (rng.uniform(-0.1, 0.1, (B_E, 2)) if kin == "unicycle" else rng.normal(0, 0.5, (B_E, 2))).astype(np.float32)


def _oracle_mixed(oracle, case):
    """The oracle's two runs of a B engine: done [T][E] of each."""
    key = ("B",) + case
    if key not in _ORACLE:
        kin, vis, rng_mode, scen = case
        out = {}
        for what, steps, limit, seed in (("tf", B_TF_STEPS, B_TF_LIMIT, 5), ("free", FREE_STEPS, FREE_LIMIT, 11)):
            ref = oracle.RefMixedEngine(*_b_cfgs(kin, vis, rng_mode, scen, limit))
            ref.reset()
            rng = np.random.RandomState(seed)
            act = _b_tf_action if what == "tf" else _b_free_action
            out[what] = np.stack([ref.step(act(rng, kin))[2] for t in range(steps)])
        _ORACLE[key] = out
    return _ORACLE[key]


def _mixed_premises(run):
    """Every one of the 1147 envs (so every group) auto-resets at least 4 times in the first 24 free-running steps
    and at least twice teacher-forced (the floors of tests/test_step_plans.py)."""
    free, tf = run["free"][:24].sum(axis=0), run["tf"].sum(axis=0)
    assert free.shape == (B_E,) and free.min() >= 4, free
    assert tf.min() >= 2, tf


@pytest.mark.parametrize("case", B_ENGINES, ids=B_IDS)
def test_oracle_mixed_meets_the_premises(oracle, case):
    cfgs, eg = _b_cfgs(*case, FREE_LIMIT)
    assert [int(c.human_num) for c in cfgs] == B_NUMS and all(int(c.num_envs) == B_PER for c in cfgs)
    assert np.array_equal(np.asarray(B_NUMS)[eg], _b_counts())
    assert all(bool(c.robot_visible) == case[1] and c.rng_mode == abi.RNG_MODE[case[2]] for c in cfgs)
    _mixed_premises(_oracle_mixed(oracle, case))


class _MixedNumpy:
    """The oracle's interface over a mixed CrowdNavEngine (what NumpyEngine is for a plain one)."""

    def __init__(self, cfgs, eg):
        import torch

        from crowdnav_dsrnn_amd.engine import CrowdNavEngine

        self.torch = torch
        self.eng = CrowdNavEngine.mixed(cfgs, eg, DEV)

    def reset(self):
        o = self.eng.reset()
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    def step(self, actions):
        a = self.torch.from_numpy(np.ascontiguousarray(actions, np.float32).reshape(self.eng.E, 2)).to(DEV)
        obs, *rest = self.eng.step(a)
        self.torch.cuda.synchronize()
        return ({k: v.cpu().numpy() for k, v in obs.items()},) + tuple(x.cpu().numpy() for x in rest)

    def get_state(self):
        return self.eng.get_state()

    def set_state(self, svs):
        self.eng.set_state(svs)


def _group_errs(ref, g, where=""):
    errs = []
    for (rows, rs), (grows, gs) in zip(ref.get_state(), g.get_state()):
        assert np.array_equal(rows, grows)
        d = {"post_" + n: np.asarray(getattr(rs, n)) for n, _, _ in abi.STATE_FIELDS if n != "mt"}
        d["post_mt_crc"] = H.mt_crc(rs)
        errs += H.compare_state(gs, d, "post_", tol=1e-5, where="%sN=%d " % (where, rs.N))
    return errs


@pytest.mark.gpu
@pytest.mark.parametrize("case", B_ENGINES, ids=B_IDS)
def test_gpu_mixed_teacher_forced_every_count(oracle, case):
    """48 steps at time_limit 6 from the oracle's state, at the bars of the oracle half of
    tests/test_varied_humans.py::test_varied_vec_env_vs_plain_engines_and_oracle: done and event exact; reward and
    the observations (padding slots included) within 1e-5; every group's state within 1e-5 with its streams;
    compare_info and compare_monitor."""
    kin, vis, rng_mode, scen = case
    cfgs, eg = _b_cfgs(kin, vis, rng_mode, scen, B_TF_LIMIT)
    ref, g = oracle.RefMixedEngine(cfgs, eg), _MixedNumpy(cfgs, eg)
    assert g.eng.env_humans.cpu().numpy().tolist() == _b_counts().tolist()
    ref.reset()
    rng = np.random.RandomState(5)
    done = []
    for t in range(B_TF_STEPS):
        g.set_state(ref.get_state())
        a = _b_tf_action(rng, kin)
        r_out, g_out = ref.step(a), g.step(a)
        np.testing.assert_array_equal(g_out[2], r_out[2], err_msg="done t=%d" % t)
        np.testing.assert_array_equal(g_out[3], r_out[3], err_msg="event t=%d" % t)
        np.testing.assert_allclose(g_out[1], r_out[1], atol=1e-5, rtol=0, err_msg="reward t=%d" % t)
        for k in ("robot_node", "temporal_edges", "spatial_edges"):
            np.testing.assert_allclose(g_out[0][k], r_out[0][k], atol=1e-5, rtol=0, err_msg="%s t=%d" % (k, t))
        errs = _group_errs(ref, g, "t=%d " % t)
        errs += H.compare_info(g_out[4], r_out[4], r_out[3], where="t=%d " % t)
        errs += H.compare_monitor(g_out[5], g_out[6], r_out[5], r_out[6], r_out[2], where="t=%d " % t)
        assert not errs, errs
        done.append(r_out[2])
    run = _oracle_mixed(oracle, case)
    np.testing.assert_array_equal(np.stack(done), run["tf"])
    _mixed_premises(run)
    g.eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", B_ENGINES, ids=B_IDS)
def test_gpu_mixed_free_running_every_count(oracle, case):
    """40 steps at time_limit 2 with _free_run_exact's bars on the whole engine's rows, after the reset observations;
    then every group's end state within 1e-5 with every stream where the oracle's stands, and the per-env counts."""
    kin, vis, rng_mode, scen = case
    cfgs, eg = _b_cfgs(kin, vis, rng_mode, scen, FREE_LIMIT)
    ref, g = oracle.RefMixedEngine(cfgs, eg), _MixedNumpy(cfgs, eg)
    o1, o2 = ref.reset(), g.reset()
    for k in o1:
        np.testing.assert_allclose(o2[k], o1[k], atol=1e-6, rtol=0, err_msg=k)
    whole = types.SimpleNamespace(num_envs=B_E, min_personal_space=cfgs[0].min_personal_space)
    assert all(c.min_personal_space == whole.min_personal_space for c in cfgs)
    _free_run_exact(ref, g, whole, FREE_STEPS, kin, 11)
    errs = _group_errs(ref, g)
    assert not errs, errs
    counts = np.zeros(B_E, np.int64)
    for rows, rs in ref.get_state():
        counts[rows] = rs.N
    np.testing.assert_array_equal(g.eng.env_humans.cpu().numpy(), counts)
    np.testing.assert_array_equal(counts, _b_counts())
    run = _oracle_mixed(oracle, case)
    rc = np.zeros(B_E, np.int64)
    for rows, rs in ref.get_state():
        rc[rows] = np.asarray(rs.reset_count)
    np.testing.assert_array_equal(rc, 1 + run["free"].sum(axis=0))
    _mixed_premises(run)
    g.eng.close()


# ---- C. graph-mode kernels: replay equals eager, all 62 plans x both RNGs ----
@pytest.mark.gpu
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("N,vis", PLANS, ids=_ids(PLANS))
def test_gpu_graph_replay_equals_eager_every_plan(N, vis, rng):
    """The shape of tests/test_envs.py::test_graph_mode_at_most_humans_has_its_lds at E = 37 and time_limit 2: one
    eager warm-up step, 8 eng.step launches captured as a single chain, replayed 4 times from a refilled action
    buffer, against 33 eager steps from the same reset and actions: the state blob and the last step's nine outputs
    bit for bit. On the eager run every env's reset_count rises by at least 3."""
    import torch

    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    T, R = 8, 4
    cfg, kin = _plan_cfg(N, vis, 2, rng)
    acts = SC._actions(1 + T * R, E, kin, 300 + N)
    runs = []
    for graph in (False, True):
        eng = CrowdNavEngine(cfg, DEV)
        eng.reset()
        torch.cuda.synchronize()
        rc0 = np.asarray(eng.get_state().reset_count).astype(np.int64)
        eng.step(acts[0])
        if graph:
            buf = acts[1:1 + T].clone()
            eng.set_graph_mode(True)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for t in range(T):
                    eng.step(buf[t])
            for r in range(R):
                buf.copy_(acts[1 + r * T:1 + (r + 1) * T])
                gr.replay()
            torch.cuda.synchronize()
            eng.set_graph_mode(False)
        else:
            for t in range(T * R):
                eng.step(acts[1 + t])
            torch.cuda.synchronize()
        out = {k: getattr(eng, k).cpu().numpy().copy() for k in SC.OUTPUTS}
        sv = eng.get_state()
        out["state"] = np.asarray(sv.blob).view(np.uint8).copy()
        if not graph:
            rose = np.asarray(sv.reset_count).astype(np.int64) - rc0
            assert (rose >= 3).all(), rose
        eng.close()
        runs.append(out)
    SC._same(runs[1], runs[0], "graph replay, N=%d visible=%s %s" % (N, vis, rng))


# ---- D. multi-step Philox kernel at the 19 quad plans ----
@pytest.mark.gpu
@pytest.mark.parametrize("N,vis", QUAD_PLANS, ids=_ids(QUAD_PLANS))
def test_gpu_multi_step_philox_every_quad_plan(N, vis):
    """_seq_check of tests/test_step_plans.py under Philox: T = 37, chunks 2, 8 and 32 against chunk 1 (the
    single-step kernel that part A pins to the oracle)."""
    cfg, _ = SP._seq_case(N, vis, "philox")
    assert cfg.rng_mode == abi.RNG_MODE["philox"]
    SP._seq_check(N, vis, (2, 8, 32), "philox")


# ---- E. scripted-rollout kernels at every quad plan ----
@pytest.mark.gpu
@pytest.mark.parametrize("name,N", SP.ROLLOUT_CASES)
def test_gpu_fused_rollout_philox_other_counts(name, N):
    """tests/test_rollout.py::test_gpu_fused_rollout_equals_pairs under Philox at the human counts that
    tests/test_step_plans.py runs under MT19937 only (that test asserts the fused launch count itself)."""
    RO.test_gpu_fused_rollout_equals_pairs(name, "philox", N, None)


VISIBLE_QUAD = [(name, rng, N) for N in range(1, 10) for rng in RNGS for name in RO.NAMES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,rng,N", VISIBLE_QUAD)
def test_gpu_fused_rollout_visible_quad_plans(name, rng, N):
    """The same at the robot.visible quad plans (N = 1..9: the step's simulators hold N + 1 <= 10 agents, and so
    does the robot's own ORCA, so every case runs fused, which the test asserts through num_launches)."""
    RO.test_gpu_fused_rollout_equals_pairs(name, rng, N, None, visible=True)


# N = 10: ORCA has N + 1 = 11 agents and runs as launch pairs (asserted by the files' own launch counts), so social
# force is what runs the recording kernels at that plan.
REC_CASES = [("orca", N) for N in range(1, 11)] + [("social_force", 10)]
LK = "b65_r11"


@pytest.mark.gpu
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("name,N", REC_CASES)
def test_gpu_lidar_rollout_every_count(name, N, rng):
    """cn_rollout_lidar at N = 1..10 under both RNGs: tests/test_rollout_lidar.py's premises on the eager reference
    run, "rows equal the eager loop" (clean and noisy) and "fused equals chunk one (and five)", at the 65-beam
    LiDAR setting."""
    RL.test_gpu_premises_hold_on_the_reference_run(name, N, 2.0, rng=rng, lks=(LK,))
    for noisy in (False, True):
        RL.test_gpu_rows_equal_the_eager_loop(name, N, 2.0, noisy, LK, rng=rng)
    RL.test_gpu_fused_equals_chunk_one_equals_chunk_five(name, N, 2.0, LK, rng=rng)


MASK_CASES = [("orca5", N) for N in range(1, 11)] + [("sf5", 10)]


@pytest.mark.gpu
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("case,N", MASK_CASES)
def test_gpu_masked_rollout_every_count(case, N, rng):
    """cn_rollout_masked at N = 1..10 under both RNGs (robot.FOV 0.5 pi): tests/test_rollout_mask.py's premises on
    the eager run, "rows equal the eager loop" (noisy and clean) and "chunks give the same rows" at chunk 1."""
    RM.test_gpu_premises_hold_on_the_eager_run(case, N=N, rng=rng)
    for noisy in (True, False):
        RM.test_gpu_rows_equal_the_eager_loop(case, noisy, N=N, rng=rng)
    RM.test_gpu_chunks_give_the_same_rows(case, 1, N=N, rng=rng)


# ---- F. mixed-group SEQ / ROBOT / ROBOT_MASK kernels ----
F_NUMS = list(range(1, 11))
F_PER, F_T, F_SEED = 13, 37, 7
F_E = F_PER * len(F_NUMS)
F_CASES = [(rng, vis) for rng in RNGS for vis in (False, True)]
F_IDS = ["%s%s" % (rng, "-visible" if vis else "") for rng, vis in F_CASES]


def _f_config(vis):
    c = clone_config(Config())
    c.action_space.kinematics = "holonomic"
    c.humans.policy = "orca"
    c.robot.visible = vis
    c.robot.FOV = 0.5
    c.env.time_limit = 2
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.sim.human_nums = list(F_NUMS)
    c.sim.human_nums_scripted = True
    return c


def _f_mixed(rng, vis, chunk=None):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    cfgs, eg = make_varied_cn_configs(_f_config(vis), F_NUMS, F_E, phase="train", seed=F_SEED, rng=rng)
    eng = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=True)
    assert eng.env_humans.tolist() == [F_NUMS[r % len(F_NUMS)] for r in range(F_E)]
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    return eng


def _f_state(eng):
    import torch

    torch.cuda.synchronize()
    return b"".join(np.asarray(v.blob).view(np.uint8).tobytes() for _, v in eng.get_state())


@pytest.mark.gpu
@pytest.mark.parametrize("rng,vis", F_CASES, ids=F_IDS)
def test_gpu_mixed_step_seq_chunk_32_equals_chunk_1(rng, vis):
    """human_nums = [1..10], 13 envs per group: step_seq over T = 37 at chunk 32 against chunk 1 (the single-step
    mixed kernels of part B), the nine outputs and every group's state blob bit for bit. Every env resets inside
    launches (time_limit 2)."""
    import torch

    tape = torch.from_numpy(np.random.RandomState(5).normal(0, 0.6, (F_T, F_E, 2)).astype(np.float32)).to(DEV)
    runs = []
    for chunk in (1, 32):
        eng = _f_mixed(rng, vis, chunk)
        eng.reset()
        eng.step_seq(tape)
        torch.cuda.synchronize()
        out = {k: getattr(eng, k).cpu().numpy().copy() for k in SC.OUTPUTS}
        out["state"] = np.frombuffer(_f_state(eng), np.uint8)
        if chunk == 1:
            for _, sv in eng.get_state():
                rc = np.asarray(sv.reset_count).astype(np.int64) - 1
                assert (rc >= (1 + F_T) // 5).all(), (sv.N, rc)
        eng.close()
        runs.append(out)
    SC._same(runs[1], runs[0], "mixed step_seq chunk 32 vs 1, %s visible=%s" % (rng, vis))


F_ROWS = [g + k * len(F_NUMS) for g in range(len(F_NUMS)) for k in (0, 6, 12)]   # three envs of every group


@pytest.mark.gpu
@pytest.mark.parametrize("policy", RO.NAMES)
@pytest.mark.parametrize("rng,vis", F_CASES, ids=F_IDS)
def test_gpu_mixed_rollout_rows_equal_plain_engines(rng, vis, policy):
    """cn_rollout and cn_rollout_masked on the mixed engine (T = 37, noise as in tests/test_rollout_mask.py): the
    first, the middle and the last env of every group against the plain one-env engine of its count at its global
    index (the comparison of test_gpu_mixed_engine_pads_with_zeros_and_equals_plain_engines and
    tests/test_varied_scripted.py): every row bit for bit, the observation's padded slots the never-seen human, the
    mask's padded slots exactly 0. The two mixed rollouts also agree with each other on every shared row and on the
    state."""
    import torch

    from crowdnav_dsrnn_amd.engine import CrowdNavEngine, RolloutNoise

    nz = RolloutNoise(RM.SIGMA, RM.SEED, RM.STEP0)
    keys = ("actions", "executed", "robot_node", "temporal_edges") + RO.RECORDS
    got = {}
    for mask in (False, True):
        eng = _f_mixed(rng, vis)
        eng.reset()
        bufs = eng.rollout_buffers(F_T, executed=True, mask=mask)
        if mask:
            bufs["visible_masks"].fill_(7.0)
        out = eng.rollout(policy, F_T, out=bufs, noise=nz, mask=mask)
        torch.cuda.synchronize()
        got[mask] = {k: out[k].cpu().numpy() for k in keys + ("spatial_edges",) + (("visible_masks",) if mask else ())}
        got[mask]["state"] = _f_state(eng)
        eng.close()
    for k in keys + ("spatial_edges",):
        assert got[True][k].tobytes() == got[False][k].tobytes(), k
    assert got[True]["state"] == got[False]["state"]
    m = got[True]["visible_masks"]
    assert m.shape == (F_T, F_E, max(F_NUMS)) and set(np.unique(m)) <= {0.0, 1.0}
    assert got[False]["done"].sum(axis=0).min() >= 4, got[False]["done"].sum(axis=0)
    seen = []
    for r in F_ROWS:
        n = F_NUMS[r % len(F_NUMS)]
        c = _f_config(vis)
        c.sim.human_nums, c.sim.human_num = None, n
        p = CrowdNavEngine(make_cn_config(c, num_envs=1, env_offset=r, nenv=F_E, phase="train", seed=F_SEED, rng=rng),
                           DEV)
        p.reset()
        want = p.rollout(policy, F_T, noise=nz, mask=True)
        torch.cuda.synchronize()
        for mask in (False, True):
            for k in keys:
                assert want[k].cpu().numpy()[:, 0].tobytes() == np.ascontiguousarray(got[mask][k][:, r]).tobytes(), (r, n, k)
            se = got[mask]["spatial_edges"][:, r]
            assert want["spatial_edges"].cpu().numpy()[:, 0].tobytes() == np.ascontiguousarray(se[:, :n]).tobytes(), (r, n)
            if n < max(F_NUMS):
                pad = se[:, n:]
                assert (pad == pad[:, :1]).all(), (r, n)
                never = 15.0 - got[mask]["robot_node"][:, r, 0, :2].astype(np.float64)
                assert np.abs(pad[:, 0].astype(np.float64) - never).max() <= 1e-5, (r, n)
        assert want["visible_masks"].cpu().numpy()[:, 0].tobytes() == np.ascontiguousarray(m[:, r, :n]).tobytes(), (r, n)
        assert (m[:, r, n:] == 0.0).all(), (r, n)
        seen.append(float(m[:, r, :n].mean()))
        p.close()
    assert 0.1 < np.mean(seen) < 0.9, seen   # (robot.FOV 0.5 pi: the mask is neither all ones nor all zeros)
