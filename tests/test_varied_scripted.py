"""Scripted controllers, fused rollouts and cloning on envs of varying human count (a mixed engine), on the GPU.

Every comparison is exact: the rows of robot_act / step_seq / rollout on the mixed engine against the per-step loop on
an identically built twin and against plain one-env engines of each env's own count.

Common shape: human_nums = [1, 5, 10, 12], E = 28 (7 envs per group, one more than the 6 of a quad-path step
workgroup), holonomic. The groups are the smallest one (1), ORCA's fused path (5), ORCA's 11-agent controller on a
quad-path step, which runs as launch pairs (10), and the kd-tree step path (12); with robot.visible the humans'
simulators hold one agent more and count 10 moves to the kd-tree step path. time_limit = 3 s at time_step 0.25: an
episode ends after 12 steps at the latest, so in T = 40 steps every env of every group resets at least three times
(asserted below as a condition on the inputs; on an MI355X every env recorded 4 `done` in each 40-step call, one
env 5, for both controllers, both RNG modes and the visible robot: profiles/varied_rollout/done_per_env.txt).
T = 40 is one full 32-step chunk plus a remainder at the default chunk; chunk 5 gives many chunks with resets at
their edges. The engines and configs carry the opt-in that lets the scripted calls serve them (cn_mixed_scripted /
sim.human_nums_scripted); without it they refuse, which the refusal test checks."""
import math

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config, make_cn_config, make_varied_cn_configs
from tests.rollout_noise_ref import perturb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUMS, E, T, SEED = [1, 5, 10, 12], 28, 40, 7
COUNTS = [NUMS[r % 4] for r in range(E)]
OBS = ("robot_node", "temporal_edges", "spatial_edges")
RECORDS = ("reward", "done", "event", "info", "ep_return", "ep_len")
POLICIES = ("orca", "social_force")
# (rng, robot.visible, seq chunk or None for the default): both RNG modes, a visible robot once, chunk 5
CASES = [("mt19937", False, None), ("philox", False, None), ("mt19937", False, 5), ("philox", True, 5)]


def _cfg(visible=False, kin="holonomic"):
    c = clone_config(Config())
    c.action_space.kinematics = kin
    c.humans.policy = "orca"
    c.robot.visible = visible
    c.env.time_limit = 3
    c.sim.human_nums = list(NUMS)
    c.sim.human_nums_scripted = True
    return c


def _mixed(rng, visible=False, chunk=None, kin="holonomic", scripted=True):
    """The mixed engine of the common shape, with the scripted calls enabled (cn_mixed_scripted) unless told not."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    cfgs, eg = make_varied_cn_configs(_cfg(visible, kin), NUMS, E, phase="train", seed=SEED, rng=rng)
    eng = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=scripted)
    assert eng.env_humans.tolist() == COUNTS
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    return eng


def _plain(r, rng, visible=False):
    """The plain one-env engine of env r: its own count, env_offset r of nenv E."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    c = _cfg(visible)
    c.sim.human_nums, c.sim.human_num = None, COUNTS[r]
    return CrowdNavEngine(make_cn_config(c, num_envs=1, env_offset=r, nenv=E, phase="train", seed=SEED, rng=rng), DEV)


def _same(a, b, what):
    """Bit equality (torch.equal, with NaN equal to itself: the info row holds NaN where the reference does)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if not torch.equal(a, b):
        x, y = a.detach().cpu().contiguous().numpy(), b.detach().cpu().contiguous().numpy()
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(~((x == y) | ((x != x) & (y != y))))
            assert bad.size == 0, "%s: %d elements differ, first at %s: %s vs %s" % (
                what, len(bad), bad[0], x[tuple(bad[0])], y[tuple(bad[0])])


def _state_bits(eng):
    torch.cuda.synchronize()
    st = eng.get_state()
    views = [st] if eng.groups is None else [v for _, v in st]
    return b"".join(np.asarray(v.blob).view(np.uint8).tobytes() for v in views)


def _noisy(actions, noise, t, env_offset=0):
    if noise is None or noise.sigma == 0.0:
        return actions
    x = perturb(actions.cpu().numpy()[None], noise.sigma, noise.seed, noise.step0 + t, env_offset)[0]
    return torch.from_numpy(x).to(actions.device)


def _eager(eng, policy, T, noise=None, env_offset=0):
    """The per-step loop robot_act -> step, every row cloned; with noise the step takes a + sigma * n computed on the
    host (tests/rollout_noise_ref.py), keyed by the global env index env_offset + row."""
    rows = {k: [] for k in ("actions", "executed") + OBS + RECORDS}
    for t in range(T):
        a = eng.robot_act(policy).clone()
        x = _noisy(a, noise, t, env_offset)
        obs, rew, done, ev, info, epr, epl = eng.step(x)
        rows["actions"].append(a)
        rows["executed"].append(x.clone())
        for k in OBS:
            rows[k].append(obs[k].clone())
        for k, v in zip(RECORDS, (rew, done, ev, info, epr, epl)):
            rows[k].append(v.clone())
    return {k: torch.stack(v) for k, v in rows.items()}


def _poisoned(eng, T, every, executed=False):
    """rollout_buffers with every row poisoned, so that a row the rollout does not write shows."""
    out = eng.rollout_buffers(T, obs_every_step=every, executed=executed)
    for k, v in out.items():
        if every or k not in OBS:   # (without obs_every_step the observation is the engine's own buffer)
            v.fill_(1 if v.dtype == torch.uint8 else 77)
    return out


def _check_rows(got, want, every, keys=None, what=""):
    for k in keys or (("actions",) + OBS + RECORDS):
        w = want[k][-1] if (k in OBS and not every) else want[k]
        _same(got[k].reshape(w.shape), w, "%s %s" % (what, k))


# ---- 1. robot_act ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng,visible", [("mt19937", False), ("philox", True)])
def test_robot_act_rows_equal_plain_engines(rng, visible):
    """Row r of robot_act on the mixed engine == robot_act of the plain one-env engine of env r (env_offset r of
    nenv E, its own count) in the same state: after reset, and after 15 steps of one random action tape. The poison
    written into the action buffer beforehand is gone from every row."""
    mixed = _mixed(rng, visible)
    plain = [_plain(r, rng, visible) for r in range(E)]
    tape = torch.from_numpy(np.random.RandomState(3).normal(0, 0.6, (15, E, 2)).astype(np.float32)).to(DEV)
    mixed.reset()
    for p in plain:
        p.reset()

    def check(where):
        for pol in POLICIES:
            out = torch.full((E, 2), 1e30, device=DEV)
            assert mixed.robot_act(pol, out=out) is out
            assert not (out == 1e30).any(), (where, pol)
            want = torch.cat([p.robot_act(pol) for p in plain])
            _same(out, want, "robot_act %s %s" % (pol, where))
            _same(mixed.robot_act(pol), want, "robot_act (own buffer) %s %s" % (pol, where))

    check("after reset")
    for t in range(15):
        mixed.step(tape[t])
        for r, p in enumerate(plain):
            p.step(tape[t, r:r + 1])
    check("after 15 steps")
    for e in [mixed] + plain:
        e.close()


# ---- 2. step_seq -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng,visible,chunk", CASES)
def test_step_seq_equals_the_step_loop(rng, visible, chunk):
    """step_seq((T, E, 2) random actions) on the mixed engine == T step calls on an identically built twin: every
    output tensor and the final state blob; a second call continues without a reset."""
    a, b = _mixed(rng, visible, chunk), _mixed(rng, visible)
    tape = torch.from_numpy(np.random.RandomState(5).normal(0, 0.6, (2 * T, E, 2)).astype(np.float32)).to(DEV)
    a.reset()
    b.reset()
    for half in range(2):
        acts = tape[half * T:(half + 1) * T]
        got = a.step_seq(acts)
        ndone = torch.zeros(E, dtype=torch.int64, device=DEV)
        for t in range(T):
            want = b.step(acts[t])
            ndone += want[2].long()
        for k in OBS:
            _same(got[0][k], want[0][k], "step_seq %s call %d" % (k, half))
        for k, x, y in zip(RECORDS, got[1:], want[1:]):
            _same(x, y, "step_seq %s call %d" % (k, half))
        assert int(ndone.min()) >= 1, ndone.tolist()
        assert _state_bits(a) == _state_bits(b)
    a.close()
    b.close()


# ---- 3. rollout == the eager loop --------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [True, False])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("rng,visible,chunk", CASES)
def test_rollout_equals_the_eager_loop(rng, visible, chunk, policy, every):
    """rollout(policy, T) on the mixed engine == the eager loop robot_act -> step on a twin: actions, the three
    observation tensors with their padded slots, reward, done, event, info, ep_return, ep_len at every row and the
    state blob, for two calls in a row (the second starts without a reset). Every group sees at least one done."""
    a, b = _mixed(rng, visible, chunk), _mixed(rng, visible)
    a.reset()
    b.reset()
    for call in range(2):
        got = a.rollout(policy, T, obs_every_step=every, out=_poisoned(a, T, every))
        want = _eager(b, policy, T)
        _check_rows(got, want, every, what="rollout %s call %d" % (policy, call))
        per_env = want["done"].long().sum(0)
        assert int(per_env.min()) >= 1, per_env.tolist()       # (every env, hence every group, reset in this call)
        assert _state_bits(a) == _state_bits(b)
    a.close()
    b.close()


# ---- 4. rollout with noise ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("rng,visible,chunk", CASES)
def test_noisy_rollout_equals_the_eager_loop(rng, visible, chunk, policy):
    """rollout(noise=RolloutNoise(0.3, 7, 11)): `executed` and every other row == the eager loop whose step takes
    a + sigma * n from the host restatement keyed by the global env index; two chunked calls (17 then 23 steps,
    step0 continued) == one call of 40; sigma = 0 == the plain rollout with executed == actions."""
    from crowdnav_dsrnn_amd.engine import RolloutNoise

    nz = RolloutNoise(sigma=0.3, seed=7, step0=11)
    a, b, c = _mixed(rng, visible, chunk), _mixed(rng, visible), _mixed(rng, visible, chunk)
    for e in (a, b, c):
        e.reset()
    got = a.rollout(policy, T, out=_poisoned(a, T, True, executed=True), noise=nz)
    want = _eager(b, policy, T, noise=nz)
    _check_rows(got, want, True, keys=("actions", "executed") + OBS + RECORDS, what="noisy %s" % policy)
    assert float((got["executed"] - got["actions"]).abs().max()) > 0.05
    assert int(want["done"].long().sum(0).min()) >= 1
    assert _state_bits(a) == _state_bits(b)
    p1 = c.rollout(policy, 17, noise=nz)
    p2 = c.rollout(policy, 23, noise=RolloutNoise(0.3, 7, 11 + 17))
    for k in ("actions", "executed") + OBS + RECORDS:
        _same(torch.cat([p1[k], p2[k]]), got[k], "chunked noisy %s %s" % (policy, k))
    assert _state_bits(c) == _state_bits(a)
    # sigma = 0 from the state all three share now
    z = a.rollout(policy, T, noise=RolloutNoise(0.0, 7, 0))
    plain = c.rollout(policy, T)
    _same(z["executed"], z["actions"], "sigma 0 executed")
    _check_rows(z, plain, True, what="sigma 0 %s" % policy)
    assert z["num_launches"] == plain["num_launches"] + 1      # the copy into `executed`
    for e in (a, b, c):
        e.close()


# ---- 5. each env against a plain engine ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_rollout_rows_equal_plain_one_env_engines(rng, policy):
    """Two envs of the fused group (count 5) and of the pair group (count 10): their rollout rows, with and without
    noise, == rollout on the plain one-env engine of that count, env_offset and nenv (the paths plain engines
    already had). The padded slots hold the never-seen human of the per-step path."""
    from crowdnav_dsrnn_amd.engine import RolloutNoise

    for nz in (None, RolloutNoise(0.3, 7, 11)):
        mixed = _mixed(rng)
        mixed.reset()
        got = mixed.rollout(policy, T, noise=nz)
        for r in (1, 9, 2, 26):                                 # counts 5, 5, 10, 10
            n = COUNTS[r]
            p = _plain(r, rng)
            p.reset()
            want = p.rollout(policy, T, noise=nz)
            for k in ("actions",) + (("executed",) if nz else ()) + ("robot_node", "temporal_edges") + RECORDS:
                _same(got[k][:, r], want[k][:, 0], "env %d %s" % (r, k))
            _same(got["spatial_edges"][:, r, :n], want["spatial_edges"][:, 0], "env %d spatial_edges" % r)
            pad = got["spatial_edges"][:, r, n:]
            _same(pad, pad[:, :1].expand_as(pad).contiguous(), "env %d padding" % r)
            assert float((pad[:, 0].double() - (15.0 - got["robot_node"][:, r, 0, :2].double())).abs().max()) <= 1e-5
            p.close()
        mixed.close()


# ---- 6. num_launches ---------------------------------------------------------------------------------------------
def _expected_launches(policy, visible, chunk, noisy):
    """The per-group rule of a plain engine of that count, from a fresh reset: fused chunks on the quad step path
    (count + visible <= 10 agents per simulator) where the controller fits (social force; ORCA at count + 1 <= 10),
    after the first step's launch pair; launch pairs (triples with noise) otherwise. Fused noise: one block write."""
    total = 0
    for n in NUMS:
        fused = n + int(visible) <= 10 and (policy == "social_force" or n + 1 <= 10) and chunk > 1
        per_step = 3 if noisy else 2
        if fused:
            total += per_step + math.ceil((T - 1) / chunk) + (1 if noisy else 0)
        else:
            total += per_step * T
    return total


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("visible", [False, True])
def test_num_launches_follows_the_per_group_rule(policy, visible):
    from crowdnav_dsrnn_amd.engine import RolloutNoise

    for nz in (None, RolloutNoise(0.3, 7, 0)):
        eng = _mixed("mt19937", visible)
        assert eng.seq_chunk == 32
        eng.reset()
        got = eng.rollout(policy, T, noise=nz)["num_launches"]
        assert got == _expected_launches(policy, visible, eng.seq_chunk, nz is not None), (policy, visible, nz, got)
        eng.close()


def test_profile_window_keeps_counting_steps():
    """While a cn_profile window is open on the mixed engine, rollout and step_seq run a step at a time: the window
    counts T steps, the launches are pairs (triples with noise) for every group, and the rows are the same."""
    import ctypes

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.engine import RolloutNoise

    L = _lib.lib()
    nz = RolloutNoise(0.3, 7, 11)
    a, b = _mixed("mt19937"), _mixed("mt19937")
    a.reset()
    b.reset()

    def window(fn, steps):
        _lib.check(L.cn_profile(a._h, 1, steps))
        out = fn()
        ms, ms2, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _lib.check(L.cn_profile_read(a._h, ctypes.byref(ms), ctypes.byref(ms2), ctypes.byref(n)))
        _lib.check(L.cn_profile(a._h, 0, 0))
        assert n.value == steps and ms.value > 0.0
        return out

    got = window(lambda: a.rollout("orca", T, noise=nz), T)
    assert got["num_launches"] == 3 * T * len(NUMS)
    _check_rows(got, _eager(b, "orca", T, noise=nz), True, keys=("actions", "executed") + OBS + RECORDS, what="window")
    tape = torch.from_numpy(np.random.RandomState(2).normal(0, 0.6, (T, E, 2)).astype(np.float32)).to(DEV)
    seq = window(lambda: a.step_seq(tape), T)
    for t in range(T):
        want = b.step(tape[t])
    for k, x, y in zip(RECORDS, seq[1:], want[1:]):
        _same(x, y, "window step_seq " + k)
    # the window closed: the groups fuse again
    fused = [n for n in NUMS if n <= 10]                       # (social force: every quad-path group)
    assert a.rollout("social_force", T)["num_launches"] == (len(fused) * math.ceil(T / a.seq_chunk)
                                                             + 2 * T * (len(NUMS) - len(fused)))
    a.close()
    b.close()


# ---- 7. refusals that stay ---------------------------------------------------------------------------------------
def test_refusals_that_stay():
    """rollout(lidar=) and graph mode on a mixed engine, the controllers on a unicycle mixed engine or on one without
    the opt-in (cn_mixed_scripted / sim.human_nums_scripted), and ScriptedRobot on a unicycle env of varying count
    are refused; after each the engine steps as its twin does."""
    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    L = _lib.lib()
    a, b = _mixed("mt19937"), _mixed("mt19937")
    a.reset()
    b.reset()
    act = torch.from_numpy(np.random.RandomState(1).normal(0, 0.6, (E, 2)).astype(np.float32)).to(DEV)

    def still_steps():
        for x, y in zip(a.step(act)[1:], b.step(act)[1:]):
            _same(x, y, "step after a refusal")
        assert _state_bits(a) == _state_bits(b)

    with pytest.raises(RuntimeError, match="mixed"):
        a.rollout("orca", 4, lidar=dict(beams=16, max_range=5.0, robot_radius=0.3))
    assert L.cn_last_error().startswith(b"cn_rollout: not on a mixed engine")
    still_steps()
    with pytest.raises(RuntimeError, match="graph mode"):
        a.set_graph_mode(True)
    still_steps()
    out = torch.zeros((E, 1, 7 + 16), device=DEV)
    with pytest.raises(RuntimeError, match="mixed"):
        a.lidar_scan(out, beams=16)
    still_steps()
    uni, uni2 = _mixed("mt19937", kin="unicycle"), _mixed("mt19937", kin="unicycle")
    uni.reset()
    uni2.reset()
    for call in (lambda: uni.robot_act("orca"), lambda: uni.rollout("social_force", 4),
                 lambda: uni.rollout("orca", 4, noise=dict(sigma=0.1))):
        with pytest.raises(RuntimeError, match="unicycle mixed engine"):
            call()
    small = act * 0.1
    for x, y in zip(uni.step(small)[1:], uni2.step(small)[1:]):
        _same(x, y, "unicycle step after a refusal")
    venv = type("V", (), {"config": _cfg(kin="unicycle"), "obs_mode": "srnn"})()
    with pytest.raises(UnsupportedConfig, match="holonomic"):
        ScriptedRobot(venv, "orca")
    # without the opt-in a mixed engine refuses the scripted calls as it always has; step_seq needs none
    off, off2 = _mixed("mt19937", scripted=False), _mixed("mt19937", scripted=False)
    off.reset()
    off2.reset()
    for call in (lambda: off.robot_act("orca"), lambda: off.rollout("social_force", 4),
                 lambda: off.rollout("orca", 4, noise=dict(sigma=0.1))):
        with pytest.raises(RuntimeError, match="not on a mixed engine"):
            call()
    tape = act.unsqueeze(0).repeat(6, 1, 1).contiguous()
    got = off.step_seq(tape)
    for t in range(6):
        want = off2.step(tape[t])
    for x, y in zip(got[1:], want[1:]):
        _same(x, y, "step_seq without the opt-in")
    assert _lib.check(L.cn_mixed_scripted(off._h, 1)) == 0      # the opt-in can be given later
    assert tuple(off.robot_act("orca").shape) == (E, 2)
    plain = _plain(1, "mt19937")
    assert L.cn_mixed_scripted(plain._h, 1) == -1 and L.cn_mixed_scripted(None, 1) == -1     # CN_EINVAL
    off_cfg = _cfg()
    off_cfg.sim.human_nums_scripted = False
    with pytest.raises(UnsupportedConfig, match="human_nums_scripted"):
        ScriptedRobot(type("V", (), {"config": off_cfg, "obs_mode": "srnn"})(), "orca")
    for e in (a, b, uni, uni2, off, off2, plain):
        e.close()


# ---- 8. ScriptedRobot as an actor --------------------------------------------------------------------------------
class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def _eval_cfg():
    c = clone_config(Config())
    c.action_space.kinematics = "holonomic"
    c.humans.policy = "orca"
    c.sim.human_nums = [5, 10]
    c.sim.human_nums_scripted = True
    c.env.test_size = 16
    c.env.time_limit = 12
    return c


def test_scripted_robot_evaluates_a_varied_env_per_count():
    """evaluate(ScriptedRobot(venv, 'orca')) on human_nums = [5, 10] with 8 envs and 16 test episodes: the per-count
    block holds 8 episodes per count and its totals are the overall line's; evaluate_scripted records the same."""
    from crowdnav_dsrnn_amd import abi
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.evaluation import evaluate, evaluate_scripted
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    c = _eval_cfg()

    def venv():
        return CrowdNavVecEnv(c, 8, c.env.seed, DEV, allow_early_resets=True, nenv=8, phase="test")

    v = venv()                                                 # the actor's own calls, on an env of their own
    robot = ScriptedRobot(v, "orca")
    assert robot.base.human_num == 10
    o = v.reset()
    _, action, _, _ = robot.act(o, None, None)
    assert tuple(action.shape) == (8, 2)
    ro = robot.rollout(3)
    assert tuple(ro["detected_human_num"].shape) == (3, 8, 1)
    assert torch.equal(ro["detected_human_num"][2], v.engine.env_humans.float().reshape(8, 1))
    assert tuple(ro["spatial_edges"].shape) == (3, 8, 10, 2)
    v.close()
    v = venv()
    robot = ScriptedRobot(v, "orca")
    log = _Log()
    evaluate(robot, None, v, 8, DEV, c, log, verbose=False)
    last = dict(evaluate.last)
    pc = last["per_count"]
    assert list(pc) == [5, 10] and all(pc[n]["episodes"] == 8 for n in pc)
    for key, ev in (("success_rate", abi.EV_REACHGOAL), ("collision_rate", abi.EV_COLLISION),
                    ("timeout_rate", abi.EV_TIMEOUT)):
        assert abs(sum(pc[n][key] * pc[n]["episodes"] for n in pc) / 16 - last[key]) < 1e-12
        for n in pc:
            sel = last["records"]["humans"] == n
            assert pc[n][key] == float((last["records"]["event"][sel] == ev).sum()) / 8
    assert last["records"]["humans"].tolist() == [[5, 10][g % 2] for g in range(16)]
    i = log.lines.index("PER HUMAN COUNT: ")
    assert len(log.lines) == i + 3 and log.lines[i + 1].startswith("5 humans: success rate: ")
    assert log.lines[i + 2].startswith("10 humans: success rate: ") and log.lines[i + 2].endswith("episodes: 8")
    log2 = _Log()
    evaluate_scripted("orca", venv(), 8, DEV, c, log2, verbose=False)
    assert log2.lines == log.lines
    for k, x in last["records"].items():
        np.testing.assert_array_equal(evaluate.last["records"][k], x, err_msg=k)
    assert evaluate.last["per_count"] == pc


# ---- 9. BehaviourCloning -----------------------------------------------------------------------------------------
BE, BT = 8, 8


def _bc(sigma=0.2):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import BehaviourCloning
    from tests.helpers import make_policy

    c = clone_config(Config())
    c.action_space.kinematics = "holonomic"
    c.humans.policy = "orca"
    c.sim.human_nums = [5, 10]
    c.sim.human_nums_scripted = True
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.env.time_limit = 1.5
    c.training.num_processes = BE
    c.ppo.num_steps, c.ppo.num_mini_batch, c.ppo.epoch = BT, 1, 2
    envs = CrowdNavVecEnv(c, BE, c.env.seed, DEV, allow_early_resets=True, nenv=BE, phase="train")
    pol = make_policy(10, E=BE, T=BT, device=DEV)
    pol.train()
    return c, envs, pol, BehaviourCloning(c, envs, pol, expert="orca", sigma=sigma, seed=11, lr=1e-3, value_coef=0.0)


def test_behaviour_cloning_on_a_varied_env():
    """BehaviourCloning on human_nums = [5, 10] (8 envs x 8 steps): after collect() the storage's rows equal a replayed
    ScriptedRobot.rollout with the same noise and detected_human_num is filled in all T + 1 slots; the NLL of one
    fixed chunk falls over 20 passes; the policy then goes through one RolloutTrainer update."""
    from crowdnav_dsrnn_amd.engine import RolloutNoise
    from crowdnav_dsrnn_amd.learner import PPO
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    c, envs, pol, bc = _bc()
    r = bc.rollouts
    counts = envs.engine.env_humans.float().reshape(1, BE, 1)
    assert sorted(set(envs.env_human_nums)) == [5, 10]
    assert tuple(r.obs["spatial_edges"].shape) == (BT + 1, BE, 10, 2)
    before = envs.engine.get_state()
    first = {k: r.obs[k][0].clone() for k in OBS}
    out = bc.collect()
    for k in OBS:
        assert out[k].data_ptr() == r.obs[k][1:].data_ptr(), k     # the chunk buffers are the storage's own tensors
    assert out["actions"].data_ptr() == r.actions.data_ptr()
    _same(r.obs["detected_human_num"], counts.expand(BT + 1, BE, 1).contiguous(), "detected_human_num")
    stored = {k: r.obs[k].clone() for k in OBS}
    actions, rewards, masks = r.actions.clone(), r.rewards.clone(), r.masks.clone()
    executed, done = out["executed"].clone(), out["done"].clone()
    assert done.any() and not done.all()
    envs.engine.set_state(before)
    ref = ScriptedRobot(envs, "orca").rollout(BT, noise=RolloutNoise(0.2, 11, 0))
    for k in OBS:
        _same(stored[k][0], first[k], "obs[0] " + k)
        _same(stored[k][1:], ref[k], "stored " + k)
    _same(actions, ref["actions"], "labels")
    _same(executed, ref["executed"], "executed")
    _same(rewards[..., 0], ref["reward"], "rewards")
    _same(done, ref["done"], "done")
    assert torch.equal(masks[1:, :, 0], 1.0 - ref["done"].float())
    assert float((executed - actions).abs().max()) > 0.05
    # (the replay left the engine where collect() had left it: the same state, the same noise)
    nll0 = float(bc.chunk_nll())
    bc.fit(20)
    nll1 = float(bc.chunk_nll())
    print("nll before %.6f, after 20 passes %.6f" % (nll0, nll1))
    assert np.isfinite(nll0) and np.isfinite(nll1) and nll1 < nll0, (nll0, nll1)
    agent = PPO(pol, c.ppo.clip_param, c.ppo.epoch, c.ppo.num_mini_batch, c.ppo.value_loss_coef, c.ppo.entropy_coef,
                lr=c.training.lr, eps=c.training.eps, max_grad_norm=c.training.max_grad_norm)
    tr = RolloutTrainer(c, envs, pol, agent)
    st = tr.update()
    assert all(np.isfinite(st[k]) for k in ("value_loss", "action_loss", "dist_entropy")), st
    _same(tr.rollouts.obs["detected_human_num"], counts.expand(BT + 1, BE, 1).contiguous(), "trainer counts")
    envs.close()
