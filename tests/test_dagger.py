"""The learner in the loop: cn_robot_mix (the per-env coin between the learner's action and the expert's label) and
learner.DAgger (the trainer around it).

The coin and the select are DEFINED in include/crowdnav.h; tests/dagger_ref.py restates them in numpy, and every GPU
comparison with it is exact. The label is cn_robot_act's own launch, so it is compared with robot_act bit for bit, and
the trainer's chunks are compared bit for bit with what they are defined as: the expert's rollout at beta = 1, a
hand-written act -> robot_act -> step_device loop at beta = 0, the eager loop for the captured one.

Trainer shapes: 16 envs x 5 humans, chunks of 8 steps, time_limit 1.5 s at time_step 0.25 (an episode lasts at most 6
steps), so episode boundaries fall inside every chunk."""
import copy
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dagger_ref  # noqa: E402

from crowdnav_dsrnn_amd.config import (Config, UnsupportedConfig, clone_config, make_cn_config,  # noqa: E402
                                       make_varied_cn_configs)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EINVAL = -1
E, N, T = 16, 5, 8
OBS = ("robot_node", "temporal_edges", "spatial_edges")
SEED, STEP0 = 20240607, 5
BETAS = (0.0, 0.25, 0.5, 1.0)


def _config(kin="holonomic", dwa=False, policy="srnn", masks=False, n_env=E):
    c = clone_config(Config())
    c.sim.human_num = N
    c.humans.policy = "orca"
    c.robot.policy = policy
    c.action_space.kinematics = kin
    if dwa:
        c.robot.scripted_dwa = True
    if policy == "convgru":
        c.lidar.enable = True
        c.lidar.live = True
    c.sim.visible_masks = masks
    if masks:
        c.robot.FOV = 0.5
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.env.time_limit = 1.5
    c.env.time_step = 0.25
    c.training.num_processes = n_env
    c.ppo.num_steps = T
    c.ppo.num_mini_batch = 1
    c.ppo.epoch = 2
    return c


# ---- CPU ----------------------------------------------------------------------------------------
def test_header_struct_equals_the_ctypes_mirror_and_the_symbols_are_exported():
    from crowdnav_dsrnn_amd import _lib, abi

    txt = open(os.path.join(REPO, "include", "crowdnav.h")).read()
    m = re.search(r"typedef struct cn_mix_ctl \{(.*?)\} cn_mix_ctl;", txt, re.S)
    assert m, "include/crowdnav.h does not define cn_mix_ctl"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [tuple(f.split()) for f in body.split(";") if f.strip()]
    assert fields == [("float", "beta"), ("uint32_t", "seed"), ("int64_t", "step0")]
    assert [f[0] for f in abi.CnMixCtl._fields_] == [f[1] for f in fields]
    assert ctypes.sizeof(abi.CnMixCtl) == 16
    assert (abi.CnMixCtl.beta.offset, abi.CnMixCtl.seed.offset, abi.CnMixCtl.step0.offset) == (0, 4, 8)
    want = {"cn_mix_ctl_set": ["void*", "cn_mix_ctl*", "constcn_mix_ctl*"],
            "cn_robot_mix": ["cn_engine*", "void*", "int", "constfloat*", "constcn_mix_ctl*", "int32_t", "float*",
                             "float*", "uint8_t*"]}
    for fn, types in want.items():
        m = re.search(r"^int %s\((.*?)\);" % fn, txt, re.S | re.M)
        assert m, "include/crowdnav.h does not declare %s" % fn
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == types
        assert fn in _lib.EXPORTED


def test_null_arguments_are_einval_without_a_launch():
    from crowdnav_dsrnn_amd import _lib, abi, build

    build.build()
    L = _lib.lib()
    assert len(L.cn_robot_mix.argtypes) == 9 and len(L.cn_mix_ctl_set.argtypes) == 3
    v = abi.CnMixCtl(0.5, 1, 0)
    assert L.cn_mix_ctl_set(None, None, ctypes.byref(v)) == EINVAL and b"cn_mix_ctl_set" in L.cn_last_error()
    assert L.cn_mix_ctl_set(None, 16, None) == EINVAL
    for bad in (-0.25, 1.5, float("nan"), float("inf")):   # (16: a non-NULL address that must never be written)
        assert L.cn_mix_ctl_set(None, 16, ctypes.byref(abi.CnMixCtl(bad, 1, 0))) == EINVAL, bad
        assert b"beta" in L.cn_last_error()
    assert L.cn_robot_mix(None, None, 0, 16, 16, 0, 16, 16, 16) == EINVAL and b"null engine" in L.cn_last_error()


def test_coin_known_answers_and_the_package_restatement():
    from crowdnav_dsrnn_amd import policy_factory as pf

    assert int(dagger_ref.coin_word(11, 5, 0)) == 0xd95b6302
    u = dagger_ref.coin(11, 5, 0)
    assert u.dtype == np.float32 and float(u) == 0xd95b63 / 2.0 ** 24 and abs(float(u) - 0.8490507) < 5e-8
    assert abs(float(dagger_ref.coin(0, 0, 0)) - 0.73571277) < 5e-8   # word z of Random123's zero vector: 0xbc57ac4c
    assert float(dagger_ref.coin(0, 0, 0)) == 0xbc57ac / 2.0 ** 24
    k, G = np.arange(-3, 40)[:, None], np.arange(990, 1300)[None, :]
    for seed in (0, 11, 0xFFFFFFFF, SEED):
        a, b = pf.mix_coin(seed, k, G), dagger_ref.coin(seed, k, G)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert b.min() >= 0.0 and b.max() < 1.0
    # step0 continues the sequence; the env's global index selects the stream
    assert np.array_equal(pf.mix_coin(7, 12 + np.arange(4)[:, None], 3 + np.arange(5)[None, :]),
                          pf.mix_coin(7, 10 + np.arange(6)[:, None], np.arange(8)[None, :])[2:, 3:])


def test_restated_select_is_the_identity_at_beta_zero_and_one():
    from crowdnav_dsrnn_amd import policy_factory as pf

    rs = np.random.RandomState(4)
    label = rs.uniform(-1, 1, (6, 40, 2)).astype(np.float32)
    learner = rs.uniform(-1, 1, (6, 40, 2)).astype(np.float32)
    label[0, 0], learner[0, 0] = (-0.0, 1e-42), (0.0, 1e-42)     # differ in the sign bit alone
    learner[1] = label[1]
    label[2, 3, 0] = learner[2, 3, 0] = -0.0
    k, G = (STEP0 + np.arange(6))[:, None], (100 + np.arange(40))[None, :]
    x0, f0 = pf.robot_mix_ref(label, learner, 0.0, SEED, k, G)
    x1, f1 = pf.robot_mix_ref(label, learner, 1.0, SEED, k, G)
    assert x0.dtype == np.float32 and x0.tobytes() == learner.tobytes() and x1.tobytes() == label.tobytes()
    assert np.signbit(x1[0, 0, 0]) and not np.signbit(x0[0, 0, 0]) and x0[0, 0, 1] == np.float32(1e-42)
    assert f0.dtype == np.uint8 and not (f0 & 1).any() and (f1 & 1).all()
    agree = np.zeros((6, 40), bool)
    agree[1] = True
    assert np.array_equal((f0 & 2) != 0, agree) and np.array_equal(f0 & 2, f1 & 2) and f0[0, 0] == 0
    for beta in (0.25, 0.5):
        x, f = pf.robot_mix_ref(label, learner, beta, SEED, k, G)
        xr, fr = dagger_ref.mix(label, learner, beta, SEED, STEP0, 100)
        assert x.tobytes() == xr.tobytes() and f.tobytes() == fr.tobytes()
        assert 0.5 * beta < (f & 1).mean() < 1.5 * beta


class _Stub:
    """What DAgger reads before it touches the engine (no GPU behind it)."""

    num_envs = 8
    obs_mode = "srnn"

    def __init__(self, config):
        self.config = config

    def __getattr__(self, name):
        raise AssertionError("the check must come before the engine is touched (%s)" % name)


class _Pol:
    srnn, convgru = True, False


def test_dagger_is_exported_and_checks_before_the_gpu():
    from crowdnav_dsrnn_amd import learner

    assert hasattr(learner, "DAgger")
    holo, uni = _config(), _config(kin="unicycle")
    with pytest.raises(UnsupportedConfig):
        learner.DAgger(holo, _Stub(holo), _Pol(), expert="cadrl")
    with pytest.raises(UnsupportedConfig):      # 'dwa' (the default expert) without config.robot.scripted_dwa
        learner.DAgger(uni, _Stub(uni), _Pol())
    with pytest.raises(UnsupportedConfig):      # ... and on a holonomic env
        learner.DAgger(holo, _Stub(holo), _Pol(), expert="dwa")
    for beta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="beta"):
            learner.DAgger(holo, _Stub(holo), _Pol(), expert="orca", beta=beta)
    for k in (0, -2):
        with pytest.raises(ValueError, match="aggregate"):
            learner.DAgger(holo, _Stub(holo), _Pol(), expert="orca", aggregate=k)
    varied = _config()
    varied.sim.human_nums = [3, 5]              # robot_act's rule: only with sim.human_nums_scripted
    with pytest.raises(UnsupportedConfig, match="human_nums_scripted"):
        learner.DAgger(varied, _Stub(varied), _Pol(), expert="orca")
    conv = _config(policy="convgru")
    stub = _Stub(conv)
    stub.obs_mode = "convgru"
    with pytest.raises(UnsupportedConfig, match="ConvGRU"):   # the DSRNN cannot read the LiDAR row
        learner.DAgger(conv, stub, _Pol(), expert="orca")


# ---- GPU: the kernel ----------------------------------------------------------------------------
KERNEL_CASES = {"orca": ("holonomic", "orca", False), "social_force": ("holonomic", "social_force", False),
                "dwa": ("unicycle", "dwa", False), "mixed": ("holonomic", "orca", True)}


def _engine(case, n_env, offset=0):
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    kin, name, mixed = KERNEL_CASES[case]
    c = _config(kin=kin, dwa=name == "dwa")
    nenv = offset + n_env
    if mixed:
        cfgs, eg = make_varied_cn_configs(c, [3, 5], n_env, env_offset=offset, nenv=nenv, phase="train")
        eng = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=True)
    else:
        eng = CrowdNavEngine(make_cn_config(c, num_envs=n_env, env_offset=offset, nenv=nenv, phase="train"), DEV,
                             scripted_dwa=True if name == "dwa" else None)
    eng.reset()
    return eng, name


def _learner_actions(label, seed):
    """Learner actions for the labels of one state: random ones, a -0.0f and a denormal in row 0, and the label itself
    in every third row (bit 1 of the flags must be set there and only there)."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-1, 1, label.shape).astype(np.float32)
    a[0] = (-0.0, 1e-42)
    a[1::3] = label[1::3]
    return a


def _kernel_case(case, n_env, offset, steps):
    """robot_mix at every beta and every t of `steps` on one engine: label against robot_act, executed and flags
    against the restatement. Returns {beta: share of coins taken}."""
    import torch

    eng, name = _engine(case, n_env, offset)
    want_label = eng.robot_act(name).clone()
    torch.cuda.synchronize()
    lab = want_label.cpu().numpy()
    assert np.isfinite(lab).all() and np.abs(lab).max() > 0
    ctl = eng.mix_ctl()
    share = {}
    for beta in BETAS:
        eng.set_mix_ctl(ctl, beta, SEED, STEP0)
        taken = []
        for t in steps:
            a = _learner_actions(lab, 100 + t)
            label = torch.full((n_env, 2), 7.0, device=DEV)
            executed = torch.full((n_env, 2), 7.0, device=DEV)
            flags = torch.full((n_env,), 255, dtype=torch.uint8, device=DEV)
            out = eng.robot_mix(name, torch.from_numpy(a).to(DEV), ctl, t, label=label, executed=executed, flags=flags)
            assert out[0] is label and out[1] is executed and out[2] is flags
            torch.cuda.synchronize()
            assert label.cpu().numpy().tobytes() == lab.tobytes(), (case, n_env, beta, t)
            x, f = dagger_ref.mix(lab[None], a[None], beta, SEED, STEP0, offset, t0=t)
            assert executed.cpu().numpy().tobytes() == x[0].tobytes(), (case, n_env, beta, t)
            assert flags.cpu().numpy().tobytes() == f[0].tobytes(), (case, n_env, beta, t)
            agree = np.zeros(n_env, bool)
            agree[1::3] = True
            assert np.array_equal((f[0] & 2) != 0, agree)
            if beta == 1.0:
                assert np.signbit(a[0, 0]) and (f[0] & 1).all()
            if beta == 0.0:
                assert not (f[0] & 1).any() and np.signbit(executed.cpu().numpy()[0, 0])
            taken.append((f[0] & 1).astype(np.float64))
        share[beta] = float(np.concatenate(taken).mean())
    eng.close()
    return share


@pytest.mark.gpu
@pytest.mark.parametrize("n_env", [1, 3, 65])
@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
def test_gpu_kernel_equals_the_restatement(case, n_env):
    _kernel_case(case, n_env, 0, (0, 7))


@pytest.mark.gpu
@pytest.mark.parametrize("case,offset", [("orca", 0), ("social_force", 0), ("dwa", 0), ("mixed", 0), ("orca", 1000),
                                         ("mixed", 1000)])
def test_gpu_kernel_at_257_envs_takes_a_binomial_share_of_the_coins(case, offset):
    """Two 256-lane workgroups. The share of coins taken over t = 0..7 lies within 4 binomial standard deviations of
    beta (n = 8 * 257; the reference coin itself lies within 1.5 at offsets 0 and 1000), so the exact comparison
    with the restatement is not one of constants."""
    n_env = 257
    share = _kernel_case(case, n_env, offset, range(8))
    assert share[0.0] == 0.0 and share[1.0] == 1.0
    for beta in (0.25, 0.5):
        sd = (beta * (1 - beta) / (8 * n_env)) ** 0.5
        print("%s offset %d beta %.2f: share %.4f (%.2f sd)" % (case, offset, beta, share[beta],
                                                                 (share[beta] - beta) / sd))
        assert abs(share[beta] - beta) <= 4 * sd, (beta, share[beta])


@pytest.mark.gpu
def test_gpu_captured_graph_reads_the_block_at_run_time():
    """One graph of robot_mix at t = 0..3, captured under (beta 0.5, SEED, step0 5), replayed after set_mix_ctl to
    another beta, seed and step0: the rows are the eager calls' with those values, not the captured ones'."""
    import torch

    from crowdnav_dsrnn_amd import _lib

    n_env, Tg = 65, 4
    eng, name = _engine("orca", n_env)
    lab = eng.robot_act(name).clone().cpu().numpy()
    a = np.stack([_learner_actions(lab, 200 + t) for t in range(Tg)])
    learner = torch.from_numpy(a).to(DEV)
    ctl = eng.mix_ctl()
    eng.set_mix_ctl(ctl, 0.5, SEED, STEP0)
    bufs = [torch.zeros((Tg, n_env, 2), device=DEV), torch.zeros((Tg, n_env, 2), device=DEV),
            torch.zeros((Tg, n_env), dtype=torch.uint8, device=DEV)]
    eng.robot_mix(name, learner[0], ctl, 0)   # one eager call before the capture
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        for t in range(Tg):
            eng.robot_mix(name, learner[t], ctl, t, label=bufs[0][t], executed=bufs[1][t], flags=bufs[2][t])
    counts = _lib.graph_node_counts(g.raw_cuda_graph())
    assert counts.get("memset", 0) == 0 and counts["kernel"] == counts["total"] == 2 * Tg, counts
    g.instantiate()
    seen = []
    for beta, seed, step0 in ((0.5, SEED, STEP0), (0.25, SEED + 1, 1000), (1.0, 3, 2 ** 32 + 7), (0.0, 3, 0)):
        eng.set_mix_ctl(ctl, beta, seed, step0)
        g.replay()
        torch.cuda.synchronize()
        got = [b.cpu().numpy().copy() for b in bufs]
        x, f = dagger_ref.mix(np.broadcast_to(lab, a.shape), a, beta, seed, step0, 0)
        assert got[0].tobytes() == np.broadcast_to(lab, a.shape).tobytes()
        assert got[1].tobytes() == x.tobytes() and got[2].tobytes() == f.tobytes(), (beta, seed, step0)
        eager = [eng.robot_mix(name, learner[t], ctl, t) for t in range(Tg)]
        torch.cuda.synchronize()
        for t in range(Tg):
            assert eager[t][1].cpu().numpy().tobytes() == got[1][t].tobytes()
            assert eager[t][2].cpu().numpy().tobytes() == got[2][t].tobytes()
        seen.append(got[2].tobytes())
    assert len(set(seen)) == 4
    eng.close()


@pytest.mark.gpu
def test_gpu_robot_mix_error_codes_come_before_any_launch():
    import torch

    from crowdnav_dsrnn_amd import _lib
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    L = _lib.lib()
    n_env = 8
    bufs = [torch.zeros((n_env, 2), device=DEV) for _ in range(3)]
    flags = torch.zeros((n_env,), dtype=torch.uint8, device=DEV)
    EUNSUPPORTED = -2

    def call(eng, policy, ctl, t=0, null=None):
        p = [bufs[0].data_ptr(), ctl.data_ptr(), t, bufs[1].data_ptr(), bufs[2].data_ptr(), flags.data_ptr()]
        if null is not None:
            p[null] = None
        return L.cn_robot_mix(eng._h, None, policy, *p)

    eng = CrowdNavEngine(make_cn_config(_config(), num_envs=n_env), DEV)
    eng.reset()
    ctl = eng.mix_ctl()
    for null in (0, 1, 3, 4, 5):
        assert call(eng, 0, ctl, null=null) == EINVAL, null
    assert call(eng, 0, ctl, t=-1) == EINVAL
    assert call(eng, 3, ctl) == EINVAL and call(eng, 2, ctl) == EINVAL     # unknown; 'dwa' without cn_scripted_dwa
    with pytest.raises(ValueError):
        eng.set_mix_ctl(ctl, 1.25)
    with pytest.raises(ValueError):
        eng.robot_mix("orca", bufs[0], ctl, -1)
    with pytest.raises(ValueError):
        eng.robot_mix("orca", bufs[0], ctl, 0, label=bufs[0])
    eng.close()
    uni = CrowdNavEngine(make_cn_config(_config(kin="unicycle"), num_envs=n_env), DEV)
    uni.reset()
    assert call(uni, 0, ctl) == EUNSUPPORTED and b"holonomic" in L.cn_last_error()
    uni.close()
    cfgs, eg = make_varied_cn_configs(_config(), [3, 5], n_env, phase="train")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV)
    mixed.reset()
    assert call(mixed, 0, ctl) == EUNSUPPORTED and b"mixed" in L.cn_last_error()
    mixed.close()
    torch.cuda.synchronize()
    assert all(float(b.abs().max()) == 0.0 for b in bufs) and int(flags.max()) == 0   # nothing was launched


# ---- GPU: the trainer ---------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _envs(c, n_env=E):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    return CrowdNavVecEnv(c, n_env, c.env.seed, DEV, allow_early_resets=True, nenv=n_env, phase="train")


def _trainer(expert="orca", kin="holonomic", seed=11, **kw):
    from crowdnav_dsrnn_amd.learner import DAgger
    from tests.helpers import make_policy

    c = _config(kin=kin, dwa=expert == "dwa")
    envs = _envs(c)
    pol = make_policy(N, E=E, T=T, device=DEV)
    pol.train()
    return c, envs, pol, DAgger(c, envs, pol, expert=expert, seed=seed, **kw)


@pytest.mark.gpu
def test_gpu_beta_one_is_the_experts_rollout():
    import torch

    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    c, envs, pol, dg = _trainer(beta=1.0, beta_decay=1.0)
    dg.collect()
    r = dg.rollouts
    envs2 = _envs(_config())
    envs2.reset()
    ref = ScriptedRobot(envs2, "orca").rollout(T)
    torch.cuda.synchronize()
    for k in OBS:
        assert _bits(r.obs[k][1:]) == _bits(ref[k]), k
    assert _bits(dg.labels) == _bits(ref["actions"]) == _bits(dg.executed) == _bits(r.actions)
    assert _bits(r.rewards[..., 0]) == _bits(ref["reward"])
    assert _bits(dg.done) == _bits(ref["done"]) and _bits(dg.event) == _bits(ref["event"])
    assert bool(dg.done.any()) and not bool(dg.done.all())
    assert torch.equal(r.masks[1:, :, 0], 1.0 - ref["done"].float())
    assert bool((dg.flags & 1).all())
    envs.close()
    envs2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("expert,kin", [("orca", "holonomic"), ("dwa", "unicycle")])
def test_gpu_beta_zero_is_the_learners_loop(expert, kin):
    """The chunk against act -> robot_act -> step_device written out by hand on a second env and a copy of the
    policy: observations, labels (robot_act of the state BEFORE step t), proposed = executed, rewards, done."""
    import torch

    c, envs, pol, dg = _trainer(expert=expert, kin=kin, beta=0.0)
    pol2 = copy.deepcopy(pol)
    dg.collect()
    r = dg.rollouts
    torch.cuda.synchronize()
    assert _bits(dg.executed) == _bits(dg.proposed) and not bool((dg.flags & 1).any())
    assert _bits(r.actions) == _bits(dg.labels) and _bits(dg.labels) != _bits(dg.proposed)
    envs2 = _envs(_config(kin=kin, dwa=expert == "dwa"))
    obs = {k: v.clone() for k, v in envs2.reset().items()}
    hxs = {"human_node_rnn": torch.zeros(E, 1, c.SRNN.human_node_rnn_size, device=DEV),
           "human_human_edge_rnn": torch.zeros(E, N + 1, c.SRNN.human_human_edge_rnn_size, device=DEV)}
    masks = torch.ones(E, 1, device=DEV)
    ended = 0
    with torch.no_grad():
        for t in range(T):
            for k in OBS:
                assert _bits(r.obs[k][t]) == _bits(obs[k]), (k, t)
            _, action, _, hxs = pol2.act(obs, hxs, masks, deterministic=True)
            label = envs2.robot_act(expert).clone()
            assert _bits(dg.labels[t]) == _bits(label), t
            assert _bits(dg.proposed[t]) == _bits(action), t
            o, rew, done, ev, _, _, _ = envs2.step_device(action)
            assert _bits(r.rewards[t, :, 0]) == _bits(rew) and _bits(dg.done[t]) == _bits(done), t
            assert _bits(dg.event[t]) == _bits(ev), t
            obs = {k: o[k].clone() for k in OBS}
            masks = 1.0 - done.float().unsqueeze(1)
            assert torch.equal(r.masks[t + 1], masks), t
            ended += int(done.sum())
    for k in OBS:
        assert _bits(r.obs[k][T]) == _bits(obs[k]), k
    assert ended > 0   # episode boundaries inside the chunk: the recurrent state was cleared there
    envs.close()
    envs2.close()


@pytest.mark.gpu
def test_gpu_graph_equals_eager_over_changing_beta():
    """beta = 1, 0.5, 0.25, 0.125 over four chunks: eager warm-up, capture, two replays against four eager chunks."""
    import torch

    def run(graphs):
        torch.manual_seed(5)
        c, envs, pol, dg = _trainer(beta=1.0, beta_decay=0.5, graphs=graphs, lr=1e-3)
        rows = []
        for i in range(4):
            st = dg.update()
            assert st["beta"] == 0.5 ** i
            torch.cuda.synchronize()
            r = dg.rollouts
            row = {k: _bits(r.obs[k]) for k in OBS}
            row.update(actions=_bits(r.actions), rewards=_bits(r.rewards), masks=_bits(r.masks),
                       returns=_bits(r.returns), executed=_bits(dg.executed), flags=_bits(dg.flags),
                       proposed=_bits(dg.proposed), done=_bits(dg.done))
            row.update({"w:" + k: _bits(v) for k, v in pol.state_dict().items()})
            row["stats"] = (st["nll"], st["value_loss"], st["took_expert"], st["agree"], st["episodes"])
            x, f = dagger_ref.mix(dg.labels.cpu().numpy(), dg.proposed.cpu().numpy(), st["beta"], 11, i * T, 0)
            assert row["flags"] == f.tobytes() and row["executed"] == x.tobytes(), i
            assert st["took_expert"] == float((f & 1).mean()) and st["agree"] == float(((f & 2) != 0).mean())
            rows.append(row)
        audit, on = dg.graph_audit, dg.graphs
        envs.close()
        return rows, audit, on

    eager, audit_e, on_e = run(False)
    graph, audit, on = run(True)
    assert audit_e is None and not on_e
    assert on and audit is not None and audit.get("memset", 0) == 0 and audit["kernel"] > 0, audit
    for i, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert a[k] == b[k], (i, k)
    assert eager[0]["stats"][2] == 1.0 and 0.0 < eager[3]["stats"][2] < 0.5


@pytest.mark.gpu
def test_gpu_fitting_lowers_the_nll_of_a_fixed_chunk():
    c, envs, pol, dg = _trainer(beta=0.5, lr=1e-3, num_mini_batch=1, value_coef=0.0)
    dg.collect()
    nll0 = float(dg.chunk_nll())
    acc, n = dg.fit(20)
    nll1 = float(dg.chunk_nll())
    print("nll before %.6f, after 20 passes %.6f" % (nll0, nll1))
    assert n == 20 and np.isfinite(nll0) and np.isfinite(nll1) and nll1 < nll0, (nll0, nll1)
    envs.close()


@pytest.mark.gpu
def test_gpu_two_trainers_agree_bit_for_bit_and_hand_over_to_ppo():
    import torch

    from crowdnav_dsrnn_amd.learner import PPO
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer
    from tests.helpers import load

    def run(hand_over):
        torch.manual_seed(3)
        c, envs, pol, dg = _trainer(beta=1.0, beta_decay=0.5, num_mini_batch=2, epochs=2, aggregate=2)
        stats = [dg.update() for _ in range(3)]
        sd = {k: v.detach().cpu().numpy().copy() for k, v in pol.state_dict().items()}
        if hand_over:
            agent = PPO(pol, c.ppo.clip_param, c.ppo.epoch, c.ppo.num_mini_batch, c.ppo.value_loss_coef,
                        c.ppo.entropy_coef, lr=c.training.lr, eps=c.training.eps,
                        max_grad_norm=c.training.max_grad_norm)
            st = RolloutTrainer(c, envs, pol, agent).update()
            assert all(np.isfinite(st[k]) for k in ("value_loss", "action_loss", "dist_entropy"))
            assert sorted(pol.state_dict().keys()) == list(load("dsrnn.npz")["N%d_keys" % N])
            assert (pol.base.seq_length, pol.base.nenv, pol.base.nminibatch) == (T, E, 1)
        envs.close()
        return stats, sd

    s0, p0 = run(False)
    s1, p1 = run(True)
    for a, b in zip(s0, s1):
        for k in ("nll", "value_loss", "episodes", "took_expert", "agree", "beta"):
            assert a[k] == b[k], k
    for k in p0:
        assert p0[k].tobytes() == p1[k].tobytes(), k
    assert s0[0]["episodes"] == s0[0]["success"] + s0[0]["collision"] + s0[0]["timeout"] > 0


@pytest.mark.gpu
def test_gpu_aggregation_keeps_the_last_chunks():
    import torch

    c, envs, pol, dg = _trainer(beta=0.5, beta_decay=1.0, aggregate=3, num_mini_batch=2, epochs=1)
    labels, starts = [], []
    for i in range(4):
        starts.append(_bits(dg.rollouts.obs["robot_node"][0]))
        dg.update()
        torch.cuda.synchronize()
        labels.append(_bits(dg.labels))
        held = dg.held()
        assert len(held) == min(i + 1, 3)
        assert [_bits(s.actions) for s in held] == labels[-len(held):], i
        assert [_bits(s.obs["robot_node"][0]) for s in held] == starts[-len(held):], i
    assert len(set(labels)) == 4
    acc, n = dg.fit()
    assert n == 3 * 2
    acc, n = dg.fit(2)
    assert n == 2 * 3 * 2
    envs.close()


def _replay(envs, dg, before, expert, check):
    """Restore the state from before collect() and replay the chunk with the recorded executed actions:
    labels[t] == robot_act of the state before step t; check(t, obs) sees what step_device returned after step t."""
    import torch

    eng = envs.engine
    eng.set_state(before)
    for t in range(T):
        assert _bits(dg.labels[t]) == _bits(envs.robot_act(expert)), t
        out = envs.step_device(dg.executed[t].clone())
        torch.cuda.synchronize()
        assert _bits(dg.done[t]) == _bits(out[2]), t
        check(t, out[0])


@pytest.mark.gpu
def test_gpu_convgru_env_stores_the_live_lidar_rows():
    import torch

    from crowdnav_dsrnn_amd.learner import DAgger
    from crowdnav_dsrnn_amd.policy import Policy
    from crowdnav_dsrnn_amd.spaces import action_space, lidar_observation_space
    from tests.helpers import procedural_state_dict

    n_env = 4
    c = _config(policy="convgru", n_env=n_env)
    envs = _envs(c, n_env)
    pol = Policy(lidar_observation_space(int(c.lidar.cfg["num_beams"])), action_space(), base="convgru", base_kwargs=c)
    pol.load_state_dict(procedural_state_dict(pol))
    pol = pol.to(DEV)
    dg = DAgger(c, envs, pol, expert="orca", beta=0.5, seed=2)
    before = envs.engine.get_state()
    dg.collect()
    torch.cuda.synchronize()
    stored = dg.rollouts.obs.clone()
    assert tuple(stored.shape) == (T + 1, n_env, 1, 7 + int(c.lidar.cfg["num_beams"]))
    assert 0 < int((dg.flags & 1).sum()) < T * n_env

    def check(t, obs):
        assert _bits(stored[t + 1]) == _bits(obs), t

    _replay(envs, dg, before, "orca", check)
    assert float(stored[1:, :, :, 7:].std()) > 0
    envs.close()


@pytest.mark.gpu
def test_gpu_visible_masks_env_needs_no_scripted_opt_in():
    import torch

    from crowdnav_dsrnn_amd.learner import BehaviourCloning, DAgger
    from tests.helpers import make_policy

    n_env = 4
    c = _config(masks=True, n_env=n_env)
    assert not c.sim.visible_masks_scripted
    envs = _envs(c, n_env)
    pol = make_policy(N, E=n_env, T=T, device=DEV)
    with pytest.raises(UnsupportedConfig, match="visible_masks_scripted"):
        BehaviourCloning(c, envs, pol, expert="orca")
    dg = DAgger(c, envs, pol, expert="orca", beta=0.5, seed=2)
    before = envs.engine.get_state()
    dg.collect()
    torch.cuda.synchronize()
    stored = dg.rollouts.obs["visible_masks"].clone()
    assert tuple(stored.shape) == (T + 1, n_env, N)

    def check(t, obs):
        assert _bits(stored[t + 1]) == _bits(envs.engine.visible_mask()) == _bits(obs["visible_masks"]), t

    _replay(envs, dg, before, "orca", check)
    assert 0.0 < float(stored.mean()) < 1.0   # FOV 0.5 pi: some humans seen, some not
    envs.close()
