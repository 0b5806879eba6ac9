"""The lattice action head on the GPU: cn_lattice_act and cn_lattice_eval_fwd / _bwd against the float64 statement of
include/crowdnav.h's definition (tests/lattice_ref.py, where the tolerances are derived), Policy.act against the torch
restatement on the same generator state, and the head inside RolloutTrainer (HIP-graph rollout) and
BehaviourCloning(expert='dwa')."""
import math

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd import _lib, ops
from crowdnav_dsrnn_amd.config import Config, clone_config
from tests import lattice_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _act(logits, u, choice=True):
    """cn_lattice_act itself (ops.lattice_act draws its own u): -> action, logp, choice as numpy."""
    E = logits.shape[0]
    lt = torch.from_numpy(logits).to(DEV)
    ut = torch.from_numpy(u).to(DEV) if u is not None else None
    action = torch.full((E, 2), float("nan"), device=DEV)
    logp = torch.full((E,), float("nan"), device=DEV)
    ch = torch.full((E,), -1, dtype=torch.int32, device=DEV) if choice else None
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().cn_lattice_act(ops._stream(torch.device(DEV)), E, lt.data_ptr(),
                                             ut.data_ptr() if ut is not None else None, action.data_ptr(),
                                             logp.data_ptr(), ch.data_ptr() if ch is not None else None))
    torch.cuda.synchronize()
    return action.cpu().numpy(), logp.cpu().numpy(), ch.cpu().numpy() if ch is not None else None


# E = 257: a partial last workgroup (4 rows each); the starts put every kind of row into the small cases
@pytest.mark.parametrize("E,start", [(1, 4), (3, 0), (5, 3), (257, 0)])
def test_act_kernel_vs_float64(E, start):
    logits, u = ref.rows(E, start), ref.draws(E)
    s = ref.softmax(logits)
    r = np.arange(E)
    # mode: exact
    action, logp, c = _act(logits, None)
    want = ref.mode(logits)
    assert np.array_equal(c, want)
    assert np.array_equal(action, ref.ACTIONS32[want])
    lp = s["logp"][r, want]
    assert (np.abs(logp - lp) <= ref.logp_tol(lp)).all(), np.abs(logp - lp).max()
    # sample: the interval rule, p_c > 0, the action the lattice point of c bit for bit
    action, logp, c = _act(logits, u)
    assert not ref.sample_errors(logits, u, c)
    assert np.array_equal(action, ref.ACTIONS32[c])
    lp = s["logp"][r, c]
    assert (np.abs(logp - lp) <= ref.logp_tol(lp)).all(), np.abs(logp - lp).max()
    # choice = NULL: the same action and log-probability
    a2, lp2, _ = _act(logits, u, choice=False)
    assert np.array_equal(a2, action) and np.array_equal(lp2, logp)


def test_act_kernel_draws_every_likely_candidate_at_its_rate():
    """One fixed row, 65536 draws: every candidate of probability >= 1/64 within 5 binomial standard deviations of
    E q_c; no candidate of float32 probability zero at all."""
    E = 65536
    row = (1.5 * np.random.RandomState(21).standard_normal(64)).astype(np.float32)
    row[50:] = -150.0   # (p = 0 in float32)
    logits = np.repeat(row[None], E, 0)
    u = np.minimum(np.random.RandomState(22).random_sample(E).astype(np.float32), ref.U_MAX)
    _, _, c = _act(logits, u)
    counts = np.bincount(c, minlength=64)
    q = ref.softmax(row[None])["q"][0]
    likely = q >= 1 / 64
    assert likely.sum() >= 10
    sd = np.sqrt(E * q * (1 - q))
    assert (np.abs(counts - E * q)[likely] <= 5 * sd[likely]).all(), (counts[likely], (E * q)[likely])
    assert counts[50:].sum() == 0 and counts.sum() == E


@pytest.mark.parametrize("B,start", [(1, 4), (5, 2), (257, 0)])
def test_evaluate_kernels_vs_float64_autograd(B, start):
    """ops.lattice_evaluate (cn_lattice_eval_fwd / _bwd) against float64 log_softmax autograd, with non-unit upstream
    gradients; rows of kind 4 hold underflowed candidates: the gradient is finite, and exactly 0 where q_j == 0 and
    the candidate is not the action's."""
    logits, actions = ref.rows(B, start), ref.eval_actions(B)
    rs = np.random.RandomState(5)
    g_lp, g_H = rs.uniform(-2, 2, B), rs.uniform(-2, 2, B)
    lt = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    logp, ent = ops.lattice_evaluate(lt, torch.from_numpy(actions).to(DEV))
    assert logp.shape == (B, 1) and ent.shape == (B,)
    (logp[:, 0] * torch.from_numpy(g_lp).float().to(DEV)).sum().add(
        (ent * torch.from_numpy(g_H).float().to(DEV)).sum()).backward()
    got = lt.grad.cpu().numpy()
    # float64 autograd of the definition
    l64 = torch.from_numpy(logits).double().requires_grad_(True)
    lsm = torch.log_softmax(l64, -1)
    idx = torch.from_numpy(ref.index(actions))
    lp64 = lsm.gather(1, idx[:, None])[:, 0]
    H64 = -(lsm.exp() * lsm).sum(-1)
    ((lp64 * torch.from_numpy(g_lp)).sum() + (H64 * torch.from_numpy(g_H)).sum()).backward()
    want = l64.grad.numpy()
    lp64, H64 = lp64.detach().numpy(), H64.detach().numpy()
    assert (np.abs(logp.detach().cpu().numpy()[:, 0] - lp64) <= ref.logp_tol(lp64)).all()
    assert (np.abs(ent.detach().cpu().numpy() - H64) <= ref.logp_tol(H64)).all()
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= ref.logp_tol(want)).all(), np.abs(got - want).max()
    dead = ref.softmax(logits)["d"] < -110.0          # q_j == 0 in float32, whatever the device's denormal handling
    dead[np.arange(B), idx.numpy()] = False
    kinds = (start + np.arange(B)) % ref.KINDS
    assert (dead[kinds == 4].sum(1) >= 19).all() and (got[dead] == 0).all()   # (20 per row, less the action's own)


def _unicycle_config(N=5, E=8, T=4):
    c = clone_config(Config())
    c.sim.human_num = N
    c.humans.policy = "orca"
    c.action_space.kinematics = "unicycle"
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.robot.action_head = "lattice"
    c.training.num_processes = E
    c.ppo.num_steps, c.ppo.num_mini_batch, c.ppo.epoch = T, 1, 1
    return c


def _lattice_policy(c, envs, seed=3, gain=None):
    from crowdnav_dsrnn_amd.policy import Policy

    torch.manual_seed(seed)
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=c)
    assert pol.head == "lattice"
    if gain:   # logits far from uniform, so that a wrong index or a wrong draw shows
        with torch.no_grad():
            pol.dist.fc_logits.weight.mul_(gain)
    return pol.to(DEV)


def test_policy_act_equals_the_restatement_on_the_same_generator_state():
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    E = 37
    c = _unicycle_config(E=E)
    envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, nenv=E, phase="train")
    pol = _lattice_policy(c, envs, gain=300.0).eval()
    obs = envs.reset()
    hxs = {"human_node_rnn": torch.zeros(E, 1, c.SRNN.human_node_rnn_size, device=DEV),
           "human_human_edge_rnn": torch.zeros(E, c.sim.human_num + 1, c.SRNN.human_human_edge_rnn_size, device=DEV)}
    masks = torch.ones(E, 1, device=DEV)
    with torch.no_grad():
        _, feats, _ = pol._infer(obs, dict(hxs), masks)
        logits = pol.dist.fc_logits(feats)
        assert float(logits.max() - logits.min()) > 1.0
        torch.manual_seed(77)
        u = torch.rand((E,), dtype=torch.float32, device=DEV)
        torch.manual_seed(77)
        value, action, logp, _ = pol.act(obs, dict(hxs), masks)
        a_t, lp_t, c_t = ops.lattice_act_torch(logits, u)
        mode = pol.act(obs, dict(hxs), masks, deterministic=True)
    assert tuple(action.shape) == (E, 2) and tuple(logp.shape) == (E, 1) and action.dtype == torch.float32
    got_c = ops.lattice_index(action).cpu().numpy()
    l, un = logits.cpu().numpy(), u.cpu().numpy()
    assert np.array_equal(action.cpu().numpy(), ref.ACTIONS32[got_c])
    assert not ref.sample_errors(l, un, got_c)                       # the kernel's draw
    assert not ref.sample_errors(l, un, c_t.cpu().numpy())           # the restatement's, on the same u
    same = got_c == c_t.cpu().numpy()
    assert same.mean() > 0.9                                         # (they part only within rounding of a sum)
    lp64 = ref.softmax(l)["logp"][np.arange(E), got_c]
    assert (np.abs(logp.cpu().numpy()[:, 0] - lp64) <= ref.logp_tol(lp64)).all()
    assert (np.abs(lp_t.cpu().numpy()[same, 0] - lp64[same]) <= ref.logp_tol(lp64[same])).all()
    assert np.array_equal(ops.lattice_index(mode[1]).cpu().numpy(), ref.mode(l))
    envs.close()


def test_rollout_trainer_runs_the_lattice_head_in_its_hip_graph():
    """8 unicycle envs x 5 humans x 4 steps: the captured rollout equals the eager one bit for bit (mode actions; the
    PPO updates in between change the weights), its graph holds no memset node and stays on, the sampled rollout
    captures as well, and a PPO update leaves finite parameters."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import PPO
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer

    E, T = 8, 4

    def run(graphs, deterministic):
        c = _unicycle_config(E=E, T=T)
        envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, nenv=E, phase="train")
        pol = _lattice_policy(c, envs, gain=100.0)
        agent = PPO(pol, c.ppo.clip_param, 1, 1, c.ppo.value_loss_coef, c.ppo.entropy_coef, lr=1e-3,
                    eps=c.training.eps, max_grad_norm=c.training.max_grad_norm)
        tr = RolloutTrainer(c, envs, pol, agent, deterministic=deterministic, graphs=graphs)
        out = []
        for _ in range(3):
            tr.update()
            r = tr.rollouts
            out.append((r.actions.cpu().numpy().copy(), r.action_log_probs.cpu().numpy().copy(),
                        r.rewards.cpu().numpy().copy(), r.value_preds.cpu().numpy().copy()))
        finite = all(bool(torch.isfinite(p).all()) for p in pol.parameters())
        envs.close()
        return out, tr, finite

    eager, tr0, fin0 = run(False, True)
    graph, tr1, fin1 = run(True, True)
    assert tr0._graph is None and tr1._graph is not None and tr1.graphs
    assert tr1.graph_audit is not None and not tr1.graph_audit.get("memset"), tr1.graph_audit
    assert fin0 and fin1
    for u, (a, b) in enumerate(zip(eager, graph)):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y, err_msg="update %d" % u)
        lab = a[0].reshape(-1, 2)
        assert np.array_equal(lab, ref.ACTIONS32[ref.index(lab)])       # lattice points, bit for bit
        assert np.isfinite(a[1]).all() and (a[1] < 0).all()
    sampled, tr2, fin2 = run(True, False)
    assert tr2._graph is not None and tr2.graphs and not tr2.graph_audit.get("memset"), tr2.graph_audit
    assert fin2
    for a in sampled:
        lab = a[0].reshape(-1, 2)
        assert np.array_equal(lab, ref.ACTIONS32[ref.index(lab)])
    assert len({tuple(r) for a in sampled for r in a[0].reshape(-1, 2).tolist()}) > 4   # (it does sample)


def test_behaviour_cloning_of_the_dwa_expert_into_the_lattice_head():
    """16 unicycle envs x 5 humans x 8 steps: every stored label is a lattice point bit for bit and its index is the
    candidate the head scores; the chunk's NLL starts within 0.05 of log 64 and falls over 20 fit passes."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import BehaviourCloning

    E, N, T = 16, 5, 8
    c = _unicycle_config(N, E, T)
    c.robot.scripted_dwa = True
    envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
    pol = _lattice_policy(c, envs)
    pol.train()
    bc = BehaviourCloning(c, envs, pol, expert="dwa", sigma=0.03, seed=11, lr=1e-3, num_mini_batch=1, value_coef=0.5)
    bc.collect()
    lab = bc.rollouts.actions.reshape(T * E, 2)
    idx = ops.lattice_index(lab)
    assert torch.equal(lab, ops.lattice_actions(DEV)[idx])
    assert np.array_equal(idx.cpu().numpy(), ref.index(lab.cpu().numpy()))
    bc.rollouts.compute_returns(torch.zeros(E, 1, device=DEV), False, c.reward.gamma, c.ppo.gae_lambda,
                                c.training.use_proper_time_limits)
    first = float(bc.chunk_nll())
    assert abs(first - math.log(64)) <= 0.05, first
    for _ in range(20):
        acc, n = bc.fit(1)
    last = float(bc.chunk_nll())
    assert math.isfinite(last) and last < first, (first, last)
    envs.close()
