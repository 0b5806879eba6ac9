"""learner.BehaviourCloning: expert chunks from ScriptedRobot.rollout(noise=) into an SRNNRolloutStorage, the
recurrent state carried between chunks, the cloning loss, repeatability, and the handover to RolloutTrainer.

16 envs x 5 humans, chunks of 8 steps, time_limit 1.5 s at time_step 0.25 (an episode lasts at most 6 steps), so
episode boundaries fall inside every chunk."""
import copy

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd.config import Config, clone_config
from tests.helpers import load, make_policy

E, N, T = 16, 5, 8
DEV = "cuda:0"
OBS = ("robot_node", "temporal_edges", "spatial_edges")


def _config():
    c = clone_config(Config())
    c.sim.human_num = N
    c.humans.policy = "orca"
    c.action_space.kinematics = "holonomic"
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.env.time_limit = 1.5
    c.env.time_step = 0.25
    c.training.num_processes = E
    c.ppo.num_steps = T
    c.ppo.num_mini_batch = 1
    c.ppo.epoch = 2
    return c


def _envs(c):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    return CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")


def _trainer(sigma=0.2, seed=11, **kw):
    from crowdnav_dsrnn_amd.learner import BehaviourCloning

    c = _config()
    envs = _envs(c)
    pol = make_policy(N, E=E, T=T, device=DEV)
    pol.train()
    return c, envs, pol, BehaviourCloning(c, envs, pol, expert="orca", sigma=sigma, seed=seed, **kw)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def test_behaviour_cloning_is_exported_and_checks_before_the_gpu():
    from crowdnav_dsrnn_amd import learner
    from crowdnav_dsrnn_amd.config import UnsupportedConfig

    assert hasattr(learner, "BehaviourCloning")

    class Stub:
        num_envs = 8
        obs_mode = "srnn"

        def __init__(self, config):
            self.config = config

        def __getattr__(self, name):
            raise AssertionError("the check must come before the engine is touched (%s)" % name)

    uni = _config()
    uni.action_space.kinematics = "unicycle"
    with pytest.raises(UnsupportedConfig):
        learner.BehaviourCloning(uni, Stub(uni), None)
    with pytest.raises(UnsupportedConfig):
        learner.BehaviourCloning(_config(), Stub(_config()), None, expert="cadrl")


@pytest.mark.gpu
def test_gpu_storage_rows_are_aligned_with_the_replayed_expert():
    """obs[t] and actions[t] are the observation and the robot_act label of the SAME state for every t: restore the
    state from before collect() and replay the eager loop with the recorded executed actions."""
    c, envs, pol, bc = _trainer()
    eng = envs.engine
    before = eng.get_state()
    reset_obs = {k: eng.obs()[k].clone() for k in OBS}
    out = bc.collect()
    r = bc.rollouts
    torch.cuda.synchronize()
    stored_obs = {k: r.obs[k].clone() for k in OBS}
    actions, rewards, masks = r.actions.clone(), r.rewards.clone(), r.masks.clone()
    executed, done = out["executed"].clone(), out["done"].clone()
    assert done.any() and not done.all()
    assert float((executed - actions).abs().max()) > 0.05   # the steps took perturbed actions
    eng.set_state(before)
    obs = reset_obs
    for t in range(T):
        for k in OBS:
            assert _bits(stored_obs[k][t]) == _bits(obs[k]), (k, t)
        label = eng.robot_act("orca").clone()
        assert _bits(actions[t]) == _bits(label), t
        o, rew, dn, _, _, _, _ = eng.step(executed[t].contiguous())
        obs = {k: o[k].clone() for k in OBS}
        assert _bits(rewards[t, :, 0]) == _bits(rew), t
        assert _bits(done[t]) == _bits(dn), t
        assert torch.equal(masks[t + 1, :, 0], 1.0 - dn.float()), t
    for k in OBS:
        assert _bits(stored_obs[k][T]) == _bits(obs[k]), k
    envs.close()


@pytest.mark.gpu
def test_gpu_state_carried_into_the_next_chunk():
    """The recurrent state at the start of chunk 2 == act(deterministic=True) stepped through chunk 1's observations
    and masks under the weights of before the update. DSRNN parity tolerance: 2e-5 + 1e-4 |x|."""
    c, envs, pol, bc = _trainer()
    r = bc.rollouts
    pol0 = copy.deepcopy(pol)
    obs0 = {k: r.obs[k][0].clone() for k in OBS}
    st = bc.update()
    assert st["episodes"] > 0 and np.isfinite(st["nll"]) and np.isfinite(st["value_loss"])
    hxs = {"human_node_rnn": torch.zeros(E, 1, c.SRNN.human_node_rnn_size, device=DEV),
           "human_human_edge_rnn": torch.zeros(E, N + 1, c.SRNN.human_human_edge_rnn_size, device=DEV)}
    masks = torch.cat([torch.ones(1, E, 1, device=DEV), r.masks[1:T]])
    assert (masks == 0).any()   # an episode starts inside the chunk: the state is cleared there
    with torch.no_grad():
        for t in range(T):
            o = obs0 if t == 0 else {k: r.obs[k][t] for k in OBS}
            _, _, _, hxs = pol0.act(o, hxs, masks[t], deterministic=True)
    for k in hxs:
        got, want = r.recurrent_hidden_states[k][0].cpu().numpy(), hxs[k].cpu().numpy().reshape(
            r.recurrent_hidden_states[k][0].shape)
        assert np.abs(want).max() > 1e-3
        np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-4, err_msg=k)
    envs.close()


@pytest.mark.gpu
def test_gpu_cloning_lowers_the_nll_of_a_fixed_chunk():
    c, envs, pol, bc = _trainer(lr=1e-3, num_mini_batch=1, value_coef=0.0)
    bc.collect()
    nll0 = float(bc.chunk_nll())
    before = {k: p.detach().clone() for k, p in pol.named_parameters()}
    bc.fit(1)
    # "Receives a gradient" in float32 terms: Adam's first step of an element is lr * g / (|g| + eps) (p.grad is the
    # clipped gradient the optimiser saw), and it shows in the parameter when it exceeds the element's spacing,
    # 2^-23 |p| at most; twice that spacing is demanded here. (The bias of attn.spatial_edge_layer shifts every
    # human's score alike, which the softmax ignores: its gradient is rounding noise of ~1e-10 and moves nothing.)
    lr, eps = 1e-3, float(c.training.eps)
    moved, still = 0, []
    for k, p in pol.named_parameters():
        if p.grad is None:
            assert torch.equal(p.detach(), before[k]), k
            continue
        g = p.grad.abs()
        must = lr * g / (g + eps) > 2.0 ** -22 * before[k].abs().clamp_min(1e-30)
        assert bool((p.detach() != before[k])[must].all()), k
        if bool(must.any()):
            moved += 1
        else:
            still.append(k)
    print("parameters moved: %d; with a gradient below float32 spacing: %s" % (moved, still))
    assert moved >= 20 and len(still) <= 1, (moved, still)
    assert any(k.startswith("dist.") for k, p in pol.named_parameters() if p.grad is not None)
    assert all(p.grad is None for k, p in pol.named_parameters() if "critic" in k)   # value_coef = 0: the actor alone
    bc.fit(19)
    nll1 = float(bc.chunk_nll())
    print("nll before %.6f, after 20 passes %.6f" % (nll0, nll1))
    assert np.isfinite(nll0) and np.isfinite(nll1) and nll1 < nll0, (nll0, nll1)
    envs.close()


@pytest.mark.gpu
def test_gpu_two_trainers_from_the_same_seeds_agree_bit_for_bit():
    def run():
        torch.manual_seed(3)
        c, envs, pol, bc = _trainer(num_mini_batch=2, epochs=2)
        stats = [bc.update() for _ in range(3)]
        sd = {k: v.detach().cpu().numpy().copy() for k, v in pol.state_dict().items()}
        envs.close()
        return stats, sd

    s0, p0 = run()
    s1, p1 = run()
    for a, b in zip(s0, s1):
        assert a["nll"] == b["nll"] and a["value_loss"] == b["value_loss"] and a["episodes"] == b["episodes"]
    for k in p0:
        assert p0[k].tobytes() == p1[k].tobytes(), k
    assert s0[0]["episodes"] == s0[0]["success"] + s0[0]["collision"] + s0[0]["timeout"]


@pytest.mark.gpu
def test_gpu_handover_to_the_ppo_trainer():
    from crowdnav_dsrnn_amd.learner import PPO
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer

    c, envs, pol, bc = _trainer()
    for _ in range(2):
        bc.update()
    agent = PPO(pol, c.ppo.clip_param, c.ppo.epoch, c.ppo.num_mini_batch, c.ppo.value_loss_coef, c.ppo.entropy_coef,
                lr=c.training.lr, eps=c.training.eps, max_grad_norm=c.training.max_grad_norm)
    tr = RolloutTrainer(c, envs, pol, agent)
    st = tr.update()
    assert all(np.isfinite(st[k]) for k in ("value_loss", "action_loss", "dist_entropy"))
    assert sorted(pol.state_dict().keys()) == list(load("dsrnn.npz")["N%d_keys" % N])
    assert (pol.base.seq_length, pol.base.nenv, pol.base.nminibatch) == (T, E, 1)
    envs.close()


@pytest.mark.gpu
def test_gpu_sigma_zero_gives_the_clean_rollout():
    from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot

    c, envs, pol, bc = _trainer(sigma=0.0)
    out = bc.collect()
    r = bc.rollouts
    c2 = _config()
    envs2 = _envs(c2)
    envs2.reset()
    ref = ScriptedRobot(envs2, "orca").rollout(T)
    torch.cuda.synchronize()
    for k in OBS:
        assert _bits(r.obs[k][1:]) == _bits(ref[k]), k
    assert _bits(r.actions) == _bits(ref["actions"]) == _bits(out["executed"])
    assert _bits(r.rewards[..., 0]) == _bits(ref["reward"])
    assert _bits(out["done"]) == _bits(ref["done"]) and _bits(out["event"]) == _bits(ref["event"])
    assert torch.equal(r.masks[1:, :, 0], 1.0 - ref["done"].float())
    envs.close()
    envs2.close()
