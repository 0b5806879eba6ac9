"""learner.BehaviourCloning with the ConvGRU policy on a live-LiDAR env: expert chunks from
ScriptedRobot.rollout(noise=) (cn_rollout_lidar) straight into a RolloutStorage, the recurrent state carried between
chunks, the cloning loss, repeatability, and the handover to RolloutTrainer -- tests/test_imitation.py's five checks.

The same sizes: 16 envs x 5 humans, chunks of 8 steps, time_limit 1.5 s at time_step 0.25 (an episode lasts at most 6
steps), so episode boundaries fall inside every chunk."""
import copy

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd.config import Config, clone_config
from tests import helpers as H

E, N, T = 16, 5, 8
DEV = "cuda:0"


def _config(live=True):
    c = clone_config(Config())
    c.robot.policy = "convgru"
    c.lidar.enable = True
    c.lidar.live = live
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


def _policy(c, device=DEV):
    from crowdnav_dsrnn_amd.policy import Policy
    from crowdnav_dsrnn_amd.spaces import action_space, lidar_observation_space

    pol = Policy(lidar_observation_space(int(c.lidar.cfg["num_beams"])), action_space(), base="convgru", base_kwargs=c)
    pol.load_state_dict(H.procedural_state_dict(pol))
    return pol.to(device)


def _trainer(sigma=0.2, seed=11, **kw):
    from crowdnav_dsrnn_amd.learner import BehaviourCloning

    c = _config()
    envs = _envs(c)
    pol = _policy(c)
    pol.train()
    return c, envs, pol, BehaviourCloning(c, envs, pol, expert="orca", sigma=sigma, seed=seed, **kw)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def test_behaviour_cloning_checks_the_convgru_pairing_before_the_gpu():
    from crowdnav_dsrnn_amd import learner
    from crowdnav_dsrnn_amd.config import UnsupportedConfig

    class Stub:
        num_envs = 8
        obs_mode = "convgru"

        def __init__(self, config):
            self.config = config

        def __getattr__(self, name):
            raise AssertionError("the check must come before the engine is touched (%s)" % name)

    class Pol:
        def __init__(self, base):
            self.srnn, self.convgru = base == "srnn", base == "convgru"

    live, parity = _config(True), _config(False)
    with pytest.raises(UnsupportedConfig, match="lidar.live"):   # the held per-episode scan cannot be recorded
        learner.BehaviourCloning(parity, Stub(parity), Pol("convgru"))
    with pytest.raises(UnsupportedConfig, match="ConvGRU"):       # the DSRNN cannot read the LiDAR row
        learner.BehaviourCloning(live, Stub(live), Pol("srnn"))
    uni = _config(True)
    uni.action_space.kinematics = "unicycle"
    with pytest.raises(UnsupportedConfig, match="holonomic"):
        learner.BehaviourCloning(uni, Stub(uni), Pol("convgru"))


@pytest.mark.gpu
def test_gpu_storage_rows_are_aligned_with_the_replayed_expert():
    """obs[t] and actions[t] are the LiDAR observation and the robot_act label of the SAME state for every t: restore
    the state from before collect() and replay the eager loop (step_device: cn_step + cn_lidar_scan) with the recorded
    executed actions."""
    from crowdnav_dsrnn_amd.learner.storage import RolloutStorage

    c, envs, pol, bc = _trainer()
    eng = envs.engine
    r = bc.rollouts
    assert isinstance(r, RolloutStorage) and r.obs.shape == (T + 1, E, 1, 187)
    before = eng.get_state()
    reset_obs = r.obs[0].clone()
    out = bc.collect()
    torch.cuda.synchronize()
    assert out["lidar"].data_ptr() == r.obs[1].data_ptr()   # recorded straight into the storage
    assert out["robot_node"].shape[0] == E                    # the SRNN observation stays a single row
    stored = r.obs.clone()
    actions, rewards, masks = r.actions.clone(), r.rewards.clone(), r.masks.clone()
    executed, done = out["executed"].clone(), out["done"].clone()
    assert done.any() and not done.all()
    assert float((executed - actions).abs().max()) > 0.05   # the steps took perturbed actions
    assert bool((stored[:, :, 0, 7:] != 0).any(-1).float().mean() > 0.5)   # live scans: the crowd is in sight
    eng.set_state(before)
    obs = reset_obs
    for t in range(T):
        assert _bits(stored[t]) == _bits(obs), t
        label = eng.robot_act("orca").clone()
        assert _bits(actions[t]) == _bits(label), t
        o, rew, dn, *_ = envs.step_device(executed[t].contiguous())
        obs = o.clone()
        assert _bits(rewards[t, :, 0]) == _bits(rew), t
        assert _bits(done[t]) == _bits(dn), t
        assert torch.equal(masks[t + 1, :, 0], 1.0 - dn.float()), t
    assert _bits(stored[T]) == _bits(obs)
    envs.close()


@pytest.mark.gpu
def test_gpu_state_carried_into_the_next_chunk():
    """The recurrent state at the start of chunk 2 == act(deterministic=True) stepped through chunk 1's observations
    and masks under the weights of before the update. The sequence forward and the per-step one run the same GRU
    kernels' arithmetic on the same float32 inputs up to the convolutions' batch shape (T * E rows against E): the
    DSRNN test's parity tolerance, 2e-5 + 1e-4 |x|."""
    c, envs, pol, bc = _trainer()
    r = bc.rollouts
    pol0 = copy.deepcopy(pol)
    obs0 = r.obs[0].clone()
    st = bc.update()
    assert st["episodes"] > 0 and np.isfinite(st["nll"]) and np.isfinite(st["value_loss"])
    hxs = torch.zeros(E, pol.base.recurrent_hidden_state_size, device=DEV)
    masks = torch.cat([torch.ones(1, E, 1, device=DEV), r.masks[1:T]])
    assert (masks == 0).any()   # an episode starts inside the chunk: the state is cleared there
    with torch.no_grad():
        for t in range(T):
            _, _, _, hxs = pol0.act(obs0 if t == 0 else r.obs[t], hxs, masks[t], deterministic=True)
    got, want = r.recurrent_hidden_states[0].cpu().numpy(), hxs.cpu().numpy()
    assert np.abs(want).max() > 1e-3
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-4)
    envs.close()


@pytest.mark.gpu
def test_gpu_cloning_lowers_the_nll_of_a_fixed_chunk():
    c, envs, pol, bc = _trainer(lr=1e-3, num_mini_batch=1, value_coef=0.0)
    bc.collect()
    nll0 = float(bc.chunk_nll())
    before = {k: p.detach().clone() for k, p in pol.named_parameters()}
    bc.fit(1)
    moved = [k for k, p in pol.named_parameters() if p.grad is not None and not torch.equal(p.detach(), before[k])]
    for k, p in pol.named_parameters():
        if p.grad is None:
            assert torch.equal(p.detach(), before[k]), k
    # value_coef = 0: the actor alone -- the convolutions, the GRU, the actor head and the distribution
    assert all(p.grad is None for k, p in pol.named_parameters() if "critic" in k)
    for part in ("base.conv_blk.conv1", "base.conv_blk.conv3", "base.gru.weight_ih", "base.gru.weight_hh",
                 "base.actor.fc1", "base.actor.fc2", "dist."):
        assert any(k.startswith(part) for k in moved), (part, moved)
    bc.fit(19)
    nll1 = float(bc.chunk_nll())
    print("nll before %.6f, after 20 passes %.6f" % (nll0, nll1))
    assert np.isfinite(nll0) and np.isfinite(nll1) and nll1 < nll0, (nll0, nll1)
    envs.close()


@pytest.mark.gpu
def test_gpu_two_trainers_from_the_same_seeds_agree_bit_for_bit():
    """With torch's deterministic convolution algorithms selected (torch.backends.cudnn.deterministic, the usual
    reproducibility switch): the library's default Conv1d forward differs by an ulp from call to call on the same
    input (measured: 4 calls, 3 shapes, max 9e-8), which no trainer on top of it can undo. Everything else -- the
    expert rollouts, the scan, the GRU, the optimiser -- is this project's and repeats bit for bit."""
    def run():
        torch.manual_seed(3)
        c, envs, pol, bc = _trainer(num_mini_batch=2, epochs=2)
        stats = [bc.update() for _ in range(3)]
        sd = {k: v.detach().cpu().numpy().copy() for k, v in pol.state_dict().items()}
        envs.close()
        return stats, sd

    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        s0, p0 = run()
        s1, p1 = run()
    finally:
        torch.backends.cudnn.deterministic = keep
    for a, b in zip(s0, s1):
        assert a["nll"] == b["nll"] and a["value_loss"] == b["value_loss"] and a["episodes"] == b["episodes"]
    for k in p0:
        assert p0[k].tobytes() == p1[k].tobytes(), k
    assert s0[0]["episodes"] == s0[0]["success"] + s0[0]["collision"] + s0[0]["timeout"]


@pytest.mark.gpu
def test_gpu_handover_to_the_ppo_trainer():
    from crowdnav_dsrnn_amd.learner import PPO
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer
    from crowdnav_dsrnn_amd.learner.storage import RolloutStorage

    c, envs, pol, bc = _trainer()
    keys = sorted(pol.state_dict().keys())
    for _ in range(2):
        bc.update()
    agent = PPO(pol, c.ppo.clip_param, c.ppo.epoch, c.ppo.num_mini_batch, c.ppo.value_loss_coef, c.ppo.entropy_coef,
                lr=c.training.lr, eps=c.training.eps, max_grad_norm=c.training.max_grad_norm)
    tr = RolloutTrainer(c, envs, pol, agent)
    assert isinstance(tr.rollouts, RolloutStorage)
    st = tr.update()
    assert all(np.isfinite(st[k]) for k in ("value_loss", "action_loss", "dist_entropy"))
    assert sorted(pol.state_dict().keys()) == keys
    envs.close()


class _Log:
    def info(self, msg):
        pass


@pytest.mark.gpu
def test_gpu_evaluate_and_evaluate_scripted_serve_the_live_convgru_env():
    """tools/imitation_pretrain.py --policy convgru prints three kinds of row: the expert's (evaluate_scripted) and
    the policies' (evaluate). The expert acts on the full state, so its records on the 'convgru' env equal those on
    an 'srnn' env of the same config; evaluate() runs the ConvGRU policy on the LiDAR rows."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.evaluation import evaluate, evaluate_scripted

    EE = 8
    keys = ("success_rate", "collision_rate", "timeout_rate")

    def envs_of(c):
        c.env.test_size = 2 * EE
        return c, CrowdNavVecEnv(c, EE, c.env.seed, DEV, allow_early_resets=True, nenv=EE, phase="test")

    rows = []
    for policy in ("convgru", "srnn"):
        c = _config()
        c.robot.policy = policy
        c, envs = envs_of(c)
        evaluate_scripted("orca", envs, EE, DEV, c, _Log(), keep_traces=False, verbose=False)
        rows.append({k: evaluate.last[k] for k in keys})
        envs.close()
    assert rows[0] == rows[1], rows
    assert abs(sum(rows[0].values()) - 1.0) < 1e-9
    c, envs = envs_of(_config())
    pol = _policy(c).eval()
    evaluate(pol, None, envs, EE, DEV, c, _Log(), keep_traces=False, verbose=False)
    assert abs(sum(evaluate.last[k] for k in keys) - 1.0) < 1e-9
    envs.close()
