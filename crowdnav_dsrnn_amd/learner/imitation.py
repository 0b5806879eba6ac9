"""Device-resident behaviour cloning of a scripted robot (ORCA / social force) into the DSRNN policy, or into the
ConvGRU policy on a live-LiDAR env (robot.policy 'convgru' with lidar.live).

    bc = BehaviourCloning(config, envs, actor_critic, expert="orca", sigma=0.1)
    stats = bc.update()      # one expert chunk of num_steps steps of every env + `epochs` passes over it
    ...
    trainer = RolloutTrainer(config, envs, actor_critic, agent)   # the same policy continues with PPO

The expert drives the envs in whole rollouts (ScriptedRobot.rollout -> cn_rollout_noisy: the multi-step launches with
the controller inside, no learner in the loop, no launch per step from Python) that record straight into an
SRNNRolloutStorage. With sigma > 0 the executed action is the expert's plus uniform noise while the recorded label
stays the clean expert action (noise injection in the style of DART, Laskey et al. 2017): the learner sees the states
a perturbed policy reaches, labelled with what the expert does there. The loss is the negative log-likelihood of the
label under the policy's Gaussian plus, optionally, a value regression onto the expert's discounted returns, over
the minibatches PPO.update walks (env subsets, whole sequences, the recurrent state of the chunk's start).

The ConvGRU policy sees 180 ranges where the expert sees every human's state. Its chunks come from the same rollout
with the LiDAR rows recorded as well (cn_rollout_lidar) straight into a RolloutStorage; labels, noise, masks, returns,
the carried recurrent state, fit() and update() are the DSRNN branch's.

An env of varying human count (config.sim.human_nums with sim.human_nums_scripted; the DSRNN policy built for the
largest count): the rollout runs
on the mixed engine and records the padded observation into the same storage tensors; the storage's
'detected_human_num' rows, constant over the env's life, are filled once, and the policy reads them as under PPO (the
attention of ops.spatial_attention_var).

An env with config.sim.visible_masks and sim.visible_masks_scripted: the rollout records 'visible_masks' into the
storage as well (cn_rollout_masked, row 0 from reset()), and the DSRNN policy attends to the visible humans only, as
under PPO (ops.spatial_attention_mask). Without the second opt-in: UnsupportedConfig.

A unicycle env (action_space.kinematics 'unicycle' with the opt-in config.robot.scripted_unicycle): the expert's
velocity goes through the tracking law on the device (policy_factory.unicycle_track) and the labels are the unicycle
actions (dv, dtheta), each within [-0.1, 0.1]. `sigma` is then in those action units -- 0.1 is the whole range, so
0.03 there is a large perturbation -- and the step clips the perturbed action. expert='dwa' (the opt-in
config.robot.scripted_dwa) is the expert made for that robot: a dynamic-window controller whose labels are grid points
of the unicycle action space (policy_factory.dwa_predict), with sigma in the same units.

The action head: the loss goes through evaluate_actions, so "the policy's Gaussian" above is whatever head the policy
has. With the lattice head (config.robot.action_head = 'lattice', unicycle envs) the NLL is the cross-entropy of a
64-way classification: a 'dwa' label is one of the head's candidates and is scored at its own index, exactly; a
continuous label (ORCA or the social force through the tracking law) is scored at its nearest lattice point. Nothing
else in this trainer depends on the head.
"""
import contextlib
import time

import torch
import torch.nn as nn
import torch.optim as optim

from ..engine import RolloutNoise
from .storage import RolloutStorage, SRNNRolloutStorage

EVENT_COLLISION, EVENT_SUCCESS, EVENT_TIMEOUT = 2, 3, 4   # cn_step's event codes of an episode's end


class BehaviourCloning:
    def __init__(self, config, envs, actor_critic, expert="orca", sigma=0.0, seed=0, num_steps=None,
                 num_mini_batch=None, epochs=1, lr=None, value_coef=0.5):
        from ..config import UnsupportedConfig, no_visible_masks
        from ..policy_factory import ScriptedRobot

        ScriptedRobot.check(envs, expert)   # unknown controller / unicycle without its opt-in: before anything touches the GPU
        # sim.visible_masks: only with sim.visible_masks_scripted, where the rollout records 'visible_masks' as well
        masked = no_visible_masks(envs.config, "BehaviourCloning")
        mode = getattr(envs, "obs_mode", "srnn")
        self.convgru = mode == "convgru"
        if self.convgru:
            lc = config.lidar
            if not getattr(actor_critic, "convgru", False) or not (getattr(lc, "live", False) and lc.enable):
                raise UnsupportedConfig("BehaviourCloning: a 'convgru' env needs the ConvGRU policy (base='convgru') "
                                        "and config.lidar.live (the rollout records the live scan only)")
        elif mode != "srnn" or not getattr(actor_critic, "srnn", False):
            raise UnsupportedConfig("BehaviourCloning: the DSRNN policy (base='srnn') on the 'srnn' observation, or the "
                                    "ConvGRU policy (base='convgru') on a live 'convgru' one")
        self.config = config
        self.envs = envs
        self.ac = actor_critic
        self.robot = ScriptedRobot(envs, expert)
        self.noise = RolloutNoise(sigma, seed, 0)   # step0 advances by num_steps per chunk
        self.num_steps = int(config.ppo.num_steps if num_steps is None else num_steps)
        self.num_mini_batch = int(config.ppo.num_mini_batch if num_mini_batch is None else num_mini_batch)
        self.epochs = int(epochs)
        self.value_coef = float(value_coef)
        self.max_grad_norm = config.training.max_grad_norm
        E = envs.num_envs
        if self.num_steps < 1 or self.epochs < 1 or not 1 <= self.num_mini_batch <= E or E % self.num_mini_batch:
            raise ValueError("BehaviourCloning: num_steps >= 1, epochs >= 1 and a num_mini_batch that divides the %d "
                             "envs required" % E)
        self.optimizer = optim.Adam(actor_critic.parameters(), lr=config.training.lr if lr is None else lr,
                                    eps=config.training.eps)
        dev = envs.engine.device
        self.device = dev
        if self.convgru:
            self.rollouts = RolloutStorage(self.num_steps, E, envs.observation_space.shape, envs.action_space,
                                           actor_critic.base.recurrent_hidden_state_size, device=dev,
                                           compact_hidden=True)
        else:
            self.rollouts = SRNNRolloutStorage(self.num_steps, E, envs.observation_space.spaces, envs.action_space,
                                               config.SRNN.human_node_rnn_size, config.SRNN.human_human_edge_rnn_size,
                                               "GRU", device=dev, compact_hidden=True)
        r, T = self.rollouts, self.num_steps
        # the rollout records into the storage itself: rows t of the observation are obs[t + 1], the labels the
        # actions, the rewards the rewards; done / event / executed are the trainer's own
        if self.convgru:
            # obs[1:] is contiguous: the scan of all T * E rows lands there. The SRNN observation is not read: the
            # engine's own single-row buffers take the last step's (obs_every_step=False); the state rows are the
            # rollout's workspace
            N = int(config.sim.human_num)
            self._buf = dict(envs.engine.obs())
            self._buf["lidar"] = r.obs[1:]
            self._buf["robot_state"] = torch.zeros((9, T, E), dtype=torch.float64, device=dev)
            self._buf["human_state"] = torch.zeros((3, T, E, N), dtype=torch.float64, device=dev)
        else:
            self._buf = {k: r.obs[k][1:] for k in ("robot_node", "temporal_edges", "spatial_edges")}
            if masked:   # (cn_rollout_masked writes the rows; SRNN.forward reads the key as under PPO)
                self._buf["visible_masks"] = r.obs["visible_masks"][1:]
        self._buf["actions"] = r.actions
        self._buf["reward"] = r.rewards.view(T, E)
        self._buf["done"] = torch.zeros((T, E), dtype=torch.uint8, device=dev)
        self._buf["event"] = torch.zeros((T, E), dtype=torch.int8, device=dev)
        self._buf["executed"] = torch.zeros((T, E, 2), dtype=torch.float32, device=dev)
        self.last = None          # the dict of the last chunk's rollout (executed, done, event, num_launches)
        self.env_steps = 0
        self.chunks = 0
        obs = envs.reset()
        if self.convgru:
            r.obs[0].copy_(obs)
        else:
            for k in r.obs:
                r.obs[k][0].copy_(obs[k])
            if "detected_human_num" in r.obs:   # no rollout row rewrites it: every slot, once
                r.obs["detected_human_num"].copy_(obs["detected_human_num"].unsqueeze(0).expand_as(
                    r.obs["detected_human_num"]))

    def _obs(self, fn):
        """fn over the storage's observation: the DSRNN's dict of tensors or the ConvGRU's one tensor."""
        o = self.rollouts.obs
        return {k: fn(v) for k, v in o.items()} if isinstance(o, dict) else fn(o)

    def _hxs(self, fn):
        h = self.rollouts.recurrent_hidden_states
        return {k: fn(v) for k, v in h.items()} if isinstance(h, dict) else fn(h)

    @contextlib.contextmanager
    def _sequence_shape(self, B):
        """SRNN.forward reads the sequence length and the envs per minibatch from its own attributes (the reference's
        seq_length / nenv / nminibatch): set them for this trainer's chunk, put PPO's back afterwards. (ConvGRU
        reads both from its arguments' shapes.)"""
        if self.convgru:
            yield
            return
        b = self.ac.base
        keep = (b.seq_length, b.nenv, b.nminibatch)
        b.seq_length, b.nenv, b.nminibatch = self.num_steps, B, 1
        try:
            yield
        finally:
            b.seq_length, b.nenv, b.nminibatch = keep

    @torch.no_grad()
    def collect(self):
        """One expert chunk into the storage: obs[t + 1] = rollout row t (obs[0]: the previous chunk's last, or the
        reset observation), actions[t] = the clean label of row t, rewards[t], masks[t + 1] = 1 - done[t]. One
        ScriptedRobot.rollout call; no host synchronisation."""
        r, T = self.rollouts, self.num_steps
        noise = RolloutNoise(self.noise.sigma, self.noise.seed, self.noise.step0 + self.chunks * T)
        self.last = self.robot.rollout(T, obs_every_step=not self.convgru, out=self._buf, noise=noise)
        r.masks[1:].copy_(torch.rsub(self._buf["done"].unsqueeze(-1), 1.0))   # 1 - done as float32
        self.chunks += 1
        self.env_steps += T * self.envs.num_envs
        return self.last

    @torch.no_grad()
    def _advance_state(self):
        """The recurrent state at the end of the chunk from the one at its start, under the current weights: a
        sequence forward of obs[0..T-1] with masks[0..T-1] (a zero mask clears the state where an episode starts),
        in the env groups of the minibatches; into the storage's latest-state slot, which after_update() carries to
        the next chunk's start -- what a PPO rollout leaves there."""
        r, T, E = self.rollouts, self.num_steps, self.envs.num_envs
        B = E // self.num_mini_batch
        with self._sequence_shape(B):
            for s in range(0, E, B):
                obs = self._obs(lambda v: v[:-1, s:s + B].reshape(T * B, *v.shape[2:]))
                hxs = self._hxs(lambda v: v[0][s:s + B])
                _, _, out = self.ac.base(obs, hxs, r.masks[:-1, s:s + B].reshape(T * B, 1))
                if self.convgru:
                    r.recurrent_hidden_states[-1][s:s + B].copy_(out)
                    continue
                for k, v in r.recurrent_hidden_states.items():
                    v[-1][s:s + B].copy_(out[k].reshape(v[-1][s:s + B].shape))

    def _losses(self, obs_b, hxs_b, masks_b, actions_b, return_b):
        values, logp, _, _ = self.ac.evaluate_actions(obs_b, hxs_b, masks_b, actions_b)
        nll = -logp.mean()
        value_loss = 0.5 * (values - return_b).pow(2).mean()
        return nll, value_loss

    @torch.no_grad()
    def chunk_nll(self):
        """The stored chunk's mean negative log-likelihood under the current weights (device scalar)."""
        r, T, E = self.rollouts, self.num_steps, self.envs.num_envs
        with self._sequence_shape(E):
            obs = self._obs(lambda v: v[:-1].reshape(T * E, *v.shape[2:]))
            hxs = self._hxs(lambda v: v[0])
            return self._losses(obs, hxs, r.masks[:-1].reshape(T * E, 1), r.actions.reshape(T * E, -1),
                                r.returns[:-1].reshape(T * E, 1))[0]

    def fit(self, epochs=None):
        """`epochs` passes over the stored chunk (recurrent_generator's minibatches): device tensor
        [sum of nll, sum of value_loss] over the minibatches, and their number."""
        r = self.rollouts
        acc, n = torch.zeros(2, dtype=torch.float64, device=self.device), 0
        B = self.envs.num_envs // self.num_mini_batch
        with self._sequence_shape(B):
            for _ in range(self.epochs if epochs is None else int(epochs)):
                for obs_b, hxs_b, actions_b, _, return_b, masks_b, _, _ in r.recurrent_generator(r.returns[:-1],
                                                                                               self.num_mini_batch):
                    nll, value_loss = self._losses(obs_b, hxs_b, masks_b, actions_b, return_b)
                    self.optimizer.zero_grad()
                    (nll + self.value_coef * value_loss if self.value_coef else nll).backward()
                    nn.utils.clip_grad_norm_(self.ac.parameters(), self.max_grad_norm)
                    self.optimizer.step()
                    acc += torch.stack([nll.detach(), value_loss.detach()]).double()
                    n += 1
        return acc, n

    def update(self):
        """One expert chunk + `epochs` passes over it. rollout_s / update_s are GPU time between HIP events on the
        current stream (RolloutTrainer.update's convention); one host synchronisation, at the end."""
        c = self.config
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.device.type == "cuda" else None
        t0 = time.perf_counter()
        if ev:
            ev[0].record()
        self.collect()
        if ev:
            ev[1].record()
        t1 = time.perf_counter()
        r = self.rollouts
        self._advance_state()
        with torch.no_grad(), self._sequence_shape(self.envs.num_envs):
            next_value = self.ac.get_value(self._obs(lambda v: v[-1]), r.hidden(r.num_steps), r.masks[-1])
        r.compute_returns(next_value, False, c.reward.gamma, c.ppo.gae_lambda, c.training.use_proper_time_limits)
        acc, n = self.fit()
        done, event = self._buf["done"], self._buf["event"]
        ended = done != 0
        counts = torch.stack([ended.sum()] + [(ended & (event == e)).sum()
                                              for e in (EVENT_SUCCESS, EVENT_COLLISION, EVENT_TIMEOUT)])
        r.after_update()
        if ev:
            ev[2].record()
        vals = torch.cat([acc / n, counts.double()]).cpu().tolist()   # the update's one host sync
        t2 = time.perf_counter()
        if ev:
            ev[2].synchronize()
            rollout_s, update_s = ev[0].elapsed_time(ev[1]) / 1e3, ev[1].elapsed_time(ev[2]) / 1e3
        else:
            rollout_s, update_s = t1 - t0, t2 - t1
        return {"nll": vals[0], "value_loss": vals[1], "episodes": int(vals[2]), "success": int(vals[3]),
                "collision": int(vals[4]), "timeout": int(vals[5]), "rollout_s": rollout_s, "update_s": update_s,
                "host_s": t2 - t0}
