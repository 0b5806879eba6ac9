"""DAgger (Ross, Gordon & Bagnell 2011): the learner drives the envs, the scripted expert labels every state it runs
into, and the policy is fitted to those labels.

    dg = DAgger(config, envs, actor_critic, expert="dwa", beta=1.0, beta_decay=0.5)
    stats = dg.update()      # one chunk of num_steps steps of every env + `epochs` passes over the chunks held
    ...
    trainer = RolloutTrainer(config, envs, actor_critic, agent)   # the same policy continues with PPO

BehaviourCloning sees the states a (perturbed) EXPERT reaches. Here chunk i is driven by the mixture policy: at every
step and env a coin of probability beta_i = max(beta_min, beta * beta_decay**i) decides whether the expert's action or
the learner's own is executed (cn_robot_mix; policy_factory.robot_mix_ref restates it), while the label recorded for
the state is always the expert's. beta = 1 with beta_decay = 1 is the expert's clean rollout; beta = 0 is the learner
alone, relabelled.

Per step t of a chunk: act on storage slot t (the new recurrent state straight into the storage, as
RolloutTrainer._rollout does), envs.robot_mix -> labels[t], executed[t], flags[t], envs.step_device(executed[t]), and
the storage insert with THE LABEL in the storage's `actions`; the learner's own action is kept in `proposed`. No host
synchronisation inside the loop. With graphs (the default on CUDA, plain engines) the first chunk runs eagerly, the
second is captured as one HIP graph under the engine's graph mode -- audited for memset nodes as
RolloutTrainer.collect audits its own, with the same fall-back -- and every later chunk is a replay: beta and the
coin's step0 live in a 16-byte device block that one small launch outside the graph rewrites before each chunk
(CrowdNavEngine.set_mix_ctl), so the replay reads the new values.

aggregate = K keeps the last K chunks on the device (observations, chunk-start recurrent state, masks, labels,
returns) and fit() walks the minibatches of every chunk held, newest last: the data aggregation that gives the method
its name, bounded to a ring. An older chunk keeps the recurrent start state it was recorded with, computed under
weights that have moved since: the staleness PPO already accepts within one update, where the later epochs start from
the state the rollout's weights produced. K = 1 is pure on-policy relabelling.

The loss is BehaviourCloning's (`_losses`: the label's negative log-likelihood under whatever head the policy has, plus
the value regression), the policy / observation pairs are the ones it accepts, and the trained module hands over to
RolloutTrainer exactly as a cloned one does. An env with sim.visible_masks needs no sim.visible_masks_scripted here:
the loop goes through step_device, which returns the mask. An env with sim.human_nums needs sim.human_nums_scripted
(robot_act's rule) and runs eagerly (graph mode is the plain engine's).

soft_tau = tau > 0 (expert 'dwa' with the lattice head; None, the default: the hard label above, with exactly the calls
made without this option) fits the head to ALL 64 of the expert's candidate costs instead of its one choice. The
labelling launch of every step also writes the expert's regret row (envs.robot_mix(..., regret=): (float)(J_c - J_best),
0 at the choice) into a fixed (T, E, 64) buffer -- the captured chunk replays into it -- which _keep copies to the
chunk's ring slot, and fit() minimises the cross-entropy against the target softmax(-regret / tau)
(Policy.evaluate_soft -> cn_lattice_soft_fwd / _bwd) plus the same value regression. Many of the 64 candidates are
near-ties, and among exact ties the hard label is "the lowest index": the soft target spreads its mass over every
candidate within about tau of the best and tells the head which others are catastrophic. update() keeps 'nll' as the
HARD label's negative log-likelihood (-logp of the expert's choice, from the same pass), so that column compares with
hard runs, and adds 'soft_ce', 'kl' (KL(target || policy)) and 'soft_tau'. BehaviourCloning has no such option -- its
data comes from cn_rollout*, which record no regret rows; DAgger(beta=1, beta_decay=1, soft_tau=tau) is the expert's
clean rollout with soft labels.
"""
import math
import os
import time
import warnings

import torch
import torch.nn as nn
import torch.optim as optim

from .imitation import EVENT_COLLISION, EVENT_SUCCESS, EVENT_TIMEOUT, BehaviourCloning
from .storage import RolloutStorage, SRNNRolloutStorage, _copy_all


class DAgger(BehaviourCloning):
    """See the module's docstring. Shares BehaviourCloning's loss, minibatch shapes and chunk_nll(); the collection,
    the ring of chunks and update() are its own."""

    def __init__(self, config, envs, actor_critic, expert="dwa", beta=1.0, beta_decay=0.5, beta_min=0.0, seed=0,
                 num_steps=None, num_mini_batch=None, epochs=1, lr=None, value_coef=0.5, aggregate=1,
                 deterministic=True, graphs=None, soft_tau=None):
        from ..config import UnsupportedConfig
        from ..policy_factory import ScriptedRobot

        ScriptedRobot.check(envs, expert)   # before anything touches the GPU, as everything down to the optimizer
        if soft_tau is not None:
            soft_tau = float(soft_tau)
            if not (math.isfinite(soft_tau) and soft_tau > 0.0):
                raise ValueError("DAgger: soft_tau must be a finite temperature > 0 (None: the hard label), got %r"
                                 % (soft_tau,))
            if expert != "dwa" or getattr(actor_critic, "head", None) != "lattice":
                raise UnsupportedConfig("DAgger: soft_tau needs expert='dwa' (the one controller with a candidate set) "
                                        "and a policy with the lattice head (robot.action_head = 'lattice')")
        self.soft_tau = soft_tau
        for name, v in (("beta", beta), ("beta_decay", beta_decay), ("beta_min", beta_min)):
            if not 0.0 <= float(v) <= 1.0:   # (a NaN fails both)
                raise ValueError("DAgger: %s in [0, 1] required, got %r" % (name, v))
        if int(aggregate) < 1:
            raise ValueError("DAgger: aggregate >= 1 (chunks held) required, got %r" % (aggregate,))
        mode = getattr(envs, "obs_mode", "srnn")
        self.convgru = mode == "convgru"
        if self.convgru:
            lc = config.lidar
            if not getattr(actor_critic, "convgru", False) or not (getattr(lc, "live", False) and lc.enable):
                raise UnsupportedConfig("DAgger: a 'convgru' env needs the ConvGRU policy (base='convgru') and "
                                        "config.lidar.live")
        elif mode != "srnn" or not getattr(actor_critic, "srnn", False):
            raise UnsupportedConfig("DAgger: the DSRNN policy (base='srnn') on the 'srnn' observation, or the ConvGRU "
                                    "policy (base='convgru') on a live 'convgru' one")
        self.config = config
        self.envs = envs
        self.ac = actor_critic
        self.expert = expert
        self.beta0, self.beta_decay, self.beta_min = float(beta), float(beta_decay), float(beta_min)
        self.seed = int(seed)
        self.aggregate = int(aggregate)
        self.deterministic = bool(deterministic)
        self.num_steps = int(config.ppo.num_steps if num_steps is None else num_steps)
        self.num_mini_batch = int(config.ppo.num_mini_batch if num_mini_batch is None else num_mini_batch)
        self.epochs = int(epochs)
        self.value_coef = float(value_coef)
        self.max_grad_norm = config.training.max_grad_norm
        E = envs.num_envs
        if self.num_steps < 1 or self.epochs < 1 or not 1 <= self.num_mini_batch <= E or E % self.num_mini_batch:
            raise ValueError("DAgger: num_steps >= 1, epochs >= 1 and a num_mini_batch that divides the %d envs "
                             "required" % E)
        dev = envs.engine.device
        self.device = dev
        # HIP-graph chunks (collect); CN_NO_GRAPHS=1 or graphs=False: every chunk eager. Graph mode is the plain
        # engine's: an env over a mixed engine (config.sim.human_nums) runs eagerly, chosen here
        if graphs is None:
            graphs = dev.type == "cuda" and os.environ.get("CN_NO_GRAPHS", "") in ("", "0")
        self.graphs = bool(graphs) and getattr(envs.engine, "groups", None) is None
        self._graph, self._warm = None, False
        self.graph_audit = None   # node census of the captured chunk (collect)
        self.optimizer = optim.Adam(actor_critic.parameters(), lr=config.training.lr if lr is None else lr,
                                    eps=config.training.eps)
        self.srnn = not self.convgru
        self.rollouts = self._storage()
        # the chunks fit() walks: the live storage itself at aggregate 1, else a ring of copies
        self.ring = [self.rollouts] if self.aggregate == 1 else [self._storage() for _ in range(self.aggregate)]
        T = self.num_steps
        self.labels = torch.zeros((T, E, 2), dtype=torch.float32, device=dev)     # the expert's action, every state
        self.proposed = torch.zeros((T, E, 2), dtype=torch.float32, device=dev)   # the learner's own
        self.executed = torch.zeros((T, E, 2), dtype=torch.float32, device=dev)   # what the step took
        self.flags = torch.zeros((T, E), dtype=torch.uint8, device=dev)           # bit 0 took the expert, bit 1 agree
        if self.soft_tau is not None:   # the expert's regret rows: the live chunk's (fixed addresses), and per ring slot
            self.regret = torch.zeros((T, E, 64), dtype=torch.float32, device=dev)
            self.ring_regret = ([self.regret] if self.aggregate == 1
                                else [torch.zeros_like(self.regret) for _ in range(self.aggregate)])
        self.done = torch.zeros((T, E), dtype=torch.uint8, device=dev)
        self.event = torch.zeros((T, E), dtype=torch.int8, device=dev)
        self._ones = torch.ones((E, 1), device=dev)
        self.ctl = envs.engine.mix_ctl()
        self.beta = self.beta0    # the last chunk's
        self.env_steps = 0
        self.chunks = 0
        obs = envs.reset()
        r = self.rollouts
        if self.convgru:
            r.obs[0].copy_(obs)
        else:
            for k in r.obs:
                r.obs[k][0].copy_(obs[k])

    def _storage(self):
        c, envs, T, E = self.config, self.envs, self.num_steps, self.envs.num_envs
        if self.convgru:
            return RolloutStorage(T, E, envs.observation_space.shape, envs.action_space,
                                  self.ac.base.recurrent_hidden_state_size, device=self.device, compact_hidden=True)
        return SRNNRolloutStorage(T, E, envs.observation_space.spaces, envs.action_space, c.SRNN.human_node_rnn_size,
                                  c.SRNN.human_human_edge_rnn_size, "GRU", device=self.device, compact_hidden=True)

    def chunk_beta(self, i):
        """beta of chunk i: max(beta_min, beta * beta_decay**i)."""
        return max(self.beta_min, self.beta0 * self.beta_decay ** int(i))

    def _chunk(self):
        """num_steps steps: act, robot_mix, step_device, the storage insert (the label as the action) and one
        multi-tensor copy of the loop's own records. No host synchronisation."""
        r, T = self.rollouts, self.num_steps
        for t in range(T):
            obs_s = {k: v[t] for k, v in r.obs.items()} if isinstance(r.obs, dict) else r.obs[t]
            value, action, logp, hxs = self.ac.act(obs_s, r.hidden(t), r.masks[t], deterministic=self.deterministic,
                                                   **({"out_hxs": r.hidden_slot()} if self.srnn else {}))
            action = action.contiguous()
            if self.soft_tau is None:
                self.envs.robot_mix(self.expert, action, self.ctl, t, label=self.labels[t], executed=self.executed[t],
                                    flags=self.flags[t])
            else:   # the same launches, the labelling one writing the regret rows too
                self.envs.robot_mix(self.expert, action, self.ctl, t, label=self.labels[t], executed=self.executed[t],
                                    flags=self.flags[t], regret=self.regret[t])
            obs, reward, done, event, _, _, _ = self.envs.step_device(self.executed[t])
            masks = torch.rsub(done.unsqueeze(1), 1.0)   # 1 - done as float32 (one kernel)
            r.insert(obs, hxs, self.labels[t], logp, value, reward.unsqueeze(1), masks, self._ones)
            _copy_all([self.proposed[t], self.done[t], self.event[t]], [action, done, event])

    @torch.no_grad()
    def collect(self):
        """Chunk i = self.chunks into the storage: obs[t] the state the learner acted on, actions[t] = labels[t] the
        expert's action there, executed[t] what the step took under beta_i. One small launch sets beta_i and
        step0 = i * num_steps in the device block; then the loop, eager or as one graph replay."""
        r, i = self.rollouts, self.chunks
        self.beta = self.chunk_beta(i)
        eng = self.envs.engine
        eng.set_mix_ctl(self.ctl, self.beta, self.seed, i * self.num_steps)
        with self._sequence_shape(self.envs.num_envs):   # (act reads the DSRNN's nenv)
            if self.graphs and self._warm and self._graph is None:
                from .. import _lib

                g = torch.cuda.CUDAGraph(keep_graph=True)   # kept until audited, then instantiated
                step0 = r.step
                try:
                    eng.set_graph_mode(True)   # cn_step launches without per-call arguments
                    with torch.cuda.graph(g):   # records only; the replay below runs it
                        self._chunk()
                except RuntimeError as e:   # a capture-unsafe call on this path: stay eager
                    warnings.warn("DAgger HIP-graph capture failed (%s); running eagerly" % e)
                    self.graphs = False
                    g = None
                    eng.set_graph_mode(False)
                r.step = step0
                if g is not None:
                    # no memset nodes: this runtime can replay one with stale bytes (RolloutTrainer.collect)
                    self.graph_audit = _lib.graph_node_counts(g.raw_cuda_graph())
                    if self.graph_audit.get("memset", 0):
                        warnings.warn("DAgger HIP graph holds %d memset node(s) (%s); running eagerly"
                                      % (self.graph_audit["memset"], self.graph_audit))
                        self.graphs = False
                        g = None
                        eng.set_graph_mode(False)
                    else:
                        g.instantiate()
                self._graph = g
            if self.graphs and self._graph is not None:
                self._graph.replay()   # (r.step is back at its start value: num_steps inserts wrap it)
            else:
                self._chunk()
                self._warm = True
        self.chunks += 1
        self.env_steps += self.num_steps * self.envs.num_envs

    def held(self):
        """The storages of the chunks fit() walks, oldest first (at most `aggregate`)."""
        K, n = self.aggregate, self.chunks
        if K == 1:
            return [self.rollouts]
        return [self.ring[j % K] for j in range(max(0, n - K), n)]

    def held_regret(self):
        """soft_tau: the (T, E, 64) regret rows of the chunks held(), in its order."""
        K, n = self.aggregate, self.chunks
        if K == 1:
            return [self.regret]
        return [self.ring_regret[j % K] for j in range(max(0, n - K), n)]

    @torch.no_grad()
    def _keep(self):
        """The chunk just collected (returns computed) into its ring slot: what recurrent_generator and the loss
        read -- observations, the chunk-start recurrent state, masks, labels, returns."""
        if self.aggregate == 1:
            return
        r, s = self.rollouts, self.ring[(self.chunks - 1) % self.aggregate]
        if isinstance(r.obs, dict):
            for k in r.obs:
                s.obs[k].copy_(r.obs[k])
            for k in r.recurrent_hidden_states:
                s.recurrent_hidden_states[k][0].copy_(r.recurrent_hidden_states[k][0])
        else:
            s.obs.copy_(r.obs)
            s.recurrent_hidden_states[0].copy_(r.recurrent_hidden_states[0])
        s.masks.copy_(r.masks)
        s.actions.copy_(r.actions)
        s.returns.copy_(r.returns)
        if self.soft_tau is not None:
            self.ring_regret[(self.chunks - 1) % self.aggregate].copy_(self.regret)

    @torch.no_grad()
    def chunk_soft_ce(self):
        """soft_tau: the live chunk's mean soft cross-entropy under the current weights (device scalar); chunk_nll()'s
        counterpart."""
        r, T, E = self.rollouts, self.num_steps, self.envs.num_envs
        with self._sequence_shape(E):
            obs = self._obs(lambda v: v[:-1].reshape(T * E, *v.shape[2:]))
            hxs = self._hxs(lambda v: v[0])
            return self.ac.evaluate_soft(obs, hxs, r.masks[:-1].reshape(T * E, 1), self.regret.reshape(T * E, 64),
                                         self.soft_tau)[1].mean()

    def _fit_soft(self, epochs=None):
        """fit() with soft labels: the same walk with each minibatch's env indices (with_ind: the same randperm draw),
        which select the chunk's regret rows in the minibatch's (step, env) order; minimises ce.mean() + value_coef *
        value_loss. Device tensor [sum of hard nll, sum of value_loss, sum of soft ce, sum of kl], and the number."""
        acc, n = torch.zeros(4, dtype=torch.float64, device=self.device), 0
        B = self.envs.num_envs // self.num_mini_batch
        with self._sequence_shape(B):
            for _ in range(self.epochs if epochs is None else int(epochs)):
                for s, reg in zip(self.held(), self.held_regret()):
                    for obs_b, hxs_b, _, _, return_b, masks_b, _, _, ind in s.recurrent_generator(
                            s.returns[:-1], self.num_mini_batch, with_ind=True):
                        regret_b = reg.index_select(1, ind).reshape(-1, 64)
                        values, ce, kl, logp_best, _ = self.ac.evaluate_soft(obs_b, hxs_b, masks_b, regret_b,
                                                                             self.soft_tau)
                        soft_ce = ce.mean()
                        value_loss = 0.5 * (values - return_b).pow(2).mean()
                        self.optimizer.zero_grad()
                        (soft_ce + self.value_coef * value_loss if self.value_coef else soft_ce).backward()
                        nn.utils.clip_grad_norm_(self.ac.parameters(), self.max_grad_norm)
                        self.optimizer.step()
                        acc += torch.stack([-logp_best.mean(), value_loss.detach(), soft_ce.detach(),
                                            kl.mean()]).double()
                        n += 1
        return acc, n

    def fit(self, epochs=None):
        """`epochs` passes over every chunk held, oldest first (recurrent_generator's minibatches of each): device
        tensor [sum of nll, sum of value_loss] over the minibatches, and their number. With soft_tau: _fit_soft, whose
        tensor carries two more sums."""
        if self.soft_tau is not None:
            return self._fit_soft(epochs)
        acc, n = torch.zeros(2, dtype=torch.float64, device=self.device), 0
        B = self.envs.num_envs // self.num_mini_batch
        with self._sequence_shape(B):
            for _ in range(self.epochs if epochs is None else int(epochs)):
                for s in self.held():
                    for obs_b, hxs_b, actions_b, _, return_b, masks_b, _, _ in s.recurrent_generator(
                            s.returns[:-1], self.num_mini_batch):
                        nll, value_loss = self._losses(obs_b, hxs_b, masks_b, actions_b, return_b)
                        self.optimizer.zero_grad()
                        (nll + self.value_coef * value_loss if self.value_coef else nll).backward()
                        nn.utils.clip_grad_norm_(self.ac.parameters(), self.max_grad_norm)
                        self.optimizer.step()
                        acc += torch.stack([nll.detach(), value_loss.detach()]).double()
                        n += 1
        return acc, n

    def update(self):
        """One chunk under the mixture policy + `epochs` passes over the chunks held: BehaviourCloning.update()'s dict
        plus 'beta' (the chunk's), 'took_expert' (share of env-steps whose executed action was the expert's) and
        'agree' (share whose learner action equalled the label bit for bit). rollout_s / update_s are GPU time
        between HIP events on the current stream; one host synchronisation, at the end. With soft_tau: 'nll' stays the
        hard label's (-logp of the expert's choice), and the dict gains 'soft_ce' (the loss fitted), 'kl' and
        'soft_tau'."""
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
        with torch.no_grad(), self._sequence_shape(self.envs.num_envs):
            next_value = self.ac.get_value(self._obs(lambda v: v[-1]), r.hidden(r.num_steps), r.masks[-1])
        r.compute_returns(next_value, False, c.reward.gamma, c.ppo.gae_lambda, c.training.use_proper_time_limits)
        self._keep()
        acc, n = self.fit()
        ended = self.done != 0
        counts = torch.stack([ended.sum()] + [(ended & (self.event == e)).sum()
                                              for e in (EVENT_SUCCESS, EVENT_COLLISION, EVENT_TIMEOUT)]
                             + [((self.flags & 1) != 0).sum(), ((self.flags & 2) != 0).sum()])
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
        steps = float(self.flags.numel())
        soft = {}
        if self.soft_tau is not None:   # acc is [nll, value_loss, soft_ce, kl]: the counts follow those four
            soft = {"soft_ce": vals[2], "kl": vals[3], "soft_tau": self.soft_tau}
            vals = vals[:2] + vals[4:]
        return dict({"nll": vals[0], "value_loss": vals[1], "episodes": int(vals[2]), "success": int(vals[3]),
                     "collision": int(vals[4]), "timeout": int(vals[5]), "rollout_s": rollout_s, "update_s": update_s,
                     "host_s": t2 - t0, "beta": self.beta, "took_expert": vals[6] / steps, "agree": vals[7] / steps},
                    **soft)
