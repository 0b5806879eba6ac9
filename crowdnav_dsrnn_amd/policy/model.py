"""Policy wrapper (pytorchBaselines/a2c_ppo_acktr/model.py:17-104): base='srnn' or 'convgru' + DiagGaussian.

API and return values as in the reference:
  act(inputs, rnn_hxs, masks, deterministic=False) -> value (E,1), action (E,2), log_prob (E,1), rnn_hxs
  get_value(inputs, rnn_hxs, masks) -> value (E,1)
  evaluate_actions(inputs, rnn_hxs, masks, action) -> value, log_prob, entropy, rnn_hxs
`base.nenv` is writable (test.py:199) and `base.human_num` readable (evaluation.py:34).

head (this project's opt-in; None reads base_kwargs.robot.action_head, default 'gaussian'): 'lattice' replaces the
Gaussian by a 64-way categorical over the unicycle actions cn_dwa_predict chooses from (LatticeCategorical; state_dict
keys dist.fc_logits.{weight,bias}). act() still returns a float32 (E, 2) action -- the lattice point -- so envs,
storages, evaluate() and the captured rollout are the Gaussian head's; evaluate_actions scores an action at its nearest
lattice point. Unicycle action spaces only (UnsupportedConfig otherwise).
"""
import torch
import torch.nn as nn

from .. import ops
from .convgru_model import ConvGRU
from ..config import UnsupportedConfig
from .distributions import DiagGaussian, LatticeCategorical
from .srnn_model import SRNN


class Policy(nn.Module):
    HEADS = ("gaussian", "lattice")

    def __init__(self, obs_shape, action_space, base=None, base_kwargs=None, head=None):
        super().__init__()
        if base == "srnn":
            self.base = SRNN(obs_shape, base_kwargs)
            self.srnn, self.convgru = True, False
            dist_in = self.base.output_size
        elif base == "convgru":   # model.py:25-33: the LiDAR policy; its distribution reads actor.fc2 (64)
            self.base = ConvGRU(obs_shape, base_kwargs)
            self.srnn, self.convgru = False, True
            dist_in = self.base.actor.fc2.out_features
        else:
            raise NotImplementedError("base must be 'srnn' or 'convgru'")
        if action_space.__class__.__name__ != "Box":
            raise NotImplementedError("CrowdSimDict drives a Box(2,) action space")
        if head is None:
            head = getattr(getattr(base_kwargs, "robot", None), "action_head", "gaussian")
        if head not in self.HEADS:
            raise UnsupportedConfig("Policy: action head %r (one of %s)" % (head, ", ".join(self.HEADS)))
        if head == "lattice":
            kin = getattr(getattr(base_kwargs, "action_space", None), "kinematics", None)
            if kin != "unicycle":
                raise UnsupportedConfig("Policy: the 'lattice' action head is the unicycle robot's (its candidates are "
                                        "(dv, dtheta) pairs); config.action_space.kinematics is %r" % (kin,))
            self.dist = LatticeCategorical(dist_in)
        else:
            self.dist = DiagGaussian(dist_in, action_space.shape[0])
        self.head = head

    @property
    def is_recurrent(self):
        return self.base.is_recurrent

    def forward(self, inputs, rnn_hxs, masks):
        raise NotImplementedError

    def _infer(self, inputs, rnn_hxs, masks, out_hxs=None):
        if self.srnn:
            return self.base(inputs, rnn_hxs, masks, infer=True, out_hxs=out_hxs)
        return self.base(inputs, rnn_hxs, masks)

    def act(self, inputs, rnn_hxs, masks, deterministic=False, out_hxs=None):
        """out_hxs (optional, srnn, no-grad): tensors that receive the new recurrent state (SRNN.forward)."""
        value, actor_features, rnn_hxs = self._infer(inputs, rnn_hxs, masks, out_hxs)
        if actor_features.is_cuda and not torch.is_grad_enabled() and isinstance(self.dist, DiagGaussian):
            # sample / mode and log_probs of the same distribution in one launch (ops.gaussian_act)
            d = self.dist
            action, action_log_probs = ops.gaussian_act(d.fc_mean(actor_features), d.logstd._bias.view(-1),
                                                        deterministic)
            return value, action, action_log_probs, rnn_hxs
        if self.head == "lattice" and not torch.is_grad_enabled():
            # sample / mode and its log-probability from one pass over the logits (ops.lattice_act: on CUDA one
            # cn_lattice_act launch after fc_logits)
            action, action_log_probs = ops.lattice_act(self.dist.fc_logits(actor_features), deterministic)
            return value, action, action_log_probs, rnn_hxs
        dist = self.dist(actor_features)
        action = dist.mode() if deterministic else dist.sample()
        action_log_probs = dist.log_probs(action)
        return value, action, action_log_probs, rnn_hxs

    def get_value(self, inputs, rnn_hxs, masks):
        value, _, _ = self._infer(inputs, rnn_hxs, masks)
        return value

    def evaluate_actions(self, inputs, rnn_hxs, masks, action):
        value, actor_features, rnn_hxs = self.base(inputs, rnn_hxs, masks)
        dist = self.dist(actor_features)
        if self.head == "lattice":   # both from one pass (ops.lattice_evaluate)
            action_log_probs, entropy = dist.evaluate(action)
            return value, action_log_probs, entropy.mean(), rnn_hxs
        action_log_probs = dist.log_probs(action)
        dist_entropy = dist.entropy().mean()
        return value, action_log_probs, dist_entropy, rnn_hxs

    def evaluate_soft(self, inputs, rnn_hxs, masks, regret, tau):
        """evaluate_actions against soft labels (the lattice head only): regret (B, 64) float32, the expert's regret
        row of every state (CrowdNavEngine.robot_mix's `regret`), tau > 0 -> value, ce (B, 1) the cross-entropy
        against softmax(-regret / tau) with its gradient, kl (B, 1) and logp_best (B, 1) the log-probability of the
        expert's own choice, both reported without gradient (ops.lattice_soft_ce), rnn_hxs."""
        if self.head != "lattice":
            raise UnsupportedConfig("Policy.evaluate_soft: soft labels are a distribution over the lattice head's 64 "
                                    "candidates; this policy's head is %r" % (self.head,))
        value, actor_features, rnn_hxs = self.base(inputs, rnn_hxs, masks)
        ce, kl, logp_best = self.dist(actor_features).soft_cross_entropy(regret, tau)
        return value, ce.unsqueeze(1), kl.unsqueeze(1), logp_best.unsqueeze(1), rnn_hxs
