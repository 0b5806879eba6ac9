"""Action distribution of the Box action space (pytorchBaselines/a2c_ppo_acktr/distributions.py:36-94), and this
project's opt-in lattice head for the unicycle robot (LatticeCategorical: no reference counterpart)."""
import torch
import torch.nn as nn

from .. import ops
from .utils import AddBias, Linear, init


class FixedNormal(torch.distributions.Normal):
    """distributions.py:36-45: log_probs summed over action dims, mode = mean.

    Built with validate_args=False: torch's default argument validation reduces loc / scale / the
    actions to a host bool (three device->host synchronisations per act()); it only raises on NaN or
    non-positive inputs and never changes a value."""

    def __init__(self, loc, scale):
        super().__init__(loc, scale, validate_args=False)

    def sample(self, sample_shape=torch.Size()):
        """loc + scale * N(0, 1): the draw torch.normal(loc, scale) makes, without its std >= 0 check
        (a device min + host read per call)."""
        shape = self._extended_shape(sample_shape)
        with torch.no_grad():
            eps = torch.randn(shape, dtype=self.loc.dtype, device=self.loc.device)
            return eps * self.scale.expand(shape) + self.loc.expand(shape)

    def log_probs(self, actions):
        return super().log_prob(actions).sum(-1, keepdim=True)

    def entrop(self):
        return super().entropy().sum(-1)

    def mode(self):
        return self.mean


class DiagGaussian(nn.Module):
    """distributions.py:74-94: mean from a linear layer, state-independent log-std (AddBias on zeros)."""

    def __init__(self, num_inputs, num_outputs):
        super().__init__()
        self.fc_mean = init(Linear(num_inputs, num_outputs), nn.init.orthogonal_, lambda x: nn.init.constant_(x, 0))
        self.logstd = AddBias(torch.zeros(num_outputs))

    def forward(self, x):
        action_mean = self.fc_mean(x)
        action_logstd = self.logstd(torch.zeros_like(action_mean))
        return FixedNormal(action_mean, action_logstd.exp())


class FixedLattice:
    """The lattice head's distribution over cn_dwa_predict's 64 unicycle actions for a batch of logits (B, 64)
    (include/crowdnav.h, cn_lattice_*): actions are lattice points (B, 2); log_probs scores an action at its nearest
    lattice point, so a continuous label (ORCA or the social force through the tracking law) is scored there too."""

    def __init__(self, logits):
        self.logits = logits

    def mode(self):
        with torch.no_grad():
            return ops.lattice_act(self.logits, True)[0]

    def sample(self):
        with torch.no_grad():
            return ops.lattice_act(self.logits, False)[0]

    def evaluate(self, actions):
        """(log_probs (B, 1), entropy (B,)) from one pass over the logits."""
        return ops.lattice_evaluate(self.logits, actions)

    def log_probs(self, actions):
        return self.evaluate(actions)[0]

    def entropy(self):
        return ops.lattice_evaluate(self.logits, self.logits.new_zeros((self.logits.shape[0], 2)))[1]

    def soft_cross_entropy(self, regret, tau):
        """(ce (B,), kl (B,), logp_best (B,)) against the target softmax(-regret / tau) of the expert's regret rows
        (B, 64) (ops.lattice_soft_ce: the gradient reaches the logits through ce)."""
        return ops.lattice_soft_ce(self.logits, regret, tau)


class LatticeCategorical(nn.Module):
    """The opt-in action head of the unicycle robot (robot.action_head = 'lattice'): 64 logits from a linear layer
    (orthogonal, gain 0.01, zero bias: a near-uniform policy at the start), one per candidate of the 8 x 8 lattice."""

    def __init__(self, num_inputs):
        super().__init__()
        self.fc_logits = init(Linear(num_inputs, ops.LATTICE), nn.init.orthogonal_,
                              lambda x: nn.init.constant_(x, 0), gain=0.01)

    def forward(self, x):
        return FixedLattice(self.fc_logits(x))
