"""On-device PPO learner for the DSRNN policy.

Same classes and methods as the reference's pytorchBaselines/a2c_ppo_acktr/{storage.py,algo/ppo.py}, kept
resident on the GPU; with torch.distributed initialised (one process per GPU, backend "nccl" = RCCL)
the gradients are all-reduced per minibatch and the advantage normalisation uses global statistics.
BehaviourCloning (imitation.py) pre-trains the same policy on noise-injected rollouts of a scripted expert.
DAgger (dagger.py) puts the learner in that loop: it drives the envs and the expert labels what it runs into.
"""
from .dagger import DAgger  # noqa: F401
from .imitation import BehaviourCloning  # noqa: F401
from .ppo import PPO  # noqa: F401
from .storage import RolloutStorage, SRNNRolloutStorage  # noqa: F401
