"""Train the DSRNN policy for a robot with a limited field of view, with and without the visible-humans attention.

PPO (RolloutTrainer) on --humans humans at robot.FOV --fov (default 5 at 0.5), once with config.sim.visible_masks (the
spatial attention runs over the humans the robot sees) and once without (it runs over all belief slots, stale and
never-seen ones included), same seed and budget (tools/train_varied.py's), then evaluate() of each on the default test
episodes at that FOV (the opt-in policy on an opt-in env). Every row (budgets and wall times included) goes to stdout
and to --out as JSON lines. The outcome is whatever is measured: nothing about it is assumed here."""
import argparse
import json
import logging
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crowdnav_dsrnn_amd.config import Config, clone_config  # noqa: E402
from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv  # noqa: E402
from crowdnav_dsrnn_amd.evaluation import evaluate  # noqa: E402
from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer  # noqa: E402
from crowdnav_dsrnn_amd.learner.ppo import PPO  # noqa: E402
from crowdnav_dsrnn_amd.policy import Policy  # noqa: E402

DEV = "cuda:0"


def base_config(a, visible):
    c = clone_config(Config())
    c.training.num_processes = a.envs
    c.ppo.num_steps = a.steps
    c.ppo.num_mini_batch = a.mini_batch
    c.ppo.epoch = a.epoch
    c.training.lr = a.lr
    c.env.test_size = a.test_size
    c.env.seed = a.seed
    c.sim.human_num = a.humans
    c.robot.FOV = a.fov
    c.sim.visible_masks = visible
    return c


def train(a, visible):
    c = base_config(a, visible)
    torch.manual_seed(a.seed)
    envs = CrowdNavVecEnv(c, a.envs, a.seed, DEV, nenv=a.envs, phase="train")
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=envs.config).to(DEV)
    agent = PPO(pol, c.ppo.clip_param, c.ppo.epoch, c.ppo.num_mini_batch, c.ppo.value_loss_coef, c.ppo.entropy_coef,
                lr=c.training.lr, eps=c.training.eps, max_grad_norm=c.training.max_grad_norm)
    tr = RolloutTrainer(c, envs, pol, agent)
    t0 = time.perf_counter()
    episodes, ret, stats = 0, 0.0, None
    for _ in range(a.updates):
        stats = tr.update()
        episodes += stats["episodes"]
        ret = stats["mean_episode_return"]
    torch.cuda.synchronize()
    row = {"kind": "train", "visible_masks": visible, "humans": a.humans, "robot_fov": a.fov, "updates": a.updates,
           "envs": a.envs, "num_steps": a.steps, "env_steps": tr.env_steps, "epoch": c.ppo.epoch,
           "num_mini_batch": c.ppo.num_mini_batch, "lr": c.training.lr, "seed": a.seed,
           "wall_s": round(time.perf_counter() - t0, 2), "graph_rollouts": tr._graph is not None,
           "graph_nodes": tr.graph_audit, "episodes": episodes, "last_mean_episode_return": round(ret, 4),
           "last_value_loss": stats["value_loss"], "last_action_loss": stats["action_loss"]}
    if visible:
        row["visible_share_last_rollout"] = round(float(tr.rollouts.obs["visible_masks"].mean()), 4)
    envs.close()
    return {k: v.detach().clone() for k, v in pol.state_dict().items()}, row


def test(a, sd, visible):
    c = base_config(a, visible)
    E = min(a.eval_envs, a.test_size)
    c.training.num_processes = E
    envs = CrowdNavVecEnv(c, E, a.seed, DEV, allow_early_resets=True, nenv=E, phase="test")
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=c).to(DEV)
    pol.load_state_dict(sd)
    pol.eval()
    log = logging.getLogger("train_fov")
    t0 = time.perf_counter()
    evaluate(pol, False, envs, E, DEV, c, log, keep_traces=False, verbose=False)
    last = evaluate.last
    envs.close()
    return {"kind": "test", "visible_masks": visible, "humans": a.humans, "robot_fov": a.fov, "test_size": a.test_size,
            "eval_envs": E, "success_rate": last["success_rate"], "collision_rate": last["collision_rate"],
            "timeout_rate": last["timeout_rate"], "wall_s": round(time.perf_counter() - t0, 2), "updates": a.updates,
            "seed": a.seed}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--fov", type=float, default=0.5, help="robot.FOV in units of pi")
    ap.add_argument("--updates", type=int, default=1200)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--mini-batch", type=int, default=2)
    ap.add_argument("--epoch", type=int, default=5)
    ap.add_argument("--lr", type=float, default=4e-5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--test-size", type=int, default=500)
    ap.add_argument("--eval-envs", type=int, default=100)
    ap.add_argument("--out", default=os.path.join("profiles", "visible_attn", "train_fov.jsonl"))
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()

        for visible in (True, False):
            sd, row = train(a, visible)
            emit(row)
            emit(test(a, sd, visible))


if __name__ == "__main__":
    main()
