"""Train one DSRNN policy over crowds of varying size and compare it with policies trained at a single size.

PPO (RolloutTrainer) on config.sim.human_nums (default 5 10) for --updates updates, then evaluate() of the resulting
state_dict on the plain test sets of each trained count and of one count it never saw (default 7): a varied-count
policy is evaluated per density on plain VecEnvs with a Policy built at that human_num from the same state_dict.
The same rows for policies trained at each single count with the same budget and seed. Every row (budgets and
wall times included) goes to stdout and to --out as JSON lines. The outcome is whatever is measured: nothing about
it is assumed here."""
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


def base_config(a):
    c = clone_config(Config())
    c.training.num_processes = a.envs
    c.ppo.num_steps = a.steps
    c.ppo.num_mini_batch = a.mini_batch
    c.ppo.epoch = a.epoch
    c.training.lr = a.lr
    c.env.test_size = a.test_size
    c.env.seed = a.seed
    return c


def train(a, nums):
    """nums: a list of counts (one mixed engine) or one int (the plain engine). Returns (state_dict, row)."""
    c = base_config(a)
    if isinstance(nums, int):
        c.sim.human_num = nums
    else:
        c.sim.human_nums = list(nums)
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
    counts = envs.engine.env_humans.tolist()
    nmax = max(counts)
    row = {"kind": "train", "trained_on": nums, "updates": a.updates, "envs": a.envs, "num_steps": a.steps,
           "env_steps": tr.env_steps, "epoch": c.ppo.epoch, "num_mini_batch": c.ppo.num_mini_batch, "lr": c.training.lr,
           "seed": a.seed, "wall_s": round(time.perf_counter() - t0, 2), "graph_rollouts": tr._graph is not None,
           "episodes": episodes, "last_mean_episode_return": round(ret, 4),
           "last_value_loss": stats["value_loss"], "last_action_loss": stats["action_loss"],
           # rows of the spatial edge GRU that are padding (the size of the compaction left as follow-up)
           "padded_row_share": round(1.0 - sum(counts) / float(nmax * len(counts)), 4)}
    envs.close()
    return {k: v.detach().clone() for k, v in pol.state_dict().items()}, row


def test(a, sd, trained_on, n):
    """evaluate() of the state_dict on the plain test set at human_num = n."""
    c = base_config(a)
    c.sim.human_num = n
    E = min(a.eval_envs, a.test_size)
    c.training.num_processes = E
    envs = CrowdNavVecEnv(c, E, a.seed, DEV, allow_early_resets=True, nenv=E, phase="test")
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=c).to(DEV)
    pol.load_state_dict(sd)
    pol.eval()
    log = logging.getLogger("train_varied")
    t0 = time.perf_counter()
    evaluate(pol, False, envs, E, DEV, c, log, keep_traces=False, verbose=False)
    last = evaluate.last
    return {"kind": "test", "trained_on": trained_on, "human_num": n, "test_size": a.test_size, "eval_envs": E,
            "success_rate": last["success_rate"], "collision_rate": last["collision_rate"],
            "timeout_rate": last["timeout_rate"], "wall_s": round(time.perf_counter() - t0, 2),
            "updates": a.updates, "seed": a.seed}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--human-nums", type=int, nargs="+", default=[5, 10])
    ap.add_argument("--unseen", type=int, default=7, help="a count none of the policies is trained on")
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--mini-batch", type=int, default=2)
    ap.add_argument("--epoch", type=int, default=5)
    ap.add_argument("--lr", type=float, default=4e-5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--test-size", type=int, default=500)
    ap.add_argument("--eval-envs", type=int, default=100)
    ap.add_argument("--no-single", action="store_true", help="skip the single-count baselines")
    ap.add_argument("--out", default=os.path.join("profiles", "varied", "train_varied.jsonl"))
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    densities = sorted(set(a.human_nums) | {a.unseen})
    with open(a.out, "a") as fh:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()

        runs = [list(a.human_nums)] + ([] if a.no_single else sorted(set(a.human_nums)))
        for nums in runs:
            sd, row = train(a, nums)
            emit(row)
            for n in densities:
                emit(test(a, sd, nums, n))


if __name__ == "__main__":
    main()
