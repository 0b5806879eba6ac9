#!/usr/bin/env python
"""HIP-event timings of learner.DAgger's chunk beside RolloutTrainer's rollout of the same policy and shape.

On the unicycle robot with the 'dwa' expert (1024 envs x 32 steps x 5 humans by default), per graph setting (one
captured HIP graph per chunk / every launch eager):
  ppo_rollout     RolloutTrainer.collect(): act -> step_device -> storage, stochastic actions
  dagger_rollout  DAgger.collect() at beta = 0: the same loop plus the expert's launch, the mix launch and the
                  loop's own records (proposed, done, event) per step; the learner alone drives, deterministic
  dagger_update   the rest of DAgger.update(): returns, `epochs` passes over the chunks held, at aggregate 1 and 4
seconds per chunk between two events on the current stream, the mean over --chunks chunks after 3 warm-up chunks (the
eager one and the capture among them); three runs each, the median reported with the runs' spread. RolloutTrainer is
not touched by DAgger, so its figure is the one of the commit before it. Needs a GPU; prints one JSON line per setting.

Usage: python tools/dagger_time.py [--envs 1024] [--steps 32] [--chunks 20] [--head gaussian|lattice] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, clone_config  # noqa: E402
from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv  # noqa: E402
from crowdnav_dsrnn_amd.learner import DAgger  # noqa: E402
from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer  # noqa: E402
from crowdnav_dsrnn_amd.policy import Policy  # noqa: E402

DEV = "cuda:0"


def per_chunk(fn, chunks, warmup=3):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(chunks):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--mini-batch", type=int, default=2)
    ap.add_argument("--head", default="gaussian", choices=Policy.HEADS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dagger_time: needs a GPU")
    E = args.envs
    c = clone_config(Config())
    c.sim.human_num = 5
    c.action_space.kinematics = "unicycle"
    c.robot.scripted_unicycle = True
    c.robot.scripted_dwa = True
    c.robot.action_head = args.head
    c.training.num_processes = E
    c.ppo.num_steps = args.steps
    c.ppo.num_mini_batch = args.mini_batch

    def fresh():
        envs = CrowdNavVecEnv(c, E, 0, DEV, allow_early_resets=True, nenv=E, phase="train")
        torch.manual_seed(0)
        pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=envs.config).to(DEV)
        return envs, pol

    def ppo_rollout(graphs):
        envs, pol = fresh()
        tr = RolloutTrainer(c, envs, pol, None, graphs=graphs)
        s = per_chunk(tr.collect, args.chunks)
        envs.close()
        return s

    def dagger(graphs, aggregate):
        envs, pol = fresh()
        dg = DAgger(c, envs, pol, expert="dwa", beta=0.0, lr=1e-3, aggregate=aggregate, graphs=graphs)
        roll = upd = 0.0
        for u in range(3 + args.chunks):
            st = dg.update()
            if u >= 3:
                roll += st["rollout_s"]
                upd += st["update_s"]
        envs.close()
        return roll / args.chunks, upd / args.chunks

    lines = []
    for graphs in (True, False):
        runs = {"ppo_rollout": [], "dagger_rollout": [], "dagger_update_k1": [], "dagger_update_k4": []}
        for _ in range(3):
            runs["ppo_rollout"].append(ppo_rollout(graphs))
            r1, u1 = dagger(graphs, 1)
            _, u4 = dagger(graphs, 4)
            runs["dagger_rollout"].append(r1)
            runs["dagger_update_k1"].append(u1)
            runs["dagger_update_k4"].append(u4)
        rec = {"envs": E, "steps": args.steps, "humans": 5, "head": args.head, "expert": "dwa", "beta": 0.0,
               "graphs": graphs, "chunks": args.chunks, "unit": "s per chunk (HIP events)",
               "device": torch.cuda.get_device_name(0)}
        for k, v in runs.items():
            v = sorted(v)
            rec[k] = round(v[1], 5)
            rec[k + "_min_max"] = [round(v[0], 5), round(v[2], 5)]
        rec["dagger_over_ppo_rollout"] = round(rec["dagger_rollout"] / rec["ppo_rollout"], 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
