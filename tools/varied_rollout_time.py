#!/usr/bin/env python
"""HIP-event timings of scripted rollouts on an env of varying human count (one mixed engine) against the plain
engines they replace.

  --mode mixed   ONE mixed engine of --envs envs whose env g has human_nums[g % len] humans: `rollout` (cn_rollout on
                 the mixed engine: every group its own fused sequence on its own stream) and `eager` (the Python loop
                 robot_act() -> step(), one launch per group and call)
  --mode plain   one plain engine of envs / len(human_nums) envs per count, their `rollout`s one after the other on
                 the same stream (what served such a crowd before), and the same `eager` loop over them. With
                 CN_LIB_PATH aimed at a library built from another revision this is that revision's figure.
tools/rollout_lidar_time.py's method: between two events on the current stream after one warm-up pass, --rounds
rounds alternating between the functions; every round is printed (us per recorded closed-loop step of the whole
crowd). For a comparison across libraries run the two modes in alternating processes. Needs a GPU; one JSON line.

Usage: python tools/varied_rollout_time.py --mode mixed|plain [--human-nums 5 9] [--robot orca] [--envs 4096]
           [--steps 200] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config, make_varied_cn_configs  # noqa: E402
from crowdnav_dsrnn_amd.engine import CrowdNavEngine  # noqa: E402


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps      # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("mixed", "plain"))
    ap.add_argument("--human-nums", type=int, nargs="+", default=[5, 9])
    ap.add_argument("--robot", default="orca", choices=("orca", "social_force"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("varied_rollout_time: needs a GPU")
    E, T, nums, robot = args.envs, args.steps, list(args.human_nums), args.robot
    if E % len(nums):
        raise SystemExit("varied_rollout_time: --envs must split evenly over --human-nums")
    c = clone_config(Config())
    c.action_space.kinematics = "holonomic"
    c.humans.policy = "orca"
    if args.mode == "mixed":
        cfgs, eg = make_varied_cn_configs(c, nums, E)
        engines = [CrowdNavEngine.mixed(cfgs, eg, "cuda:0", scripted=True)]
    else:
        engines = []
        for n in nums:
            cn = clone_config(c)
            cn.sim.human_num = n
            engines.append(CrowdNavEngine(make_cn_config(cn, num_envs=E // len(nums)), "cuda:0"))
    for e in engines:
        e.reset()
        e.step(e.robot_act(robot))   # (the first step after cn_reset is launched singly on every path)
    bufs = [e.rollout_buffers(T) for e in engines]
    launches = {}

    def rollout():
        launches["rollout"] = sum(e.rollout(robot, T, out=b)["num_launches"] for e, b in zip(engines, bufs))

    def eager():
        for _ in range(T):
            for e in engines:
                e.step(e.robot_act(robot))

    fns = {"rollout": rollout, "eager": eager}
    for fn in fns.values():
        fn()                        # warm-up pass
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            rounds[k].append(round(timed(fn, T), 2))
    rec = {"mode": args.mode, "human_nums": nums, "robot": robot, "envs": E, "engines": len(engines), "steps": T,
           "chunk": engines[0].seq_chunk, "unit": "us per step of all envs (HIP events)",
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "library": os.environ.get("CN_LIB_PATH") or "in-tree", "rounds": rounds}
    for e in engines:
        e.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
