#!/usr/bin/env python
"""HIP-event timings of the scripted robot (cn_robot_act) beside the step it drives.

Per shape (4096 envs x 5 humans: the quad path, A = 6 agents; 4096 x 10 humans: the kd-tree path, A = 11;
holonomic ORCA humans): 200 launches each of
  step              cn_step of that engine (random actions; auto-resets included)
  robot_orca        cn_robot_act(CN_ROBOT_ORCA) on the state the steps left
  robot_social_force  cn_robot_act(CN_ROBOT_SOCIAL_FORCE) on the same state
between two events on the current stream after 20 warm-up launches, three alternating rounds; the median
round is reported (us per launch) with the rounds' spread. Needs a GPU; prints one JSON line per shape.

Usage: python tools/robot_act_time.py [--envs 4096] [--launches 200] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config  # noqa: E402
from crowdnav_dsrnn_amd.engine import CrowdNavEngine  # noqa: E402


def timed(fn, launches, warmup=20):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches      # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robot_act_time: needs a GPU")
    E = args.envs
    lines = []
    for N in (5, 10):
        c = clone_config(Config())
        c.sim.human_num = N
        c.action_space.kinematics = "holonomic"
        eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
        eng.reset()
        g = torch.Generator(device="cuda:0").manual_seed(1)
        acts = torch.randn((E, 2), generator=g, device="cuda:0") * 0.5
        out = torch.zeros((E, 2), device="cuda:0")
        fns = {"step": lambda: eng.step(acts),
               "robot_orca": lambda: eng.robot_act("orca", out),
               "robot_social_force": lambda: eng.robot_act("social_force", out)}
        rounds = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, args.launches))
        rec = {"envs": E, "humans": N, "orca_path": "quad" if N + 1 <= 10 else "kd", "launches": args.launches,
               "unit": "us per launch (HIP events)", "device": torch.cuda.get_device_name(0)}
        for k, v in rounds.items():
            v = sorted(v)
            rec[k] = round(v[1], 2)
            rec[k + "_min_max"] = [round(v[0], 2), round(v[2], 2)]
        rec["orca_over_step"] = round(rec["robot_orca"] / rec["step"], 3)
        rec["social_force_over_step"] = round(rec["robot_social_force"] / rec["step"], 3)
        eng.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
