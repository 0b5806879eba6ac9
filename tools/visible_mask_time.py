#!/usr/bin/env python
"""HIP-event timings of cn_visible_mask beside the step it follows.

Per shape (4096 envs x 10 humans and x 25 humans, holonomic ORCA, robot.FOV 0.5): 200 launches each of
  step          cn_step of that engine (random actions; auto-resets included)
  visible_mask  cn_visible_mask on the state the steps left
between two events on the current stream after 20 warm-up launches, three alternating rounds; the median round is
reported (us per launch) with the rounds' spread (the method of tools/lidar_live_time.py). Needs a GPU; prints one
JSON line per shape.

Usage: python tools/visible_mask_time.py [--envs 4096] [--launches 200] [--out FILE]
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
    ap.add_argument("--fov", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("visible_mask_time: needs a GPU")
    E = args.envs
    lines = []
    for N in (10, 25):
        c = clone_config(Config())
        c.sim.human_num = N
        c.action_space.kinematics = "holonomic"
        c.robot.FOV = args.fov
        eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
        eng.reset()
        g = torch.Generator(device="cuda:0").manual_seed(1)
        acts = torch.randn((E, 2), generator=g, device="cuda:0") * 0.5
        out = torch.zeros((E, N), device="cuda:0")
        fns = {"step": lambda: eng.step(acts), "visible_mask": lambda: eng.visible_mask(out)}
        rounds = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, args.launches))
        rec = {"envs": E, "humans": N, "robot_fov": args.fov, "launches": args.launches,
               "unit": "us per launch (HIP events)", "device": torch.cuda.get_device_name(0),
               "visible_share": round(float(out.mean()), 4)}
        for k, v in rounds.items():
            v = sorted(v)
            rec[k] = round(v[1], 2)
            rec[k + "_min_max"] = [round(v[0], 2), round(v[2], 2)]
        rec["mask_over_step"] = round(rec["visible_mask"] / rec["step"], 4)
        eng.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
