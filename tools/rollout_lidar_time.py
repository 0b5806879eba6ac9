#!/usr/bin/env python
"""HIP-event timings of scripted rollouts that record the live LiDAR observation (cn_rollout_lidar) against the
eager triple they replace, and of the plain rollout beside them.

Per shape (4096 envs, 180 beams / range 5, holonomic, ORCA humans, ORCA robot at 5, 9 and 10 humans; at 10 humans
ORCA's 11 agents leave the step's quad path, so the rollout is launch triples from native code there), 200 steps each:
  eager_triple   the Python loop robot_act() -> step() -> lidar_scan(): three launches per step, the one closed loop
                 that produced LiDAR rows before (its rows are not kept per step, so it does strictly less)
  rollout_lidar  rollout(lidar=): every step recorded, the state rows and the scan of all T * E rows included
  rollout        rollout() without lidar: every step recorded (cn_rollout)
between two events on the current stream after one warm-up pass, three alternating rounds; the median round is
reported (us per step) with the rounds' spread. Needs a GPU; prints one JSON line per shape.
--plain-only times `rollout` alone: with CN_LIB_PATH aimed at a library built from another revision this gives that
revision's figure for the same shapes.

Usage: python tools/rollout_lidar_time.py [--envs 4096] [--steps 200] [--beams 180] [--plain-only] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config  # noqa: E402
from crowdnav_dsrnn_amd.engine import CrowdNavEngine  # noqa: E402


def timed(fn, steps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps      # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--beams", type=int, default=180)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_lidar_time: needs a GPU")
    E, T, B = args.envs, args.steps, args.beams
    lidar = dict(beams=B, max_range=5.0, robot_radius=0.3)
    lines = []
    for N in (5, 9, 10):
        c = clone_config(Config())
        c.sim.human_num = N
        c.action_space.kinematics = "holonomic"
        c.humans.policy = "orca"
        eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
        eng.reset()
        eng.step(eng.robot_act("orca"))   # (the first step after cn_reset is launched singly on every path)
        plain = eng.rollout_buffers(T)
        launches = {}

        def rollout():
            launches["rollout"] = eng.rollout("orca", T, out=plain)["num_launches"]

        fns = {"rollout": rollout}
        if not args.plain_only:
            row = torch.zeros((E, 1, 7 + B), device="cuda:0")
            buf = eng.rollout_buffers(T, lidar=lidar)

            def eager_triple():
                for _ in range(T):
                    eng.step(eng.robot_act("orca"))
                    eng.lidar_scan(row, **lidar)
                launches["eager_triple"] = 3 * T

            def rollout_lidar():
                launches["rollout_lidar"] = eng.rollout("orca", T, out=buf, lidar=lidar)["num_launches"]

            fns = {"eager_triple": eager_triple, "rollout_lidar": rollout_lidar, "rollout": rollout}
        rounds = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, T))
        rec = {"envs": E, "humans": N, "robot": "orca", "beams": B, "steps": T, "chunk": eng.seq_chunk,
               "unit": "us per step (HIP events)", "device": torch.cuda.get_device_name(0), "launches": launches,
               "library": os.environ.get("CN_LIB_PATH") or "in-tree"}
        for k, v in rounds.items():
            v = sorted(v)
            rec[k] = round(v[1], 2)
            rec[k + "_min_max"] = [round(v[0], 2), round(v[2], 2)]
        if not args.plain_only:
            rec["rollout_lidar_over_eager_triple"] = round(rec["rollout_lidar"] / rec["eager_triple"], 3)
        eng.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
