#!/usr/bin/env python
"""Parameter grid of the unicycle robot's dynamic-window controller ('dwa', policy_factory.dwa_predict).

Every combination of --horizon x --w-clear x --d-safe (w_goal and w_col fixed) is run through evaluate_scripted on
--episodes episodes of the VALIDATION phase of the default unicycle config (5 humans, the default scenarios, robot
invisible to the humans) -- not the test episodes the baseline rows and tests/test_dwa.py report on. One JSON line per
combination: the parameters, success / collision / timeout rates, the mean navigation time of the successful episodes
and the wall time; then a line {"selected": ...} with the combination of the highest success rate (ties: the lower
collision rate, then the earlier row). policy_factory.DWA_DEFAULTS holds the selected row. Needs a GPU.

Usage: python tools/dwa_grid.py [--horizon 6 8 12] [--w-clear 0.5 1 2] [--d-safe 0.3 0.5] [--w-goal 1] [--w-col 100]
           [--envs 100] [--episodes 500] [--humans 5] [--out FILE]
"""
import argparse
import itertools
import json
import logging
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, clone_config  # noqa: E402
from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv  # noqa: E402
from crowdnav_dsrnn_amd.evaluation import evaluate, evaluate_scripted  # noqa: E402
from crowdnav_dsrnn_amd.policy_factory import dwa_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, nargs="+", default=[6, 8, 12])
    ap.add_argument("--w-clear", type=float, nargs="+", default=[0.5, 1.0, 2.0])
    ap.add_argument("--d-safe", type=float, nargs="+", default=[0.3, 0.5])
    ap.add_argument("--w-goal", type=float, default=1.0)
    ap.add_argument("--w-col", type=float, default=100.0)
    ap.add_argument("--envs", type=int, default=100)
    ap.add_argument("--episodes", type=int, default=500)
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwa_grid: needs a GPU")
    log = logging.getLogger("dwa_grid")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    lines, rows = [], []
    E = args.envs
    for H, wc, ds in itertools.product(args.horizon, args.w_clear, args.d_safe):
        p = dwa_params({"horizon": H, "w_goal": args.w_goal, "w_clear": wc, "d_safe": ds, "w_col": args.w_col})
        c = clone_config(Config())
        c.sim.human_num = args.humans
        c.action_space.kinematics = "unicycle"
        c.robot.scripted_dwa = p
        # (the recorder counts config.env.test_size episodes; the phase's own case size is val_size)
        c.env.test_size = c.env.val_size = args.episodes
        envs = CrowdNavVecEnv(c, E, c.env.seed, "cuda:0", allow_early_resets=True, nenv=E, phase="val")
        t0 = time.time()
        evaluate_scripted("dwa", envs, E, "cuda:0", c, log, keep_traces=False, verbose=False)
        wall = time.time() - t0
        envs.close()
        last = evaluate.last
        row = {"dwa": p, "phase": "val", "episodes": args.episodes, "humans": args.humans, "envs": E,
               "success_rate": round(last["success_rate"], 3), "collision_rate": round(last["collision_rate"], 3),
               "timeout_rate": round(last["timeout_rate"], 3),
               "nav_time_mean_s": round(float(last["metrics"]["navigation time"][0]), 2), "wall_s": round(wall, 2)}
        rows.append(row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    best = max(range(len(rows)), key=lambda k: (rows[k]["success_rate"], -rows[k]["collision_rate"], -k))
    lines.append(json.dumps({"selected": rows[best]["dwa"], "row": best, "success_rate": rows[best]["success_rate"]}))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
