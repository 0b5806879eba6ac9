#!/usr/bin/env python
"""The scripted-robot baseline rows: evaluate() with policy_factory.ScriptedRobot ('orca', 'social_force', 'dwa').

The reference's default test configuration (crowd_nav/configs/config.py: 500 test episodes, 5 ORCA humans,
holonomic robot, circle radius 6, the four default test scenarios -- taken round-robin by env here, where the
reference draws one per reset with the unseeded `random` module), with the robot invisible to the humans (the
default) and visible. The robot acts on its belief of the humans, every step computed on the device
(cn_robot_act); no host round trip except evaluate()'s own end-of-run check every 8 steps.
Prints one JSON line per (policy, visibility): success / collision / timeout rates, the mean navigation time of
the successful episodes and the wall time of the run. Needs a GPU.

--rollout runs the same evaluation on whole rollouts (evaluate_scripted -> cn_rollout: the controller inside the
multi-step launches, every step recorded, the end-of-run check once per chunk); the per-episode records, and so the
rows, are the same.

--human-nums 5 10 runs it on ONE env of varying human count (config.sim.human_nums; env g has
human_nums[g % len] humans) and prints, after each overall row, one row per distinct count from the report's
per-count block (evaluate.last["per_count"]).

--kinematics unicycle runs it on the unicycle robot (config.robot.scripted_unicycle: the controller's velocity goes
through the tracking law on the device, policy_factory.unicycle_track), on either loop, and adds the rows of 'dwa',
the dynamic-window controller of the unicycle robot (config.robot.scripted_dwa; policy_factory.dwa_predict).
--robots restricts the run to some controllers; --dwa '{"horizon": 12}' overrides policy_factory.DWA_DEFAULTS;
--phase val evaluates the validation episodes (the same count, what the defaults were selected on) instead of the test
episodes; --visible 0 / 1 restricts the run to one visibility.

--fov F sets robot.FOV (in units of pi; default 2.0, the full circle). --visible-masks runs on an env with
sim.visible_masks and sim.visible_masks_scripted (the rollouts then record the mask as well, cn_rollout_masked); a
scripted robot does not read the mask, so the rows are those of the same env without it.

Usage: python tools/baseline_eval.py [--envs 100] [--test-size 500] [--humans 5 | --human-nums 5 10] [--rollout]
           [--kinematics holonomic|unicycle] [--robots orca dwa] [--dwa JSON] [--phase test|val] [--visible 0|1]
           [--fov F] [--visible-masks] [--out FILE]
"""
import argparse
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
from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot, dwa_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=100)
    ap.add_argument("--test-size", type=int, default=500)
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--human-nums", type=int, nargs="+", default=None,
                    help="an env of varying human count (one mixed engine); adds the per-count rows")
    ap.add_argument("--rollout", action="store_true", help="evaluate on whole rollouts (evaluate_scripted)")
    ap.add_argument("--kinematics", default="holonomic", choices=("holonomic", "unicycle"),
                    help="unicycle: the controllers drive the unicycle robot through the tracking law")
    ap.add_argument("--robots", nargs="+", default=None, choices=ScriptedRobot.NAMES,
                    help="the controllers to run (default: all the kinematics serves)")
    ap.add_argument("--dwa", default=None, help="JSON dict of overrides of policy_factory.DWA_DEFAULTS")
    ap.add_argument("--phase", default="test", choices=("test", "val"))
    ap.add_argument("--visible", type=int, default=None, choices=(0, 1))
    ap.add_argument("--fov", type=float, default=None, help="robot.FOV in units of pi (default: the config's 2.0)")
    ap.add_argument("--visible-masks", action="store_true",
                    help="an env with sim.visible_masks + sim.visible_masks_scripted")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    uni = args.kinematics == "unicycle"
    names = args.robots or [n for n in ScriptedRobot.NAMES if uni or n != "dwa"]
    dwa = json.loads(args.dwa) if args.dwa else True
    if not torch.cuda.is_available():
        raise SystemExit("baseline_eval: needs a GPU")
    log = logging.getLogger("baseline_eval")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    lines = []
    for visible in ((False, True) if args.visible is None else (bool(args.visible),)):
        for name in names:
            c = clone_config(Config())
            c.sim.human_num = args.humans
            if args.human_nums:
                c.sim.human_nums = list(args.human_nums)
                c.sim.human_nums_scripted = True
            c.env.test_size = c.env.val_size = args.test_size
            c.robot.visible = visible
            if args.fov is not None:
                c.robot.FOV = args.fov
            if args.visible_masks:
                c.sim.visible_masks = c.sim.visible_masks_scripted = True
            c.action_space.kinematics = args.kinematics
            c.robot.scripted_unicycle = uni
            c.robot.scripted_dwa = dwa if uni and name == "dwa" else None
            E = args.envs
            envs = CrowdNavVecEnv(c, E, c.env.seed, "cuda:0", allow_early_resets=True, nenv=E, phase=args.phase)
            t0 = time.time()
            if args.rollout:
                evaluate_scripted(name, envs, E, "cuda:0", c, log, keep_traces=False, verbose=False)
            else:
                evaluate(ScriptedRobot(envs, name), None, envs, E, "cuda:0", c, log, keep_traces=False, verbose=False)
            wall = time.time() - t0
            last = evaluate.last
            nav = last["metrics"]["navigation time"]
            envs.close()
            rec = {"robot": name, "robot_visible": visible, "kinematics": args.kinematics, "humans": args.human_nums or args.humans,
                   "episodes": args.test_size,
                   "envs": E, "path": "rollout" if args.rollout else "step",
                   "counts": {k: int(v["total"]) for k, v in last["num_events"].items()},
                   "success_rate": round(last["success_rate"], 3),
                   "collision_rate": round(last["collision_rate"], 3), "timeout_rate": round(last["timeout_rate"], 3),
                   "nav_time_mean_s": round(float(nav[0]), 2), "nav_time_std_s": round(float(nav[1]), 2),
                   "wall_s": round(wall, 2)}
            if args.fov is not None or args.visible_masks:
                rec["fov"], rec["visible_masks"] = float(c.robot.FOV), bool(args.visible_masks)
            if name == "dwa":
                rec["dwa"] = dwa_params(dwa)
            if args.phase != "test":
                rec["phase"] = args.phase
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            for n, v in (last.get("per_count") or {}).items():
                lines.append(json.dumps({"robot": name, "robot_visible": visible, "humans": n, "of": args.human_nums,
                                         "episodes": v["episodes"], "path": rec["path"],
                                         "success_rate": round(v["success_rate"], 3),
                                         "collision_rate": round(v["collision_rate"], 3),
                                         "timeout_rate": round(v["timeout_rate"], 3)}))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
