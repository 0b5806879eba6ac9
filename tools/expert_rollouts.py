#!/usr/bin/env python
"""Expert demonstrations of a scripted robot ('orca' / 'social_force') as an .npz file.

E envs are reset and driven for T steps by ScriptedRobot.rollout (cn_rollout: where the engine allows it the
controller runs inside the multi-step launches, so a trajectory costs about T / 32 launches and no host round
trip). The file holds

  robot_node      (T + 1, E, 1, 7)   observation rows: row 0 is the reset observation, row t + 1 the observation
  temporal_edges  (T + 1, E, 1, 2)   after step t (the new episode's first one where `done[t]`)
  spatial_edges   (T + 1, E, N, 2)
  actions         (T, E, 2)          the controller's action of step t
  reward, done, event  (T, E)        of step t
  pairing         'obs[t] -> actions[t]'

i.e. with the reset observation stored in front, the imitation pair of step t is (observation row t, actions row
t): the action was computed from the state that observation shows (in cn_rollout's own row numbering, where row -1
is the reset observation: obs[t-1] -> actions[t]). The controller reads the engine's state, not the float32
observation: its belief of the humans (the spatial edges) and its own full state. A behaviour-cloning trainer is
not part of the project.

Usage: python tools/expert_rollouts.py --out demos.npz [--robot orca] [--envs 256] [--steps 512] [--humans 5]
                                       [--seed 0] [--chunk-steps 128]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, clone_config  # noqa: E402
from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv  # noqa: E402
from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot  # noqa: E402

OBS = ("robot_node", "temporal_edges", "spatial_edges")
STEP = ("actions", "reward", "done", "event")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--robot", default="orca", choices=ScriptedRobot.NAMES)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chunk-steps", type=int, default=128, help="steps per rollout call (bounds the device buffers)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expert_rollouts: needs a GPU")
    c = clone_config(Config())
    c.sim.human_num = args.humans
    c.action_space.kinematics = "holonomic"
    E, T = args.envs, args.steps
    envs = CrowdNavVecEnv(c, E, args.seed, "cuda:0", allow_early_resets=True, nenv=E, phase="train")
    robot = ScriptedRobot(envs, args.robot)
    obs0 = envs.reset()
    rows = {k: [obs0[k].reshape((1,) + tuple(obs0[k].shape)).cpu().numpy()] for k in OBS}
    rows.update({k: [] for k in STEP})
    launches, t = 0, 0
    while t < T:
        n = min(args.chunk_steps, T - t)
        out = robot.rollout(n)
        launches += out["num_launches"]
        torch.cuda.synchronize()
        for k in OBS + STEP:
            rows[k].append(out[k].cpu().numpy())
        t += n
    data = {k: np.concatenate(v, axis=0) for k, v in rows.items()}
    data["pairing"] = np.array("obs[t] -> actions[t]")
    data["robot"] = np.array(args.robot)
    np.savez_compressed(args.out, **data)
    print("%s: %d envs x %d steps of %r, %d episodes ended, %d kernel launches"
          % (args.out, E, T, args.robot, int(data["done"].sum()), launches))
    envs.close()


if __name__ == "__main__":
    main()
