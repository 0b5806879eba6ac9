#!/usr/bin/env python
"""Expert demonstrations of a scripted robot ('orca' / 'social_force') as an .npz file.

E envs are reset and driven for T steps by ScriptedRobot.rollout (cn_rollout: where the engine allows it the
controller runs inside the multi-step launches, so a trajectory costs about T / 32 launches and no host round
trip). The file holds

  robot_node      (T + 1, E, 1, 7)   observation rows: row 0 is the reset observation, row t + 1 the observation
  temporal_edges  (T + 1, E, 1, 2)   after step t (the new episode's first one where `done[t]`)
  spatial_edges   (T + 1, E, N, 2)
  actions         (T, E, 2)          the controller's action of step t (with --noise-sigma: the clean label)
  executed        (T, E, 2)          with --noise-sigma only: the perturbed action the step took
  reward, done, event  (T, E)        of step t
  pairing         'obs[t] -> actions[t]'

i.e. with the reset observation stored in front, the imitation pair of step t is (observation row t, actions row
t): the action was computed from the state that observation shows (in cn_rollout's own row numbering, where row -1
is the reset observation: obs[t-1] -> actions[t]). The controller reads the engine's state, not the float32
observation: its belief of the humans (the spatial edges) and its own full state. learner.BehaviourCloning trains on
the same rollouts straight from the device buffers (tools/imitation_pretrain.py); this file is for other consumers.

--lidar records LiDAR demonstrations for the ConvGRU policy: the env runs with robot.policy 'convgru', lidar.enable and
lidar.live, and the file also holds (cn_rollout_lidar)

  lidar           (T + 1, E, 1, 7 + beams)   the live LiDAR observation, rows as above (pair: lidar[t] -> actions[t])
  robot_state     (9, T, E)          the state step t left, float64: r_px, r_py, r_vx, r_vy, r_radius, r_gx, r_gy,
  human_state     (3, T, E, N)       r_vpref, r_theta and h_px, h_py, h_r -- what the scan of row t + 1 was taken from
  lidar_beams, lidar_max_range, lidar_robot_radius

--noise-sigma S (m/s) injects noise: the steps take actions + S * uniform[-1, 1) per component (cn_rollout_noisy, seed
--noise-seed), the labels stay clean; the chunks continue one noise sequence (step0 = steps done so far).

--kinematics unicycle drives the unicycle robot (config.robot.scripted_unicycle): `actions` holds the unicycle action
(dv, dtheta) the tracking law derives from the controller's velocity, each within [-0.1, 0.1], and --noise-sigma is
ABSOLUTE in those action units (0.1 is the whole range); the step clips the perturbed action. --robot dwa (unicycle
only) records the dynamic-window controller (config.robot.scripted_dwa), whose actions are grid points of that range.

--visible-masks (with --fov F, robot.FOV in units of pi) records on an env with sim.visible_masks and
sim.visible_masks_scripted: the file also holds (cn_rollout_masked)

  visible_masks   (T + 1, E, N)      1.0 for the humans the robot sees in the state of that observation row

Usage: python tools/expert_rollouts.py --out demos.npz [--robot orca] [--envs 256] [--steps 512] [--humans 5]
                                       [--seed 0] [--chunk-steps 128] [--noise-sigma S] [--noise-seed K] [--lidar]
                                       [--kinematics holonomic|unicycle] [--fov F] [--visible-masks]
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
    ap.add_argument("--noise-sigma", type=float, default=None, help="perturb the executed action (labels stay clean); m/s, or with --kinematics unicycle absolute in "
                         "action units, where 0.1 is the whole range")
    ap.add_argument("--noise-seed", type=int, default=0)
    ap.add_argument("--kinematics", default="holonomic", choices=("holonomic", "unicycle"),
                    help="unicycle: the controller drives the unicycle robot through the tracking law")
    ap.add_argument("--lidar", action="store_true", help="record the live LiDAR observation and the state rows as well")
    ap.add_argument("--fov", type=float, default=None, help="robot.FOV in units of pi (default: the config's 2.0)")
    ap.add_argument("--visible-masks", action="store_true", help="record the 'visible_masks' rows as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expert_rollouts: needs a GPU")
    c = clone_config(Config())
    c.sim.human_num = args.humans
    c.action_space.kinematics = args.kinematics
    c.robot.scripted_unicycle = args.kinematics == "unicycle"
    if args.robot == "dwa":
        if args.kinematics != "unicycle":
            raise SystemExit("expert_rollouts: --robot dwa needs --kinematics unicycle")
        c.robot.scripted_dwa = True   # (policy_factory.DWA_DEFAULTS)
    if args.fov is not None:
        c.robot.FOV = args.fov
    if args.visible_masks:
        if args.lidar:
            raise SystemExit("expert_rollouts: --visible-masks is not for --lidar (no human slots to mask)")
        c.sim.visible_masks = c.sim.visible_masks_scripted = True
    if args.lidar:
        c.robot.policy = "convgru"
        c.lidar.enable = True
        c.lidar.live = True
    E, T = args.envs, args.steps
    envs = CrowdNavVecEnv(c, E, args.seed, "cuda:0", allow_early_resets=True, nenv=E, phase="train")
    robot = ScriptedRobot(envs, args.robot)
    obs0 = envs.reset()
    if args.lidar:   # (the env's observation is the LiDAR row; the SRNN one of the same state is the engine's own)
        rows = {"lidar": [obs0.reshape((1,) + tuple(obs0.shape)).cpu().numpy()]}
        obs0 = envs.engine.obs()
    else:
        rows = {}
    obs_keys = OBS + (("visible_masks",) if args.visible_masks else ())
    rows.update({k: [obs0[k].reshape((1,) + tuple(obs0[k].shape)).cpu().numpy()] for k in obs_keys})
    step_keys = STEP + (("executed",) if args.noise_sigma is not None else ())
    state_keys = ("robot_state", "human_state") if args.lidar else ()
    rows.update({k: [] for k in step_keys + state_keys})
    launches, t = 0, 0
    while t < T:
        n = min(args.chunk_steps, T - t)
        if args.noise_sigma is None:
            out = robot.rollout(n)
        else:
            out = robot.rollout(n, noise={"sigma": args.noise_sigma, "seed": args.noise_seed, "step0": t})
        launches += out["num_launches"]
        torch.cuda.synchronize()
        for k in obs_keys + step_keys + state_keys + (("lidar",) if args.lidar else ()):
            rows[k].append(out[k].cpu().numpy())
        t += n
    data = {k: np.concatenate(v, axis=1 if k in state_keys else 0) for k, v in rows.items()}
    if args.lidar:
        lc = c.lidar.cfg
        data["lidar_beams"], data["lidar_max_range"] = np.array(int(lc["num_beams"])), np.array(float(lc["max_range"]))
        data["lidar_robot_radius"] = np.array(float(lc["robot_radius"]))
    data["pairing"] = np.array("obs[t] -> actions[t]")
    data["robot"] = np.array(args.robot)
    data["kinematics"] = np.array(args.kinematics)
    if args.noise_sigma is not None:
        data["noise_sigma"], data["noise_seed"] = np.array(args.noise_sigma), np.array(args.noise_seed)
    np.savez_compressed(args.out, **data)
    print("%s: %d envs x %d steps of %r, %d episodes ended, %d kernel launches"
          % (args.out, E, T, args.robot, int(data["done"].sum()), launches))
    envs.close()


if __name__ == "__main__":
    main()
