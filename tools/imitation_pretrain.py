#!/usr/bin/env python
"""Behaviour-cloning pre-training of the DSRNN policy (or, with --policy convgru, of the ConvGRU policy on the live
LiDAR observation) from a scripted expert, with the evaluation rows next to it.

For every --sigma-frac f (the noise half-width as a fraction of robot.v_pref; 0 = plain behaviour cloning) a fresh
DSRNN policy (same initial weights) is cloned from the expert for --updates chunks with learner.BehaviourCloning
(noise-injected expert rollouts, labels clean) and then run through evaluate() on the default test set
(--test-size episodes, the four default test scenarios). The untrained policy and the expert itself
(evaluate_scripted) are evaluated the same way. One JSON line per row: success / collision / timeout rates, updates,
env steps, the last update's losses and the wall time of the training. --policy convgru runs all of it on an env with
robot.policy 'convgru', lidar.enable and lidar.live: the expert still acts on the full state, the cloned policy sees
the 180 ranges (the rollouts record them: cn_rollout_lidar), and the same three kinds of row are printed. --out saves the state_dict of the LAST
sigma's policy (keys as the reference checkpoints'), ready for RolloutTrainer / train.py to continue with PPO.
--human-nums 5 10 (DSRNN only) clones the expert on ONE env of varying human count (config.sim.human_nums) into a
policy built for the largest count, and evaluates every row per density: at each trained count and at --unseen (7),
on a plain test VecEnv of that count with a Policy of that size loaded from the same state_dict (as
tools/train_varied.py does); the expert row of a density is the expert on that plain env.
--kinematics unicycle runs all of it on the unicycle robot (config.robot.scripted_unicycle): the expert's velocity
goes through the tracking law on the device and the labels are the unicycle actions (dv, dtheta), each within
[-0.1, 0.1]. There the noise is given with --sigma, ABSOLUTE in those action units (0.1 is the whole range; --sigma-frac
is not read). --expert dwa (unicycle only) clones the dynamic-window controller made for that robot
(config.robot.scripted_dwa at policy_factory.DWA_DEFAULTS) instead of ORCA or the social force behind the tracking law.
--head lattice (unicycle only) gives every policy of the run the 64-way categorical head over that controller's grid
of actions (config.robot.action_head; policy.LatticeCategorical) in place of the Gaussian: dwa's labels are its
candidates themselves, a continuous label (ORCA or the social force through the law) is scored at its nearest one.
--fov F sets robot.FOV (in units of pi; the default config's is 2.0, the full circle) for training and evaluation
alike; --visible-masks (DSRNN only) also runs all of it on envs with sim.visible_masks and sim.visible_masks_scripted:
the rollouts record the 'visible_masks' rows (cn_rollout_masked) and the policy attends to the visible humans only.
--dagger replaces the rows per sigma by ONE row "dagger": the same fresh policy trained with learner.DAgger -- the learner
drives the envs, the expert labels every state it runs into -- with --beta (the probability that the expert's action is
the one executed in the first chunk), --beta-decay (its factor per chunk) and --aggregate (chunks held for the fit).
--soft-tau TAU (only with --dagger --expert dwa --head lattice) fits the head to the expert's 64 candidate costs -- the
target softmax(-regret / TAU), learner.DAgger's soft_tau -- instead of its one choice; every row carries soft_tau (null:
hard labels), the dagger row also the last update's soft_ce and kl, and its nll stays the hard label's.
Needs a GPU.

Usage: python tools/imitation_pretrain.py [--policy srnn|convgru] [--expert orca] [--updates 3000] [--envs 1024] [--steps 32] [--epochs 1]
           [--mini-batch 2] [--lr 1e-3] [--value-coef 0.5] [--sigma-frac 0 0.1 0.3] [--humans 5] [--seed 0]
           [--human-nums 5 10 [--unseen 7]] [--kinematics holonomic|unicycle [--sigma 0 0.03] [--head gaussian|lattice]]
           [--fov F] [--visible-masks] [--dagger [--beta 1.0] [--beta-decay 0.5] [--aggregate 1] [--soft-tau TAU]] [--eval-envs 100] [--test-size 500] [--log-every K] [--out policy.pt]
           [--json FILE]
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
from crowdnav_dsrnn_amd.learner import BehaviourCloning, DAgger  # noqa: E402
from crowdnav_dsrnn_amd.policy import Policy  # noqa: E402
from crowdnav_dsrnn_amd.policy_factory import ScriptedRobot  # noqa: E402

DEV = "cuda:0"


def rates(row):
    last = evaluate.last
    row.update({"success_rate": round(last["success_rate"], 3), "collision_rate": round(last["collision_rate"], 3),
                "timeout_rate": round(last["timeout_rate"], 3)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", default="srnn", choices=("srnn", "convgru"))
    ap.add_argument("--expert", default="orca", choices=ScriptedRobot.NAMES)
    ap.add_argument("--updates", type=int, default=3000)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--mini-batch", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--value-coef", type=float, default=0.5)
    ap.add_argument("--sigma-frac", type=float, nargs="+", default=[0.0, 0.1, 0.3])
    ap.add_argument("--kinematics", default="holonomic", choices=("holonomic", "unicycle"),
                    help="unicycle: clone the controller driving the unicycle robot through the tracking law")
    ap.add_argument("--sigma", type=float, nargs="+", default=[0.0, 0.03],
                    help="with --kinematics unicycle: the noise half-widths, absolute, in action units (0.1 is the "
                         "whole range of an action component); replaces --sigma-frac there")
    ap.add_argument("--head", default="gaussian", choices=Policy.HEADS,
                    help="the policy's action head; lattice (with --kinematics unicycle): a categorical over the 64 "
                         "unicycle actions the dwa expert chooses from")
    ap.add_argument("--humans", type=int, default=5)
    ap.add_argument("--human-nums", type=int, nargs="+", default=None,
                    help="clone on an env of varying human count; every row per density")
    ap.add_argument("--unseen", type=int, default=7, help="with --human-nums: a density the cloning never saw")
    ap.add_argument("--fov", type=float, default=None, help="robot.FOV in units of pi (default: the config's 2.0)")
    ap.add_argument("--visible-masks", action="store_true",
                    help="envs with sim.visible_masks + sim.visible_masks_scripted: the masked spatial attention")
    ap.add_argument("--dagger", action="store_true",
                    help="train with learner.DAgger (the learner in the loop) instead of BehaviourCloning: one row")
    ap.add_argument("--beta", type=float, default=1.0, help="with --dagger: the first chunk's expert probability")
    ap.add_argument("--beta-decay", type=float, default=0.5, help="with --dagger: beta's factor per chunk")
    ap.add_argument("--aggregate", type=int, default=1, help="with --dagger: chunks held for the fit")
    ap.add_argument("--soft-tau", type=float, default=None,
                    help="with --dagger --expert dwa --head lattice: fit the soft target softmax(-regret / TAU) of the "
                         "expert's 64 candidate costs instead of its choice")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eval-envs", type=int, default=100)
    ap.add_argument("--test-size", type=int, default=500)
    ap.add_argument("--log-every", type=int, default=0, help="print a progress line to stderr every K updates")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.soft_tau is not None and not (args.dagger and args.expert == "dwa" and args.head == "lattice"):
        raise SystemExit("imitation_pretrain: --soft-tau needs --dagger --expert dwa --head lattice")
    if not torch.cuda.is_available():
        raise SystemExit("imitation_pretrain: needs a GPU")
    if args.human_nums and args.policy != "srnn":
        raise SystemExit("imitation_pretrain: --human-nums is the DSRNN policy's (no LiDAR on a mixed engine)")
    if args.visible_masks and args.policy != "srnn":
        raise SystemExit("imitation_pretrain: --visible-masks is the DSRNN policy's (no human slots in the LiDAR row)")
    log = logging.getLogger("imitation_pretrain")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    c = clone_config(Config())
    c.sim.human_num = args.humans
    c.action_space.kinematics = args.kinematics
    uni = args.kinematics == "unicycle"
    c.robot.scripted_unicycle = uni
    if args.head == "lattice" and not uni:
        raise SystemExit("imitation_pretrain: --head lattice needs --kinematics unicycle")
    c.robot.action_head = args.head
    if args.fov is not None:
        c.robot.FOV = args.fov
    if args.visible_masks:
        c.sim.visible_masks = c.sim.visible_masks_scripted = True
    if args.expert == "dwa":
        if not uni:
            raise SystemExit("imitation_pretrain: --expert dwa needs --kinematics unicycle")
        c.robot.scripted_dwa = True   # (policy_factory.DWA_DEFAULTS)
    # (sigma, the fraction it was given as or None): holonomic in fractions of v_pref, unicycle absolute
    sigmas = [(s, None) for s in args.sigma] if uni else [(f * float(c.robot.v_pref), f) for f in args.sigma_frac]
    if args.policy == "convgru":
        c.robot.policy = "convgru"
        c.lidar.enable = True
        c.lidar.live = True
    c.env.test_size = args.test_size
    c.training.num_processes = args.envs
    c.ppo.num_steps = args.steps
    c.ppo.num_mini_batch = args.mini_batch
    E, EE = args.envs, args.eval_envs
    lines = []
    # the densities every row is evaluated at (one, the env's own, without --human-nums), and the training config
    densities = sorted(set(args.human_nums) | {args.unseen}) if args.human_nums else [args.humans]
    ct = clone_config(c)
    if args.human_nums:
        ct.sim.human_nums = list(args.human_nums)
        ct.sim.human_nums_scripted = True

    def emit(row):
        row = dict(row, fov=float(c.robot.FOV), visible_masks=bool(args.visible_masks), head=args.head,
                   soft_tau=args.soft_tau)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def density_config(n):
        cn = clone_config(c)
        cn.sim.human_num = n
        return cn

    def test_envs(cn):
        return CrowdNavVecEnv(cn, EE, cn.env.seed, DEV, allow_early_resets=True, nenv=EE, phase="test")

    def evaluate_policy(pol, row):
        """One row per density: the policy itself on its own env, or (--human-nums) a Policy of that size with the
        same state_dict on the plain test env of that count."""
        for n in densities:
            cn = density_config(n)
            envs = test_envs(cn)
            p = pol
            if args.human_nums:
                p = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=cn).to(DEV)
                p.load_state_dict(pol.state_dict())
                p.train(pol.training)
            keep = getattr(p.base, "nenv", None)   # (the DSRNN reads its batch shape from attributes)
            if keep is not None:
                p.base.nenv = EE
            try:
                evaluate(p, None, envs, EE, DEV, cn, log, keep_traces=False, verbose=False)
            finally:
                if keep is not None:
                    p.base.nenv = keep
                envs.close()
            emit(rates(dict(row, humans=n, **({"trained_on": args.human_nums} if args.human_nums else {}))))

    def fresh_policy(spaces, action_space, cfg):
        torch.manual_seed(args.seed)
        return Policy(spaces, action_space, base=args.policy, base_kwargs=cfg).to(DEV)

    for n in densities:
        envs = test_envs(density_config(n))
        evaluate_scripted(args.expert, envs, EE, DEV, density_config(n), log, keep_traces=False, verbose=False)
        emit(rates({"row": "expert", "policy": args.policy, "expert": args.expert, "humans": n,
                    "kinematics": args.kinematics,
                    "episodes": args.test_size}))
        envs.close()
    # the policy's spaces and size: the training env's (a varied env: the padded observation, the largest count)
    envs = CrowdNavVecEnv(ct, E, args.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
    spaces = envs.observation_space if args.policy == "convgru" else envs.observation_space.spaces
    action_space, cpol = envs.action_space, envs.config
    envs.close()
    evaluate_policy(fresh_policy(spaces, action_space, cpol), {"row": "untrained", "policy": args.policy,
                                                               "kinematics": args.kinematics,
                                                               "episodes": args.test_size})
    if args.dagger:
        pol = fresh_policy(spaces, action_space, cpol)
        envs = CrowdNavVecEnv(ct, E, args.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
        dg = DAgger(ct, envs, pol, expert=args.expert, beta=args.beta, beta_decay=args.beta_decay, seed=args.seed,
                    epochs=args.epochs, lr=args.lr, value_coef=args.value_coef, aggregate=args.aggregate,
                    soft_tau=args.soft_tau)
        torch.cuda.synchronize()
        t0 = time.time()
        gpu_roll = gpu_upd = 0.0
        first = st = None
        for u in range(args.updates):
            st = dg.update()
            first = first or st
            if args.log_every and (u + 1) % args.log_every == 0:
                print("dagger update %d beta %.4g nll %.4f value_loss %.4f agree %.4f took_expert %.4f"
                      % (u + 1, st["beta"], st["nll"], st["value_loss"], st["agree"], st["took_expert"]),
                      file=sys.stderr, flush=True)
            gpu_roll += st["rollout_s"]
            gpu_upd += st["update_s"]
        wall = time.time() - t0
        envs.close()
        evaluate_policy(pol, {"row": "dagger", "policy": args.policy, "expert": args.expert, "beta": args.beta,
                              "beta_decay": args.beta_decay, "aggregate": args.aggregate, "graphs": dg.graphs,
                              "kinematics": args.kinematics, "updates": args.updates, "envs": E, "steps": args.steps,
                              "epochs": args.epochs, "lr": args.lr, "env_steps": dg.env_steps,
                              "nll_first": round(first["nll"], 4), "nll_last": round(st["nll"], 4),
                              "value_loss_last": round(st["value_loss"], 4), "agree_first": round(first["agree"], 4),
                              "agree_last": round(st["agree"], 4), "took_expert_last": round(st["took_expert"], 4),
                              "beta_last": st["beta"], "train_wall_s": round(wall, 2),
                              **({"soft_ce_first": round(first["soft_ce"], 4), "soft_ce_last": round(st["soft_ce"], 4),
                                  "kl_first": round(first["kl"], 4), "kl_last": round(st["kl"], 4)}
                                 if args.soft_tau is not None else {}),
                              "rollout_gpu_s": round(gpu_roll, 3), "update_gpu_s": round(gpu_upd, 3),
                              "episodes": args.test_size})
    for sigma, frac in ([] if args.dagger else sigmas):
        pol = fresh_policy(spaces, action_space, cpol)
        envs = CrowdNavVecEnv(ct, E, args.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
        bc = BehaviourCloning(ct, envs, pol, expert=args.expert, sigma=sigma, seed=args.seed,
                              epochs=args.epochs, lr=args.lr, value_coef=args.value_coef)
        torch.cuda.synchronize()
        t0 = time.time()
        gpu_roll = gpu_upd = 0.0
        first = st = None
        for u in range(args.updates):
            st = bc.update()
            first = first or st
            if args.log_every and (u + 1) % args.log_every == 0:
                print("sigma %g update %d nll %.4f value_loss %.4f" % (sigma, u + 1, st["nll"], st["value_loss"]),
                      file=sys.stderr, flush=True)
            gpu_roll += st["rollout_s"]
            gpu_upd += st["update_s"]
        wall = time.time() - t0
        envs.close()
        evaluate_policy(pol, {"row": "bc", "policy": args.policy, "expert": args.expert, "sigma_frac": frac,
                              "sigma": sigma, "kinematics": args.kinematics,
                              "updates": args.updates, "envs": E, "steps": args.steps, "epochs": args.epochs, "lr": args.lr,
                              "env_steps": bc.env_steps, "nll_first": round(first["nll"], 4), "nll_last": round(st["nll"], 4),
                              "value_loss_last": round(st["value_loss"], 4), "train_wall_s": round(wall, 2),
                              "rollout_gpu_s": round(gpu_roll, 3), "update_gpu_s": round(gpu_upd, 3),
                              "episodes": args.test_size})
    if args.out:
        torch.save(pol.state_dict(), args.out)
    if args.json:
        with open(args.json, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
