#!/usr/bin/env python
"""HIP-event timings of closed-loop scripted rollouts (cn_rollout) against the launch pairs they replace.

Per configuration (4096 envs, T = 256 steps, holonomic, ORCA humans): (a) 5 humans, ORCA robot; (b) 9 humans, ORCA
robot; (c) 10 humans, social-force robot; (d) 5 humans, social-force robot. Three paths over the same T steps, every
step recorded:
  fused         cn_rollout at the default chunk: the controller inside the multi-step launches
  native_pairs  cn_rollout at chunk 1: cn_robot_act + cn_step launch pairs issued from native code
  python_pairs  the Python loop of robot_act() + step() (what the library offered before cn_rollout; its outputs are
                not kept per step, so it does strictly less)
between two events on the current stream after one warm-up rollout, three alternating rounds; the median round
is reported (us per step) with the rounds' spread. Needs a GPU; prints one JSON line per configuration.
--noise-sigma S runs the two cn_rollout paths through cn_rollout_noisy with that sigma (0: its cn_rollout path plus the
copy into `executed`); the Python loop stays the clean one.

--kinematics unicycle times the same paths on the unicycle robot (the engine's cn_scripted_unicycle opt-in: the
tracking law between the controller and the step); --configs a b restricts the run to some configurations.
Two more configurations exist there and run only when named: (e) 5 humans and (f) 9 humans with the dynamic-window
controller 'dwa' (cn_scripted_dwa at policy_factory.DWA_DEFAULTS). It always runs as launch pairs, so `fused` equals
`native_pairs` for it; its rows gain `robot_act_only`, T controller launches alone, for the controller's share.

--mask (with --fov F, robot.FOV in units of pi, default 0.5 then) times the masked rollout (cn_rollout_masked: the
'visible_masks' rows recorded by the rollout launches themselves) on both cn_rollout paths and adds two rows per
configuration: `fused_unmasked`, the same engine's cn_rollout without the mask, and `python_triple`, the Python loop
robot_act() + step() + visible_mask().

Usage: python tools/rollout_time.py [--envs 4096] [--steps 256] [--noise-sigma S] [--kinematics holonomic|unicycle]
           [--configs a b c d e f] [--fov F] [--mask] [--out FILE]
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
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--noise-sigma", type=float, default=None)
    ap.add_argument("--kinematics", default="holonomic", choices=("holonomic", "unicycle"))
    ap.add_argument("--configs", nargs="+", default=["a", "b", "c", "d"], choices=("a", "b", "c", "d", "e", "f"))
    ap.add_argument("--fov", type=float, default=None, help="robot.FOV in units of pi (default: the config's 2.0)")
    ap.add_argument("--mask", action="store_true", help="time the masked rollout (cn_rollout_masked)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_time: needs a GPU")
    E, T = args.envs, args.steps
    lines = []
    noise = None if args.noise_sigma is None else {"sigma": args.noise_sigma, "seed": 1, "step0": 0}
    kw = {} if noise is None else {"noise": noise}
    fov = args.fov if args.fov is not None else (0.5 if args.mask else None)
    for tag, N, name in (("a", 5, "orca"), ("b", 9, "orca"), ("c", 10, "social_force"), ("d", 5, "social_force"),
                         ("e", 5, "dwa"), ("f", 9, "dwa")):
        if tag not in args.configs:
            continue
        if name == "dwa" and args.kinematics != "unicycle":
            raise SystemExit("rollout_time: configurations e and f (dwa) need --kinematics unicycle")
        c = clone_config(Config())
        c.sim.human_num = N
        c.action_space.kinematics = args.kinematics
        c.humans.policy = "orca"
        if fov is not None:
            c.robot.FOV = fov
        eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
        if args.kinematics == "unicycle":
            eng.scripted_unicycle(True)
        if name == "dwa":
            eng.scripted_dwa(True)
        chunk = eng.seq_chunk
        eng.reset()
        eng.step(eng.robot_act(name))   # (the first step after cn_reset is a pair on every path)
        buf = eng.rollout_buffers(T, **({} if noise is None else {"executed": True}))
        mbuf = eng.rollout_buffers(T, mask=True, **({} if noise is None else {"executed": True})) if args.mask else buf
        launches = {}

        def fused():
            eng.set_seq_chunk(chunk)
            launches["fused"] = eng.rollout(name, T, out=mbuf, **kw)["num_launches"]

        def native_pairs():
            eng.set_seq_chunk(1)
            launches["native_pairs"] = eng.rollout(name, T, out=mbuf, **kw)["num_launches"]

        def fused_unmasked():
            eng.set_seq_chunk(chunk)
            launches["fused_unmasked"] = eng.rollout(name, T, out=buf, **kw)["num_launches"]

        def python_triple():
            for _ in range(T):
                eng.step(eng.robot_act(name))
                eng.visible_mask()
            launches["python_triple"] = 3 * T

        def python_pairs():
            for _ in range(T):
                eng.step(eng.robot_act(name))
            launches["python_pairs"] = 2 * T

        def robot_act_only():
            for _ in range(T):
                eng.robot_act(name)
            launches["robot_act_only"] = T

        fns = {"fused": fused, "native_pairs": native_pairs, "python_pairs": python_pairs}
        if name == "dwa":
            fns["robot_act_only"] = robot_act_only
        if args.mask:
            fns["fused_unmasked"], fns["python_triple"] = fused_unmasked, python_triple
        rounds = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, T))
        rec = {"config": tag, "kinematics": args.kinematics, "envs": E, "humans": N, "robot": name, "steps": T, "chunk": chunk,
               "noise_sigma": args.noise_sigma, "fov": fov, "mask": bool(args.mask),
               "unit": "us per step (HIP events)", "device": torch.cuda.get_device_name(0), "launches": launches}
        for k, v in rounds.items():
            v = sorted(v)
            rec[k] = round(v[1], 2)
            rec[k + "_min_max"] = [round(v[0], 2), round(v[2], 2)]
        rec["fused_over_native_pairs"] = round(rec["fused"] / rec["native_pairs"], 3)
        rec["fused_over_python_pairs"] = round(rec["fused"] / rec["python_pairs"], 3)
        eng.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
