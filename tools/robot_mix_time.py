#!/usr/bin/env python
"""HIP-event timings of cn_robot_mix beside the cn_robot_act launch it contains.

cn_robot_mix is cn_robot_act's launch plus one launch of the mix kernel (the coin and the select), so the mix kernel
alone is the difference of the two. Per expert on 4096 envs x 5 humans (ORCA and the social force on a holonomic
engine, the dynamic window on a unicycle one), 1000 launches each of
  robot_act   cn_robot_act(expert) on the state a few random steps left
  robot_mix   cn_robot_mix(expert) on the same state, beta 0.5
between two events on the current stream after 20 warm-up launches, three alternating rounds; the median round is
reported (us per call) with the rounds' spread -- once issued eagerly from Python, where a call shorter than the host's
issue time measures the host, and once as replays of one captured graph of all the launches, where it does not.
Needs a GPU; prints one JSON line per expert.

Usage: python tools/robot_mix_time.py [--envs 4096] [--launches 1000] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config  # noqa: E402
from crowdnav_dsrnn_amd.engine import CrowdNavEngine  # noqa: E402


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robot_mix_time: needs a GPU")
    E, L = args.envs, args.launches
    lines = []
    for expert, kin in (("orca", "holonomic"), ("social_force", "holonomic"), ("dwa", "unicycle")):
        c = clone_config(Config())
        c.sim.human_num = 5
        c.action_space.kinematics = kin
        eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0", scripted_dwa=True if expert == "dwa" else None)
        eng.reset()
        g = torch.Generator(device="cuda:0").manual_seed(1)
        for _ in range(8):
            eng.step(torch.randn((E, 2), generator=g, device="cuda:0") * 0.1)
        learner = torch.randn((E, 2), generator=g, device="cuda:0") * 0.1
        label, executed = torch.zeros((E, 2), device="cuda:0"), torch.zeros((E, 2), device="cuda:0")
        flags = torch.zeros((E,), dtype=torch.uint8, device="cuda:0")
        ctl = eng.set_mix_ctl(eng.mix_ctl(), 0.5, 1, 0)

        def act():
            eng.robot_act(expert, label)

        def mix(t=0):
            eng.robot_mix(expert, learner, ctl, t, label=label, executed=executed, flags=flags)

        def loop(fn):
            return lambda: [fn() for _ in range(L)]

        fns = {"robot_act": loop(act), "robot_mix": loop(mix)}
        for k, one in (("robot_act", act), ("robot_mix", mix)):
            for _ in range(20):
                one()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(L):
                    one()
            gr.replay()   # (the first replay uploads the graph)
            fns[k + "_graph"] = gr.replay
        rounds = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, L))
        rec = {"envs": E, "humans": 5, "expert": expert, "kinematics": kin, "launches": L,
               "unit": "us per call (HIP events)", "device": torch.cuda.get_device_name(0)}
        for k, v in rounds.items():
            v = sorted(v)
            rec[k] = round(v[1], 2)
            rec[k + "_min_max"] = [round(v[0], 2), round(v[2], 2)]
        rec["mix_kernel_eager"] = round(rec["robot_mix"] - rec["robot_act"], 2)
        rec["mix_kernel_graph"] = round(rec["robot_mix_graph"] - rec["robot_act_graph"], 2)
        eng.close()
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
