#!/usr/bin/env python
"""HIP-event timings of the soft-label path beside the hard-label one.

controller  on 4096 unicycle envs x 5 and x 9 humans, the state a few random steps left: cn_robot_act('dwa') and
            cn_robot_act_regret (the same launch with the 1 MiB of regret rows stored beside the actions), each as
            replays of one captured graph of --launches launches (a call this short, issued eagerly, measures the host),
            after 20 warm-up launches, three alternating rounds; the median round in us per call with the rounds' spread.
            --plain-only: the first of the two alone (for a library that has no regret entry point).
loss        on 32768 rows of random logits and regrets at tau 0.1: ops.lattice_soft_ce forward + backward (the two
            kernels), its torch restatement on the same device tensors, and the hard pair ops.lattice_evaluate
            forward + backward, 200 calls between two events, three alternating rounds.
trainer     (--trainer, alone) learner.DAgger.update() at 1024 envs x 32 steps x 5 humans, aggregate 4, lattice head,
            beta 1 halved per chunk, graphs on: rollout_s / update_s (GPU time between HIP events) of 20 updates after 6
            warm-ups, median [min, max] in ms, hard labels and soft_tau 0.1 alternating, twice each.
Needs a GPU; prints one JSON line per record.

Usage: python tools/soft_label_time.py [--envs 4096] [--humans 5 9] [--launches 1000] [--rows 32768] [--plain-only]
           [--trainer] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crowdnav_dsrnn_amd import ops  # noqa: E402
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config  # noqa: E402
from crowdnav_dsrnn_amd.engine import CrowdNavEngine  # noqa: E402

DEV = "cuda:0"


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls      # us per call


def rounds_of(fns, calls, rec):
    rounds = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            rounds[k].append(timed(fn, calls))
    for k, v in rounds.items():
        v = sorted(v)
        rec[k] = round(v[1], 2)
        rec[k + "_min_max"] = [round(v[0], 2), round(v[2], 2)]
    return rec


def controller(E, N, L, plain_only):
    c = clone_config(Config())
    c.sim.human_num = N
    c.action_space.kinematics = "unicycle"
    eng = CrowdNavEngine(make_cn_config(c, num_envs=E), DEV, scripted_dwa=True)
    eng.reset()
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(8):
        eng.step(torch.randn((E, 2), generator=g, device=DEV) * 0.1)
    label = torch.zeros((E, 2), device=DEV)
    regret = torch.zeros((E, 64), device=DEV)
    calls = {"robot_act": lambda: eng.robot_act("dwa", label)}
    if not plain_only:
        calls["robot_act_regret"] = lambda: eng.robot_act("dwa", label, regret=regret)
    fns = {}
    for k, one in calls.items():
        for _ in range(20):
            one()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(L):
                one()
        gr.replay()   # (the first replay uploads the graph)
        fns[k + "_graph"] = gr.replay
    rec = rounds_of(fns, L, {"what": "controller", "envs": E, "humans": N, "launches": L,
                             "unit": "us per call (HIP events, graph replays)",
                             "device": torch.cuda.get_device_name(0)})
    if not plain_only:
        rec["regret_minus_plain"] = round(rec["robot_act_regret_graph"] - rec["robot_act_graph"], 2)
        rec["regret_bytes"] = E * 256
    eng.close()
    return rec


def loss(B, calls=200):
    g = torch.Generator(device=DEV).manual_seed(2)
    logits = (torch.randn((B, 64), generator=g, device=DEV) * 3.0).requires_grad_(True)
    regret = torch.rand((B, 64), generator=g, device=DEV) * 2.0
    regret[torch.arange(B, device=DEV), torch.randint(0, 64, (B,), generator=g, device=DEV)] = 0.0
    actions = ops.lattice_actions(DEV)[torch.randint(0, 64, (B,), generator=g, device=DEV)]

    def soft():
        logits.grad = None
        ops.lattice_soft_ce(logits, regret, 0.1)[0].mean().backward()

    def soft_torch():
        logits.grad = None
        ops.lattice_soft_ce_torch(logits, regret, 0.1)[0].mean().backward()

    def hard():
        logits.grad = None
        (-ops.lattice_evaluate(logits, actions)[0].mean()).backward()

    fns = {}
    for k, one in (("soft_kernels", soft), ("soft_torch", soft_torch), ("hard_kernels", hard)):
        for _ in range(20):
            one()
        fns[k] = (lambda f: lambda: [f() for _ in range(calls)])(one)
    return rounds_of(fns, calls, {"what": "loss fwd + bwd (with the mean and its backward)", "rows": B, "calls": calls,
                                  "unit": "us per call (HIP events, eager)", "device": torch.cuda.get_device_name(0)})


def trainer(tau, E=1024, T=32):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import DAgger
    from crowdnav_dsrnn_amd.policy import Policy

    c = clone_config(Config())
    c.sim.human_num = 5
    c.action_space.kinematics = "unicycle"
    c.robot.scripted_unicycle = True
    c.robot.scripted_dwa = True
    c.robot.action_head = "lattice"
    c.training.num_processes = E
    c.ppo.num_steps, c.ppo.num_mini_batch = T, 2
    envs = CrowdNavVecEnv(c, E, 0, DEV, allow_early_resets=True, nenv=E, phase="train")
    torch.manual_seed(0)
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=envs.config).to(DEV)
    dg = DAgger(c, envs, pol, expert="dwa", beta=1.0, beta_decay=0.5, seed=0, lr=1e-3, aggregate=4, soft_tau=tau)
    for _ in range(6):
        dg.update()
    st = [dg.update() for _ in range(20)]
    r = sorted(s["rollout_s"] for s in st)
    u = sorted(s["update_s"] for s in st)
    rec = {"soft_tau": tau, "envs": E, "steps": T, "aggregate": 4, "graphs": dg.graphs, "updates": 20,
           "rollout_ms_median_min_max": [round(1e3 * r[10], 3), round(1e3 * r[0], 3), round(1e3 * r[-1], 3)],
           "update_ms_median_min_max": [round(1e3 * u[10], 3), round(1e3 * u[0], 3), round(1e3 * u[-1], 3)],
           "nll": st[-1]["nll"], "agree": st[-1]["agree"], "soft_ce": st[-1].get("soft_ce"), "kl": st[-1].get("kl")}
    envs.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 9])
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("soft_label_time: needs a GPU")
    lines = []
    for tau in ((None, 0.1, None, 0.1) if args.trainer else ()):
        lines.append(json.dumps(trainer(tau)))
        print(lines[-1], flush=True)
    for N in ([] if args.trainer else args.humans):
        lines.append(json.dumps(controller(args.envs, N, args.launches, args.plain_only)))
        print(lines[-1], flush=True)
    if not (args.plain_only or args.trainer):
        lines.append(json.dumps(loss(args.rows)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
