"""Diagnostic: phase breakdown of the step and RNG kernels from the -DCN_STAMPS build.

    bash tools/build_stamps.sh      (python -m crowdnav_dsrnn_amd.build -DCN_STAMPS --out .../libcrowdnav_hip_stamps.so)

    CN_LIB_PATH=crowdnav_dsrnn_amd/lib/libcrowdnav_hip_stamps.so python tools/probe_stamps.py [variant]

"xcd [rot [step]]" (run_xcd) and "phase2 <step> [walk]" (run_phase2: phase 2 per wave, with the linear programs'
linearProgram1 body counts) read a -DCN_STAMP_STEP=<step> build through C2's multi-step launches.
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crowdnav_dsrnn_amd import _lib  # noqa: E402
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config  # noqa: E402
from crowdnav_dsrnn_amd.engine import CrowdNavEngine  # noqa: E402


def run(variant, E=4096, N=10, steps=300):
    if variant.endswith("_301"):   # a last step that is not a multiple of 20 (random goal changes every 5 s)
        variant, steps = variant[:-4], 301
    if variant == "c2w":   # the crowded circle centre of bench.py's --steps 20 --warmup 5 window
        steps = 16
    c = clone_config(Config())
    c.sim.human_num = N
    c.sim.train_val_sim = ["circle_crossing"]
    c.action_space.kinematics = "unicycle"
    if variant == "nogoal":
        c.humans.random_goal_changing = False
        c.humans.end_goal_changing = False
    if variant == "sf":
        c.humans.policy = "social_force"
    if variant in ("c3", "c3nogoal"):
        N = 25
        c.sim.human_num = N
        c.sim.train_val_sim = ["square_crossing"]
        c.action_space.kinematics = "holonomic"
        c.robot.FOV = c.humans.FOV = 1.0
        if variant == "c3nogoal":
            c.humans.random_goal_changing = False
            c.humans.end_goal_changing = False
    if variant in ("c5a", "c5b", "c5a_nonorm", "c5b_nonorm"):   # the two C5 engines (bench.engines_for)
        c.humans.policy = "orca"
        c.action_space.kinematics = "holonomic"
        c.reward.norm_zones = not variant.endswith("nonorm")
        if variant.startswith("c5a"):
            N = 5
            c.sim.train_val_sim = c.sim.test_sim = ["parallel_traffic", "perpendicular_traffic"]
        else:
            N = 1
            c.sim.train_val_sim = c.sim.test_sim = ["side_pref_passing", "side_pref_overtaking", "side_pref_crossing"]
            c.test.side_preference = True
            c.sim.circle_radius = 4
            c.humans.random_goal_changing = False
            c.humans.end_goal_changing = False
        c.sim.human_num = N
    eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
    eng.reset()
    L = _lib.lib()
    L.cn_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    a = np.zeros(4096 * 24, np.uint64)
    b = np.zeros(8192 * 24, np.uint64)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0)
    acts = torch.rand((steps, E, 2), generator=g, device="cuda:0") * 0.2 - 0.1
    _lib.check(L.cn_profile(eng._h, 1, steps))
    for s in range(steps):
        eng.step(acts[s])
    torch.cuda.synchronize()
    ta, tb, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    L.cn_profile_read(eng._h, ctypes.byref(ta), ctypes.byref(tb), ctypes.byref(n))
    L.cn_debug_stamps(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p))
    blocks = (E + (64 // N) - 1) // (64 // N)
    A = a.reshape(-1, 24)[:blocks].astype(np.int64)
    d = np.diff(A[:, :7], axis=1)
    print("[%s] kernel A avg %.1f us, kernel B avg %.1f us over %d steps" % (variant, ta.value * 1e3 / n.value,
                                                                          tb.value * 1e3 / n.value, n.value))
    names = ["load", "visibility", "policy+reward terms", "stores issued (wave 0)", "wave 0 at the barrier", "rng work (phase 5)"]
    tot = (A[:, 6] - A[:, 0])
    print("  kernel A cycles per workgroup (last step): total median %d max %d" % (np.median(tot), tot.max()))
    for k, nm in enumerate(names):
        print("    %-26s median %8d  max %8d  (%.0f%%)" % (nm, np.median(d[:, k]), d[:, k].max(),
                                                            100 * np.median(d[:, k]) / np.median(tot)))
    slow = tot >= np.percentile(tot, 95)
    print("  slowest 5%% workgroups (total >= %d): mean per phase %s" % (
        np.percentile(tot, 95), ", ".join("%s %d" % (nm.split()[0], d[slow, k].mean()) for k, nm in enumerate(names))))
    # the slowest workgroups of the last launch: phases, and each env's phase-5 item (kind, cycles from the
    # workgroup's phase-5 start; per-env stamps of the same workgroup share its XCD's clock)
    Bx = b.reshape(-1, 24).astype(np.int64)
    epb_ = 64 // N
    nbk = len(tot)
    xq, xr = nbk >> 3, nbk & 7
    for k in np.argsort(-tot)[:8]:
        items = []
        xi = k & 7
        blk = xi * xq + min(xi, xr) + (k >> 3)   # the kernel's XCD-aware env placement
        for e in range(blk * epb_, min((blk + 1) * epb_, E)):
            st_, rs, gl = Bx[e, 0], Bx[e, 5], Bx[e, 4]
            if A[k, 5] <= st_ <= A[k, 6]:
                kind = "reset" if A[k, 5] <= rs <= A[k, 6] and rs >= st_ else "goal"
                end = rs if kind == "reset" else gl
                items.append("%s %d-%d" % (kind, st_ - A[k, 5], end - A[k, 5]))
        print("    WG %d total %d: %s | phase 5: wave 0 past its item count %d; %s" % (
            k, tot[k], " ".join("%d" % d[k, j] for j in range(6)), A[k, 22] - A[k, 5], ", ".join(items) or "-"))
    span = A[:, 6].max() - A[:, 0].min()
    print("  launch span (first start -> last end) %d cycles; start skew max %d" % (span, A[:, 0].max() - A[:, 0].min()))
    # the whole grid on the device-wide 100 MHz clock (s_memtime above is per XCD: durations only)
    L.cn_debug_stamps_r.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    r = np.zeros(8192 * 2, np.uint64)
    L.cn_debug_stamps_r(r.ctypes.data_as(ctypes.c_void_p), None)
    R = r.reshape(-1, 2).astype(np.int64)
    live = np.nonzero(R[:, 1] > 0)[0]
    if len(live):
        R = R[:live.max() + 1]
        t0r = R[R[:, 0] > 0, 0].min()
        st, en = (R[:, 0] - t0r) * 10, (R[:, 1] - t0r) * 10     # ns
        kd = variant in ("c3", "c3nogoal")
        nb = len(R)
        is_step = np.zeros(nb, bool)
        if kd:
            is_step[nb - blocks:] = True
        else:
            is_step[:blocks] = True
        print("  grid timeline (ns from the first workgroup's start; %d step + %d spawn workgroups):" % (
            is_step.sum(), (~is_step).sum()))
        for nm, sel in (("step", is_step), ("spawn", ~is_step)):
            if sel.any():
                print("    %-5s start median %6d max %6d | end median %6d p95 %6d max %6d | duration median %6d max %6d" % (
                    nm, np.median(st[sel]), st[sel].max(), np.median(en[sel]), np.percentile(en[sel], 95), en[sel].max(),
                    np.median(en[sel] - st[sel]), (en[sel] - st[sel]).max()))
        last = np.argsort(-en)[:8]
        print("    last to end: " + ", ".join("%s#%d [%d, %d]" % ("step" if is_step[k] else "spawn", k, st[k], en[k])
                                              for k in last))
    B = b.reshape(-1, 24).astype(np.int64)[:E]
    t0 = A[:, 0].min()
    sub = [("p0 human loads", A[:, 12] - A[:, 0]), ("p0 env loads", A[:, 13] - A[:, 12]), ("p0 clip", A[:, 10] - A[:, 13]), ("p0 barrier", A[:, 1] - A[:, 10]),
           ("lines+sort", A[:, 7] - A[:, 2]), ("LP2", A[:, 8] - A[:, 7]), ("LP3", A[:, 9] - A[:, 8]), ("VR+terms", A[:, 3] - A[:, 9])]
    if (A[:, 14] > A[:, 2]).all():
        sub += [("kd: table", A[:, 15] - A[:, 2]), ("kd: walk", A[:, 14] - A[:, 15]),
                ("kd: rank+lines", A[:, 7] - A[:, 14])]
    if variant in ("c3", "c3nogoal"):
        it = A[:, 13]
        print("      kd walk iterations (thread 0's human, round 2): median %d max %d mean %.2f" % (np.median(it), it.max(), it.mean()))
        sub = [x for x in sub if not x[0].startswith("p0")]
    for nm, v in sub:
        print("      wave0 %-12s median %8d  max %8d" % (nm, np.median(v), v.max()))
    if variant not in ("c3", "c3nogoal"):   # linearProgram3 sub-problems of the workgroup (lp3_tasks): count, cycles B1 -> B2
        cyc = A[:, 23]
        print("      lp3 task rounds (lp3_tasks + replays) cycles: median %d max %d" % (np.median(cyc), cyc.max()))
    if variant not in ("c3", "c3nogoal"):   # per-wave ends of phases 0-2 (-DCN_STAMPS lanes 0 / 64 / 128), from the phase start
        per = [("p0 wave1 env load+clip+VR", A[:, 16] - A[:, 0]), ("p1 wave0 visibility", A[:, 19] - A[:, 1]),
               ("p1 wave1 reward terms", A[:, 17] - A[:, 1]), ("p1 wave2 robot terms", A[:, 18] - A[:, 1]),
               ("p2 wave1 quads done", A[:, 21] - A[:, 2]), ("p2 wave1 +ladder", A[:, 20] - A[:, 2])]
        for nm, v in per:
            print("      %-26s median %8d  max %8d" % (nm, np.median(v), v.max()))
    cur = B[:, 0] >= t0                      # items of the last step only
    res = B[cur & (B[:, 5] >= B[:, 0])]
    goal = B[cur & (B[:, 4] >= B[:, 0]) & (B[:, 5] < B[:, 0])]
    if len(res):
        r = res[:, 5] - res[:, 0]
        print("  phase-5 resets (last step, %d envs): cycles median %d p90 %d max %d" % (len(res), np.median(r), np.percentile(r, 90), r.max()))
    if len(goal):
        gg = np.diff(goal[:, :5], axis=1)
        tot = goal[:, 4] - goal[:, 0]
        print("  phase-5 goal items (last step, %d envs): mt load %d  random %d  end %d  write %d (median); total median %d p90 %d max %d"
              % (len(goal), *np.median(gg, axis=0), np.median(tot), np.percentile(tot, 90), tot.max()))
        for slot, nm in ((6, "random"), (7, "end")):
            v = goal[:, slot]
            rounds, chg, elig = v // 1000, (v % 1000) // 100, v % 100
            part = gg[:, 1] if slot == 6 else gg[:, 2]
            print("     %s pass: eligible mean %.2f, rounds mean %.2f max %d, changes (1st round) mean %.2f" % (
                nm, elig.mean(), rounds.mean(), rounds.max(), chg.mean()))
            k0 = 8 if slot == 6 else 11
            for r in range(int(rounds.max()) + 1):
                sel = rounds == r
                if sel.any():
                    print("        %d rounds: %4d envs, cycles median %d max %d | walk %d first-tries %d reject-loop %d (mean)" % (
                        r, sel.sum(), np.median(part[sel]), part[sel].max(), goal[sel, k0].mean(), goal[sel, k0 + 1].mean(),
                        goal[sel, k0 + 2].mean()))
    if len(goal) or len(res):   # the slowest 5 % workgroups' envs: what their RNG waves did (last step)
        epb = 64 // N
        slow_b = np.nonzero(slow)[0]
        sel = np.zeros(E, bool)
        for b in slow_b:
            sel[b * epb:(b + 1) * epb] = True
        rows = np.nonzero(cur)[0]
        ss = rows[sel[rows]]
        kinds = {"reset": ss[B[ss, 5] >= B[ss, 0]], "goal": ss[(B[ss, 4] >= B[ss, 0]) & (B[ss, 5] < B[ss, 0])]}
        print("  slowest 5%% workgroups' envs (%d WGs, %d env items): resets %d, goal items %d" % (
            len(slow_b), len(ss), len(kinds["reset"]), len(kinds["goal"])))
        gi = kinds["goal"]
        if len(gi):
            gg = np.diff(B[gi, :5], axis=1)
            print("    goal items: mt load %d random %d end %d write %d (mean); random changes mean %.2f, end changes mean %.2f" % (
                *gg.mean(axis=0), ((B[gi, 6] % 1000) // 100).mean(), ((B[gi, 7] % 1000) // 100).mean()))
    if variant in ("c3", "c3nogoal"):
        L.cn_debug_stamps_c.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        cc = np.zeros(8192 * 4, np.uint64)
        pp = np.zeros(8192 * 2, np.uint64)
        L.cn_debug_stamps_c(cc.ctypes.data_as(ctypes.c_void_p), pp.ctypes.data_as(ctypes.c_void_p))
        P = pp.reshape(-1, 2).astype(np.int64)[:E]
        ok = P[:, 1] > P[:, 0]
        if ok.any():
            dur = P[ok, 1] - P[ok, 0]    # the latest spawn of each env (s_memtime differs across XCDs: durations only)
            print("  spawn waves (latest spawn per env, %d envs): cycles median %d p90 %d max %d" % (
                ok.sum(), np.median(dur), np.percentile(dur, 90), dur.max()))
        C = cc.reshape(-1, 4).astype(np.float64)[:E]
        n = C[:, 3].sum()
        if n:
            print("  crowded rejection, all steps: %d passes; per pass cycles: ensure (MT gen) %.0f, candidates %.0f, "
                  "tests + ballot %.0f" % (n, C[:, 0].sum() / n, C[:, 1].sum() / n, C[:, 2].sum() / n))
    eng.close()


def run_xcd(rot=0, step=None, launches=60, warm=130, chunk=32, E=4096, N=10):
    """Where the step workgroups of C2's multi-step launches run and how long they take: per workgroup label
    (step workgroup index & 7: the workgroups that share an XCD under round-robin dispatch), per XCC id, and per
    place in their CU's residency order.

        CN_LIB_PATH=<stamps build> python tools/probe_stamps.py xcd [rot [step]]

    rot: the CN_LABEL_ROT the library was built with (the labels' env ranges in the order of (label + rot) & 7), so
    that a slowness that stays with the label can be told from one that moves with the env range.
    step: the CN_STAMP_STEP the library was built with (the step of a launch its phase stamps record; default: the
    launch's last step, the one that stores the outputs), which adds step_detail's report of that step.
    Durations on the device-wide 100 MHz clock (s_memrealtime); a workgroup's clock is its shader-clock span
    (s_memtime) over that."""
    c = clone_config(Config())
    c.humans.policy = "orca"
    c.sim.human_num = N
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.action_space.kinematics = "unicycle"
    eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
    eng.reset()
    eng.set_seq_chunk(chunk)
    L = _lib.lib()
    L.cn_debug_stamps_r.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.cn_debug_stamps_x.argtypes = [ctypes.c_void_p]
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0)
    acts = torch.rand((warm + chunk * launches, E, 2), generator=g, device="cuda:0") * 0.2 - 0.1
    eng.step_seq(acts[:warm])
    epb = min(64 // N, 16)
    nstep = (E + epb - 1) // epb
    r = np.zeros(8192 * 2, np.uint64)
    x = np.zeros(8192 * 4, np.uint64)
    ta, tb, nn = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    lab = np.arange(nstep) & 7
    dur = np.zeros((launches, nstep))
    clk = np.zeros((launches, nstep))
    xcc = np.zeros((launches, nstep), int)
    order = np.zeros((launches, nstep), int)     # place in the CU's residency order: 0 = the first to start there
    share = np.zeros((launches, nstep), int)     # step workgroups on the same CU
    wslot = np.zeros((launches, nstep), int)     # HW_ID wave slot of the workgroup's wave 0
    kern, last_end = [], []
    st0 = eng.spawn_stats()
    for k in range(launches):
        _lib.check(L.cn_profile(eng._h, 1, chunk))
        eng.step_seq(acts[warm + k * chunk:warm + (k + 1) * chunk])
        _lib.check(L.cn_profile_read(eng._h, ctypes.byref(ta), ctypes.byref(tb), ctypes.byref(nn)))
        L.cn_debug_stamps_r(r.ctypes.data_as(ctypes.c_void_p), None)
        L.cn_debug_stamps_x(x.ctypes.data_as(ctypes.c_void_p))
        R = r.reshape(-1, 2).astype(np.int64)[:nstep]
        X = x.reshape(-1, 4).astype(np.int64)[:nstep]
        dur[k] = (R[:, 1] - R[:, 0]) / 100.0                                            # us
        clk[k] = (X[:, 3] - X[:, 2]) / np.maximum(R[:, 1] - R[:, 0], 1) * 100.0          # MHz
        xcc[k] = X[:, 0] & 0xf
        wslot[k] = X[:, 1] & 0xf
        key = xcc[k] * 256 + (X[:, 1] >> 8 & 0xff)     # XCC id, then HW_ID's CU / SH / SE fields (bits 8-15)
        for kk in np.unique(key):
            m = np.nonzero(key == kk)[0]
            share[k, m] = len(m)
            order[k, m[np.argsort(R[m, 0], kind="stable")]] = np.arange(len(m))
        kern.append(ta.value * 1e3)
        last_end.append((R[:, 1].max() - R[:, 0].min()) / 100.0)
    _lib.check(L.cn_profile(eng._h, 0, 0))
    st1 = eng.spawn_stats()
    kern = np.asarray(kern)
    print("[xcd rot %d] chunk %d, %d launches after %d warm-up steps (us; stamps build), %d step workgroups"
          % (rot, chunk, launches, warm, nstep))
    wg_mean = dur.mean(axis=0)
    allm = dur.mean()
    print("  kernel %.2f  step-WG mean %.2f  max %.2f  last step-WG end %.2f  -> kernel / mean step-WG %.3f, max / mean %.3f"
          % (kern.mean(), allm, dur.max(axis=1).mean(), np.mean(last_end), kern.mean() / allm,
             dur.max(axis=1).mean() / allm))
    h, edges = np.histogram(wg_mean, bins=12)
    print("  histogram of per-workgroup means: " + " ".join("%.1f:%d" % (edges[i], h[i]) for i in range(len(h))))
    print("  (a) by label: label | env range | WGs | XCC ids seen | per-WG means: mean  std  min  max | clock MHz")
    lm, ls = [], []
    for b in range(8):
        v = wg_mean[lab == b]
        lm.append(v.mean())
        ls.append(v.std())
        print("      %5d | %9d | %3d | %-12s | %8.2f %8.2f %8.2f %8.2f | %8.1f" % (
            b, (b + rot) & 7, len(v), ",".join(map(str, np.unique(xcc[:, lab == b]))), v.mean(), v.std(), v.min(), v.max(),
            clk[:, lab == b].mean()))
    print("      spread between the labels' means: std %.2f, max - min %.2f; within a label (std of its workgroups' means): %.2f"
          % (np.std(lm), np.max(lm) - np.min(lm), np.mean(ls)))
    print("  (b) by dispatch order (step workgroup index // 256: one workgroup per CU and round): "
          + "; ".join("%d: %d WGs mean %.2f std %.2f" % (q, (np.arange(nstep) // 256 == q).sum(),
                                                          wg_mean[np.arange(nstep) // 256 == q].mean(),
                                                          wg_mean[np.arange(nstep) // 256 == q].std())
                      for q in range((nstep + 255) // 256)))
    print("  (c) by place in the CU's residency order (per launch: rank of the workgroup's start among the step "
          "workgroups of its XCC / SE / SH / CU), all launches:")
    for q in range(order.max() + 1):
        m = order == q
        print("      place %d: %6d samples  duration mean %.2f std %.2f  clock %.1f MHz" % (
            q, m.sum(), dur[m].mean(), dur[m].std(), clk[m].mean()))
    for sh in np.unique(share):
        print("      CUs with %d step workgroups: " % sh + "; ".join(
            "place %d mean %.2f" % (q, dur[(share == sh) & (order == q)].mean()) for q in range(sh)))
    stable = (order == order[0]).all(axis=0)
    print("      workgroups with the same place in every launch: %d of %d; their per-WG means by place: %s" % (
        stable.sum(), nstep, "; ".join("%d: %d WGs mean %.2f std %.2f" % (
            q, (stable & (order[0] == q)).sum(), wg_mean[stable & (order[0] == q)].mean(),
            wg_mean[stable & (order[0] == q)].std()) for q in range(order.max() + 1) if (stable & (order[0] == q)).any())))
    print("      HW_ID wave slot of wave 0 by place (last launch): " + "; ".join(
        "place %d: %s" % (q, dict(zip(*[a.tolist() for a in np.unique(wslot[-1][order[-1] == q], return_counts=True)])))
        for q in range(order.max() + 1)))
    resid = dur - np.choose(order, [dur[order == q].mean() for q in range(order.max() + 1)])
    print("  (d) left after the place's mean is taken out: std of per-WG means %.2f (raw %.2f); per label means %s"
          % (resid.mean(axis=0).std(), wg_mean.std(), " ".join("%.2f" % resid[:, lab == b].mean() for b in range(8))))
    print("  spawn stats delta: %s" % {k: st1[k] - st0[k] for k in st1})
    print("  per step: kernel %.2f us" % (kern.mean() / chunk))
    # the phases of one fused step: the per-workgroup stamps hold the last launch's last step (every step rewrites
    # them; that step is the one that stores the state and the outputs)
    L.cn_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    a = np.zeros(4096 * 24, np.uint64)
    b = np.zeros(8192 * 24, np.uint64)
    L.cn_debug_stamps(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p))
    A = a.reshape(-1, 24)[:nstep].astype(np.int64)
    d = np.diff(A[:, :7], axis=1)
    tot = A[:, 6] - A[:, 0]
    names = ["load", "visibility", "policy+reward terms", "stores issued (wave 0)", "wave 0 at the barrier", "rng work (phase 5)"]
    which = "last step" if step is None else "step %d" % step
    print("  %s of the last launch, cycles per workgroup: total median %d max %d" % (which, np.median(tot), tot.max()))
    for k, nm in enumerate(names):
        print("    %-26s median %8d  max %8d" % (nm, np.median(d[:, k]), d[:, k].max()))
    if step is not None:
        step_detail(A, b.reshape(-1, 24).astype(np.int64)[:E], E, epb, kern.mean() / allm)
    eng.close()


def step_detail(A, B, E, epb, launch_over_wg):
    """One step of a multi-step launch (a -DCN_STAMP_STEP=k build): the per-wave ends, the window between phase 2's
    closing barrier and the next one, the step's goal items and resets per workgroup, and what the chain would
    save if the goal items ran on waves 2 and 3 inside that window."""
    nstep = len(A)
    per = [("p0 wave1 env load+clip", A[:, 16] - A[:, 0]), ("p1 wave0 visibility", A[:, 19] - A[:, 1]),
           ("p1 wave1 reward terms", A[:, 17] - A[:, 1]), ("p1 wave2 robot terms", A[:, 18] - A[:, 1]),
           ("p2 wave1 quads done", A[:, 21] - A[:, 2]), ("p2 wave1 +ladder", A[:, 20] - A[:, 2]),
           ("window: wave 0 stores issued", A[:, 4] - A[:, 3]), ("window: wave 1 at the barrier", A[:, 11] - A[:, 3]),
           ("window: barrier to barrier", A[:, 5] - A[:, 3])]
    for nm, v in per:
        print("      %-30s median %8d  max %8d" % (nm, np.median(v), v.max()))
    tot = A[:, 6] - A[:, 0]
    window = A[:, 5] - A[:, 3]
    p5 = A[:, 6] - A[:, 5]
    xq, xr = nstep >> 3, nstep & 7
    k = np.arange(nstep)
    blk = (k & 7) * xq + np.minimum(k & 7, xr) + (k >> 3)   # the kernel's XCD-aware env placement
    wg_of_env = np.empty(E, int)
    for kk in range(nstep):
        wg_of_env[blk[kk] * epb:min((blk[kk] + 1) * epb, E)] = kk
    a0, a6 = A[wg_of_env, 0], A[wg_of_env, 6]
    cur = (B[:, 0] >= a0) & (B[:, 0] <= a6)            # items of this step (a workgroup's stamps share its XCD's clock)
    is_res = cur & (B[:, 5] >= B[:, 0]) & (B[:, 5] <= a6)
    is_goal = cur & ~is_res & (B[:, 4] >= B[:, 0])
    ng = np.bincount(wg_of_env[is_goal], minlength=nstep)
    nr = np.bincount(wg_of_env[is_res], minlength=nstep)
    print("  step items: %d goal items, %d resets; workgroups with >= 1 goal item %.3f, with >= 3 %.3f, with a reset %.3f, "
          "with neither %.3f" % (is_goal.sum(), is_res.sum(), (ng >= 1).mean(), (ng >= 3).mean(), (nr >= 1).mean(),
                                 ((ng == 0) & (nr == 0)).mean()))
    gdur = B[:, 4] - B[:, 0]
    if is_goal.any():
        gg = np.diff(B[is_goal][:, :5], axis=1)
        v = gdur[is_goal]
        print("  goal items: mt load %d  random %d  end %d  write %d (median); total median %d p90 %d max %d" % (
            *np.median(gg, axis=0), np.median(v), np.percentile(v, 90), v.max()))
        # an item that starts before the window's closing barrier (an early item): still running at that barrier?
        early = is_goal & (B[:, 0] < A[wg_of_env, 5])
        if early.any():
            late = early & (B[:, 4] > A[wg_of_env, 5])
            over = (B[:, 4] - A[wg_of_env, 5])[late]
            print("  early goal items: %d, still running when waves 0 / 1 passed the barrier: %d (outlasting it by median %d "
                  "p90 %d max %d cycles)" % (early.sum(), late.sum(), np.median(over) if len(over) else 0,
                                             np.percentile(over, 90) if len(over) else 0, over.max() if len(over) else 0))
    if is_res.any():
        v = (B[:, 5] - B[:, 0])[is_res]
        print("  resets: cycles median %d p90 %d max %d" % (np.median(v), np.percentile(v, 90), v.max()))
    for nm, sel in (("no item", (ng == 0) & (nr == 0)), ("goal items only", (ng > 0) & (nr == 0)), ("a reset", nr > 0)):
        if sel.any():
            print("    workgroups with %-16s %4d: step median %6d  window %6d  phase 5 median %6d max %6d" % (
                nm + ":", sel.sum(), np.median(tot[sel]), np.median(window[sel]), np.median(p5[sel]), p5[sel].max()))
    # prediction: a workgroup without a reset runs its goal items on waves 2 and 3 from the window's start, item j on
    # wave 2 + (j & 1), in env order; what outlasts the window stays on the chain. (a) the issue's formula,
    # min(item, window) with item = the workgroup's phase 5 today; (b) with the two waves' serial chains.
    save_a = np.zeros(nstep)
    save_b = np.zeros(nstep)
    left_b = np.zeros(nstep)
    for kk in np.nonzero((ng > 0) & (nr == 0))[0]:
        envs = np.nonzero(is_goal & (wg_of_env == kk))[0]
        ch = [gdur[envs[0::2]].sum(), gdur[envs[1::2]].sum()]
        save_a[kk] = min(p5[kk], window[kk])
        left_b[kk] = max(0, max(ch) - window[kk])
        save_b[kk] = p5[kk] - left_b[kk]
    sel = (ng > 0) & (nr == 0)
    print("  predicted saving of goal items inside the window (workgroups without a reset), share of the sum of step "
          "durations: (a) min(phase 5, window) %.4f; (b) phase 5 - what the two waves' chains outlast the window by "
          "%.4f (remainder median %d p90 %d max %d over those workgroups)" % (
              save_a.sum() / tot.sum(), save_b.sum() / tot.sum(), np.median(left_b[sel]) if sel.any() else 0,
              np.percentile(left_b[sel], 90) if sel.any() else 0, left_b.max()))
    print("  launch / mean step workgroup %.3f" % launch_over_wg)


def run_phase2(step, walk=False, launches=12, warm=130, chunk=32, E=4096, N=10):
    """Phase 2 of one step of C2's multi-step launches per WAVE (a -DCN_STAMPS -DCN_STAMP_STEP=<step> build):
    lines + ranking, lp2_r, the wait at the barrier before lp3_tasks, lp3_tasks, lp3_replay + human_post, and the
    linearProgram1 bodies the wave ran in lp2_r and lp3_tasks beside what its busiest quad needed (stamps.h: STAMP_W).

        CN_LIB_PATH=<stamps build> python tools/probe_stamps.py phase2 <step> [walk]

    walk: the library's lp2_r is the walk, whose waves run one body per trip (the busiest quad's count), not one per
    distinct line index of the wave."""
    c = clone_config(Config())
    c.humans.policy = "orca"
    c.sim.human_num = N
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.action_space.kinematics = "unicycle"
    eng = CrowdNavEngine(make_cn_config(c, num_envs=E), "cuda:0")
    eng.reset()
    eng.set_seq_chunk(chunk)
    L = _lib.lib()
    L.cn_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.cn_debug_stamps_w.argtypes = [ctypes.c_void_p]
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0)
    acts = torch.rand((warm + chunk * launches, E, 2), generator=g, device="cuda:0") * 0.2 - 0.1
    eng.step_seq(acts[:warm])
    epb = min(64 // N, 16)
    nstep = (E + epb - 1) // epb
    nwave = (epb * N + 15) // 16          # waves that hold quads
    a = np.zeros(4096 * 24, np.uint64)
    b = np.zeros(8192 * 24, np.uint64)
    w = np.zeros(4096 * 4 * 16, np.uint64)
    As, Ws = [], []
    for k in range(launches):
        eng.step_seq(acts[warm + k * chunk:warm + (k + 1) * chunk])
        L.cn_debug_stamps(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p))
        L.cn_debug_stamps_w(w.ctypes.data_as(ctypes.c_void_p))
        As.append(a.reshape(-1, 24)[:nstep].astype(np.int64))
        Ws.append(w.reshape(-1, 4, 16)[:nstep, :nwave].astype(np.int64))
    A = np.concatenate(As)
    W = np.concatenate(Ws)                 # [launch x workgroup][wave][16]
    tot = A[:, 6] - A[:, 0]
    p2 = A[:, 3] - A[:, 2]
    print("[phase2] step %d of %d-step launches, %d launches after %d warm-up steps, %d workgroups x %d quad waves; lp2_r: %s"
          % (step, chunk, launches, warm, nstep, nwave, "walk" if walk else "unrolled"))
    print("  cycles per workgroup: step median %d max %d; phase 2 (barrier to barrier) median %d max %d (%.1f%% of the step)"
          % (np.median(tot), tot.max(), np.median(p2), p2.max(), 100 * np.median(p2) / np.median(tot)))
    t2 = A[:, 2][:, None]
    spans = [("lines + ranking", W[:, :, 0] - t2), ("lp2_r", W[:, :, 1] - W[:, :, 0]),
             ("wait at the barrier", W[:, :, 2] - W[:, :, 1]), ("lp3_tasks", W[:, :, 3] - W[:, :, 2]),
             ("lp3_replay + human_post", W[:, :, 4] - W[:, :, 3])]
    print("  span (cycles)              all waves: median   mean    max | slowest wave of the workgroup: median   mean | per wave medians")
    for nm, v in spans:
        print("    %-26s %8d %8d %8d | %8d %8d | %s" % (nm, np.median(v), v.mean(), v.max(), np.median(v.max(axis=1)),
                                                        v.max(axis=1).mean(), " ".join("%d" % np.median(v[:, k]) for k in range(nwave))))
    lp2 = W[:, :, 1] - W[:, :, 0]
    uni, mx = W[:, :, 5], W[:, :, 6]
    ran = mx if walk else uni
    print("  lp2_r linearProgram1 bodies per wave: distinct indices of the wave mean %.2f, busiest quad mean %.2f (the wave "
          "ran: %.2f)" % (uni.mean(), mx.mean(), ran.mean()))
    # cycles per body: the slope of the span over the bodies the wave ran (least squares), and the plain ratio
    x, y = ran.ravel().astype(float), lp2.ravel().astype(float)
    slope, icpt = np.polyfit(x, y, 1)
    print("    lp2_r span vs bodies run: %.0f cycles per body + %.0f (least squares); mean span / mean bodies %.0f"
          % (slope, icpt, y.mean() / max(x.mean(), 1e-9)))
    if not walk:
        rem = (uni - mx).mean()
        print("    a walk removes %.2f bodies per wave (%.0f%%): predicted %.0f cycles per wave, %.2f%% of the step's median"
              % (rem, 100 * rem / max(uni.mean(), 1e-9), rem * slope, 100 * rem * slope / np.median(tot)))
    u3, m3, r3 = W[:, :, 7], W[:, :, 8], W[:, :, 9]
    l3 = W[:, :, 3] - W[:, :, 2]
    has = r3 > 0
    print("  lp3_tasks: waves with a sub-problem %.3f; rounds mean %.2f; bodies per wave: distinct indices %.2f, busiest quad "
          "%.2f (over all waves)" % (has.mean(), r3.mean(), u3.mean(), m3.mean()))
    if has.any():
        s3, i3 = np.polyfit(u3.ravel().astype(float), l3.ravel().astype(float), 1)
        rem3 = (u3 - m3).mean()
        print("    span vs bodies run: %.0f cycles per body + %.0f; a walk removes %.2f bodies per wave: predicted %.0f cycles "
              "per wave, %.2f%% of the step's median" % (s3, i3, rem3, rem3 * s3, 100 * rem3 * s3 / np.median(tot)))
    eng.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["phase2"]:
        run_phase2(int(sys.argv[2]), walk=sys.argv[3:4] == ["walk"])
        sys.exit(0)
    if sys.argv[1:2] == ["xcd"]:
        run_xcd(int(sys.argv[2]) if len(sys.argv) > 2 else 0, int(sys.argv[3]) if len(sys.argv) > 3 else None)
        sys.exit(0)
    for v in (sys.argv[1:] or ["c2", "nogoal", "sf"]):
        run(v)
