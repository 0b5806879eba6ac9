#!/usr/bin/env python
"""Record the fixtures of the live LiDAR scan (cn_lidar_scan) from the reference — CPU box only.

  tests/golden/lidar_live/direct_*.npz   direct LidarSensor.sensor_spin(normalize=True) calls: sensor position,
                                         heading, human (x, y, r), half world, beams, max range, robot radius
                                         -> rel_dist
  tests/golden/lidar_live/roll_*.npz     CrowdSimDict (convgru, lidar.enable, E = 4, N = 5) stepped with random
                                         actions: every post-step state and the rel_distances step() computed
                                         (and discards: crowd_sim_dict.py:224-251), taken by wrapping
                                         env.lidar.sensor_spin
Every case carries an `unstable` mask: the reference scan rerun 8 times with every input moved by up to
+-1e-10; a beam that moves by more than 1e-6 in any rerun sits on an angular edge or a disc's rim, where
the last ulp of the trigonometry decides, and is excluded from exact comparison. At most 0.5 % of a file's
beams may be unstable (asserted here; pick other seeds if a file exceeds it).

oracle.gen_golden provides the import path of the reference, the shims and the recording helpers.
Usage: python tools/gen_lidar_live_golden.py [--out tests/golden/lidar_live]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (sets sys.path for the reference and its shims)

if not hasattr(np, "int"):
    np.int = int   # lidarv2.py:251 (np.int was removed in NumPy 1.24)

from crowd_sim.envs.utils.lidarv2 import LidarSensor  # noqa: E402

RERUNS, EPS, TOL, CAP = 8, 1e-10, 1e-6, 0.005


def ref_scan(sensor, heading, xyr, beams, max_range, robot_radius, half_world):
    s = LidarSensor({"max_range": max_range, "num_beams": int(beams), "robot_radius": robot_radius})
    t = half_world
    s.parse_obstacles(np.array(xyr, np.float64).reshape(-1, 3), "agents")
    s.parse_obstacles([(-t, -t), (t, -t), (t, t), (-t, t)], "walls")
    s.update_sensor((sensor[0], sensor[1]), heading)
    return np.asarray(s.sensor_spin(normalize=True)[1], np.float64)


def unstable(rng, sensor, heading, xyr, beams, max_range, robot_radius, half_world, base):
    bad = np.zeros(base.shape, bool)
    xyr = np.array(xyr, np.float64).reshape(-1, 3)
    for _ in range(RERUNS):
        p = (np.array(sensor, np.float64) + rng.uniform(-EPS, EPS, 2))
        h = float(heading) + rng.uniform(-EPS, EPS)
        x = xyr + rng.uniform(-EPS, EPS, xyr.shape)
        bad |= np.abs(ref_scan(p, h, x, beams, max_range, robot_radius, half_world) - base) > TOL
    return bad


class Cases:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.out, self.n, self.beams_total, self.unstable_total = {}, 0, 0, 0

    def add(self, sensor, heading, xyr, beams, max_range, robot_radius=0.3, half_world=10.0, tag=""):
        xyr = np.array(xyr, np.float64).reshape(-1, 3)
        rd = ref_scan(sensor, heading, xyr, beams, max_range, robot_radius, half_world)
        un = unstable(self.rng, sensor, heading, xyr, beams, max_range, robot_radius, half_world, rd)
        k = "c%d_" % self.n
        for name, v in (("sensor", np.array(sensor, np.float64)), ("heading", np.float64(heading)), ("xyr", xyr),
                        ("half_world", np.float64(half_world)), ("beams", np.int32(beams)),
                        ("max_range", np.float64(max_range)), ("robot_radius", np.float64(robot_radius)),
                        ("rel_dist", rd), ("unstable", un), ("tag", np.array(tag))):
            self.out[k + name] = v
        self.n += 1
        self.beams_total += rd.size
        self.unstable_total += int(un.sum())
        return rd

    def save(self, path):
        share = self.unstable_total / max(self.beams_total, 1)
        assert share <= CAP, "%s: unstable share %.4f above the cap: choose other seeds" % (path, share)
        self.out["cases"] = np.int32(self.n)
        np.savez_compressed(path, **self.out)
        print(os.path.basename(path), "cases", self.n, "unstable %.4f" % share, os.path.getsize(path), "bytes")


def random_humans(rng, N, sensor, spread):
    xyr = np.zeros((N, 3))
    ang, dist = rng.uniform(0, 2 * np.pi, N), rng.uniform(0.6, spread, N)
    xyr[:, 0], xyr[:, 1] = sensor[0] + dist * np.cos(ang), sensor[1] + dist * np.sin(ang)
    xyr[:, 2] = rng.uniform(0.2, 0.5, N)
    return xyr


HEADINGS = (0.0, -0.7, 2.4, np.pi - 1e-3, -np.pi + 1e-3, -np.pi, 1.1, -2.9)


def gen_direct(outdir, max_range, seed):
    """Random crowds: N = 1, 5, 10, 31 x beams = 2, 64, 65, 180, five cases each (the GPU test packs the five
    into one E = 5 engine). max_range 11: the sensor sits within 3 m of a wall, so walls are hit."""
    C = Cases(seed)
    rng = np.random.RandomState(seed + 1000)
    for N in (1, 5, 10, 31):
        for beams in (2, 64, 65, 180):
            for j in range(5):
                if max_range > 10:
                    side = rng.randint(4)
                    off, along = 10.0 - rng.uniform(0.5, 3.0), rng.uniform(-9, 9)
                    sensor = [(off, along), (-off, along), (along, off), (along, -off)][side]
                else:
                    sensor = tuple(rng.uniform(-6, 6, 2))
                xyr = random_humans(rng, N, sensor, 7.0 if N > 1 else 4.0)
                if j == 1:      # human 0 straddles angle 0: its window is >= pi wide and is flipped by beam 0
                    xyr[0] = (sensor[0] + rng.uniform(1.0, 3.0), sensor[1] + rng.uniform(-0.05, 0.05), 0.4)
                if j == 2:      # the sensor inside the last human's disc
                    xyr[-1] = (sensor[0] + 0.1, sensor[1] - 0.05, 0.45)
                if j == 3:      # a human beyond range
                    xyr[0] = (sensor[0] - (max_range + 2.5), sensor[1] + 0.3, 0.3)
                heading = HEADINGS[(C.n * 3 + j) % len(HEADINGS)] if j else rng.uniform(-np.pi, np.pi)
                C.add(sensor, heading, xyr, beams, float(max_range), tag="N%d_b%d_%d" % (N, beams, j))
    C.save(os.path.join(outdir, "direct_r%d.npz" % int(max_range)))


def gen_direct_edge(outdir, seed):
    """Hand-built cases, among them the nearest-centre rule: a small disc whose centre is nearest but which
    lies beyond range shadows a larger, farther disc that reaches into range — the reference reports no hit."""
    C = Cases(seed)
    for beams in (180, 65):
        for k in (10, int(0.55 * beams)):
            a = 1.0
            heading = a - k * 2 * np.pi / (beams - 1) + 0.003    # beam k points at the two discs
            near = (5.2 * np.cos(a), 5.2 * np.sin(a), 0.1)
            far = (5.4 * np.cos(a), 5.4 * np.sin(a), 0.6)
            other = (-3.0, -2.0, 0.3)
            both = C.add((0.0, 0.0), heading, [near, far, other], beams, 5.0, tag="shadow")
            alone = ref_scan((0.0, 0.0), heading, [far, other], beams, 5.0, 0.3, 10.0)
            ang = (np.linspace(0, 2 * np.pi, beams) + heading + 2 * np.pi) % (2 * np.pi)
            behind = np.abs((ang - a + np.pi) % (2 * np.pi) - np.pi) < 0.8 * np.arctan(0.1 / 5.2)
            assert behind.any(), "no beam points at the near disc"
            assert (alone[behind] < 1.0).all(), "the far disc alone must be hit"
            assert (both[behind] == 1.0).all(), "the reference must report no hit behind the near disc"
    # a huge disc around the sensor (a window nearly pi wide), humans on the axes
    C.add((0.0, 0.0), 0.0, [(0.3, 0.2, 2.0), (3.0, 0.0, 0.3)], 180, 5.0, tag="wide")
    C.add((1.0, -1.0), -np.pi, [(1.0, 1.5, 0.3), (3.5, -1.0, 0.5), (-1.0, -1.0, 0.3)], 65, 5.0, tag="axes")
    C.add((1.0, -1.0), np.pi, [(1.0, 1.5, 0.3), (3.5, -1.0, 0.5), (-1.0, -1.0, 0.3)], 2, 11.0, tag="axes2")
    C.add((9.5, 9.5), -0.4, [(8.0, 8.0, 0.4)], 180, 5.0, tag="corner")
    C.add((9.5, 9.5), 0.9, [(8.0, 8.0, 0.4)], 64, 11.0, tag="corner11")
    C.save(os.path.join(outdir, "direct_edge.npz"))


def gen_roll(outdir, kin, T, seed):
    cfg = G.make_ref_config(kin=kin, N=5)
    cfg.sim.circle_radius = 6.0
    cfg.robot.policy = "convgru"
    cfg.lidar.enable = True
    E = 4
    lc = cfg.lidar.cfg
    beams, max_range, rr = int(lc["num_beams"]), float(lc["max_range"]), float(lc["robot_radius"])
    half = cfg.sim.square_width / 2
    envs = [G.make_ref_env(cfg, r, E) for r in range(E)]
    log = [[] for _ in envs]
    for e, env in enumerate(envs):
        def spin(normalize=True, _orig=env.lidar.sensor_spin, _env=env, _log=log[e]):
            res = _orig(normalize=normalize)
            _log.append((np.array(_env.lidar.sensor_pos, np.float64), _env.lidar.sensor_heading,
                         np.array(_env.lidar.agent_attrs, np.float64), np.array(res[1], np.float64)))
            return res
        env.lidar.sensor_spin = spin
        G.env_reset(env)
    rng = np.random.RandomState(seed)
    out = {"meta_" + k: np.array(v) for k, v in G.cfg_meta(cfg, E).items()}
    out.update(meta_max_range=np.array(max_range), meta_num_beams=np.array(beams),
               meta_lidar_robot_radius=np.array(rr), steps=np.int32(T))
    total = bad = 0
    for t in range(T):
        rel, un, head, dones = [], [], [], []
        for e, env in enumerate(envs):
            a = (rng.normal(0, 0.7, 2) if kin == "holonomic" else rng.uniform(-0.15, 0.15, 2)).astype(np.float32)
            del log[e][:]
            _, rew, done, _ = G.run_in(env, env.step, a)
            env.ep_ret += rew
            env.ep_len += 1
            pos, h, xyr, rd = log[e][-1]
            assert xyr.shape == (5, 3)
            rel.append(rd)
            head.append(np.float64(h))
            un.append(unstable(rng, pos, float(h), xyr, beams, max_range, rr, half, rd))
            dones.append(done)
        sv = G.extract(envs, cfg)          # the post-step state, before any reset
        G.pack_state(sv, "t%d_post_" % t, out, False)
        out["t%d_rel_dist" % t], out["t%d_unstable" % t] = np.stack(rel), np.stack(un)
        out["t%d_heading" % t] = np.array(head)
        total += np.stack(un).size
        bad += int(np.stack(un).sum())
        for env, d in zip(envs, dones):
            if d:
                G.env_reset(env)
    assert bad / total <= CAP, "roll %s: unstable share %.4f above the cap: choose another seed" % (kin, bad / total)
    path = os.path.join(outdir, "roll_%s.npz" % kin)
    np.savez_compressed(path, **out)
    print(os.path.basename(path), "steps", T, "unstable %.4f" % (bad / total), os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "lidar_live"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    gen_direct_edge(args.out, 11)
    gen_direct(args.out, 5, 21)
    gen_direct(args.out, 11, 31)
    gen_roll(args.out, "holonomic", 16, 5)
    gen_roll(args.out, "unicycle", 16, 6)


if __name__ == "__main__":
    main()
