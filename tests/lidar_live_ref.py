"""numpy restatement of the live LiDAR scan (cn_lidar_scan) — TEST INFRASTRUCTURE ONLY.

The scan CrowdSimDict.step() computes every step and then discards (crowd_sim_dict.py:224-251):
LidarSensor.sensor_spin(normalize=True) at the robot's position, heading atan2(vy, vx), against all N
humans (in index order) and the world walls. Pinned by tests/golden/lidar_live/*.npz, recorded from the
reference itself (tools/gen_lidar_live_golden.py). float64 throughout, like the reference:
  * beam angles: rescale(linspace(0, 2 pi, beams) + heading); beam samples: linspace(0, max_range, n_pts)
    rotated and translated, n_pts = max_range / 0.01 rounded up;
  * per obstacle an angular window (lo, up) from two points at +-radius across the line of sight; the
    window test flips windows at least pi wide IN PLACE, so the flip is seen by every later beam;
  * of the obstacles whose window holds the beam, only the one with the nearest centre (first on ties) is
    tested: the beam ends at its first sample strictly inside that disc;
  * otherwise at the first wall (in wall order) its full-range segment crosses, if that is within range;
  * never inside the robot's own radius.
"""
import numpy as np

TWO_PI = 2 * np.pi


def _rescale(t):
    return (t + TWO_PI) % TWO_PI


def n_samples(max_range):
    q = max_range / 0.01
    return int(q) + 1 if q % 1 != 0 else int(q)


def _turn(p, q, r):
    v = (float(q[1] - p[1]) * (r[0] - q[0])) - (float(q[0] - p[0]) * (r[1] - q[1]))
    return 1 if v > 0 else (2 if v < 0 else 0)


def _within(p, q, r):
    return max(p[0], r[0]) >= q[0] >= min(p[0], r[0]) and max(p[1], r[1]) >= q[1] >= min(p[1], r[1])


def _cross(p1, q1, p2, q2):
    o1, o2, o3, o4 = _turn(p1, q1, p2), _turn(p1, q1, q2), _turn(p2, q2, p1), _turn(p2, q2, q1)
    if o1 != o2 and o3 != o4:
        return True
    return ((o1 == 0 and _within(p1, p2, q1)) or (o2 == 0 and _within(p1, q2, q1)) or
            (o3 == 0 and _within(p2, p1, q2)) or (o4 == 0 and _within(p2, q1, q2)))


def _meet(p1, q1, p2, q2):
    xd = (p1[0] - q1[0], p2[0] - q2[0])
    yd = (p1[1] - q1[1], p2[1] - q2[1])
    div = xd[0] * yd[1] - xd[1] * yd[0]
    if div == 0:
        return None
    d = (p1[0] * q1[1] - p1[1] * q1[0], p2[0] * q2[1] - p2[1] * q2[0])
    return ((d[0] * xd[1] - d[1] * xd[0]) / div, (d[0] * yd[1] - d[1] * yd[0]) / div)


def windows(sensor, xyr):
    """(lo, up) (N,) float64: the unflipped angular window of every obstacle."""
    xyr = np.asarray(xyr, np.float64).reshape(-1, 3)
    rx, ry = xyr[:, 0] - sensor[0], xyr[:, 1] - sensor[1]
    head = _rescale(np.arctan2(ry, rx))
    dx, dy = xyr[:, 2] * np.sin(head), xyr[:, 2] * np.cos(head)
    a = _rescale(np.arctan2(ry - dy, rx + dx))
    b = _rescale(np.arctan2(ry + dy, rx - dx))
    return np.minimum(a, b), np.maximum(a, b)


def scan(sensor, heading, xyr, beams=180, max_range=5.0, robot_radius=0.3, half_world=10.0):
    """(beams,) float64 clip(dist / max_range, 0, 1) — sensor_spin's rel_dist. The observation carries
    |1 - rel_dist| (to_obs)."""
    sx, sy = float(sensor[0]), float(sensor[1])
    xyr = np.asarray(xyr, np.float64).reshape(-1, 3)
    s = np.linspace(0, max_range, n_samples(max_range))
    ang = _rescale(np.linspace(0, TWO_PI, beams) + heading)
    c, sn = np.cos(ang), np.sin(ang)
    bx = c[:, None] * s[None, :] + sx
    by = sn[:, None] * s[None, :] + sy
    lo, up = windows((sx, sy), xyr)
    centre_d = np.sqrt((xyr[:, 0] - sx) ** 2 + (xyr[:, 1] - sy) ** 2)
    t = half_world
    walls = [(-t, -t), (t, -t), (t, t), (-t, t), (-t, -t)]
    out = np.zeros(beams)
    for b in range(beams):
        wide = up - lo >= np.pi                       # flipped in place: later beams see the flipped window
        tt = np.where(wide, ang[b] - TWO_PI, ang[b])
        lo, up = np.where(wide, up - TWO_PI, lo), np.where(wide, lo, up)
        ok = (tt - lo) % TWO_PI < (up - lo) % TWO_PI
        end, hit = (bx[b, -1], by[b, -1]), False
        if ok.any():
            i = np.flatnonzero(ok)[np.argmin(centre_d[ok])]
            inside = np.flatnonzero(np.sqrt((xyr[i, 0] - bx[b]) ** 2 + (xyr[i, 1] - by[b]) ** 2) < xyr[i, 2])
            if len(inside):
                end, hit = (bx[b, inside[0]], by[b, inside[0]]), True
        if not hit:
            p1, q1 = (bx[b, 0], by[b, 0]), (bx[b, -1], by[b, -1])
            for j in range(4):
                if _cross(p1, q1, walls[j], walls[j + 1]):
                    ip = _meet(p1, q1, walls[j], walls[j + 1])
                    if ip is not None and np.linalg.norm([ip[0] - sx, ip[1] - sy]) <= max_range:
                        end = ip
                    break
        if np.linalg.norm([end[0] - sx, end[1] - sy]) < robot_radius:
            end = (sx + robot_radius * np.cos(ang[b]), sy + robot_radius * np.sin(ang[b]))
        out[b] = np.sqrt((end[0] - sx) ** 2 + (end[1] - sy) ** 2)
    return np.clip(out / max_range, 0, 1)


def to_obs(rel_dist):
    return np.abs(1 - np.asarray(rel_dist))


def unstable_mask(fn, args, rng, reruns=8, eps=1e-10, tol=1e-6):
    """Beams that move by more than tol when every float input of fn(*args) moves by up to +-eps: beams at
    an obstacle's angular edge or a sample on a disc's rim, where the last ulp of the trigonometry decides."""
    base = fn(*args)
    bad = np.zeros(base.shape, bool)
    for _ in range(reruns):
        pert = [np.asarray(a, np.float64) + rng.uniform(-eps, eps, np.shape(a)) for a in args]
        bad |= np.abs(fn(*pert) - base) > tol
    return bad


def state_scans(sv, beams, max_range, robot_radius, half_world):
    """(E, beams) float64 rel_dist of every env of an abi.StateView."""
    out = np.zeros((sv.E, beams))
    for e in range(sv.E):
        out[e] = scan((sv.r_px[e], sv.r_py[e]), np.arctan2(sv.r_vy[e], sv.r_vx[e]),
                      np.stack([sv.h_px[e], sv.h_py[e], sv.h_r[e]], 1), beams, max_range, robot_radius, half_world)
    return out


def robot_part(sv, max_range):
    rs = np.stack([sv.r_px, sv.r_py, sv.r_radius, sv.r_gx, sv.r_gy, sv.r_vpref, sv.r_theta], 1).astype(np.float64)
    return np.clip(rs / max_range, 0, 1).astype(np.float32)
