"""Restatement of the unicycle robot's tracking law (include/crowdnav.h, cn_scripted_unicycle), self-contained.

Written from the formulas, on Python floats with math.remainder / math.atan2 / math.cos; nothing is imported from the
package. The controller's velocity (ux, uy) is a float32 pair, so ux * ux and uy * uy are exact in float64 and
sqrt(ux * ux + uy * uy) rounds once, as the engine's norm (an fma of the two squares) does."""
import math

import numpy as np


def track_one(ux, uy, theta, v):
    """(a0, a1) as Python floats (float64, before the rounding to float32) and delta (None where s == 0)."""
    ux, uy, theta, v = float(ux), float(uy), float(theta), float(v)
    s = math.sqrt(ux * ux + uy * uy)
    delta = None
    if s == 0.0:
        a1, target = 0.0, 0.0
    else:
        psi = math.atan2(uy, ux)
        delta = math.remainder(psi - theta, 2.0 * math.pi)
        a1 = min(max(delta, -0.1), 0.1)
        target = s * max(0.0, math.cos(delta - a1))
    a0 = min(max(target - v, -0.1), 0.1)
    return a0, a1, delta


def track(vxy, theta, v):
    """actions (n, 2) float32 = (float32(a0), float32(a1)) and delta (n,) float64 (NaN where s == 0) for float32
    velocities vxy (n, 2) and float64 theta, v (n,)."""
    vxy = np.asarray(vxy)
    assert vxy.dtype == np.float32 and vxy.ndim == 2 and vxy.shape[1] == 2
    out = np.zeros((len(vxy), 2), np.float32)
    delta = np.full(len(vxy), np.nan)
    for k in range(len(vxy)):
        a0, a1, d = track_one(vxy[k, 0], vxy[k, 1], theta[k], v[k])
        out[k] = (np.float32(a0), np.float32(a1))
        if d is not None:
            delta[k] = d
    return out, delta
