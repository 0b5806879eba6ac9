"""numpy restatement of cn_robot_mix's coin and select (include/crowdnav.h), self-contained but for the Philox block
of tests/rollout_noise_ref.py.

    w = philox4x32_10(counter ((uint32)k, 0, 0, 0), key (seed, (uint32)G)),  k = step0 + t,  G = env_offset + e
    u = (float32)(w.z >> 8) * 2^-24            (exact, in [0, 1))
    took = u < beta;  executed = took ? label : learner (bits);  flags = took | (learner == label as bits) << 1"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rollout_noise_ref import philox4x32_10  # noqa: E402

_MASK = np.uint64(0xFFFFFFFF)


def coin_word(seed, k, G):
    """Word z of the block, uint64 < 2^32; k and G broadcast."""
    k = np.asarray(k, dtype=np.int64).astype(np.uint64) & _MASK
    G = np.asarray(G, dtype=np.int64).astype(np.uint64) & _MASK
    k, G = np.broadcast_arrays(k, G)
    return philox4x32_10((k, 0, 0, 0), (np.uint64(int(seed) & 0xFFFFFFFF), G))[2]


def coin(seed, k, G):
    """u float32 in [0, 1)."""
    return ((coin_word(seed, k, G) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def mix(label, learner, beta, seed, step0, env_offset, t0=0):
    """(executed (T, E, 2) float32, flags (T, E) uint8) for label / learner (T, E, 2) float32: row i is step
    k = step0 + t0 + i, column e the env of global index env_offset + e."""
    lab, lea = np.ascontiguousarray(label), np.ascontiguousarray(learner)
    assert lab.dtype == lea.dtype == np.float32 and lab.shape == lea.shape and lab.ndim == 3 and lab.shape[2] == 2
    T, E, _ = lab.shape
    k = (int(step0) + int(t0) + np.arange(T, dtype=np.int64))[:, None]
    G = (int(env_offset) + np.arange(E, dtype=np.int64))[None, :]
    took = coin(seed, k, G) < np.float32(beta)
    lb, le = lab.view(np.uint32), lea.view(np.uint32)
    executed = np.where(took[:, :, None], lb, le).astype(np.uint32).view(np.float32)
    same = (lb[..., 0] == le[..., 0]) & (lb[..., 1] == le[..., 1])
    return executed, (took.astype(np.uint8) | (same.astype(np.uint8) << np.uint8(1))).astype(np.uint8)
