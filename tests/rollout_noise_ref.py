"""numpy restatement of cn_rollout_noisy's perturbation (include/crowdnav.h), self-contained.

Philox4x32-10 in uint64 arithmetic (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
Random123 constants), then the float32 steps: u = (w >> 8) * 2^-24, n = 2 u - 1 (both exact), x = a + sigma * n with
one rounded product and one rounded sum."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2; returns the 4 output words as uint64 arrays < 2^32."""
    x = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64)
                                                                               for v in counter])]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK for v in key)
    x0, x1, x2, x3 = x
    for _ in range(10):
        p0, p1 = _M0 * x0, _M1 * x2          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _MASK, p1 >> _S32, p1 & _MASK
        x0, x1, x2, x3 = hi1 ^ x1 ^ k0, lo1, hi0 ^ x3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return x0, x1, x2, x3


def unit_noise(seed, k, G):
    """n (..., 2) float32 in [-1, 1): words x, y of philox(counter ((uint32)k, 0, 0, 0), key (seed, (uint32)G))."""
    k = np.asarray(k, dtype=np.int64).astype(np.uint64) & _MASK
    G = np.asarray(G, dtype=np.int64).astype(np.uint64) & _MASK
    k, G = np.broadcast_arrays(k, G)
    w = philox4x32_10((k, 0, 0, 0), (np.uint64(seed & 0xFFFFFFFF), G))
    n = []
    for j in range(2):
        u = (w[j] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        n.append(np.float32(2.0) * u - np.float32(1.0))
    return np.stack(n, axis=-1).astype(np.float32)


def perturb(actions, sigma, seed, step0, env_offset):
    """executed (T, E, 2) float32 for clean `actions` (T, E, 2) float32: row t is step k = step0 + t, column e the
    env of global index env_offset + e."""
    a = np.asarray(actions)
    assert a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == 2
    T, E, _ = a.shape
    k = (int(step0) + np.arange(T, dtype=np.int64))[:, None]
    G = (int(env_offset) + np.arange(E, dtype=np.int64))[None, :]
    n = unit_noise(seed, k, G)
    prod = (np.float32(sigma) * n).astype(np.float32)
    return (a + prod).astype(np.float32)
