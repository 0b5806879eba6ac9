"""The lattice action head's definition (include/crowdnav.h, cn_lattice_*) in float64 numpy, the rows the tests share
and the acceptance rules that compare a float32 evaluation (the HIP kernels, the torch restatements) with it.

Tolerances, none of them measured on the code under test:
  LOGP_TOL  2e-6 * max(1, |ref|): what the project already asks of cn_gaussian_act's log-probability.
  sampling  a float32 evaluation's prefix sums and total differ from the exact ones by at most the rounding of a
            64-term float32 sum, t = 64 * 2^-23 * Z, so its choice c is accepted iff u * Z lies in
            [S_{c-1} - t, S_c + t] (S in float64, S_{-1} = 0).
  p_c > 0   in float32: expf(x) is 0 for x < -103.98 (half the smallest denormal is e^-103.97), so a chosen candidate
            must have l_c - max l > -103.98."""
import numpy as np

K = 64
GRID = (0.1 * (2.0 * np.arange(8, dtype=np.float64) - 7.0)) / 7.0            # cn_dwa_predict's dv of a, dtheta of b
ACTIONS = np.stack([np.repeat(GRID, 8), np.tile(GRID, 8)], 1)                # (64, 2) float64, row c = 8 a + b
ACTIONS32 = ACTIONS.astype(np.float32)
U_MAX = np.float32(1.0 - 2.0 ** -24)                                         # the largest float32 below 1
EXP_FLOOR = -103.98
KINDS = 8


def logp_tol(ref):
    return 2e-6 * np.maximum(1.0, np.abs(ref))


def rows(E, start=0, seed=0):
    """(E, 64) float32 logits; row i is of kind (start + i) % 8: 0 all equal, 1 the maximum at lane 0, 2 at lane 63,
    3 logits 1e4 + small, 4 a spread of +-80 (most candidates underflow in float32), 5 two equal maxima (lanes 17
    and 40), 6 and 7 plain normal rows of scale 3 and 0.3."""
    rs = np.random.RandomState(1234 + seed)
    out = np.empty((E, K), np.float64)
    for i in range(E):
        kind = (start + i) % KINDS
        r = rs.standard_normal(K)
        if kind == 0:
            r[:] = 0.25
        elif kind == 1:
            r[0] = 6.0
        elif kind == 2:
            r[63] = 6.0
        elif kind == 3:
            r = 1e4 + r
        elif kind == 4:
            r = rs.permutation(np.linspace(-80.0, 80.0, K))
        elif kind == 5:
            r[17] = r[40] = 5.0
        elif kind == 6:
            r = 3.0 * r
        else:
            r = 0.3 * r
        out[i] = r
    return out.astype(np.float32)


def draws(E, seed=0):
    """(E,) float32 in [0, 1): random, with 0 at every 7th row from row 0 and 1 - 2^-24 at every 7th from row 3 (7 and
    the 8 kinds of rows() are coprime, so every kind meets both ends within 56 rows); a single row gets 1 - 2^-24."""
    u = np.random.RandomState(99 + seed).random_sample(E).astype(np.float32)
    u = np.minimum(u, U_MAX)
    u[0::7] = 0.0
    u[3::7] = U_MAX
    if E == 1:
        u[0] = U_MAX
    return u


def softmax(logits):
    """float64 statement of the row quantities: dict of m (E,), p, logp, S (E, 64), Z, H (E,)."""
    l = np.asarray(logits, np.float64)
    m = l.max(1)
    d = l - m[:, None]
    p = np.exp(d)
    Z = p.sum(1)
    logp = d - np.log(Z)[:, None]
    q = p / Z[:, None]
    H = -np.where(p > 0, q * logp, 0.0).sum(1)
    return {"m": m, "d": d, "p": p, "Z": Z, "logp": logp, "S": np.cumsum(p, 1), "q": q, "H": H}


def mode(logits):
    return np.argmax(np.asarray(logits, np.float64), 1)   # (the first of equal maxima)


def index(actions):
    """The definition's index of (x, y) actions, in float32 as stated: clamp(rintf((x * 70 + 7) * 0.5), 0, 7)."""
    a = np.asarray(actions, np.float32)
    k = np.clip(np.rint((a * np.float32(70.0) + np.float32(7.0)) * np.float32(0.5)), 0, 7).astype(np.int64)
    return k[..., 0] * 8 + k[..., 1]


def sample_errors(logits, u, choice):
    """The rows (list of messages) whose sampled choice the definition does not admit: the interval rule and
    p_c > 0 in float32 (module docstring)."""
    s = softmax(logits)
    u = np.asarray(u, np.float64)
    c = np.asarray(choice, np.int64)
    errs = []
    for e in range(len(c)):
        if not 0 <= c[e] < K:
            errs.append("row %d: choice %d" % (e, c[e]))
            continue
        Z, S = s["Z"][e], s["S"][e]
        t = 64.0 * 2.0 ** -23 * Z
        lo = (S[c[e] - 1] if c[e] else 0.0) - t
        if not lo <= u[e] * Z <= S[c[e]] + t:
            errs.append("row %d: u Z = %r outside [%r, %r] of choice %d" % (e, u[e] * Z, lo, S[c[e]] + t, c[e]))
        if not s["d"][e, c[e]] > EXP_FLOOR:
            errs.append("row %d: choice %d has l - m = %r (p = 0 in float32)" % (e, c[e], s["d"][e, c[e]]))
    return errs


def eval_actions(B, seed=0):
    """(B, 2) float32 actions for evaluate: lattice points, points off the lattice inside and outside the range."""
    rs = np.random.RandomState(7 + seed)
    a = ACTIONS32[rs.randint(0, K, B)].copy()
    off = np.arange(B) % 3 == 1
    a[off] = rs.uniform(-0.13, 0.13, (int(off.sum()), 2)).astype(np.float32)
    return a
