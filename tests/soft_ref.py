"""The soft-label loss of the lattice head (include/crowdnav.h, cn_lattice_soft_fwd / _bwd) in float64 numpy, the
regret rows the tests share and the tolerances that compare a float32 evaluation (the HIP kernels, the torch
restatement) with it. The logit rows are tests/lattice_ref.py's.

Tolerances: derived here from float32 rounding of the definition, none of them measured on the code under test. With
u = 2^-24 (half an ulp), per row, from the float64 values of the definition:

  logp_j   LOGP_TOL of lattice_ref: 2e-6 * max(1, |logp_j|), the project's rule for a log-probability.
  x_j      a_j = r_j - min r and x_j = -(a_j * inv_tau) are two float32 roundings: |dx_j| <= 2u |x_j|.
  t_j      expf(x_j): relative error e_t(j) = 2u |x_j| (the argument's rounding, |d exp(x)| = exp(x) |dx|) + 4u (the
           function itself, 2 ulp). The first term matters only where t_j is not negligible: q_j |x_j| <= 1 / e.
  Zt       a 64-term float32 sum of the t_j, in any order: relative error e_Z = sum_k q_k e_t(k) + 64u.
  q_j      t_j / Zt: absolute error E_q(j) = q_j (e_t(j) + e_Z + u). A t_j below the float32 normal range (2^-126)
           loses relative precision or is flushed to 0; what it can add to any sum here is below 64 * 2^-126 times
           the largest factor, the `tiny` term.
  ce       -sum q_j logp_j over q_j > 0: the factors' errors, a rounding per product and the 64-term sum,
           tol_ce = sum_j (q_j LOGP_TOL(logp_j) + E_q(j) |logp_j|) + 65u sum_j |q_j logp_j| + tiny.
  Hq       -sum q_j w_j with w_j = x_j - logf(Zt): |dw_j| <= 2u |x_j| + e_Z + 4u |log Zt| + u |w_j| (logf: 2 ulp, and
           d log(Zt) = the relative error of Zt),
           tol_Hq = sum_j (q_j |dw_j| + E_q(j) |w_j|) + 65u sum_j |q_j w_j| + tiny.
  kl       ce - Hq, one more rounding: tol_kl = tol_ce + tol_Hq + u |kl|.
  dl_j     g (P_j - q_j) with P_j = p_j / Z = exp(logp_j): |dP_j| <= P_j (LOGP_TOL(logp_j) + 4u), the relative error
           of an exponential being the absolute error of its argument; an evaluation that forms P_j * (sum_k q_k) - q_j
           (autograd through log_softmax does) carries sum_k q_k = 1 only to e_Z + 65u, which P_j e_Z + 65u P_j
           covers; then the subtraction's and the product's roundings,
           tol_dl(j) = |g| (P_j (LOGP_TOL(logp_j) + 4u + e_Z + 65u) + E_q(j) + 2u |P_j - q_j|) + tiny.
  logp_best  LOGP_TOL of its reference value. Which candidates have a_j == 0 is exact in any precision (r_j == min r).

On this project's test rows tol_ce lies between about 3e-6 and 1.6e-3 (the +-80 logit spread, whose log-probabilities
reach -160, sets the upper end through LOGP_TOL and E_q |logp|). The torch restatement ops.lattice_soft_ce_torch, an
independent float32 evaluation, is checked against these bounds on every test row by tests/test_soft_labels.py on the
CPU."""
import functools

import numpy as np

from tests import lattice_ref

K = 64
U = 2.0 ** -24
TINY = 64 * 2.0 ** -126
KINDS = 7          # coprime to lattice_ref.KINDS = 8: over 56 rows every regret kind meets every logit kind
TAUS = (0.02, 0.1, 0.5)
BATCHES = ((1, 4), (5, 0), (257, 0))   # (B, start): a lone wave (a real DWA row), a workgroup and a wave, 64 and a wave


def inv_tau32(tau):
    """1 / tau as the float32 the entry points take."""
    return np.float32(1.0 / float(tau))


@functools.lru_cache(maxsize=None)
def dwa_rows(n=128):
    """(n, 64) float32 regret rows of the DWA controller itself: policy_factory.dwa_predict at the defaults on the first
    n of tests/test_dwa.py's 400 random 5-human states (seed 1), through policy_factory.dwa_regret. They reach 800
    (w_col = 100 per step left after a forecast collision), so most targets underflow somewhere."""
    from crowdnav_dsrnn_amd.policy_factory import dwa_predict, dwa_regret
    from tests.test_dwa import _random_states

    s, v, o = _random_states(np.random.RandomState(1), 400, 5)
    _, choice, costs = dwa_predict(s[:n], v[:n], o[:n], 0.25)
    return dwa_regret(costs, choice)


def regrets(B, start=0, seed=0):
    """(B, 64) float32 regret rows; row i is of kind (start + i) % 7: 0 all zeros (the uniform target), 1 one zero
    (lane 9) and the rest 1e4 (the hard limit), 2 two exact zeros (lanes 3 and 50) among values in (0.01, 1), 3 four
    exact zeros (lanes 0, 1, 62, 63) among values in (0.001, 0.3), 4 and 6 real DWA rows, 5 a real row plus the
    constant 37.5 (the shift: its minimum is not 0)."""
    rs = np.random.RandomState(4321 + seed)
    real = dwa_rows()
    out = np.empty((B, K), np.float32)
    for i in range(B):
        kind = (start + i) % KINDS
        if kind == 0:
            r = np.zeros(K)
        elif kind == 1:
            r = np.full(K, 1e4)
            r[9] = 0.0
        elif kind == 2:
            r = rs.uniform(0.01, 1.0, K)
            r[[3, 50]] = 0.0
        elif kind == 3:
            r = rs.uniform(0.001, 0.3, K)
            r[[0, 1, 62, 63]] = 0.0
        else:
            r = real[(start + i) % len(real)].astype(np.float64)
            if kind == 5:
                r = r + 37.5
        out[i] = r
    return out


def kinds(B, start=0):
    return (start + np.arange(B)) % KINDS


def soft(logits, regret, tau):
    """The definition in float64 on float32 rows: dict of a, x, q (B, 64), Zt, ce, Hq, kl, logp_best, best (B,), P and
    logp (B, 64), and the tolerances tol_ce, tol_kl, tol_best (B,) of the module docstring."""
    s = lattice_ref.softmax(logits)
    logp, P = s["logp"], s["q"]
    r = np.asarray(regret, np.float32).astype(np.float64)
    it = float(inv_tau32(tau))
    a = r - r.min(1, keepdims=True)
    x = -(a * it)
    t = np.exp(x)
    Zt = t.sum(1)
    q = t / Zt[:, None]
    on = q > 0
    w = x - np.log(Zt)[:, None]
    qlogp = np.where(on, q * logp, 0.0)
    qw = np.where(on, q * w, 0.0)
    ce, Hq = -qlogp.sum(1), -qw.sum(1)
    kl = ce - Hq
    best = np.argmax(a == 0, 1)   # (the first of them)
    logp_best = logp[np.arange(len(a)), best]
    # the tolerances
    e_t = 2 * U * np.abs(x) + 4 * U
    e_Z = (q * e_t).sum(1) + 64 * U
    E_q = q * (e_t + e_Z[:, None] + U)
    tol_logp = lattice_ref.logp_tol(logp)
    tiny_ce = TINY * np.abs(logp).max(1)
    tol_ce = (q * tol_logp + E_q * np.abs(logp)).sum(1) + 65 * U * np.abs(qlogp).sum(1) + tiny_ce
    wf = np.where(np.isfinite(w), w, 0.0)   # (q_j == 0 there: the term is not summed)
    xf = np.where(np.isfinite(x), x, 0.0)
    dw = 2 * U * np.abs(xf) + e_Z[:, None] + 4 * U * np.abs(np.log(Zt))[:, None] + U * np.abs(wf)
    tol_Hq = (q * dw + E_q * np.abs(wf)).sum(1) + 65 * U * np.abs(qw).sum(1) + TINY * np.abs(wf).max(1)
    tol_kl = tol_ce + tol_Hq + U * np.abs(kl)
    return {"a": a, "x": x, "q": q, "Zt": Zt, "ce": ce, "Hq": Hq, "kl": kl, "best": best, "logp_best": logp_best,
            "P": P, "logp": logp, "E_q": E_q, "e_Z": e_Z, "tol_logp": tol_logp, "tol_ce": tol_ce, "tol_kl": tol_kl,
            "tol_best": lattice_ref.logp_tol(logp_best)}


def grad(s, g):
    """dlogits (B, 64) of upstream g (B,) on ce, and its tolerance, from soft()'s dict."""
    g = np.asarray(g, np.float64)[:, None]
    want = g * (s["P"] - s["q"])
    tol = np.abs(g) * (s["P"] * (s["tol_logp"] + 4 * U + s["e_Z"][:, None] + 65 * U) + s["E_q"]
                       + 2 * U * np.abs(s["P"] - s["q"])) + TINY
    return want, tol


def upstream(B, seed=0):
    """(B,) float32 non-unit upstream gradients in +-2, none of them 0."""
    g = np.random.RandomState(11 + seed).uniform(-2, 2, B)
    return np.where(np.abs(g) < 0.05, 0.5, g).astype(np.float32)
