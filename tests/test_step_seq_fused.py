"""cn_step_seq's multi-step launches (the SEQ kernels: a step workgroup runs a chunk of steps of its own envs in
one launch) against the per-step path (chunk 1: the single-step kernels, one launch per step, which the rest of
the suite pins against the oracle): the whole state blob and all nine outputs of the last step, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd import _lib
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config

pytestmark = pytest.mark.gpu

OUTPUTS = ("robot_node", "temporal_edges", "spatial_edges", "reward", "done", "event", "info", "ep_return", "ep_len")


def _cfg(N=10, kin="unicycle", E=64, rng="mt19937", time_limit=None):
    c = clone_config(Config())
    c.sim.human_num = N
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.env.rng = rng
    if time_limit is not None:
        c.env.time_limit = time_limit
    return make_cn_config(c, num_envs=E, nenv=E, phase="train")


def _actions(T, E, kin, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    if kin == "unicycle":
        return (torch.rand((T, E, 2), generator=g, device="cuda:0") * 0.2 - 0.1).contiguous()
    return (torch.randn((T, E, 2), generator=g, device="cuda:0") * 0.5).contiguous()


def _run(cfg, acts, ops, chunk=None, state0=None, budget=None, stats=None):
    """A fresh engine from cn_reset (or cn_set_state of `state0`), then `ops`: ("seq", a, b) = one step_seq call
    over acts[a:b], ("step", t) = one step call. Returns the nine outputs of the last step and the state blob."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(cfg, "cuda:0")
    if chunk is not None:
        eng.set_seq_chunk(chunk)
    if budget is not None:
        eng.set_spawn_budget(budget)
    if state0 is None:
        eng.reset()
    else:
        eng.set_state(state0)
    s0 = eng.spawn_stats() if stats is not None else None
    for op in ops:
        if op[0] == "seq":
            eng.step_seq(acts[op[1]:op[2]])
        else:
            eng.step(acts[op[1]])
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in OUTPUTS}
    sv = eng.get_state()
    out["state"] = np.asarray(sv.blob).view(np.uint8).copy()
    if stats is not None:
        s1 = eng.spawn_stats()
        stats.update({k: s1[k] - s0[k] for k in s1})
        stats["reset_count"] = np.asarray(sv.reset_count).astype(np.int64).copy()
    eng.close()
    return out


def _same(got, ref, what):
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s: %s" % (what, k))


def _state_after(cfg, acts, n):
    """A state to start from with cn_set_state: `n` single steps after cn_reset."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    eng = CrowdNavEngine(cfg, "cuda:0")
    eng.reset()
    for t in range(n):
        eng.step(acts[t])
    torch.cuda.synchronize()
    sv = eng.get_state()
    eng.close()
    return sv


@pytest.mark.parametrize("E", [13, 64])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("kin", ["unicycle", "holonomic"])
def test_chunking_equals_single_steps(kin, rng, E):
    """C2-like config (10 humans, circle_crossing, ORCA, goal changing), T = 37; E = 13 leaves a partial last
    workgroup (6 envs per workgroup). Chunk lengths 1 (the reference), 2, 5, 8 and 64: the remainder chunk, T < C
    and chunks that divide nothing; two consecutive step_seq calls (5, then 32 steps); step_seq interleaved with
    step."""
    T = 37
    cfg = _cfg(10, kin, E, rng)
    acts = _actions(T, E, kin, 7)
    ref = _run(cfg, acts, [("step", t) for t in range(T)])
    _same(_run(cfg, acts, [("seq", 0, T)], chunk=1), ref, "chunk 1")
    for chunk in (2, 5, 8, 64):
        _same(_run(cfg, acts, [("seq", 0, T)], chunk=chunk), ref, "chunk %d" % chunk)
    _same(_run(cfg, acts, [("seq", 0, 5), ("seq", 5, T)]), ref, "two calls, default chunk")
    _same(_run(cfg, acts, [("seq", 0, 5), ("seq", 5, T)], chunk=8), ref, "two calls, chunk 8")
    _same(_run(cfg, acts, [("step", 0), ("seq", 1, 12), ("step", 12), ("step", 13), ("seq", 14, 36), ("step", 36)],
               chunk=8), ref, "interleaved with step")


@pytest.mark.parametrize("budget", [None, 1])
@pytest.mark.parametrize("start", ["reset", "set_state"])
@pytest.mark.parametrize("tl", [1, 2])
def test_many_resets_per_launch(tl, start, budget):
    """time_limit = 1: every env ends its episode at every step, so it resets 24 times inside one launch of 24
    steps (8 times at chunk 8); time_limit = 2: every few steps. An env then queues several spawns per launch:
    the one-entry-per-env-and-slot-parity cap of the spawn list. From cn_reset and from cn_set_state (whose first
    launch stays a single step: it redraws every pending spawn); at the default spawn budget and with every
    spawn parking after each human (budget 1)."""
    E, T = 64, 24
    cfg = _cfg(10, "unicycle", E, time_limit=tl)
    acts = _actions(T + 3, E, "unicycle", 23)
    state0 = _state_after(cfg, acts[T:], 3) if start == "set_state" else None
    st = {}
    ref = _run(cfg, acts, [("seq", 0, T)], chunk=1, state0=state0, budget=budget, stats=st)
    if state0 is None:   # (reset_count starts at 1 after cn_reset)
        assert (st["reset_count"] - 1 >= (T if tl == 1 else T // 5)).all(), st["reset_count"]
    for chunk in (8, 24):
        _same(_run(cfg, acts, [("seq", 0, T)], chunk=chunk, state0=state0, budget=budget), ref,
              "tl %d, %s, budget %s, chunk %d" % (tl, start, budget, chunk))


def test_small_n_quad_path():
    """3 humans per env (16 envs per workgroup, the most the quad path packs), E = 50, T = 30, chunk 8."""
    E, T = 50, 30
    cfg = _cfg(3, "holonomic", E)
    acts = _actions(T, E, "holonomic", 3)
    ref = _run(cfg, acts, [("seq", 0, T)], chunk=1)
    _same(_run(cfg, acts, [("seq", 0, T)], chunk=8), ref, "N = 3, chunk 8")


def test_resets_consume_pending_spawns_at_full_size():
    """E = 4096, T = 120 at the default chunk and spawn budget: the state equals the chunk-1 run, and some of
    the run's resets consumed a pending spawn (fewer inline draws than resets), so the equality covers both
    branches of the reset."""
    E, T = 4096, 120
    cfg = _cfg(10, "unicycle", E)
    acts = _actions(T, E, "unicycle", 11)
    ref = _run(cfg, acts, [("seq", 0, T)], chunk=1)
    st = {}
    got = _run(cfg, acts, [("seq", 0, T)], stats=st)
    resets = int((st["reset_count"] - 1).sum())
    print("resets %d, drawn inline %d, spawn stats %s" % (resets, st["inline_resets"],
                                                         {k: v for k, v in st.items() if k != "reset_count"}))
    assert resets > 0
    assert st["inline_resets"] < resets, st
    _same(got, ref, "E = 4096, default chunk")


@pytest.mark.parametrize("T", [20, 30])
def test_profile_window_counts_steps(T):
    """cn_profile(eng, 1, K) then step_seq at chunk 8: cn_profile_read reports K steps (not launches) without
    error, whether the call ends with the window (T = K = 20) or runs past it (T = 30: the chunk that would
    straddle the end of the window is split there)."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    K, E = 20, 64
    eng = CrowdNavEngine(_cfg(10, "unicycle", E), "cuda:0")
    eng.set_seq_chunk(8)
    eng.reset()
    acts = _actions(T + 2, E, "unicycle", 1)
    eng.step_seq(acts[T:T + 2])   # (the first launch after cn_reset is a single step; the window below starts in chunks)
    L = _lib.lib()
    _lib.check(L.cn_profile(eng._h, 1, K))
    eng.step_seq(acts[0:T])
    a_ms, b_ms, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    _lib.check(L.cn_profile_read(eng._h, ctypes.byref(a_ms), ctypes.byref(b_ms), ctypes.byref(n)))
    _lib.check(L.cn_profile(eng._h, 0, 0))
    eng.close()
    assert n.value == K
    assert a_ms.value > 0.0
