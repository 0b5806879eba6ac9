"""lp2_r as a walk: each quad's linearProgram2 jumps to its next violated line (csrc/engine/orca_lp.h).

cn_debug_orca runs orca_lines_quad, the walk and lp3_r on one quad per simulator, 16 simulators per wave. Its whole
output row (velocity, failing line, line count) is compared bit for bit with the CPU: the velocity with
oracle.cpu_ref's cnref_rvo2_agent0, the failing line and the count with tests/lp_walk_helper.py's float32 trace of
RVO2's linearProgram2, which is first checked against the oracle on the same inputs (velocity, and whether
linearProgram2 failed: the oracle counts its linearProgram3 calls). What makes a batch worth running -- which
lines each simulator's loop acts on -- is asserted on the host from that trace, so it holds on any machine.

The batches (tests/golden/lp_walk_sims.npz, drawn by lp_walk_helper.generate) are the smallest at which the walk
can go wrong: 1..9 lines (both register-slot boundaries, 4 -> 5 and 8 -> 9) and none; a wave whose quads make 0, 1
and >= 5 trips; the only violated line last / first; consecutive violated lines; a line an earlier update
satisfies again and one it newly violates; failures at the first violated line, at the last line and by the
parallel-line rule; n = 1 (15 idle quads) and n = 17 (a second wave of one quad).
"""
import ctypes

import numpy as np
import pytest

from tests import lp_walk_helper as W

_CACHE = {}


def _batches():
    """name -> (simulators, their traces); loaded and traced once."""
    if not _CACHE:
        b = W.load()
        b["single"] = [b["mixed"][2]]                  # n = 1: the quad with five or more trips, 15 idle quads
        b["parallel"] = [W.parallel_fail_sim()] * 3
        for name, sims in b.items():
            _CACHE[name] = (sims, [W.trace(*s) for s in sims])
    return _CACHE


def _lp3_calls(oracle):
    c = (ctypes.c_longlong * 3)()
    oracle.lib().cnref_debug_counters(c)
    return c[1]


def _oracle_rows(oracle, name):
    """[n][4] the oracle's velocity beside the trace's failing line and line count, the trace checked against the
    oracle first."""
    sims, trs = _batches()[name]
    rows = np.zeros((len(sims), 4), np.float32)
    for k, (s, tr) in enumerate(zip(sims, trs)):
        n3 = _lp3_calls(oracle)
        v = oracle.rvo2_agent0(s[0][:, 0], s[0][:, 1], s[0][:, 2], s[0][:, 3], s[0][:, 4], float(s[1]), s[2], 10.0, 5.0, s[3])
        failed = _lp3_calls(oracle) - n3
        assert v.tobytes() == tr.velocity.tobytes(), (name, k, v, tr.velocity)
        assert failed == int(tr.fail < tr.n), (name, k, failed, tr.fail, tr.n)
        rows[k] = (v[0], v[1], tr.fail, tr.n)
    return rows


def test_trace_equals_oracle_and_batches_hold_their_premises(oracle):
    """CPU: the float32 trace gives the oracle's velocity bit for bit and fails where it does, on every batch; and
    every batch is what its name says."""
    B = _batches()
    for name in B:
        _oracle_rows(oracle, name)
    for A in range(2, 11):   # 1..9 lines and none, n = 17
        sims, trs = B["count%d" % A]
        assert len(sims) == 17 and all(len(s[0]) == A for s in sims)
        assert trs[0].n == A - 1 and trs[16].n == 0, (A, trs[0].n, trs[16].n)
        assert any(t.acted for t in trs), A
    sims, trs = B["mixed"]
    assert len(sims) == 64 and all(len(s[0]) == 10 for s in sims)
    for k, r in enumerate(W.MIXED_ROLES):   # one wave (the first 16): a quad per role, 0 / 1 / >= 5 trips among them
        assert r in W.role(trs[k]), (r, trs[k].acted, trs[k].fail, trs[k].n)
    assert len(W.MIXED_ROLES) <= 16
    assert trs[0].acted == [] and len(trs[1].acted) == 1 and len(trs[2].acted) >= 5
    assert trs[3].acted == [trs[3].n - 1] and trs[4].acted == [0]
    assert trs[8].fail < trs[8].n and trs[8].acted == [trs[8].fail]           # fails at its first violated line
    assert trs[9].fail == trs[9].n - 1                                        # fails at the last line
    for w in range(4):   # every wave mixes trip counts
        assert len({len(t.acted) for t in trs[16 * w:16 * w + 16]}) >= 3, w
    _, trs = B["parallel"]
    assert trs[0].parallel and trs[0].fail == 1 and trs[0].acted == [0, 1]
    _, trs = B["single"]
    assert len(trs) == 1 and len(trs[0].acted) >= 5


def _gpu_rows(sims):
    import torch

    from crowdnav_dsrnn_amd import _lib

    dev = torch.device("cuda:0")
    ag = torch.from_numpy(np.stack([s[0] for s in sims]).astype(np.float32)).to(dev)
    se = torch.from_numpy(np.array([[s[1], s[2][0], s[2][1]] for s in sims], np.float32)).to(dev)
    out = torch.zeros((len(sims), 4), dtype=torch.float32, device=dev)
    L = _lib.lib()
    _lib.check(L.cn_debug_orca(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), len(sims), len(sims[0][0]),
                               ag.data_ptr(), se.data_ptr(), 10.0, 5.0, float(sims[0][3]), out.data_ptr()))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


NAMES = ["count%d" % A for A in range(2, 11)] + ["mixed", "parallel", "single"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_walk_equals_oracle_bit_for_bit(oracle, name):
    """cn_debug_orca's rows out[n][4] = the oracle's velocity, the failing line and the line count, bit for bit."""
    want = _oracle_rows(oracle, name)
    got = _gpu_rows(_batches()[name][0])
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert not len(bad), (name, bad[:8], got[bad[:8]], want[bad[:8]], [_batches()[name][1][k].acted for k in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("vis", [False, True], ids=["hidden", "visible"])
def test_gpu_step_seq_equals_oracle_with_lp2_failures(oracle, vis):
    """The step kernel's multi-step launches with the walk: N = 10 (9 lines, 10 with robot.visible), E = 7 (a full
    workgroup of 6 envs and one of 1), 30 steps from reset through step_seq at the default chunk, against
    oracle.cpu_ref.RefEngine with tests/test_step_matrix.py's end-state comparison (the whole state within 1e-5, the
    MT streams by CRC). Premise, from the oracle: some human's linearProgram2 fails on the way, so lp3_tasks and
    lp3_replay run."""
    import torch

    from crowdnav_dsrnn_amd.engine import NumpyEngine
    from tests.test_gpu_parity import _cfg
    from tests.test_step_matrix import _end_state_errs

    E, T = 7, 30
    cfg = _cfg(10, "unicycle", "circle_crossing", "orca", E, robot__visible=vis)
    assert cfg.robot_visible == vis and cfg.human_num == 10
    ref, g = oracle.RefEngine(cfg), NumpyEngine(cfg)
    ref.reset()
    g.reset()
    acts = np.random.RandomState(3).uniform(-0.1, 0.1, (T, E, 2)).astype(np.float32)
    n3 = _lp3_calls(oracle)
    for t in range(T):
        ref.step(acts[t])
    assert _lp3_calls(oracle) > n3, "no linearProgram2 failed in the oracle's run"
    g.eng.step_seq(torch.from_numpy(acts).to("cuda:0"))
    torch.cuda.synchronize()
    errs = _end_state_errs(ref.get_state(), g.get_state())
    g.eng.close()
    assert not errs, errs
