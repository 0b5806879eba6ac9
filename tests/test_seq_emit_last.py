"""A multi-step launch of cn_step_seq stores the caller's outputs (observation, reward, done, event, info,
ep_return, ep_len; the first observation of an episode begun by a reset) in its last step only: the earlier
steps' values would be overwritten unread. cn_step_seq at chunk 32 against the same engine configuration at
chunk 1 (the single-step kernels, one launch per step, which store every step), the whole state blob and all nine
outputs bit for bit, with envs that reset several times inside a launch and in its last step."""
import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config

pytestmark = pytest.mark.gpu

OUTPUTS = ("robot_node", "temporal_edges", "spatial_edges", "reward", "done", "event", "info", "ep_return", "ep_len")
E = 100
# N = 10: 17 workgroups of 6 envs, the last one partial; N = 3: 7 workgroups of 16 envs
SHAPES = {"n10": (10, "mt19937"), "n3": (3, "mt19937"), "n10-philox": (10, "philox")}


def _cfg(N, rng):
    c = clone_config(Config())
    c.sim.human_num = N
    c.action_space.kinematics = "unicycle"
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.env.rng = rng
    c.env.time_limit = 2   # every env resets every few steps: several times inside one launch of 32
    return make_cn_config(c, num_envs=E, nenv=E, phase="train")


def _run(shape, pre, T, chunk, poison=False):
    """A fresh engine from cn_reset and `pre` >= 1 single steps (the first launch after cn_reset is always one),
    then one step_seq call of T steps. poison: the output buffers are filled with a pattern before the call, so an
    output the last step failed to store would show."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    N, rng = SHAPES[shape]
    g = torch.Generator(device="cuda:0").manual_seed(29)
    acts = (torch.rand((pre + T, E, 2), generator=g, device="cuda:0") * 0.2 - 0.1).contiguous()
    eng = CrowdNavEngine(_cfg(N, rng), "cuda:0")
    eng.set_seq_chunk(chunk)
    eng.reset()
    for t in range(pre):
        eng.step(acts[t])
    if poison:
        torch.cuda.synchronize()
        for k in OUTPUTS:
            getattr(eng, k).fill_(77)
    eng.step_seq(acts[pre:])
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in OUTPUTS}
    sv = eng.get_state()
    out["state"] = np.asarray(sv.blob).view(np.uint8).copy()
    out["resets"] = np.asarray(sv.reset_count).astype(np.int64).copy()
    eng.close()
    return out


# time_limit 2 at time_step 0.25: an episode that nothing ends earlier times out in its 5th step, so counted from
# cn_reset the steps 5, 10, 15, ... reset most envs at once. (pre, T): single steps, then the step_seq call.
CASES = {"T1-reset-last": (4, 1), "T1": (3, 1), "T33-reset-last": (2, 33), "T33": (1, 33), "T70-reset-last": (5, 70),
         "T70": (1, 70)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_outputs_and_state_equal_single_steps(shape, case):
    """T = 70: launches of 32 + 32 + 6 steps; T = 33: a 32-step launch and a 1-step remainder launch; T = 1: a
    single-step launch. With and without a mass reset in the call's last step (there the outputs are the new
    episode's first observation, written by the reset)."""
    pre, T = CASES[case]
    ref = _run(shape, pre, T, 1)
    assert (ref["resets"] - 1 >= (pre + T) // 5).all(), ref["resets"]
    nd = int(ref["done"].sum())
    print("%s %s: %d of %d envs done in the last step" % (shape, case, nd, E))
    assert nd > E // 2 if (pre + T) % 5 == 0 else nd < E // 2
    got = _run(shape, pre, T, 32, poison=True)
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s, %s: %s" % (shape, case, k))
