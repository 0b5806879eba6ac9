"""Attention over the humans the robot sees (config.sim.visible_masks), on the GPU: the masked spatial attention
kernels (cn_spatial_attn_mask_fwd / _bwd) against the float64 composition and, bit for bit, against the fixed and
per-row-count kernels; cn_visible_mask against the engine's own belief and a numpy restatement of detect_visible on
the downloaded state; the policy and RolloutTrainer on an opt-in env."""
import types
import warnings

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config, make_varied_cn_configs
from tests.helpers import make_policy
from tests.test_gpu_parity import _actions, _cfg
from tests.test_visible_config import A, SHAPES, attn_inputs, check_vs_ref, masks_for, run_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("out", "attn", "d_hs", "d_te", "d_ws", "d_bs")


# ---- the kernels ------------------------------------------------------------------------------------------------
def _run(fn, hs, te, ws, bs, dout, datt):
    """fn(hs, te, ws, bs) -> (out, attn) on the device, backward with dout and datt: the six results on the CPU."""
    xs = [t.to(DEV).requires_grad_(True) for t in (hs, te, ws, bs)]
    out, att = fn(*xs)
    torch.autograd.backward([out, att], [dout.to(DEV), datt.to(DEV)])
    return [x.detach().cpu() for x in [out, att] + [t.grad for t in xs]]


def _assert_bits(got, want, what):
    for n, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and torch.equal(a, b), "%s: %s differs (max |d| %.3e)" % (
            what, n, float((a.double() - b.double()).abs().max()))


@pytest.mark.parametrize("R,N,Hh", SHAPES)
def test_spatial_attention_mask_kernels_vs_fp64(R, N, Hh):
    """cn_spatial_attn_mask_fwd / _bwd through ops.spatial_attention_mask vs the float64 composition (-inf-masked
    softmax, pooling): out, attn and the gradients of hs, te, ws, bs with a gradient arriving on attn too. The
    masked slots of hs and of the incoming d attn hold NaN: every output finite, attn and d hs exactly 0.0 there
    and in the empty rows, whose out, d te are 0 as well."""
    from crowdnav_dsrnn_amd import ops

    hs, te, ws, bs, dout, datt = attn_inputs(R, N, Hh)
    vis = masks_for(R, N)
    nan = ~vis.unsqueeze(-1)
    got = _run(lambda *xs: ops.spatial_attention_mask(*xs, vis.float().to(DEV), A),
               hs.masked_fill(nan, float("nan")), te, ws, bs, dout, datt.masked_fill(nan, float("nan")))
    got = [x.double() for x in got]
    want = run_fp64(hs, te, ws, bs, dout, datt, vis, N / np.sqrt(A))
    check_vs_ref(got, want, R)
    assert (got[1].squeeze(-1)[~vis] == 0.0).all() and (got[2][~vis] == 0.0).all()
    empty = vis.sum(1) == 0
    assert (got[0][empty] == 0.0).all() and (got[3][empty] == 0.0).all()
    # mask values: any nonzero number is visible, NaN and -0.0 are not
    odd = torch.where(vis, torch.rand(R, N, generator=torch.Generator().manual_seed(1)) * 4 - 5,
                      torch.tensor(float("nan")))
    odd[:, 0] = torch.where(vis[:, 0], odd[:, 0], torch.tensor(-0.0))
    again = _run(lambda *xs: ops.spatial_attention_mask(*xs, odd.to(DEV), A),
                 hs.masked_fill(nan, float("nan")), te, ws, bs, dout, datt.masked_fill(nan, float("nan")))
    _assert_bits(again, [x.float() for x in got], "mask values")


@pytest.mark.parametrize("R,N,Hh", SHAPES)
def test_full_masks_equal_fixed_attention_bit_for_bit(R, N, Hh):
    from crowdnav_dsrnn_amd import ops

    ins = attn_inputs(R, N, Hh)
    got = _run(lambda *xs: ops.spatial_attention_mask(*xs, torch.ones(R, N, device=DEV), A), *ins)
    want = _run(lambda *xs: ops.spatial_attention(*xs, N / np.sqrt(A)), *ins)
    _assert_bits(got, want, "full mask vs cn_spatial_attn_*")


@pytest.mark.parametrize("R,N,Hh", SHAPES)
def test_prefix_masks_equal_var_attention_bit_for_bit(R, N, Hh):
    """A prefix mask with the count's temperature (the mask ANDed with slot < count by the op, from an all-ones mask
    and from the prefix mask itself) against ops.spatial_attention_var with that count."""
    from crowdnav_dsrnn_amd import ops
    from tests.test_varied_humans import _counts

    ins = attn_inputs(R, N, Hh)
    count = _counts(R, N)
    prefix = (torch.arange(N)[None, :] < count[:, None]).float()
    want = _run(lambda *xs: ops.spatial_attention_var(*xs, count.to(DEV), A), *ins)
    for name, m in (("ones", torch.ones(R, N)), ("prefix", prefix)):
        got = _run(lambda *xs: ops.spatial_attention_mask(*xs, m.to(DEV), A, count.to(DEV)), *ins)
        _assert_bits(got, want, "prefix mask (%s) vs cn_spatial_attn_var_*" % name)


@pytest.mark.parametrize("R,N,Hh", SHAPES)
def test_any_mask_equals_var_attention_on_compacted_rows_bit_for_bit(R, N, Hh):
    """Arbitrary masks against cn_spatial_attn_var_fwd / _bwd run on the rows compacted on the host (visible slots
    first, in slot order; count = the number of visible slots; the same row_scale), results scattered back."""
    from crowdnav_dsrnn_amd import ops

    hs, te, ws, bs, dout, datt = attn_inputs(R, N, Hh)
    vis = masks_for(R, N)
    got = _run(lambda *xs: ops.spatial_attention_mask(*xs, vis.float().to(DEV), A), hs, te, ws, bs, dout, datt)
    idx = torch.argsort((~vis).to(torch.int8), dim=1, stable=True)                       # visible slots first
    count = vis.sum(1).to(torch.int32)
    hs_c = hs.gather(1, idx.unsqueeze(-1).expand(R, N, Hh))
    datt_c = datt.gather(1, idx.unsqueeze(-1))
    scale = ops.row_scale_full(R, N, A, torch.device(DEV))
    w = _run(lambda *xs: ops._SpatialAttnVar.apply(*xs, count.to(DEV), scale), hs_c, te, ws, bs, dout, datt_c)
    want = list(w)
    want[1] = torch.zeros(R, N, 1).scatter(1, idx.unsqueeze(-1), w[1])
    want[2] = torch.zeros(R, N, Hh).scatter(1, idx.unsqueeze(-1).expand(R, N, Hh), w[2])
    assert (want[1].squeeze(-1)[~vis] == 0).all() and (want[2][~vis] == 0).all()
    _assert_bits(got, want, "mask vs compacted cn_spatial_attn_var_*")


def test_spatial_attention_mask_rejects_bad_arguments():
    from crowdnav_dsrnn_amd import _lib

    L = _lib.lib()
    assert L.cn_spatial_attn_mask_fwd(None, 4, 65, 256, None, None, None, None, None, None, None) != 0   # N > 64
    assert L.cn_spatial_attn_mask_fwd(None, 4, 10, 96, None, None, None, None, None, None, None) != 0    # H = 96
    x = torch.zeros(4 * 10 * 256 + 4, device=DEV)
    p = x.data_ptr()
    assert L.cn_spatial_attn_mask_fwd(None, 0, 10, 256, p, p, p, p, p, p, p) != 0                        # R = 0
    assert L.cn_spatial_attn_mask_fwd(None, 4, 10, 256, None, p, p, p, p, p, p) != 0                     # null mask
    assert L.cn_spatial_attn_mask_fwd(None, 4, 10, 256, p, None, p, p, p, p, p) != 0                     # null scale
    assert L.cn_spatial_attn_mask_fwd(None, 4, 10, 256, p, p, p + 4, p, p, p, p) != 0                    # hs alignment
    assert b"cn_spatial_attn_mask_fwd" in L.cn_last_error()
    assert L.cn_spatial_attn_mask_bwd(None, 4, 10, 256, None, p, p, p, p, p, None, p, p, 256, p, 1) != 0
    assert L.cn_spatial_attn_mask_bwd(None, 4, 65, 256, p, p, p, p, p, p, None, p, p, 256, p, 1) != 0
    assert L.cn_spatial_attn_mask_bwd(None, 4, 10, 256, p, p, p, p, p, p, None, p, p, 128, p, 1) != 0    # ldu < H
    assert b"cn_spatial_attn_mask_bwd" in L.cn_last_error()
    assert L.cn_visible_mask(None, None, p) != 0 and b"cn_visible_mask" in L.cn_last_error()
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0                                                   # nothing was launched


# ---- the engine -------------------------------------------------------------------------------------------------
E, STEPS = 64, 40
BELIEF = (("b_px", "h_px"), ("b_py", "h_py"), ("b_vx", "h_vx"), ("b_vy", "h_vy"), ("b_r", "h_r"))


def _detect_visible(sv, kin, fov):
    """CrowdSim.detect_visible(robot, human, robot1=True) (crowd_sim.py:820-847) on a downloaded state, in float64:
    (visible (E, N), |angle - fov / 2| (E, N))."""
    rx, ry = np.array(sv.r_px), np.array(sv.r_py)
    th = np.arctan2(np.array(sv.r_vy), np.array(sv.r_vx)) if kin == "holonomic" else np.array(sv.r_theta)
    n_env = rx.shape[0]
    hx, hy = np.array(sv.h_px).reshape(n_env, -1), np.array(sv.h_py).reshape(n_env, -1)
    dx, dy = hx - rx[:, None], hy - ry[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (np.cos(th)[:, None] * dx + np.sin(th)[:, None] * dy) / np.sqrt(dx * dx + dy * dy)
        ang = np.arccos(np.clip(c, -1, 1))
        return np.abs(ang) <= fov / 2, np.abs(ang - fov / 2)


def _belief_is_state(sv):
    n_env = np.array(sv.r_px).shape[0]
    eq = None
    for b, h in BELIEF:
        x = np.array(getattr(sv, b)).reshape(n_env, -1).view(np.uint64) == np.array(getattr(sv, h)).reshape(n_env, -1).view(np.uint64)
        eq = x if eq is None else eq & x
    return eq


class _Tally:
    def __init__(self):
        self.slots = self.ones = self.near = self.stale_exact = 0

    def add(self, mask, sv, kin, fov):
        """One downloaded state and its mask (E, N): (a) and (b) asserted, the counts of (c) and (d) gathered."""
        assert set(np.unique(mask)) <= {0.0, 1.0}
        m = mask == 1.0
        same = _belief_is_state(sv)
        assert not (m & ~same).any(), "a visible human's belief differs from its state"              # (a)
        want, gap = _detect_visible(sv, kin, fov)
        far = gap > 1e-6
        assert (m == want)[far | np.isnan(gap)].all(), "mask differs from detect_visible away from the FOV edge"   # (b)
        self.slots += m.size
        self.ones += int(m.sum())
        self.near += int((~far & ~np.isnan(gap)).sum())
        self.stale_exact += int((~m & same).sum())

    def check(self, label, floor=100):
        print("%s: slots %d visible %.3f near-edge %d invisible-with-exact-belief %d"
              % (label, self.slots, self.ones / self.slots, self.near, self.stale_exact))
        assert self.near <= 0.005 * self.slots                                                       # (b)
        assert 0.15 <= self.ones / self.slots <= 0.85                                                # (c)
        assert self.stale_exact >= floor                                                             # (d)


@pytest.mark.parametrize("kin,fov,N", [("holonomic", 0.5, 5), ("holonomic", 1.0, 5), ("unicycle", 0.5, 5),
                                       ("unicycle", 1.0, 5), ("holonomic", 1.0, 12)])
def test_visible_mask_vs_belief_and_detect_visible(kin, fov, N):
    """64 envs x 40 free-running steps (N = 12: the kd-tree step path), state and mask downloaded after the reset and
    after every step: mask == 1 implies belief == state bit for bit; the mask equals a numpy restatement of
    detect_visible on that state wherever the angle is more than 1e-6 rad from FOV / 2 (at most 0.5 % of the slots
    excluded); both mask values fill at least 15 % of the slots; at least 100 invisible slots hold a belief bit-equal
    to the true state, so the observation does not determine the mask."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    cfg = _cfg(N, kin, "circle_crossing", "orca", E, fov)
    eng = CrowdNavEngine(cfg, DEV)
    rng = np.random.RandomState(5)
    tally = _Tally()
    eng.reset()
    for t in range(STEPS + 1):
        mask = eng.visible_mask().cpu().numpy()
        tally.add(mask, eng.get_state(), kin, np.pi * fov)
        if t < STEPS:
            eng.step(torch.from_numpy(_actions(rng, cfg, kin)).to(DEV))
    tally.check("%s FOV %.1f N %d" % (kin, fov, N))
    out = torch.full((E, N), 7.0, device=DEV)
    assert eng.visible_mask(out) is out and torch.equal(out.cpu(), torch.from_numpy(mask))
    with pytest.raises(ValueError):
        eng.visible_mask(torch.zeros(E, N + 1, device=DEV))
    eng.close()


def _varied_config(kin, fov, nums):
    c = clone_config(Config())
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.humans.policy = "orca"
    c.robot.FOV = c.humans.FOV = fov
    c.sim.human_nums = list(nums)
    return c


def test_visible_mask_on_a_mixed_engine():
    """human_nums = [1, 5, 12] (quad and kd-tree groups) at FOV 1.0, 64 envs x 40 steps: the padded slots are 0, every
    group's rows pass (a) and (b), and each env's row equals the mask of a plain one-env engine of its own count
    driven by the same actions."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    nums, kin, fov = [1, 5, 12], "holonomic", 1.0
    c = _varied_config(kin, fov, nums)
    cfgs, eg = make_varied_cn_configs(c, nums, E, nenv=E, phase="train", seed=5)
    eng = CrowdNavEngine.mixed(cfgs, eg, DEV)
    counts = eng.env_humans.tolist()
    plain = []
    for r in range(E):
        c1 = clone_config(c)
        c1.sim.human_nums, c1.sim.human_num = None, counts[r]
        plain.append(CrowdNavEngine(make_cn_config(c1, num_envs=1, env_offset=r, nenv=E, phase="train", seed=5), DEV))
    rng = np.random.RandomState(5)
    tally = _Tally()
    eng.reset()
    for p in plain:
        p.reset()
    fake = types.SimpleNamespace(num_envs=E)
    for t in range(STEPS + 1):
        mask = eng.visible_mask()
        assert tuple(mask.shape) == (E, 12)
        assert float((mask * (~eng.human_mask).float()).abs().sum()) == 0.0               # padded slots
        rows = torch.stack([torch.nn.functional.pad(p.visible_mask()[0], (0, 12 - counts[r]))
                            for r, p in enumerate(plain)])
        assert torch.equal(mask, rows), "t=%d" % t
        m = mask.cpu().numpy()
        for env_rows, sv in eng.get_state():
            tally.add(m[np.asarray(env_rows)][:, :sv.N], sv, kin, np.pi * fov)
        if t < STEPS:
            a = torch.from_numpy(_actions(rng, fake, kin)).to(DEV)
            eng.step(a)
            for r, p in enumerate(plain):
                p.step(a[r:r + 1])
    tally.check("mixed [1, 5, 12]")
    eng.close()
    for p in plain:
        p.close()


def _env_config(fov, visible, kin="holonomic", N=5):
    c = clone_config(Config())
    c.sim.human_num = N
    c.action_space.kinematics = kin
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.robot.FOV = fov
    c.sim.visible_masks = visible
    return c


def test_full_fov_sees_everyone_and_the_policy_acts_as_on_the_plain_env():
    """robot.FOV = 2: every slot whose human is not coincident with the robot is 1, and a policy's act on the opt-in
    env (masked attention kernels, all slots visible) equals its act on the plain env bit for bit, step after step."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    n_env, steps = 16, 12
    pol = make_policy(5, E=n_env, T=steps, device=DEV)
    runs = []
    for visible in (True, False):
        envs = CrowdNavVecEnv(_env_config(2.0, visible), n_env, 3, DEV, nenv=n_env, phase="train")
        assert ("visible_masks" in envs.observation_space.spaces) == visible
        obs = envs.reset()
        hxs = {"human_node_rnn": torch.zeros(n_env, 1, 128, device=DEV),
               "human_human_edge_rnn": torch.zeros(n_env, 6, 256, device=DEV)}
        masks = torch.ones(n_env, 1, device=DEV)
        rec = []
        for t in range(steps):
            assert ("visible_masks" in obs) == visible
            if visible:
                sv = envs.engine.get_state()
                apart = (np.array(sv.h_px).reshape(n_env, 5) != np.array(sv.r_px)[:, None]) | (
                    np.array(sv.h_py).reshape(n_env, 5) != np.array(sv.r_py)[:, None])
                assert tuple(obs["visible_masks"].shape) == (n_env, 5)
                assert (obs["visible_masks"].cpu().numpy()[apart] == 1.0).all() and apart.mean() > 0.99
            with torch.no_grad():
                value, action, logp, hxs = pol.act(obs, hxs, masks, deterministic=True)
            rec.append((value.cpu(), action.cpu(), logp.cpu(), hxs["human_human_edge_rnn"].cpu().clone()))
            out = envs.step_device(action)
            obs = {k: v.clone() for k, v in out[0].items()}
            masks = (1.0 - out[2].float()).unsqueeze(1)
        runs.append(rec)
        envs.close()
    for t, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), "t=%d" % t


def test_opt_in_env_of_varying_human_count():
    """sim.human_nums with sim.visible_masks: 'visible_masks' (E, 12) sits next to 'detected_human_num', is 0 in the
    padded slots, and the policy acts on it (count and mask together) with finite outputs; the same policy on the
    observation with an all-ones mask acts as it does without the key, bit for bit (the padding is masked either
    way)."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    n_env = 12
    c = _varied_config("holonomic", 0.5, [1, 5, 12])
    c.sim.visible_masks = True
    envs = CrowdNavVecEnv(c, n_env, 5, DEV, nenv=n_env, phase="train")
    assert list(envs.observation_space.spaces) == ["robot_node", "temporal_edges", "spatial_edges",
                                                   "detected_human_num", "visible_masks"]
    pol = make_policy(12, E=n_env, T=4, device=DEV)
    obs = envs.reset()
    hxs = {"human_node_rnn": torch.zeros(n_env, 1, 128, device=DEV),
           "human_human_edge_rnn": torch.zeros(n_env, 13, 256, device=DEV)}
    masks = torch.ones(n_env, 1, device=DEV)
    seen = 0.0
    for t in range(6):
        m = obs["visible_masks"]
        assert tuple(m.shape) == (n_env, 12) and float((m * (~envs.engine.human_mask).float()).sum()) == 0.0
        seen += float(m.sum())
        with torch.no_grad():
            value, action, logp, new_hxs = pol.act(obs, {k: v.clone() for k, v in hxs.items()}, masks,
                                                   deterministic=True)
            ones = dict(obs, visible_masks=torch.ones_like(m))
            plain = {k: v for k, v in obs.items() if k != "visible_masks"}
            a = pol.act(ones, {k: v.clone() for k, v in hxs.items()}, masks, deterministic=True)
            b = pol.act(plain, {k: v.clone() for k, v in hxs.items()}, masks, deterministic=True)
        assert torch.isfinite(value).all() and torch.isfinite(action).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        hxs = new_hxs
        out = envs.step_device(action)
        obs = {k: v.clone() for k, v in out[0].items()}
        masks = (1.0 - out[2].float()).unsqueeze(1)
    assert seen > 0
    envs.close()


def test_visible_mask_graph_replay_equals_eager():
    """A HIP graph of 8 step_device calls of an opt-in env (engine in graph mode: cn_visible_mask is one more kernel
    node per step) replayed once equals 8 eager calls, masks and observations."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv

    n_env, T = 64, 8
    g = torch.Generator(device=DEV).manual_seed(9)
    acts = (torch.randn((T + 1, n_env, 2), generator=g, device=DEV) * 0.6).contiguous()
    res = []
    for graph in (False, True):
        envs = CrowdNavVecEnv(_env_config(0.5, True), n_env, 0, DEV)
        envs.reset()
        envs.step_device(acts[0])        # one eager step before the capture, as RolloutTrainer's warm-up
        rec_m = torch.zeros((T, n_env, 5), device=DEV)
        rec_s = torch.zeros((T, n_env, 5, 2), device=DEV)
        if graph:
            buf = acts[1:].clone()
            envs.engine.set_graph_mode(True)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for t in range(T):
                    o = envs.step_device(buf[t])[0]
                    rec_m[t].copy_(o["visible_masks"])
                    rec_s[t].copy_(o["spatial_edges"])
            envs.engine.set_graph_mode(False)   # (recorded, not run: the device sequence is unchanged)
            envs.engine.set_graph_mode(True)
            gr.replay()
            torch.cuda.synchronize()
            envs.engine.set_graph_mode(False)
        else:
            for t in range(T):
                o = envs.step_device(acts[1 + t])[0]
                rec_m[t].copy_(o["visible_masks"])
                rec_s[t].copy_(o["spatial_edges"])
        torch.cuda.synchronize()
        res.append((rec_m.cpu().numpy(), rec_s.cpu().numpy()))
        envs.close()
    assert (res[0][0][1:] != res[0][0][:-1]).any() and 0.1 < res[0][0].mean() < 0.9
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


# ---- the policy and the learner ---------------------------------------------------------------------------------
def _policy_batch(content_seed):
    """Observations (T, B, ...) at N = 7 with a visibility pattern that has empty rows; the masked slots of
    spatial_edges hold values drawn from content_seed, everything else comes from one fixed seed."""
    T, B, N = 4, 6, 7
    g = torch.Generator().manual_seed(3)
    obs = {"robot_node": torch.randn(T, B, 1, 7, generator=g), "temporal_edges": torch.randn(T, B, 1, 2, generator=g),
           "spatial_edges": torch.randn(T, B, N, 2, generator=g) * 3}
    vis = torch.rand(T, B, N, generator=g) < 0.5
    vis[0, 0] = vis[2, 3] = False                                                        # rows that see nobody
    vis[1, 1] = True
    fill = torch.randn(T, B, N, 2, generator=torch.Generator().manual_seed(content_seed)) * 5
    obs["spatial_edges"] = torch.where(vis.unsqueeze(-1), obs["spatial_edges"], fill)
    obs["visible_masks"] = vis.float()
    hxs = {"human_node_rnn": torch.randn(B, 1, 128, generator=g) * 0.3,
           "human_human_edge_rnn": torch.randn(B, N + 1, 256, generator=g) * 0.3}
    masks = torch.ones(T, B, 1)
    masks[2, 1] = 0.0
    actions = torch.randn(T, B, 2, generator=g)
    return obs, hxs, masks, actions, vis


def test_masked_slot_content_is_inert_for_the_attention_and_gradients_are_finite():
    """Two observations that differ only in the spatial_edges of masked slots: the attention (weights and pooled
    vector) of a step taken from equal edge states is equal, exactly, in SRNN._infer_step's and in the training
    path's first step, with attention 0 on the masked slots. evaluate_actions over T = 4 with rows that see nobody:
    finite outputs and finite parameter gradients."""
    T, B, N = 4, 6, 7
    pol = make_policy(N, E=B, T=T, device=DEV)
    seen = []
    hook = pol.base.attn.register_forward_hook(lambda m, i, o: seen.append((o[0].detach().cpu(), o[1].detach().cpu())))
    grads = None
    for seed in (21, 22):
        obs, hxs, masks, actions, vis = _policy_batch(seed)
        to = lambda d: {k: v.to(DEV) for k, v in d.items()}   # noqa: E731
        with torch.no_grad():
            pol.act(to({k: v[0] for k, v in obs.items()}), to({k: v.clone() for k, v in hxs.items()}),
                    masks[0].to(DEV), deterministic=True)
        pol.zero_grad()
        flat = to({k: v.reshape(T * B, *v.shape[2:]) for k, v in obs.items()})
        value, logp, ent, _ = pol.evaluate_actions(flat, to({k: v.clone() for k, v in hxs.items()}),
                                                   masks.reshape(T * B, 1).to(DEV), actions.reshape(T * B, 2).to(DEV))
        assert torch.isfinite(value).all() and torch.isfinite(logp).all() and torch.isfinite(ent).all()
        (value.sum() + logp.sum() + ent).backward()
        grads = {k: p.grad.detach().cpu() for k, p in pol.named_parameters() if p.grad is not None}
        assert len(grads) > 20 and all(bool(torch.isfinite(v).all()) for v in grads.values())
    hook.remove()
    (w_a0, a_a0), (w_t0, a_t0), (w_a1, a_a1), (w_t1, a_t1) = seen
    assert not torch.equal(_policy_batch(21)[0]["spatial_edges"], _policy_batch(22)[0]["spatial_edges"])
    # act: the step's masked slots feed only their own edge states, which the attention does not read
    assert torch.equal(w_a0, w_a1) and torch.equal(a_a0, a_a1)
    assert (a_a0.reshape(B, N)[~vis[0]] == 0).all() and float(w_a0[0, 0].abs().max()) == 0.0
    # training path: step 0 starts from the same states (later steps carry the masked slots' own GRU history on)
    assert torch.equal(w_t0[0], w_t1[0]) and torch.equal(a_t0[:B], a_t1[:B])
    assert (a_t0.reshape(T, B, N)[~vis] == 0).all()
    assert float(w_t0[0, 0].abs().max()) == 0.0 and float(w_t0[2, 3].abs().max()) == 0.0


def test_rollout_trainer_on_an_opt_in_env():
    """RolloutTrainer on an opt-in env at FOV 0.5, 16 envs x 8 steps, two updates (the second rollout is the captured
    HIP graph): finite losses, the stored masks are 0 / 1 with both values present, and the graph holds exactly one
    more kernel node per step than the plain env's (cn_visible_mask; the masked attention replaces the fixed one
    launch for launch)."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer
    from crowdnav_dsrnn_amd.learner.ppo import PPO
    from crowdnav_dsrnn_amd.policy import Policy

    T = 8

    def run(visible):
        c = _env_config(0.5, visible)
        c.training.num_processes = 16
        c.ppo.num_steps, c.ppo.num_mini_batch, c.ppo.epoch = T, 2, 2
        torch.manual_seed(5)
        envs = CrowdNavVecEnv(c, 16, c.env.seed, DEV, nenv=16, phase="train")
        pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=envs.config).to(DEV)
        agent = PPO(pol, c.ppo.clip_param, 2, 2, c.ppo.value_loss_coef, c.ppo.entropy_coef, lr=1e-3,
                    eps=c.training.eps, max_grad_norm=c.training.max_grad_norm)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            tr = RolloutTrainer(c, envs, pol, agent)
            stats = [tr.update() for _ in range(2)]
        warned = [str(x.message) for x in w if x.filename.endswith("loop.py")]
        assert tr.graphs and tr._graph is not None and not warned, warned
        for s in stats:
            assert all(np.isfinite(s[k]) for k in ("value_loss", "action_loss", "dist_entropy")), s
        audit = dict(tr.graph_audit)
        keys = sorted(pol.state_dict())
        m = tr.rollouts.obs["visible_masks"].cpu() if visible else None
        envs.close()
        return audit, keys, m

    a1, k1, m = run(True)
    a0, k0, _ = run(False)
    assert k1 == k0                                                                       # no new parameters
    assert tuple(m.shape) == (T + 1, 16, 5) and set(m.unique().tolist()) == {0.0, 1.0}
    print("graph nodes: opt-in %s plain %s" % (a1, a0))
    assert not a1.get("memset") and a1["kernel"] == a0["kernel"] + T
