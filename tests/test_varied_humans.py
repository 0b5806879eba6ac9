"""One DSRNN policy over crowds of varying size (config.sim.human_nums), on the GPU: the per-row-count spatial
attention kernels (cn_spatial_attn_var_fwd / _bwd) against the reference composition in float64, the policy on a
padded batch (padding inert; every env equal to the plain policy of its own size), the VecEnv over a mixed
engine against plain one-env engines and the oracle, and RolloutTrainer on such an env."""
import warnings

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config, make_varied_cn_configs
from tests import helpers as H
from tests.helpers import make_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 64
# every <HQ, NR> of the kernels' (H, N) ladder: H in {256, 128, 64} x (N <= 10, N > 10); (3, 10, 128) is <32, 10>'s,
# (3, 11, 128) the other side of the ladder's N <= 10
SHAPES = [(1, 1, 256), (37, 10, 256), (300, 25, 128), (5, 3, 64), (9, 64, 64), (4099, 20, 256), (3, 10, 128),
          (3, 11, 128)]
ATOL, RTOL = 2e-5, 1e-4       # the DSRNN's pinned tolerance


def _counts(R, N):
    """Seeded counts over 1..N; the first rows are pinned to 1, N and both sides of the register-held NR
    (10 / 11 for the NR = 10 kernels, 16 / 17 for NR = 16), as far as R and N allow."""
    c = torch.randint(1, N + 1, (R,), generator=torch.Generator().manual_seed(R * 7 + N)).to(torch.int32)
    for k, v in enumerate((1, N, 10, 11, 16, 17)):
        if k < R:
            c[k] = min(v, N)
    return c


def test_counts_cover_the_kernel_paths():
    """Over SHAPES the counts hold 1, N, values on both sides of NR = 10 (N <= 10 kernels hold every vector, the
    N > 10 kernels 16) and of 16, rows with padding, and a ragged last workgroup (R not a multiple of the rows
    per workgroup)."""
    seen = set()
    for R, N, Hh in SHAPES:
        c = _counts(R, N).tolist()
        seen |= {("one", 1 in c), ("full", N in c), ("pad", any(x < N for x in c))}
        if N > 10:
            seen |= {("le16", any(x <= 16 for x in c)), ("gt16", any(x > 16 for x in c)),
                     ("le10", any(x <= 10 for x in c))}
        seen.add(("ragged", R % (256 // (Hh // 4)) != 0))
    assert {k for k, v in seen if v} == {"one", "full", "pad", "le16", "gt16", "le10", "ragged"}


def _attn_inputs(R, N, Hh):
    g = torch.Generator().manual_seed(R * 11 + N)
    hs = torch.randn(R, N, Hh, generator=g)
    te = torch.relu(torch.randn(R, A, generator=g)) * 0.3
    ws = torch.randn(A, Hh, generator=g) / 16
    bs = torch.randn(A, generator=g) * 0.1
    dout = torch.randn(R, Hh, generator=g)
    datt = torch.randn(R, N, 1, generator=g)
    return hs, te, ws, bs, dout, datt


def spatial_attention_var_ref(hs, te, ws, bs, count):
    """The reference composition (spatial_embed, product, sum, per-row scale, softmax over the first count slots,
    pooling) in the operands' dtype."""
    R, N, _ = hs.shape
    real = torch.arange(N)[None, :] < count[:, None]
    scale = (count.to(hs.dtype) / np.sqrt(A)).unsqueeze(-1)
    se = hs @ ws.t() + bs
    score = (se * te.unsqueeze(1)).sum(-1) * scale
    attn = torch.softmax(score.masked_fill(~real, float("-inf")), -1).unsqueeze(-1)
    return torch.bmm(hs.transpose(1, 2), attn).squeeze(-1), attn


def _check_vs_ref(got, want, R, label=""):
    for n, a, b in zip(("out", "attn", "d_hs", "d_te", "d_ws", "d_bs"), got, want):
        # the bound of tests/test_policy.py::test_spatial_attention_kernels_vs_fp64 (d_bs is 0 in exact
        # arithmetic: rounding noise that d_ws bounds)
        ref = want[4] if n == "d_bs" else b
        tol = 2e-5 * max(1.0, float(ref.abs().max())) * (max(1.0, R / 256) if n in ("d_ws", "d_bs") else 1.0)
        print("%s%s max|err| %.3e tol %.3e" % (label, n, float((a - b).abs().max()), tol))
        assert torch.isfinite(a).all(), n
        np.testing.assert_allclose(a.numpy(), b.numpy(), atol=tol, rtol=0, err_msg=n)


@pytest.mark.parametrize("R,N,Hh", SHAPES)
def test_spatial_attention_var_kernels_vs_fp64(R, N, Hh):
    """cn_spatial_attn_var_fwd / _bwd through ops.spatial_attention_var vs the float64 composition: out, attn and
    the gradients of hs, te, ws, bs with a gradient arriving on attn too. The padded slots of hs and of the
    incoming d attn hold NaN: every output finite, attn and d hs exactly 0.0 there."""
    from crowdnav_dsrnn_amd import ops

    hs, te, ws, bs, dout, datt = _attn_inputs(R, N, Hh)
    count = _counts(R, N)
    pad = ~(torch.arange(N)[None, :] < count[:, None])                      # (R, N)
    xs = [t.to(DEV).requires_grad_(True) for t in
          (hs.masked_fill(pad.unsqueeze(-1), float("nan")), te, ws, bs)]
    out, att = ops.spatial_attention_var(*xs, count.to(DEV), A)
    torch.autograd.backward([out, att], [dout.to(DEV), datt.masked_fill(pad.unsqueeze(-1), float("nan")).to(DEV)])
    got = [x.detach().cpu().double() for x in [out, att] + [t.grad for t in xs]]

    ys = [t.double().requires_grad_(True) for t in (hs.masked_fill(pad.unsqueeze(-1), 0.0), te, ws, bs)]
    o64, a64 = spatial_attention_var_ref(*ys, count)
    torch.autograd.backward([o64, a64], [dout.double(), datt.double().masked_fill(pad.unsqueeze(-1), 0.0)])
    want = [x.detach() for x in [o64, a64] + [t.grad for t in ys]]
    _check_vs_ref(got, want, R)
    assert (got[1].squeeze(-1)[pad] == 0.0).all() and (got[2][pad] == 0.0).all()
    assert (want[2][pad] == 0.0).all()


@pytest.mark.parametrize("R,N,Hh", SHAPES)
def test_full_counts_equal_fixed_attention(R, N, Hh):
    """count = N everywhere: ops.spatial_attention_var against ops.spatial_attention, at the tolerance of the
    float64 test (prints whether the two were in fact bit-equal)."""
    from crowdnav_dsrnn_amd import ops

    hs, te, ws, bs, dout, datt = _attn_inputs(R, N, Hh)

    def run(var):
        xs = [t.to(DEV).requires_grad_(True) for t in (hs, te, ws, bs)]
        if var:
            out, att = ops.spatial_attention_var(*xs, torch.full((R,), N, dtype=torch.int32, device=DEV), A)
        else:
            out, att = ops.spatial_attention(*xs, N / np.sqrt(A))
        torch.autograd.backward([out, att], [dout.to(DEV), datt.to(DEV)])
        return [x.detach().cpu().double() for x in [out, att] + [t.grad for t in xs]]

    got, want = run(True), run(False)
    print("bit-equal:", [bool(torch.equal(a, b)) for a, b in zip(got, want)])
    _check_vs_ref(got, want, R)


def test_spatial_attention_var_rejects_bad_shapes():
    from crowdnav_dsrnn_amd import _lib

    L = _lib.lib()
    assert L.cn_spatial_attn_var_fwd(None, 4, 65, 256, None, None, None, None, None, None, None) != 0   # N > 64
    assert L.cn_spatial_attn_var_fwd(None, 4, 10, 96, None, None, None, None, None, None, None) != 0    # H = 96
    x = torch.zeros(4 * 10 * 256, device=DEV)
    p = x.data_ptr()
    assert L.cn_spatial_attn_var_fwd(None, 4, 10, 256, None, p, p, p, p, p, p) != 0                     # null count
    assert L.cn_spatial_attn_var_bwd(None, 4, 10, 256, None, p, p, p, p, p, None, p, p, 256, p, 1) != 0
    assert L.cn_spatial_attn_var_bwd(None, 4, 65, 256, p, p, p, p, p, p, None, p, p, 256, p, 1) != 0
    assert b"cn_spatial_attn_var_bwd" in L.cn_last_error()


# ---- the policy on a padded batch -------------------------------------------------------------------------------
NMAX, COUNTS, T = 7, (1, 3, 5, 7, 2, 7), 4
B = len(COUNTS)


def _policy_batch(pad_seed):
    """Observations (T, B, ...) and start states (B, ...) at N = 7 for envs of COUNTS humans; the padded
    spatial_edges slots and edge-state rows hold finite values drawn from pad_seed (None: the engine's never-seen
    human, (15, 15) relative to the robot), everything else from one fixed seed."""
    g = torch.Generator().manual_seed(3)
    obs = {"robot_node": torch.randn(T, B, 1, 7, generator=g), "temporal_edges": torch.randn(T, B, 1, 2, generator=g),
           "spatial_edges": torch.randn(T, B, NMAX, 2, generator=g) * 3}
    hxs = {"human_node_rnn": torch.randn(B, 1, 128, generator=g) * 0.3,
           "human_human_edge_rnn": torch.randn(B, NMAX + 1, 256, generator=g) * 0.3}
    cnt = torch.tensor(COUNTS)
    pad = ~(torch.arange(NMAX)[None, :] < cnt[:, None])                                     # (B, N)
    if pad_seed is None:
        fill = (15.0 - obs["robot_node"][..., :2]).expand(T, B, NMAX, 2)
        hfill = torch.zeros(B, NMAX, 256)
    else:
        gp = torch.Generator().manual_seed(pad_seed)
        fill = torch.randn(T, B, NMAX, 2, generator=gp) * 5
        hfill = torch.randn(B, NMAX, 256, generator=gp)
    obs["spatial_edges"] = torch.where(pad[None, :, :, None], fill, obs["spatial_edges"])
    hxs["human_human_edge_rnn"][:, 1:] = torch.where(pad[:, :, None], hfill, hxs["human_human_edge_rnn"][:, 1:])
    obs["detected_human_num"] = cnt.float().reshape(1, B, 1).expand(T, B, 1).contiguous()
    masks = torch.ones(T, B, 1)
    masks[2, 1] = masks[2, 4] = 0.0                                                         # episode starts at t = 2
    actions = torch.randn(T, B, 2, generator=g)
    return obs, hxs, masks, actions, pad


def _to(d, dev=DEV):
    return {k: v.to(dev) for k, v in d.items()}


def _act(pol, obs, hxs, masks):
    """act (no_grad: SRNN._infer_step) on step 0 -> base outputs and the distribution's, all on the CPU."""
    with torch.no_grad():
        o0 = _to({k: v[0] for k, v in obs.items()})
        value, feat, nh = pol.base(o0, _to({k: v.clone() for k, v in hxs.items()}), masks[0].to(DEV), infer=True)
        v2, action, logp, nh2 = pol.act(o0, _to({k: v.clone() for k, v in hxs.items()}), masks[0].to(DEV),
                                        deterministic=True)
    assert torch.equal(v2, value)
    return {"value": value.cpu(), "feat": feat.cpu(), "action": action.cpu(), "logp": logp.cpu(),
            "node": nh["human_node_rnn"].cpu(), "edge": nh["human_human_edge_rnn"].cpu()}


def _train(pol, obs, hxs, masks, actions, nb):
    """evaluate_actions over the T steps (the training path) + backward -> outputs and parameter gradients."""
    pol.zero_grad()
    flat = _to({k: v.reshape(T * nb, *v.shape[2:]) for k, v in obs.items()})
    h = _to({k: v.clone() for k, v in hxs.items()})
    value, feat, nh = pol.base(flat, dict(h), masks.reshape(T * nb, 1).to(DEV))
    v2, logp, ent, _ = pol.evaluate_actions(flat, dict(h), masks.reshape(T * nb, 1).to(DEV),
                                            actions.reshape(T * nb, 2).to(DEV))
    g = torch.Generator().manual_seed(9)
    (v2 * torch.randn(T * nb, 1, generator=g).to(DEV)).sum().add((logp * torch.randn(T * nb, 1, generator=g).to(DEV)).sum()
                                                                 ).add(ent).backward()
    grads = {k: p.grad.detach().cpu().clone() for k, p in pol.named_parameters() if p.grad is not None}
    return ({"value": v2.detach().cpu(), "feat": feat.detach().cpu(), "logp": logp.detach().cpu(),
             "ent": ent.detach().cpu(), "node": nh["human_node_rnn"].detach().cpu(),
             "edge": nh["human_human_edge_rnn"].detach().cpu()}, grads)


@pytest.fixture(scope="module")
def padded_runs():
    """The N = 7 policy on the padded batch, act and training path, for two paddings (computed once)."""
    pol = make_policy(NMAX, E=B, T=T, device=DEV)
    runs = []
    for seed in (None, 21):
        obs, hxs, masks, actions, pad = _policy_batch(seed)
        runs.append((_act(pol, obs, hxs, masks), _train(pol, obs, hxs, masks, actions, B)))
    return pol, runs, _policy_batch(None)


def test_padded_content_is_inert(padded_runs):
    """Two observation / state sets that differ only in the padded slots (the never-seen human against random
    finite values): act gives equal value, action mean, log-prob and node state and equal edge state in the real
    slots; evaluate_actions over T = 4 with an episode start at t = 2 gives equal outputs and equal parameter
    gradients. Exact: the real rows' arithmetic does not read the padded ones."""
    _, runs, (_, _, _, _, pad) = padded_runs
    (a0, (t0, g0)), (a1, (t1, g1)) = runs
    real = torch.cat((torch.ones(B, 1, dtype=torch.bool), ~pad), 1)                         # (B, N + 1)
    for k in ("value", "feat", "action", "logp", "node"):
        assert torch.equal(a0[k], a1[k]), "act " + k
    assert torch.equal(a0["edge"][real], a1["edge"][real])
    assert not torch.equal(a0["edge"][~real], a1["edge"][~real])                            # (the paddings did differ)
    for k in ("value", "feat", "logp", "ent", "node"):
        assert torch.equal(t0[k], t1[k]), "train " + k
    assert torch.equal(t0["edge"][real], t1["edge"][real])
    assert set(g0) == set(g1) and len(g0) > 20
    for k in g0:
        assert torch.isfinite(g0[k]).all() and torch.equal(g0[k], g1[k]), "grad " + k


def test_each_env_equals_plain_policy_of_its_size(padded_runs):
    """Env i of the padded batch against a Policy at human_num = COUNTS[i] (same state_dict, nenv = 1) on that
    env's unpadded observation and state: value, actor features and new hidden states, act path and T = 4
    training path, at the DSRNN's pinned tolerance."""
    pol, runs, (obs, hxs, masks, actions, _) = padded_runs
    act_v, (train_v, _) = runs[0]
    sd = pol.state_dict()
    worst = 0.0
    for i, n in enumerate(COUNTS):
        p1 = make_policy(n, E=1, T=T, device=DEV)
        p1.load_state_dict(sd)
        o = {k: obs[k][:, i:i + 1] for k in ("robot_node", "temporal_edges")}
        o["spatial_edges"] = obs["spatial_edges"][:, i:i + 1, :n]
        h = {"human_node_rnn": hxs["human_node_rnn"][i:i + 1], "human_human_edge_rnn": hxs["human_human_edge_rnn"][i:i + 1, :n + 1]}
        a = _act(p1, o, h, masks[:, i:i + 1])
        with torch.no_grad():
            t, _ = _train_nograd(p1, o, h, masks[:, i:i + 1], actions[:, i:i + 1])
        for name, got, want in (("act", act_v, a), ("train", train_v, t)):
            rows = slice(i, i + 1) if name == "act" else slice(i, None, B)                 # (T*B) rows of env i
            for k in ("value", "feat"):
                x, y = got[k][rows].numpy(), want[k].numpy()
                worst = max(worst, float(np.abs(x - y).max()))
                np.testing.assert_allclose(x, y, atol=ATOL, rtol=RTOL, err_msg="%s %s env %d" % (name, k, i))
            np.testing.assert_allclose(got["node"][i:i + 1].numpy(), want["node"].numpy(), atol=ATOL, rtol=RTOL)
            np.testing.assert_allclose(got["edge"][i:i + 1, :n + 1].numpy(), want["edge"].numpy(), atol=ATOL, rtol=RTOL,
                                       err_msg="%s edge state env %d" % (name, i))
    print("worst |value / feature difference| %.3e" % worst)


def _train_nograd(pol, obs, hxs, masks, actions):
    flat = _to({k: v.reshape(T, *v.shape[2:]) for k, v in obs.items()})
    value, feat, nh = pol.base(flat, _to({k: v.clone() for k, v in hxs.items()}), masks.reshape(T, 1).to(DEV))
    return {"value": value.cpu(), "feat": feat.cpu(), "node": nh["human_node_rnn"].cpu(),
            "edge": nh["human_human_edge_rnn"].cpu()}, None


# ---- the VecEnv -------------------------------------------------------------------------------------------------
NUMS, E, OFF, NENV, STEPS = [1, 5, 12], 12, 3, 19, 20


def _venv_cfg(kin):
    c = clone_config(Config())
    c.action_space.kinematics = kin
    c.sim.human_nums = list(NUMS)
    c.sim.human_num = 3            # (not read on this path: the env's clone carries the largest count)
    return c


@pytest.mark.parametrize("kin", ["holonomic", "unicycle"])
def test_varied_vec_env_vs_plain_engines_and_oracle(kin, oracle):
    """human_nums = [1, 5, 12] (quad and kd-tree groups), 12 envs at env_offset 3 of 19, a seeded action tape of 20
    steps. Each env's observation rows [:count], reward, done, event and info row equal those of a plain one-env
    engine at env_offset 3 + r, human_num = count, bit for bit; the same run teacher-forced against
    oracle.RefMixedEngine at the bar of tests/test_gpu_parity.py; detected_human_num == engine.env_humans; padded
    slots hold the never-seen human; make_vec_envs returns the same env."""
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv, make_vec_envs

    c = _venv_cfg(kin)
    venv = CrowdNavVecEnv(c, E, 5, DEV, env_offset=OFF, nenv=NENV)
    counts = [NUMS[(OFF + r) % 3] for r in range(E)]
    assert c.sim.human_num == 3 and c.sim.human_nums == NUMS and venv.config is not c       # caller's config untouched
    assert venv.config.sim.human_num == 12 and venv.engine.env_humans.tolist() == counts
    assert [venv.venv.envs[i].env.human_num for i in range(E)] == counts
    sp = venv.observation_space.spaces
    assert {k: tuple(v.shape) for k, v in sp.items()} == {"robot_node": (1, 7), "temporal_edges": (1, 2),
                                                          "spatial_edges": (12, 2), "detected_human_num": (1,)}
    plain = []
    for r in range(E):
        c1 = clone_config(c)
        c1.sim.human_nums, c1.sim.human_num = None, counts[r]
        plain.append(CrowdNavEngine(make_cn_config(c1, num_envs=1, env_offset=OFF + r, nenv=NENV, phase="train", seed=5),
                                    DEV))
    tape = torch.from_numpy(np.random.RandomState(8).normal(0, 0.6, (STEPS, E, 2)).astype(np.float32))

    def check(obs, t, rest=None):
        assert torch.equal(obs["detected_human_num"], venv.engine.env_humans.float().reshape(E, 1))
        for r, eng in enumerate(plain):
            n = counts[r]
            po = eng.obs()
            for k in ("robot_node", "temporal_edges"):
                assert torch.equal(obs[k][r], po[k][0]), "%s env %d t=%d" % (k, r, t)
            assert torch.equal(obs["spatial_edges"][r, :n], po["spatial_edges"][0]), "spatial env %d t=%d" % (r, t)
            if rest is not None:
                for j, name in enumerate(("reward", "done", "event", "info")):
                    x, y = rest[j][r], (eng.reward, eng.done, eng.event, eng.info)[j][0]
                    assert torch.equal(x.to(y.dtype), y) or (name == "info" and _same_with_nan(x, y)), \
                        "%s env %d t=%d: %s vs %s" % (name, r, t, x, y)
            # padded slots: the never-seen human (15, 15) relative to the robot, the same value in every slot
            if n < 12:
                padv = obs["spatial_edges"][r, n:]
                assert torch.equal(padv, padv[:1].expand_as(padv))
                want = 15.0 - obs["robot_node"][r, 0, :2].double()
                assert float((padv[0].double() - want).abs().max()) <= 1e-5, (r, t, padv[0], want)

    obs = venv.reset()
    for eng in plain:
        eng.reset()
    check(obs, -1)
    for t in range(STEPS):
        out = venv.step_device(tape[t])
        for r, eng in enumerate(plain):
            eng.step(tape[t, r:r + 1])
        check(out[0], t, out[1:5])
    obs, rew, done, infos = venv.step(tape[0])                                   # the host-side API carries the key too
    assert torch.equal(obs["detected_human_num"].cpu(), torch.tensor(counts).float().reshape(E, 1))
    assert tuple(rew.shape) == (E, 1) and len(infos) == E

    # the same tape, teacher-forced against the oracle's mixed engine
    cfgs, eg = make_varied_cn_configs(c, NUMS, E, env_offset=OFF, nenv=NENV, phase="train", seed=5)
    ref = oracle.RefMixedEngine(cfgs, eg)
    ref.reset()
    for t in range(STEPS):
        pre = ref.get_state()
        venv.engine.set_state(pre)
        a = tape[t].numpy()
        r_out = ref.step(a)
        g = venv.step_device(tape[t])
        torch.cuda.synchronize()
        g_out = [{k: v.cpu().numpy() for k, v in g[0].items()}] + [x.cpu().numpy() for x in g[1:]]
        np.testing.assert_array_equal(g_out[2], r_out[2], err_msg="done t=%d" % t)
        np.testing.assert_array_equal(g_out[3], r_out[3], err_msg="event t=%d" % t)
        np.testing.assert_allclose(g_out[1], r_out[1], atol=1e-5, rtol=0, err_msg="reward t=%d" % t)
        for k in ("robot_node", "temporal_edges", "spatial_edges"):
            np.testing.assert_allclose(g_out[0][k], r_out[0][k], atol=1e-5, rtol=0, err_msg="%s t=%d" % (k, t))
        errs = []
        for (rows, rs), (_, gs) in zip(ref.get_state(), venv.engine.get_state()):
            d = {"post_" + n: np.asarray(getattr(rs, n)) for n, _, _ in abi.STATE_FIELDS if n != "mt"}
            d["post_mt_crc"] = H.mt_crc(rs)
            errs += H.compare_state(gs, d, "post_", tol=1e-5, where="t=%d " % t)
        errs += H.compare_info(g_out[4], r_out[4], r_out[3], where="t=%d " % t)
        errs += H.compare_monitor(g_out[5], g_out[6], r_out[5], r_out[6], r_out[2], where="t=%d " % t)
        assert not errs, errs
    venv.close()

    # make_vec_envs with config.sim.human_nums: the same env (shard 0 of 1 here, so the offset is 0)
    a = make_vec_envs("CrowdSimDict-v0", 5, E, 0.99, None, DEV, False, config=c)
    b = CrowdNavVecEnv(c, E, 5, DEV, nenv=E)
    assert type(a) is type(b) and a.human_nums == b.human_nums == NUMS and a.env_human_nums == b.env_human_nums
    assert list(a.observation_space.spaces) == list(b.observation_space.spaces)
    oa, ob = a.reset(), b.reset()
    assert all(torch.equal(oa[k], ob[k]) for k in ob) and set(oa) == set(ob)
    a.close()
    b.close()


def _same_with_nan(x, y):
    return bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all())


# ---- the trainer ------------------------------------------------------------------------------------------------
def test_rollout_trainer_on_varied_env_stays_eager():
    """RolloutTrainer on an env of varying human count, 16 envs x 8 steps, two updates: eager rollouts chosen up
    front (no capture, no warning), finite losses, every parameter with a non-zero gradient moved, the storage's
    detected_human_num constant over time; the same two updates on a plain env capture their graph as before."""
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner.loop import RolloutTrainer
    from crowdnav_dsrnn_amd.learner.ppo import PPO
    from crowdnav_dsrnn_amd.policy import Policy

    def run(nums):
        c = clone_config(Config())
        c.sim.human_num = 5
        c.sim.human_nums = nums
        c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
        c.training.num_processes = 16
        c.ppo.num_steps, c.ppo.num_mini_batch, c.ppo.epoch = 8, 2, 2
        torch.manual_seed(5)
        envs = CrowdNavVecEnv(c, 16, c.env.seed, DEV, nenv=16, phase="train")
        pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=envs.config).to(DEV)
        agent = PPO(pol, c.ppo.clip_param, 2, 2, c.ppo.value_loss_coef, c.ppo.entropy_coef, lr=1e-3,
                    eps=c.training.eps, max_grad_norm=c.training.max_grad_norm)
        before = {k: p.detach().clone() for k, p in pol.named_parameters()}
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            tr = RolloutTrainer(c, envs, pol, agent)
            stats = [tr.update() for _ in range(2)]
        # (the trainer's own warnings: a failed capture or a memset node in the graph, both raised in loop.py)
        return c, envs, pol, tr, stats, before, [str(x.message) for x in w if x.filename.endswith("loop.py")]

    c, envs, pol, tr, stats, before, warned = run([3, 5, 8])
    assert not tr.graphs and tr._graph is None and tr.graph_audit is None
    assert not warned, warned
    for s in stats:
        assert all(np.isfinite(s[k]) for k in ("value_loss", "action_loss", "dist_entropy")), s
    moved = still = 0
    for k, p in pol.named_parameters():
        if p.grad is not None and float(p.grad.abs().max()) > 0:
            assert not torch.equal(p.detach(), before[k]), k
            moved += 1
        else:
            still += 1
    assert moved > 20, (moved, still)
    d = tr.rollouts.obs["detected_human_num"]
    assert tuple(d.shape) == (9, 16, 1)
    assert torch.equal(d, envs.engine.env_humans.float().reshape(1, 16, 1).expand(9, 16, 1))
    assert sorted(set(envs.engine.env_humans.tolist())) == [3, 5, 8]
    envs.close()

    _, envs, _, tr, stats, _, warned = run(None)
    assert tr.graphs and tr._graph is not None and not warned, warned
    envs.close()
