"""The lattice action head without a GPU: the torch restatements of include/crowdnav.h's definition (ops.*_torch)
against its float64 numpy statement (tests/lattice_ref.py), Policy(..., head='lattice') on the CPU, and the argument
checks of the three cn_lattice_* entry points (the library loads on the CPU, as in tests/test_abi.py)."""
import os

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd import _lib, ops
from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config
from crowdnav_dsrnn_amd.policy import LatticeCategorical, Policy
from crowdnav_dsrnn_amd.policy_factory import DWA_GRID
from crowdnav_dsrnn_amd.spaces import action_space, lidar_observation_space
from tests import lattice_ref as ref
from tests.helpers import GOLDEN, BoxSpace, attention_pool_ref, edge_features_fp32, gru_infer_step_ref, masked_gru_ref

EINVAL = -1


# ---- the lattice and the index ----------------------------------------------------------------------------------
def test_lattice_is_the_dwa_grid_bit_for_bit_and_round_trips():
    a = ops.lattice_actions().numpy()
    g = np.array(DWA_GRID, np.float64).astype(np.float32)
    assert a.dtype == np.float32 and a.shape == (64, 2)
    assert np.array_equal(a, np.stack([np.repeat(g, 8), np.tile(g, 8)], 1))
    assert np.array_equal(a, ref.ACTIONS32)
    assert np.array_equal(ops.lattice_index(torch.from_numpy(a)).numpy(), np.arange(64))
    assert np.array_equal(ref.index(a), np.arange(64))


def test_index_is_the_nearest_lattice_point_off_the_lattice_and_the_stated_one_at_ties():
    rs = np.random.RandomState(3)
    x = rs.uniform(-0.2, 0.2, (4000, 2)).astype(np.float32)
    got = ops.lattice_index(torch.from_numpy(x)).numpy()
    assert np.array_equal(got, ref.index(x))
    # away from the midpoints between lattice coordinates the stated index is the nearest point in float64
    mid = (ref.GRID[:-1] + ref.GRID[1:]) / 2
    clear = (np.abs(x.astype(np.float64)[:, :, None] - mid[None, None, :]).min(-1) > 1e-6).all(1)
    near = np.abs(x.astype(np.float64)[:, :, None] - ref.GRID[None, None, :]).argmin(-1)
    assert clear.sum() > 3900
    assert np.array_equal(got[clear], (near[:, 0] * 8 + near[:, 1])[clear])
    # half-way points (as near as float32 holds them) and the ends of the range: the float32 statement decides
    t = np.concatenate([mid, mid + 1e-9, mid - 1e-9, [-1.0, 1.0, -0.1, 0.1, 0.0]]).astype(np.float32)
    ties = np.stack([t, t[::-1]], 1)
    assert np.array_equal(ops.lattice_index(torch.from_numpy(ties)).numpy(), ref.index(ties))
    assert ops.lattice_index(torch.tensor([[-1.0, 1.0]])).item() == 7 and ops.lattice_index(
        torch.tensor([[1.0, -1.0]])).item() == 56


# ---- act: mode and sample ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    E = 257
    return ref.rows(E), ref.draws(E)


def test_mode_of_the_restatement_is_exact(case):
    logits, _ = case
    action, logp, c = ops.lattice_act_torch(torch.from_numpy(logits), None)
    want = ref.mode(logits)
    assert np.array_equal(c.numpy(), want)
    kinds = np.arange(len(want)) % ref.KINDS
    assert (want[kinds == 0] == 0).all() and (want[kinds == 1] == 0).all() and (want[kinds == 2] == 63).all()
    assert (want[kinds == 5] == 17).all()
    assert np.array_equal(action.numpy(), ref.ACTIONS32[want])
    s = ref.softmax(logits)
    lp = s["logp"][np.arange(len(want)), want]
    assert (np.abs(logp.numpy()[:, 0] - lp) <= ref.logp_tol(lp)).all()
    assert logp.shape == (len(want), 1) and logp.dtype == torch.float32


def test_sample_of_the_restatement_follows_the_interval_rule(case):
    logits, u = case
    action, logp, c = ops.lattice_act_torch(torch.from_numpy(logits), torch.from_numpy(u))
    c = c.numpy()
    assert not ref.sample_errors(logits, u, c)
    assert np.array_equal(action.numpy(), ref.ACTIONS32[c])
    s = ref.softmax(logits)
    lp = s["logp"][np.arange(len(c)), c]
    assert (np.abs(logp.numpy()[:, 0] - lp) <= ref.logp_tol(lp)).all()
    # u = 0 takes the first candidate of nonzero float32 probability, u = 1 - 2^-24 one at the far end of the mass
    live = s["d"] > ref.EXP_FLOOR
    zero = np.nonzero(u == 0)[0]
    assert len(zero) > 30 and np.array_equal(c[zero], live[zero].argmax(1))
    top = np.nonzero(u == ref.U_MAX)[0]
    assert len(top) > 30 and (s["S"][top, c[top]] >= (1 - 1e-5) * s["Z"][top]).all()
    # the spread rows: the 23 candidates more than 104 below the maximum (steps of 160 / 63) have p = 0 in float32
    # and are never drawn (sample_errors checks it per row); here that the rows are what they claim
    spread = np.arange(len(c)) % ref.KINDS == 4
    assert ((~live[spread]).sum(1) == 23).all()


def test_sample_of_the_restatement_never_leaves_the_row_empty_handed():
    """Rounding may leave no S_c above u * S_63 (u = 1 - 2^-24 with the total held by the first lanes): the highest
    candidate with p_c > 0 then, never one with p_c == 0."""
    l = np.full((1, 64), -200.0, np.float32)
    l[0, 5], l[0, 9] = 0.0, -20.0
    for u in (0.0, 0.5, float(ref.U_MAX)):
        c = ops.lattice_act_torch(torch.from_numpy(l), torch.tensor([u]))[2].item()
        assert c in (5, 9) and not ref.sample_errors(l, [u], [c])


# ---- evaluate ---------------------------------------------------------------------------------------------------
def test_evaluate_restatement_vs_float64(case):
    logits = case[0]
    B = len(logits)
    actions = ref.eval_actions(B)
    lt = torch.from_numpy(logits).requires_grad_(True)
    logp, ent = ops.lattice_evaluate(lt, torch.from_numpy(actions))   # (CPU tensors: the restatement)
    s = ref.softmax(logits)
    idx = ref.index(actions)
    lp = s["logp"][np.arange(B), idx]
    assert logp.shape == (B, 1) and ent.shape == (B,)
    assert (np.abs(logp.detach().numpy()[:, 0] - lp) <= ref.logp_tol(lp)).all()
    assert (np.abs(ent.detach().numpy() - s["H"]) <= ref.logp_tol(s["H"])).all()
    rs = np.random.RandomState(5)
    g_lp, g_H = rs.uniform(-2, 2, B), rs.uniform(-2, 2, B)
    (logp[:, 0] * torch.from_numpy(g_lp).float()).sum().add((ent * torch.from_numpy(g_H).float()).sum()).backward()
    onehot = np.eye(64)[idx]
    want = g_lp[:, None] * (onehot - s["q"]) - g_H[:, None] * s["q"] * (s["logp"] + s["H"][:, None])
    got = lt.grad.numpy()
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= ref.logp_tol(want)).all()


# ---- Policy -----------------------------------------------------------------------------------------------------
def _config(kin="unicycle", head=None, N=5, E=4):
    c = clone_config(Config())
    c.sim.human_num = N
    c.action_space.kinematics = kin
    c.training.num_processes = E
    c.ppo.num_steps, c.ppo.num_mini_batch = 8, 1
    if head is not None:
        c.robot.action_head = head
    return c


def _cpu_ops(monkeypatch):
    monkeypatch.setattr(ops, "edge_features", edge_features_fp32)
    monkeypatch.setattr(ops, "masked_gru", masked_gru_ref)
    monkeypatch.setattr(ops, "gru_infer_step", gru_infer_step_ref)
    monkeypatch.setattr(ops, "attention_pool", attention_pool_ref)


def test_lattice_policy_on_the_cpu(monkeypatch):
    _cpu_ops(monkeypatch)
    d = np.load(os.path.join(GOLDEN, "dsrnn.npz"))
    torch.manual_seed(2)
    pol = Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config(), head="lattice").eval()
    assert isinstance(pol.dist, LatticeCategorical) and pol.head == "lattice"
    w = pol.dist.fc_logits.weight
    assert tuple(w.shape) == (64, pol.base.output_size) and not pol.dist.fc_logits.bias.detach().any()
    assert float(w.detach().abs().max()) < 0.01   # orthogonal with gain 0.01: near-uniform at the start
    p = "N5_act_"
    obs = {k: torch.from_numpy(d[p + "obs_" + k]) for k in ("robot_node", "temporal_edges", "spatial_edges")}
    hxs = {k: torch.from_numpy(d[p + "hxs_" + k].copy()) for k in ("human_node_rnn", "human_human_edge_rnn")}
    masks = torch.from_numpy(d[p + "masks"])
    E = masks.shape[0]
    lattice = {tuple(r) for r in ref.ACTIONS32.tolist()}
    with torch.no_grad():
        for det in (True, False):
            v, a, lp, _ = pol.act(obs, hxs, masks, deterministic=det)
            assert tuple(v.shape) == (E, 1) and tuple(a.shape) == (E, 2) and tuple(lp.shape) == (E, 1)
            assert a.dtype == torch.float32 and lp.dtype == torch.float32
            assert all(tuple(r) in lattice for r in a.tolist())
            assert (lp < 0).all() and (lp - np.log(1 / 64)).abs().max() < 0.05   # near-uniform logits
    v, a, lp, _ = pol.act(obs, hxs, masks, deterministic=True)   # (the autograd path: the distribution object)
    assert all(tuple(r) in lattice for r in a.tolist()) and lp.requires_grad
    p = "N5_ev_"
    obs = {k: torch.from_numpy(d[p + "obs_" + k]) for k in ("robot_node", "temporal_edges", "spatial_edges")}
    hxs = {k: torch.from_numpy(d[p + "hxs_" + k].copy()) for k in ("human_node_rnn", "human_human_edge_rnn")}
    actions = torch.from_numpy(d[p + "actions"])   # continuous labels: scored at the nearest lattice point
    v, lp, ent, _ = pol.evaluate_actions(obs, hxs, torch.from_numpy(d[p + "masks"]), actions)
    B = actions.shape[0]
    assert tuple(v.shape) == (B, 1) and tuple(lp.shape) == (B, 1) and ent.dim() == 0
    assert abs(float(ent.detach()) - np.log(64)) < 0.01
    (-lp.mean() - 0.01 * ent).backward()
    g = pol.dist.fc_logits.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_lattice_head_is_the_unicycle_robots_and_an_opt_in():
    with pytest.raises(UnsupportedConfig):
        Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config("holonomic"), head="lattice")
    with pytest.raises(UnsupportedConfig):
        Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config("holonomic", head="lattice"))
    with pytest.raises(UnsupportedConfig):
        Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config(), head="mixture")
    assert Config().robot.action_head == "gaussian"
    # head=None reads the config; an explicit head overrides it
    assert Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config(head="lattice")).head == "lattice"
    assert Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config(head="lattice"), head="gaussian").head == "gaussian"


def test_state_dict_keys_of_both_heads():
    ref_keys = list(np.load(os.path.join(GOLDEN, "dsrnn.npz"))["N5_keys"])
    default = Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config())
    assert default.head == "gaussian" and sorted(default.state_dict().keys()) == ref_keys
    z = np.load(os.path.join(GOLDEN, "ckpt_55554.npz"))   # the reference's unicycle checkpoint still loads
    default.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files})
    lat = Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=_config(), head="lattice")
    keys = set(lat.state_dict().keys())
    assert {"dist.fc_logits.weight", "dist.fc_logits.bias"} <= keys
    assert not [k for k in keys if "fc_mean" in k or "logstd" in k]
    assert keys - {"dist.fc_logits.weight", "dist.fc_logits.bias"} == {k for k in ref_keys if not k.startswith("dist.")}


def test_convgru_base_takes_the_lattice_head():
    c = _config()
    c.robot.policy = "convgru"
    pol = Policy(lidar_observation_space(180), action_space(), base="convgru", base_kwargs=c, head="lattice")
    assert pol.dist.fc_logits.in_features == pol.base.actor.fc2.out_features
    assert "dist.fc_logits.weight" in pol.state_dict()


# ---- the C entry points -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from crowdnav_dsrnn_amd import build

    build.build()
    return _lib.lib()


def test_entry_points_reject_bad_arguments_without_launching(L):
    """Null or non-positive arguments: CN_EINVAL before any launch (the non-null dummy addresses are never
    dereferenced; there is no GPU in this test), each entry point naming itself in cn_last_error()."""
    for name in ("cn_lattice_act", "cn_lattice_eval_fwd", "cn_lattice_eval_bwd"):
        assert name in _lib.EXPORTED and hasattr(L, name)

    def rejected(rc, who):
        return rc == EINVAL and who in L.cn_last_error()

    # cn_lattice_act(stream, E, logits, u, action, logp, choice): u and choice may be NULL
    act = b"cn_lattice_act"
    assert rejected(L.cn_lattice_act(None, 0, 16, 32, 48, 64, 80), act)
    assert rejected(L.cn_lattice_act(None, -3, 16, 32, 48, 64, 80), act)
    assert rejected(L.cn_lattice_act(None, 4 * (2 ** 31 - 1) + 1, 16, 32, 48, 64, 80), act)
    assert rejected(L.cn_lattice_act(None, 4, None, 32, 48, 64, 80), act)
    assert rejected(L.cn_lattice_act(None, 4, 16, None, None, 64, None), act)
    assert rejected(L.cn_lattice_act(None, 4, 16, None, 48, None, None), act)
    # cn_lattice_eval_fwd(stream, B, logits, actions, logp, entropy, choice)
    fwd = b"cn_lattice_eval_fwd"
    assert rejected(L.cn_lattice_eval_fwd(None, 0, 16, 32, 48, 64, 80), fwd)
    for k in range(5):
        args = [16, 32, 48, 64, 80]
        args[k] = None
        assert rejected(L.cn_lattice_eval_fwd(None, 4, *args), fwd), k
    # cn_lattice_eval_bwd(stream, B, logits, choice, g_logp, g_entropy, dlogits)
    bwd = b"cn_lattice_eval_bwd"
    assert rejected(L.cn_lattice_eval_bwd(None, -1, 16, 32, 48, 64, 80), bwd)
    for k in range(5):
        args = [16, 32, 48, 64, 80]
        args[k] = None
        assert rejected(L.cn_lattice_eval_bwd(None, 4, *args), bwd), k
