"""Soft DWA labels without a GPU: the four entry points' declarations, bindings and argument checks (the library loads
on the CPU, as in tests/test_abi.py), the torch restatement ops.lattice_soft_ce_torch and its autograd gradient against
the float64 definition (tests/soft_ref.py, whose tolerances it documents), the hard-label limit, the host restatement
of the regret row, the storages' with_ind, and the refusals of DAgger(soft_tau=) and Policy.evaluate_soft."""
import os
import re

import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd import _lib, ops
from crowdnav_dsrnn_amd.config import Config, UnsupportedConfig, clone_config
from crowdnav_dsrnn_amd.policy_factory import dwa_predict, dwa_regret
from tests import lattice_ref, soft_ref
from tests.helpers import BoxSpace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ---- 1. bindings ------------------------------------------------------------------------------------------------
def test_header_binding_and_export_list_agree_on_the_four_functions():
    from crowdnav_dsrnn_amd import build

    txt = open(os.path.join(REPO, "include", "crowdnav.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)   # (the declarations carry shape comments)
    want = {"cn_robot_act_regret": ["cn_engine*", "void*", "int", "float*", "float*"],
            "cn_robot_mix_regret": ["cn_engine*", "void*", "int", "constfloat*", "constcn_mix_ctl*", "int32_t", "float*",
                                    "float*", "uint8_t*", "float*"],
            "cn_lattice_soft_fwd": ["void*", "int64_t", "constfloat*", "constfloat*", "float", "float*", "float*",
                                    "float*"],
            "cn_lattice_soft_bwd": ["void*", "int64_t", "constfloat*", "constfloat*", "float", "constfloat*", "float*"]}
    build.build()
    L = _lib.lib()
    for fn, types in want.items():
        m = re.search(r"^int %s\((.*?)\);" % fn, txt, re.S | re.M)
        assert m, "include/crowdnav.h does not declare %s" % fn
        params = [p.strip() for p in m.group(1).split(",")]
        assert [re.sub(r"\w+$", "", p).replace(" ", "") for p in params] == types, fn
        assert fn in _lib.EXPORTED
        assert hasattr(L, fn) and len(getattr(L, fn).argtypes) == len(params), fn


def test_entry_points_reject_bad_arguments_without_launching():
    """(No GPU here: a call that got as far as a launch would fail with another code.)"""
    L = _lib.lib()

    def rejected(rc, who):
        return rc == EINVAL and who in L.cn_last_error()

    fwd, bwd = b"cn_lattice_soft_fwd", b"cn_lattice_soft_bwd"
    for B in (0, -3, 4 * 0x7fffffff + 1):
        assert rejected(L.cn_lattice_soft_fwd(None, B, 16, 32, 10.0, 48, 64, 80), fwd), B
        assert rejected(L.cn_lattice_soft_bwd(None, B, 16, 32, 10.0, 48, 64), bwd), B
    for k in range(3):                                        # logits, regret (the NULL regret), ce
        args = [16, 32, 48]
        args[k] = None
        assert rejected(L.cn_lattice_soft_fwd(None, 4, args[0], args[1], 10.0, args[2], None, None), fwd), k
    for k in range(4):                                        # logits, regret, g_ce, dlogits
        args = [16, 32, 48, 64]
        args[k] = None
        assert rejected(L.cn_lattice_soft_bwd(None, 4, args[0], args[1], 10.0, args[2], args[3]), bwd), k
    for bad in (0.0, -0.0, -2.0, float("inf"), float("-inf"), float("nan"), 1e39):   # (1e39: inf as a float32)
        assert rejected(L.cn_lattice_soft_fwd(None, 4, 16, 32, bad, 48, None, None), fwd), bad
        assert b"inv_tau" in L.cn_last_error()
        assert rejected(L.cn_lattice_soft_bwd(None, 4, 16, 32, bad, 48, 64), bwd), bad
    assert L.cn_robot_act_regret(None, None, 2, 16, 32) == EINVAL and b"null engine" in L.cn_last_error()
    assert L.cn_robot_mix_regret(None, None, 2, 16, 32, 0, 48, 64, 80, 96) == EINVAL
    assert b"null engine" in L.cn_last_error()
    for tau in (0.0, -1.0, float("inf"), float("nan"), 1e-39):   # the wrapper's rule, before any tensor is touched
        with pytest.raises(ValueError, match="tau"):
            ops.lattice_soft_ce(torch.zeros((2, 64)), torch.zeros((2, 64)), tau)
    with pytest.raises(ValueError):
        ops.lattice_soft_ce(torch.zeros((2, 64)), torch.zeros((2, 63)), 0.1)
    with pytest.raises(ValueError):
        ops.lattice_soft_ce(torch.zeros((2, 64)), torch.zeros((2, 64), dtype=torch.float64), 0.1)


# ---- 2. the restatement against the float64 definition -----------------------------------------------------------
@pytest.fixture(scope="module", params=soft_ref.BATCHES, ids=lambda p: "B%d" % p[0])
def batch(request):
    B, start = request.param
    return lattice_ref.rows(B, start), soft_ref.regrets(B, start), soft_ref.kinds(B, start), start


def _restatement(logits, regret, tau, g):
    lt = torch.from_numpy(logits).requires_grad_(True)
    ce, kl, best = ops.lattice_soft_ce(lt, torch.from_numpy(regret), tau)   # (CPU tensors: the restatement)
    assert ce.shape == kl.shape == best.shape == (len(logits),)
    assert ce.requires_grad and not kl.requires_grad and not best.requires_grad
    (ce * torch.from_numpy(g)).sum().backward()
    return ce.detach().numpy(), kl.numpy(), best.numpy(), lt.grad.numpy()


def check_against_definition(logits, regret, tau, g, ce, kl, best, dl, who=""):
    """Every figure of one evaluation against tests/soft_ref.py's definition and tolerances (the GPU tests' too)."""
    s = soft_ref.soft(logits, regret, tau)
    want, tol = soft_ref.grad(s, g)
    for name, got, ref, t in (("ce", ce, s["ce"], s["tol_ce"]), ("kl", kl, s["kl"], s["tol_kl"]),
                              ("logp_best", best, s["logp_best"], s["tol_best"]), ("dlogits", dl, want, tol)):
        err = np.abs(got.astype(np.float64) - ref)
        print("%s tau %g %s: max error %.3g, max error / tolerance %.3g" % (who, tau, name, err.max(), (err / t).max()))
        assert np.isfinite(got).all(), name
        assert (err <= t).all(), (name, tau, np.argwhere(err > t)[:4].tolist())
    return s


@pytest.mark.parametrize("tau", soft_ref.TAUS)
def test_restatement_vs_float64(batch, tau):
    logits, regret, _, _ = batch
    g = soft_ref.upstream(len(logits))
    s = check_against_definition(logits, regret, tau, g, *_restatement(logits, regret, tau, g), who="restatement")
    print("tol_ce %.3g .. %.3g, tol_kl %.3g .. %.3g" % (s["tol_ce"].min(), s["tol_ce"].max(), s["tol_kl"].min(),
                                                        s["tol_kl"].max()))
    assert (s["tol_ce"] < 1e-2).all() and (s["tol_kl"] < 1e-2).all()      # the bounds stay bounds


def test_the_rows_hold_what_they_were_built_for():
    B, start = soft_ref.BATCHES[-1]
    r, k = soft_ref.regrets(B, start), soft_ref.kinds(B, start)
    assert set((k * 8 + (start + np.arange(B)) % lattice_ref.KINDS).tolist()) == set(range(56))   # every pairing
    assert (r[k == 0] == 0).all() and ((r[k == 1] == 0).sum(1) == 1).all()
    assert ((r[k == 2] == 0).sum(1) == 2).all() and ((r[k == 3] == 0).sum(1) == 4).all()
    real = r[(k == 4) | (k == 6)]
    assert (real.min(1) == 0).all() and real.max() > 500 and (r[k == 5].min(1) == 37.5).all()
    # the issue's counts on the controller's own rows: near-ties are the rule, and part of every target underflows
    rows = soft_ref.dwa_rows()
    assert 1.2 < (rows <= 0.01).sum(1).mean() < 2.0 and 4.0 < (rows <= 0.1).sum(1).mean() < 8.0
    q32 = np.exp(-(rows * soft_ref.inv_tau32(0.1))).astype(np.float32)
    assert 0.02 < (q32 == 0).mean() < 0.5
    assert soft_ref.BATCHES[0] == (1, 4) and soft_ref.kinds(1, 4)[0] == 4   # the lone row is a real one


# ---- 3. the hard limit and the uniform target --------------------------------------------------------------------
@pytest.mark.parametrize("tau", soft_ref.TAUS)
def test_one_zero_rows_are_the_hard_label(tau):
    """regret 0 at lane 9 and 1e4 elsewhere: the target is one-hot in float32 at every tau served here, so ce is the
    label's negative log-likelihood and the gradient is lattice_evaluate's with no entropy term."""
    B, start = soft_ref.BATCHES[-1]
    hard = soft_ref.kinds(B, start) == 1
    logits, regret = lattice_ref.rows(B, start)[hard], soft_ref.regrets(B, start)[hard]
    n = len(logits)
    assert n >= 32
    g = soft_ref.upstream(n)
    ce, kl, best, dl = _restatement(logits, regret, tau, g)
    s = soft_ref.soft(logits, regret, tau)
    assert (s["q"][:, 9] == 1).all() and (s["best"] == 9).all()
    lp = lattice_ref.softmax(logits)["logp"][:, 9]
    assert (np.abs(ce + lp) <= s["tol_ce"]).all() and (np.abs(best - lp) <= s["tol_best"]).all()
    assert (np.abs(kl - ce) <= s["tol_kl"]).all()                                         # H(q) = 0
    lt = torch.from_numpy(logits).requires_grad_(True)
    actions = torch.from_numpy(lattice_ref.ACTIONS32[np.full(n, 9)])
    logp, ent = ops.lattice_evaluate(lt, actions)
    (-(logp[:, 0]) * torch.from_numpy(g)).sum().add((ent * 0.0).sum()).backward()          # g_H = 0
    _, tol = soft_ref.grad(s, g)
    assert (np.abs(dl - lt.grad.numpy()) <= tol + lattice_ref.logp_tol(lt.grad.numpy())).all()


@pytest.mark.parametrize("tau", soft_ref.TAUS)
def test_all_zero_rows_are_the_uniform_target(tau):
    B, start = soft_ref.BATCHES[-1]
    k = soft_ref.kinds(B, start)
    uniform = k == 0
    logits, regret = lattice_ref.rows(B, start)[uniform], soft_ref.regrets(B, start)[uniform]
    lk = ((start + np.arange(B)) % lattice_ref.KINDS)[uniform]
    ce, kl, best, _ = _restatement(logits, regret, tau, soft_ref.upstream(len(logits)))
    s = soft_ref.soft(logits, regret, tau)
    assert (s["q"] == 1.0 / 64).all() and (s["best"] == 0).all()
    assert (np.abs(s["Hq"] - np.log(64.0)) < 1e-12).all()
    assert (kl >= -s["tol_kl"]).all() and (kl[s["kl"] > s["tol_kl"]] > 0).all()            # KL >= 0
    assert (lk == 0).any() and (np.abs(kl[lk == 0]) <= s["tol_kl"][lk == 0]).all()         # all-equal logits: KL = 0
    assert (s["kl"][lk != 0] > 1e-3).all()


# ---- 4. the host restatement of the regret row -------------------------------------------------------------------
def test_dwa_regret_is_zero_at_the_choice_and_nowhere_negative():
    from tests.test_dwa import _random_states, _self

    s, v, o = _random_states(np.random.RandomState(1), 24, 5)
    _, choice, costs = dwa_predict(s, v, o, 0.25)
    r = dwa_regret(costs, choice)
    assert r.dtype == np.float32 and r.shape == (24, 64)
    assert (r[np.arange(24), choice] == 0).all() and not np.signbit(r[np.arange(24), choice]).any()
    assert (r >= 0).all() and np.isfinite(r).all()
    assert r.tobytes() == (costs - costs[np.arange(24), choice][:, None]).astype(np.float32).tobytes()
    # subtracting before rounding keeps a near-tie apart where J itself is large
    J = np.full((1, 64), 1000.0 + 1e-5)
    J[0, 7] = 1000.0
    assert dwa_regret(J, [7])[0, 8] > 0 and np.float32(J[0, 8]) == np.float32(J[0, 7])
    # w_goal = 0 with no human within d_safe of any arc: all 64 costs are exactly 0, the row is all +0.0
    s2 = np.concatenate([_self(theta=0.0, gx=4.0), _self(theta=0.0, gx=4.0)])
    far = np.array([[[0.0, 5.0, 0.0, 0.0, 0.3], [3.0, -6.0, 0.0, 0.0, 0.3]],
                    [[0.0, -5.0, 0.0, 0.0, 0.3], [3.0, 6.0, 0.0, 0.0, 0.3]]])
    for hum in (np.zeros((2, 0, 5)), far):
        _, ch, co = dwa_predict(s2, np.array([0.3, 0.3]), hum, 0.25, {"w_goal": 0.0})
        assert (ch == 0).all()
        assert dwa_regret(co, ch).tobytes() == np.zeros((2, 64), np.float32).tobytes()
    with pytest.raises(ValueError):
        dwa_regret(costs, choice[:-1])


# ---- 5. the storages' with_ind -----------------------------------------------------------------------------------
def _storages():
    from crowdnav_dsrnn_amd.learner import RolloutStorage, SRNNRolloutStorage

    T, E = 4, 6
    g = torch.Generator().manual_seed(3)
    obs = {"robot_node": BoxSpace((1, 7)), "temporal_edges": BoxSpace((1, 2)), "spatial_edges": BoxSpace((3, 2))}
    a = SRNNRolloutStorage(T, E, obs, BoxSpace((2,)), 8, 8, device="cpu")
    b = RolloutStorage(T, E, (1, 10), BoxSpace((2,)), 8)
    for st in (a, b):
        for x in ([st.actions, st.returns, st.masks, st.value_preds, st.action_log_probs]
                  + (list(st.obs.values()) if isinstance(st.obs, dict) else [st.obs])):
            x.copy_(torch.randn(x.shape, generator=g))
    return a, b


def _same(x, y):
    if isinstance(x, dict):
        return set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x)
    return torch.equal(x, y)


def test_with_ind_appends_the_env_indices_and_changes_nothing_else():
    for st in _storages():
        T, E = st.num_steps, st.rewards.size(1)
        adv = st.returns[:-1]
        for nmb in (1, 2, 3):
            torch.manual_seed(17)
            plain = list(st.recurrent_generator(adv, nmb))
            torch.manual_seed(17)
            plus = list(st.recurrent_generator(adv, nmb, with_ind=True))
            assert len(plain) == len(plus) == nmb
            seen = []
            for p, q in zip(plain, plus):
                assert len(p) == 8 and len(q) == 9                   # the default: every caller's tuple as it was
                assert all(_same(x, y) for x, y in zip(p, q[:8]))
                ind = q[8]
                assert ind.dtype == torch.int64 and ind.shape == (E // nmb,)
                assert torch.equal(st.actions.index_select(1, ind).reshape(T * len(ind), -1), q[2])
                side = torch.arange(T * E * 64, dtype=torch.float32).reshape(T, E, 64)   # a record beside the storage
                rows = side.index_select(1, ind).reshape(-1, 64)
                assert torch.equal(rows[:, 0].reshape(T, -1), side[:, ind, 0])           # (step, env) order
                seen += ind.tolist()
            assert sorted(seen) == list(range(E))


# ---- 6. refusals -------------------------------------------------------------------------------------------------
class _Stub:
    """What DAgger reads before it touches the engine (no GPU behind it)."""

    num_envs = 8
    obs_mode = "srnn"

    def __init__(self, config):
        self.config = config

    def __getattr__(self, name):
        raise AssertionError("the check must come before the engine is touched (%s)" % name)


class _Pol:
    srnn, convgru = True, False

    def __init__(self, head):
        self.head = head


def _config(kin="unicycle", dwa=True, head=None, N=5):
    c = clone_config(Config())
    c.sim.human_num = N
    c.action_space.kinematics = kin
    c.robot.scripted_dwa = dwa
    c.robot.scripted_unicycle = kin == "unicycle"
    if head is not None:
        c.robot.action_head = head
    return c


def test_dagger_soft_tau_refusals_come_before_the_engine():
    from crowdnav_dsrnn_amd import learner

    uni = _config()
    with pytest.raises(UnsupportedConfig, match="lattice"):                 # a Gaussian head
        learner.DAgger(uni, _Stub(uni), _Pol("gaussian"), expert="dwa", soft_tau=0.1)
    for expert in ("orca", "social_force"):                                  # no candidate set
        with pytest.raises(UnsupportedConfig, match="dwa"):
            learner.DAgger(uni, _Stub(uni), _Pol("lattice"), expert=expert, soft_tau=0.1)
    for tau in (0.0, -0.5, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="soft_tau"):
            learner.DAgger(uni, _Stub(uni), _Pol("lattice"), expert="dwa", soft_tau=tau)
    # a good soft_tau passes these checks and goes on to the engine (the stub's own error), as soft_tau=None does
    for tau in (0.1, None):
        with pytest.raises(AssertionError, match="engine is touched"):
            learner.DAgger(uni, _Stub(uni), _Pol("lattice"), expert="dwa", soft_tau=tau)


def test_evaluate_soft_is_the_lattice_heads():
    from crowdnav_dsrnn_amd.policy import Policy
    from crowdnav_dsrnn_amd.spaces import action_space, observation_space

    c = _config(head="gaussian")
    pol = Policy(observation_space(5).spaces, action_space(), base="srnn", base_kwargs=c)
    assert pol.head == "gaussian"
    with pytest.raises(UnsupportedConfig, match="lattice"):
        pol.evaluate_soft(None, None, None, torch.zeros((4, 64)), 0.1)       # (before the inputs are read)
