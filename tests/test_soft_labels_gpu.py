"""Soft DWA labels on the GPU: the controller's regret rows (cn_robot_act_regret / cn_robot_mix_regret) against
cn_dwa_predict's costs on the same state, bit for bit; the loss kernels (cn_lattice_soft_fwd / _bwd) against the
float64 definition and tolerances of tests/soft_ref.py; Policy.evaluate_soft; and DAgger(soft_tau=) on a plain engine
(ring of regret rows, graph against eager, the fit) and on an env of varying human count."""
import numpy as np
import pytest
import torch

from crowdnav_dsrnn_amd import _lib, ops
from crowdnav_dsrnn_amd.config import Config, clone_config, make_varied_cn_configs
from tests import lattice_ref, soft_ref
from tests.test_dwa import _config as _dwa_config
from tests.test_dwa import _engine, _state_arrays
from tests.test_soft_labels import check_against_definition

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -2


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _want_rows(eng, sv):
    """(float32)(J_c - J_choice) of cn_dwa_predict on one state view: what the regret kernels must write, as numpy."""
    s, v, o = _state_arrays(sv)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)   # noqa: E731
    _, ch, co = eng.dwa_predict(t(s), t(v), t(o), 0.25, None)
    torch.cuda.synchronize()
    ch, co = ch.cpu().numpy(), co.cpu().numpy()
    return (co - co[np.arange(len(co)), ch][:, None]).astype(np.float32), ch


def _guarded(E):
    """(E + 1, 64) NaN and (E + 1, 2) sevens: the calls get the first E rows, row E is the guard."""
    return torch.full((E + 1, 64), float("nan"), device=DEV), torch.full((E + 1, 2), 7.0, device=DEV)


# ---- 1. regret rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 11])
@pytest.mark.parametrize("E", [8, 67])
def test_regret_rows_equal_predicts_costs_on_the_same_state(E, N):
    """E = 8: whole workgroups; 67: 16 workgroups and 3 waves. After a reset and after 3 of the controller's steps."""
    eng = _engine(_dwa_config(N, time_limit=None), E, nenv=131)
    eng.reset()
    spread = 0
    for where in ("reset", "after 3 steps"):
        want, ch = _want_rows(eng, eng.get_state())
        plain = eng.robot_act("dwa").clone()
        R, A = _guarded(E)
        got = eng.robot_act("dwa", out=A[:E], regret=R[:E])
        torch.cuda.synchronize()
        assert got.data_ptr() == A.data_ptr()
        assert _bits(A[:E]) == _bits(plain), (E, N, where)                       # the action, bit for bit
        r = R.cpu().numpy()
        assert not np.isnan(r[:E]).any(), (E, N, where)                          # every entry written
        assert np.isnan(r[E]).all() and (A[E] == 7.0).all()                      # and nothing past row E - 1
        assert r[:E].tobytes() == want.tobytes(), (E, N, where)
        assert (r[:E] >= 0).all() and not np.signbit(r[np.arange(E), ch]).any() and (r[np.arange(E), ch] == 0).all()
        spread += int((r[:E] > 0).sum())
        if where == "reset":
            for _ in range(3):
                eng.step(eng.robot_act("dwa"))
    assert spread > 32 * E
    eng.close()


# ---- 2. a mixed engine -------------------------------------------------------------------------------------------
def test_mixed_engine_rows_land_at_their_envs():
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    NUMS, E = [3, 5], 10
    c = _dwa_config(5, time_limit=None)
    c.sim.human_nums, c.sim.human_nums_scripted = list(NUMS), True
    cfgs, eg = make_varied_cn_configs(c, NUMS, E, phase="train", seed=7, rng="mt19937")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=True, scripted_dwa=True)
    mixed.reset()
    for where in range(2):
        plain = mixed.robot_act("dwa").clone()
        R, A = _guarded(E)
        mixed.robot_act("dwa", out=A[:E], regret=R[:E])
        torch.cuda.synchronize()
        r = R.cpu().numpy()
        assert _bits(A[:E]) == _bits(plain) and np.isnan(r[E]).all()
        seen = np.zeros(E, bool)
        for rows, sv in mixed.get_state():
            want, _ = _want_rows(mixed, sv)
            assert sv.b_px.shape[1] == NUMS[int(rows[0]) % 2]
            assert r[rows].tobytes() == want.tobytes(), (where, rows)
            seen[rows] = True
        assert seen.all()
        for _ in range(3):
            mixed.step(mixed.robot_act("dwa"))
    mixed.close()


# ---- 3. robot_mix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_robot_mix_with_regret_is_robot_mix_plus_the_rows(beta):
    E = 67
    eng = _engine(_dwa_config(5, time_limit=None), E, nenv=131)
    eng.reset()
    for _ in range(3):
        eng.step(eng.robot_act("dwa"))
    want, _ = _want_rows(eng, eng.get_state())
    ctl = eng.set_mix_ctl(eng.mix_ctl(), beta, seed=9, step0=40)
    learner = torch.from_numpy(lattice_ref.ACTIONS32[np.random.RandomState(2).randint(0, 64, E)]).to(DEV)
    a = eng.robot_mix("dwa", learner, ctl, 3)
    R, _ = _guarded(E)
    b = eng.robot_mix("dwa", learner, ctl, 3, regret=R[:E])
    torch.cuda.synchronize()
    for x, y, name in zip(a, b, ("label", "executed", "flags")):
        assert _bits(x) == _bits(y), (name, beta)
    took = (b[2] & 1).float().mean().item()
    assert took == beta if beta in (0.0, 1.0) else 0.2 < took < 0.8
    r = R.cpu().numpy()
    assert r[:E].tobytes() == want.tobytes() and np.isnan(r[E]).all()
    eng.close()


# ---- 4. error codes ----------------------------------------------------------------------------------------------
def test_error_codes_come_before_any_launch():
    from crowdnav_dsrnn_amd.engine import CrowdNavEngine

    L = _lib.lib()
    E = 8
    R, A = _guarded(E)
    lab, exe, fl = torch.full((E, 2), 5.0, device=DEV), torch.full((E, 2), 6.0, device=DEV), torch.full(
        (E,), 9, dtype=torch.uint8, device=DEV)
    learner = torch.zeros((E, 2), device=DEV)

    def act(eng, policy, regret=True, actions=True):
        return L.cn_robot_act_regret(eng._h, None, policy, A.data_ptr() if actions else None,
                                     R.data_ptr() if regret else None)

    def mix(eng, policy, ctl, regret=True, t=0):
        return L.cn_robot_mix_regret(eng._h, None, policy, learner.data_ptr(), ctl.data_ptr(), t, lab.data_ptr(),
                                     exe.data_ptr(), fl.data_ptr(), R.data_ptr() if regret else None)

    def untouched():
        torch.cuda.synchronize()
        return (bool(R.isnan().all()) and bool((A == 7.0).all()) and bool((lab == 5.0).all())
                and bool((exe == 6.0).all()) and bool((fl == 9).all()))

    eng = _engine(_dwa_config(5), E)
    eng.reset()
    ctl = eng.set_mix_ctl(eng.mix_ctl(), 0.5)
    for policy in (0, 1):                                                   # ORCA, social force: no candidate set
        assert act(eng, policy) == EUNSUPPORTED and b"candidate" in L.cn_last_error()
        assert mix(eng, policy, ctl) == EUNSUPPORTED
    assert act(eng, 3) == EINVAL and mix(eng, 3, ctl) == EINVAL             # unknown
    assert act(eng, 2, regret=False) == EINVAL and b"regret" in L.cn_last_error()
    assert act(eng, 2, actions=False) == EINVAL
    assert mix(eng, 2, ctl, regret=False) == EINVAL and b"regret" in L.cn_last_error()
    assert mix(eng, 2, ctl, t=-1) == EINVAL
    for policy in ("orca", "social_force"):
        with pytest.raises(RuntimeError):
            eng.robot_act(policy, regret=R[:E])
    with pytest.raises(ValueError):
        eng.robot_act("dwa", regret=R)                                      # (E + 1, 64)
    with pytest.raises(ValueError):
        eng.robot_mix("dwa", learner, ctl, 0, regret=R[:E].double())
    assert untouched()
    eng.close()
    off = _engine(_dwa_config(5), E, dwa=None)                              # 'dwa' without cn_scripted_dwa
    off.reset()
    assert act(off, 2) == EINVAL and mix(off, 2, ctl) == EINVAL
    with pytest.raises(RuntimeError):
        off.robot_act("dwa", regret=R[:E])
    assert untouched()
    off.close()
    c = _dwa_config(5)
    c.sim.human_nums, c.sim.human_nums_scripted = [3, 5], True
    cfgs, eg = make_varied_cn_configs(c, [3, 5], E, phase="train", seed=7, rng="mt19937")
    mixed = CrowdNavEngine.mixed(cfgs, eg, DEV, scripted=False, scripted_dwa=True)   # cn_robot_act's own refusal
    assert act(mixed, 2) == EUNSUPPORTED and b"mixed" in L.cn_last_error()
    assert untouched()
    mixed.close()


# ---- 5. the loss kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", soft_ref.TAUS)
@pytest.mark.parametrize("B,start", soft_ref.BATCHES)
def test_loss_kernels_vs_float64(B, start, tau):
    logits, regret = lattice_ref.rows(B, start), soft_ref.regrets(B, start)
    g = soft_ref.upstream(B)
    lt = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    rt = torch.from_numpy(regret).to(DEV)
    ce, kl, best = ops.lattice_soft_ce(lt, rt, tau)
    assert ce.shape == kl.shape == best.shape == (B,) and ce.requires_grad and not kl.requires_grad
    (ce * torch.from_numpy(g).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    dl = lt.grad.cpu().numpy()
    s = check_against_definition(logits, regret, tau, g, ce.detach().cpu().numpy(), kl.cpu().numpy(),
                                 best.cpu().numpy(), dl, who="kernels B %d" % B)
    # exactly 0 where both q_j and p_j / Z are 0 in float32, whatever the device's denormal handling
    dead = (s["x"] < -110.0) & (lattice_ref.softmax(logits)["d"] < -110.0)
    assert (dl[dead] == 0).all() and (B < 56 or dead.sum() > 0)
    # kl = NULL / logp_best = NULL: the same ce bytes
    inv = float(soft_ref.inv_tau32(tau))
    for kl_p, best_p in ((None, None), (kl.data_ptr(), None), (None, best.data_ptr())):
        ce2 = torch.full((B,), float("nan"), device=DEV)
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().cn_lattice_soft_fwd(ops._stream(torch.device(DEV)), B, lt.data_ptr(), rt.data_ptr(),
                                                      inv, ce2.data_ptr(), kl_p, best_p))
        torch.cuda.synchronize()
        assert _bits(ce2) == _bits(ce)


# ---- 6. / 7. / 8. the policy and the trainer ---------------------------------------------------------------------
E, N, T, TAU = 8, 5, 4, 0.1


def _config(n_env=E):
    c = clone_config(Config())
    c.sim.human_num = N
    c.humans.policy = "orca"
    c.action_space.kinematics = "unicycle"
    c.robot.scripted_dwa = True
    c.robot.action_head = "lattice"
    c.sim.train_val_sim = c.sim.test_sim = ["circle_crossing"]
    c.env.time_limit = 1.5
    c.env.time_step = 0.25
    c.training.num_processes = n_env
    c.ppo.num_steps, c.ppo.num_mini_batch, c.ppo.epoch = T, 1, 1
    return c


def _trainer(c=None, seed=3, **kw):
    from crowdnav_dsrnn_amd.envs import CrowdNavVecEnv
    from crowdnav_dsrnn_amd.learner import DAgger
    from crowdnav_dsrnn_amd.policy import Policy

    c = _config() if c is None else c
    envs = CrowdNavVecEnv(c, E, c.env.seed, DEV, allow_early_resets=True, nenv=E, phase="train")
    torch.manual_seed(seed)
    pol = Policy(envs.observation_space.spaces, envs.action_space, base="srnn", base_kwargs=envs.config).to(DEV)
    assert pol.head == "lattice"
    with torch.no_grad():
        pol.dist.fc_logits.weight.mul_(100.0)   # logits away from uniform, so that a wrong row or target shows
    pol.train()
    kw.setdefault("soft_tau", TAU)
    return c, envs, pol, DAgger(c, envs, pol, expert="dwa", seed=11, lr=1e-3, **kw)


def _check_engine_rows(dg):
    """Every recorded row is a regret row of the recorded label: 0 at the label's candidate, nowhere negative."""
    r = dg.regret.reshape(-1, 64)
    idx = ops.lattice_index(dg.labels.reshape(-1, 2))
    assert bool((r.gather(1, idx.unsqueeze(1)) == 0).all()) and bool((r >= 0).all()) and bool(r.isfinite().all())
    assert bool((r > 0).any(1).all())
    first_zero = torch.where(r == 0, torch.arange(64, device=DEV), 64).amin(1)
    assert torch.equal(first_zero, idx)                                     # ties go to the lowest candidate


def test_policy_evaluate_soft_equals_the_restatement_on_the_same_weights():
    c, envs, pol, dg = _trainer(beta=0.5, num_mini_batch=1)
    dg.collect()
    _check_engine_rows(dg)
    r = dg.rollouts
    seen = []

    def keep(module, inputs, out):   # the head's logits, with their gradient
        out.retain_grad()
        seen.append(out)

    hook = pol.dist.fc_logits.register_forward_hook(keep)
    with dg._sequence_shape(E):
        obs_b, hxs_b, _, _, _, masks_b, _, _, ind = next(iter(r.recurrent_generator(r.returns[:-1], 1, with_ind=True)))
        regret_b = dg.regret.index_select(1, ind).reshape(-1, 64)
        value, ce, kl, best, _ = pol.evaluate_soft(obs_b, hxs_b, masks_b, regret_b, TAU)
        ce.mean().backward()
    hook.remove()
    B = T * E
    assert tuple(value.shape) == tuple(ce.shape) == tuple(kl.shape) == tuple(best.shape) == (B, 1)
    assert ce.requires_grad and not kl.requires_grad and not best.requires_grad
    logits = seen[0].detach()
    assert float(logits.max() - logits.min()) > 1.0
    ce_t, kl_t, best_t = ops.lattice_soft_ce_torch(logits, regret_b, TAU)
    torch.cuda.synchronize()
    l, rg, g = logits.cpu().numpy(), regret_b.cpu().numpy(), np.full(B, 1.0 / B, np.float32)
    s = check_against_definition(l, rg, TAU, g, ce[:, 0].detach().cpu().numpy(), kl[:, 0].cpu().numpy(),
                                 best[:, 0].cpu().numpy(), seen[0].grad.cpu().numpy(), who="evaluate_soft")
    for name, a, b, tol in (("ce", ce[:, 0], ce_t, s["tol_ce"]), ("kl", kl[:, 0], kl_t, s["tol_kl"]),
                            ("logp_best", best[:, 0], best_t, s["tol_best"])):
        d = (a.detach() - b).abs().cpu().numpy()
        assert (d <= 2 * tol).all(), (name, d.max())                         # two float32 evaluations of one definition
    # the hard label's log-probability, from the same pass: the stored labels' candidates under the same logits
    labels_b = r.actions.index_select(1, ind).reshape(-1, 2)
    idx = ops.lattice_index(labels_b).cpu().numpy()
    assert np.array_equal(idx, s["best"])
    assert (np.abs(best[:, 0].cpu().numpy() - s["logp"][np.arange(B), idx]) <= s["tol_best"]).all()
    envs.close()


def test_dagger_soft_keeps_each_chunks_regret_rows_and_reports_the_new_keys():
    c, envs, pol, dg = _trainer(beta=1.0, beta_decay=0.5, aggregate=2, num_mini_batch=2)
    kept = []
    for i in range(3):
        st = dg.update()
        torch.cuda.synchronize()
        _check_engine_rows(dg)
        kept.append(_bits(dg.regret))
        held = dg.held_regret()
        assert len(held) == len(dg.held()) == min(i + 1, 2)
        assert [_bits(x) for x in held] == kept[-len(held):], i
        for k in ("soft_ce", "kl", "nll", "value_loss"):
            assert np.isfinite(st[k]), (k, st)
        assert st["soft_tau"] == TAU and st["kl"] >= 0 and st["soft_ce"] >= st["kl"]
        assert {"beta", "took_expert", "agree", "episodes", "rollout_s", "update_s"} <= set(st)
    assert len(set(kept)) == 3
    acc, n = dg.fit()
    assert n == 2 * 2 and tuple(acc.shape) == (4,)
    envs.close()


def test_dagger_soft_graph_equals_eager():
    """tests/test_dagger.py's comparison with soft_tau set: eager warm-up, capture, two replays against four eager
    chunks; the captured chunk replays into the fixed regret buffer."""

    def run(graphs):
        torch.manual_seed(5)
        c, envs, pol, dg = _trainer(beta=1.0, beta_decay=0.5, graphs=graphs, aggregate=2)
        rows = []
        for i in range(4):
            st = dg.update()
            torch.cuda.synchronize()
            row = {"regret": _bits(dg.regret), "labels": _bits(dg.labels), "executed": _bits(dg.executed),
                   "flags": _bits(dg.flags), "actions": _bits(dg.rollouts.actions)}
            row.update({"w:" + k: _bits(v) for k, v in pol.state_dict().items()})
            row["stats"] = (st["nll"], st["soft_ce"], st["kl"], st["value_loss"], st["agree"])
            rows.append(row)
        audit, on = dg.graph_audit, dg.graphs
        envs.close()
        return rows, audit, on

    eager, audit_e, on_e = run(False)
    graph, audit, on = run(True)
    assert audit_e is None and not on_e
    assert on and audit is not None and audit.get("memset", 0) == 0 and audit["kernel"] > 0, audit
    for i, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert a[k] == b[k], (i, k)
    assert len({r["regret"] for r in eager}) == 4


def test_dagger_soft_fitting_lowers_the_soft_ce_of_a_fixed_chunk():
    c, envs, pol, dg = _trainer(beta=0.5, num_mini_batch=1, value_coef=0.0)
    dg.collect()
    first = float(dg.chunk_soft_ce())
    acc, n = dg.fit(10)
    last = float(dg.chunk_soft_ce())
    print("soft_ce before %.6f, after 10 passes %.6f" % (first, last))
    assert n == 10 and np.isfinite(first) and np.isfinite(last) and last < first, (first, last)
    envs.close()


def test_dagger_soft_on_a_varied_count_env():
    c = _config()
    c.sim.human_nums, c.sim.human_nums_scripted = [3, 5], True
    c, envs, pol, dg = _trainer(c, beta=0.5, num_mini_batch=2)
    assert sorted(set(envs.env_human_nums)) == [3, 5] and not dg.graphs
    st = dg.update()
    torch.cuda.synchronize()
    _check_engine_rows(dg)
    assert all(np.isfinite(st[k]) for k in ("nll", "soft_ce", "kl", "value_loss")) and st["soft_tau"] == TAU
    assert tuple(dg.regret.shape) == (T, E, 64)
    envs.close()
