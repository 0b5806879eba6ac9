"""Shared test helpers: build engine configs from fixture metadata, move fixture states into blobs,
compare states with the tolerances the north star fixes (bit-exact on indices/flags/events;
1e-5 on positions and rewards). compare_info / compare_monitor hold the one definition of how a step's info
row and Monitor outputs are compared, for the recorded fixtures and for every GPU-vs-oracle test."""
import os
import zlib

import numpy as np

from crowdnav_dsrnn_amd import abi
from crowdnav_dsrnn_amd.config import Config, clone_config, make_cn_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# f64 state fields compared with an absolute tolerance (positions, velocities, rewards ...)
FLOAT_FIELDS = {n for n, t, _ in abi.STATE_FIELDS if t in (0, 1)}
EXACT_FIELDS = {"case_counter", "ep_len", "scenario", "reset_count", "flags", "mt_pos", "o_dmask", "o_perm"}
POS_TOL = 1e-5


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def ref_config(meta):
    c = clone_config(Config())
    c.action_space.kinematics = str(meta["meta_kinematics"])
    c.humans.policy = str(meta["meta_policy"])
    sc = str(meta["meta_scenarios"]).split(",")
    c.sim.train_val_sim = sc
    c.sim.test_sim = sc
    c.sim.human_num = int(meta["meta_N"])
    c.robot.FOV = float(meta["meta_robot_fov"])
    c.humans.FOV = float(meta["meta_human_fov"])
    c.test.side_preference = bool(meta["meta_side_pref"])
    c.test.social_metrics = bool(meta["meta_social_metrics"])
    c.robot.visible = bool(meta["meta_robot_visible"])
    c.humans.random_radii = bool(meta["meta_random_radii"])
    c.humans.random_v_pref = bool(meta["meta_random_v_pref"])
    c.reward.time_factor = bool(meta["meta_time_factor"])
    c.env.time_step = float(meta["meta_time_step"])
    c.reward.discomfort_penalty_factor = 10 * c.env.time_step
    c.sim.circle_radius = float(meta["meta_circle_radius"])
    if c.test.side_preference:
        c.humans.random_goal_changing = False
        c.humans.end_goal_changing = False
    c.reward.norm_zones = bool(meta["meta_norm_zones"])
    over = meta_overrides(meta)
    for k, v in over.items():
        sec, fld = k.split("__")
        assert hasattr(getattr(c, sec), fld), k
        setattr(getattr(c, sec), fld, v)   # numbers as float: make_cn_config converts every field itself
    if "reward__discomfort_penalty_factor" not in over:
        c.reward.discomfort_penalty_factor = 10 * c.env.time_step
    for k in ("seed", "val_size", "test_size"):
        if "meta_" + k in meta:
            setattr(c.env, k, int(meta["meta_" + k]))
    return c


def meta_overrides(meta):
    """{"section__field": value} a fixture was recorded with (oracle/gen_golden.py:make_ref_config's `over`):
    numbers from meta_over_keys / meta_over_vals, strings from meta_over_skeys / meta_over_svals. Fixtures
    recorded at the default settings have none of these keys."""
    over = {}
    if "meta_over_keys" in meta:
        over.update((str(k), float(v)) for k, v in zip(meta["meta_over_keys"], meta["meta_over_vals"]))
    if "meta_over_skeys" in meta:
        over.update((str(k), str(v)) for k, v in zip(meta["meta_over_skeys"], meta["meta_over_svals"]))
    return over


def cn_config_from_meta(meta, E=None):
    c = ref_config(meta)
    E = int(meta["meta_E"]) if E is None else E
    phase = str(meta["meta_phase"]) if "meta_phase" in meta else None
    return make_cn_config(c, num_envs=E, nenv=int(meta["meta_E"]), phase=phase)


def state_from(d, prefix, cfg, mt=None):
    sv = abi.StateView(None, cfg.num_envs, cfg.human_num, cfg.robot_visible)
    for name, _, _ in abi.STATE_FIELDS:
        key = prefix + name
        if key in d:
            getattr(sv, name)[...] = d[key].reshape(getattr(sv, name).shape)
    if mt is not None:
        sv.mt[...] = mt
    return sv


def mt_crc(sv):
    return np.array([zlib.crc32(np.ascontiguousarray(sv.mt[e]).tobytes()) for e in range(sv.E)], np.uint32)


def compare_state(got, d, prefix, tol=POS_TOL, skip=(), env_mask=None, where=""):
    """Compare a StateView with fixture fields `prefix+name`; returns list of mismatch strings."""
    errs = []
    for name, _, _ in abi.STATE_FIELDS:
        if name in skip or name == "mt" or (prefix + name) not in d:
            continue
        a = np.asarray(getattr(got, name))
        b = d[prefix + name].reshape(a.shape)
        if env_mask is not None:
            a, b = a[env_mask], b[env_mask]
        if name in EXACT_FIELDS:
            bad = a != b
        else:
            af, bf = a.astype(np.float64), b.astype(np.float64)
            bad = ~((np.abs(af - bf) <= tol) | (np.isnan(af) & np.isnan(bf)) | (af == bf))
        if bad.any():
            idx = np.argwhere(bad)[:3]
            errs.append("%s%s: %d mismatches, e.g. %s got=%s want=%s" % (
                where, name, int(bad.sum()), idx.tolist(), a[tuple(idx[0])], b[tuple(idx[0])]))
    if (prefix + "mt_crc") in d:
        c = mt_crc(got)
        want = d[prefix + "mt_crc"]
        if env_mask is not None:
            c, want = c[env_mask], want[env_mask]
        if (c != want).any():
            errs.append("%smt stream: %d envs differ" % (where, int((c != want).sum())))
    return errs


def at(d, prefix, t):
    """Slice step t out of stacked fixture fields `prefix*` -> {prefix+name: value}."""
    return {k: v[t] for k, v in d.items() if k.startswith(prefix)}


# info columns (include/crowdnav.h CN_INFO_*): counts, flags and ids are exact; the three float32 metrics get
# the bar the fixture comparison has always used; MIN_DIST is a distance (POS_TOL)
INFO_EXACT = (abi.INFO_AGG_NAV_TIME, abi.INFO_PATH_VIOLATION, abi.INFO_PERSONAL_VIOLATION, abi.INFO_SPEED_VIOLATION,
              abi.INFO_SCENARIO, abi.INFO_SIDE_LEFT, abi.INFO_SIDE_RIGHT, abi.INFO_OVERFLOW)
INFO_CLOSE = (abi.INFO_DIST_TO_GOAL, abi.INFO_SEPARATION, abi.INFO_JERK_COST)
INFO_NAMES = {v: k[5:] for k, v in vars(abi).items() if k.startswith("INFO_") and k != "INFO_K"}
assert sorted(INFO_EXACT + INFO_CLOSE + (abi.INFO_MIN_DIST,)) == list(range(abi.INFO_K))


def _info_err(errs, where, k, bad, got, want, event):
    r = np.nonzero(bad)[0]
    errs.append("%sinfo %s: %d of %d rows differ, e.g. rows %s (events %s) got=%s want=%s" % (
        where, INFO_NAMES[k], r.size, bad.size, r[:3].tolist(), np.asarray(event)[r[:3]].tolist(),
        got[r[:3], k].tolist(), want[r[:3], k].tolist()))


def compare_info(got, want, event, where="", min_personal_space=None, tally=None):
    """Compare [E][INFO_K] info rows, every column of every row; returns a list of mismatch strings.
    INFO_EXACT columns must be equal, INFO_CLOSE columns agree within atol 1e-4 + rtol 1e-5, MIN_DIST within
    POS_TOL on every row (inf equals inf; inf against a finite value, or a NaN on either side, is a mismatch).
    `event` ([E] event codes) names the rows in the messages.

    Free-running comparisons (states only within POS_TOL) pass min_personal_space: a PERSONAL_VIOLATION
    difference is then let through only where want's own MIN_DIST lies within POS_TOL of that threshold.
    `tally` (a dict) accumulates "rows" and "personal_flips" so that the caller can cap the latter."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.ndim == 2 and got.shape[1] == abi.INFO_K, (got.shape, want.shape)
    errs = []
    if tally is not None:
        tally["rows"] = tally.get("rows", 0) + got.shape[0]
    for k in INFO_EXACT:
        bad = ~(got[:, k] == want[:, k])
        if k == abi.INFO_PERSONAL_VIOLATION and min_personal_space is not None:
            near = np.abs(want[:, abi.INFO_MIN_DIST].astype(np.float64) - min_personal_space) <= POS_TOL
            if tally is not None:
                tally["personal_flips"] = tally.get("personal_flips", 0) + int((bad & near).sum())
            bad &= ~near
        if bad.any():
            _info_err(errs, where, k, bad, got, want, event)
    for k in INFO_CLOSE:
        a, b = got[:, k].astype(np.float64), want[:, k].astype(np.float64)
        bad = ~(np.abs(a - b) <= 1e-4 + 1e-5 * np.abs(b))
        if bad.any():
            _info_err(errs, where, k, bad, got, want, event)
    k = abi.INFO_MIN_DIST
    a, b = got[:, k].astype(np.float64), want[:, k].astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~((a == b) | (np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= POS_TOL)))
    if bad.any():
        _info_err(errs, where, k, bad, got, want, event)
    return errs


def compare_monitor(got_epr, got_epl, want_epr, want_epl, done, where="", keep=None):
    """Monitor outputs of the episodes that ended at this step (rows where `done`): ep_len exact, ep_return
    within atol 1e-4. `keep` ([E] bool) takes rows out of the ep_return comparison only (a reward masked by a
    norm-zone flip, tests/test_gpu_parity.py::_teacher_forced). Returns a list of mismatch strings."""
    dm = np.asarray(done).astype(bool)
    errs = []
    a, b = np.asarray(got_epl)[dm], np.asarray(want_epl)[dm]
    if not np.array_equal(a, b):
        errs.append("%sep_len %s vs %s" % (where, a, b))
    if keep is not None:
        dm = dm & np.asarray(keep, bool)
    a, b = np.asarray(got_epr, np.float64)[dm], np.asarray(want_epr, np.float64)[dm]
    if not (np.abs(a - b) <= 1e-4).all():
        errs.append("%sep_return %s vs %s" % (where, a, b))
    return errs


def min_dist_ref(sv):
    """calc_reward's dmin of a pre-step state (crowd_sim.py:909-946), float64: the least surface distance
    over the humans in order, up to the first human in collision; inf when human 0 collides."""
    E, N = sv.E, sv.N
    dx = np.asarray(sv.h_px, np.float64).reshape(E, N) - np.asarray(sv.r_px, np.float64).reshape(E, 1)
    dy = np.asarray(sv.h_py, np.float64).reshape(E, N) - np.asarray(sv.r_py, np.float64).reshape(E, 1)
    cd = (dx ** 2 + dy ** 2) ** 0.5 - np.asarray(sv.h_r, np.float64).reshape(E, N) \
        - np.asarray(sv.r_radius, np.float64).reshape(E, 1)
    counted = np.cumsum(cd < 0, axis=1) == 0
    return np.where(counted, cd, np.inf).min(axis=1)


def compare_step(t, d, obs, rew, done, ev, info, epr, epl, tol=POS_TOL, pre=None):
    """One step of an engine against step t of a roll_*.npz fixture. The fixtures hold MIN_DIST only where the
    reference reports it (Danger rows, NaN elsewhere); with `pre` (the state the step started from) the other
    rows are compared with min_dist_ref(pre)."""
    errs = []
    for key, ok in (("robot_node", "robot_node"), ("temporal", "temporal_edges"), ("spatial", "spatial_edges")):
        a = np.asarray(obs[ok]).reshape(d[key][t].shape).astype(np.float64)
        b = d[key][t].astype(np.float64)
        if not np.allclose(a, b, atol=tol, rtol=0):
            i = np.unravel_index(np.argmax(np.abs(a - b)), a.shape)
            errs.append("t=%d obs %s max err %g at %s" % (t, key, np.abs(a - b).max(), i))
    if not np.array_equal(np.asarray(done).astype(np.uint8), d["done"][t]):
        errs.append("t=%d done %s vs %s" % (t, np.asarray(done).astype(int), d["done"][t]))
    if not np.array_equal(np.asarray(ev), d["event"][t]):
        errs.append("t=%d event %s vs %s" % (t, np.asarray(ev), d["event"][t]))
    if not np.allclose(np.asarray(rew, np.float64), d["reward"][t].astype(np.float64), atol=tol, rtol=0):
        errs.append("t=%d reward %s vs %s" % (t, rew, d["reward"][t]))
    errs += compare_monitor(epr, epl, d["ep_return"][t], d["ep_len"][t], d["done"][t], where="t=%d " % t)
    want = d["info"][t]
    unrecorded = np.isnan(want[:, abi.INFO_MIN_DIST]) & (d["event"][t] != abi.EV_DANGER)
    if pre is not None and unrecorded.any():
        want = want.copy()
        want[unrecorded, abi.INFO_MIN_DIST] = min_dist_ref(pre)[unrecorded]
    errs += compare_info(info, want, ev, where="t=%d " % t)
    return errs


def run_teacher_forced(eng, d, cfg, tol=POS_TOL, max_errs=20):
    """Teacher-forced replay of a roll_*.npz fixture on an engine exposing set_state/step/get_state.
    Before step t the engine gets the reference's post-state of step t-1 (its own MT19937 words are
    carried forward: the fixture stores a CRC of the reference stream, checked every step)."""
    errs = []
    T = d["actions"].shape[0]
    st = state_from(d, "init_", cfg)
    pv_mismatch = 0
    for t in range(T):
        eng.set_state(st)
        obs, rew, done, ev, info, epr, epl = eng.step(d["actions"][t])
        got = eng.get_state()
        errs += compare_step(t, d, obs, rew, done, ev, info, epr, epl, tol, pre=st)
        errs += compare_state(got, at(d, "post_", t), "post_", tol, where="t=%d " % t)
        pv_mismatch += int((np.asarray(info)[:, abi.INFO_PATH_VIOLATION] != d["info"][t][:, abi.INFO_PATH_VIOLATION]).sum())
        if len(errs) >= max_errs:
            break
        st = state_from(at(d, "post_", t), "post_", cfg, mt=got.mt)
    if pv_mismatch:
        errs.append("path_violation mismatches: %d" % pv_mismatch)
    return errs


# ---- DSRNN policy fixtures (tests/golden/dsrnn.npz, generated by oracle/gen_golden.py:gen_dsrnn) ----
def procedural_state_dict(model):
    """Same deterministic weights the fixture generator loaded into the reference Policy
    (oracle/gen_golden.py:procedural_state_dict): sorted key p ~ RandomState(1000+p).uniform(+-1/sqrt(fan_in))."""
    import math

    import torch

    out = {}
    for p, (k, v) in enumerate(sorted(model.state_dict().items())):
        shape = tuple(v.shape)
        s = 1.0 / math.sqrt(shape[-1] if len(shape) > 1 else 1)
        out[k] = torch.from_numpy(np.random.RandomState(1000 + p).uniform(-s, s, shape).astype(np.float32))
    return out


class BoxSpace:
    """Stand-in for gym.spaces.Box (only the class name and shape are read by Policy)."""

    def __init__(self, shape):
        self.shape = shape


BoxSpace.__name__ = "Box"


def make_policy(N, E=4, T=8, device="cpu", **srnn_sizes):
    """srnn_sizes: overrides of config.SRNN fields (e.g. human_node_rnn_size=96)."""
    from crowdnav_dsrnn_amd.policy import Policy

    c = clone_config(Config())
    c.sim.human_num = N
    c.training.num_processes = E
    c.ppo.num_steps = T
    c.ppo.num_mini_batch = 1
    for k, v in srnn_sizes.items():
        assert hasattr(c.SRNN, k), k
        setattr(c.SRNN, k, v)
    pol = Policy({}, BoxSpace((2,)), base="srnn", base_kwargs=c)
    pol.load_state_dict(procedural_state_dict(pol))
    return pol.to(device).eval()


def edge_features_fp32(robot_node, temporal, spatial, Wt, bt, Ws, bs, Wr, br, Wn, bn):
    """Plain PyTorch fp32 restatement of the fused input layers (srnn_model.py:160-161, 210-211, 466)."""
    import torch

    E, N = temporal.shape[0], spatial.shape[1]
    t = torch.relu(temporal.reshape(E, 2) @ Wt.t() + bt)
    s = torch.relu(spatial.reshape(E * N, 2) @ Ws.t() + bs).reshape(E, N, 64)
    n = torch.relu((robot_node.reshape(E, 7) @ Wr.t() + br) @ Wn.t() + bn)
    return t, s, n


def masked_gru_ref(x, h0, masks, w_ih, w_hh, b_ih, b_hh):
    """Plain PyTorch fp32 restatement of the mask-segmented GRU (srnn_model.py:52-104): per step
    h <- h * mask[t], then torch.gru_cell (nn.GRU's cell)."""
    import torch

    outs = []
    h = h0
    for t in range(x.shape[0]):
        h = torch.gru_cell(x[t], h * masks[t].unsqueeze(-1), w_ih, w_hh, b_ih, b_hh)
        outs.append(h)
    return torch.stack(outs, 0), h


def gru_infer_step_ref(x, h0, m, w_ih, w_hh, b_ih, b_hh, dest):
    """Plain PyTorch restatement of ops.gru_infer_step: one masked GRU cell step over grouped rows,
    the new state also written into dest."""
    import torch

    h0g = h0 if h0.dim() == 3 else h0.unsqueeze(1)
    R, G, H = h0g.shape
    hm = (h0g * m.reshape(R, 1, 1)).reshape(R * G, H)
    h = torch.gru_cell(x.reshape(R * G, -1), hm, w_ih, w_hh, b_ih, b_hh)
    if dest is not None:
        (dest if dest.dim() == 3 else dest.unsqueeze(1)).copy_(h.view(R, G, H))
    return h


def attention_pool_ref(hs, attn):
    """Plain PyTorch restatement of EdgeAttention's weighted sum (srnn_model.py:320-333)."""
    import torch

    return torch.bmm(hs.transpose(1, 2), attn).squeeze(-1)


def gru_step_fwd_ref(gi, gh, hm, m_next=None):
    """One GRU step after the two GEMMs as include/crowdnav.h states it for cn_gru_fwd_step (gate order
    r | z | n), in the operands' dtype (float64 in the tests): returns h, hm_next = h * m_next (h itself with
    m_next None) and the record save = r | z | n | gh_n."""
    import torch

    H = hm.shape[1]
    r = torch.sigmoid(gh[:, :H] + gi[:, :H])
    z = torch.sigmoid(gh[:, H:2 * H] + gi[:, H:2 * H])
    ghn = gh[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * ghn)
    h = (hm - n) * z + n
    hm_next = h if m_next is None else h * m_next.unsqueeze(-1)
    return h, hm_next, torch.cat((r, z, n, ghn), 1)


def gru_step_bwd_ref(acc, m_next, dout, save, hm):
    """Gradient of one step as include/crowdnav.h states it for cn_gru_bwd_step: g = acc * m_next + dout is
    dL/dh_t; returns the new acc = g * z, dgi = dr | dz | dn and dgh = dr | dz | dhn ([B][3H] each)."""
    import torch

    H = hm.shape[1]
    r, z, n, ghn = (save[:, k * H:(k + 1) * H] for k in range(4))
    g = acc if m_next is None else acc * m_next.unsqueeze(-1)
    if dout is not None:
        g = g + dout
    dn = g * (1 - z) * (1 - n * n)
    dz = g * (hm - n) * z * (1 - z)
    dr = dn * ghn * r * (1 - r)
    dhn = dn * r
    return g * z, torch.cat((dr, dz, dn), 1), torch.cat((dr, dz, dhn), 1)


def gru_row_tile(Bs, H):
    """Row tile (128, or 32 = split-K) the sequence / fused-step GRU kernels pick on the current device for
    one launch over GRUs of Bs rows: cn_gru_bwd_seq_work_elems(1, H, ...) is 64 x 4H floats for the bias
    reduction plus 4H per row tile of every GRU. Needs row counts at which the two tilings differ."""
    from crowdnav_dsrnn_amd import _lib

    Bs = tuple(int(b) for b in ((Bs,) if isinstance(Bs, int) else Bs))
    segs = (_lib.GruSeqBwd * len(Bs))()
    for s, b in zip(segs, Bs):
        s.B = b
    tiles = (_lib.lib().cn_gru_bwd_seq_work_elems(1, H, len(Bs), segs) - 64 * 4 * H) // (4 * H)
    n128, n32 = (sum((b + t - 1) // t for b in Bs) for t in (128, 32))
    assert n128 != n32, "row counts %s do not tell the tilings apart" % (Bs,)
    assert tiles in (n128, n32), (tiles, n128, n32)
    return 128 if tiles == n128 else 32


def gru_form_rows(H, cus):
    """(B_hi, B_lo): total row counts on either side of the sequence kernels' threshold on a device with
    `cus` compute units. 128-row tiles run when ceil(rows / 128) * (H / 32) >= cus, so the smallest such
    row count is Rmin = 128 * (ceil(cus / (H / 32)) - 1) + 1; B_hi = Rmin + 40 has a ragged last 128-row
    tile and B_lo = Rmin - 20 is split-K with a ragged last 32-row tile."""
    ut = H // 32
    rmin = 128 * ((cus + ut - 1) // ut - 1) + 1
    return rmin + 40, rmin - 20
