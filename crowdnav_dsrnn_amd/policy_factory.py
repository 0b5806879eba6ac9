"""Agent policy plugin surface: `policy_factory[name](config).predict(JointState) -> ActionXY`.

Mirrors crowd_nav/policy/policy_factory.py:1-17: the reference's humans call
`policy.predict(JointState(self FullState, [ObservableState]))` once per human per step
(crowd_sim.py:1121-1161 -> human.py:11-20). Here 'orca' and 'social_force' run on the GPU through the
C ABI (`cn_orca_predict`: the step kernel's quad-cooperative RVO2 code path; `cn_social_force_predict`:
the step kernel's f64 social force), one launch per call; `predict_batch` takes many agents' states in
one launch (the MI355X-shaped use). 'none' returns None like the reference; 'srnn' / 'convgru' keep
SRNN.clip_action (crowd_nav/policy/srnn.py:18-48). Any other name is absent, as in the reference.

ORCA keeps the reference's per-object simulator semantics (orca.py:85-115): the simulator -- and with it
every agent's ORCA radius (radius + 0.01 + safety_space) and max speed (own v_pref, others 1) -- is
created at the first predict and only re-created when the number of agents changes; later calls only
update positions and velocities. RVO2 works in float32 (positions, velocities, radii, the preferred
velocity are cast at the boundary) and returns float32 velocities. Simulators of <= 10 agents run on the
engine's quad path (`cn_orca_predict`); 11 to 64 agents on the kd-tree path (`cn_orca_predict_kd`, RVO2's
KdTree neighbour order with the persisted agents_ permutation); more than 64 raise UnsupportedConfig.

`ScriptedRobot(venv, name)` is the other direction: an actor stand-in that drives the ROBOT of a
CrowdNavVecEnv with 'orca' / 'social_force' computed on the device from the engine's state
(`cn_robot_act`), for baseline rows of `evaluate()` and expert rollouts without a host round trip. For the
unicycle robot it also takes 'dwa', this project's dynamic-window controller (`dwa_predict` restates it on the
host; `DWA_DEFAULTS`; the device side is `cn_dwa_predict` / `cn_scripted_dwa`).
"""
import collections
import ctypes
import math

import numpy as np

from . import _lib
from .config import UnsupportedConfig, no_visible_masks

ActionXY = collections.namedtuple("ActionXY", ["vx", "vy"])      # crowd_sim/envs/utils/action.py:3
ActionRot = collections.namedtuple("ActionRot", ["v", "r"])      # crowd_sim/envs/utils/action.py:4


class FullState:
    """crowd_sim/envs/utils/state.py FullState(px, py, vx, vy, radius, gx, gy, v_pref, theta)."""

    def __init__(self, px, py, vx, vy, radius, gx, gy, v_pref, theta):
        self.px, self.py, self.vx, self.vy, self.radius = px, py, vx, vy, radius
        self.gx, self.gy, self.v_pref, self.theta = gx, gy, v_pref, theta
        self.position = (px, py)
        self.goal_position = (gx, gy)
        self.velocity = (vx, vy)


class ObservableState:
    """crowd_sim/envs/utils/state.py ObservableState(px, py, vx, vy, radius)."""

    def __init__(self, px, py, vx, vy, radius):
        self.px, self.py, self.vx, self.vy, self.radius = px, py, vx, vy, radius
        self.position = (px, py)
        self.velocity = (vx, vy)


class JointState:
    """crowd_sim/envs/utils/state.py JointState(self_state, human_states)."""

    def __init__(self, self_state, human_states):
        assert isinstance(self_state, FullState)
        for h in human_states:
            assert isinstance(h, ObservableState)
        self.self_state = self_state
        self.human_states = human_states


def _torch_stream():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("agent policies run on the GPU (torch.cuda.is_available() is False)")
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


MAX_ORCA_AGENTS = 64   # cn_orca_predict_kd's simulator size limit (include/crowdnav.h)


class Policy:
    """crowd_nav/policy/policy.py:5-19 (attributes the env sets: time_step, phase, env, ...)."""

    def __init__(self, config):
        self.trainable = False
        self.phase = None
        self.model = None
        self.device = None
        self.last_state = None
        self.time_step = None
        self.env = None
        self.config = config

    def predict(self, state):
        raise NotImplementedError

    @staticmethod
    def reach_destination(state):
        s = state.self_state
        return np.linalg.norm((s.py - s.gy, s.px - s.gx)) < s.radius


class ORCA(Policy):
    """crowd_nav/policy/orca.py:6-139 on the GPU (cn_orca_predict)."""

    def __init__(self, config):
        super().__init__(config)
        self.name = "ORCA"
        self.max_neighbors = None
        self.radius = None
        self.max_speed = 1
        # the simulator's state that outlives a predict (orca.py:85-115): agent count, frozen radii f32 [A],
        # self max speed f32, and RVO2's KdTree agent order (KdTree::agents_, re-permuted by every doStep's
        # tree build; it decides the order of equally distant neighbours when A > 10)
        self.sim = None

    def _frame(self, state):
        """float32 agents [A][5] (px, py, vx, vy, frozen radius) and [maxSpeed, pref.x, pref.y] of agent 0."""
        s, hs = state.self_state, state.human_states
        A = len(hs) + 1
        if A > MAX_ORCA_AGENTS:
            raise UnsupportedConfig("ORCA.predict: %d agents per simulator (the GPU predict serves <= %d)"
                                    % (A, MAX_ORCA_AGENTS))
        self.max_neighbors = len(hs)
        self.radius = s.radius
        if self.sim is not None and self.sim[0] != A:   # orca.py:85-90
            self.sim = None
        if self.sim is None:                            # orca.py:91-109: parameters frozen at creation
            safety = self.config.orca.safety_space
            radii = np.array([s.radius + 0.01 + safety] + [h.radius + 0.01 + safety for h in hs], np.float32)
            self.sim = (A, radii, np.float32(s.v_pref), np.arange(A, dtype=np.uint8))
        ag = np.zeros((A, 5), np.float32)
        ag[0, :4] = (s.px, s.py, s.vx, s.vy)
        for k, h in enumerate(hs):
            ag[k + 1, :4] = (h.px, h.py, h.vx, h.vy)
        ag[:, 4] = self.sim[1]
        v = np.array((s.gx - s.px, s.gy - s.py))     # orca.py:118-122
        speed = np.linalg.norm(v)
        pref = v / speed if speed > 1 else v
        return ag, np.array([self.sim[2], pref[0], pref[1]], np.float32)

    def predict(self, state):
        return predict_batch([self], [state])[0]


class SOCIAL_FORCE(Policy):
    """crowd_nav/policy/social_force.py:6-66 on the GPU (cn_social_force_predict, float64)."""

    def __init__(self, config):
        super().__init__(config)
        self.name = "social_force"

    def predict(self, state):
        return predict_batch([self], [state])[0]


class SRNN(Policy):
    """crowd_nav/policy/srnn.py:6-48: the robot policy placeholder of the env (the network is
    crowdnav_dsrnn_amd.policy.Policy); clip_action mutates raw_action in place like the reference."""

    def __init__(self, config):
        super().__init__(config)
        self.time_step = config.env.time_step
        self.name = "srnn" if config.robot.policy == "srnn" else config.robot.policy
        self.trainable = True
        self.multiagent_training = True

    def clip_action(self, raw_action, v_pref):
        if self.config.action_space.kinematics == "holonomic":
            n = np.linalg.norm(raw_action)
            if n > v_pref:
                raw_action[0] = raw_action[0] / n * v_pref
                raw_action[1] = raw_action[1] / n * v_pref
            return ActionXY(raw_action[0], raw_action[1])
        raw_action[0] = np.clip(raw_action[0], -0.1, 0.1)
        raw_action[1] = np.clip(raw_action[1], -0.1, 0.1)
        return ActionRot(raw_action[0], raw_action[1])

    def predict(self, state):
        raise NotImplementedError("the srnn robot is driven by the learner's actions (CrowdSimDict.step)")


def none_policy():
    return None


def predict_batch(policies, states):
    """predict() of many agents in one launch per policy kind: policies[i].predict(states[i]) for all i
    (ORCA agents grouped by simulator size). Returns a list of ActionXY (python floats)."""
    if len(policies) != len(states):
        raise ValueError("one state per policy")
    out = [None] * len(policies)
    torch, dev, st = None, None, None
    L = _lib.lib()
    orca_by_a, sf_by_m = {}, {}
    for i, (p, s) in enumerate(zip(policies, states)):
        if isinstance(p, ORCA):
            orca_by_a.setdefault(len(s.human_states) + 1, []).append(i)
        elif isinstance(p, SOCIAL_FORCE):
            sf_by_m.setdefault(len(s.human_states), []).append(i)
        else:
            raise TypeError("predict_batch: ORCA / SOCIAL_FORCE policies only, got %r" % type(p).__name__)
    if orca_by_a or sf_by_m:
        torch, dev, st = _torch_stream()
    for A, idx in orca_by_a.items():
        frames = [policies[i]._frame(states[i]) for i in idx]
        ag = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
        sf = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
        res = torch.zeros((len(idx), 4), dtype=torch.float32, device=dev)
        c = policies[idx[0]].config
        ts = policies[idx[0]].time_step or c.env.time_step
        if A > 10:   # KdTree path: each simulator's persisted agent order goes in and comes back re-permuted
            perm = torch.from_numpy(np.stack([policies[i].sim[3] for i in idx])).to(dev)
            _lib.check(L.cn_orca_predict_kd(st, len(idx), A, ag.data_ptr(), sf.data_ptr(),
                                            float(c.orca.neighbor_dist), float(c.orca.time_horizon), float(ts),
                                            perm.data_ptr(), res.data_ptr()))
            pn = perm.cpu().numpy()
            for k, i in enumerate(idx):
                policies[i].sim[3][:] = pn[k]
        else:
            _lib.check(L.cn_orca_predict(st, len(idx), A, ag.data_ptr(), sf.data_ptr(), float(c.orca.neighbor_dist),
                                         float(c.orca.time_horizon), float(ts), res.data_ptr()))
        r = res.cpu().numpy()
        for k, i in enumerate(idx):
            out[i] = ActionXY(float(r[k, 0]), float(r[k, 1]))
            policies[i].last_state = states[i]
    for M, idx in sf_by_m.items():
        selfs = np.array([[states[i].self_state.px, states[i].self_state.py, states[i].self_state.vx,
                           states[i].self_state.vy, states[i].self_state.radius, states[i].self_state.gx,
                           states[i].self_state.gy, states[i].self_state.v_pref, states[i].self_state.theta]
                          for i in idx], np.float64)
        oth = np.array([[[h.px, h.py, h.vx, h.vy, h.radius] for h in states[i].human_states] for i in idx],
                       np.float64).reshape(len(idx), M, 5)
        s_d = torch.from_numpy(selfs).to(dev)
        o_d = torch.from_numpy(np.ascontiguousarray(oth)).to(dev)
        res = torch.zeros((len(idx), 2), dtype=torch.float64, device=dev)
        c = policies[idx[0]].config
        _lib.check(L.cn_social_force_predict(st, len(idx), M, s_d.data_ptr(), o_d.data_ptr() if M else None,
                                             float(c.sf.A), float(c.sf.B), float(c.sf.KI), float(c.env.time_step),
                                             res.data_ptr()))
        r = res.cpu().numpy()
        for k, i in enumerate(idx):
            out[i] = ActionXY(float(r[k, 0]), float(r[k, 1]))
    return out


def unicycle_track(vxy, theta, v):
    """The unicycle robot's tracking law on the host (numpy float64), for a robot driven from a host-side `predict`:
    from desired velocities vxy (..., 2) -- an ORCA / SOCIAL_FORCE ActionXY -- and the robot's heading `theta` and
    speed `v` (the engine's r_theta and r_dv), the (..., 2) float32 unicycle actions (dv, dtheta) that the env's step
    takes. What cn_robot_act / cn_rollout compute on the device after cn_scripted_unicycle (include/crowdnav.h):

        s = |vxy|;  s == 0: dtheta = 0, target = 0
        else: delta = remainder(atan2(vy, vx) - theta, 2 pi);  dtheta = clip(delta, -0.1, 0.1)
              target = s * max(0, cos(delta - dtheta))         (on the heading the step will have; never backwards)
        dv = clip(target - v, -0.1, 0.1)

    The velocity is rounded to float32 first, as the device controllers round theirs. The transcendental functions
    are the C library's (math.atan2 / remainder / cos per row), not numpy's vector variants, which may differ from
    them in the last bit.
    Both components lie in [-0.1, 0.1], the range the step clips a unicycle action to."""
    vxy = np.asarray(vxy, np.float32).astype(np.float64)   # (the squares below are then exact: one rounding in s)
    ux, uy, theta, v = np.broadcast_arrays(vxy[..., 0], vxy[..., 1], np.asarray(theta, np.float64),
                                           np.asarray(v, np.float64))
    out = np.empty(ux.shape + (2,), np.float64)
    flat = out.reshape(-1, 2)
    for k, (x, y, th, sp) in enumerate(zip(ux.ravel().tolist(), uy.ravel().tolist(), theta.ravel().tolist(),
                                           v.ravel().tolist())):
        s = math.sqrt(x * x + y * y)
        turn = target = 0.0
        if s != 0.0:
            delta = math.remainder(math.atan2(y, x) - th, 2.0 * math.pi)
            turn = min(max(delta, -0.1), 0.1)
            target = s * max(0.0, math.cos(delta - turn))
        flat[k, 0] = min(max(target - sp, -0.1), 0.1)
        flat[k, 1] = turn
    return out.astype(np.float32)


# The dynamic-window controller's default parameters (cn_dwa_params): the row of the highest success rate on 500
# validation episodes of the default unicycle config over the grids of tools/dwa_grid.py tabulated in DESIGN.md §4
# ("A dynamic-window expert for the unicycle robot"; profiles/dwa/grid_val*.jsonl).
DWA_DEFAULTS = {"horizon": 10, "w_goal": 1.0, "w_clear": 8.0, "d_safe": 2.0, "w_col": 100.0}


def dwa_params(params=None):
    """DWA_DEFAULTS with the overrides of `params` (None / True: none; a dict with some of its keys), checked by the
    rule of include/crowdnav.h: horizon in 1..16, d_safe > 0, every weight finite."""
    p = dict(DWA_DEFAULTS)
    if isinstance(params, dict):
        extra = set(params) - set(p)
        if extra:
            raise ValueError("dwa parameters: unknown keys %s (of %s)" % (sorted(extra), sorted(p)))
        p.update(params)
    elif params is not None and params is not True:
        raise TypeError("dwa parameters: None, True or a dict, got %r" % type(params).__name__)
    p["horizon"] = int(p["horizon"])
    for k in ("w_goal", "w_clear", "d_safe", "w_col"):
        p[k] = float(p[k])
        if not math.isfinite(p[k]):
            raise ValueError("dwa parameters: %s must be finite, got %r" % (k, p[k]))
    if not 1 <= p["horizon"] <= 16 or not p["d_safe"] > 0:
        raise ValueError("dwa parameters: horizon in 1..16 and d_safe > 0 required, got %r" % (p,))
    return p


DWA_GRID = tuple((0.1 * (2 * k - 7)) / 7 for k in range(8))   # dv of a = k, dtheta of b = k


def dwa_predict(self_state, v, others, time_step, params=None, detail=False):
    """The unicycle robot's dynamic-window controller on the host (Python floats: float64), the definition in
    include/crowdnav.h restated; what cn_dwa_predict, and cn_robot_act / cn_rollout with the policy 'dwa', compute on
    the device. self_state (n, 9) = (px, py, vx, vy, radius, gx, gy, v_pref, theta), v (n,) the robot's speed (the
    engine's r_dv), others (n, M, 5) = (px, py, vx, vy, radius) of the humans; params: see dwa_params.
    Returns (actions (n, 2) float32, choice (n,) int32, costs (n, 64) float64); with detail=True also a dict of
    (n, 64) arrays 'hit', 'gterm', 'cmin' and 'sharp' (False where some c_k, or some g_k - r, of the candidate's walk
    lies within 1e-9 of 0: a last-bit difference of the device's sin / cos could then flip a comparison).
    math.sin / cos / sqrt per value, not numpy's vector variants, which may differ from them in the last bit."""
    p = dwa_params(params)
    H, wg, wc, ds, wk = p["horizon"], p["w_goal"], p["w_clear"], p["d_safe"], p["w_col"]
    S = np.asarray(self_state, np.float64).reshape(-1, 9)
    n = len(S)
    V = np.asarray(v, np.float64).reshape(n)
    O = np.asarray(others, np.float64).reshape(n, -1, 5)
    dt = float(time_step)
    inf = float("inf")
    sin, cos, sqrt = math.sin, math.cos, math.sqrt
    costs = np.empty((n, 64), np.float64)
    hits, gterms, cmins = np.zeros((n, 64), np.int32), np.zeros((n, 64)), np.zeros((n, 64))
    sharp = np.ones((n, 64), bool)
    choice = np.zeros(n, np.int32)
    for e in range(n):
        px, py, _, _, r, gx, gy, vpref, theta = S[e].tolist()
        hum = O[e].tolist()
        s0, c0 = sin(theta), cos(theta)
        best = 0
        for c in range(64):
            dv, dth = DWA_GRID[c >> 3], DWA_GRID[c & 7]
            v1 = min(max(V[e].item() + dv, -vpref), vpref)
            R = v1 / (dth / dt)
            cx, cy = px - R * s0, py + R * c0
            cmin, hit, gterm, ok = inf, 0, 0.0, True
            for k in range(1, H + 1):
                phi = theta + k * dth
                x, y = cx + R * sin(phi), cy - R * cos(phi)
                kt = k * dt
                ck = inf
                for bx, by, bvx, bvy, br in hum:
                    dx, dy = x - (bx + kt * bvx), y - (by + kt * bvy)
                    ck = min(ck, sqrt(dx * dx + dy * dy) - r - br)
                cmin = min(cmin, ck)
                if ck < 0.0 and hit == 0:
                    hit = H + 1 - k
                dx, dy = x - gx, y - gy
                gk = sqrt(dx * dx + dy * dy)
                ok = ok and abs(ck) > 1e-9 and abs(gk - r) > 1e-9
                gterm = gk
                if gk < r:
                    gterm = 0.0
                    break
            J = (wg * gterm + (wc * max(0.0, ds - cmin)) / ds) + wk * hit
            costs[e, c], hits[e, c], gterms[e, c], cmins[e, c], sharp[e, c] = J, hit, gterm, cmin, ok
            if J < costs[e, best]:
                best = c
        choice[e] = best
    grid = np.array(DWA_GRID, np.float64)
    actions = np.stack([grid[choice >> 3], grid[choice & 7]], axis=1).astype(np.float32)
    if detail:
        return actions, choice, costs, {"hit": hits, "gterm": gterms, "cmin": cmins, "sharp": sharp}
    return actions, choice, costs


def dwa_regret(costs, choice):
    """cn_robot_act_regret's regret rows on the host (numpy), include/crowdnav.h restated: costs (n, 64) float64 and
    choice (n,) -- dwa_predict's or cn_dwa_predict's -- -> (n, 64) float32, (float32)(J_c - J_choice) with the
    subtraction in float64 and the rounding to float32 the only rounding: +0.0 at the choice and at every candidate tied
    with it, >= 0 everywhere (the choice has the smallest cost)."""
    J = np.asarray(costs, np.float64).reshape(-1, 64)
    b = np.asarray(choice).reshape(-1).astype(np.int64)
    if len(b) != len(J):
        raise ValueError("dwa_regret: costs (n, 64) and choice (n,) required")
    return (J - J[np.arange(len(J)), b][:, None]).astype(np.float32)


def _philox4x32_10(c0, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) of counter (c0, 0, 0, 0) under key (k0, k1),
    broadcast over numpy arrays, in uint64 arithmetic: the four output words as uint64 arrays < 2^32. The block of
    cn_rollout_noisy and cn_robot_mix (include/crowdnav.h)."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, k0, k1 = np.broadcast_arrays(*[np.asarray(v, np.int64).astype(np.uint64) & m32 for v in (c0, k0, k1)])
    x0, x1, x2, x3 = c0, np.zeros_like(c0), np.zeros_like(c0), np.zeros_like(c0)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x0, np.uint64(0xCD9E8D57) * x2   # 32 x 32 -> 64 bits: no overflow
        x0, x1, x2, x3 = (p1 >> np.uint64(32)) ^ x1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ x3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return x0, x1, x2, x3


def mix_coin(seed, k, G):
    """cn_robot_mix's coin on the host (numpy): u = (float32)(w.z >> 8) * 2^-24 in [0, 1), w = philox4x32_10(counter
    (uint32)k, key ((uint32)seed, (uint32)G)); k = step0 + t of the caller's coin sequence, G the env's global index
    (env_offset + e). k and G broadcast; float32 out. The expert's action is executed where u < beta."""
    z = _philox4x32_10(k, np.int64(int(seed) & 0xFFFFFFFF), G)[2]
    return ((z >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def robot_mix_ref(label, learner, beta, seed, k, G):
    """cn_robot_mix's select on the host (numpy), include/crowdnav.h restated: for labels and learner actions
    (..., 2) float32 with k and G broadcasting over the leading axes, (executed (..., 2) float32, flags (...) uint8):
    took = mix_coin(seed, k, G) < (float32)beta; executed = label where took, else learner, copied as bits; flags bit
    0 = took, bit 1 = learner equals label in both components as bits."""
    lab = np.ascontiguousarray(label, np.float32)
    lea = np.ascontiguousarray(learner, np.float32)
    if lab.shape != lea.shape or lab.shape[-1:] != (2,):
        raise ValueError("robot_mix_ref: label and learner of one shape (..., 2) required")
    took = np.broadcast_to(mix_coin(seed, k, G) < np.float32(beta), lab.shape[:-1])
    lb, le = lab.view(np.uint32), lea.view(np.uint32)
    executed = np.where(took[..., None], lb, le).astype(np.uint32).view(np.float32)
    same = (lb == le).all(axis=-1)
    return executed, (took.astype(np.uint8) | (same.astype(np.uint8) << 1)).astype(np.uint8)


class _ScriptedBase:
    """The one attribute evaluate() reads of an actor's `base` (it sizes the edge RNN state by it)."""

    def __init__(self, human_num):
        self.human_num = human_num


class ScriptedRobot:
    """Actor stand-in that drives the robot of a CrowdNavVecEnv with a scripted controller on the device
    (cn_robot_act): the reference's "for orca and sf" robot (crowd_sim.py:1113-1114 -> robot.py:9-15), whose
    policy predicts from the robot's own state and its belief of the humans. `name`: 'orca', 'social_force', or
    'dwa' (this project's dynamic-window controller of the unicycle robot, dwa_predict: unicycle configs with the
    opt-in config.robot.scripted_dwa; it emits the unicycle action itself, no tracking law). With it evaluate() and EpisodeRecorder run a baseline unchanged:

        evaluate(ScriptedRobot(venv, 'orca'), None, venv, E, device, config, logging)

    The env's config keeps robot.policy 'srnn' / 'convgru' (that selects the observation); holonomic, as the
    controllers return ActionXY, or unicycle with the opt-in config.robot.scripted_unicycle, where a tracking law
    (unicycle_track) turns the controller's velocity into the unicycle action on the device. There a rollout's noise
    sigma is in action units: 0.1 is the whole range. On an env of varying human count (config.sim.human_nums, with the opt-in
    config.sim.human_nums_scripted) every env is driven by the controller of its own count; `base.human_num` is the
    padded (largest) one."""

    NAMES = ("orca", "social_force", "dwa")

    @classmethod
    def check(cls, venv, name):
        """UnsupportedConfig for an unknown controller, a unicycle config without the opt-in
        config.robot.scripted_unicycle ('dwa': anything but a unicycle config with the opt-in
        config.robot.scripted_dwa), or an env of varying human count
        (config.sim.human_nums) without the opt-in config.sim.human_nums_scripted (before anything touches the
        GPU)."""
        if name not in cls.NAMES:
            raise UnsupportedConfig("ScriptedRobot: %r (one of %s)" % (name, ", ".join(cls.NAMES)))
        config = venv.config
        if name == "dwa":
            if config.action_space.kinematics != "unicycle" or not getattr(config.robot, "scripted_dwa", None):
                raise UnsupportedConfig("ScriptedRobot: 'dwa' plans in the unicycle robot's action space: "
                                        "action_space.kinematics 'unicycle' with the opt-in config.robot.scripted_dwa "
                                        "required (kinematics=%r)" % config.action_space.kinematics)
        elif config.action_space.kinematics != "holonomic" and not getattr(config.robot, "scripted_unicycle", False):
            raise UnsupportedConfig("ScriptedRobot: action_space.kinematics=%r (the controllers return ActionXY: "
                                    "holonomic only, unless config.robot.scripted_unicycle puts the tracking law "
                                    "behind them)" % config.action_space.kinematics)
        if getattr(config.sim, "human_nums", None) is not None and not getattr(config.sim, "human_nums_scripted", False):
            raise UnsupportedConfig("ScriptedRobot: an env of varying human count (config.sim.human_nums) serves the "
                                    "scripted controllers only with config.sim.human_nums_scripted")

    @classmethod
    def check_rollout(cls, venv, name):
        """check(), and UnsupportedConfig for an env whose observation a rollout cannot record: 'convgru' without
        lidar.live, or an env with config.sim.visible_masks without the opt-in config.sim.visible_masks_scripted, whose
        mask the recorded rows would not carry (before anything touches the GPU)."""
        cls.check(venv, name)
        no_visible_masks(venv.config, "ScriptedRobot.rollout")
        mode = getattr(venv, "obs_mode", "srnn")
        if mode == "convgru":
            lc = venv.config.lidar
            if not (getattr(lc, "live", False) and lc.enable):
                raise UnsupportedConfig("ScriptedRobot.rollout: obs_mode='convgru' needs config.lidar.live (the held "
                                        "per-episode scan is not a function of the recorded state)")
        elif mode != "srnn":
            raise UnsupportedConfig("ScriptedRobot.rollout: obs_mode=%r" % mode)

    def __init__(self, venv, name):
        self.check(venv, name)
        config = venv.config
        self.venv = venv
        self.name = name
        self.base = _ScriptedBase(int(config.sim.human_num))

    def act(self, obs, hxs, masks, deterministic=False):
        """Policy.act's signature and return shape (value, action, log-prob, hidden state). `obs` is not read:
        the engine's state is the state `obs` came from."""
        return None, self.venv.robot_act(self.name), None, hxs

    def rollout(self, T, obs_every_step=True, out=None, noise=None):
        """T closed-loop steps of this controller from the env's current state, every step recorded
        (CrowdNavVecEnv.rollout -> cn_rollout): a dict of (T, E, ...) device tensors -- actions, the observation
        after each step, reward, done, event, info, ep_return, ep_len -- and 'num_launches'. Expert pairs are
        (observation row t-1, actions row t), row -1 being the reset observation.
        `noise` (engine.RolloutNoise or a dict with sigma / seed / step0): noise-injected demonstrations -- the steps
        take actions + sigma * uniform[-1, 1) noise (returned as 'executed'), the labels in 'actions' stay clean.
        On a 'convgru' env with lidar.live the dict also holds 'lidar' (T, E, 1, 7 + beams), the LiDAR observation
        after each step, with the state rows it was scanned from (cn_rollout_lidar); without lidar.live the
        observation carries the scan held since the episode's reset, which no recorded row determines:
        UnsupportedConfig.
        On an env with sim.visible_masks and sim.visible_masks_scripted the dict also holds 'visible_masks' (T, E, N),
        the mask after each step (cn_rollout_masked); without that opt-in: UnsupportedConfig."""
        self.check_rollout(self.venv, self.name)
        return self.venv.rollout(self.name, T, obs_every_step=obs_every_step, out=out, noise=noise)


policy_factory = {"orca": ORCA, "none": none_policy, "social_force": SOCIAL_FORCE, "srnn": SRNN, "convgru": SRNN}
