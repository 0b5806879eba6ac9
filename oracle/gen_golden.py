"""Generate golden vectors from the REFERENCE implementation (run in the build container only).

    python oracle/gen_golden.py [--out tests/golden]

Imports the reference's own code from /root/reference (read-only) through the shims in
oracle/shims (gym, shapely, rvo2, torchvision — see oracle/shims/README.md) and records:

  spawn_*.npz    CrowdSimDict.reset() states for the reference seed schedule
                 (crowd_sim_dict.py:105-203, crowd_sim.py:555-663, 296-393)
  roll_*.npz     teacher-forced step sequences: per step the actions, the post-step state, the
                 observation, reward, done, event, info — with the VecEnv worker's auto-reset
                 (shmem_vec_env.py:164-168) and bench.Monitor's episode return
  *_cfg_*.npz    the same two kinds at non-default numeric settings (config_cases: time step, time limit,
                 geometry, radii / v_pref, goal-change chances, reward constants, ORCA / social-force parameters,
                 norm-zone side and penalty, social thresholds, phase 'test' with a small test_size, seeds);
                 the overrides are stored in the fixture (cfg_meta) and applied by tests/helpers.py
  dsrnn.npz      DSRNN Policy.act / evaluate_actions with procedural weights
                 (pytorchBaselines/a2c_ppo_acktr/model.py:63-104, srnn_model.py:409-504)
  eval_*.npz     pytorchBaselines/evaluation.py evaluate() + metrics.py Metrics driven by a scripted
                 episode stream (stand-in VecEnv / policy objects; the bookkeeping is the reference's)
  lidar_*.npz    CrowdSimDict.reset() with robot.policy = 'convgru' and lidar.enable: post-reset states and
                 the (1, 7 + 180) observation (crowd_sim_dict.py:96-101,170-191; lidarv2.py)
  convgru.npz    ConvGRU Policy.act / evaluate_actions with procedural weights (convgru_model.py, model.py)
  ppo.npz        SRNNRolloutStorage + compute_returns + PPO.update on procedural weights
                 (pytorchBaselines/a2c_ppo_acktr/storage.py:14-292, algo/ppo.py:36-118)
  train_loop.npz train.py:219-330 for one update on real reference envs (act, step with auto-reset,
                 insert, get_value, compute_returns, PPO.update; deterministic actions)

The fixtures are data only (inputs and expected outputs); nothing of the reference's source is
copied. The reference never travels to the GPU box; these .npz files do.
Deviations applied to the reference while recording (each documented in DESIGN.md):
  - unicycle: ActionRot gets vx/vy = commanded world-frame velocity so calc_reward's jerk/speed
    metrics do not raise (crowd_sim.py:1004 reads action.vx);
  - the ORCA frozen-simulator parameters are read back from the rvo2 shim into the state;
  - LiDAR: `np.int` (removed in NumPy 1.24, used at lidarv2.py:251) is aliased to `int` while recording.
"""
import argparse
import math
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
sys.path[:0] = [os.path.join(HERE, "shims"), REF, REPO]

from crowdnav_dsrnn_amd import abi  # noqa: E402
from crowdnav_dsrnn_amd.config import clone_config  # noqa: E402

# ---- reference imports (through the shims) ----
import crowd_sim.envs.utils.action as ref_action  # noqa: E402

_CUR = {"theta": 0.0}


class ActionRotV(ref_action.ActionRot):
    """ActionRot + the commanded world-frame velocity (SURVEY §9-1 patch; metrics only)."""

    @property
    def vx(self):
        th = (self._theta() + self.r) % (2 * np.pi)
        return self.v * np.cos(th)

    @property
    def vy(self):
        th = (self._theta() + self.r) % (2 * np.pi)
        return self.v * np.sin(th)

    def _theta(self):
        return _CUR["theta"]


ref_action.ActionRot = ActionRotV

from crowd_nav.configs.config import Config as RefConfig  # noqa: E402
from crowd_nav.policy import orca as ref_orca  # noqa: E402
from crowd_sim.envs import crowd_sim as ref_crowd_sim  # noqa: E402
from crowd_sim.envs import crowd_sim_dict as ref_csd  # noqa: E402
from crowd_sim.envs.utils import info as ref_info  # noqa: E402

ref_csd.ActionRot = ActionRotV
import crowd_nav.policy.srnn as ref_srnn  # noqa: E402

ref_srnn.ActionRot = ActionRotV

_orig_calc_reward = ref_crowd_sim.CrowdSim.calc_reward


def _calc_reward(self, action):
    _CUR["theta"] = self.robot.theta
    return _orig_calc_reward(self, action)


ref_crowd_sim.CrowdSim.calc_reward = _calc_reward

# record which observed slots were dummies when each human's RVO2 simulator was created
_orig_predict = ref_orca.ORCA.predict


def _predict(self, state):
    creating = self.sim is None
    out = _orig_predict(self, state)
    if creating:
        self.dummy_mask = 0
        for k, hs in enumerate(state.human_states):
            if hs.px == 7 and hs.py == 7 and hs.vx == 0 and hs.vy == 0:
                self.dummy_mask |= 1 << k
    return out


ref_orca.ORCA.predict = _predict

EVENT_CODE = {ref_info.Nothing: 0, ref_info.Danger: 1, ref_info.Collision: 2, ref_info.ReachGoal: 3,
              ref_info.Timeout: 4}


def make_ref_config(kin="holonomic", policy="orca", scenarios=("circle_crossing",), N=5, fov_robot=2.0,
                    fov_human=2.0, side_pref=False, norm_zones=False, social_metrics=False, robot_visible=False,
                    random_radii=False, random_v_pref=False, time_factor=False, time_step=0.25, over=None):
    """`over` maps "section__field" to a value, set after every other argument (the convention of the GPU tests'
    _cfg). discomfort_penalty_factor follows time_step (10 * time_step) unless it is overridden itself. Every
    override is recorded in the fixture (cfg_meta) so that tests/helpers.py rebuilds the same config."""
    c = clone_config(RefConfig())
    c.action_space.kinematics = kin
    c.humans.policy = policy
    c.sim.train_val_sim = list(scenarios)
    c.sim.test_sim = list(scenarios)
    c.sim.human_num = N
    c.robot.FOV = fov_robot
    c.humans.FOV = fov_human
    c.test.side_preference = side_pref
    c.test.social_metrics = social_metrics
    c.robot.visible = robot_visible
    c.humans.random_radii = random_radii
    c.humans.random_v_pref = random_v_pref
    c.reward.time_factor = time_factor
    c.env.time_step = time_step
    c.reward.discomfort_penalty_factor = 10 * time_step
    if side_pref:
        c.sim.circle_radius = 4
        c.humans.random_goal_changing = False
        c.humans.end_goal_changing = False
    c.reward.norm_zones = norm_zones
    c.overrides = dict(over or {})
    for k, v in c.overrides.items():
        sec, fld = k.split("__")
        assert hasattr(getattr(c, sec), fld), k
        setattr(getattr(c, sec), fld, v)
    if "reward__discomfort_penalty_factor" not in c.overrides:
        c.reward.discomfort_penalty_factor = 10 * c.env.time_step
    return c


def default_phase(nenv):
    return "train" if nenv > 1 else "test"


def make_ref_env(cfg, rank, nenv, phase=None, seed=None):
    """Env `rank` of `nenv` as the reference's make_env sets it up (envs.py:66-73): thisSeed = seed + rank
    (seed defaults to config.env.seed), phase 'train' when nenv > 1 unless given."""
    env = ref_csd.CrowdSimDict()
    env.configure(cfg)
    env.rank = rank
    env.thisSeed = (cfg.env.seed if seed is None else seed) + rank
    env.nenv = nenv
    env.phase = default_phase(nenv) if phase is None else phase
    env.ep_ret, env.ep_len = 0.0, 0
    return env


def extract(envs, cfg):
    """Reference env objects -> abi.StateView (every field of include/crowdnav_state.h)."""
    E, N = len(envs), cfg.sim.human_num
    sv = abi.StateView(None, E, N, cfg.robot.visible)
    A = abi.sim_agents(N, cfg.robot.visible)
    for e, env in enumerate(envs):
        r = env.robot
        for f, v in (("r_px", r.px), ("r_py", r.py), ("r_gx", r.gx), ("r_gy", r.gy), ("r_vx", r.vx),
                     ("r_vy", r.vy), ("r_theta", r.theta), ("r_dv", env.desiredVelocity[0]),
                     ("r_radius", r.radius), ("r_vpref", r.v_pref), ("potential", env.potential),
                     ("gtime", env.global_time), ("last_ax", env.last_acceleration[0]),
                     ("last_ay", env.last_acceleration[1]), ("ep_return", env.ep_ret)):
            getattr(sv, f)[e] = float(v)
        sv.case_counter[e] = env.case_counter[env.phase]
        sv.ep_len[e] = env.ep_len
        sv.scenario[e] = abi.SCENARIO_ID[env.current_scenario]
        sv.reset_count[e] = env.scenario_counter
        frozen = cfg.humans.policy == "orca" and env.humans[0].policy.sim is not None
        nan = any(not (math.isfinite(h.px) and math.isfinite(h.py)) for h in env.humans)
        rf32 = isinstance(r.vx, np.float32)
        sv.flags[e] = ((abi.FLAG_ORCA_FROZEN if frozen else 0) | (abi.FLAG_NAN if nan else 0) |
                       (abi.FLAG_ROBOT_F32 if rf32 else 0))
        st = env.rng_state
        sv.mt[e] = st[1]
        sv.mt_pos[e] = st[2]
        for i, h in enumerate(env.humans):
            for f, v in (("h_px", h.px), ("h_py", h.py), ("h_gx", h.gx), ("h_gy", h.gy), ("h_vx", h.vx),
                         ("h_vy", h.vy), ("h_r", h.radius), ("h_vpref", h.v_pref), ("h_theta", h.theta)):
                getattr(sv, f)[e, i] = float(v)
            sv.b_px[e, i], sv.b_py[e, i], sv.b_vx[e, i], sv.b_vy[e, i], sv.b_r[e, i] = env.last_human_states[i]
            if frozen:
                sim = h.policy.sim
                sv.o_r[e, i] = sim.agents[0].radius
                sv.o_vmax[e, i] = sim.agents[0].maxSpeed
                sv.o_dmask[e, i] = h.policy.dummy_mask
                if A > 10:
                    sv.o_perm[e, i * A:(i + 1) * A] = sim.kd_agents
    return sv


# Each reference env owns the process-global np.random stream while it runs (one env per process in
# the reference's ShmemVecEnv); we swap the stream in and out around every call.
_ACTIVE = {"env": None}


class _ScenarioChoice(object):
    """Replaces the unseeded `random.choices` of crowd_sim_dict.py:125 with the engine's deterministic
    assignment (global env index round-robin); identical to the reference for one scenario."""

    @staticmethod
    def choices(seq, weights=None):
        return [seq[_CUR["gidx"] % len(seq)]]


ref_csd.random = _ScenarioChoice


def run_in(env, fn, *a):
    _CUR["gidx"] = getattr(env, "rank", env.thisSeed)
    if getattr(env, "rng_state", None) is not None:
        np.random.set_state(env.rng_state)
    _ACTIVE["env"] = env
    out = fn(*a)
    env.rng_state = np.random.get_state()
    _ACTIVE["env"] = None
    return out


def obs32(ob):
    return (np.asarray(ob["robot_node"], np.float32).reshape(1, 7),
            np.asarray(ob["temporal_edges"], np.float32).reshape(1, 2),
            np.asarray(ob["spatial_edges"], np.float32))


def env_reset(env):
    ob = run_in(env, env.reset)
    env.ep_ret, env.ep_len = 0.0, 0
    return ob


def env_step(env, action):
    a = np.array(action, dtype=np.float32)
    ob, rew, done, info = run_in(env, env.step, a)
    env.ep_ret += rew  # bench.Monitor: sum(self.rewards)
    env.ep_len += 1
    ep = (env.ep_ret, env.ep_len)
    if done:
        ob = env_reset(env)
    return ob, rew, done, info, ep


def info_vec(info, scenario):
    si = info["info"]
    v = np.zeros(abi.INFO_K, np.float32)
    v[abi.INFO_AGG_NAV_TIME] = si["aggregate_nav_time"]
    v[abi.INFO_PATH_VIOLATION] = si["path_violation"]
    v[abi.INFO_PERSONAL_VIOLATION] = si["personal_violation"]
    v[abi.INFO_JERK_COST] = si["jerk_cost"]
    v[abi.INFO_DIST_TO_GOAL] = si["dist_to_goal"]
    v[abi.INFO_SPEED_VIOLATION] = si["speed_violation"]
    ev = si["event"]
    v[abi.INFO_MIN_DIST] = ev.min_dist if isinstance(ev, ref_info.Danger) else np.nan
    v[abi.INFO_SCENARIO] = abi.SCENARIO_ID[si["scenario"]]
    if scenario in si:
        v[abi.INFO_SIDE_LEFT] = si[scenario]["left"]
        v[abi.INFO_SIDE_RIGHT] = si[scenario]["right"]
        v[abi.INFO_SEPARATION] = si["separation"]
    return v, EVENT_CODE[type(ev)]


def cfg_meta(cfg, E, phase=None, seed=None):
    """Fixture metadata. Overrides of make_ref_config(over=...) travel as data: numbers in over_keys / over_vals,
    strings (norm_zone_side) in over_skeys / over_svals; phase, seed and the two case sizes always."""
    over = getattr(cfg, "overrides", {})
    num = sorted(k for k, v in over.items() if not isinstance(v, str))
    txt = sorted(k for k, v in over.items() if isinstance(v, str))
    extra = dict(phase=default_phase(E) if phase is None else phase, seed=int(cfg.env.seed if seed is None else seed),
                 val_size=int(cfg.env.val_size), test_size=int(cfg.env.test_size))
    if over:
        extra.update(over_keys=np.array(num, dtype="U64"), over_vals=np.array([float(over[k]) for k in num], np.float64),
                     over_skeys=np.array(txt, dtype="U64"), over_svals=np.array([over[k] for k in txt], dtype="U64"))
    return dict(extra, kinematics=cfg.action_space.kinematics, policy=cfg.humans.policy, N=cfg.sim.human_num, E=E,
                scenarios=",".join(cfg.sim.train_val_sim), robot_fov=cfg.robot.FOV, human_fov=cfg.humans.FOV,
                side_pref=int(cfg.test.side_preference), norm_zones=int(cfg.reward.norm_zones),
                social_metrics=int(cfg.test.social_metrics), robot_visible=int(cfg.robot.visible),
                random_radii=int(cfg.humans.random_radii), random_v_pref=int(cfg.humans.random_v_pref),
                time_factor=int(cfg.reward.time_factor), time_step=cfg.env.time_step,
                circle_radius=cfg.sim.circle_radius)


def pack_state(sv, prefix, out, with_mt):
    for name, _, _ in abi.STATE_FIELDS:
        if name == "mt" and not with_mt:
            continue
        out[prefix + name] = np.array(getattr(sv, name))
    out[prefix + "mt_crc"] = np.array([zlib.crc32(np.ascontiguousarray(sv.mt[e]).tobytes())
                                       for e in range(sv.E)], np.uint32)


def gen_spawn(name, cfg, E, resets, outdir, phase=None, seed=None):
    nenv = E
    envs = [make_ref_env(cfg, r, nenv, phase, seed) for r in range(E)]
    out = {"meta_" + k: np.array(v) for k, v in cfg_meta(cfg, E, phase, seed).items()}
    for k in range(resets):
        # start from a blank state carrying only the case counters (all the reset reads)
        pre = extract_pre_reset(envs, cfg)
        obs = [obs32(env_reset(env)) for env in envs]
        post = extract(envs, cfg)
        pack_state(pre, "k%d_pre_" % k, out, True)
        pack_state(post, "k%d_post_" % k, out, False)
        out["k%d_robot_node" % k] = np.stack([o[0] for o in obs])
        out["k%d_temporal" % k] = np.stack([o[1] for o in obs])
        out["k%d_spatial" % k] = np.stack([o[2] for o in obs])
    out["resets"] = np.array(resets)
    np.savez_compressed(os.path.join(outdir, "spawn_%s.npz" % name), **out)
    print("spawn", name, "ok")


def extract_pre_reset(envs, cfg):
    E, N = len(envs), cfg.sim.human_num
    sv = abi.StateView(None, E, N, cfg.robot.visible)
    for e, env in enumerate(envs):
        sv.case_counter[e] = env.case_counter[env.phase]
        sv.reset_count[e] = env.scenario_counter
    return sv


def goal_action(env, kin, rng):
    r = env.robot
    dx, dy = r.gx - r.px, r.gy - r.py
    d = math.hypot(dx, dy) + 1e-9
    if kin == "holonomic":
        return np.array([dx / d * 1.2, dy / d * 1.2], np.float32) + rng.normal(0, 0.05, 2).astype(np.float32)
    want = math.atan2(dy, dx)
    dth = (want - r.theta + math.pi) % (2 * math.pi) - math.pi
    return np.array([0.12, np.clip(dth, -0.15, 0.15)], np.float32)


def gen_roll(name, cfg, E, T, outdir, act_seed=1, goal_frac=0.5, phase=None, seed=None):
    """`act_seed` seeds the recorded actions; `phase` / `seed` are the envs' (make_ref_env)."""
    nenv = E
    kin = cfg.action_space.kinematics
    envs = [make_ref_env(cfg, r, nenv, phase, seed) for r in range(E)]
    for env in envs:
        env_reset(env)
    rng = np.random.RandomState(act_seed)
    out = {"meta_" + k: np.array(v) for k, v in cfg_meta(cfg, E, phase, seed).items()}
    pack_state(extract(envs, cfg), "init_", out, True)
    acts = np.zeros((T, E, 2), np.float32)
    keys = ["robot_node", "temporal", "spatial", "reward", "done", "event", "info", "ep_return", "ep_len"]
    rec = {k: [] for k in keys}
    posts = []
    for t in range(T):
        for e, env in enumerate(envs):
            if e < int(E * goal_frac):
                acts[t, e] = goal_action(env, kin, rng)
            elif kin == "holonomic":
                acts[t, e] = rng.normal(0, 0.7, 2).astype(np.float32)
            else:
                acts[t, e] = rng.uniform(-0.15, 0.15, 2).astype(np.float32)
        step_out = []
        for e, env in enumerate(envs):
            sc = env.current_scenario
            ob, rew, done, info, ep = env_step(env, acts[t, e].copy())
            iv, ev = info_vec(info, sc)
            step_out.append((obs32(ob), rew, done, ev, iv, ep))
        rec["robot_node"].append(np.stack([s[0][0] for s in step_out]))
        rec["temporal"].append(np.stack([s[0][1] for s in step_out]))
        rec["spatial"].append(np.stack([s[0][2] for s in step_out]))
        rec["reward"].append(np.array([np.float32(s[1]) for s in step_out], np.float32))
        rec["done"].append(np.array([s[2] for s in step_out], np.uint8))
        rec["event"].append(np.array([s[3] for s in step_out], np.int8))
        rec["info"].append(np.stack([s[4] for s in step_out]))
        rec["ep_return"].append(np.array([s[5][0] for s in step_out], np.float64))
        rec["ep_len"].append(np.array([s[5][1] for s in step_out], np.int32))
        posts.append(extract(envs, cfg))
    out["actions"] = acts
    for k in keys:
        out[k] = np.stack(rec[k])
    for name_, _, _ in abi.STATE_FIELDS:
        if name_ == "mt":
            continue
        out["post_" + name_] = np.stack([np.array(getattr(p, name_)) for p in posts])
    out["post_mt_crc"] = np.stack([np.array([zlib.crc32(np.ascontiguousarray(p.mt[e]).tobytes())
                                             for e in range(E)], np.uint32) for p in posts])
    np.savez_compressed(os.path.join(outdir, "roll_%s.npz" % name), **out)
    ev = out["event"]
    print("roll", name, "events:", {k: int((ev == k).sum()) for k in range(5)}, "dones", int(out["done"].sum()))


# --------------------------------------------------------------------------------------------------
# DSRNN forward vectors (procedural weights)
# --------------------------------------------------------------------------------------------------
def procedural_state_dict(model):
    """Deterministic weights: param p (sorted state_dict order) ~ RandomState(1000 + p).uniform(-s, s),
    s = 1/sqrt(fan_in) (fan_in = last dim, 1 for 1-D params). Reproducible without files."""
    import torch

    sd = model.state_dict()
    out = {}
    for p, k in enumerate(sorted(sd.keys())):
        shape = tuple(sd[k].shape)
        fan_in = shape[-1] if len(shape) > 1 else 1
        s = 1.0 / math.sqrt(fan_in)
        out[k] = torch.from_numpy(np.random.RandomState(1000 + p).uniform(-s, s, shape).astype(np.float32))
    return out


def gen_dsrnn(outdir):
    import torch

    torch.set_num_threads(4)
    from pytorchBaselines.a2c_ppo_acktr.model import Policy

    import gym

    out = {}
    for N in (5, 10, 25):   # N in {5, 10, 25} (25 = C3's spatial-edge width)
        E, T = 4, 8
        cfg = make_ref_config(N=N)
        cfg.training.cuda = False
        cfg.training.num_processes = E
        cfg.ppo.num_steps = T
        cfg.ppo.num_mini_batch = 1
        obs_space = {"robot_node": gym.spaces.Box(-np.inf, np.inf, (1, 7)),
                     "temporal_edges": gym.spaces.Box(-np.inf, np.inf, (1, 2)),
                     "spatial_edges": gym.spaces.Box(-np.inf, np.inf, (N, 2))}
        act_space = gym.spaces.Box(-np.inf, np.inf, (2,))
        act_space.__class__.__name__  # Box
        torch.manual_seed(0)
        pol = Policy(obs_space, act_space, base="srnn", base_kwargs=cfg)
        pol.load_state_dict(procedural_state_dict(pol))
        pol.eval()
        rng = np.random.RandomState(7 + N)
        # act (infer, seq_len 1)
        obs = {"robot_node": rng.normal(0, 3, (E, 1, 7)).astype(np.float32),
               "temporal_edges": rng.normal(0, 0.5, (E, 1, 2)).astype(np.float32),
               "spatial_edges": rng.normal(0, 4, (E, N, 2)).astype(np.float32)}
        hxs = {"human_node_rnn": rng.normal(0, 0.3, (E, 1, 128)).astype(np.float32),
               "human_human_edge_rnn": rng.normal(0, 0.3, (E, N + 1, 256)).astype(np.float32)}
        masks = np.array([[1.0], [0.0], [1.0], [1.0]], np.float32)
        with torch.no_grad():
            t_obs = {k: torch.from_numpy(v) for k, v in obs.items()}
            t_hxs = {k: torch.from_numpy(v.copy()) for k, v in hxs.items()}
            value, action, logp, nh = pol.act(t_obs, t_hxs, torch.from_numpy(masks), deterministic=True)
        p = "N%d_" % N
        for k, v in obs.items():
            out[p + "act_obs_" + k] = v
        for k, v in hxs.items():
            out[p + "act_hxs_" + k] = v
        out[p + "act_masks"] = masks
        out[p + "act_value"] = value.numpy()
        out[p + "act_action"] = action.numpy()
        out[p + "act_logp"] = logp.numpy()
        for k, v in nh.items():
            out[p + "act_new_" + k] = v.numpy()
        # evaluate_actions (training mode: seq T, nenv E with mid-sequence episode starts)
        obs_T = {"robot_node": rng.normal(0, 3, (T * E, 1, 7)).astype(np.float32),
                 "temporal_edges": rng.normal(0, 0.5, (T * E, 1, 2)).astype(np.float32),
                 "spatial_edges": rng.normal(0, 4, (T * E, N, 2)).astype(np.float32)}
        hxs0 = {"human_node_rnn": rng.normal(0, 0.3, (E, 1, 128)).astype(np.float32),
                "human_human_edge_rnn": rng.normal(0, 0.3, (E, N + 1, 256)).astype(np.float32)}
        masks_T = np.ones((T * E, 1), np.float32)
        masks_T[3 * E + 1] = 0.0
        masks_T[5 * E + 2] = 0.0
        masks_T[0 * E + 0] = 0.0
        acts = rng.normal(0, 0.5, (T * E, 2)).astype(np.float32)
        with torch.no_grad():
            v2, lp2, ent, _ = pol.evaluate_actions({k: torch.from_numpy(v) for k, v in obs_T.items()},
                                                   {k: torch.from_numpy(v.copy()) for k, v in hxs0.items()},
                                                   torch.from_numpy(masks_T), torch.from_numpy(acts))
        for k, v in obs_T.items():
            out[p + "ev_obs_" + k] = v
        for k, v in hxs0.items():
            out[p + "ev_hxs_" + k] = v
        out[p + "ev_masks"] = masks_T
        out[p + "ev_actions"] = acts
        out[p + "ev_value"] = v2.numpy()
        out[p + "ev_logp"] = lp2.numpy()
        out[p + "ev_entropy"] = np.array(float(ent))
        out[p + "keys"] = np.array(sorted(pol.state_dict().keys()))
        out[p + "shapes"] = np.array([str(tuple(v.shape)) for k, v in sorted(pol.state_dict().items())])
    np.savez_compressed(os.path.join(outdir, "dsrnn.npz"), **out)
    print("dsrnn ok")


def gen_ppo(outdir):
    """SRNNRolloutStorage.insert / compute_returns / recurrent_generator + PPO.update of the reference
    (pytorchBaselines/a2c_ppo_acktr/storage.py:14-292, algo/ppo.py:36-118) on procedural DSRNN weights:
    inputs, the returns and the parameters after one update (torch RNG seeded before the update, so the
    minibatch permutation is reproducible)."""
    import torch

    torch.set_num_threads(4)
    import gym
    from pytorchBaselines.a2c_ppo_acktr import algo
    from pytorchBaselines.a2c_ppo_acktr.model import Policy
    from pytorchBaselines.a2c_ppo_acktr.storage import SRNNRolloutStorage

    out = {}
    N, E, T = 5, 4, 8
    cfg = make_ref_config(N=N)
    cfg.training.cuda = False
    cfg.training.num_processes = E
    cfg.ppo.num_steps = T
    cfg.ppo.num_mini_batch = 2
    obs_space = {"robot_node": gym.spaces.Box(-np.inf, np.inf, (1, 7)),
                 "temporal_edges": gym.spaces.Box(-np.inf, np.inf, (1, 2)),
                 "spatial_edges": gym.spaces.Box(-np.inf, np.inf, (N, 2))}
    act_space = gym.spaces.Box(-np.inf, np.inf, (2,))
    torch.manual_seed(0)
    pol = Policy(obs_space, act_space, base="srnn", base_kwargs=cfg)
    pol.load_state_dict(procedural_state_dict(pol))
    rol = SRNNRolloutStorage(T, E, obs_space, act_space, 128, 256, recurrent_cell_type="GRU")
    rng = np.random.RandomState(31)

    def rnd(*shape, s=1.0):
        return rng.normal(0, s, shape).astype(np.float32)

    obs0 = {"robot_node": rnd(E, 1, 7, s=3), "temporal_edges": rnd(E, 1, 2, s=0.5), "spatial_edges": rnd(E, N, 2, s=4)}
    for k, v in obs0.items():
        rol.obs[k][0].copy_(torch.from_numpy(v))
        out["obs0_" + k] = v
    ins = []
    for t in range(T):
        d = {"obs_robot_node": rnd(E, 1, 7, s=3), "obs_temporal_edges": rnd(E, 1, 2, s=0.5),
             "obs_spatial_edges": rnd(E, N, 2, s=4),
             "hxs_human_node_rnn": rnd(E, 1, 128, s=0.3), "hxs_human_human_edge_rnn": rnd(E, N + 1, 256, s=0.3),
             "actions": rnd(E, 2, s=0.5), "logp": rnd(E, 1), "values": rnd(E, 1), "rewards": rnd(E, 1),
             "masks": (rng.uniform(size=(E, 1)) > 0.2).astype(np.float32),
             "bad_masks": (rng.uniform(size=(E, 1)) > 0.1).astype(np.float32)}
        rol.insert({k[4:]: torch.from_numpy(d[k]) for k in d if k.startswith("obs_")},
                   {k[4:]: torch.from_numpy(d[k]) for k in d if k.startswith("hxs_")},
                   torch.from_numpy(d["actions"]), torch.from_numpy(d["logp"]), torch.from_numpy(d["values"]),
                   torch.from_numpy(d["rewards"]), torch.from_numpy(d["masks"]), torch.from_numpy(d["bad_masks"]))
        for k, v in d.items():
            out["t%d_%s" % (t, k)] = v
    next_value = rnd(E, 1)
    out["next_value"] = next_value
    rol.compute_returns(torch.from_numpy(next_value), True, 0.99, 0.95, True)
    out["returns_gae_ptl"] = rol.returns.numpy().copy()
    agent = algo.PPO(pol, 0.2, 2, 2, 0.5, 0.01, lr=4e-5, eps=1e-5, max_grad_norm=0.5)
    torch.manual_seed(1234)
    vl, al, de = agent.update(rol)
    out["update_losses"] = np.array([vl, al, de])
    for k, v in pol.state_dict().items():
        out["param_" + k] = v.numpy().copy()
    # the other compute_returns branches on the same data
    for use_gae, ptl, name in ((False, True, "returns_nogae_ptl"), (True, False, "returns_gae"),
                               (False, False, "returns_nogae")):
        rol.compute_returns(torch.from_numpy(next_value), use_gae, 0.99, 0.95, ptl)
        out[name] = rol.returns.numpy().copy()
    np.savez_compressed(os.path.join(outdir, "ppo.npz"), **out)
    print("ppo ok")


def gen_train_loop(outdir, N=5, E=4, T=32, epochs=2):
    """The body of the reference's train.py:219-330 for one update, on real reference envs
    (CrowdSimDict + the VecEnv worker's auto-reset, ORCA humans through the rvo2 stand-in) and the
    reference Policy / SRNNRolloutStorage / PPO on procedural weights: act -> envs.step -> masks ->
    rollouts.insert for num_steps steps, get_value, compute_returns (GAE, proper time limits), one
    PPO.update (num_mini_batch 1: the minibatch permutation then only reorders a mean), after_update.
    Actions are the policy's mode (deterministic=True): train.py samples them from the torch RNG, whose
    stream a device-side sampler cannot reproduce; everything downstream of the action is unchanged."""
    import torch

    torch.set_num_threads(4)
    import gym
    from pytorchBaselines.a2c_ppo_acktr import algo
    from pytorchBaselines.a2c_ppo_acktr.model import Policy
    from pytorchBaselines.a2c_ppo_acktr.storage import SRNNRolloutStorage

    cfg = make_ref_config(N=N)
    cfg.training.cuda = False
    cfg.training.num_processes = E
    cfg.ppo.num_steps = T
    cfg.ppo.num_mini_batch = 1
    cfg.ppo.epoch = epochs
    obs_space = {"robot_node": gym.spaces.Box(-np.inf, np.inf, (1, 7)),
                 "temporal_edges": gym.spaces.Box(-np.inf, np.inf, (1, 2)),
                 "spatial_edges": gym.spaces.Box(-np.inf, np.inf, (N, 2))}
    act_space = gym.spaces.Box(-np.inf, np.inf, (2,))
    torch.manual_seed(0)
    pol = Policy(obs_space, act_space, base="srnn", base_kwargs=cfg)
    pol.load_state_dict(procedural_state_dict(pol))
    envs = [make_ref_env(cfg, r, E) for r in range(E)]
    rol = SRNNRolloutStorage(T, E, obs_space, act_space, 128, 256, recurrent_cell_type="GRU")
    obs = [obs32(env_reset(env)) for env in envs]
    rol.obs["robot_node"][0].copy_(torch.from_numpy(np.stack([o[0] for o in obs])))
    rol.obs["temporal_edges"][0].copy_(torch.from_numpy(np.stack([o[1] for o in obs])))
    rol.obs["spatial_edges"][0].copy_(torch.from_numpy(np.stack([o[2] for o in obs])))
    out = {"meta_" + k: np.array(v) for k, v in cfg_meta(cfg, E).items()}
    out["T"], out["epochs"] = np.array(T), np.array(epochs)
    rec = {k: [] for k in ("action", "value", "logp", "reward", "done", "robot_node", "spatial")}
    for step in range(T):
        with torch.no_grad():
            o_s = {k: rol.obs[k][step] for k in rol.obs}
            h_s = {k: rol.recurrent_hidden_states[k][step] for k in rol.recurrent_hidden_states}
            value, action, logp, hxs = pol.act(o_s, h_s, rol.masks[step], deterministic=True)
        res = [env_step(env, action[e].numpy().copy()) for e, env in enumerate(envs)]
        ob = [obs32(r[0]) for r in res]
        t_obs = {"robot_node": torch.from_numpy(np.stack([o[0] for o in ob])),
                 "temporal_edges": torch.from_numpy(np.stack([o[1] for o in ob])),
                 "spatial_edges": torch.from_numpy(np.stack([o[2] for o in ob]))}
        reward = torch.tensor([[np.float32(r[1])] for r in res], dtype=torch.float32)
        done = [r[2] for r in res]
        masks = torch.FloatTensor([[0.0] if d else [1.0] for d in done])          # train.py:259-260
        bad_masks = torch.FloatTensor([[1.0] for _ in done])                     # no 'bad_transition'
        rol.insert(t_obs, hxs, action, logp, value, reward, masks, bad_masks)
        rec["action"].append(action.numpy().copy())
        rec["value"].append(value.numpy().copy())
        rec["logp"].append(logp.numpy().copy())
        rec["reward"].append(reward.numpy().copy())
        rec["done"].append(np.array(done, np.uint8))
        rec["robot_node"].append(t_obs["robot_node"].numpy().copy())
        rec["spatial"].append(t_obs["spatial_edges"].numpy().copy())
    with torch.no_grad():
        next_value = pol.get_value({k: rol.obs[k][-1] for k in rol.obs},
                                   {k: rol.recurrent_hidden_states[k][-1] for k in rol.recurrent_hidden_states},
                                   rol.masks[-1]).detach()
    rol.compute_returns(next_value, cfg.ppo.use_gae, cfg.reward.gamma, cfg.ppo.gae_lambda,
                        cfg.training.use_proper_time_limits)
    out["returns"] = rol.returns.numpy().copy()
    agent = algo.PPO(pol, cfg.ppo.clip_param, epochs, 1, cfg.ppo.value_loss_coef, cfg.ppo.entropy_coef,
                     lr=cfg.training.lr, eps=cfg.training.eps, max_grad_norm=cfg.training.max_grad_norm)
    torch.manual_seed(99)
    vl, al, de = agent.update(rol)
    rol.after_update()
    out["update_losses"] = np.array([vl, al, de])
    for k, v in rec.items():
        out[k] = np.stack(v)
    for k, v in pol.state_dict().items():
        out["param_" + k] = v.numpy().copy()
    for k, v in rol.recurrent_hidden_states.items():
        out["hxs0_after_" + k] = v[0].numpy().copy()
    out["hparams"] = np.array([cfg.ppo.clip_param, cfg.ppo.value_loss_coef, cfg.ppo.entropy_coef, cfg.training.lr,
                               cfg.training.eps, cfg.training.max_grad_norm, cfg.reward.gamma, cfg.ppo.gae_lambda,
                               float(cfg.ppo.use_gae), float(cfg.training.use_proper_time_limits)])
    np.savez_compressed(os.path.join(outdir, "train_loop.npz"), **out)
    print("train_loop ok: dones", int(out["done"].sum()), "losses", out["update_losses"])


def gen_lidar(name, cfg, E, resets, outdir):
    """Post-reset states + ConvGRU observations of the reference (LiDAR scan at reset)."""
    if not hasattr(np, "int"):
        np.int = int   # lidarv2.py:251 (np.int was removed in NumPy 1.24)
    cfg.robot.policy = "convgru"
    cfg.lidar.enable = True
    envs = [make_ref_env(cfg, r, E) for r in range(E)]
    out = {"meta_" + k: np.array(v) for k, v in cfg_meta(cfg, E).items()}
    out["meta_max_range"] = np.array(float(cfg.lidar.cfg["max_range"]))
    out["meta_num_beams"] = np.array(int(cfg.lidar.cfg["num_beams"]))
    out["meta_lidar_robot_radius"] = np.array(float(cfg.lidar.cfg["robot_radius"]))
    for k in range(resets):
        obs = [np.asarray(env_reset(env), np.float32).reshape(1, -1) for env in envs]
        pack_state(extract(envs, cfg), "k%d_post_" % k, out, True)
        out["k%d_obs" % k] = np.stack(obs)
    out["resets"] = np.array(resets)
    np.savez_compressed(os.path.join(outdir, "lidar_%s.npz" % name), **out)
    print("lidar", name, "ok")


def gen_convgru(outdir):
    """ConvGRU policy (pytorchBaselines/a2c_ppo_acktr/convgru_model.py + model.py) on procedural weights:
    act (one step, E envs) and evaluate_actions (T steps x E envs, episode starts inside)."""
    import torch

    torch.set_num_threads(4)
    import gym
    from pytorchBaselines.a2c_ppo_acktr.model import Policy

    E, T, B = 5, 4, 180
    cfg = make_ref_config(N=5)
    cfg.robot.policy = "convgru"
    obs_space = gym.spaces.Box(-np.inf, np.inf, (1, 7 + B))
    act_space = gym.spaces.Box(-np.inf, np.inf, (2,))
    torch.manual_seed(0)
    pol = Policy(obs_space, act_space, base="convgru", base_kwargs=cfg)
    pol.load_state_dict(procedural_state_dict(pol))
    pol.srnn = False
    rng = np.random.RandomState(17)
    out = {"state_dict_keys": np.array(sorted(pol.state_dict().keys()))}
    obs = rng.uniform(0, 1, (E, 1, 7 + B)).astype(np.float32)
    hxs = (rng.normal(0, 0.5, (E, 256))).astype(np.float32)
    masks = np.array([[1.0], [0.0], [1.0], [1.0], [0.0]], np.float32)
    with torch.no_grad():
        v, a, lp, h = pol.act(torch.from_numpy(obs), torch.from_numpy(hxs), torch.from_numpy(masks), deterministic=True)
    out.update(act_obs=obs, act_hxs=hxs, act_masks=masks, act_value=v.numpy(), act_action=a.numpy(),
               act_logp=lp.numpy(), act_hxs_out=h.numpy())
    obs_t = rng.uniform(0, 1, (T * E, 1, 7 + B)).astype(np.float32)
    m_t = np.ones((T * E, 1), np.float32)
    m_t[[0, 7, 13]] = 0.0
    acts = rng.normal(0, 1, (T * E, 2)).astype(np.float32)
    v, lp, ent, h = pol.evaluate_actions(torch.from_numpy(obs_t), torch.from_numpy(hxs), torch.from_numpy(m_t),
                                         torch.from_numpy(acts))
    out.update(ev_obs=obs_t, ev_masks=m_t, ev_actions=acts, ev_value=v.detach().numpy(),
               ev_logp=lp.detach().numpy(), ev_entropy=np.float32(ent.item()), ev_hxs_out=h.detach().numpy())
    np.savez_compressed(os.path.join(outdir, "convgru.npz"), **out)
    print("convgru ok")


def gen_rollout_storage(outdir):
    """RolloutStorage (storage.py:295-508, the ConvGRU buffer): inserts, the four compute_returns branches
    and the recurrent / feed-forward minibatches for seeded torch permutations."""
    import torch

    import gym
    from pytorchBaselines.a2c_ppo_acktr.storage import RolloutStorage

    T, E, D, H = 6, 4, 10, 8
    rng = np.random.RandomState(23)
    out = {}
    r = lambda *s: rng.normal(0, 1, s).astype(np.float32)  # noqa: E731
    seq = {"obs0": r(E, 1, D)}
    for t in range(T):
        seq["t%d" % t] = dict(obs=r(E, 1, D), hxs=r(E, H), act=r(E, 2), logp=r(E, 1), val=r(E, 1), rew=r(E, 1),
                             masks=(rng.rand(E, 1) > 0.3).astype(np.float32),
                             bad=(rng.rand(E, 1) > 0.2).astype(np.float32))
    nv = r(E, 1)
    out["obs0"] = seq["obs0"]
    out["next_value"] = nv
    for t in range(T):
        for k, v in seq["t%d" % t].items():
            out["t%d_%s" % (t, k)] = v

    def filled():
        st = RolloutStorage(T, E, (1, D), gym.spaces.Box(-np.inf, np.inf, (2,)), H)
        st.obs[0].copy_(torch.from_numpy(seq["obs0"]))
        for t in range(T):
            g = seq["t%d" % t]
            st.insert(*[torch.from_numpy(g[k]) for k in ("obs", "hxs", "act", "logp", "val", "rew", "masks", "bad")])
        return st

    for gae in (True, False):
        for ptl in (True, False):
            st = filled()
            st.compute_returns(torch.from_numpy(nv), gae, 0.99, 0.95, ptl)
            out["returns_%d%d" % (gae, ptl)] = st.returns.numpy().copy()
    st = filled()
    adv = torch.from_numpy(r(T, E, 1))
    out["adv"] = adv.numpy()
    torch.manual_seed(5)
    for i, b in enumerate(st.recurrent_generator(adv, 2)):
        for j, x in enumerate(b):
            out["rec%d_%d" % (i, j)] = x.numpy().copy()
    torch.manual_seed(6)
    for i, b in enumerate(st.feed_forward_generator(adv, 3)):
        for j, x in enumerate(b):
            out["ff%d_%d" % (i, j)] = x.numpy().copy()
    st.after_update()
    out["after_obs0"] = st.obs[0].numpy().copy()
    out["after_hxs0"] = st.recurrent_hidden_states[0].numpy().copy()
    np.savez_compressed(os.path.join(outdir, "rollout_storage.npz"), **out)
    print("rollout_storage ok")


EVAL_SCEN = ("circle_crossing", "square_crossing", "parallel_traffic")


def make_eval_script(n_ep, seed, scenarios, side_scenario=None, max_len=25):
    """A synthetic test-episode stream in the VecEnv's step format (float32 obs / reward / info values):
    per episode a spawn (reset obs, zero velocity) and per step the post-step robot position / velocity,
    reward, event code, info fields. Terminal events cycle through success / collision / timeout."""
    rng = np.random.RandomState(seed)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    eps = []
    for k in range(n_ep):
        L = int(rng.randint(1, max_len + 1))
        first = rng.uniform(-6, 6, 2).astype(np.float32)
        term = [abi.EV_REACHGOAL, abi.EV_COLLISION, abi.EV_TIMEOUT][int(rng.randint(3)) if k > 2 else k]
        scen = scenarios[int(rng.randint(len(scenarios)))] if side_scenario is None else side_scenario
        pos = first.copy()
        steps = []
        for t in range(L):
            pos = (pos + rng.uniform(-0.3, 0.3, 2)).astype(np.float32)
            vel = rng.uniform(-1, 1, 2).astype(np.float32)
            ev = term if t == L - 1 else (abi.EV_DANGER if rng.rand() < 0.25 else abi.EV_NOTHING)
            st = {"pos": pos.copy(), "vel": vel, "reward": f32(rng.normal()), "event": ev,
                  "min_dist": f32(rng.uniform(0, 0.25)),
                  "aggregate_nav_time": int(rng.randint(0, 3)), "path_violation": int(rng.randint(0, 3)),
                  "personal_violation": int(rng.rand() < 0.3), "jerk_cost": f32(rng.uniform(0, 2)) * (rng.rand() < 0.7),
                  "dist_to_goal": f32(rng.uniform(0, 9)) * (rng.rand() < 0.9),
                  "speed_violation": int(rng.rand() < 0.2), "left": int(rng.rand() < 0.4),
                  "right": int(rng.rand() < 0.4)}
            steps.append(st)
        eps.append({"first": first, "scenario": scen, "steps": steps})
    return eps


def run_ref_evaluate(cfg, eps):
    """Drive pytorchBaselines/evaluation.py:evaluate (1 env, sequential episodes) over the script with
    stand-in env / policy objects; returns (log lines, raw_rewards, discounted_rewards, dist_to_goal)."""
    import contextlib
    import io

    import torch
    from crowd_sim.envs.utils import info as ref_info
    from pytorchBaselines.evaluation import evaluate as ref_evaluate

    dt = cfg.env.time_step
    side = cfg.test.side_preference
    ev_cls = {abi.EV_NOTHING: lambda d: ref_info.Nothing(), abi.EV_DANGER: lambda d: ref_info.Danger(d),
              abi.EV_COLLISION: lambda d: ref_info.Collision(), abi.EV_REACHGOAL: lambda d: ref_info.ReachGoal(),
              abi.EV_TIMEOUT: lambda d: ref_info.Timeout()}

    def obs_of(pos, vel):
        rn = torch.zeros(1, 1, 7)
        rn[0, 0, 0], rn[0, 0, 1] = float(pos[0]), float(pos[1])
        te = torch.tensor([[[float(vel[0]), float(vel[1])]]], dtype=torch.float32)
        return {"robot_node": rn, "temporal_edges": te, "spatial_edges": torch.zeros(1, 1, 2)}

    class Robot:
        time_step = dt
        v_pref = cfg.robot.v_pref

    class BaseEnv:
        time_step = dt
        time_limit = cfg.env.time_limit
        robot = Robot()
        global_time = 0.0

    class Envs:
        def __init__(self):
            self.base = BaseEnv()
            self.venv = type("V", (), {})()
            self.venv.envs = [type("M", (), {"env": self.base})()]
            self.k, self.t = 0, 0

        def reset(self):
            e = eps[0]
            return obs_of(e["first"], (0.0, 0.0))

        def step(self, action):
            e = eps[self.k % len(eps)]
            st = e["steps"][self.t]
            self.t += 1
            done = self.t == len(e["steps"])
            si = {"aggregate_nav_time": st["aggregate_nav_time"], "path_violation": st["path_violation"]}
            if side:
                si[e["scenario"]] = {"left": st["left"], "right": st["right"]}
            si.update(personal_violation=st["personal_violation"], jerk_cost=st["jerk_cost"],
                      dist_to_goal=st["dist_to_goal"], speed_violation=st["speed_violation"],
                      scenario=e["scenario"], event=ev_cls[st["event"]](st["min_dist"]))
            self.base.global_time += dt
            if done:
                self.k += 1
                self.t = 0
                self.base.global_time = 0.0
                nxt = eps[self.k % len(eps)]
                ob = obs_of(nxt["first"], (0.0, 0.0))
            else:
                ob = obs_of(st["pos"], st["vel"])
            return ob, torch.tensor([[st["reward"]]], dtype=torch.float32), np.array([done]), ({"info": si},)

        def close(self):
            pass

    class Pol:
        base = type("B", (), {"human_num": 1})()

        def act(self, obs, hxs, masks, deterministic=False):
            return None, torch.zeros(1, 2), None, hxs

    class Log:
        lines = []

        def info(self, msg):
            self.lines.append(str(msg))

    log = Log()
    log.lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        raw, disc, d2g = ref_evaluate(Pol(), False, Envs(), 1, "cpu", cfg, log)
    return log.lines, raw, disc, d2g


def pack_eval_script(eps, out):
    names = sorted(set(e["scenario"] for e in eps))
    out["ep_len"] = np.array([len(e["steps"]) for e in eps], np.int32)
    out["ep_first"] = np.stack([e["first"] for e in eps]).astype(np.float32)
    out["ep_scenario"] = np.array([e["scenario"] for e in eps])
    cat = lambda key, dt: np.array([st[key] for e in eps for st in e["steps"]], dt)  # noqa: E731
    out["st_pos"] = np.stack([st["pos"] for e in eps for st in e["steps"]]).astype(np.float32)
    out["st_vel"] = np.stack([st["vel"] for e in eps for st in e["steps"]]).astype(np.float32)
    for key, dt in (("reward", np.float32), ("event", np.int8), ("min_dist", np.float32),
                    ("aggregate_nav_time", np.int32), ("path_violation", np.int32),
                    ("personal_violation", np.int32), ("jerk_cost", np.float32), ("dist_to_goal", np.float32),
                    ("speed_violation", np.int32), ("left", np.int32), ("right", np.int32)):
        out["st_" + key] = cat(key, dt)
    return names


def gen_eval(outdir):
    """evaluate() golden logs / returns for two configurations (social metrics; side preference)."""
    cases = [("eval_social", dict(scenarios=EVAL_SCEN, social_metrics=True), 16, None),
             ("eval_sidepref", dict(scenarios=("side_pref_passing",), side_pref=True, N=1), 12, "side_pref_passing")]
    for name, kw, n_ep, side_scen in cases:
        cfg = make_ref_config(**kw)
        cfg.env.test_size = n_ep
        eps = make_eval_script(n_ep, 7 + n_ep, list(kw["scenarios"]), side_scen)
        lines, raw, disc, d2g = run_ref_evaluate(cfg, eps)
        out = {}
        pack_eval_script(eps, out)
        out["log"] = np.array("\n".join(lines))
        out["test_size"] = np.int32(n_ep)
        out["time_step"] = np.float64(cfg.env.time_step)
        out["time_limit"] = np.float64(cfg.env.time_limit)
        out["social_metrics"] = np.int32(cfg.test.social_metrics)
        out["side_preference"] = np.int32(cfg.test.side_preference)
        out["train_val_sim"] = np.array(cfg.sim.train_val_sim)
        out["test_sim"] = np.array(cfg.sim.test_sim)
        for tag, d in (("raw", raw), ("disc", disc), ("d2g", d2g)):
            for b, lists in d.items():
                out["ret_%s_%s_len" % (tag, b)] = np.array([len(x) for x in lists], np.int32)
                out["ret_%s_%s" % (tag, b)] = np.array([v for x in lists for v in x], np.float64)
        np.savez_compressed(os.path.join(outdir, name + ".npz"), **out)
        print("eval", name, len(lines), "log lines")


def config_cases():
    """Non-default numeric settings (roll_cfg_* / spawn_cfg_*): name -> (make_ref_config kwargs, E, T, spawn
    resets, phase). Every field varied here is read by the engine's step, reset or spawn kernels; the fixtures
    carry the overrides as data (cfg_meta). test_wrap: 4 envs on test_size 5, so the case counter runs
    0, 4, 3, 2, 1 over the spawn fixture's five resets."""
    K = dict
    return [
        ("ts01", K(N=5, over={"env__time_step": 0.1}), 6, 60, 2, None),
        ("ts04_uni", K(kin="unicycle", N=6, over={"env__time_step": 0.4}), 6, 40, 2, None),
        ("tl7", K(N=3, over={"env__time_limit": 7}), 4, 60, 2, None),
        ("radius35_uni", K(kin="unicycle", N=5, over={"sim__circle_radius": 3.5}), 6, 40, 2, None),
        ("sq31", K(N=12, scenarios=("square_crossing",), over={"sim__square_width": 31}), 4, 40, 2, None),
        ("rr045", K(over={"robot__radius": 0.45, "robot__v_pref": 0.7}), 6, 60, 2, None),
        ("hum", K(N=6, over={"humans__radius": 0.22, "humans__v_pref": 1.4, "env__randomize_attributes": False}),
         6, 60, 2, None),
        ("goalchg", K(over={"humans__goal_change_chance": 0.7, "humans__end_goal_change_chance": 0.4}), 6, 60, 2, None),
        ("rewards", K(over={"reward__success_reward": 3.5, "reward__collision_penalty": -7.25,
                            "reward__potential_factor": 0.75, "reward__discomfort_penalty_factor": 1.3,
                            "sim__circle_radius": 4}), 6, 60, 2, None),
        ("disc06", K(over={"reward__discomfort_dist_front": 0.6, "reward__discomfort_dist_back": 0.6}), 6, 60, 2, None),
        ("orca", K(N=9, over={"orca__neighbor_dist": 3, "orca__safety_space": 0.05, "orca__time_horizon": 2}),
         4, 60, 2, None),
        ("sf", K(policy="social_force", N=6, over={"sf__A": 3.5, "sf__B": 0.6, "sf__KI": 2.5}), 6, 60, 2, None),
        ("nz_rhs", K(norm_zones=True, scenarios=("parallel_traffic", "perpendicular_traffic"),
                     over={"reward__norm_zone_side": "rhs", "reward__norm_zone_penalty": -1.25}), 4, 40, 2, None),
        ("social", K(over={"social__min_personal_space": 0.5, "social__max_walking_speed": 0.7}), 6, 60, 2, None),
        ("test_wrap", K(over={"env__test_size": 5, "env__seed": 77, "env__time_limit": 4}), 4, 60, 5, "test"),
        ("seed_train", K(over={"env__seed": 123456789, "env__time_limit": 4}), 4, 60, 2, None),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    only = set(args.only.split(",")) if args.only else None

    def want(n):
        return only is None or n in only

    spawn_cases = [
        ("holo_circle_N5", make_ref_config(N=5), 8),
        ("holo_circle_N10", make_ref_config(N=10), 8),
        ("uni_circle_N10", make_ref_config(kin="unicycle", N=10), 8),
        ("holo_square_N10", make_ref_config(N=10, scenarios=("square_crossing",)), 8),
        ("holo_parallel_N5", make_ref_config(N=5, scenarios=("parallel_traffic",)), 8),
        ("holo_perp_N5", make_ref_config(N=5, scenarios=("perpendicular_traffic",)), 8),
        ("side_pref_N1", make_ref_config(N=1, side_pref=True, scenarios=(
            "side_pref_passing", "side_pref_overtaking", "side_pref_crossing")), 3),
        ("uni_square_N12", make_ref_config(kin="unicycle", N=12, scenarios=("square_crossing",)), 6),
    ]
    for name, cfg, E in spawn_cases:
        if want("spawn_" + name):
            gen_spawn(name, cfg, E, 2, args.out)

    roll_cases = [
        ("holo_orca_circle_N5", make_ref_config(N=5), 8, 60),
        ("uni_orca_circle_N10", make_ref_config(kin="unicycle", N=10), 6, 60),
        ("holo_sf_circle_N5", make_ref_config(policy="social_force", N=5), 6, 60),
        ("uni_sf_circle_N5", make_ref_config(kin="unicycle", policy="social_force", N=5), 4, 40),
        ("holo_orca_square_fov_N12", make_ref_config(N=12, scenarios=("square_crossing",), fov_robot=1.0,
                                                     fov_human=1.0), 4, 40),
        ("uni_orca_square_fov_N8", make_ref_config(kin="unicycle", N=8, scenarios=("square_crossing",),
                                                    fov_robot=1.0, fov_human=1.0), 4, 40),
        ("holo_orca_parallel_N5", make_ref_config(N=5, scenarios=("parallel_traffic",)), 4, 40),
        ("holo_orca_perp_N5", make_ref_config(N=5, scenarios=("perpendicular_traffic",)), 4, 40),
        ("holo_orca_sidepref_N1", make_ref_config(N=1, side_pref=True, scenarios=(
            "side_pref_passing", "side_pref_overtaking", "side_pref_crossing")), 3, 40),
        ("holo_orca_normzone_N5", make_ref_config(N=5, norm_zones=True), 4, 40),
        ("holo_orca_visible_N5", make_ref_config(N=5, robot_visible=True, random_radii=True,
                                                 random_v_pref=True, time_factor=True), 4, 60),
        ("holo_orca_timeout_N3", make_ref_config(N=3), 2, 200),
    ]
    import signal

    def _alarm(signum, frame):
        raise TimeoutError("reference did not finish (unbounded rejection loop, SURVEY §9-2)")

    signal.signal(signal.SIGALRM, _alarm)
    for name, cfg, E, T in roll_cases:
        if want("roll_" + name):
            signal.alarm(400)
            try:
                gen_roll(name, cfg, E, T, args.out, goal_frac=0.0 if "timeout" in name else 0.5)
            except TimeoutError as ex:
                print("roll", name, "SKIPPED:", ex)
            signal.alarm(0)
    for name, kw, E, T, resets, phase in config_cases():
        for kind in ("spawn", "roll"):
            if not want("%s_cfg_%s" % (kind, name)):
                continue
            signal.alarm(400)
            try:
                if kind == "spawn":
                    gen_spawn("cfg_" + name, make_ref_config(**kw), E, resets, args.out, phase=phase)
                else:
                    gen_roll("cfg_" + name, make_ref_config(**kw), E, T, args.out, phase=phase)
            except TimeoutError as ex:
                print(kind, name, "SKIPPED:", ex)
            signal.alarm(0)
    if want("dsrnn"):
        gen_dsrnn(args.out)
    if want("ppo"):
        gen_ppo(args.out)
    if want("train_loop"):
        gen_train_loop(args.out)
    if want("eval"):
        gen_eval(args.out)
    def _radius(c, r):
        c.sim.circle_radius = r
        return c

    lidar_cases = [("circle_N5_r7", _radius(make_ref_config(N=5), 7.0), 16, 3),
                   ("circle_N10_r6", _radius(make_ref_config(N=10), 6.0), 16, 3),
                   ("square_N8_unicycle", make_ref_config(kin="unicycle", N=8, scenarios=("square_crossing",)), 12, 3),
                   ("circle_N1_r8", _radius(make_ref_config(N=1), 8.0), 16, 4)]
    for name, cfg, E, R in lidar_cases:
        if want("lidar_" + name):
            gen_lidar(name, cfg, E, R, args.out)
    if want("convgru"):
        gen_convgru(args.out)
    if want("rollout_storage"):
        gen_rollout_storage(args.out)


if __name__ == "__main__":
    main()
