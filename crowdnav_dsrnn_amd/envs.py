"""VecEnv drop-in for the reference's environment stack, backed by the batched HIP engine.

Reference stack this replaces:
    gym.make('CrowdSimDict-v0')                      crowd_sim/__init__.py:9-11
    make_env / make_vec_envs                         pytorchBaselines/a2c_ppo_acktr/envs.py:33-156
    bench.Monitor (episode r/l/t)                    baselines (external), consumed at train.py:266-267
    ShmemVecEnv / DummyVecEnv (auto-reset)           pytorchBaselines/a2c_ppo_acktr/shmem_vec_env.py:89-168
    VecPyTorch (torch obs, (E,1) reward)             pytorchBaselines/a2c_ppo_acktr/envs.py:208-239

`make_vec_envs(...)` keeps the reference signature and returns a `CrowdNavVecEnv` whose reset/step have
VecPyTorch's return types:
    reset()      -> {'robot_node' (E,1,7), 'temporal_edges' (E,1,2), 'spatial_edges' (E,N,2)} float32 on `device`
    step(action) -> obs dict on `device`, reward (E,1) float32 CPU tensor, done np.ndarray bool (E,),
                    infos: a tuple-like of E dicts {'info': step_info[, 'episode': {r, l, t}]}, built lazily
                    on access from the engine's event codes and metrics (events are info.py instances)
With config.sim.human_nums (a list of human counts; this project's opt-in) the envs differ in crowd size inside one
mixed engine: spatial_edges is padded to the largest count and the dict gains 'detected_human_num' (E,1), each env's
own count; `venv.config` is then a clone of the caller's config whose sim.human_num is that largest count.
With config.sim.visible_masks (this project's opt-in as well) the dict gains 'visible_masks' (E,N) float32: 1.0 for the
humans the robot sees in the state the observation describes (the step's own FOV decisions, one cn_visible_mask launch).
All env work runs on the GPU in one cn_step launch pair; there is no per-env Python and no CPU fallback.
`step_device(actions)` is the zero-copy variant for on-device rollouts (no host sync).

Sharding: `shard=(rank, world)` makes this process own the contiguous env block
[rank*E/world, (rank+1)*E/world) of the `num_processes` global envs, with the reference's global seed
schedule (thisSeed = seed + global index, nenv = num_processes), so a sharded run steps exactly the envs
an unsharded run would.
"""
import time

import numpy as np

from . import abi, info as info_mod, spaces
from .config import (UnsupportedConfig, clone_config, make_cn_config, make_varied_cn_configs, no_visible_masks,
                     varied_human_nums, visible_masks_on, visible_masks_scripted)

_REGISTRY = {}


def register(id, entry_point):  # noqa: A002 - gym's keyword name
    """gym.envs.registration.register equivalent (crowd_sim/__init__.py:9-11): `entry_point` is a
    "module:Class" string (or the class) of a batched env with CrowdNavVecEnv's constructor; make_vec_envs
    resolves it like gym.make does. When gym itself is importable the id is registered there too, so
    `gym.spec(id)` / `gym.envs.registry` list it as the reference's registration does."""
    _REGISTRY[id] = entry_point
    try:
        import gym  # noqa: F401  (absent in this image; optional)
        from gym.envs.registration import register as gym_register
    except Exception:
        return
    try:
        gym_register(id=id, entry_point=entry_point)
    except Exception:   # already registered
        pass


def registry():
    return dict(_REGISTRY)


def resolve(env_name):
    """The registered entry point of `env_name` as a class (gym's load("module:attr"))."""
    if env_name not in _REGISTRY:
        raise KeyError("No registered env with id: %s (registered: %s)" % (env_name, sorted(_REGISTRY)))
    ep = _REGISTRY[env_name]
    if not isinstance(ep, str):
        return ep
    import importlib

    mod, _, attr = ep.partition(":")
    obj = importlib.import_module(mod)
    for a in attr.split("."):
        obj = getattr(obj, a)
    return obj


register("CrowdSimDict-v0", "crowdnav_dsrnn_amd.envs:CrowdNavVecEnv")


def make_vec_envs(env_name, seed, num_processes, gamma, log_dir, device, allow_early_resets,
                  num_frame_stack=None, config=None, ax=None, test_case=-1, fig=None, shard=None,
                  engine_device=None):
    """envs.py:106-156. `gamma` / `log_dir` are accepted for signature compatibility (VecNormalize only
    wraps Box observations, the Monitor writes no file: envs.py:79,141-146). `ax` / `fig` select the
    matplotlib rendering path, which is out of scope and rejected."""
    env_cls = resolve(env_name)
    if config is None:
        raise ValueError("config is required (CrowdSim.configure(config), envs.py:65)")
    if ax is not None or fig is not None:
        raise NotImplementedError("rendering (render_axis / render_figure / test_case) is out of scope")
    if num_frame_stack is not None:
        raise NotImplementedError("frame stacking applies to image observations only")
    rank, world = shard if shard is not None else (0, 1)
    if num_processes % world != 0:
        raise ValueError("num_processes=%d does not split over %d shards" % (num_processes, world))
    E = num_processes // world
    return env_cls(config, E, seed, device, allow_early_resets=allow_early_resets,
                   env_offset=rank * E, nenv=num_processes, engine_device=engine_device)


def _no_varied(config, what):
    """UnsupportedConfig for what an env of varying human count serves only with the opt-in
    config.sim.human_nums_scripted (read from the config alone)."""
    if getattr(config.sim, "human_nums", None) is not None and not getattr(config.sim, "human_nums_scripted", False):
        raise UnsupportedConfig("%s: not served on an env of varying human count (config.sim.human_nums) unless "
                                "config.sim.human_nums_scripted is set" % what)


class _LazyInfos:
    """Tuple-like of E info dicts, each built on first access (train.py iterates them; most callers only
    read a few). Holds host copies of the step's event codes / metrics / Monitor counters."""

    def __init__(self, venv, event, done, info, ep_return, ep_len, t):
        self._v, self._event, self._done, self._info = venv, event, done, info
        self._ep_return, self._ep_len, self._t = ep_return, ep_len, t
        self._cache = [None] * len(event)

    def __len__(self):
        return len(self._cache)

    def _build(self, i):
        v, row = self._v, self._info[i]
        sc = v.scenario_names[int(row[abi.INFO_SCENARIO])]
        si = {"aggregate_nav_time": int(row[abi.INFO_AGG_NAV_TIME]),
              "path_violation": int(row[abi.INFO_PATH_VIOLATION])}
        if v.side_preference:
            si[sc] = {"left": int(row[abi.INFO_SIDE_LEFT]), "right": int(row[abi.INFO_SIDE_RIGHT])}
            si["separation"] = float(row[abi.INFO_SEPARATION])
        si["personal_violation"] = int(row[abi.INFO_PERSONAL_VIOLATION])
        si["jerk_cost"] = float(row[abi.INFO_JERK_COST])
        si["dist_to_goal"] = float(row[abi.INFO_DIST_TO_GOAL])
        si["speed_violation"] = int(row[abi.INFO_SPEED_VIOLATION])
        si["scenario"] = sc
        si["event"] = info_mod.make_event(int(self._event[i]), row[abi.INFO_MIN_DIST])
        d = {"info": si}
        if self._done[i]:
            d["episode"] = {"r": round(float(self._ep_return[i]), 6), "l": int(self._ep_len[i]), "t": self._t}
        return d

    def __getitem__(self, i):
        if isinstance(i, slice):
            return tuple(self[j] for j in range(*i.indices(len(self))))
        if i < 0:
            i += len(self)
        if self._cache[i] is None:
            self._cache[i] = self._build(i)
        return self._cache[i]

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


class _RobotView:
    """Read-only view of env i's robot (Agent attributes read by evaluation.py:206,284)."""

    def __init__(self, env):
        self._env = env

    def _s(self, name):
        return float(getattr(self._env._venv._state(), name)[self._env._i])

    time_step = property(lambda self: self._env.time_step)
    v_pref = property(lambda self: self._s("r_vpref"))
    radius = property(lambda self: self._s("r_radius"))
    px = property(lambda self: self._s("r_px"))
    py = property(lambda self: self._s("r_py"))
    gx = property(lambda self: self._s("r_gx"))
    gy = property(lambda self: self._s("r_gy"))
    vx = property(lambda self: self._s("r_vx"))
    vy = property(lambda self: self._s("r_vy"))
    theta = property(lambda self: self._s("r_theta"))

    @property
    def kinematics(self):
        return self._env._venv.config.action_space.kinematics


class _EnvView:
    """Stands in for `venv.envs[i].env` (the CrowdSimDict behind the Monitor; evaluation.py:71-251)."""

    def __init__(self, venv, i):
        self._venv, self._i = venv, i
        self.robot = _RobotView(self)

    @property
    def env(self):  # Monitor.env -> the CrowdSimDict
        return self

    global_time = property(lambda self: float(self._venv._state().gtime[self._i]))
    time_step = property(lambda self: float(self._venv.config.env.time_step))
    time_limit = property(lambda self: float(self._venv.config.env.time_limit))
    human_num = property(lambda self: int(self._venv.env_human_nums[self._i]))
    thisSeed = property(lambda self: int(self._venv.cn_cfg.seed + self._venv.cn_cfg.env_offset + self._i))
    nenv = property(lambda self: int(self._venv.cn_cfg.nenv))
    phase = property(lambda self: self._venv.phase)

    @property
    def current_scenario(self):
        return self._venv.scenario_names[int(self._venv._state().scenario[self._i])]

    def render(self, *a, **k):
        raise NotImplementedError("rendering is out of scope")

    render_traj = render


class _VecView:
    def __init__(self, venv):
        self.envs = [_EnvView(venv, i) for i in range(venv.num_envs)]
        self.num_envs = venv.num_envs


class CrowdNavVecEnv:
    """E CrowdSimDict envs on one GPU with VecPyTorch/ShmemVecEnv/Monitor semantics."""

    def __init__(self, config, num_envs, seed, device, allow_early_resets=False, env_offset=0, nenv=None,
                 engine_device=None, phase=None):
        import torch

        from .engine import CrowdNavEngine

        self.torch = torch
        self.config = config
        self.num_envs = int(num_envs)
        nenv = self.num_envs if nenv is None else int(nenv)
        self.phase = phase if phase is not None else ("train" if nenv > 1 else "test")
        seed = seed if seed is not None else config.env.seed
        # sim.human_nums: envs of varying human count in one mixed engine (UnsupportedConfig, e.g. with 'convgru',
        # before anything touches the GPU); self.config is then a clone whose sim.human_num is the largest count
        # (what a Policy over this env's padded observation is built with), the caller's config stays as it is
        self.human_nums = varied_human_nums(config)
        # sim.visible_masks: the observation also carries 'visible_masks' (UnsupportedConfig with 'convgru')
        self.visible_masks = visible_masks_on(config)
        visible_masks_scripted(config)   # (UnsupportedConfig when set without sim.visible_masks)
        mixed = None
        if self.human_nums is not None:
            mixed = make_varied_cn_configs(config, self.human_nums, self.num_envs, env_offset=env_offset, nenv=nenv,
                                           phase=self.phase, seed=seed)
            self.config = clone_config(config)
            self.config.sim.human_num = max(self.human_nums)
            self.cn_cfg = mixed[0][0]
            self.env_human_nums = [self.human_nums[(env_offset + r) % len(self.human_nums)]
                                   for r in range(self.num_envs)]
        else:
            self.cn_cfg = make_cn_config(config, num_envs=self.num_envs, env_offset=env_offset, nenv=nenv,
                                         phase=self.phase, seed=seed)
            self.env_human_nums = [int(config.sim.human_num)] * self.num_envs
        self.device = torch.device(device)
        if engine_device is None and self.device.type == "cuda":
            engine_device = self.device
        # robot.scripted_unicycle: the scripted controllers serve unicycle kinematics (the engine's opt-in)
        uni = bool(getattr(config.robot, "scripted_unicycle", False))
        # robot.scripted_dwa (True, or a dict of parameter overrides): the engine's policy 'dwa', unicycle only
        dwa = getattr(config.robot, "scripted_dwa", None) or None
        if dwa is not None and config.action_space.kinematics != "unicycle":
            raise UnsupportedConfig("config.robot.scripted_dwa: the dynamic-window controller emits the unicycle "
                                    "action (action_space.kinematics=%r)" % config.action_space.kinematics)
        if mixed is not None:
            self.engine = CrowdNavEngine.mixed(mixed[0], mixed[1], engine_device,
                                               scripted=bool(getattr(config.sim, "human_nums_scripted", False)),
                                               scripted_unicycle=uni, scripted_dwa=dwa)
            assert self.engine.env_humans.tolist() == self.env_human_nums
            # the observation's 'detected_human_num': constant over the env's life, (E, 1) float32 on the engine's GPU
            self._detected = self.engine.env_humans.to(torch.float32).reshape(self.num_envs, 1)
        else:
            self.engine = CrowdNavEngine(self.cn_cfg, engine_device, scripted_unicycle=uni, scripted_dwa=dwa)
        # 'convgru' observation (crowd_sim_dict.py:57-62, 96-101): robot state + the episode's LiDAR scan (or the
        # live one)
        self.obs_mode = "convgru" if getattr(config.robot, "policy", "srnn") == "convgru" else "srnn"
        if self.obs_mode == "convgru":
            lc = dict(config.lidar.cfg)
            self._lidar_cfg = dict(enable=bool(config.lidar.enable), beams=int(lc["num_beams"]),
                                   max_range=float(lc["max_range"]), robot_radius=float(lc["robot_radius"]))
            # lidar.live: the scan of the current state at every reset / step (cn_lidar_scan) instead of the
            # reference's held per-episode scan; only with lidar.enable
            self._lidar_live = bool(getattr(config.lidar, "live", False)) and self._lidar_cfg["enable"]
            B = self._lidar_cfg["beams"]
            self.observation_space = spaces.lidar_observation_space(B)
            self._lidar = torch.zeros((self.num_envs, B), dtype=torch.float32, device=self.engine.device)
            self._lidar_obs = torch.zeros((self.num_envs, 1, 7 + B), dtype=torch.float32, device=self.engine.device)
        else:
            self.observation_space = spaces.observation_space(int(self.config.sim.human_num),
                                                              detected_human_num=mixed is not None,
                                                              visible_masks=self.visible_masks)
        self.action_space = spaces.action_space()
        self.scenario_names = list(abi.SCENARIOS)
        self.side_preference = bool(config.test.side_preference)
        self.allow_early_resets = allow_early_resets
        self.venv = _VecView(self)
        self._tstart = time.time()
        self._was_reset = False
        self._state_cache = None
        self._pending = None
        E = self.num_envs
        pin = dict(pin_memory=True)
        self._h_reward = torch.empty((E,), dtype=torch.float32, **pin)
        self._h_done = torch.empty((E,), dtype=torch.uint8, **pin)
        self._h_event = torch.empty((E,), dtype=torch.int8, **pin)
        self._h_info = torch.empty((E, abi.INFO_K), dtype=torch.float32, **pin)
        self._h_epr = torch.empty((E,), dtype=torch.float64, **pin)
        self._h_epl = torch.empty((E,), dtype=torch.int32, **pin)

    # ---- VecEnv API --------------------------------------------------------------------------
    def _obs_out(self, o):
        if isinstance(o, dict):
            return {k: v.to(self.device, copy=True) for k, v in o.items()}
        return o.to(self.device, copy=True)

    def _srnn_extras(self, o):
        """The 'srnn' observation with this env's opt-in keys: 'detected_human_num' (sim.human_nums) and
        'visible_masks' (sim.visible_masks: one cn_visible_mask launch on the state the observation describes, (E, N)
        float32 in a buffer the engine owns). Without either the dict is returned as it is."""
        if self.human_nums is not None:
            o = dict(o, detected_human_num=self._detected)
        if self.visible_masks:
            o = dict(o, visible_masks=self.engine.visible_mask())
        return o

    def _convgru_obs(self, reset_mask):
        if self._lidar_live:
            c = self._lidar_cfg
            return self.engine.lidar_scan(self._lidar_obs, c["beams"], c["max_range"], c["robot_radius"])
        return self.engine.lidar_obs(self._lidar_obs, self._lidar, reset_mask, **self._lidar_cfg)

    def reset(self):
        """VecPyTorch.reset (envs.py:215-222). Monitor forbids a second reset of a running episode
        unless allow_early_resets (baselines bench.Monitor.reset)."""
        if self._was_reset and not self.allow_early_resets:
            raise RuntimeError("Tried to reset an environment before done. If you want to allow early resets, "
                               "wrap your env with Monitor(env, path, allow_early_resets=True)")
        self._was_reset = True
        self._state_cache = None
        o = self.engine.reset()
        if self.obs_mode == "convgru":
            o = self._convgru_obs(None)
        else:
            o = self._srnn_extras(o)
        return self._obs_out(o)

    def step_async(self, actions):
        self._pending = actions

    def step_wait(self):
        if self._pending is None:
            raise RuntimeError("step_wait() without step_async()")
        actions, self._pending = self._pending, None
        obs, rew, done, ev, info, epr, epl = self.step_device(actions)
        t = self.torch
        for h, d in ((self._h_reward, rew), (self._h_done, done), (self._h_event, ev), (self._h_info, info),
                     (self._h_epr, epr), (self._h_epl, epl)):
            h.copy_(d, non_blocking=True)
        out_obs = self._obs_out(obs)
        t.cuda.current_stream(self.engine.device).synchronize()
        reward = self._h_reward.clone().unsqueeze(1)
        done_np = self._h_done.numpy().astype(bool)
        infos = _LazyInfos(self, self._h_event.numpy().copy(), done_np, self._h_info.numpy().copy(),
                           self._h_epr.numpy().copy(), self._h_epl.numpy().copy(),
                           round(time.time() - self._tstart, 6))
        return out_obs, reward, done_np, infos

    def step(self, actions):
        """VecPyTorch.step (envs.py:224-239) over CrowdSimDict.step + auto-reset + Monitor."""
        self.step_async(actions)
        return self.step_wait()

    def step_device(self, actions):
        """Zero-copy device step: actions (E,2) tensor/array -> the engine's output buffers
        (obs dict, reward (E,) f32, done (E,) u8, event (E,) i8, info (E,K) f32, ep_return f64, ep_len i32),
        all on the engine's GPU, valid until the next call. No host synchronisation."""
        t = self.torch
        if not isinstance(actions, t.Tensor):
            actions = t.as_tensor(np.asarray(actions, dtype=np.float32))
        self._state_cache = None
        out = self.engine.step(actions.reshape(self.num_envs, 2))
        if self.obs_mode == "convgru":
            out = (self._convgru_obs(out[2]),) + tuple(out[1:])
        elif self.human_nums is not None or self.visible_masks:
            out = (self._srnn_extras(out[0]),) + tuple(out[1:])
        return out

    def robot_act(self, policy, regret=None):
        """The scripted robot's action ('orca' / 'social_force') for the state the last reset / step returned:
        (E, 2) float32 on the engine's GPU (CrowdNavEngine.robot_act; no host synchronisation). An env of varying
        human count (sim.human_nums) with sim.human_nums_scripted: every env by the controller of its own count;
        without that opt-in: UnsupportedConfig. A unicycle env with robot.scripted_unicycle: the unicycle action
        (dv, dtheta) the tracking law derives from the controller's velocity, what step_device takes; without that
        opt-in the engine refuses. 'dwa': a unicycle env with robot.scripted_dwa (the dynamic-window controller's own
        unicycle action); without that opt-in the engine refuses it as an unknown policy.
        regret: an (E, 64) float32 tensor on the engine's GPU for the controller's regret rows ('dwa' only;
        CrowdNavEngine.robot_act), written by the same launch."""
        _no_varied(self.config, "robot_act")
        if regret is None:
            return self.engine.robot_act(policy)
        return self.engine.robot_act(policy, regret=regret)

    def robot_mix(self, policy, learner, ctl, t, label=None, executed=None, flags=None, regret=None):
        """The learner in the loop (CrowdNavEngine.robot_mix -> cn_robot_mix): robot_act(policy) of the state the last
        reset / step returned as `label`, and per env a coin of probability beta -- the device block `ctl`
        (engine.mix_ctl() / set_mix_ctl) -- that makes `executed` the label or the `learner`'s (E, 2) action, what
        step_device then takes. Returns (label, executed, flags); no host synchronisation. The envs it serves are
        robot_act's: the same opt-ins, the same UnsupportedConfig on an env of varying human count without
        sim.human_nums_scripted. regret: robot_act's, the expert's regret rows beside its labels ('dwa' only)."""
        _no_varied(self.config, "robot_mix")
        if regret is None:
            return self.engine.robot_mix(policy, learner, ctl, t, label=label, executed=executed, flags=flags)
        return self.engine.robot_mix(policy, learner, ctl, t, label=label, executed=executed, flags=flags, regret=regret)

    def rollout(self, policy, T, obs_every_step=True, out=None, noise=None):
        """T closed-loop steps of the scripted robot ('orca' / 'social_force') from the state the last reset / step
        left, every step recorded (CrowdNavEngine.rollout: a dict of (T, E, ...) tensors on the engine's GPU, no
        host synchronisation). `noise`: the engine's RolloutNoise (or a dict) -- the steps take perturbed actions,
        'actions' keeps the clean labels and 'executed' holds what was taken.
        obs_mode 'convgru' with lidar.live: the dict also holds 'lidar' (T, E, 1, 7 + beams), the observation
        step_device would have returned after every step, and the state rows it was scanned from (the engine's
        rollout with the env's LiDAR settings). Without lidar.live the observation carries the scan held since the
        episode's reset, which is state between steps and no function of a recorded row: UnsupportedConfig.
        An env of varying human count (sim.human_nums) with sim.human_nums_scripted: spatial_edges is padded as the
        env's observation is and the dict gains 'detected_human_num' (T, E, 1), an expanded view of the env's constant
        (E, 1) tensor; without that opt-in: UnsupportedConfig.
        A unicycle env with robot.scripted_unicycle: 'actions' holds unicycle actions (dv, dtheta), each within
        [-0.1, 0.1], and the noise sigma is in those action units (0.1 is the whole range); without that opt-in the
        engine refuses. 'dwa' (a unicycle env with robot.scripted_dwa) likewise, always as launch pairs.
        An env with sim.visible_masks and sim.visible_masks_scripted: the dict gains 'visible_masks' (T, E, N), the
        mask step_device would have returned after every step ((E, N) without obs_every_step: the last step's),
        recorded by the rollout's own launches (the engine's rollout with mask=True; `out` may bring the tensor);
        without that opt-in: UnsupportedConfig (the recorded rows would carry no mask)."""
        _no_varied(self.config, "rollout")
        mask = no_visible_masks(self.config, "rollout")
        lidar = None
        if self.obs_mode == "convgru":
            if not self._lidar_live:
                raise UnsupportedConfig("rollout: obs_mode='convgru' needs config.lidar.live (the held per-episode "
                                        "scan of the parity mode is not a function of the recorded state)")
            c = self._lidar_cfg
            lidar = dict(beams=c["beams"], max_range=c["max_range"], robot_radius=c["robot_radius"])
        elif self.obs_mode != "srnn":
            raise UnsupportedConfig("rollout: obs_mode=%r" % self.obs_mode)
        self._state_cache = None
        if lidar is None:
            ro = self.engine.rollout(policy, T, obs_every_step=obs_every_step, out=out, noise=noise, mask=mask)
            if self.human_nums is not None:
                d = self._detected
                ro["detected_human_num"] = d.unsqueeze(0).expand(int(T), -1, -1) if obs_every_step else d
            return ro
        return self.engine.rollout(policy, T, obs_every_step=obs_every_step, out=out, noise=noise, lidar=lidar)

    def _state(self):
        if self._state_cache is None:
            self._state_cache = self.engine.get_state()
        return self._state_cache

    def render(self, *a, **k):
        raise NotImplementedError("rendering is out of scope")

    def render_traj(self, *a, **k):
        raise NotImplementedError("rendering is out of scope")

    def close(self):
        self.engine.close()

    @property
    def unwrapped(self):
        return self
