"""Device-resident batched CrowdSimDict engine (torch tensors in, torch tensors out).

Thin host wrapper over the C ABI (include/crowdnav.h, crowdnav_dsrnn_amd/csrc/engine/host_api.h): it
owns the output buffers (torch, on the engine's device) and passes `data_ptr()`s and the current
torch stream to `cn_reset` / `cn_step`. No compute happens here and there is no CPU fallback.
"""
import ctypes
import dataclasses
import math

import numpy as np

from . import _lib, abi


@dataclasses.dataclass(frozen=True)
class RolloutNoise:
    """The perturbation of a rollout with noise (cn_rollout_noise): the executed action is the scripted robot's
    plus sigma * n, n uniform in [-1, 1) per component; step0 is the index of the call's first step in the caller's
    noise sequence (a chunked rollout continues it: step0 += T). sigma is in the units of the action: m/s on a
    holonomic engine; on a unicycle engine (scripted_unicycle) the action is (dv, dtheta) and 0.1 is its whole range."""
    sigma: float
    seed: int = 0
    step0: int = 0

    def __post_init__(self):
        s = float(self.sigma)
        if not (math.isfinite(s) and s >= 0.0):
            raise ValueError("RolloutNoise: a finite sigma >= 0 required, got %r" % (self.sigma,))
        object.__setattr__(self, "sigma", s)
        object.__setattr__(self, "seed", int(self.seed))
        object.__setattr__(self, "step0", int(self.step0))

    @classmethod
    def of(cls, noise):
        """None, a RolloutNoise, or a dict with sigma and optionally seed / step0."""
        if noise is None or isinstance(noise, cls):
            return noise
        if isinstance(noise, dict):
            extra = set(noise) - {"sigma", "seed", "step0"}
            if extra or "sigma" not in noise:
                raise ValueError("rollout noise: a dict with sigma and optionally seed / step0, got keys %s"
                                 % sorted(noise))
            return cls(**noise)
        raise TypeError("rollout noise: None, a RolloutNoise or a dict, got %r" % type(noise).__name__)


class CrowdNavEngine:
    """E environments of the reference's CrowdSimDict on one GPU.

    reset()                  -> obs dict (robot_node (E,1,7), temporal_edges (E,1,2), spatial_edges (E,N,2))
    step(actions (E,2) f32)  -> obs, reward (E,), done (E,) uint8, event (E,) int8, info (E,K), ep_return (E,) f64,
                                ep_len (E,) i32       (auto-reset of finished envs, like the reference VecEnv)
    Returned tensors are the engine's own buffers (overwritten by the next call); clone to keep them.
    """

    def __init__(self, cfg, device=None, _mixed=None, scripted_unicycle=False, scripted_dwa=None):
        """scripted_unicycle=True (cn_scripted_unicycle; see scripted_unicycle()): robot_act and rollout serve this
        engine when its kinematics is unicycle. Off, the default, they refuse a unicycle engine as before.
        scripted_dwa=True or a dict of parameter overrides (cn_scripted_dwa; see scripted_dwa()): robot_act and
        rollout take the policy 'dwa' on this unicycle engine. None, the default: 'dwa' is refused as an unknown
        policy."""
        import torch

        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("CrowdNavEngine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        L = _lib.lib()
        h = ctypes.c_void_p()
        if _mixed is None:
            self.cfg = cfg.copy()
            self.groups = None
            self.E, self.N = int(cfg.num_envs), int(cfg.human_num)
            _lib.check(L.cn_config_validate(ctypes.byref(self.cfg)))
            with torch.cuda.device(self.device):
                _lib.check(L.cn_create(ctypes.byref(self.cfg), self.device.index, ctypes.byref(h)))
        else:
            cfgs, env_group, scripted = _mixed
            arr = (abi.CnConfig * len(cfgs))(*[c.copy() for c in cfgs])
            for c in arr:
                if c.num_envs > 0:
                    _lib.check(L.cn_config_validate(ctypes.byref(c)))
            eg = np.ascontiguousarray(env_group, dtype=np.int32)
            self.E, self.N = int(eg.size), max(int(c.human_num) for c in cfgs)
            with torch.cuda.device(self.device):
                _lib.check(L.cn_create_mixed(arr, len(cfgs), eg.ctypes.data_as(ctypes.c_void_p), self.E,
                                             self.device.index, ctypes.byref(h)))
                if scripted:
                    _lib.check(L.cn_mixed_scripted(h, 1))
            self.cfg = arr[0].copy()
            self.groups = [(arr[g], np.nonzero(eg == g)[0].astype(np.int32)) for g in range(len(cfgs))
                           if (eg == g).any()]
        self._h = h
        if scripted_unicycle:
            self.scripted_unicycle(True)
        if scripted_dwa is not None and scripted_dwa is not False:
            self.scripted_dwa(scripted_dwa)
        nb = ctypes.c_int64()
        _lib.check(L.cn_state_bytes(h, ctypes.byref(nb)))
        self.state_bytes = nb.value
        E, N, dev = self.E, self.N, self.device
        hn = np.zeros(E, np.int32)
        _lib.check(L.cn_env_humans(h, hn.ctypes.data_as(ctypes.c_void_p)))
        self.env_humans = torch.from_numpy(hn).to(dev)            # (E,) humans of each env
        self.human_mask = torch.arange(N, device=dev)[None, :] < self.env_humans[:, None]   # (E, N) real slots
        self.robot_node = torch.zeros((E, 1, 7), dtype=torch.float32, device=dev)
        self.temporal_edges = torch.zeros((E, 1, 2), dtype=torch.float32, device=dev)
        self.spatial_edges = torch.zeros((E, N, 2), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((E,), dtype=torch.float32, device=dev)
        self.done = torch.zeros((E,), dtype=torch.uint8, device=dev)
        self.event = torch.zeros((E,), dtype=torch.int8, device=dev)
        self.info = torch.zeros((E, abi.INFO_K), dtype=torch.float32, device=dev)
        self.ep_return = torch.zeros((E,), dtype=torch.float64, device=dev)
        self.ep_len = torch.zeros((E,), dtype=torch.int32, device=dev)
        self.robot_actions = torch.zeros((E, 2), dtype=torch.float32, device=dev)   # robot_act()'s own output
        self._step_args = None   # cached output pointers of step() (the buffers above are never reallocated)
        self._seq_fn = None
        self._visible = None     # visible_mask()'s own output, allocated at its first call
        self.seq_chunk = 32   # steps per multi-step launch (the library's CN_SEQ_CHUNK, csrc/engine/plan.h; set_seq_chunk)

    @classmethod
    def mixed(cls, cfgs, env_group, device=None, scripted=False, scripted_unicycle=False, scripted_dwa=None):
        """One engine over envs of several configurations (cn_create_mixed): env r runs
        cfgs[env_group[r]] (its own human count, scenarios, radius, ...). N = the largest human count;
        spatial_edges rows past an env's own count are padding (`human_mask` False): a never-seen human
        at the reference's unseen-belief position (15, 15). Build the configs with
        config.make_mixed_cn_configs.
        scripted=True (cn_mixed_scripted; holonomic groups): robot_act and rollout (with noise=, mask=) serve this engine,
        every group on its own stream by the rule of a plain engine of its count. Off, the default, they refuse a
        mixed engine as before. step_seq needs no opt-in; rollout(lidar=) and graph mode are never served.
        scripted_unicycle=True (cn_scripted_unicycle) on top of scripted=True: unicycle groups are served as well.
        scripted_dwa (cn_scripted_dwa) on top of scripted=True, every group unicycle: the policy 'dwa' as well."""
        return cls(None, device, _mixed=(list(cfgs), env_group, bool(scripted)), scripted_unicycle=scripted_unicycle,
                   scripted_dwa=scripted_dwa)

    def scripted_unicycle(self, on=True):
        """cn_scripted_unicycle: with on, robot_act and rollout (noise=, lidar= included) serve unicycle kinematics.
        The controller's velocity (ux, uy) then goes through the tracking law of include/crowdnav.h
        (policy_factory.unicycle_track restates it) on the device, and 'actions' holds the unicycle action
        (dv, dtheta) that step() takes, both within [-0.1, 0.1]. A rollout's noise sigma is in those action units:
        0.1 is the whole range. Off: a unicycle engine is refused as before. A holonomic engine is not affected."""
        _lib.check(_lib.lib().cn_scripted_unicycle(self._h, int(bool(on))))

    def scripted_dwa(self, params=True):
        """cn_scripted_dwa: robot_act and rollout (noise=, lidar= included) take the policy 'dwa' on this unicycle
        engine, the dynamic-window controller of include/crowdnav.h (policy_factory.dwa_predict restates it), with
        policy_factory.DWA_DEFAULTS (True) or those with a dict's overrides. It emits the unicycle action (dv, dtheta)
        itself, so scripted_unicycle is not needed for it. None / False: off again -- 'dwa' is refused as an unknown
        policy, as before. A holonomic engine refuses the opt-in."""
        from .policy_factory import dwa_params

        if params is None or params is False:
            _lib.check(_lib.lib().cn_scripted_dwa(self._h, None))
            return
        p = abi.DwaParams(**dwa_params(params))
        _lib.check(_lib.lib().cn_scripted_dwa(self._h, ctypes.byref(p)))

    def dwa_predict(self, self_state, v, others, time_step, params=None, costs=True):
        """cn_dwa_predict on device tensors: self_state (n, 9) f64 (px, py, vx, vy, radius, gx, gy, v_pref, theta),
        v (n,) f64 (the robot's speed, r_dv), others (n, M, 5) f64; returns (actions (n, 2) f32, choice (n,) i32,
        costs (n, 64) f64 or None). One launch on the current stream, no host sync."""
        from .policy_factory import dwa_params

        t = self.torch
        n = int(self_state.shape[0])
        M = int(others.shape[1]) if others is not None and others.numel() else 0
        for name, x, want in (("self_state", self_state, n * 9), ("v", v, n), ("others", others, n * M * 5)):
            if x is None and want == 0:
                continue
            if x.dtype != t.float64 or x.device != self.device or not x.is_contiguous() or x.numel() != want:
                raise ValueError("dwa_predict: %s must be a contiguous float64 tensor of %d elements on %s"
                                 % (name, want, self.device))
        p = abi.DwaParams(**dwa_params(params))
        act = t.zeros((n, 2), dtype=t.float32, device=self.device)
        ch = t.zeros((n,), dtype=t.int32, device=self.device)
        co = t.zeros((n, 64), dtype=t.float64, device=self.device) if costs else None
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().cn_dwa_predict(self._stream(), n, M, self_state.data_ptr(), v.data_ptr(),
                                                 others.data_ptr() if M else None, float(time_step), ctypes.byref(p),
                                                 act.data_ptr(), ch.data_ptr(), co.data_ptr() if costs else None))
        return act, ch, co

    # -------------------------------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def obs(self):
        return {"robot_node": self.robot_node, "temporal_edges": self.temporal_edges,
                "spatial_edges": self.spatial_edges}

    def reset(self):
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().cn_reset(self._h, self._stream(), self.robot_node.data_ptr(),
                                           self.temporal_edges.data_ptr(), self.spatial_edges.data_ptr()))
        return self.obs()

    def step(self, actions):
        t = self.torch
        if actions.device != self.device or actions.dtype != t.float32 or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=t.float32).contiguous()
        if actions.numel() != self.E * 2:
            raise ValueError("actions must have E*2 = %d elements, got %d" % (self.E * 2, actions.numel()))
        # host cost per call matters when a short window starts on an idle GPU: the output pointers and the
        # bound C function are cached, and the device guard is entered only when another device is current
        if self._step_args is None:
            self.step_args()
        if t.cuda.current_device() == self.device.index:
            rc = self._step_fn(self._h, t.cuda.current_stream().cuda_stream, actions.data_ptr(), *self._step_args)
        else:
            with t.cuda.device(self.device):
                rc = self._step_fn(self._h, t.cuda.current_stream().cuda_stream, actions.data_ptr(), *self._step_args)
        _lib.check(rc)
        return self.obs(), self.reward, self.done, self.event, self.info, self.ep_return, self.ep_len

    def step_seq(self, actions):
        """T steps with actions (T, E, 2) f32 (a contiguous device tensor; views along T are fine) issued back to
        back from native code (cn_step_seq); returns the outputs of the last step, like step()."""
        t = self.torch
        if actions.device != self.device or actions.dtype != t.float32 or actions.dim() != 3:
            raise ValueError("step_seq: actions must be a float32 (T, E, 2) tensor on %s" % self.device)
        T = actions.shape[0]
        if tuple(actions.shape[1:]) != (self.E, 2) or actions.stride(2) != 1 or actions.stride(1) != 2:
            raise ValueError("step_seq: actions (T, E, 2) with each step's (E, 2) rows contiguous required")
        if self._step_args is None:
            self.step_args()
        if self._seq_fn is None:
            self._seq_fn = _lib.lib().cn_step_seq
        stride = actions.stride(0) if T > 1 else 2 * self.E
        if t.cuda.current_device() == self.device.index:
            rc = self._seq_fn(self._h, t.cuda.current_stream().cuda_stream, T, actions.data_ptr(), stride, *self._step_args)
        else:
            with t.cuda.device(self.device):
                rc = self._seq_fn(self._h, t.cuda.current_stream().cuda_stream, T, actions.data_ptr(), stride,
                                  *self._step_args)
        _lib.check(rc)
        return self.obs(), self.reward, self.done, self.event, self.info, self.ep_return, self.ep_len

    def step_args(self):
        """The output pointers of step() / step_seq() (cached: the buffers are never reallocated)."""
        if self._step_args is None:
            self._step_fn = _lib.lib().cn_step
            self._step_args = (self.robot_node.data_ptr(), self.temporal_edges.data_ptr(),
                               self.spatial_edges.data_ptr(), self.reward.data_ptr(), self.done.data_ptr(),
                               self.event.data_ptr(), self.info.data_ptr(), self.ep_return.data_ptr(),
                               self.ep_len.data_ptr())
        return self._step_args

    def set_graph_mode(self, on=True):
        """cn_set_graph_mode: keep the step sequence on the device so that step() can be captured in a
        torch.cuda.CUDAGraph (synchronises the current stream)."""
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().cn_set_graph_mode(self._h, self._stream(), int(bool(on))))

    # -------------------------------------------------------------------------------------------
    def lidar_obs(self, out, lidar, reset_mask=None, enable=True, beams=180, max_range=5.0, robot_radius=0.3):
        """The ConvGRU observation (cn_lidar_obs) into out (E,1,7+beams) f32; lidar (E,beams) f32 holds the
        per-episode scans and is refreshed where reset_mask (E,) u8 is set (None = every env)."""
        t = self.torch
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().cn_lidar_obs(self._h, self._stream(),
                                               None if reset_mask is None else reset_mask.data_ptr(),
                                               int(bool(enable)), int(beams), float(max_range), float(robot_radius),
                                               lidar.data_ptr(), out.data_ptr()))
        return out

    def lidar_scan(self, out, beams=180, max_range=5.0, robot_radius=0.3):
        """The live ConvGRU observation (cn_lidar_scan) into out (E,1,7+beams) f32: the scan of the engine's
        current state — all humans and the walls, heading along the robot's velocity. No host sync."""
        t = self.torch
        if (out.dtype != t.float32 or out.device != self.device or not out.is_contiguous()
                or out.numel() != self.E * (7 + int(beams))):
            raise ValueError("lidar_scan: out must be a contiguous float32 (E, 1, 7 + beams) tensor on %s" % self.device)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().cn_lidar_scan(self._h, self._stream(), int(beams), float(max_range),
                                                float(robot_radius), out.data_ptr()))
        return out

    def visible_mask(self, out=None):
        """Which humans the robot sees in the engine's current state (cn_visible_mask): (E, N) float32 on the device,
        1.0 where the step (or the reset) that wrote the state found human i of env e visible, 0.0 otherwise and in
        the padded slots of a mixed engine. Into `out` when given, else into a buffer the engine owns (overwritten by
        the next call). One launch (a mixed engine: one per group), no host sync."""
        t = self.torch
        if out is None:
            if self._visible is None:
                self._visible = t.zeros((self.E, self.N), dtype=t.float32, device=self.device)
            out = self._visible
        elif (out.dtype != t.float32 or out.device != self.device or not out.is_contiguous()
                or out.numel() != self.E * self.N):
            raise ValueError("visible_mask: out must be a contiguous float32 (E, N) tensor on %s" % self.device)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().cn_visible_mask(self._h, self._stream(), out.data_ptr()))
        return out

    ROBOT_POLICIES = {"orca": abi.ROBOT_ORCA, "social_force": abi.ROBOT_SOCIAL_FORCE, "dwa": abi.ROBOT_DWA}   # CN_ROBOT_*

    def _regret_arg(self, who, regret):
        """robot_act's / robot_mix's `regret`: a contiguous float32 (E, 64) tensor on the engine's device."""
        t = self.torch
        if (not isinstance(regret, t.Tensor) or regret.dtype != t.float32 or regret.device != self.device
                or not regret.is_contiguous() or regret.numel() != self.E * 64):
            raise ValueError("%s: regret must be a contiguous float32 (E, 64) tensor on %s" % (who, self.device))
        return regret

    def robot_act(self, policy, out=None, regret=None):
        """The scripted robot's action for the engine's current state (cn_robot_act): (E, 2) float32 on the
        device, what a fresh policy_factory['orca' | 'social_force'] object predicts from the robot's state and
        its belief of the humans ('dwa', after scripted_dwa: what policy_factory.dwa_predict chooses for them). Into `out` when given, else into a buffer the engine owns (overwritten by the
        next call). One launch, no host sync.
        regret: an (E, 64) float32 tensor that receives, beside the action, the controller's regret row of every env
        (cn_robot_act_regret; policy_factory.dwa_regret restates it): (float)(J_c - J_best) of the 64 candidates, 0 at
        the choice. 'dwa' only -- the other two controllers have no candidate set and the engine refuses them. The
        same single launch; the action is the one robot_act('dwa') writes, bit for bit."""
        t = self.torch
        if policy not in self.ROBOT_POLICIES:
            raise ValueError("robot_act: policy %r (one of %s)" % (policy, sorted(self.ROBOT_POLICIES)))
        if out is None:
            out = self.robot_actions
        elif (out.dtype != t.float32 or out.device != self.device or not out.is_contiguous()
                or out.numel() != self.E * 2):
            raise ValueError("robot_act: out must be a contiguous float32 (E, 2) tensor on %s" % self.device)
        if regret is not None:
            self._regret_arg("robot_act", regret)
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().cn_robot_act_regret(self._h, self._stream(), self.ROBOT_POLICIES[policy],
                                                          out.data_ptr(), regret.data_ptr()))
            return out
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().cn_robot_act(self._h, self._stream(), self.ROBOT_POLICIES[policy], out.data_ptr()))
        return out

    def mix_ctl(self):
        """A fresh 16-byte device block for robot_mix (cn_mix_ctl: beta, seed, step0), zeroed: beta 0, the learner
        alone. Fill it with set_mix_ctl."""
        return self.torch.zeros((16,), dtype=self.torch.uint8, device=self.device)

    def _is_mix_ctl(self, ctl):
        t = self.torch
        return (isinstance(ctl, t.Tensor) and ctl.dtype == t.uint8 and ctl.device == self.device
                and ctl.is_contiguous() and ctl.numel() == 16 and ctl.data_ptr() % 8 == 0)

    def set_mix_ctl(self, ctl, beta, seed=0, step0=0):
        """cn_mix_ctl_set: (beta, seed, step0) into the device block `ctl` (mix_ctl()) by one small launch on the
        current stream; no host sync. A captured graph of robot_mix calls reads whatever was set before its replay.
        beta: a finite probability in [0, 1]."""
        beta = float(beta)
        if not 0.0 <= beta <= 1.0:   # (a NaN fails both)
            raise ValueError("set_mix_ctl: beta in [0, 1] required, got %r" % (beta,))
        if not self._is_mix_ctl(ctl):
            raise ValueError("set_mix_ctl: ctl must be the 16-byte uint8 block of mix_ctl() on %s" % self.device)
        v = abi.CnMixCtl(beta, int(seed) & 0xFFFFFFFF, int(step0))
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().cn_mix_ctl_set(self._stream(), ctl.data_ptr(), ctypes.byref(v)))
        return ctl

    def robot_mix(self, policy, learner, ctl, t, label=None, executed=None, flags=None, regret=None):
        """The learner in the loop (cn_robot_mix): label = robot_act(policy) of the engine's current state, and per
        env a coin of probability ctl.beta -- word z of philox(counter step0 + t, key (seed, global env index)),
        policy_factory.mix_coin -- picks executed = label (taken) or `learner` (E, 2) float32, copied as bits.
        flags (E,) uint8: bit 0 = the label was taken, bit 1 = learner == label as bits. Returns (label, executed,
        flags), each into the tensor given or a fresh one. beta, seed and step0 are read on the device when the
        launch runs (set_mix_ctl); t >= 0 is the launch's own. robot_act's launch(es) + one more; no host sync.
        regret: robot_act's -- an (E, 64) float32 tensor for the controller's regret rows ('dwa' only), written by the
        labelling launch itself (cn_robot_mix_regret); label, executed and flags are what they are without it."""
        tc = self.torch
        if policy not in self.ROBOT_POLICIES:
            raise ValueError("robot_mix: policy %r (one of %s)" % (policy, sorted(self.ROBOT_POLICIES)))
        t = int(t)
        if t < 0:
            raise ValueError("robot_mix: t >= 0 required, got %d" % t)
        if not self._is_mix_ctl(ctl):
            raise ValueError("robot_mix: ctl must be the 16-byte uint8 block of mix_ctl() on %s" % self.device)
        E = self.E
        if label is None:
            label = tc.zeros((E, 2), dtype=tc.float32, device=self.device)
        if executed is None:
            executed = tc.zeros((E, 2), dtype=tc.float32, device=self.device)
        if flags is None:
            flags = tc.zeros((E,), dtype=tc.uint8, device=self.device)
        for name, x in (("learner", learner), ("label", label), ("executed", executed)):
            if (not isinstance(x, tc.Tensor) or x.dtype != tc.float32 or x.device != self.device
                    or not x.is_contiguous() or x.numel() != E * 2 or x.data_ptr() % 8):
                raise ValueError("robot_mix: %s must be a contiguous float32 (E, 2) tensor on %s" % (name, self.device))
        if flags.dtype != tc.uint8 or flags.device != self.device or not flags.is_contiguous() or flags.numel() != E:
            raise ValueError("robot_mix: flags must be a contiguous uint8 (E,) tensor on %s" % self.device)
        if len({learner.data_ptr(), label.data_ptr(), executed.data_ptr()}) != 3:
            raise ValueError("robot_mix: learner, label and executed must be three different buffers")
        if regret is not None:
            self._regret_arg("robot_mix", regret)
            with tc.cuda.device(self.device):
                _lib.check(_lib.lib().cn_robot_mix_regret(self._h, self._stream(), self.ROBOT_POLICIES[policy],
                                                          learner.data_ptr(), ctl.data_ptr(), t, label.data_ptr(),
                                                          executed.data_ptr(), flags.data_ptr(), regret.data_ptr()))
            return label, executed, flags
        with tc.cuda.device(self.device):
            _lib.check(_lib.lib().cn_robot_mix(self._h, self._stream(), self.ROBOT_POLICIES[policy], learner.data_ptr(),
                                               ctl.data_ptr(), t, label.data_ptr(), executed.data_ptr(),
                                               flags.data_ptr()))
        return label, executed, flags

    @staticmethod
    def _lidar_args(lidar):
        """(beams, max_range, robot_radius) of rollout's `lidar` (a dict with those keys)."""
        try:
            return int(lidar["beams"]), float(lidar["max_range"]), float(lidar["robot_radius"])
        except (KeyError, TypeError):
            raise ValueError("rollout: lidar must be a dict with beams, max_range and robot_radius")

    def rollout_buffers(self, T, obs_every_step=True, executed=False, lidar=None, mask=False):
        """Fresh device tensors for rollout(T): the `out` dict without 'num_launches' (executed=True: with the
        'executed' rows of a rollout with noise; lidar=dict(beams=, ..): with the 'lidar' rows and the state rows
        of a rollout with lidar; mask=True: with the 'visible_masks' rows of a rollout with mask)."""
        t, E, N, dev = self.torch, self.E, self.N, self.device
        out = {"actions": t.zeros((T, E, 2), dtype=t.float32, device=dev)}
        if executed:
            out["executed"] = t.zeros((T, E, 2), dtype=t.float32, device=dev)
        if lidar is not None:
            beams = self._lidar_args(lidar)[0]
            out["lidar"] = t.zeros((T, E, 1, 7 + beams), dtype=t.float32, device=dev)
            out["robot_state"] = t.zeros((9, T, E), dtype=t.float64, device=dev)
            out["human_state"] = t.zeros((3, T, E, N), dtype=t.float64, device=dev)
        if mask:
            out["visible_masks"] = t.zeros((T, E, N) if obs_every_step else (E, N), dtype=t.float32, device=dev)
        if obs_every_step:
            out["robot_node"] = t.zeros((T, E, 1, 7), dtype=t.float32, device=dev)
            out["temporal_edges"] = t.zeros((T, E, 1, 2), dtype=t.float32, device=dev)
            out["spatial_edges"] = t.zeros((T, E, N, 2), dtype=t.float32, device=dev)
        else:
            out.update(self.obs())
        out["reward"] = t.zeros((T, E), dtype=t.float32, device=dev)
        out["done"] = t.zeros((T, E), dtype=t.uint8, device=dev)
        out["event"] = t.zeros((T, E), dtype=t.int8, device=dev)
        out["info"] = t.zeros((T, E, abi.INFO_K), dtype=t.float32, device=dev)
        out["ep_return"] = t.zeros((T, E), dtype=t.float64, device=dev)
        out["ep_len"] = t.zeros((T, E), dtype=t.int32, device=dev)
        return out

    _ROLLOUT_OPTIONAL = ("reward", "done", "event", "info", "ep_return", "ep_len")

    def rollout(self, policy, T, obs_every_step=True, out=None, noise=None, lidar=None, mask=False):
        """T closed-loop steps of the scripted robot (cn_rollout): robot_act(policy) -> step, every step recorded,
        with the rows of that eager loop bit for bit. Returns a dict of device tensors: actions (T, E, 2);
        robot_node / temporal_edges / spatial_edges (T, E, ...) = the observation AFTER step t (with
        obs_every_step=False: the engine's own single-row buffers, holding the last step's); reward, done, event,
        info, ep_return, ep_len (T, E, ...); 'num_launches' (int). `out`: a dict from an earlier call (or
        rollout_buffers) to reuse; of the six per-step records any may be left out or None (not recorded). Where
        the engine allows it the steps run inside multi-step launches with the controller in the step kernel; no
        host sync either way.
        noise (a RolloutNoise or a dict with sigma / seed / step0; None: cn_rollout as ever) -> cn_rollout_noisy: the
        step takes actions + sigma * n with n uniform in [-1, 1) per component, drawn per (seed, global env index,
        step0 + t); 'actions' keeps the clean labels and the dict gains 'executed' (T, E, 2), what the step took
        (allocated when `out` lacks it).
        lidar (dict(beams=, max_range=, robot_radius=), lidar_scan's; None: none) -> cn_rollout_lidar: the dict gains
        'lidar' (T, E, 1, 7 + beams) f32, the live ConvGRU observation AFTER step t (what lidar_scan writes right
        after that step), and the state it was scanned from, 'robot_state' (9, T, E) and 'human_state' (3, T, E, N)
        f64 (r_px, r_py, r_vx, r_vy, r_radius, r_gx, r_gy, r_vpref, r_theta; h_px, h_py, h_r). Each is taken from
        `out` when given (a trainer aims 'lidar' at its storage) and allocated otherwise.
        mask (True, or `out` holding 'visible_masks'; not with lidar) -> cn_rollout_masked: the dict gains
        'visible_masks' (T, E, N) f32, what visible_mask() returns right after step t ((E, N) with
        obs_every_step=False: the last step's), written by the rollout launches themselves where the steps are fused
        and by one visible_mask launch per step elsewhere. Taken from `out` when given (a trainer aims it at its
        storage) and allocated otherwise."""
        t = self.torch
        if policy not in self.ROBOT_POLICIES:
            raise ValueError("rollout: policy %r (one of %s)" % (policy, sorted(self.ROBOT_POLICIES)))
        T = int(T)
        if T < 0:
            raise ValueError("rollout: T >= 0 required, got %d" % T)
        noise = RolloutNoise.of(noise)
        E, N = self.E, self.N
        if out is None:
            out = self.rollout_buffers(T, obs_every_step, executed=noise is not None, mask=bool(mask))
        else:
            out = dict(out)
            mask = bool(mask) or out.get("visible_masks") is not None
            if noise is not None and out.get("executed") is None:
                out["executed"] = t.zeros((T, E, 2), dtype=t.float32, device=self.device)
        rl = None
        if lidar is not None:
            beams, max_range, robot_radius = self._lidar_args(lidar)
            if not (2 <= beams <= 4096 and 0 < max_range <= 1e4):
                raise ValueError("rollout: lidar beams in [2, 4096] and max_range in (0, 1e4] required")
            lwant = {"lidar": ((T, E, 1, 7 + beams), t.float32), "robot_state": ((9, T, E), t.float64),
                     "human_state": ((3, T, E, N), t.float64)}
            for k, (shape, dt) in lwant.items():
                v = out.get(k)
                if v is None:
                    v = out[k] = t.zeros(shape, dtype=dt, device=self.device)
                n = int(np.prod(shape))
                if v.dtype != dt or v.device != self.device or not v.is_contiguous() or v.numel() != n:
                    raise ValueError("rollout: out[%r] must be a contiguous %s tensor of %d elements on %s"
                                     % (k, dt, n, self.device))
            rl = _lib.RolloutLidar(out["lidar"].data_ptr(), beams, max_range, robot_radius,
                                   out["robot_state"].data_ptr(), out["human_state"].data_ptr())
        R = 1 if not obs_every_step else T
        if mask:
            if lidar is not None:
                raise ValueError("rollout: mask and lidar exclude each other (no visible_masks with the LiDAR "
                                 "observation)")
            v = out.get("visible_masks")
            if v is None:
                v = out["visible_masks"] = t.zeros((T, E, N) if obs_every_step else (E, N), dtype=t.float32,
                                                   device=self.device)
            if v.dtype != t.float32 or v.device != self.device or not v.is_contiguous() or v.numel() != R * E * N:
                raise ValueError("rollout: out['visible_masks'] must be a contiguous %s tensor of %d elements on %s"
                                 % (t.float32, R * E * N, self.device))
        want = {"actions": (T * E * 2, t.float32), "robot_node": (R * E * 7, t.float32),
                "temporal_edges": (R * E * 2, t.float32), "spatial_edges": (R * E * N * 2, t.float32),
                "reward": (T * E, t.float32), "done": (T * E, t.uint8), "event": (T * E, t.int8),
                "info": (T * E * abi.INFO_K, t.float32), "ep_return": (T * E, t.float64), "ep_len": (T * E, t.int32)}
        ro = _lib.RolloutOut()
        for k, (n, dt) in want.items():
            v = out.get(k)
            if v is None:
                if k not in self._ROLLOUT_OPTIONAL:
                    raise ValueError("rollout: out[%r] is required" % k)
                continue
            if v.dtype != dt or v.device != self.device or not v.is_contiguous() or v.numel() != n:
                raise ValueError("rollout: out[%r] must be a contiguous %s tensor of %d elements on %s"
                                 % (k, dt, n, self.device))
            setattr(ro, k, v.data_ptr())
        ro.flags = _lib.ROLLOUT_OBS_EVERY_STEP if obs_every_step else 0
        if noise is not None:
            x = out["executed"]
            if x.dtype != t.float32 or x.device != self.device or not x.is_contiguous() or x.numel() != T * E * 2:
                raise ValueError("rollout: out['executed'] must be a contiguous %s tensor of %d elements on %s"
                                 % (t.float32, T * E * 2, self.device))
        nl = ctypes.c_int32(0)
        if T == 0:   # (empty tensors have no address to pass; cn_rollout launches nothing for T = 0 either)
            out["num_launches"] = 0
            return out
        nz = None
        if noise is not None:
            nz = _lib.RolloutNoise(noise.sigma, noise.seed & 0xFFFFFFFF, noise.step0, out["executed"].data_ptr())
        with t.cuda.device(self.device):
            if rl is not None:
                _lib.check(_lib.lib().cn_rollout_lidar(self._h, self._stream(), self.ROBOT_POLICIES[policy], T,
                                                       ctypes.byref(ro), None if nz is None else ctypes.byref(nz),
                                                       ctypes.byref(rl), ctypes.byref(nl)))
            elif mask:
                _lib.check(_lib.lib().cn_rollout_masked(self._h, self._stream(), self.ROBOT_POLICIES[policy], T,
                                                        ctypes.byref(ro), None if nz is None else ctypes.byref(nz),
                                                        out["visible_masks"].data_ptr(), ctypes.byref(nl)))
            elif noise is None:
                _lib.check(_lib.lib().cn_rollout(self._h, self._stream(), self.ROBOT_POLICIES[policy], T,
                                                 ctypes.byref(ro), ctypes.byref(nl)))
            else:
                _lib.check(_lib.lib().cn_rollout_noisy(self._h, self._stream(), self.ROBOT_POLICIES[policy], T,
                                                       ctypes.byref(ro), ctypes.byref(nz), ctypes.byref(nl)))
        out["num_launches"] = int(nl.value)
        return out

    def get_state(self):
        """abi.StateView of the engine; a mixed engine: [(rows, StateView of the group)] in group order."""
        buf = np.zeros(self.state_bytes, np.uint8)
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().cn_get_state(self._h, self._stream(), buf.ctypes.data_as(ctypes.c_void_p), 1))
        if self.groups is None:
            return abi.StateView(buf, self.E, self.N, self.cfg.robot_visible)
        out, off = [], 0
        for c, rows in self.groups:
            nb = abi.state_layout(int(c.num_envs), int(c.human_num), c.robot_visible)[1]
            out.append((rows, abi.StateView(buf[off:off + nb].copy(), int(c.num_envs), int(c.human_num),
                                            c.robot_visible)))
            off += nb
        return out

    def set_state(self, sv):
        if self.groups is not None:
            blob = np.concatenate([np.ascontiguousarray(v.blob).view(np.uint8).ravel() for _, v in sv])
        else:
            blob = np.ascontiguousarray(sv.blob)
        if blob.nbytes != self.state_bytes:
            raise ValueError("state blob has %d bytes, engine expects %d" % (blob.nbytes, self.state_bytes))
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().cn_set_state(self._h, self._stream(), blob.ctypes.data_as(ctypes.c_void_p), 1))

    def set_spawn_budget(self, cycles):
        """Test hook (cn_debug_set_spawn_budget): clock cycles a kd-tree-path spawning wave works per launch
        before it parks its spawn (default 600000; 0 = never). Results do not depend on it (round 5 fixed a rare
        case where they did: DESIGN.md)."""
        _lib.check(_lib.lib().cn_debug_set_spawn_budget(self._h, int(cycles)))

    def set_seq_chunk(self, n):
        """Steps per launch of step_seq's multi-step launches (cn_debug_set_seq_chunk); 1 = one step launch per
        step through the single-step kernels. Results do not depend on it."""
        _lib.check(_lib.lib().cn_debug_set_seq_chunk(self._h, int(n)))
        self.seq_chunk = int(n)

    def spawn_stats(self):
        """Cumulative spawn counters (cn_debug_spawn_stats; synchronises): kd-tree path spawns parked before
        starting, parked mid-way, resumed, completed by a resume; auto-resets drawn inline (no pending spawn)."""
        out = (ctypes.c_uint32 * 5)()
        _lib.check(_lib.lib().cn_debug_spawn_stats(self._h, out))
        return dict(zip(("parked_unstarted", "parked_midway", "resumed", "completed_on_resume", "inline_resets"),
                        list(out)))

    def close(self):
        if getattr(self, "_h", None) is not None:
            _lib.lib().cn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NumpyEngine:
    """numpy-in/numpy-out facade over CrowdNavEngine with the oracle's interface (used by tests)."""

    def __init__(self, cfg, device=None):
        self.eng = CrowdNavEngine(cfg, device)
        self.E, self.N = self.eng.E, self.eng.N

    def reset(self):
        o = self.eng.reset()
        self.eng.torch.cuda.synchronize(self.eng.device)
        return {k: v.cpu().numpy() for k, v in o.items()}

    def step(self, actions):
        t = self.eng.torch
        a = t.from_numpy(np.ascontiguousarray(actions, np.float32).reshape(self.E, 2)).to(self.eng.device)
        obs, rew, done, ev, info, epr, epl = self.eng.step(a)
        t.cuda.synchronize(self.eng.device)
        return ({k: v.cpu().numpy() for k, v in obs.items()}, rew.cpu().numpy(), done.cpu().numpy(),
                ev.cpu().numpy(), info.cpu().numpy(), epr.cpu().numpy(), epl.cpu().numpy())

    def get_state(self):
        return self.eng.get_state()

    def set_state(self, sv):
        self.eng.set_state(sv)
