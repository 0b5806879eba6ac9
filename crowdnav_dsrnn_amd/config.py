"""Configuration: the reference's `Config` attribute tree and its translation to `cn_config`.

`Config` mirrors crowd_nav/configs/config.py:9-214 of the reference (same sub-objects, same attribute
names, same defaults) so that code written against the reference config keeps working. Any object
with that attribute tree — including the reference's own `Config` — can be passed to
`make_cn_config`.
"""
import numpy as np

from . import abi


class BaseConfig(object):
    def __init__(self):
        pass


class Config(object):
    """Mirror of crowd_nav/configs/config.py:9-214 (defaults identical)."""

    test = BaseConfig()
    test.social_metrics = False

    sim = BaseConfig()
    sim.render = False
    sim.train_val_sim = ["circle_crossing", "square_crossing", "parallel_traffic", "perpendicular_traffic"]
    sim.test_sim = ["circle_crossing", "square_crossing", "parallel_traffic", "perpendicular_traffic"]
    sim.square_width = 20
    test.side_preference = any("side_pref" in s_ for s_ in sim.test_sim)
    sim.circle_radius = 6 if not test.social_metrics and not test.side_preference else 4
    sim.human_num = 5 if not test.side_preference else 1
    sim.group_human = False
    # human_nums (this project's opt-in, not a reference option): a list of human counts, e.g. [5, 10] -- the env
    # with global index g runs human_nums[g % len] humans in ONE mixed engine (make_varied_cn_configs), the
    # observation is padded to the largest count and carries 'detected_human_num'. None: sim.human_num for all
    sim.human_nums = None
    # human_nums_scripted (with human_nums; holonomic): the env also serves the scripted controllers -- robot_act,
    # rollout, ScriptedRobot, evaluate_scripted, BehaviourCloning (the mixed engine's cn_mixed_scripted opt-in).
    # Off, the default, those refuse an env of varying human count with UnsupportedConfig, as before.
    sim.human_nums_scripted = False
    # visible_masks (this project's opt-in, not a reference option; the key CrowdNav++ uses): the observation also
    # carries 'visible_masks' (N,), 1.0 for the humans the robot currently sees (the engine's cn_visible_mask: the
    # step's own FOV decisions), and the DSRNN's spatial attention runs over those slots only. Off, the default,
    # the observation and the policy are what they were. Not with robot.policy 'convgru' (no human slots there).
    sim.visible_masks = False
    # visible_masks_scripted (with visible_masks): the env also serves the scripted rollouts -- CrowdNavVecEnv.rollout,
    # ScriptedRobot.rollout, evaluate_scripted, BehaviourCloning -- whose rows then carry 'visible_masks' too (the
    # engine's cn_rollout_masked). Off, the default, those refuse a visible_masks env with UnsupportedConfig, as before.
    sim.visible_masks_scripted = False

    env = BaseConfig()
    env.env_name = "CrowdSimDict-v0"
    env.time_limit = 50
    env.time_step = 0.25
    env.val_size = 100
    env.test_size = 500
    if test.social_metrics:
        env.test_size = 2000
    elif test.side_preference:
        env.test_size = 200
    env.randomize_attributes = True
    env.seed = 0

    reward = BaseConfig()
    reward.time_factor = False
    reward.normalize = False
    reward.potential_based = True
    reward.exponential = False
    reward.norm_zones = False
    reward.success_reward = 10 if not reward.normalize else 1
    reward.collision_penalty = -20 if not reward.normalize else -1
    reward.timeout_penalty = -20 if not reward.normalize else -1
    reward.discomfort_dist_front = 0.25
    reward.discomfort_dist_back = 0.25
    reward.discomfort_penalty_factor = 10 if not reward.normalize else 0.5
    reward.discomfort_penalty_factor *= env.time_step
    reward.potential_factor = 2 if not reward.normalize else 0.1
    reward.exp_factor = 0.5 if not reward.normalize else 0.025
    reward.exp_denom = 6
    reward.gamma = 0.99
    reward.norm_zone_side = "lhs"
    reward.norm_zone_penalty = -0.5

    humans = BaseConfig()
    humans.visible = True
    humans.policy = "orca"
    humans.radius = 0.3
    humans.v_pref = 1
    humans.sensor = "coordinates"
    humans.FOV = 2.0
    humans.random_goal_changing = True if not test.side_preference else False
    humans.goal_change_chance = 0.25
    humans.end_goal_changing = True if not test.side_preference else False
    humans.end_goal_change_chance = 1.0
    humans.random_radii = False
    humans.random_v_pref = False
    humans.random_unobservability = False
    humans.unobservable_chance = 0.3
    humans.random_policy_changing = False

    robot = BaseConfig()
    robot.visible = False
    robot.policy = "srnn"
    robot.radius = 0.3
    robot.v_pref = 1
    robot.sensor = "coordinates"
    robot.FOV = 2.0
    # scripted_unicycle (this project's opt-in, not a reference option; with action_space.kinematics = 'unicycle'):
    # the env also serves the scripted controllers -- robot_act, rollout, ScriptedRobot, evaluate_scripted,
    # BehaviourCloning -- whose velocity a tracking law turns into the unicycle action (the engine's
    # cn_scripted_unicycle). Off, the default, those refuse a unicycle env with UnsupportedConfig, as before.
    robot.scripted_unicycle = False
    # scripted_dwa (this project's opt-in as well; with action_space.kinematics = 'unicycle'): the env also serves the
    # scripted controller 'dwa', a dynamic-window controller that plans in the unicycle's own action space
    # (policy_factory.dwa_predict; the engine's cn_scripted_dwa). True: policy_factory.DWA_DEFAULTS; a dict: those with
    # its overrides. None, the default: 'dwa' is refused, as before. It needs no scripted_unicycle (no tracking law).
    robot.scripted_dwa = None
    # action_head (this project's opt-in; read by policy.Policy alone, the engine never sees it): 'gaussian', the
    # default, is the reference's DiagGaussian; 'lattice' (with action_space.kinematics = 'unicycle') a 64-way
    # categorical over the grid of unicycle actions the 'dwa' controller chooses from (policy.LatticeCategorical,
    # state_dict keys dist.fc_logits.*). Policy(..., head=...) overrides it.
    robot.action_head = "gaussian"

    noise = BaseConfig()
    noise.add_noise = False
    noise.type = "uniform"
    noise.magnitude = 0.1

    lidar = BaseConfig()
    lidar.enable = False
    lidar.viz = False
    # live = True (this project's opt-in, not a reference option): with robot.policy = 'convgru' and
    # lidar.enable the observation carries the scan of the CURRENT state at every reset and step — all humans
    # and the walls, heading along the robot's velocity (cn_lidar_scan) — instead of the reference's held
    # per-episode scan of the last human
    lidar.live = False
    lidar.cfg = {"max_range": 5, "num_beams": 180, "robot_radius": robot.radius}

    action_space = BaseConfig()
    action_space.kinematics = "holonomic"

    orca = BaseConfig()
    orca.neighbor_dist = 10
    orca.safety_space = 0.15
    orca.time_horizon = 5
    orca.time_horizon_obst = 5

    sf = BaseConfig()
    sf.A = 2.0
    sf.B = 1
    sf.KI = 1

    social = BaseConfig()
    social.min_personal_space = 0.2
    social.max_walking_speed = 1.5

    ppo = BaseConfig()
    ppo.num_mini_batch = 2
    ppo.num_steps = 30
    ppo.recurrent_policy = True
    ppo.epoch = 5
    ppo.clip_param = 0.2
    ppo.value_loss_coef = 0.5
    ppo.entropy_coef = 0.0
    ppo.use_gae = True
    ppo.gae_lambda = 0.95

    SRNN = BaseConfig()
    SRNN.human_node_rnn_size = 128
    SRNN.human_human_edge_rnn_size = 256
    SRNN.human_node_input_size = 3
    SRNN.human_human_edge_input_size = 2
    SRNN.human_node_output_size = 256
    SRNN.human_node_embedding_size = 64
    SRNN.human_human_edge_embedding_size = 64
    SRNN.attention_size = 64

    training = BaseConfig()
    training.lr = 4e-5
    training.eps = 1e-5
    training.alpha = 0.99
    training.max_grad_norm = 0.5
    training.num_env_steps = 10e6
    training.use_linear_lr_decay = False
    training.save_interval = 200
    training.log_interval = 20
    training.use_proper_time_limits = False
    training.cuda_deterministic = False
    training.cuda = True
    training.num_processes = 12
    training.output_dir = "data/dummy"
    training.resume = False
    training.load_path = None
    training.overwrite = True
    training.num_threads = 1


class UnsupportedConfig(ValueError):
    pass


def make_cn_config(config, num_envs, env_offset=0, nenv=None, phase=None, seed=None, max_tries=1000,
                   scenarios=None, scenario_mode=None, rng=None):
    """Translate a reference-style config into `cn_config` for `num_envs` envs starting at global
    index `env_offset`; `nenv` is the reference's num_processes over all shards (make_env's envNum,
    pytorchBaselines/a2c_ppo_acktr/envs.py:66-73); `phase` defaults like make_env ('train' if nenv > 1).
    `rng` ('mt19937' default = the reference's numpy draws, or 'philox' = fast mode with the same draw
    order and distributions; also read from `config.env.rng` when set) selects the reset / goal-change
    random stream."""
    nenv = num_envs if nenv is None else nenv
    if phase is None:
        phase = "train" if nenv > 1 else "test"
    bad = []
    if getattr(config.sim, "group_human", False):
        bad.append("sim.group_human (group environment) is not part of the engine")
    if getattr(config.humans, "random_unobservability", False):
        bad.append("humans.random_unobservability")
    if getattr(config.humans, "random_policy_changing", False):
        bad.append("humans.random_policy_changing (uses the unseeded python random module)")
    if getattr(config.noise, "add_noise", False):
        bad.append("noise.add_noise")
    # lidar.enable: the LiDAR scan only feeds the 'convgru' observation, built outside the step kernel by
    # cn_lidar_obs (or, with lidar.live, cn_lidar_scan) in CrowdNavVecEnv; with the srnn policy it changes
    # nothing the reference returns
    if not config.reward.potential_based or getattr(config.reward, "exponential", False):
        bad.append("reward.exponential")
    if config.humans.policy not in ("orca", "social_force"):
        bad.append("humans.policy=%r" % config.humans.policy)
    if config.robot.policy not in ("srnn", "convgru"):
        bad.append("robot.policy=%r (the srnn observation dict and the convgru LiDAR row are produced)"
                   % config.robot.policy)
    if config.action_space.kinematics not in ("holonomic", "unicycle"):
        bad.append("action_space.kinematics=%r" % config.action_space.kinematics)
    if bad:
        raise UnsupportedConfig("; ".join(bad))

    c = abi.CnConfig()
    c.num_envs = int(num_envs)
    c.human_num = int(config.sim.human_num)
    c.env_offset = int(env_offset)
    c.nenv = int(nenv)
    c.seed = int(config.env.seed if seed is None else seed)
    c.phase = abi.PHASES[phase]
    c.kinematics = abi.HOLONOMIC if config.action_space.kinematics == "holonomic" else abi.UNICYCLE
    c.human_policy = abi.POLICY_ORCA if config.humans.policy == "orca" else abi.POLICY_SOCIAL_FORCE
    if scenarios is None:
        scenarios = config.sim.train_val_sim if phase in ("train", "val") else config.sim.test_sim
    if isinstance(scenarios, str):
        raise TypeError("config.sim.train_val_sim or config.sim.test_sim should be a list of strings")
    if not 0 < len(scenarios) <= abi.MAX_SCENARIOS:
        raise UnsupportedConfig("1..%d scenarios supported" % abi.MAX_SCENARIOS)
    c.num_scenarios = len(scenarios)
    for k, s in enumerate(scenarios):
        c.scenarios[k] = abi.SCENARIO_ID[s]
    if scenario_mode is None:
        scenario_mode = abi.SCMODE_SEQUENTIAL if config.test.social_metrics else abi.SCMODE_ROUND_ROBIN
    c.scenario_mode = scenario_mode
    c.val_size = int(config.env.val_size)
    c.test_size = int(config.env.test_size)
    c.time_step = float(config.env.time_step)
    c.time_limit = float(config.env.time_limit)
    c.circle_radius = float(config.sim.circle_radius)
    c.square_width = float(config.sim.square_width)
    c.robot_radius = float(config.robot.radius)
    c.robot_vpref = float(config.robot.v_pref)
    c.robot_fov = float(np.pi * config.robot.FOV)
    c.human_radius = float(config.humans.radius)
    c.human_vpref = float(config.humans.v_pref)
    c.human_fov = float(np.pi * config.humans.FOV)
    c.robot_visible = int(bool(config.robot.visible))
    c.randomize_attributes = int(bool(config.env.randomize_attributes))
    c.random_goal_changing = int(bool(config.humans.random_goal_changing))
    c.end_goal_changing = int(bool(config.humans.end_goal_changing))
    c.random_radii = int(bool(config.humans.random_radii))
    c.random_v_pref = int(bool(config.humans.random_v_pref))
    c.goal_change_chance = float(getattr(config.humans, "goal_change_chance", 0.25))
    c.end_goal_change_chance = float(getattr(config.humans, "end_goal_change_chance", 1.0))
    c.success_reward = float(config.reward.success_reward)
    c.collision_penalty = float(config.reward.collision_penalty)
    c.discomfort_dist = float(config.reward.discomfort_dist_back)
    c.discomfort_penalty_factor = float(config.reward.discomfort_penalty_factor)
    c.potential_factor = float(config.reward.potential_factor)
    c.norm_zone_penalty = float(getattr(config.reward, "norm_zone_penalty", -0.5))
    c.potential_based = 1
    c.time_factor = int(bool(config.reward.time_factor))
    c.norm_zones = int(bool(getattr(config.reward, "norm_zones", False)))
    c.norm_zone_lhs = int("lhs" in getattr(config.reward, "norm_zone_side", "lhs"))
    c.min_personal_space = float(config.social.min_personal_space)
    c.max_walking_speed = float(config.social.max_walking_speed)
    c.social_metrics = int(bool(config.test.social_metrics))
    c.side_preference = int(bool(config.test.side_preference))
    c.orca_neighbor_dist = float(config.orca.neighbor_dist)
    c.orca_safety_space = float(config.orca.safety_space)
    c.orca_time_horizon = float(config.orca.time_horizon)
    c.orca_time_horizon_obst = float(config.orca.time_horizon_obst)
    c.sf_A = float(config.sf.A)
    c.sf_B = float(config.sf.B)
    c.sf_KI = float(config.sf.KI)
    c.max_tries = int(max_tries)
    rng = getattr(config.env, "rng", "mt19937") if rng is None else rng
    if rng not in abi.RNG_MODE:
        raise UnsupportedConfig("rng=%r (one of %s)" % (rng, sorted(abi.RNG_MODE)))
    c.rng_mode = abi.RNG_MODE[rng]
    return c


def clone_config(config):
    """Independent copy of a reference-style config (the reference keeps its sub-configs as CLASS
    attributes, so two `Config()` instances share state; the clone gets instance-level copies)."""
    import copy

    new = Config.__new__(Config)
    for name in dir(config):
        if name.startswith("_"):
            continue
        val = getattr(config, name)
        if type(val).__name__ == "BaseConfig":
            setattr(new, name, copy.deepcopy(val))
    return new


def make_mixed_cn_configs(scenario_configs, scenarios, num_envs, env_offset=0, nenv=None, phase=None, rng=None):
    """Per-env scenario dispatch with per-env human counts for CrowdNavEngine.mixed.

    `scenarios` is the round-robin scenario list: env r (global index env_offset + r) runs
    scenarios[(env_offset + r) % len(scenarios)] (the engine's deterministic stand-in for the reference's
    per-reset `random.choices`, crowd_sim_dict.py:110-125). `scenario_configs` maps each scenario name to
    the reference-style config its envs use (human_num, circle_radius, test.side_preference, goal
    changing, ... -- e.g. the side_pref_* scenarios at N = 1, crowd_sim.py:334-357,642-651); scenarios
    that share one config object share one group. Returns (list of cn_config, env_group int32 [num_envs])."""
    nenv = num_envs if nenv is None else nenv
    keys, groups, env_group = [], [], np.zeros(num_envs, np.int32)
    for s in scenarios:
        if id(scenario_configs[s]) not in keys:
            keys.append(id(scenario_configs[s]))
            groups.append(scenario_configs[s])
    sc_group = [keys.index(id(scenario_configs[s])) for s in scenarios]
    for r in range(num_envs):
        env_group[r] = sc_group[(env_offset + r) % len(scenarios)]
    cfgs = [make_cn_config(c, num_envs=int((env_group == g).sum()), env_offset=env_offset, nenv=nenv, phase=phase,
                           scenarios=list(scenarios), scenario_mode=abi.SCMODE_ROUND_ROBIN, rng=rng)
            for g, c in enumerate(groups)]
    return cfgs, env_group


def visible_masks_on(config):
    """config.sim.visible_masks as a bool (absent: False). UnsupportedConfig with robot.policy 'convgru', whose
    observation has no human slots to mask (read from the config alone)."""
    on = bool(getattr(config.sim, "visible_masks", False))
    if on and getattr(config.robot, "policy", "srnn") == "convgru":
        raise UnsupportedConfig("sim.visible_masks with robot.policy='convgru' (the LiDAR observation has no human "
                                "slots to mask)")
    return on


def visible_masks_scripted(config):
    """config.sim.visible_masks_scripted as a bool (absent: False): the scripted rollouts serve the visible_masks env
    and record the mask. UnsupportedConfig when it is set without sim.visible_masks (read from the config alone)."""
    on = bool(getattr(config.sim, "visible_masks_scripted", False))
    if on and not getattr(config.sim, "visible_masks", False):
        raise UnsupportedConfig("sim.visible_masks_scripted without sim.visible_masks (the opt-in lets the scripted "
                                "rollouts record the mask of a visible_masks env)")
    return on


def no_visible_masks(config, what):
    """UnsupportedConfig for what an env with config.sim.visible_masks does not serve without the
    sim.visible_masks_scripted opt-in: the scripted rollouts, whose rows then carry no mask (read from the config
    alone). Returns whether the rollout has to record the mask (both keys set)."""
    if visible_masks_scripted(config):
        return visible_masks_on(config)
    if getattr(config.sim, "visible_masks", False):
        raise UnsupportedConfig("%s: not served on an env with config.sim.visible_masks (the rows a scripted "
                                "rollout records carry no mask) unless config.sim.visible_masks_scripted is set" % what)
    return False


MAX_VARIED_HUMANS = 31   # the engine's largest human count per env


def varied_human_nums(config):
    """config.sim.human_nums as a list of ints, or None when the opt-in is absent. UnsupportedConfig for an empty
    list, an entry outside 1..31, or robot.policy 'convgru' (the LiDAR scan does not run on a mixed engine)."""
    nums = getattr(config.sim, "human_nums", None)
    if nums is None:
        return None
    if isinstance(nums, (str, bytes)) or not hasattr(nums, "__len__"):
        raise UnsupportedConfig("sim.human_nums=%r (a list of human counts)" % (nums,))
    nums = list(nums)
    if not nums:
        raise UnsupportedConfig("sim.human_nums is empty")
    for n in nums:
        if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_VARIED_HUMANS:
            raise UnsupportedConfig("sim.human_nums entry %r (1..%d humans per env)" % (n, MAX_VARIED_HUMANS))
    if getattr(config.robot, "policy", "srnn") == "convgru":
        raise UnsupportedConfig("sim.human_nums with robot.policy='convgru' (the LiDAR observation is not served on a "
                                "mixed engine)")
    if getattr(config.test, "social_metrics", False):
        raise UnsupportedConfig("sim.human_nums with test.social_metrics (the mixed engine dispatches scenarios "
                                "round-robin only)")
    return [int(n) for n in nums]


def make_varied_cn_configs(config, human_nums, num_envs, env_offset=0, nenv=None, phase=None, seed=None, rng=None):
    """Envs of varying human count for CrowdNavEngine.mixed: one group per distinct count, identical except
    human_num and each with the full scenario list; the env with global index g = env_offset + r runs
    human_nums[g % len(human_nums)] humans (shards agree with an unsharded run). Returns (list of cn_config in
    the order the counts first appear in human_nums, env_group int32 [num_envs]). `config` is not modified."""
    probe = clone_config(config)
    probe.sim.human_nums = human_nums
    nums = varied_human_nums(probe)
    if nums is None:
        raise UnsupportedConfig("make_varied_cn_configs: human_nums is None")
    nenv = num_envs if nenv is None else nenv
    distinct = []
    for n in nums:
        if n not in distinct:
            distinct.append(n)
    env_group = np.array([distinct.index(nums[(env_offset + r) % len(nums)]) for r in range(num_envs)], np.int32)
    cfgs = []
    for g, n in enumerate(distinct):
        c = clone_config(config)
        c.sim.human_num = n
        cfgs.append(make_cn_config(c, num_envs=int((env_group == g).sum()), env_offset=env_offset, nenv=nenv,
                                   phase=phase, seed=seed, rng=rng))
    return cfgs, env_group
