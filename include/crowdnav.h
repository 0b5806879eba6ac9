/*
 * crowdnav.h — C ABI of the MI355X batched CrowdSimDict engine (libcrowdnav_hip.so).
 *
 * Drop-in boundary for the reference's env hot path. Each entry point replaces a reference
 * interface (paths relative to the CrowdNav_DSRNN checkout):
 *
 *   cn_create     ⟵ gym.make('CrowdSimDict-v0') + CrowdSim.configure(config) + make_env's
 *                   thisSeed/nenv/phase assignment, for E envs at once
 *                   (crowd_sim/__init__.py:9-11, crowd_sim/envs/crowd_sim.py:93-246,
 *                    pytorchBaselines/a2c_ppo_acktr/envs.py:46-75)
 *   cn_reset      ⟵ CrowdSimDict.reset() of every env (crowd_sim/envs/crowd_sim_dict.py:105-203),
 *                   i.e. ShmemVecEnv.reset (shmem_vec_env.py:89-95) + VecPyTorch.reset (envs.py:215-222)
 *   cn_step       ⟵ CrowdSimDict.step(action) of every env (crowd_sim_dict.py:205-271) followed by the
 *                   VecEnv worker's auto-reset (shmem_vec_env.py:164-168) and bench.Monitor's episode
 *                   bookkeeping; i.e. VecPyTorch.step (envs.py:224-239) minus the Python info dicts
 *   cn_get_state / cn_set_state   ⟵ no reference equivalent (state lives in forked workers there);
 *                   used for teacher-forced parity tests and rollout checkpointing
 *   cn_edge_features ⟵ the input layers of the DSRNN forward, fused:
 *                   HumanHumanEdgeRNN.encoder_linear+ReLU (srnn_model.py:210-211) for the temporal and
 *                   spatial edges, SRNN.robot_linear (srnn_model.py:466) and
 *                   HumanNodeRNN.encoder_linear+ReLU (srnn_model.py:160-161)
 *   cn_gru_fwd_step / cn_gru_bwd_step ⟵ one time step of the mask-segmented GRU
 *                   (srnn_model.py:52-104 RNNBase._forward_gru, torch nn.GRU cell math) and its gradient;
 *                   cn_gru_fwd_fused runs the recurrent GEMM hm W_hh^T on the f32 MFMA with the gates in its
 *                   epilogue (the forward's per-step kernel); cn_gru_fwd_seq / cn_gru_bwd_seq run whole
 *                   sequences (up to two GRUs per launch; the backward's dgh W_hh on the MFMA with the gate
 *                   gradients in its epilogue); x W_ih^T and the weight gradients over all steps remain
 *                   library GEMMs
 *   cn_gaussian_act ⟵ the act() tail of DiagGaussian / FixedNormal (distributions.py:36-94): sample or
 *                   mode and the summed log-probability
 *   cn_lattice_act / cn_lattice_eval_fwd / cn_lattice_eval_bwd ⟵ (no reference counterpart) the opt-in lattice action
 *                   head of the unicycle robot: a categorical policy over cn_dwa_predict's 64 candidate actions
 *   cn_robot_act_regret / cn_robot_mix_regret / cn_lattice_soft_fwd / cn_lattice_soft_bwd ⟵ (no reference
 *                   counterpart) soft labels: the controller's regret row of all 64 candidates beside its action, and
 *                   the lattice head's cross-entropy against the distribution those regrets define
 *   cn_gae         ⟵ RolloutStorage.compute_returns with use_gae (storage.py:132-177), one launch per rollout
 *   cn_orca_predict / cn_orca_predict_kd / cn_social_force_predict ⟵ the agent policy plugin
 *                   policy_factory[name](config).predict(JointState) (crowd_nav/policy/policy_factory.py:1-17)
 *   cn_dwa_predict / cn_scripted_dwa ⟵ (no reference counterpart) a dynamic-window controller that plans in the
 *                   unicycle robot's own action space; the opt-in makes it cn_robot_act's policy CN_ROBOT_DWA
 *   cn_robot_act     ⟵ Robot.act of a scripted ('orca' / 'social_force') robot on its belief
 *                   (crowd_sim/envs/utils/robot.py:9-15, crowd_sim.py:1113-1114,1185-1188), every env in one launch
 *   cn_robot_mix / cn_mix_ctl_set ⟵ (no reference counterpart) cn_robot_act as the labeller of a learner that drives
 *                   the envs: a per-env coin picks the executed action (DAgger's mixture policy), read from device memory
 *   cn_rollout       ⟵ the closed loop `action = robot.act(ob); ob, ... = env.step(action)` of a scripted robot
 *                   over T steps (crowd_nav test loop / expert demonstrations), every step recorded, in
 *                   multi-step launches with the controller inside the step kernel
 *   cn_rollout_noisy ⟵ (no reference counterpart) cn_rollout whose executed action is the clean one plus uniform
 *                   noise, the label staying clean: noise-injected expert demonstrations for behaviour cloning
 *   cn_rollout_lidar ⟵ (no reference counterpart) either of the two, recording the state every step leaves and,
 *                   from it, the live ConvGRU observation (cn_lidar_scan's) of every step in one scan launch
 *   cn_rollout_masked ⟵ (no reference counterpart) either of the two, recording cn_visible_mask's row of every step
 *                   inside the rollout launches: expert demonstrations for the masked spatial attention
 *   cn_lidar_obs     ⟵ CrowdSimDict.generate_ob's 'convgru' observation (crowd_sim_dict.py:96-101) with
 *                   LidarSensor.sensor_spin (crowd_sim/envs/utils/lidarv2.py:398-427) evaluated at reset
 *   cn_lidar_scan    ⟵ the scan CrowdSimDict.step() takes every step and discards (crowd_sim_dict.py:224-251):
 *                   all humans and the walls, heading along the robot's velocity (opt-in live mode)
 *   cn_wgrad       ⟵ the weight / bias gradient of the Linear layers with a tiny side (autograd's dy^T x)
 *   cn_attn_pool_fwd / cn_attn_pool_bwd ⟵ EdgeAttention's weighted sum of the spatial edge states
 *                   (srnn_model.py:320-333, torch.bmm(h_spatials^T, attn)) and its gradient
 *   cn_spatial_attn_fwd / cn_spatial_attn_bwd ⟵ EdgeAttention's whole spatial branch (spatial_edge_layer,
 *                   att_func's scores and softmax, the pooling: srnn_model.py:256-333) in one pass over
 *                   h_spatials, and its gradient (the training and act() paths use these)
 *   cn_spatial_attn_var_fwd / cn_spatial_attn_var_bwd ⟵ (no reference counterpart) the same with a per-row
 *                   human count and temperature: the rows of envs with different crowd sizes, padded to the
 *                   largest, in one launch (observation key 'detected_human_num')
 *   cn_visible_mask ⟵ (no reference counterpart; CrowdNav++'s 'visible_masks') which humans the robot sees in the
 *                   current state: the step's own detect_visible decisions (crowd_sim.py:820-847), one launch
 *   cn_spatial_attn_mask_fwd / cn_spatial_attn_mask_bwd ⟵ (no reference counterpart) the spatial attention over the
 *                   visible slots of each row only (observation key 'visible_masks')
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (torch tensors' data_ptr()), row-major, caller-owned.
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream). Calls are
 *     stream-ordered and asynchronous; no call allocates or synchronises except cn_create/cn_destroy
 *     and the host-copy variants of get/set_state.
 *   - Every call returns 0 on success or a negative CN_E* code; cn_last_error() gives a message
 *     (thread-local). Unsupported reference options are rejected by cn_create with CN_EUNSUPPORTED.
 */
#ifndef CROWDNAV_H
#define CROWDNAV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes */
#define CN_OK 0
#define CN_EINVAL (-1)
#define CN_EUNSUPPORTED (-2)
#define CN_EHIP (-3)
#define CN_ENOMEM (-4)

/* robot kinematics  (config.action_space.kinematics, crowd_nav/configs/config.py:137) */
#define CN_HOLONOMIC 0
#define CN_UNICYCLE 1
/* human policies    (policy_factory, crowd_nav/policy/policy_factory.py:1-17) */
#define CN_POLICY_ORCA 0
#define CN_POLICY_SOCIAL_FORCE 1
/* phases            (crowd_sim.py:110-119, 690-694) */
#define CN_PHASE_TRAIN 0
#define CN_PHASE_VAL 1
#define CN_PHASE_TEST 2
/* scenarios         (create_agent_attributes, crowd_sim.py:296-357) */
#define CN_SC_CIRCLE_CROSSING 0
#define CN_SC_SQUARE_CROSSING 1
#define CN_SC_PARALLEL_TRAFFIC 2
#define CN_SC_PERPENDICULAR_TRAFFIC 3
#define CN_SC_SIDE_PREF_PASSING 4
#define CN_SC_SIDE_PREF_OVERTAKING 5
#define CN_SC_SIDE_PREF_CROSSING 6
/* scenario selection at reset (crowd_sim_dict.py:110-125) */
#define CN_SCMODE_ROUND_ROBIN 0  /* env g uses scenarios[g % n]; n == 1 is the deterministic reference case */
#define CN_SCMODE_SEQUENTIAL 1   /* test.social_metrics: scenarios[reset_count % n] (crowd_sim_dict.py:114-122) */
/* random stream of resets and goal changes (crowd_sim_dict.py:154 reseeds numpy's global RandomState) */
#define CN_RNG_MT19937 0  /* parity: numpy legacy MT19937 per env, the reference's exact draws */
#define CN_RNG_PHILOX 1   /* fast mode: Philox4x32-10, key (episode seed, 0x43726f77), counter = word / 4;
                             same draw order and distributions, different values; no 2.5 KB key per env */
/* step events (crowd_sim/envs/utils/info.py) */
#define CN_EV_NOTHING 0
#define CN_EV_DANGER 1
#define CN_EV_COLLISION 2
#define CN_EV_REACHGOAL 3
#define CN_EV_TIMEOUT 4

/* per-step info metrics, float32 [E][CN_INFO_K]  (step_info keys, crowd_sim.py:973-1030) */
#define CN_INFO_AGG_NAV_TIME 0
#define CN_INFO_PATH_VIOLATION 1
#define CN_INFO_PERSONAL_VIOLATION 2
#define CN_INFO_JERK_COST 3
#define CN_INFO_DIST_TO_GOAL 4
#define CN_INFO_SPEED_VIOLATION 5
#define CN_INFO_MIN_DIST 6     /* Danger(min_dist) payload; dmin (inf if no human counted) */
#define CN_INFO_SCENARIO 7
#define CN_INFO_SIDE_LEFT 8    /* test.side_preference only (crowd_sim.py:977-992) */
#define CN_INFO_SIDE_RIGHT 9
#define CN_INFO_SEPARATION 10
#define CN_INFO_OVERFLOW 11    /* bounded-rejection overflows of this episode before this step: its spawn's and the
                                  goal changes' of its earlier steps (engine diagnostic; the state blob's `overflow`
                                  also holds this step's, or after an auto-reset the next episode's spawn's) */
#define CN_INFO_K 12

#define CN_MAX_SCENARIOS 8

typedef struct cn_config {
    /* batch geometry */
    int32_t num_envs;      /* E: envs owned by this engine instance (one device) */
    int32_t human_num;     /* N: config.sim.human_num */
    int64_t env_offset;    /* global index of local env 0 (sharding); thisSeed = seed + global index */
    int64_t nenv;          /* the reference's env.nenv = num_processes over ALL shards (envs.py:69) */
    int64_t seed;          /* config.env.seed (envs.py:66) */
    int32_t phase;         /* CN_PHASE_*; make_env uses 'train' if nenv > 1 else 'test' (envs.py:70-73) */
    int32_t kinematics;    /* CN_HOLONOMIC / CN_UNICYCLE */
    int32_t human_policy;  /* CN_POLICY_* */
    int32_t scenario_mode; /* CN_SCMODE_* */
    int32_t num_scenarios;
    int32_t scenarios[CN_MAX_SCENARIOS];
    int32_t val_size, test_size;          /* config.env.val_size / test_size (case_size) */
    /* env (config.env / config.sim) */
    double time_step, time_limit, circle_radius, square_width;
    /* agents */
    double robot_radius, robot_vpref, robot_fov; /* fov in radians = pi * config.robot.FOV */
    double human_radius, human_vpref, human_fov;
    int32_t robot_visible, randomize_attributes;
    int32_t random_goal_changing, end_goal_changing, random_radii, random_v_pref;
    double goal_change_chance, end_goal_change_chance;
    /* reward (config.reward) */
    double success_reward, collision_penalty, discomfort_dist, discomfort_penalty_factor;
    double potential_factor, norm_zone_penalty;
    int32_t potential_based, time_factor, norm_zones, norm_zone_lhs;
    /* social (config.social / config.test) */
    double min_personal_space, max_walking_speed;
    int32_t social_metrics, side_preference;
    /* human policies (config.orca / config.sf) */
    double orca_neighbor_dist, orca_safety_space, orca_time_horizon, orca_time_horizon_obst;
    double sf_A, sf_B, sf_KI;
    /* engine */
    int32_t max_tries;     /* bounded rejection sampling (reference loops forever) */
    int32_t rng_mode;      /* CN_RNG_MT19937 (default) / CN_RNG_PHILOX */
} cn_config;

typedef struct cn_engine cn_engine;

const char *cn_last_error(void);
const char *cn_version(void);

int cn_config_validate(const cn_config *cfg);
int cn_create(const cn_config *cfg, int device, cn_engine **out);
void cn_destroy(cn_engine *eng);

/* Mixed engine: per-env scenario dispatch with per-env human counts in ONE engine (the
 * reference picks a scenario per env reset, crowd_sim_dict.py:112-125, and the side-preference scenarios
 * run with their own human count / circle radius / fixed robot, crowd_sim.py:334-357,642-651).
 * Env r (global index env_offset + r) belongs to group env_group[r]; groups[g] is a full cn_config for
 * its envs (num_envs = how many envs env_group assigns to g; env_offset / nenv / seed / phase equal across
 * groups; round-robin scenario mode with the FULL scenario list, so env r's scenario
 * scenarios[(env_offset + r) % num_scenarios] must be one group env_group[r] is configured for).
 * The engine then behaves as one engine of num_envs envs with N = max human_num: cn_reset / cn_step take
 * [num_envs]-row buffers; spatial_edges rows beyond an env's own human count are padding (a never-seen
 * human: belief (15, 15) relative to the robot). cn_step launches one step kernel per group. cn_step_seq,
 * and, once cn_mixed_scripted has enabled them, cn_robot_act, cn_rollout and cn_rollout_noisy run every group on a
 * stream of its own between one fork from and one join to the caller's stream (holonomic groups for the last
 * three), each group by the rule of a plain engine of its count.
 * cn_get_state / cn_set_state: the groups' blobs concatenated in group order; cn_state_device_ptr: NULL;
 * cn_lidar_obs / cn_lidar_scan: CN_EUNSUPPORTED. */
int cn_create_mixed(const cn_config *groups, int num_groups, const int32_t *env_group, int64_t num_envs, int device,
                    cn_engine **out);
/* per-env human count, into host memory [E] (a plain engine: N everywhere) */
int cn_env_humans(const cn_engine *eng, int32_t *dst);
/* Opt-in of a mixed engine: with on != 0, cn_robot_act, cn_rollout and cn_rollout_noisy serve it (holonomic groups)
 * as described there; off (the default, and what an engine was before this call existed) they return
 * CN_EUNSUPPORTED for it. Host state only, no launch. CN_EINVAL: NULL or a plain engine (which they always serve). */
int cn_mixed_scripted(cn_engine *eng, int on);
/* Opt-in of any engine: with on != 0, cn_robot_act, cn_rollout, cn_rollout_noisy and cn_rollout_lidar serve unicycle
 * kinematics (a plain unicycle engine; a mixed engine with a unicycle group once cn_mixed_scripted allows it at all).
 * The controller's float32 velocity (ux, uy) -- what a holonomic engine returns -- then goes through the tracking law
 * below, on the device in the same launch, and the calls return and step the unicycle action (dv, dtheta) that
 * cn_step takes. With theta = r_theta, v = r_dv of the env's state, float64 without contraction:
 *   s = norm2(ux, uy)
 *   s == 0:  a1 = 0, target = 0
 *   else:    delta = remainder(atan2(uy, ux) - theta, 2 pi)     (IEEE remainder: in [-pi, pi])
 *            a1 = clip(delta, -0.1, 0.1)
 *            target = s * max(0, cos(delta - a1))                (on the heading the step will have; never backwards)
 *   a0 = clip(target - v, -0.1, 0.1);  action = ((float)a0, (float)a1)
 * The limits are the step's own clip of a unicycle action, so that clip does not change a clean action.
 * cn_rollout_noisy's sigma is in these action units here (0.1 is the whole range): the label row keeps the clean
 * pair, `executed` and the step get the perturbed one, which the step clips.
 * Off (the default, and what an engine was before this call existed) the four calls return CN_EUNSUPPORTED for
 * unicycle kinematics. A holonomic engine computes the same either way. Host state only, no launch. CN_EINVAL: NULL. */
int cn_scripted_unicycle(cn_engine *eng, int on);

/* Reset all envs (fresh episodes, case_counter continues). obs out: robot_node [E][7], temporal [E][2],
 * spatial [E][N][2] float32. */
int cn_reset(cn_engine *eng, void *stream, float *robot_node, float *temporal_edges, float *spatial_edges);

/* One step of every env with auto-reset of finished envs.
 * in : actions [E][2] float32 (raw policy output; clipped in place semantics of SRNN.clip_action are
 *      NOT applied to the caller's buffer — the reference mutates its private numpy copy)
 * out: obs (first obs of the new episode where done), reward [E] f32, done [E] u8, event [E] i8,
 *      info [E][CN_INFO_K] f32, ep_return [E] f64 and ep_len [E] i32 (Monitor 'r'/'l', valid where done).
 * Any output pointer except the obs may be NULL. */
int cn_step(cn_engine *eng, void *stream, const float *actions,
            float *robot_node, float *temporal_edges, float *spatial_edges,
            float *reward, uint8_t *done, int8_t *event, float *info,
            double *ep_return, int32_t *ep_len);

/* T consecutive steps issued from native code: step t takes actions + t * action_stride
 * (floats; >= 2 * E, e.g. a [T][E][2] tensor), the outputs are those of the last step (each step
 * overwrites them, as T cn_step calls would). For open-loop action sequences (scripted or pre-drawn
 * actions, bench.py's synthetic windows). A plain engine with at most 10 agents per simulator runs them
 * as multi-step launches: ceil(T / C) launches whose workgroups each step their own envs up to C times
 * (cn_debug_set_seq_chunk), so no workgroup waits for the grid's slowest one after every step. Such a launch
 * stores the outputs in its last step only (the earlier steps' values would be overwritten unread), and its
 * waves rotate their issue priority from step to step, so that the workgroups sharing a CU advance alike; every
 * other engine (graph mode, > 10 agents) and the first launch after cn_reset / cn_set_state get
 * one cn_step launch per step. Either way the results are those of the T single calls, bit for bit.
 * A mixed engine: every group runs its T steps by this rule (its own count) on its own stream, one fork before the
 * first and one join after the last launch; the actions' rows and the stride are the mixed engine's. While a
 * cn_profile window is open on a mixed engine it steps as a whole, one cn_step per step. */
int cn_step_seq(cn_engine *eng, void *stream, int T, const float *actions, int64_t action_stride,
                float *robot_node, float *temporal_edges, float *spatial_edges,
                float *reward, uint8_t *done, int8_t *event, float *info,
                double *ep_return, int32_t *ep_len);

/* State blob (layout: include/crowdnav_state.h). */
/* Graph mode (on = 1): the step sequence (triple-buffered spawn-list indices, launch ids, the draw-all flag
 * after cn_reset / cn_set_state) moves from the host into device memory, so cn_step launches carry no
 * per-call arguments and a sequence of cn_step calls (with the caller's other work) can be captured once in
 * a hipGraph and replayed (learner RolloutTrainer). Costs the launch's last workgroup one atomic; off by
 * default (separate kernel variants). Plain engines only (CN_EUNSUPPORTED for cn_create_mixed). Switching
 * synchronises `stream`. No reference equivalent (its env steps are host processes). The engine issues no
 * hipMemsetAsync on a stream (graph mode's flag writes are kernels), so a capture never holds a memset node
 * from it: see cn_graph_node_counts. */
int cn_set_graph_mode(cn_engine *eng, void *stream, int on);

/* Node census of a captured hipGraph_t (`graph`): counts[k] = nodes of hipGraphNodeType k for k < n (n <= 32;
 * kernel = 0, memcpy = 1, memset = 2, ...). The rollout trainer refuses to replay a graph that holds memset
 * nodes: on this ROCm runtime a replayed memset node can write stale bytes instead of its value (DESIGN.md §4,
 * "HIP-graph memset nodes"), e.g. torch's multi-block reductions then skip writing their result. Returns the
 * total node count in *total. No reference equivalent. */
int cn_graph_node_counts(void *graph, int64_t *counts, int n, int64_t *total);

int cn_state_bytes(const cn_engine *eng, int64_t *bytes);
int cn_state_layout_offsets(const cn_config *cfg, int64_t *offsets, int64_t *total_bytes);
int cn_state_field_info(int field, const char **name, int *type_code, int *count_kind);
int cn_get_state(cn_engine *eng, void *stream, void *dst, int dst_on_host);
int cn_set_state(cn_engine *eng, void *stream, const void *src, int src_on_host);
const void *cn_state_device_ptr(const cn_engine *eng);

/* Kernel timing (measurement hook for bench.py's roofline): while enabled, cn_step records one HIP event
 * on its stream before the launch of the window's first step and one after the launch that completes its
 * `max_steps`-th step (per-launch event pairs would cost ~12 us of stream time per step; cn_step_seq splits
 * a multi-step launch at the end of the window). cn_profile_read synchronises on the closing
 * event and returns the window's span in step_kernel_ms (back-to-back launches: the summed launch
 * durations) and the number of STEPS in `launches`; rng_kernel_ms is always 0 (the RNG work is fused into
 * the step kernel). Reading an incomplete window is CN_EINVAL. */
int cn_profile(cn_engine *eng, int enable, int max_steps);
int cn_profile_read(cn_engine *eng, double *step_kernel_ms, double *rng_kernel_ms, int64_t *launches);

/* Fused DSRNN edge-feature assembly (SRNN input layers), float32, device pointers.
 *   robot_node [E][7], temporal [E][2], spatial [E][N][2]
 *   Wt [64][2] bt[64]  (humanhumanEdgeRNN_temporal.encoder_linear)
 *   Ws [64][2] bs[64]  (humanhumanEdgeRNN_spatial.encoder_linear)
 *   Wr [3][7]  br[3]   (robot_linear)
 *   Wn [64][3] bn[64]  (humanNodeRNN.encoder_linear)
 * out: temporal_embed [E][64], spatial_embed [E][N][64], node_embed [E][64]  (post-ReLU) */
int cn_edge_features(void *stream, int64_t E, int N,
                     const float *robot_node, const float *temporal_edges, const float *spatial_edges,
                     const float *Wt, const float *bt, const float *Ws, const float *bs,
                     const float *Wr, const float *br, const float *Wn, const float *bn,
                     float *temporal_embed, float *spatial_embed, float *node_embed);

/* One GRU step after the two GEMMs (nn.GRU gate order r | z | n, ATen's cell arithmetic):
 *   r = sigmoid(gh_r + gi_r), z = sigmoid(gh_z + gi_z), n = tanh(gi_n + r * gh_n), h = (hm - n) * z + n
 * gi = x W_ih^T + b_ih, gh = hm W_hh^T + b_hh: [B][3H]; hm: [B][H] (previous state times this step's mask);
 * m_next [B] (next step's mask; NULL = 1); out h_out [B][H]; hm_next [B][H] = h * m_next (NULL = skip);
 * save [B][4H] = r | z | n | gh_n for the backward (NULL = skip). H % 4 == 0. */
int cn_gru_fwd_step(void *stream, int64_t B, int H, const float *gi, const float *gh, const float *hm,
                    const float *m_next, float *h_out, float *hm_next, float *save);
/* cn_gru_fwd_step plus a second copy of the new state h_out, written in a grouped row layout: row b at
 * h_out2 + (b / g2) * ld2 + (b % g2) * H (16-byte aligned, ld2 >= g2 * H, ld2 % 4 == 0). Lets the
 * inference step write the temporal (g2 = 1) and spatial (g2 = N) edge states straight into the
 * reference's (B, N + 1, H) 'human_human_edge_rnn' layout (srnn_model.py:406-407, 450, 460) instead of
 * a torch.cat + copy; h_out2 = NULL is cn_gru_fwd_step. */
int cn_gru_fwd_step_scatter(void *stream, int64_t B, int H, const float *gi, const float *gh, const float *hm,
                         const float *m_next, float *h_out, float *hm_next, float *save, float *h_out2, int64_t g2,
                         int64_t ld2);

/* Fused step: the recurrent GEMM gh = hm W_hh^T + b_hh (w_hh [3H][H] row-major, as nn.GRU's weight_hh_l0;
 * b_hh [3H]) on the f32 matrix cores with cn_gru_fwd_step_scatter's gate epilogue, so gh never leaves the
 * chip. Same outputs and arguments as cn_gru_fwd_step_scatter otherwise; H % 32 == 0; hm, w_hh, gi, b_hh,
 * h_out, hm_next and save 16-byte aligned (float4 accesses) with rows contiguous; CN_EINVAL otherwise. Replaces torch.addmm + cn_gru_fwd_step per time step of
 * srnn_model.py:52-104's nn.GRU. */
int cn_gru_fwd_fused(void *stream, int64_t B, int H, const float *gi, const float *hm, const float *w_hh,
                     const float *b_hh, const float *m_next, float *h_out, float *hm_next, float *save, float *h_out2,
                     int64_t g2, int64_t ld2);

/* Gradient of one step. In: acc [B][H] = dL/dhm of the later step (or dL/dh_T at the last step, with
 * m_next = NULL), m_next [B] that later step's mask, dout [B][H] = dL/dh_t from the outputs (NULL = 0),
 * save / hm as written by the forward. Out: dgi, dgh [B][3H] (pre-activation gradients of gi, gh) and
 * acc <- dL/dh_t * z (the caller then adds dgh W_hh to obtain dL/dhm_t). */
int cn_gru_bwd_step(void *stream, int64_t B, int H, float *acc, const float *m_next, const float *dout,
                    const float *save, const float *hm, float *dgi, float *dgh);
/* cn_gru_bwd_step with the bias gradients folded in: the same dgi_t / dgh_t / acc, plus the column sums of
 * dr | dz | dn | dhn of every 16-row block to part [cn_gru_bias_blocks(B)][4H] (H in {64, 128, 256}); after
 * the last step cn_gru_bias_reduce sums the partials of all steps, part [rows][4H], in a fixed order into
 * db_ih = (dr, dz, dn) and db_hh = (dr, dz, dhn) sums ([3H] each; work: cn_gru_bias_work_elems(H) floats).
 * Replaces the reference autograd's two extra passes over [T][B][3H] (dgi.sum(0), dgh.sum(0)). */
int64_t cn_gru_bias_blocks(int64_t B);
int cn_gru_bwd_step_bias(void *stream, int64_t B, int H, float *acc, const float *m_next, const float *dout,
                         const float *save, const float *hm, float *dgi, float *dgh, float *part);
/* cn_gru_bwd_step_bias with the gate gradients stored once, g [B][4H] = [dn | dr | dz | dhn] per row:
 * dgh_t = g[:, H:4H] and dgi_t = g[:, 0:3H] in gate order (n, r, z) (dgi's r / z columns equal dgh's), 2H
 * fewer floats written per row than the separate dgi / dgh. Same acc and bias partials. */
int cn_gru_bwd_step_gates(void *stream, int64_t B, int H, float *acc, const float *m_next, const float *dout,
                          const float *save, const float *hm, float *g, float *part);
int64_t cn_gru_bias_work_elems(int H);
int cn_gru_bias_reduce(void *stream, int64_t rows, int H, const float *part, float *db_ih, float *db_hh,
                       float *work);

/* The act() tail of the Box-action policy (distributions.py:74-94: DiagGaussian with AddBias(zeros) log-std,
 * FixedNormal.sample / .mode and .log_probs) for E envs in one launch: std = exp(logstd) [A],
 * action = eps * std + mean (eps [E][A] from the caller's N(0, 1) draw) or mean when eps = NULL,
 * logp [E] = sum over the A dims of the Normal log-density of action, in torch's float32 operation order.
 * mean, eps, action: [E][A]; A <= 64. */
int cn_gaussian_act(void *stream, int64_t E, int A, const float *mean, const float *logstd, const float *eps,
                    float *action, float *logp);

/* The lattice action head of the unicycle robot (no reference counterpart: this project's definition; the policy's
 * opt-in robot.action_head = 'lattice'): a categorical distribution over the 64 actions cn_dwa_predict chooses from.
 * Candidate c = 8 a + b, a, b in 0..7, is the action ((float)((0.1 * (2 a - 7)) / 7), (float)((0.1 * (2 b - 7)) / 7)):
 * cn_dwa_predict's numbering and values, bit for bit. For one row l of 64 float32 logits, in float32:
 *   m = max l,  p_j = expf(l_j - m),  Z = sum p_j,  logp_j = (l_j - m) - logf(Z)
 *   mode     the c of the largest logit, the lowest c among equal ones
 *   sample   with u in [0, 1) from the caller and S_c the inclusive prefix sums of p: the smallest c with
 *            S_c > u * S_63; if rounding leaves none, the highest c with p_c > 0. A candidate with p_c == 0 is never
 *            chosen
 *   index of an action (x, y): a = clamp(rintf((x * 70 + 7) * 0.5), 0, 7) and b from y the same way: the nearest
 *            lattice point, exact for every lattice point (cn_dwa_predict's labels among them)
 *   entropy  H = -sum over p_j > 0 of (p_j / Z) * logp_j
 *   backward with upstream g_lp, g_H and q = p / Z:  dl_j = g_lp * (delta_jc - q_j) - g_H * q_j * (logp_j + H), the
 *            terms with q_j == 0 being 0
 * The order of the 64-term sums is the kernels' own (xor butterflies for Z and H, a shuffle scan for S), so a result
 * agrees with another evaluation of the definition to float32 rounding of such a sum, not bit for bit.
 * cn_lattice_act: the act() tail for E rows in one launch: logits [E][64], u [E] or NULL (NULL: the mode);
 *   out action [E][2] (the lattice point of c), logp [E] (logp_c), choice [E] int32 (c; may be NULL).
 * cn_lattice_eval_fwd: evaluate_actions for B rows: actions [B][2] -> logp [B] of the action's index, entropy [B],
 *   choice [B] (that index, for the backward).
 * cn_lattice_eval_bwd: dlogits [B][64] from the same logits, the forward's choice, g_logp [B] and g_entropy [B]
 *   (nothing but the logits is kept between the two: the softmax is recomputed).
 * One 64-lane wavefront per row, a lane per candidate, 4 rows per workgroup; no LDS, scratch, atomics or memset.
 * Device pointers, stream-ordered. CN_EINVAL, before any launch: a row count <= 0 or above 4 * (2^31 - 1), or a NULL
 * pointer other than u / cn_lattice_act's choice. */
int cn_lattice_act(void *stream, int64_t E, const float *logits, const float *u, float *action, float *logp,
                   int32_t *choice);
int cn_lattice_eval_fwd(void *stream, int64_t B, const float *logits, const float *actions, float *logp,
                        float *entropy, int32_t *choice);
int cn_lattice_eval_bwd(void *stream, int64_t B, const float *logits, const int32_t *choice, const float *g_logp,
                        const float *g_entropy, float *dlogits);

/* Soft labels for the lattice head (no reference counterpart: this project's definition). The target is the
 * distribution the expert's regrets define at a temperature tau > 0 (inv_tau = 1 / tau): for one row l of 64 float32
 * logits and one row r of 64 float32 regrets (cn_robot_act_regret's, or any row of non-negative costs), in float32:
 *   a_j = r_j - min r,  x_j = -(a_j * inv_tau),  t_j = expf(x_j),  Zt = sum t_j,  q_j = t_j / Zt
 *            (the shift makes a row from any source safe: the best candidate has t = 1, so Zt >= 1; it changes
 *             nothing on an engine row, whose minimum is +0.0)
 *   logp_j   cn_lattice_eval_fwd's:  m = max l,  p_j = expf(l_j - m),  Z = sum p_j,  logp_j = (l_j - m) - logf(Z)
 *   ce       = -sum over q_j > 0 of q_j * logp_j                        (the cross-entropy H(q, softmax l))
 *   Hq       = -sum over q_j > 0 of q_j * (x_j - logf(Zt)),  kl = ce - Hq   (KL(q || softmax l); >= 0 up to rounding)
 *   logp_best = logp_j at the lowest j with a_j == 0: on an engine row the expert's label, so the hard-label
 *            negative log-likelihood is reported by the same pass
 *   backward with upstream g on ce:  dl_j = g * (p_j / Z - q_j). There is no gradient to the regrets, and kl and
 *            logp_best are reported values without one.
 * A candidate whose t_j underflows has q_j == 0 and adds nothing (no 0 * -inf). tau -> 0 is not served: inv_tau must
 * be finite and > 0, and the hard label is cn_lattice_eval_fwd's path. The order of the 64-term sums is the kernels'
 * own (xor butterflies), as for the three calls above.
 * cn_lattice_soft_fwd: B rows, logits [B][64], regret [B][64] -> ce [B], kl [B] (may be NULL), logp_best [B] (may be
 *   NULL).
 * cn_lattice_soft_bwd: dlogits [B][64] from the same logits and regrets and g_ce [B] (nothing else is kept between
 *   the two: both softmaxes are recomputed).
 * One 64-lane wavefront per row, a lane per candidate, 4 rows per workgroup; no LDS, scratch, atomics or memset.
 * Device pointers, stream-ordered. CN_EINVAL, before any launch: cn_lattice_eval_fwd's row rule, a NULL pointer other
 * than kl / logp_best, an inv_tau that is not finite or not > 0. */
int cn_lattice_soft_fwd(void *stream, int64_t B, const float *logits, const float *regret, float inv_tau, float *ce,
                        float *kl, float *logp_best);
int cn_lattice_soft_bwd(void *stream, int64_t B, const float *logits, const float *regret, float inv_tau,
                        const float *g_ce, float *dlogits);

/* One step of up to two GRUs of the same H in one launch (the act() path's temporal and spatial edge RNNs,
 * srnn_model.py:455-460 at T = 1): cn_gru_fwd_fused per GRU, with the input projection in the kernel when
 * x is given (gi NULL: x [B][F], w_ih [3H][F], b_ih [3H], F % 32 == 0; every GRU of a call in the same mode)
 * and the optional grouped copy h_out2 (g2, ld2) of cn_gru_fwd_step_scatter. No mask / save outputs. */
typedef struct cn_gru_step_seg {
    int64_t B;
    const float *gi;
    const float *x;
    const float *w_ih;
    const float *b_ih;
    int64_t F;
    const float *hm;     /* [B][H] masked state */
    const float *w_hh;
    const float *b_hh;
    float *h_out;        /* [B][H] */
    float *h_out2;       /* grouped copy or NULL */
    int64_t g2;
    int64_t ld2;
} cn_gru_step_seg;
int cn_gru_fwd_step_group(void *stream, int H, int nseg, const cn_gru_step_seg *segs);

/* Returns by generalized advantage estimation (storage.py:132-177 compute_returns with use_gae), one launch
 * for the whole rollout: rewards [T][E], values / masks / bad_masks [T + 1][E] (values[T] = next_value),
 * returns [T + 1][E] (rows 0 .. T-1 written); the reference's float32 operation order per step, with gamma and
 * gamma_lambda = gamma * gae_lambda as float32 scalars; use_proper_time_limits multiplies by bad_masks. */
int cn_gae(void *stream, int T, int64_t E, float gamma, float gamma_lambda, int use_proper_time_limits,
           const float *rewards, const float *values, const float *masks, const float *bad_masks, float *returns);

/* Whole sequences: the T-step loops of srnn_model.py:52-104's nn.GRU (forward) and of its autograd backward
 * issued from native code, one launch per step for up to two independent GRUs of the same H at once (the
 * DSRNN's spatial and temporal edge RNNs, srnn_model.py:455-460; their rows share each launch). H % 32 == 0;
 * every array 16-byte aligned with rows contiguous; 1 <= nseg <= 2. */
typedef struct cn_gru_seq_fwd {
    int64_t B;           /* rows */
    const float *gi;     /* [T][B][3H] = x W_ih^T + b_ih, or NULL: the kernel projects x itself (below) */
    const float *w_hh;   /* [3H][H] (weight_hh_l0) */
    const float *b_hh;   /* [3H] */
    const float *m;      /* [T][B] masks */
    float *out;          /* [T][B][H] outputs */
    float *hm;           /* [nh][B][H] masked states: hm[0] = h0 * m[0] (caller); step t reads hm[t % nh] and
                            writes hm[(t + 1) % nh] = h_t * m[t + 1] (nh = T keeps all of them for the backward) */
    float *save;         /* [T][B][4H] r | z | n | gh_n per step for the backward, or NULL */
    int64_t nh;          /* 1 <= nh <= T; nh >= 2 when T > 1 (a step's workgroups read hm[t % nh] while others
                            write hm[(t + 1) % nh]); nh == T when save is not NULL (the backward reads every hm) */
    const float *x;      /* [T][B][F] GRU inputs when gi is NULL (then gi is never stored: the step kernel runs */
    const float *w_ih;   /* x W_ih^T on the MFMA ahead of hm W_hh^T); w_ih [3H][F] (weight_ih_l0), b_ih [3H], */
    const float *b_ih;   /* F % 32 == 0. Every GRU of a call uses the same mode. */
    int64_t F;
} cn_gru_seq_fwd;
/* cn_gru_fwd_fused for t = 0 .. T - 1 (same arithmetic per row and step; like cn_gru_fwd_fused, a launch with
 * fewer 128-row tiles than CUs splits K over the workgroup's waves on 32-row tiles). */
int cn_gru_fwd_seq(void *stream, int T, int H, int nseg, const cn_gru_seq_fwd *segs);

typedef struct cn_gru_seq_bwd {
    int64_t B;
    const float *w_hh_t; /* [H][3H] = weight_hh_l0 transposed */
    const float *m;      /* [T][B] masks */
    const float *dout;   /* [T][B][H] dL/d out, or NULL */
    const float *save;   /* [T][B][4H] and */
    const float *hm;     /* [T][B][H] as written by cn_gru_fwd_seq (nh = T) */
    float *acc;          /* [B][H] in: dL/dh_{T-1} through the final state (zeros if unused);
                            out: dL/d hm_0 (the caller multiplies by m[0] for dL/dh0) */
    float *g;            /* [T][B][4H] out: dn | dr | dz | dhn per step (dgh_t = g[t][:, H:4H], dgi_t = g[t][:, 0:3H]
                            in gate order n, r, z) */
    float *db_ih;        /* [3H] out: the bias gradients (sums over all T * B rows, fixed order) */
    float *db_hh;        /* [3H] out */
} cn_gru_seq_bwd;
/* floats of workspace cn_gru_bwd_seq needs for these GRUs (reads only the B fields; the row tiling follows the
 * current device's CU count, so query on the device the backward runs on) */
int64_t cn_gru_bwd_seq_work_elems(int T, int H, int nseg, const cn_gru_seq_bwd *segs);
/* The backward of cn_gru_fwd_seq: T + 1 launches of one fused kernel, each the recurrent GEMM
 * acc_t = a_t + dgh_t W_hh of one step on the f32 matrix cores with the gate gradients of the step before in
 * its epilogue (cn_gru_bwd_step_gates' arithmetic; launches with fewer 128-row tiles than CUs split K over
 * the workgroup's waves on 32-row tiles), then the bias reduction; replaces the per-step
 * cn_gru_bwd_step_gates + GEMM pair. work_elems = the floats at work; fails (CN_EINVAL) when it is below
 * cn_gru_bwd_seq_work_elems on the current device. */
int cn_gru_bwd_seq(void *stream, int T, int H, int nseg, const cn_gru_seq_bwd *segs, float *work, int64_t work_elems);

/* The ConvGRU observation row of every env, obs [E][7 + beams] float32:
 *   [clip(robot (px, py, radius, gx, gy, v_pref, theta) / max_range, 0, 1), scan].
 * lidar [E][beams] (caller-owned, zero-initialised) holds each env's current scan
 * |1 - clip(dist / max_range, 0, 1)|. For envs with reset_mask[e] != 0 (NULL = all envs, i.e. after
 * cn_reset; pass the `done` output of cn_step after a step) the observation carries the scan held so far
 * and the scan is then retaken from the engine state — the reference builds reset()'s observation before
 * it spins the sensor (crowd_sim_dict.py:166-191), at robot heading 0, against the last human and the
 * world walls. Other envs get the held scan. enable = 0: scans stay zero (config.lidar.enable False).
 * Call after cn_reset / cn_step on the same stream. */
int cn_lidar_obs(cn_engine *eng, void *stream, const uint8_t *reset_mask, int enable, int beams, double max_range,
                 double robot_radius, float *lidar, float *obs);

/* The live ConvGRU observation row of every env, obs [E][7 + beams] float32, same layout as cn_lidar_obs:
 *   [clip(robot (px, py, radius, gx, gy, v_pref, theta) / max_range, 0, 1), |1 - clip(dist / max_range, 0, 1)|]
 * with the scan of the engine's CURRENT state: the one CrowdSimDict.step() computes every step and discards
 * (crowd_sim_dict.py:224-251) — the sensor at the robot's position, heading atan2(vy, vx) (0 right after a
 * reset), all N
 * humans in index order and the walls of the square world, lidarv2.py's semantics in float64: per-obstacle
 * angular windows with their in-place flip, only the obstacle with the nearest centre among those whose
 * window holds the beam is sampled (every 0.01 m, first sample strictly inside), else the first wall crossed
 * within range, never inside robot_radius. Nothing is held between calls: call it after cn_reset / cn_step /
 * cn_set_state on the same stream; envs that auto-reset in that step show their new episode. One launch,
 * no synchronisation and no allocation (graph-capturable). beams in [2, 4096], max_range in (0, 1e4].
 * A mixed engine: CN_EUNSUPPORTED. */
int cn_lidar_scan(cn_engine *eng, void *stream, int beams, double max_range, double robot_radius, float *obs);

/* Test hook: the norm-zone predicate of the step kernel, robot 64-gon (GEOS Point.buffer(r)) vs convex quad
 * (crowd_sim.py norm-zone penalty), for n cases on the device: px, py, r [n], qx, qy [n][4],
 * out [n] (1 = intersecting). mode 0: the kernel's function (classification + separating axes), mode 1:
 * the separating-axis test alone. Checked against oracle/cpu_ref.c:disc_quad_intersect in tests/.
 * mode 2: the step kernel's whole norm-zone penalty predicate (both zones built around the robot,
 * crowd_sim.py:918-926): robot at (px, py) of radius r with velocity (qx[i][0], qy[i][0]), float32 heading
 * if qx[i][1] != 0, zone side preference lhs = qy[i][1]. */
int cn_debug_disc_quad(void *stream, int64_t n, int mode, const double *px, const double *py, const double *r,
                       const double *qx, const double *qy, int32_t *out);

/* Test hook (SURVEY Appendix A.4 known answers): agent 0's new velocity of n independent RVO2 simulators
 * of A <= 10 agents each (crowd_nav/policy/orca.py:92-136: addAgent / setAgentPrefVelocity / doStep /
 * getAgentVelocity(0)), through the step kernel's own code path (quad-cooperative neighbour ranking and
 * ORCA lines, linearProgram2, linearProgram3). agents [n][A][5] = (px, py, vx, vy, radius) with agent 0 =
 * self; self [n][3] = (maxSpeed, prefVelocity.x, prefVelocity.y); neighbor_dist, time_horizon, time_step
 * as in PyRVOSimulator. out [n][4] = (vx, vy, index of the line linearProgram2 failed at or the line
 * count when it succeeded, the line count). Checked against oracle/cpu_ref.c:cnref_rvo2_agent0 and hand-derived answers. */
int cn_debug_orca(void *stream, int64_t n, int A, const float *agents, const float *self, float neighbor_dist,
                  float time_horizon, float time_step, float *out);

/* Agent policy plugin (replaces policy_factory[name](config).predict(JointState),
 * crowd_nav/policy/policy_factory.py:1-17; host side crowdnav_dsrnn_amd/policy_factory.py).
 * cn_orca_predict: ORCA.predict (crowd_nav/policy/orca.py:64-139) of n independent simulators of A <= 64
 *   agents, arguments and outputs as cn_debug_orca (the caller keeps the simulator's frozen radii and max
 *   speed, orca.py:85-115). A > 10 runs cn_orca_predict_kd with a fresh simulator's (identity) KdTree order.
 * cn_orca_predict_kd: the same for simulators of A <= 64 agents through RVO2's KdTree (MAX_LEAF_SIZE 10),
 *   whose build re-permutes the simulator's persisted agent order (KdTree::agents_): perm [n][A] uint8 holds
 *   each simulator's order on entry (identity for a simulator created by this predict) and the re-permuted
 *   order on return, so a caller that keeps one simulator across predicts (orca.py:85-90: the simulator
 *   lives until the agent count changes) passes it back next time. perm = NULL: identity, not written.
 *   Caller side: crowd_sim.py:1121-1161 passes N-1 humans (+ the robot when robot.visible), i.e. A = N or N+1.
 * cn_social_force_predict: SOCIAL_FORCE.predict (crowd_nav/policy/social_force.py:11-66) of n agents,
 *   float64: self [n][9] = FullState (px, py, vx, vy, radius, gx, gy, v_pref, theta), others [n][M][5] =
 *   ObservableState (px, py, vx, vy, radius), A / B / KI = config.sf, time_step = config.env.time_step;
 *   out [n][2] = the ActionXY (vx, vy). Device pointers, stream-ordered. */
int cn_orca_predict(void *stream, int64_t n, int A, const float *agents, const float *self, float neighbor_dist,
                    float time_horizon, float time_step, float *out);
int cn_orca_predict_kd(void *stream, int64_t n, int A, const float *agents, const float *self, float neighbor_dist,
                       float time_horizon, float time_step, uint8_t *perm, float *out);
int cn_social_force_predict(void *stream, int64_t n, int M, const double *self, const double *others, double A,
                            double B, double KI, double time_step, double *out);

/* The dynamic-window controller of the unicycle robot (no reference counterpart: this project's definition). It plans
 * in the unicycle's own action space with the step's own kinematics: the 64 candidate actions of one step, each held
 * over a horizon of H steps, against a constant-velocity forecast of the humans. Per env, float64 without contraction,
 * every sum and product evaluated left to right as written:
 *   robot  px, py, theta, v (the engine's r_theta and r_dv), r = radius, goal (gx, gy), vpref;  dt = time_step
 *   humans i < M: (bx, by, bvx, bvy, br)
 *   candidate c = 8 a + b, a, b in 0..7:  dv = (0.1 * (2 a - 7)) / 7,  dth = (0.1 * (2 b - 7)) / 7
 *     (both inside the step's clip range [-0.1, 0.1]; |dth| >= 0.1 / 7, so no candidate falls below the step's
 *      |dtheta| < 1e-4 rule, under which a unicycle robot does not move at all)
 *   forecast:  v1 = clip(v + dv, -vpref, vpref),  R = v1 / (dth / dt)
 *     for k = 1..H:  phi = theta + k * dth
 *                    x_k = px - R * sin(theta) + R * sin(phi),  y_k = py + R * cos(theta) - R * cos(phi)
 *     (k = 1 is the step's own arc, which is then held);  human i at step k: (bx + k * dt * bvx, by + k * dt * bvy)
 *   walk, k upwards, from cmin = +inf, hit = 0:
 *     c_k = min over i of sqrt(dx * dx + dy * dy) - r - br_i       (+inf when M = 0; dx, dy = robot minus human)
 *     cmin = min(cmin, c_k);  if c_k < 0 and hit == 0: hit = H + 1 - k
 *     g_k = sqrt(dx * dx + dy * dy) of (x_k, y_k) minus the goal;  gterm = g_k
 *     if g_k < r: gterm = 0 and the walk stops
 *   cost   J = w_goal * gterm + (w_clear * max(0, d_safe - cmin)) / d_safe + w_col * hit
 *   choice the candidate of the smallest J, the lowest c among equal ones;  action = ((float)dv, (float)dth)
 * A state or parameter set that makes a J NaN has no defined choice.
 * cn_dwa_predict: the controller on arrays, n envs of M humans each (0 <= M <= 64, n < 2^31): self [n][9] as
 *   cn_social_force_predict's (vx, vy are not read), v [n] = r_dv, others [n][M][5] (may be NULL when M = 0);
 *   out actions [n][2] float32, choice [n] int32 (the chosen c; may be NULL), costs [n][64] (every candidate's J; may
 *   be NULL). One launch, one 64-lane wavefront per env, a lane per candidate. Device pointers, stream-ordered.
 *   CN_EINVAL: n <= 0, a NULL required buffer, M out of range, p NULL or bad: horizon outside [1, 16], d_safe <= 0 or
 *   not finite, a weight not finite. */
typedef struct cn_dwa_params {
    int32_t horizon;      /* H: steps of the forecast, 1..16 */
    double  w_goal;       /* weight of the distance to the goal where the walk ends */
    double  w_clear;      /* weight of the clearance shortfall max(0, d_safe - cmin) / d_safe */
    double  d_safe;       /* clearance (m) from which on a candidate pays nothing; > 0 */
    double  w_col;        /* weight of a forecast collision, times the steps left when it happens (+ 1) */
} cn_dwa_params;
int cn_dwa_predict(void *stream, int64_t n, int M, const double *self, const double *v, const double *others,
                   double time_step, const cn_dwa_params *p, float *actions, int32_t *choice, double *costs);

/* Scripted robot baselines on the device (the "for orca and sf" robot the reference's env anticipates,
 * crowd_sim.py:1113-1114,1185-1188 -> robot.py:9-15, and then crashes on: those policies have no clip_action).
 * actions [E][2] float32 = for every env e, rounded to float32, what a FRESH policy object returns for the
 * engine's current state:
 *   policy_factory[name](config).predict(JointState(robot FullState (r_px, r_py, r_vx, r_vy, r_radius, r_gx,
 *       r_gy, r_vpref, r_theta), [ObservableState(b_px, b_py, b_vx, b_vy, b_r) of the N humans in index order]))
 * i.e. the robot acts on its belief (last_human_states). CN_ROBOT_ORCA: ORCA.predict (orca.py:64-139) as
 * cn_orca_predict computes it -- positions, velocities and radii (float)((radius + 0.01) + safety_space) cast
 * to float32, maxSpeed (float)r_vpref, the preferred velocity towards the goal in float64 (normalised only
 * above speed 1) then float32; neighbor_dist / time_horizon / time_step from the engine's cn_config; N + 1 <= 10
 * agents on the quad path, more through RVO2's KdTree in a fresh simulator's identity agent order
 * (cn_orca_predict_kd with perm = NULL). CN_ROBOT_SOCIAL_FORCE: SOCIAL_FORCE.predict (social_force.py:11-66)
 * in float64 with sf_A / sf_B / sf_KI / time_step from the cn_config, as cn_social_force_predict.
 * A pure function of the state blob, read in place: nothing is held between calls; one launch, no allocation,
 * no synchronisation, no memset (graph-capturable next to cn_step). Call it after cn_reset / cn_step /
 * cn_set_state on the same stream and feed `actions` to cn_step for a closed loop without a host round trip.
 * Two deliberate deviations from ONE reference ORCA object kept alive over an episode:
 *   - the simulator is new at every call, so the KdTree agent order does not persist from step to step (it
 *     only orders equidistant neighbours, and only when N + 1 > 10);
 *   - the radii follow the current belief instead of being frozen at the object's first predict (identical
 *     unless humans.random_radii).
 * A mixed engine after cn_mixed_scripted(eng, 1): one launch per group, side by side (group 0 on `stream`, the others
 * forked from and joined to it), each with the kernel its own count selects; env r's action at row r of `actions`.
 * A unicycle engine after cn_scripted_unicycle(eng, 1): `actions` holds the unicycle action (dv, dtheta) its tracking
 * law derives from the controller's velocity.
 * CN_EUNSUPPORTED: a unicycle engine (the controllers return ActionXY), a mixed engine without that opt-in or with a
 * unicycle group (unicycle: unless cn_scripted_unicycle enabled it);
 * CN_EINVAL: an unknown policy or actions = NULL.
 * CN_ROBOT_DWA, on an engine cn_scripted_dwa enabled it for (before that the id is an unknown policy: CN_EINVAL):
 * cn_dwa_predict's controller with that call's parameters on the robot (r_px, r_py, r_theta, r_dv, r_radius, r_gx,
 * r_gy, r_vpref), its belief of the N humans and the config's time_step; `actions` holds the unicycle action
 * (dv, dtheta). No tracking law is involved, so cn_scripted_unicycle is not needed; a mixed engine still needs
 * cn_mixed_scripted. One launch (a mixed engine: one per group), as for the other two. */
#define CN_ROBOT_ORCA 0
#define CN_ROBOT_SOCIAL_FORCE 1
#define CN_ROBOT_DWA 2
int cn_robot_act(cn_engine *eng, void *stream, int policy, float *actions);
/* Opt-in of a unicycle engine: with p != NULL, cn_robot_act, cn_rollout, cn_rollout_noisy and cn_rollout_lidar accept
 * CN_ROBOT_DWA for it and run the controller with *p (copied); p = NULL switches it off again (the default, and what
 * an engine was before this call existed: the id is CN_EINVAL). Policies 0 and 1 are not affected. Host state only,
 * no launch. CN_EINVAL: eng NULL or bad parameters (cn_dwa_predict's rule); CN_EUNSUPPORTED: p != NULL on an engine
 * with holonomic envs (the controller emits (dv, dtheta)). */
int cn_scripted_dwa(cn_engine *eng, const cn_dwa_params *p);

/* The learner in the loop (DAgger, Ross et al. 2011): the scripted controller labels the engine's current state and
 * a per-env coin decides whether its action or the learner's is the one to execute. For env e (global index
 * G = env_offset + e; a mixed engine: its row, as cn_rollout_noisy keys its noise) and k = (uint32)(ctl->step0 + t):
 *   label[e]    = what cn_robot_act(eng, stream, policy, label) writes, bit for bit (it IS that call)
 *   w           = philox4x32_10(counter k, key (seed, (uint32)G))      (cn_rollout_noisy's block)
 *   u           = (float)(w.z >> 8) * 2^-24                            (exact in float32, in [0, 1))
 *   took        = u < beta                                             (beta = 0: never; beta = 1: always, exactly)
 *   executed[e] = took ? label[e] : learner[e]                         (copied as bits: a -0.0f keeps its sign)
 *   flags[e]    = took | (learner[e] == label[e] in both components, as bits) << 1
 * Word z, because x and y are cn_rollout_noisy's: a noisy rollout and a mixed one on the same seed stay independent.
 * Bit 1 is the closed-loop agreement: with a lattice head and CN_ROBOT_DWA, the classifier's on-policy accuracy.
 * beta, seed and step0 are read from DEVICE memory when the kernel runs; only t is a launch argument. A captured
 * graph of calls at t = 0..T-1 therefore replays with whatever cn_mix_ctl_set wrote before the replay.
 * cn_mix_ctl_set: *dev = *value by one small launch on the stream (by value: no host memory is read later, no
 * memset or memcpy node when captured). CN_EINVAL: dev or value NULL, beta outside [0, 1] or not finite.
 * cn_robot_mix: cn_robot_act's launch(es) into `label` (a mixed engine: one per group, joined), then ONE launch over
 * all E rows: a lane per env in 256-lane workgroups, 8-byte loads and stores of the action pairs (learner, label
 * and executed 8-byte aligned; the three and flags must not overlap), the block read wave-uniformly; no LDS, no
 * atomics. Stream-ordered; no allocation, no synchronisation, no memset; capturable. No engine state changes.
 * CN_EINVAL: a NULL pointer, t < 0, an unknown policy (CN_ROBOT_DWA without cn_scripted_dwa included);
 * CN_EUNSUPPORTED: cn_robot_act's (a mixed engine without cn_mixed_scripted, a unicycle engine without
 * cn_scripted_unicycle). All are checked before any launch. */
typedef struct cn_mix_ctl {   /* 16 bytes, lives in DEVICE memory, owned by the caller */
    float    beta;    /* probability that the expert's action is the one executed; 0 <= beta <= 1 */
    uint32_t seed;
    int64_t  step0;   /* index of step t = 0 in the caller's coin sequence */
} cn_mix_ctl;
int cn_mix_ctl_set(void *stream, cn_mix_ctl *dev, const cn_mix_ctl *value);
int cn_robot_mix(cn_engine *eng, void *stream, int policy, const float *learner /*[E][2]*/,
                 const cn_mix_ctl *ctl /*device*/, int32_t t,
                 float *label /*[E][2]*/, float *executed /*[E][2]*/, uint8_t *flags /*[E]*/);

/* The controller's whole cost row beside its action (soft labels; cn_lattice_soft_fwd consumes it). For one env, with
 * J_c the float64 costs of cn_dwa_predict's 64 candidates on the engine's current state (cn_dwa_predict's `costs`) and
 * b its choice:
 *   regret[c] = (float)(J_c - J_b)        the subtraction in float64, the rounding to float32 the only rounding
 * so regret[b] == +0.0f exactly, every entry is >= 0 (b has the smallest J), and candidates tied with b are 0 as well.
 * Subtracting before rounding keeps near-ties resolved where J itself is large (a forecast collision adds ~1000 to
 * every candidate of an env alike). A row is 64 floats, 256 contiguous bytes: regret [E][64], env e's at row e.
 * cn_robot_act_regret: cn_robot_act(eng, stream, policy, actions) with the controller's regret kernel in place of
 *   the plain one -- the same launch count, not a second controller launch; `actions` is bit for bit what cn_robot_act
 *   writes. Each wave stores its env's row as one coalesced 256-byte store.
 * cn_robot_mix_regret: cn_robot_mix with that launch in place of cn_robot_act's; label, executed and flags are bit for
 *   bit cn_robot_mix's.
 * A mixed engine after cn_mixed_scripted: one launch per group, env r's row at row r of `regret`. Stream-ordered; no
 * allocation, no synchronisation, no memset; capturable. No engine state changes. All checks come before any launch:
 * CN_EINVAL: a NULL pointer, t < 0, an unknown policy, CN_ROBOT_DWA without cn_scripted_dwa;
 * CN_EUNSUPPORTED: CN_ROBOT_ORCA or CN_ROBOT_SOCIAL_FORCE (they have no candidate set), and whatever cn_robot_act
 * refuses (a mixed engine without cn_mixed_scripted). */
int cn_robot_act_regret(cn_engine *eng, void *stream, int policy, float *actions /*[E][2]*/, float *regret /*[E][64]*/);
int cn_robot_mix_regret(cn_engine *eng, void *stream, int policy, const float *learner /*[E][2]*/,
                        const cn_mix_ctl *ctl /*device*/, int32_t t, float *label /*[E][2]*/,
                        float *executed /*[E][2]*/, uint8_t *flags /*[E]*/, float *regret /*[E][64]*/);

/* Which humans the robot sees in the state the engine now holds (after cn_reset / cn_step / cn_step_seq /
 * cn_set_state): mask [E][NS] float32, NS = the padded human stride of the observation (N; a mixed engine: its
 * largest count), 1.0 where the robot sees human i of env e, 0.0 otherwise and in the padded slots. It is
 * detect_visible(robot, human, robot1=True) (crowd_sim.py:820-847) as the step itself evaluated it when it wrote
 * that state's belief (b_*): recomputed from r_px, r_py, r_vx, r_vy, r_theta, flags, h_px, h_py and robot_fov with
 * the step's own device functions -- the float32 heading once the robot carries its float32 state, the float64 reset
 * path before. mask == 1 implies b_* == the human's true state bit for bit; the converse does not hold (an invisible
 * human that keeps its velocity is extrapolated exactly), which is why the mask is not derivable from the
 * observation. Reads the state only. One launch (a mixed engine: one per group, group 0 on `stream`, the others
 * forked from and joined to it, no opt-in needed). Stream-ordered; no allocation, no synchronisation, no memset;
 * capturable (graph mode: one more kernel node). CN_EINVAL: eng or mask NULL (before any launch). */
int cn_visible_mask(cn_engine *eng, void *stream, float *mask);

/* Closed-loop scripted rollout: T steps of the scripted robot driving the engine, every step recorded. For
 * t = 0..T-1 the call does cn_robot_act(eng, stream, policy, actions_t) and then cn_step(eng, stream, actions_t,
 * ...row t of every output...); every recorded row and the state blob afterwards equal that pair sequence bit for
 * bit. actions[t] is computed from the state BEFORE step t (right after an auto-reset: the new episode's); an env
 * that finishes in step t carries its new episode's first observation in row t, as cn_step returns it. The pairing
 * for imitation data is therefore observation row t-1 -> actions row t (row -1: cn_reset's observation).
 * Stream-ordered; no allocation, no synchronisation, no memset. *num_launches (host, may be NULL) receives the
 * number of kernel launches issued.
 *   Fused path: a plain holonomic engine on the step's quad path (at most 10 agents per simulator) outside graph
 * mode, with a controller that fits the step workgroup (social force always; ORCA with N + 1 <= 10), runs
 * ceil(T' / C) launches of up to C = seq_chunk steps (cn_debug_set_seq_chunk; split at the end of a cn_profile
 * window, as cn_step_seq's): each step workgroup computes the actions of its own envs from the state its previous
 * step wrote, with cn_robot_act's arithmetic, then steps them, so no workgroup waits for the grid's slowest one
 * and no controller launch is issued. T' excludes a first step after cn_reset / cn_set_state, which is a pair.
 *   Everything else cn_robot_act supports (chunk 1, graph mode, > 10 agents per simulator, ORCA at N + 1 > 10) is
 * issued as T cn_robot_act + cn_step launch pairs from native code with the output pointers advanced to row t:
 * the same rows.
 *   A mixed engine after cn_mixed_scripted(eng, 1): every group runs its own T-step sequence on its own stream (one
 * fork, one join per call), fused
 * where its own count allows and as launch pairs otherwise, its envs at their rows of the (T, E, ..) buffers
 * (spatial_edges padded to the largest count, the padding written as cn_step writes it); *num_launches counts the
 * launches of all groups. While a cn_profile window is open on it: launch pairs, a step at a time.
 *   A unicycle engine after cn_scripted_unicycle(eng, 1) is served by the same rule (fused or launch pairs), its
 * actions rows holding (dv, dtheta).
 *   CN_ROBOT_DWA (after cn_scripted_dwa) always runs as launch pairs -- the controller takes a wavefront per env, which
 * the step workgroup does not have to spare -- on a mixed engine each group on its own stream; in cn_rollout_noisy and
 * cn_rollout_lidar likewise (their `elsewhere` rule).
 * CN_EUNSUPPORTED: a unicycle engine, a mixed engine without the opt-in or with a unicycle group (unicycle: unless
 * cn_scripted_unicycle enabled it). CN_EINVAL: an
 * unknown policy, T < 0, out / actions / an
 * observation pointer NULL. All are checked before any launch (*num_launches = 0). T = 0 launches nothing. */
typedef struct cn_rollout_out {
    float   *actions;        /* [T][E][2]  required: the controller's action of step t (as cn_robot_act rounds it) */
    float   *robot_node;     /* obs AFTER step t (what cn_step returns for it): [T][E][7], [T][E][2], [T][E][N][2]   */
    float   *temporal_edges; /*   when flags & CN_ROLLOUT_OBS_EVERY_STEP; otherwise one row each ([E]..), holding   */
    float   *spatial_edges;  /*   the last step's observation as cn_step_seq does. Required.                        */
    float   *reward;         /* [T][E]    any of the following may be NULL                                          */
    uint8_t *done;           /* [T][E]                                                                               */
    int8_t  *event;          /* [T][E]                                                                               */
    float   *info;           /* [T][E][CN_INFO_K]                                                                    */
    double  *ep_return;      /* [T][E]    valid where done                                                           */
    int32_t *ep_len;         /* [T][E]                                                                               */
    int32_t  flags;
} cn_rollout_out;
#define CN_ROLLOUT_OBS_EVERY_STEP 1
int cn_rollout(cn_engine *eng, void *stream, int policy, int T, const cn_rollout_out *out, int32_t *num_launches);

/* cn_rollout with a perturbed executed action (noise injection for imitation data): the recorded label stays the
 * controller's clean action, the step consumes the perturbed one. For env e (global index G = env_offset + e) and
 * step t of the call, with k = step0 + t:
 *   w   = philox4x32_10(counter (uint32)k, key (seed, (uint32)G))        (the generator of CN_RNG_PHILOX)
 *   n_j = 2 * ((float)(w_j >> 8) * 2^-24) - 1,  j = 0, 1 (words x, y)    (exact in float32, in [-1, 1))
 *   x_j = a_j + sigma * n_j                                              (float32: one rounded product, one rounded sum)
 * a (cn_robot_act's action) goes to out->actions[t][e], x to executed[t][e] (if given) and into the step, whose own
 * clip_action applies to it as to any caller's action. Every other output is cn_rollout's. A call of T steps equals
 * calls of T1 and T - T1 steps with step0 and step0 + T1. sigma == 0 is cn_rollout itself (no arithmetic: a -0.0f
 * action keeps its sign) followed by a copy of actions into executed.
 *   Fused path (cn_rollout's conditions): the rollout launches perturb the action between their controller and their
 * step; one small launch before them hands sigma / seed / executed to the engine's device block. Elsewhere a step
 * is three launches: cn_robot_act, the perturbation (into an engine-owned (E, 2) scratch), cn_step.
 * Stream-ordered; no allocation, no synchronisation, no memset. *num_launches counts every kernel launch.
 * CN_EINVAL: noise NULL, sigma < 0 or not finite, and cn_rollout's; CN_EUNSUPPORTED: cn_rollout's. All are checked
 * before any launch (*num_launches = 0). */
typedef struct cn_rollout_noise {
    float    sigma;     /* half-width of the uniform perturbation per action component (m/s; on a unicycle engine in
                           its action units, where 0.1 is the whole range); finite, >= 0 */
    uint32_t seed;
    int64_t  step0;     /* index of this call's first step in the caller's noise sequence (chunked calls continue it) */
    float   *executed;  /* [T][E][2] optional: the action the step actually took */
} cn_rollout_noise;
int cn_rollout_noisy(cn_engine *eng, void *stream, int policy, int T, const cn_rollout_out *out,
                     const cn_rollout_noise *noise, int32_t *num_launches);

/* cn_rollout / cn_rollout_noisy that also record the live ConvGRU observation of every step, so that the LiDAR
 * policy can be trained from the scripted expert. For every step t and env e the call records the state step t
 * LEAVES (after an auto-reset where one happened: the state cn_step's observation describes) -- the twelve float64
 * fields cn_lidar_scan reads, field-major:
 *   robot_state [9][T][E]    = r_px, r_py, r_vx, r_vy, r_radius, r_gx, r_gy, r_vpref, r_theta
 *   human_state [3][T][E][N] = h_px, h_py, h_r      (the humans' TRUE positions, not the robot's belief)
 * and after the last step scans all T * E rows at once: obs[t][e] is bit for bit what cn_lidar_scan(eng, stream,
 * beams, max_range, robot_radius, ..) writes for env e when called right after step t. The three buffers are
 * caller-owned and required; the state rows are workspace and output. `out` is cn_rollout's (without
 * CN_ROLLOUT_OBS_EVERY_STEP the SRNN observation stays one row); noise = NULL is cn_rollout, otherwise
 * cn_rollout_noisy (sigma == 0 included). Every row those record and the state blob afterwards are theirs bit for
 * bit; a call of T steps equals calls of T1 and T - T1 steps (each with buffers of its own length).
 * Stream-ordered; no allocation, no synchronisation, no memset. *num_launches counts every kernel launch:
 *   Fused path (cn_rollout's conditions), T' = T minus a first step after cn_reset / cn_set_state:
 *       [1 if sigma > 0: the noise block] + 1 (the row block) + ceil(T' / C) + S       (T' > 0)
 *     the rollout launches record the rows themselves: while the controller of step s >= 1 runs on one wave, the
 *     other waves of the workgroup copy the state step s - 1 left; the launch's last step copies its own.
 *   Elsewhere (chunk 1, graph mode, that first step, ORCA at N + 1 > 10, the kd-tree step path), per step:
 *       cn_robot_act, [the perturbation if sigma > 0], cn_step, the row copy: 3 or 4 launches, then + S.
 *   S = the scan: 1 launch, unless T * E * N (or T * E) reaches 2^31, where it is split into spans of rows whose
 *     indices stay in int range. + 1 for the copy into `executed` when noise is given with sigma == 0.
 * CN_EINVAL: lidar NULL, a NULL buffer in it, cn_lidar_scan's (beams in [2, 4096], max_range in (0, 1e4] and at
 * least two 0.01 m samples), cn_rollout_noisy's for a non-NULL noise, cn_rollout's. CN_EUNSUPPORTED: cn_rollout's
 * (a unicycle engine without cn_scripted_unicycle), and any mixed engine (no LiDAR there). All are checked before any launch
 * (*num_launches = 0). T = 0 launches nothing. */
struct cn_rollout_lidar {   /* (no typedef: the function below has the name, as stat() and struct stat) */
    float  *obs;           /* [T][E][7 + beams]: the ConvGRU observation AFTER step t, what cn_lidar_scan writes for that state */
    int32_t beams;  double max_range, robot_radius;      /* cn_lidar_scan's, same ranges */
    double *robot_state;   /* [9][T][E]    */
    double *human_state;   /* [3][T][E][N] */
};
int cn_rollout_lidar(cn_engine *eng, void *stream, int policy, int T, const cn_rollout_out *out,
                     const cn_rollout_noise *noise /* NULL: no noise */, const struct cn_rollout_lidar *lidar,
                     int32_t *num_launches);

/* cn_rollout / cn_rollout_noisy that also record which humans the robot sees after every step, so that a policy with
 * the masked spatial attention (the observation key 'visible_masks') can be trained from the scripted expert.
 * mask is [T][E][NS] float32, NS = cn_visible_mask's padded stride: row t of env e is bit for bit what
 * cn_visible_mask(eng, stream, ..) writes for env e when called right after step t (one device function serves
 * both). An env that ended and auto-reset inside step t therefore carries its new episode's mask (the reset path:
 * flags == 0 and the float64 test). Without CN_ROLLOUT_OBS_EVERY_STEP mask is one row [E][NS] holding the last
 * step's, as the observation buffers do. `out` is cn_rollout's; noise = NULL is cn_rollout, otherwise
 * cn_rollout_noisy (sigma == 0 included). Every row those record and the state blob afterwards are theirs bit for
 * bit; a call of T steps equals calls of T1 and T - T1 steps. It is a new function and needs no opt-in of its own.
 * Stream-ordered; no allocation, no synchronisation, no memset. *num_launches counts every kernel launch:
 *   Fused path (cn_rollout's conditions), T' = T minus a first step after cn_reset / cn_set_state:
 *       [1 if sigma > 0: the noise block] + ceil(T' / C)                               (T' > 0)
 *     i.e. cn_rollout's / cn_rollout_noisy's own count: the rollout launches record the mask themselves (their row 0
 *     travels in the kernel arguments). While the controller of step s >= 1 runs on one wave, the other waves of the
 *     workgroup evaluate the mask of the state step s - 1 left, one lane per (env, slot); the launch's last step
 *     writes its own row.
 *   Elsewhere (chunk 1, graph mode, that first step, ORCA at N + 1 > 10, the kd-tree step path, CN_ROBOT_DWA), per
 *     step: cn_robot_act, [the perturbation if sigma > 0], cn_step, cn_visible_mask's launch into row t: 3 or 4
 *     launches (graph mode: one more kernel node per step).
 *   A mixed engine after cn_mixed_scripted(eng, 1): every group on its own stream by the same rule, its envs at their
 *     rows of the buffer, the padded slots written as 0.0f in every row; *num_launches counts all groups.
 *   A unicycle engine after cn_scripted_unicycle / cn_scripted_dwa: the same rule, as in cn_rollout.
 *   + 1 for the copy into `executed` when noise is given with sigma == 0.
 * CN_EINVAL: mask NULL, cn_rollout_noisy's for a non-NULL noise, cn_rollout's. CN_EUNSUPPORTED: cn_rollout's. All are
 * checked before any launch (*num_launches = 0). T = 0 launches nothing. */
int cn_rollout_masked(cn_engine *eng, void *stream, int policy, int T, const cn_rollout_out *out,
                      const cn_rollout_noise *noise /* NULL: no noise */, float *mask, int32_t *num_launches);

/* Test hooks of the kd-tree path's resumable spawns (the spawn waves that draw upcoming episodes park a
 * crowded spawn between two humans once a wave has worked `cycles` clock cycles in a launch, and a later
 * launch resumes it; default 600000, 0 = never park; no effect on the quad path, which never parks).
 * cn_debug_spawn_stats: cumulative counts since cn_create [5] = spawns parked before they started, parked
 * mid-way, resumed, completed by a resume (kd-tree path), and auto-resets whose spawn the step kernel drew
 * inline because no pending spawn was ready (every path; synchronises the device). Results do not depend on the budget:
 * tests/test_gpu_parity.py forces parking after every human and compares with the oracle. The budget is per step:
 * a multi-step launch of cn_step_seq gives its spawn waves `cycles` times its number of steps. */
int cn_debug_set_spawn_budget(cn_engine *eng, long long cycles);
int cn_debug_spawn_stats(cn_engine *eng, uint32_t *out);

/* Steps per launch of cn_step_seq's multi-step launches (default: the library's CN_SEQ_CHUNK, csrc/engine/plan.h). n = 1 issues one
 * cn_step launch per step through the single-step kernels: the in-library A/B and the reference of
 * tests/test_step_seq_fused.py. Results do not depend on n. */
int cn_debug_set_seq_chunk(cn_engine *eng, int n);

/* Profiler calibration hook (MI355X_MICROARCH.md § HBM: FETCH_SIZE / WRITE_SIZE are calibrated only for
 * 16-B-per-lane streams): dst[k] = src[k] over n doubles with the step kernel's access shape, one 8-B load
 * and store per lane, in segments of `seg` consecutive doubles per 64-lane wave (seg = 64: a field of the
 * per-human SoA arrays; seg = 6: a per-env field of one workgroup). tools/calib_pmc.py reads the
 * counters of known byte counts through it. */
int cn_debug_copy64(void *stream, int64_t n, int seg, const double *src, double *dst);

/* out[r][h] = sum_n hs[r][n][h] * attn[r][n]; hs [R][N][H], attn [R][N], out [R][H]; H % 4 == 0. */
int cn_attn_pool_fwd(void *stream, int64_t R, int N, int H, const float *hs, const float *attn, float *out);

/* Gradient of cn_attn_pool_fwd: dhs[r][n][h] = dout[r][h] * attn[r][n],
 * dattn[r][n] = sum_h dout[r][h] * hs[r][n][h] (fixed-order reduction). H in {64, 128, 256}. */
int cn_attn_pool_bwd(void *stream, int64_t R, int N, int H, const float *hs, const float *attn, const float *dout,
                     float *dhs, float *dattn);

/* The whole spatial-edge attention of EdgeAttention.forward (srnn_model.py:256-333: spatial_edge_layer,
 * the product with temporal_embed summed over the embedding, * num_edges / sqrt(attention_size), softmax
 * over the N edges, bmm pooling) in one pass over hs, given u = temporal_embed @ Ws [R][H] and
 * c = temporal_embed . bs [R] from the caller (Ws, bs: spatial_edge_layer's weight [A][H] and bias [A]):
 *   attn[r][n] = softmax_n(scale * (hs[r][n] . u[r] + c[r])),  out[r] = sum_n attn[r][n] hs[r][n].
 * hs [R][N][H], out [R][H], attn [R][N]; H in {64, 128, 256}, 1 <= N <= 64; hs, u, out 16-byte aligned. */
int cn_spatial_attn_fwd(void *stream, int64_t R, int N, int H, float scale, const float *hs, const float *u,
                        const float *c, float *out, float *attn);

/* Gradient of cn_spatial_attn_fwd given dout [R][H] and optionally dattn [R][N] (null: none):
 * dhs [R][N][H], du rows of H at stride ldu (-> d temporal_embed = du Ws^T + dc bs^T, dWs = temporal_embed^T du
 * on the caller's side), dc at stride ldc (dc = du + H with ldc = ldu puts [du | dc] in one matrix, so
 * dWs and dbs come from one GEMM). hs, u, dout, dhs, du 16-byte aligned; ldu >= H, ldu % 4 == 0. */
int cn_spatial_attn_bwd(void *stream, int64_t R, int N, int H, float scale, const float *hs, const float *u,
                        const float *attn, const float *dout, const float *dattn, float *dhs, float *du, int64_t ldu,
                        float *dc, int64_t ldc);

/* cn_spatial_attn_fwd / _bwd with a per-row human count (rows padded to N slots: a policy over crowds of
 * varying size): row r attends to its first count[r] slots only (1 <= count[r] <= N, int32 [R]; the caller's
 * contract, not validated on the device) with its own temperature row_scale[r] (float [R]), and is computed as
 * the pair above computes a row at N = count[r], scale = row_scale[r] (same operation order). attn[r][n] and
 * dhs[r][n][:] for n >= count[r] are written as zeros; hs[r][n] and dattn[r][n] are never read there.
 * Shapes, alignment and strides as above; count and row_scale non-null. No allocation, sync or memset. */
int cn_spatial_attn_var_fwd(void *stream, int64_t R, int N, int H, const int32_t *count, const float *row_scale,
                            const float *hs, const float *u, const float *c, float *out, float *attn);
int cn_spatial_attn_var_bwd(void *stream, int64_t R, int N, int H, const int32_t *count, const float *row_scale,
                            const float *hs, const float *u, const float *attn, const float *dout, const float *dattn,
                            float *dhs, float *du, int64_t ldu, float *dc, int64_t ldc);

/* cn_spatial_attn_var_fwd / _bwd with a per-slot mask in place of the count (attention over the humans the robot
 * sees: cn_visible_mask's rows): mask [R][N] float32, nonzero and not NaN = visible. Row r attends to its visible
 * slots only, visited in ascending slot order, with the temperature row_scale[r], and is computed as the _var pair
 * computes a row that holds those slots compacted to the front (same operations, same order: a full mask is
 * cn_spatial_attn_fwd's row, a prefix mask the _var row of that count, bit for bit). attn[r][n] and dhs[r][n][:] of
 * masked slots are written as exact zeros; hs[r][n] and dattn[r][n] are never read there. A row without a visible
 * slot gives out = 0, attn = 0, du = 0, dc = 0, dhs = 0. Shapes, alignment and strides as above; mask and row_scale
 * non-null. No allocation, sync or memset. */
int cn_spatial_attn_mask_fwd(void *stream, int64_t R, int N, int H, const float *mask, const float *row_scale,
                             const float *hs, const float *u, const float *c, float *out, float *attn);
int cn_spatial_attn_mask_bwd(void *stream, int64_t R, int N, int H, const float *mask, const float *row_scale,
                             const float *hs, const float *u, const float *attn, const float *dout, const float *dattn,
                             float *dhs, float *du, int64_t ldu, float *dc, int64_t ldc);

/* Weight gradient of a Linear layer over K rows with a tiny side (ops.linear / the fused input layers'
 * backward, replacing torch's dy^T x in the reference's autograd of srnn_model.py:160-161,210-211,466 and
 * distributions.py:74-94): dW[a][j] = sum_k dy'[k][a] x[k][j] and db[a] = sum_k dy'[k][a] with
 * dy' = dy * (relu_out > 0) when relu_out != NULL (the gradient through a ReLU whose output was relu_out).
 * dy, relu_out [K][m], x [K][n] contiguous float32; dW [m][n]; db [m] or NULL; min(m, n) <= 8, max(m, n) <= 256.
 * work: caller-owned device scratch of cn_wgrad_work_elems(K, m, n) floats. Deterministic (fixed order). */
int64_t cn_wgrad_work_elems(int64_t K, int m, int n);
int cn_wgrad(void *stream, int64_t K, int m, int n, const float *dy, const float *relu_out, const float *x,
             float *dW, float *db, float *work);

#ifdef __cplusplus
}
#endif
#endif /* CROWDNAV_H */
