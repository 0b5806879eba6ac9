// host_engine.h -- the host side below the C ABI: the engine object (struct cn_engine), the norm zones' unit-
// circle table upload, the thread-local error text (set_err, HIPCHK), the launchers of the two stream-ordered
// helper kernels (ctl_set, keysnap), the table of cn_step_kernel's instantiations (step_kernels,
// step_kernel_for) and the triple-buffered spawn-list slots of a step launch (list_read_slot, step_list_slots).
// Part of cn_engine.hip's translation unit: included there after the device core (StepPlan, PendPtrs, StepArgs,
// cn_step_kernel, the c_circ_* tables).
#pragma once
#include "aux_kernels.h"

#define CN_WORK_BYTES 128
static_assert(CN_NOISE_W * 4 + sizeof(RolloutNoise) <= CN_WORK_BYTES && (CN_NOISE_W * 4) % alignof(RolloutNoise) == 0,
              "cn_engine::work_count: the RolloutNoise block behind the 16 control words");
static_assert(CN_ROWS_W * 4 >= CN_NOISE_W * 4 + sizeof(RolloutNoise) && CN_ROWS_W * 4 + sizeof(RolloutRows) <= CN_WORK_BYTES &&
                  (CN_ROWS_W * 4) % alignof(RolloutRows) == 0,
              "cn_engine::work_count: the RolloutRows block behind the RolloutNoise block");
static_assert(CN_ER_W * 4 >= CN_ROWS_W * 4 + sizeof(RolloutRows) && CN_ER_W * 4 + 4 <= CN_WORK_BYTES,
              "cn_engine::work_count: a group's row count behind the RolloutRows block");

struct cn_engine {
    cn_config c;
    int device;
    int E, N, A;
    StepPlan plan;
    void *state;
    int64_t state_bytes;
    cn_state_ptrs s;
    uint32_t *work;       // [E]
    uint32_t *work_count; // [16]: [2..4] spawn-list counters (triple buffered), [5..7] parked-spawn counters,
                          // [8..11] spawn statistics (PendLaunch::stats), [15] inline reset draws; behind them
                          // (word CN_NOISE_W) cn_rollout_noisy's RolloutNoise block and (word CN_ROWS_W)
                          // cn_rollout_lidar's RolloutRows block, and (word CN_ER_W) a mixed engine's E in its
                          // groups: CN_WORK_BYTES in all
    float *act_x;         // [E][2] cn_rollout_noisy's launch triples: the perturbed action the step reads
    uint32_t *plist;      // [3][E + 64][4] envs whose spawn after next kernel A draws, with their counters
    uint32_t *rlist;      // [3][2E][4] spawns parked by a launch (resumed by the next); counters work_count[5..7]
    int devseq;           // graph mode (cn_set_graph_mode): the step sequence lives in work_count[12..14]
    uint32_t ctl_host[4];
    int pend_all;         // next kernel A's pending mode: PEND_BOTH (after cn_set_state) or PEND_FRESH (after cn_reset)
    uint64_t nstep;
    long long spawn_budget;   // clock cycles a spawning wave works per step of a launch before parking (0: never)
    int seq_chunk;        // steps per launch of cn_step_seq (1: a cn_step launch per step)
    void *pend_mem;       // pending next-episode spawns (PendPtrs)
    PendPtrs pend;
    int pend_blocks;      // spare workgroups of kernel A running spawn waves
    int pend_waves;       // spawning waves per spare workgroup
    int a_lds;            // kernel A dynamic LDS: max(step plan, spawn waves)
    int64_t case_size, counter_offset;
    int rng_grid;
    // kernel timing (cn_profile)
    int prof_on, prof_cap, prof_n;
    hipEvent_t *ev;  // [2]: before the first, after the last launch of the window
    // output view (a group of a mixed engine: its envs' rows in the caller's buffers and the padded human
    // stride; identity / N for a plain engine)
    int32_t *rows;   // device [E] or nullptr
    int NS;
    int ER;          // envs of the caller's buffers: the mixed engine's E for a group (work_count[CN_ER_W]), E otherwise
    // mixed engine (cn_create_mixed): the groups, each a plain engine over its envs; E = all envs,
    // N = NS = the largest human count
    int ngroups;
    cn_engine **grp;
    hipStream_t *gstream;   // [ngroups]: group k > 0 steps on gstream[k] (forked from / joined to the caller's)
    hipEvent_t *gev;        // [ngroups + 1]: fork, then one join event per forked group
    int scripted;           // cn_mixed_scripted: cn_robot_act / cn_rollout / cn_rollout_noisy serve this mixed engine
    int scripted_uni;       // cn_scripted_unicycle: they (and cn_rollout_lidar) serve unicycle kinematics
    int dwa;                // cn_scripted_dwa: they accept CN_ROBOT_DWA (a mixed engine: set in its groups as well)
    cn_dwa_params dwa_p;    // ... with these parameters
};

// unit-circle table of GEOS's 64-gon point buffer (norm zones), per device; every entry point whose
// kernels read it (cn_create, cn_debug_disc_quad) uploads it first
static hipError_t circ_table_init()
{
    double cs[64], sn[64];
    for (int k = 0; k < 64; ++k) { const double a = -(k * (CN_PI / 2 / 16)); cs[k] = cos(a); sn[k] = sin(a); }
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_circ_cos), cs, sizeof cs);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_circ_sin), sn, sizeof sn);
    return e;
}

static thread_local char g_err[512];
static int set_err(int code, const char *fmt, const char *a = "")
{
    snprintf(g_err, sizeof g_err, fmt, a);
    return code;
}
int cn_set_error(int code, const char *msg) { return set_err(code, "%s", msg); }   // for cn_gru.hip
#define HIPCHK(x)                                                                       \
    do {                                                                                \
        hipError_t _e = (x);                                                            \
        if (_e != hipSuccess) return set_err(CN_EHIP, "HIP error: %s", hipGetErrorString(_e)); \
    } while (0)

// cn_ctl_set_kernel on the stream (aux_kernels.h: why a kernel and not hipMemsetAsync)
static int ctl_set(uint32_t *w, uint32_t v, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_ctl_set_kernel, dim3(1), dim3(64), 0, st, w, v);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CN_OK : set_err(CN_EHIP, hipGetErrorString(e));
}

// The spawn lists are triple-buffered by launch number t: launch t appends to slot t % 3, zeroes the counters of
// slot (t + 1) % 3 for the next launch, and READS this slot, the one launch t - 1 appended to.
static int64_t list_read_slot(uint64_t t) { return (int64_t)((t + 2) % 3); }

// the snapshot for the engine's next step launch (g->nstep: the host sequence; graph mode reads the device's)
static int keysnap(const cn_engine *g, hipStream_t st)
{
    const int host_kr = g->devseq ? -1 : (int)list_read_slot(g->nstep);
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_keysnap_kernel, dim3((g->E + 255) / 256), dim3(256), 0, st, g->s.reset_count, g->s.case_counter,
                       g->plist, (const uint32_t *)g->work_count, host_kr, (int)g->E);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CN_OK : set_err(CN_EHIP, hipGetErrorString(e));
}

// Every instantiation of cn_step_kernel, listed ONCE: cn_create raises the dynamic-LDS limit of each entry and
// step_launch picks its kernel here, so a new template flag is added in this table (and STEP_KERNEL) alone.
// Launch modes: a single step with host-passed arguments; graph mode (DEVSEQ, plain engines); a multi-step launch
// (SEQ, quad-path engines and quad-path groups of a mixed engine); a cn_rollout launch (SEQ + ROBOT, the same
// engines and groups) and a cn_rollout_lidar launch (SEQ + ROBOT + REC, plain engines: it records the state rows
// as well); a cn_rollout_masked launch (SEQ + ROBOT + MASK, the engines and groups of cn_rollout: it records the
// visible_masks rows as well). A combination that is not listed does not exist: the kd-tree path (kd) has no SEQ /
// ROBOT kernel, mixed-engine groups (mix) none for graph mode or the recording rollout (no LiDAR on a mixed engine).
// (The entries' order is the order in which the compiler emits the kernels into the code object: the groups'
// multi-step kernels and then the mask-recording kernels are appended at the end, so the earlier ones are emitted as
// before.)
enum StepMode { STEP_SINGLE, STEP_DEVSEQ, STEP_SEQ, STEP_ROBOT, STEP_ROBOT_REC, STEP_ROBOT_MASK };
typedef void (*StepKernelFn)(StepArgs, cn_config);
struct StepKernelEntry {
    bool kd, phx, mix;
    StepMode mode;
    StepKernelFn fn;
};
#define STEP_KERNEL(KD, PHX, MIX, MODE) \
    {KD, PHX, MIX, MODE,                                                                                             \
     cn_step_kernel<KD, PHX, MIX, MODE == STEP_DEVSEQ, MODE != STEP_SINGLE && MODE != STEP_DEVSEQ,                   \
                    MODE == STEP_ROBOT || MODE == STEP_ROBOT_REC || MODE == STEP_ROBOT_MASK, MODE == STEP_ROBOT_REC,  \
                    MODE == STEP_ROBOT_MASK>}
static const StepKernelEntry step_kernels[] = {
    STEP_KERNEL(false, false, false, STEP_SEQ),    STEP_KERNEL(false, true, false, STEP_SEQ),
    STEP_KERNEL(true, false, false, STEP_SINGLE),  STEP_KERNEL(false, false, false, STEP_SINGLE),
    STEP_KERNEL(true, true, false, STEP_SINGLE),   STEP_KERNEL(false, true, false, STEP_SINGLE),
    STEP_KERNEL(true, false, true, STEP_SINGLE),   STEP_KERNEL(false, false, true, STEP_SINGLE),
    STEP_KERNEL(true, true, true, STEP_SINGLE),    STEP_KERNEL(false, true, true, STEP_SINGLE),
    STEP_KERNEL(false, false, false, STEP_DEVSEQ), STEP_KERNEL(false, true, false, STEP_DEVSEQ),
    STEP_KERNEL(true, false, false, STEP_DEVSEQ),  STEP_KERNEL(true, true, false, STEP_DEVSEQ),
    STEP_KERNEL(false, false, false, STEP_ROBOT),  STEP_KERNEL(false, true, false, STEP_ROBOT),
    STEP_KERNEL(false, false, false, STEP_ROBOT_REC), STEP_KERNEL(false, true, false, STEP_ROBOT_REC),
    STEP_KERNEL(false, false, true, STEP_SEQ),     STEP_KERNEL(false, true, true, STEP_SEQ),
    STEP_KERNEL(false, false, true, STEP_ROBOT),   STEP_KERNEL(false, true, true, STEP_ROBOT),
    STEP_KERNEL(false, false, false, STEP_ROBOT_MASK), STEP_KERNEL(false, true, false, STEP_ROBOT_MASK),
    STEP_KERNEL(false, false, true, STEP_ROBOT_MASK),  STEP_KERNEL(false, true, true, STEP_ROBOT_MASK)};
#undef STEP_KERNEL

// the kernel of a launch, or null where the combination does not exist
static StepKernelFn step_kernel_for(bool kd, bool phx, bool mix, StepMode mode)
{
    for (const StepKernelEntry &k : step_kernels)
        if (k.kd == kd && k.phx == phx && k.mix == mix && k.mode == mode) return k.fn;
    return nullptr;
}

// The StepArgs / PendLaunch members that name the spawn lists of launch number t (cn_engine::nstep before the
// launch; slots as list_read_slot says), and the launch's id: nonzero, different from its neighbours'. This is
// the host sequence; in graph mode the device keeps the launch number, and cn_step_kernel's DEVSEQ prologue and
// cn_keysnap_kernel (host_kr < 0) derive the same slots from it: all of them must agree.
static void step_list_slots(const cn_engine *g, uint64_t t, StepArgs &a)
{
    const int64_t kw = (int64_t)(t % 3), kr = list_read_slot(t), kz = (int64_t)((t + 1) % 3);
    const int64_t ls = 4 * ((int64_t)g->E + 64), rs = 4 * (2 * (int64_t)g->E + 64);
    a.plist_w = g->plist + kw * ls;
    a.pcount_w = g->work_count + 2 + kw;
    a.pcount_zero = g->work_count + 2 + kz;
    a.rcount_zero = g->work_count + 5 + kz;
    a.pend.list = g->plist + kr * ls;
    a.pend.count = g->work_count + 2 + kr;
    a.pend.rlist = g->rlist + kr * rs;
    a.pend.rcount = g->work_count + 5 + kr;
    a.pend.rlist_w = g->rlist + kw * rs;
    a.pend.rcount_w = g->work_count + 5 + kw;
    a.pend.launch_id = (uint32_t)((t + 1) % 0x7ffffffeu) + 1u;
}
