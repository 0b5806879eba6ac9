// host_api.h -- the C ABI of the engine (include/crowdnav.h): configuration and state layout queries, engine
// creation (plain and mixed), reset / step / multi-step / rollout launches, graph mode, state get / set,
// profiling, the LiDAR and scripted-robot calls, and the debug / predictor entry points. Host code only; the
// kernels it launches are in cn_engine.hip's device core (which includes this file last) and the headers below.
#pragma once
#include <math.h>
#include <string.h>
#include <vector>

#include "host_engine.h"
#include "edge_features.h"
#include "lidar.h"

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int cn_graph_node_counts(void *graph, int64_t *counts, int n, int64_t *total)
{
    if (!graph || (n > 0 && !counts) || n < 0 || n > 32) return set_err(CN_EINVAL, "cn_graph_node_counts: graph, 0 <= n <= 32");
    for (int k = 0; k < n; ++k) counts[k] = 0;
    size_t num = 0;
    HIPCHK(hipGraphGetNodes((hipGraph_t)graph, nullptr, &num));
    std::vector<hipGraphNode_t> nodes(num);
    if (num) HIPCHK(hipGraphGetNodes((hipGraph_t)graph, nodes.data(), &num));
    for (size_t i = 0; i < num; ++i) {
        hipGraphNodeType t;
        HIPCHK(hipGraphNodeGetType(nodes[i], &t));
        if ((int)t >= 0 && (int)t < n) ++counts[(int)t];
    }
    if (total) *total = (int64_t)num;
    return CN_OK;
}

const char *cn_last_error(void) { return g_err; }
#ifndef CN_SRC_HASH
#define CN_SRC_HASH "unversioned"
#endif
// build.py passes the sha256 of the flags + sources; _lib.lib() compares it with the sources on disk
const char *cn_version(void) { return "crowdnav_dsrnn_amd 0.2 (gfx950) CN_SRC_HASH=" CN_SRC_HASH; }

int cn_config_validate(const cn_config *c)
{
    if (!c) return set_err(CN_EINVAL, "null config");
    if (c->num_envs <= 0) return set_err(CN_EINVAL, "num_envs must be > 0");
    if ((int64_t)c->num_envs * (c->human_num + 1) >= (1LL << 31) / 8)
        return set_err(CN_EUNSUPPORTED, "num_envs * human_num too large for one engine (shard over engines)");
    if (c->human_num < 1 || c->human_num > 31) return set_err(CN_EUNSUPPORTED, "human_num must be in [1, 31]");
    if (c->human_num + (c->robot_visible ? 1 : 0) > CN_MAX_A) return set_err(CN_EUNSUPPORTED, "too many agents");
    if (c->num_scenarios < 1 || c->num_scenarios > CN_MAX_SCENARIOS) return set_err(CN_EINVAL, "num_scenarios");
    for (int k = 0; k < c->num_scenarios; ++k)
        if (c->scenarios[k] < 0 || c->scenarios[k] > CN_SC_SIDE_PREF_CROSSING) return set_err(CN_EINVAL, "scenario id");
    if (c->kinematics != CN_HOLONOMIC && c->kinematics != CN_UNICYCLE) return set_err(CN_EINVAL, "kinematics");
    if (c->rng_mode != CN_RNG_MT19937 && c->rng_mode != CN_RNG_PHILOX) return set_err(CN_EINVAL, "rng_mode");
    if (c->human_policy != CN_POLICY_ORCA && c->human_policy != CN_POLICY_SOCIAL_FORCE)
        return set_err(CN_EUNSUPPORTED, "human policy");
    if (!c->potential_based) return set_err(CN_EUNSUPPORTED, "only potential-based reward shaping is supported");
    if (!(c->time_step > 0)) return set_err(CN_EINVAL, "time_step must be > 0");
    if (c->phase < 0 || c->phase > 2) return set_err(CN_EINVAL, "phase");
    if (c->nenv <= 0) return set_err(CN_EINVAL, "nenv must be > 0");
    if (c->max_tries <= 0) return set_err(CN_EINVAL, "max_tries must be > 0");
    return CN_OK;
}

int cn_state_field_info(int field, const char **name, int *type_code, int *count_kind)
{
    static const char *names[] = {
#define X(n, ct, tc, ck) #n,
        CN_STATE_FIELDS(X)
#undef X
    };
    static const int tcs[] = {
#define X(n, ct, tc, ck) tc,
        CN_STATE_FIELDS(X)
#undef X
    };
    static const int cks[] = {
#define X(n, ct, tc, ck) ck,
        CN_STATE_FIELDS(X)
#undef X
    };
    if (field < 0 || field >= CN_NUM_FIELDS) return set_err(CN_EINVAL, "field index");
    if (name) *name = names[field];
    if (type_code) *type_code = tcs[field];
    if (count_kind) *count_kind = cks[field];
    return CN_OK;
}

int cn_state_layout_offsets(const cn_config *cfg, int64_t *offsets, int64_t *total)
{
    if (!cfg) return set_err(CN_EINVAL, "null config");
    const int64_t t = cn_state_layout(cfg->num_envs, cfg->human_num, cfg->robot_visible, offsets);
    if (total) *total = t;
    return CN_OK;
}

int cn_create(const cn_config *cfg, int device, cn_engine **out)
{
    if (!out) return set_err(CN_EINVAL, "null out");
    *out = nullptr;
    int rc = cn_config_validate(cfg);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    cn_engine *g = new cn_engine();
    g->c = *cfg;
    g->device = device;
    g->E = cfg->num_envs;
    g->N = cfg->human_num;
    g->NS = g->N;
    g->ER = g->E;
    g->A = cn_sim_agents(g->N, cfg->robot_visible);
    g->plan = cn_step_plan(g->N, cfg->robot_visible);
    g->state_bytes = cn_state_layout(g->E, g->N, cfg->robot_visible, nullptr);
    switch (cfg->phase) {
    case CN_PHASE_TRAIN: g->case_size = 4294967295LL - 2000; g->counter_offset = 2000; break;
    case CN_PHASE_VAL: g->case_size = cfg->val_size; g->counter_offset = 0; break;
    default: g->case_size = cfg->test_size; g->counter_offset = 1000; break;
    }
    if (g->case_size <= 0) { delete g; return set_err(CN_EINVAL, "case size (val_size/test_size) must be > 0"); }
    const int64_t E = g->E, EN = (int64_t)g->E * g->N;
    auto al = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    // pending spawns: every array holds both slots ([2][...], pend_slot)
    const int64_t pb_mt = al(2 * E * CN_MT_N * 4), pb_i = al(2 * E * 4), pb_cc = al(2 * E * 8), pb_r = al(2 * 5 * E * 8),
                  pb_h = al(2 * 7 * EN * 8);
    const int64_t pend_bytes = pb_mt + 5 * pb_i + 2 * pb_cc + pb_r + pb_h;
    hipError_t e1 = hipMalloc(&g->state, g->state_bytes);
    hipError_t e2 = hipMalloc(&g->work, sizeof(uint32_t) * (g->E + 64));
    hipError_t e3 = hipMalloc(&g->work_count, CN_WORK_BYTES);
    hipError_t e4 = hipMalloc(&g->plist, sizeof(uint32_t) * 3 * 4 * (g->E + 64));
    hipError_t e6 = hipMalloc(&g->rlist, sizeof(uint32_t) * 3 * 4 * (2 * (int64_t)g->E + 64));
    hipError_t e5 = hipMalloc(&g->pend_mem, pend_bytes);
    hipError_t e7 = hipMalloc(&g->act_x, sizeof(float) * 2 * (g->E + 64));
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess ||
        e6 != hipSuccess || e7 != hipSuccess) {
        (void)hipFree(g->state); (void)hipFree(g->work); (void)hipFree(g->work_count); (void)hipFree(g->plist); (void)hipFree(g->pend_mem);
        (void)hipFree(g->rlist); (void)hipFree(g->act_x);
        delete g;
        return set_err(CN_ENOMEM, "hipMalloc failed");
    }
    if (hipMemset(g->state, 0, g->state_bytes) != hipSuccess || hipMemset(g->work_count, 0, CN_WORK_BYTES) != hipSuccess ||
        hipMemset(g->pend_mem, 0, pend_bytes) != hipSuccess) {
        cn_destroy(g);
        return set_err(CN_EHIP, "hipMemset failed");
    }
    {
        char *b = (char *)g->pend_mem;
        g->pend.mt = (uint32_t *)b; b += pb_mt;
        g->pend.pos = (int32_t *)b; b += pb_i;
        g->pend.ovf = (uint32_t *)b; b += pb_i;
        g->pend.sc = (int32_t *)b; b += pb_i;
        g->pend.rc = (int32_t *)b; b += pb_i;
        g->pend.ok = (uint64_t *)b; b += pb_cc;
        g->pend.prog = (int32_t *)b; b += pb_i;
        g->pend.cc = (int64_t *)b; b += pb_cc;
        g->pend.r = (double *)b; b += pb_r;
        g->pend.h = (double *)b;
    }
    g->pend_all = PEND_BOTH;
    {
        // the plan holds phase 5's RNG regions (laid over the ORCA scratch); spare workgroups run as many
        // spawning waves as regions fit in the same allocation
        g->a_lds = g->plan.total;
        const int fit = g->a_lds / g->plan.rng_stride;
        g->pend_waves = fit < g->plan.T / 64 ? fit : g->plan.T / 64;
        const int nw = g->pend_waves;
        const int64_t need = (E + nw - 1) / nw;
        // ~128 spawning waves on the quad path; 256 on the kd-tree path, whose crowded spawns (~1M cycles
        // each at 25 humans in square_crossing, ~4 % of the envs per step) must not queue behind each other
        const int cap = (g->plan.kd ? 256 : CN_QUAD_SPAWN_WAVES) / nw;
        const int pb = (int)(need < cap ? need : cap);
        g->pend_blocks = g->plan.kd ? (pb + 7) & ~7 : pb;   // leading: a multiple of 8 (XCD placement)
        // kd-tree path: a crowded spawn may take longer than the launch's step rounds; each spawning wave parks
        // its spawn after ~0.6 M cycles and a later launch resumes it (the spawn is needed one whole episode
        // later). Round 5: spawn-list entries carry the counters of the reset that queued them (a spawn wave
        // that read them from the state could see a later reset of the same env and queue a key that the next
        // launch queued again: two writers of one pending slot, one of them resuming from it -- 5 of 149 C3 runs
        // departed; 0 of 149 with keyed entries). The quad path parks after CN_QUAD_BUDGET cycles (round 6).
        g->spawn_budget = g->plan.kd ? 600000 : CN_QUAD_BUDGET;
        g->seq_chunk = CN_SEQ_CHUNK;
    }
    cn_state_bind(&g->s, g->state, g->E, g->N, cfg->robot_visible);
    if (circ_table_init() != hipSuccess) {
        cn_destroy(g);
        return set_err(CN_EHIP, "hipMemcpyToSymbol failed");
    }
    if (g->a_lds > 160 * 1024) { cn_destroy(g); return set_err(CN_EUNSUPPORTED, "LDS plan exceeds 160 KiB"); }
    if (!g->plan.kd && !cn_goal_early_ok(g->plan)) {   // (no plan of today's: the multi-step kernels rely on it)
        cn_destroy(g);
        return set_err(CN_EUNSUPPORTED, "LDS plan: the RNG regions of waves 2 and 3 overlap the staged human state");
    }
    if (g->a_lds > 64 * 1024)
        for (const StepKernelEntry &k : step_kernels)
            (void)hipFuncSetAttribute((const void *)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, g->a_lds);
    g->rng_grid = g->E < 2048 ? g->E : 2048;
    // the first launch draws every env's spawns (PEND_BOTH) from the key snapshot of the zeroed state
    if (keysnap(g, nullptr) != CN_OK) { cn_destroy(g); return CN_EHIP; }
    HIPCHK(hipDeviceSynchronize());
    *out = g;
    return CN_OK;
}

// Mixed engine (per-env scenario dispatch with per-env human counts). Env r of the engine
// (global index cfg.env_offset + r) belongs to group env_group[r]; each group is a plain engine over its
// envs with its own cn_config (human count, scenario set, circle radius, side preference, goal changing,
// ...), stepping them in the caller's (E, ...) buffers at their own rows (spatial_edges padded to the
// largest human count). Seeds and round-robin scenarios use the global index, so groups[g].scenarios
// must be the full scenario list and env r's scenario (scenarios[(env_offset + r) % num_scenarios]) must
// be one its group was configured for -- which the caller guarantees by assigning groups per scenario.
int cn_create_mixed(const cn_config *groups, int num_groups, const int32_t *env_group, int64_t num_envs, int device,
                    cn_engine **out)
{
    if (!out) return set_err(CN_EINVAL, "null out");
    *out = nullptr;
    if (!groups || !env_group || num_groups < 1 || num_groups > 64 || num_envs <= 0)
        return set_err(CN_EINVAL, "cn_create_mixed: 1..64 groups, env_group[num_envs] required");
    if (num_envs >= (1LL << 31) / 64) return set_err(CN_EUNSUPPORTED, "cn_create_mixed: too many envs");
    std::vector<std::vector<int32_t>> rows(num_groups);
    for (int64_t r = 0; r < num_envs; ++r) {
        if (env_group[r] < 0 || env_group[r] >= num_groups) return set_err(CN_EINVAL, "cn_create_mixed: env_group out of range");
        rows[env_group[r]].push_back((int32_t)r);
    }
    int NS = 0;
    for (int k = 0; k < num_groups; ++k) {
        const cn_config &c = groups[k];
        if ((int64_t)c.num_envs != (int64_t)rows[k].size())
            return set_err(CN_EINVAL, "cn_create_mixed: groups[g].num_envs must equal the envs assigned to group g");
        if (c.env_offset != groups[0].env_offset || c.nenv != groups[0].nenv || c.seed != groups[0].seed ||
            c.phase != groups[0].phase)
            return set_err(CN_EINVAL, "cn_create_mixed: env_offset / nenv / seed / phase must agree across groups");
        if (c.scenario_mode != CN_SCMODE_ROUND_ROBIN)
            return set_err(CN_EUNSUPPORTED, "cn_create_mixed: round-robin scenario mode only");
        NS = c.human_num > NS ? c.human_num : NS;
    }
    HIPCHK(hipSetDevice(device));
    cn_engine *m = new cn_engine();
    m->c = groups[0];
    m->c.num_envs = (int32_t)num_envs;
    m->c.human_num = NS;
    m->device = device;
    m->E = m->ER = (int)num_envs;
    m->N = m->NS = NS;
    m->grp = new cn_engine *[num_groups]();
    for (int k = 0; k < num_groups; ++k) {
        if (groups[k].num_envs == 0) continue;
        int rc = cn_create(&groups[k], device, &m->grp[m->ngroups]);
        if (rc) { cn_destroy(m); return rc; }
        cn_engine *g = m->grp[m->ngroups++];
        g->NS = NS;
        g->ER = (int)num_envs;
        if (hipMemcpy(g->work_count + CN_ER_W, &g->ER, sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            cn_destroy(m);
            return set_err(CN_EHIP, "hipMemcpy failed");
        }
        // the perturbed actions of a launch triple lie at the envs' rows, like every buffer a group's step reads
        (void)hipFree(g->act_x);
        g->act_x = nullptr;
        if (hipMalloc(&g->act_x, sizeof(float) * 2 * (num_envs + 64)) != hipSuccess) {
            cn_destroy(m);
            return set_err(CN_ENOMEM, "hipMalloc failed");
        }
        if (hipMalloc(&g->rows, sizeof(int32_t) * rows[k].size()) != hipSuccess) {
            cn_destroy(m);
            return set_err(CN_ENOMEM, "hipMalloc failed");
        }
        if (hipMemcpy(g->rows, rows[k].data(), sizeof(int32_t) * rows[k].size(), hipMemcpyHostToDevice) != hipSuccess) {
            cn_destroy(m);
            return set_err(CN_EHIP, "hipMemcpy failed");
        }
        m->state_bytes += g->state_bytes;
    }
    // the groups' step launches are independent (disjoint envs and output rows): run them concurrently,
    // group 0 on the caller's stream, group k > 0 on its own stream forked after the caller's prior work
    // and joined back before the caller's next work (stream order is kept for the caller)
    m->gstream = new hipStream_t[m->ngroups]();
    m->gev = new hipEvent_t[m->ngroups + 1]();
    for (int k = 0; k <= m->ngroups; ++k)
        if (hipEventCreateWithFlags(&m->gev[k], hipEventDisableTiming) != hipSuccess) {
            cn_destroy(m);
            return set_err(CN_EHIP, "hipEventCreate failed");
        }
    for (int k = 1; k < m->ngroups; ++k)
        if (hipStreamCreateWithFlags(&m->gstream[k], hipStreamNonBlocking) != hipSuccess) {
            cn_destroy(m);
            return set_err(CN_EHIP, "hipStreamCreate failed");
        }
    *out = m;
    return CN_OK;
}

// per-env human count of an engine (plain: N everywhere), into host memory [E]
int cn_env_humans(const cn_engine *g, int32_t *dst)
{
    if (!g || !dst) return set_err(CN_EINVAL, "null argument");
    if (!g->ngroups) {
        for (int64_t r = 0; r < g->E; ++r) dst[r] = g->N;
        return CN_OK;
    }
    for (int k = 0; k < g->ngroups; ++k) {
        const cn_engine *q = g->grp[k];
        std::vector<int32_t> rows(q->E);
        HIPCHK(hipMemcpy(rows.data(), q->rows, sizeof(int32_t) * q->E, hipMemcpyDeviceToHost));
        for (int64_t e = 0; e < q->E; ++e) dst[rows[e]] = q->N;
    }
    return CN_OK;
}

static void prof_free(cn_engine *g)
{
    if (g->ev) {
        for (int k = 0; k < 2; ++k) (void)hipEventDestroy(g->ev[k]);
        delete[] g->ev;
    }
    g->ev = nullptr;
    g->prof_cap = g->prof_n = g->prof_on = 0;
}

// Two events bracket the whole window of `max_steps` launches (one before the first, one after the
// last): per-launch event pairs cost ~12 us of stream time each on this GPU, more than the launch gaps
// they would exclude (back-to-back step launches are separated by < 0.2 us).
int cn_profile(cn_engine *g, int enable, int max_steps)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    prof_free(g);
    if (!enable) return CN_OK;
    if (max_steps <= 0) return set_err(CN_EINVAL, "max_steps must be > 0");
    g->ev = new hipEvent_t[2];
    for (int k = 0; k < 2; ++k) HIPCHK(hipEventCreate(&g->ev[k]));
    g->prof_cap = max_steps;
    g->prof_on = 1;
    return CN_OK;
}

int cn_profile_read(cn_engine *g, double *a_ms, double *b_ms, int64_t *launches)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    float ta = 0;
    if (g->prof_n > 0) {
        if (g->prof_n < g->prof_cap) return set_err(CN_EINVAL, "profile window not complete (fewer launches than max_steps)");
        HIPCHK(hipEventSynchronize(g->ev[1]));
        HIPCHK(hipEventElapsedTime(&ta, g->ev[0], g->ev[1]));
    }
    if (a_ms) *a_ms = ta;
    if (b_ms) *b_ms = 0;
    if (launches) *launches = g->prof_n;
    return CN_OK;
}

void cn_destroy(cn_engine *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    prof_free(g);
    if (g->grp) {
        for (int k = 0; k < g->ngroups; ++k) cn_destroy(g->grp[k]);
        if (g->gstream)
            for (int k = 1; k < g->ngroups; ++k) (void)hipStreamDestroy(g->gstream[k]);
        if (g->gev)
            for (int k = 0; k <= g->ngroups; ++k) (void)hipEventDestroy(g->gev[k]);
        delete[] g->grp;
        delete[] g->gstream;
        delete[] g->gev;
        delete g;
        return;
    }
    (void)hipFree(g->rows);
    (void)hipFree(g->state);
    (void)hipFree(g->work);
    (void)hipFree(g->work_count);
    (void)hipFree(g->plist);
    (void)hipFree(g->rlist);
    (void)hipFree(g->pend_mem);
    (void)hipFree(g->act_x);
    delete g;
}

// A mixed engine's groups work side by side on disjoint envs and rows: group 0 on the caller's stream, group
// k > 0 on its own, which waits for the caller's prior work (mix_fork) and which the caller's next work waits for
// (mix_join). One fork and one join bracket everything a call launches for the groups.
static hipStream_t mix_stream(const cn_engine *m, int k, hipStream_t st) { return k > 0 ? m->gstream[k] : st; }

static int mix_fork(cn_engine *m, hipStream_t st)
{
    if (m->ngroups < 2) return CN_OK;
    HIPCHK(hipEventRecord(m->gev[0], st));
    for (int k = 1; k < m->ngroups; ++k) HIPCHK(hipStreamWaitEvent(m->gstream[k], m->gev[0], 0));
    return CN_OK;
}

// (also after a failed launch, so that no side-stream work outlives the caller's order)
static int mix_join(cn_engine *m, hipStream_t st)
{
    hipError_t e = hipSuccess;
    for (int k = 1; k < m->ngroups; ++k) {
        const hipError_t e1 = hipEventRecord(m->gev[k], m->gstream[k]);
        const hipError_t e2 = hipStreamWaitEvent(st, m->gev[k], 0);
        if (e == hipSuccess) e = e1 != hipSuccess ? e1 : e2;
    }
    return e == hipSuccess ? CN_OK : set_err(CN_EHIP, "HIP error: %s", hipGetErrorString(e));
}

// every env holonomic (the scripted controllers return ActionXY)
static bool all_holonomic(const cn_engine *g)
{
    for (int k = 0; k < g->ngroups; ++k)
        if (g->grp[k]->c.kinematics != CN_HOLONOMIC) return false;
    return g->ngroups || g->c.kinematics == CN_HOLONOMIC;
}

int cn_reset(cn_engine *g, void *stream, float *robot_node, float *temporal, float *spatial)
{
    if (!g || !robot_node || !temporal || !spatial) return set_err(CN_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (g->ngroups) {
        for (int k = 0; k < g->ngroups; ++k) {
            const int rc = cn_reset(g->grp[k], stream, robot_node, temporal, spatial);
            if (rc) return rc;
        }
        return CN_OK;
    }
    RngArgs a;
    a.o.s = g->s; a.o.robot_node = robot_node; a.o.temporal = temporal; a.o.spatial = spatial;
    a.o.case_size = g->case_size;
    a.o.ov.row = g->rows; a.o.ov.NS = g->NS;
    a.pend = g->pend; a.E = g->E; a.counter_offset = g->counter_offset;
    // the reset kernel draws the next two spawns too, so the first step launches (whose spawns would otherwise
    // run inline in step workgroups until the budgeted spawn waves catch up) find them drawn (PEND_FRESH)
    a.draw_next = 1;
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_reset_kernel, dim3(g->rng_grid), dim3(64), 0, st, a, g->c);
    HIPCHK(hipGetLastError());
    // every env starts a new episode with its next two spawns drawn: the next step launch draws them (none)
    // and ignores the earlier launches' lists (host flag; graph mode: the device flag, stream-ordered)
    g->pend_all = PEND_FRESH;
    if (g->devseq) return ctl_set(g->work_count + CN_CTL_ALL, (uint32_t)g->pend_all, st);
    return CN_OK;
}

// One step launch. nsteps == 1: cn_step's launch (every engine, graph mode). nsteps > 1: a multi-step launch of
// cn_step_seq (a quad-path engine or group outside graph mode, pend_all == 0: seq_fusable), whose step workgroups
// run nsteps steps with the actions at actions + t * action_stride. g->nstep counts LAUNCHES (the triple-buffer
// index of the spawn lists, the launch id, graph mode's hand-over); cn_profile's window counts STEPS.
// rollout >= 0 (cn_rollout's fused launches, nsteps >= 1, same engines): StepArgs::rollout of the ROBOT kernels,
// which compute the actions themselves and record every step at row t of the outputs (`actions` is written).
// rec (cn_rollout_lidar's fused launches): the ROBOT kernels that record the state rows as well (RolloutRows block).
// mask (cn_rollout_masked's fused launches, never with rec): the ROBOT kernels that record the visible_masks rows as
// well, from the launch's row 0 (StepArgs::mask).
static int step_launch(cn_engine *g, void *stream, const float *actions, int nsteps, int64_t action_stride,
                       float *robot_node, float *temporal, float *spatial, float *reward, uint8_t *done, int8_t *event,
                       float *info, double *ep_return, int32_t *ep_len, int64_t rollout = -1, bool rec = false,
                       float *mask = nullptr)
{
    if (!g || !actions || !robot_node || !temporal || !spatial) return set_err(CN_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const uint64_t t = g->nstep++;   // this launch's number (host sequence; graph mode keeps its own on the device)
    // the window's events: before the launch of its first step, after the launch that completes the count
    // (cn_step_seq splits a chunk that would straddle the end of the window)
    const bool prof = g->prof_on && g->prof_n < g->prof_cap;
    if (prof && g->prof_n == 0) HIPCHK(hipEventRecord(g->ev[0], st));
    if (g->ngroups) {   // one step launch per group, concurrently (fork / join around the caller's stream)
        int rc = mix_fork(g, st);
        if (rc) return rc;
        for (int k = 0; k < g->ngroups && !rc; ++k)
            rc = cn_step(g->grp[k], (void *)mix_stream(g, k, st), actions, robot_node, temporal, spatial, reward, done,
                         event, info, ep_return, ep_len);
        const int rj = mix_join(g, st);
        if (rc || rj) return rc ? rc : rj;
        if (prof && ++g->prof_n == g->prof_cap) HIPCHK(hipEventRecord(g->ev[1], st));
        return CN_OK;
    }
    StepArgs a;
    a.s = g->s; a.actions = actions; a.robot_node = robot_node; a.temporal = temporal; a.spatial = spatial;
    a.reward = reward; a.done = done; a.event = event; a.info = info; a.ep_return = ep_return; a.ep_len = ep_len;
    a.E = g->E;
    a.case_size = g->case_size;
    a.ctl = g->work_count; a.plist_base = g->plist; a.rlist_base = g->rlist;
    step_list_slots(g, t, a);
    // the budget is clock cycles per STEP: a multi-step launch lasts nsteps times as long and draws the spawns its
    // predecessor queued over as many steps, so its spawning waves get nsteps times the budget, the default one
    // and one set through cn_debug_set_spawn_budget alike. (Taken per launch, a small test budget left a run of
    // 300 steps with ~10 launches of one or two humans' progress each: no parked spawn ever completed.)
    a.pend.budget = g->spawn_budget * nsteps;
    a.nsteps = nsteps;
    if (nsteps > 1) a.action_stride = action_stride;   // (shares ctl's slot: the SEQ kernels are never graph mode's)
    if (rollout >= 0) a.rollout = rollout;
    a.pend.stats = g->work_count + 8;
    const int blocks = (g->E + g->plan.EPB - 1) / g->plan.EPB;
    a.pend.P = g->pend;
    a.pend.all = g->pend_all;
    a.pend.step_blocks = blocks; a.pend.pend_blocks = g->pend_blocks; a.pend.counter_offset = g->counter_offset;
    a.pend.first = g->plan.kd ? 1 : 0;
    a.pend.waves = g->pend_waves;
    a.pend.stride = g->plan.rng_stride;
    a.pend.case_size = g->case_size;
    a.ov.row = g->rows; a.ov.NS = g->NS;
    a.pend.ov = a.ov;
    a.cth_h = cos(g->c.human_fov / 2); a.cth_r = cos(g->c.robot_fov / 2);
    g->pend_all = 0;
    const int grid = blocks + g->pend_blocks;
    const bool phx = g->c.rng_mode == CN_RNG_PHILOX;
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    const bool multi = nsteps > 1 || rollout >= 0;
    if (multi && (g->devseq || g->plan.kd || a.pend.all || (rec && (g->rows || mask))))
        return set_err(CN_EINVAL, "multi-step launch: quad-path engine outside graph mode required");
    if (mask && rollout >= 0) a.mask = mask;   // (shares rlist_base's slot: the ROBOT kernels are never graph mode's)
    const StepMode mode = rollout >= 0 ? (rec ? STEP_ROBOT_REC : mask ? STEP_ROBOT_MASK : STEP_ROBOT)
                          : nsteps > 1 ? STEP_SEQ : g->devseq ? STEP_DEVSEQ : STEP_SINGLE;
    const StepKernelFn kern = step_kernel_for(g->plan.kd, phx, g->rows != nullptr, mode);
    // (a guard only: the check above and cn_set_graph_mode's refusal of mixed engines exclude every combination
    // the table lacks, so no caller reaches this today)
    if (!kern) return set_err(CN_EINVAL, "step launch: this engine has no kernel for this launch mode");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(g->plan.T), g->a_lds, st, a, g->c);
    HIPCHK(hipGetLastError());
    if (prof && (g->prof_n += nsteps) >= g->prof_cap) HIPCHK(hipEventRecord(g->ev[1], st));
    return CN_OK;
}

int cn_step(cn_engine *g, void *stream, const float *actions, float *robot_node, float *temporal, float *spatial,
            float *reward, uint8_t *done, int8_t *event, float *info, double *ep_return, int32_t *ep_len)
{
    return step_launch(g, stream, actions, 1, 0, robot_node, temporal, spatial, reward, done, event, info, ep_return,
                       ep_len);
}

// T steps as ceil(T / C) multi-step launches of up to C = seq_chunk steps (the last one of the remainder), with
// the results of T cn_step launches bit for bit. A launch per step where the multi-step kernels do not apply:
// C == 1, graph mode, the kd-tree path (> 10 agents per simulator), and the first launch after
// cn_reset / cn_set_state (pend_all != 0: its spawn waves redraw or ignore the pending lists; the chunks start
// after it). g: a plain engine, a group of a mixed engine on its own stream (the rule applies to the group's
// own count), or a mixed engine stepped as a whole (fuse false: a launch per group and step, cn_step's).
static int step_seq_run(cn_engine *g, void *stream, bool fuse, int T, const float *actions, int64_t action_stride,
                        float *robot_node, float *temporal, float *spatial, float *reward, uint8_t *done, int8_t *event,
                        float *info, double *ep_return, int32_t *ep_len)
{
    const bool fusable = fuse && g->seq_chunk > 1 && !g->ngroups && !g->devseq && !g->plan.kd;
    for (int t = 0; t < T;) {
        int n = 1;
        if (fusable && !g->pend_all) {
            n = T - t < g->seq_chunk ? T - t : g->seq_chunk;
            // a chunk never straddles the end of cn_profile's window: its last event follows the launch that
            // completes the count
            if (g->prof_on && g->prof_n < g->prof_cap && n > g->prof_cap - g->prof_n) n = g->prof_cap - g->prof_n;
        }
        const int rc = step_launch(g, stream, actions + (int64_t)t * action_stride, n, action_stride, robot_node,
                                   temporal, spatial, reward, done, event, info, ep_return, ep_len);
        if (rc) return rc;
        t += n;
    }
    return CN_OK;
}

// A mixed engine: every group runs its whole T-step sequence on its own stream (the groups never read each
// other's rows), one fork before the first and one join after the last launch of the call. While a cn_profile
// window is open the mixed engine steps as a whole, a step at a time, so that the window counts steps.
int cn_step_seq(cn_engine *g, void *stream, int T, const float *actions, int64_t action_stride, float *robot_node,
                float *temporal, float *spatial, float *reward, uint8_t *done, int8_t *event, float *info,
                double *ep_return, int32_t *ep_len)
{
    if (!g || !actions) return set_err(CN_EINVAL, "null argument");
    if (T < 0 || (T > 1 && action_stride < 2 * g->E))
        return set_err(CN_EINVAL, "cn_step_seq: T >= 0 and action_stride >= 2 * E required");
    if (!g->ngroups || (g->prof_on && g->prof_n < g->prof_cap) || T == 0) {
        if (T > 0 && (!robot_node || !temporal || !spatial)) return set_err(CN_EINVAL, "null argument");
        return step_seq_run(g, stream, !g->ngroups, T, actions, action_stride, robot_node, temporal, spatial, reward,
                            done, event, info, ep_return, ep_len);
    }
    if (!robot_node || !temporal || !spatial) return set_err(CN_EINVAL, "null argument");
    const hipStream_t st = (hipStream_t)stream;
    int rc = mix_fork(g, st);
    if (rc) return rc;
    for (int k = 0; k < g->ngroups && !rc; ++k)
        rc = step_seq_run(g->grp[k], (void *)mix_stream(g, k, st), true, T, actions, action_stride, robot_node,
                          temporal, spatial, reward, done, event, info, ep_return, ep_len);
    const int rj = mix_join(g, st);
    return rc ? rc : rj;
}

int cn_set_graph_mode(cn_engine *g, void *stream, int on)
{
    if (!g) return set_err(CN_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (g->ngroups || g->rows) return set_err(CN_EUNSUPPORTED, "graph mode: plain engines only (not cn_create_mixed)");
    if (on && !g->devseq) {   // hand the host sequence to the device
        g->ctl_host[0] = (uint32_t)g->nstep; g->ctl_host[1] = (uint32_t)g->pend_all; g->ctl_host[2] = 0u;
        HIPCHK(hipMemcpyAsync(g->work_count + CN_CTL_NSTEP, g->ctl_host, 3 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));   // ctl_host may be rewritten by the next call
    } else if (!on && g->devseq) {   // and back
        HIPCHK(hipMemcpyAsync(g->ctl_host, g->work_count + CN_CTL_NSTEP, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        g->nstep = g->ctl_host[0]; g->pend_all = (int)g->ctl_host[1];
    }
    g->devseq = on ? 1 : 0;
    return CN_OK;
}

int cn_state_bytes(const cn_engine *g, int64_t *bytes)
{
    if (!g || !bytes) return set_err(CN_EINVAL, "null argument");
    *bytes = g->state_bytes;
    return CN_OK;
}

const void *cn_state_device_ptr(const cn_engine *g) { return g && !g->ngroups ? g->state : nullptr; }

int cn_get_state(cn_engine *g, void *stream, void *dst, int dst_on_host)
{
    if (!g || !dst) return set_err(CN_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (g->ngroups) {   // the groups' blobs, concatenated in group order
        char *d = (char *)dst;
        for (int k = 0; k < g->ngroups; ++k) {
            const int rc = cn_get_state(g->grp[k], stream, d, dst_on_host);
            if (rc) return rc;
            d += g->grp[k]->state_bytes;
        }
        return CN_OK;
    }
    if (dst_on_host) {
        HIPCHK(hipMemcpyAsync(dst, g->state, g->state_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } else {
        HIPCHK(hipMemcpyAsync(dst, g->state, g->state_bytes, hipMemcpyDeviceToDevice, st));
    }
    return CN_OK;
}

int cn_set_state(cn_engine *g, void *stream, const void *src, int src_on_host)
{
    if (!g || !src) return set_err(CN_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (g->ngroups) {
        const char *d = (const char *)src;
        for (int k = 0; k < g->ngroups; ++k) {
            const int rc = cn_set_state(g->grp[k], stream, d, src_on_host);
            if (rc) return rc;
            d += g->grp[k]->state_bytes;
        }
        return CN_OK;
    }
    if (src_on_host) {
        HIPCHK(hipMemcpyAsync(g->state, src, g->state_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    } else {
        HIPCHK(hipMemcpyAsync(g->state, src, g->state_bytes, hipMemcpyDeviceToDevice, st));
    }
    // pending spawns are keyed by (case_counter, reset_count); redraw them for the new state, keyed from a
    // snapshot of its counters (the next launch's own resets rewrite the state's while its spawn waves run)
    g->pend_all = PEND_BOTH;
    const int rk = keysnap(g, st);
    if (rk) return rk;
    if (g->devseq) return ctl_set(g->work_count + CN_CTL_ALL, PEND_BOTH, st);
    return CN_OK;
}

#ifdef CN_STAMPS
int cn_debug_stamps_c(unsigned long long *c, unsigned long long *p)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(c, HIP_SYMBOL(cn_stamp_c), sizeof(unsigned long long) * 8192 * 4));
    HIPCHK(hipMemcpyFromSymbol(p, HIP_SYMBOL(cn_stamp_p), sizeof(unsigned long long) * 8192 * 2));
    return CN_OK;
}

// per-workgroup start / end on the device-wide 100 MHz realtime clock; spawn_env's segment stamps
int cn_debug_stamps_r(unsigned long long *r, unsigned long long *sp)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(r, HIP_SYMBOL(cn_stamp_r), sizeof(unsigned long long) * 8192 * 2));
    if (sp) HIPCHK(hipMemcpyFromSymbol(sp, HIP_SYMBOL(cn_stamp_s), sizeof(unsigned long long) * 8192 * 16));
    return CN_OK;
}

// per workgroup [8192][4]: HW_REG_XCC_ID, HW_REG_HW_ID, start / end on the XCD's shader clock
int cn_debug_stamps_x(unsigned long long *x)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(x, HIP_SYMBOL(cn_stamp_x), sizeof(unsigned long long) * 8192 * 4));
    return CN_OK;
}

// phase 2 per wave [4096][4][CN_NWSTAMP] (stamps.h: STAMP_W)
int cn_debug_stamps_w(unsigned long long *w)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(w, HIP_SYMBOL(cn_stamp_w), sizeof(unsigned long long) * 4096 * 4 * CN_NWSTAMP));
    return CN_OK;
}

int cn_debug_stamps(unsigned long long *a, unsigned long long *b)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(a, HIP_SYMBOL(cn_stamp_a), sizeof(unsigned long long) * 4096 * CN_NSTAMP));
    HIPCHK(hipMemcpyFromSymbol(b, HIP_SYMBOL(cn_stamp_b), sizeof(unsigned long long) * 8192 * CN_NSTAMP));
    return CN_OK;
}
#endif

int cn_debug_set_spawn_budget(cn_engine *g, long long cycles)
{
    if (!g || cycles < 0) return set_err(CN_EINVAL, "cn_debug_set_spawn_budget: engine and cycles >= 0 required");
    for (int k = 0; k < g->ngroups; ++k) cn_debug_set_spawn_budget(g->grp[k], cycles);
    if (!g->ngroups) g->spawn_budget = cycles;
    return CN_OK;
}

int cn_debug_set_seq_chunk(cn_engine *g, int n)
{
    if (!g || n < 1) return set_err(CN_EINVAL, "cn_debug_set_seq_chunk: engine and n >= 1 required");
    for (int k = 0; k < g->ngroups; ++k) cn_debug_set_seq_chunk(g->grp[k], n);   // (each group chunks its own steps)
    g->seq_chunk = n;
    return CN_OK;
}

int cn_debug_spawn_stats(cn_engine *g, uint32_t *out)
{
    if (!g || !out) return set_err(CN_EINVAL, "null argument");
    for (int j = 0; j < 5; ++j) out[j] = 0;
    if (g->ngroups) {
        for (int k = 0; k < g->ngroups; ++k) {
            uint32_t v[5];
            const int rc = cn_debug_spawn_stats(g->grp[k], v);
            if (rc) return rc;
            for (int j = 0; j < 5; ++j) out[j] += v[j];
        }
        return CN_OK;
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, g->work_count + 8, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + 4, g->work_count + 15, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CN_OK;
}

int cn_lidar_obs(cn_engine *g, void *stream, const uint8_t *reset_mask, int enable, int beams, double max_range,
                 double robot_radius, float *lidar, float *obs)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (g->ngroups) return set_err(CN_EUNSUPPORTED, "cn_lidar_obs: not on a mixed engine");
    if (beams < 2 || beams > 4096 || !(max_range > 0) || !lidar || !obs)
        return set_err(CN_EINVAL, "cn_lidar_obs: beams in [2, 4096], max_range > 0 and buffers required");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_lidar_obs_kernel, dim3((unsigned)((g->E + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g->s,
                       g->E, g->N, 0.5 * g->c.square_width, reset_mask, enable, beams, max_range, robot_radius,
                       lidar, obs);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

// cn_lidar_scan's argument check (cn_rollout_lidar's too); *npts: the samples of a beam
static int lidar_scan_check(int beams, double max_range, const float *obs, int *npts)
{
    if (beams < 2 || beams > 4096 || !(max_range > 0) || !(max_range <= 1e4) || !obs)
        return set_err(CN_EINVAL, "cn_lidar_scan: beams in [2, 4096], max_range in (0, 1e4] and obs required");
    // beam samples every 0.01 m (lidarv2.py:130-133): max_range / 0.01 of them, rounded up
    const double q = max_range / 0.01;
    *npts = fmod(q, 1.0) != 0.0 ? (int)q + 1 : (int)q;
    if (*npts < 2) return set_err(CN_EINVAL, "cn_lidar_scan: max_range below two 0.01 m samples");
    return CN_OK;
}

// The scan of `rows` state rows behind S (the engine's blob: rows = E; cn_rollout_lidar's state rows: T * E, human i
// of row r at r * N + i) into obs [rows][7 + beams]. One launch, unless the kernel's int indices (r * N + i) would
// overflow: then one per span of rows that fits. *launches (may be null) counts them.
static int lidar_scan_launch(const cn_engine *g, hipStream_t st, cn_state_ptrs S, int64_t rows, int beams, int npts,
                             double max_range, double robot_radius, float *obs, int *launches)
{
    // rows per workgroup: the G in [1, CN_LIDAR_G] whose G * beams beams fill whole 256-lane rounds best
    int G = 1;
    double fill = 0.0;
    for (int k = 1; k <= CN_LIDAR_G && k <= rows; ++k) {
        const int items = k * beams;
        const double f = (double)items / (double)(((items + 255) / 256) * 256);
        if (f > fill + 1e-9) { fill = f; G = k; }
    }
    const int64_t N = g->N;
    int64_t span = ((int64_t)0x7fffffff / (N > 0 ? N : 1) - CN_LIDAR_G) / G * G;   // (r + G) * N stays an int
    for (int64_t r0 = 0; r0 < rows; r0 += span) {
        const int64_t n = rows - r0 < span ? rows - r0 : span;
        cn_state_ptrs P = S;
        P.r_px += r0; P.r_py += r0; P.r_vx += r0; P.r_vy += r0; P.r_radius += r0; P.r_gx += r0; P.r_gy += r0;
        P.r_vpref += r0; P.r_theta += r0;
        P.h_px += r0 * N; P.h_py += r0 * N; P.h_r += r0 * N;
        (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
        hipLaunchKernelGGL(cn_lidar_scan_kernel, dim3((unsigned)((n + G - 1) / G)), dim3(256), 0, st, P, (int)n, g->N, G,
                           0.5 * g->c.square_width, beams, npts, max_range, robot_radius, obs + r0 * (7 + beams));
        HIPCHK(hipGetLastError());
        if (launches) *launches += 1;
    }
    return CN_OK;
}

int cn_lidar_scan(cn_engine *g, void *stream, int beams, double max_range, double robot_radius, float *obs)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (g->ngroups) return set_err(CN_EUNSUPPORTED, "cn_lidar_scan: not on a mixed engine");
    int npts;
    const int rc = lidar_scan_check(beams, max_range, obs, &npts);
    if (rc) return rc;
    return lidar_scan_launch(g, (hipStream_t)stream, g->s, g->E, beams, npts, max_range, robot_radius, obs, nullptr);
}

// cn_robot_act's launch for a plain engine or a group of a mixed engine (its own count picks the kernel; its envs'
// actions go to their rows of the caller's buffer). regret != NULL (cn_robot_act_regret, CN_ROBOT_DWA only): the
// controller's regret kernel in place of the plain one, the envs' regret rows at the same rows of that buffer.
static int robot_act_launch(const cn_engine *g, hipStream_t st, int policy, float *actions, float *regret = nullptr)
{
    const cn_config &c = g->c;
    const int32_t *const rows = g->rows;   // a group: the *_mix_kernel twins (the same bodies, the actions at rows[e])
    const int uni = c.kinematics != CN_HOLONOMIC;   // (cn_scripted_unicycle let it through): robot_unicycle_track
    const dim3 quads((unsigned)((g->E + 15) / 16)), lanes((unsigned)((g->E + 63) / 64));
    const float nd = (float)c.orca_neighbor_dist, th = (float)c.orca_time_horizon, ts = (float)c.time_step;
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    if (policy == CN_ROBOT_DWA) {   // (cn_scripted_dwa let it through: a unicycle engine) a wave per env
        const dim3 waves((unsigned)((g->E + CN_DWA_WAVES - 1) / CN_DWA_WAVES)), wg(64 * CN_DWA_WAVES);
        if (regret && rows)
            hipLaunchKernelGGL(cn_robot_dwa_regret_mix_kernel, waves, wg, 0, st, g->s, g->E, g->N, c.time_step, g->dwa_p,
                               actions, rows, regret);
        else if (regret)
            hipLaunchKernelGGL(cn_robot_dwa_regret_kernel, waves, wg, 0, st, g->s, g->E, g->N, c.time_step, g->dwa_p,
                               actions, regret);
        else if (rows)
            hipLaunchKernelGGL(cn_robot_dwa_mix_kernel, waves, wg, 0, st, g->s, g->E, g->N, c.time_step, g->dwa_p, actions,
                               rows);
        else
            hipLaunchKernelGGL(cn_robot_dwa_kernel, waves, wg, 0, st, g->s, g->E, g->N, c.time_step, g->dwa_p, actions);
    } else if (policy == CN_ROBOT_SOCIAL_FORCE) {
        if (rows)
            hipLaunchKernelGGL(cn_robot_sf_mix_kernel, lanes, dim3(64), 0, st, g->s, g->E, g->N, c.sf_A, c.sf_B, c.sf_KI,
                               c.time_step, actions, rows, uni);
        else
            hipLaunchKernelGGL(cn_robot_sf_kernel, lanes, dim3(64), 0, st, g->s, g->E, g->N, c.sf_A, c.sf_B, c.sf_KI,
                               c.time_step, actions, uni);
    } else if (g->N + 1 > 10) {
        if (rows)
            hipLaunchKernelGGL(cn_robot_orca_kd_mix_kernel, quads, dim3(64), orca_kd_lds(g->N + 1), st, g->s, g->E, g->N,
                               c.orca_safety_space, nd, th, ts, actions, rows, uni);
        else
            hipLaunchKernelGGL(cn_robot_orca_kd_kernel, quads, dim3(64), orca_kd_lds(g->N + 1), st, g->s, g->E, g->N,
                               c.orca_safety_space, nd, th, ts, actions, uni);
    } else {
        if (rows)
            hipLaunchKernelGGL(cn_robot_orca_mix_kernel, quads, dim3(64), 0, st, g->s, g->E, g->N, c.orca_safety_space, nd,
                               th, ts, actions, rows, uni);
        else
            hipLaunchKernelGGL(cn_robot_orca_kernel, quads, dim3(64), 0, st, g->s, g->E, g->N, c.orca_safety_space, nd, th,
                               ts, actions, uni);
    }
    HIPCHK(hipGetLastError());
    return CN_OK;
}

// The scripted calls on a mixed engine are an opt-in of the engine (off: they refuse it as they always have).
int cn_mixed_scripted(cn_engine *g, int on)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (!g->ngroups) return set_err(CN_EINVAL, "cn_mixed_scripted: a mixed engine (cn_create_mixed) required");
    g->scripted = on ? 1 : 0;
    return CN_OK;
}

// The scripted calls on a unicycle engine (plain, or a mixed engine with a unicycle group) are an opt-in as well: on,
// the controllers' velocity goes through robot_unicycle_track and the calls return the step's (dv, dtheta); off, they
// refuse the engine as they always have. A holonomic engine computes what it computed either way.
int cn_scripted_unicycle(cn_engine *g, int on)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    g->scripted_uni = on ? 1 : 0;
    return CN_OK;
}

// cn_dwa_predict's and cn_scripted_dwa's rule for the parameters
static bool dwa_params_ok(const cn_dwa_params *p)
{
    return p && p->horizon >= 1 && p->horizon <= 16 && isfinite(p->w_goal) && isfinite(p->w_clear) &&
           isfinite(p->w_col) && isfinite(p->d_safe) && p->d_safe > 0;
}

// CN_ROBOT_DWA is an opt-in of the engine too: off, the id is the unknown policy it always was. The controller emits
// the unicycle action, so only an engine whose envs are all unicycle can switch it on. A mixed engine's groups launch
// with their own copy of the parameters.
int cn_scripted_dwa(cn_engine *g, const cn_dwa_params *p)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (p) {
        if (!dwa_params_ok(p))
            return set_err(CN_EINVAL, "cn_scripted_dwa: horizon in [1, 16], d_safe > 0 and finite weights required");
        bool uni = g->ngroups || g->c.kinematics == CN_UNICYCLE;
        for (int k = 0; k < g->ngroups; ++k) uni = uni && g->grp[k]->c.kinematics == CN_UNICYCLE;
        if (!uni) return set_err(CN_EUNSUPPORTED, "cn_scripted_dwa: the controller emits (dv, dtheta): unicycle engines only");
    }
    for (int k = -1; k < g->ngroups; ++k) {
        cn_engine *q = k < 0 ? g : g->grp[k];
        q->dwa = p ? 1 : 0;
        if (p) q->dwa_p = *p;
    }
    return CN_OK;
}

// A mixed engine (after cn_mixed_scripted): one controller launch per group, side by side like the groups' step
// launches. regret != NULL: cn_robot_act_regret, which has checked its own arguments and that the policy is the
// dynamic window.
static int robot_act_checked(cn_engine *g, void *stream, int policy, float *actions, float *regret)
{
    const bool dwa = policy == CN_ROBOT_DWA && g->dwa;   // (without cn_scripted_dwa the id is unknown, as ever)
    if ((policy != CN_ROBOT_ORCA && policy != CN_ROBOT_SOCIAL_FORCE && !dwa) || !actions)
        return set_err(CN_EINVAL, "cn_robot_act: policy CN_ROBOT_ORCA / CN_ROBOT_SOCIAL_FORCE and actions required");
    if (g->ngroups && !g->scripted)
        return set_err(CN_EUNSUPPORTED, "cn_robot_act: not on a mixed engine (unless cn_mixed_scripted enabled it)");
    if (!dwa && !all_holonomic(g) && !g->scripted_uni)
        return set_err(CN_EUNSUPPORTED, g->ngroups ? "cn_robot_act: not on a unicycle mixed engine (the controllers return ActionXY)"
                                                   : "cn_robot_act: the controllers return ActionXY (holonomic engines only)");
    const hipStream_t st = (hipStream_t)stream;
    if (!g->ngroups) return robot_act_launch(g, st, policy, actions, regret);
    int rc = mix_fork(g, st);
    if (rc) return rc;
    for (int k = 0; k < g->ngroups && !rc; ++k)
        rc = robot_act_launch(g->grp[k], mix_stream(g, k, st), policy, actions, regret);
    const int rj = mix_join(g, st);
    return rc ? rc : rj;
}

int cn_robot_act(cn_engine *g, void *stream, int policy, float *actions)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    return robot_act_checked(g, stream, policy, actions, nullptr);
}

// cn_robot_act_regret's and cn_robot_mix_regret's rule for the policy: only the dynamic window has a candidate set
static int regret_policy_check(const cn_engine *g, int policy)
{
    if (policy == CN_ROBOT_ORCA || policy == CN_ROBOT_SOCIAL_FORCE)
        return set_err(CN_EUNSUPPORTED, "regret rows: ORCA and the social force have no candidate set (CN_ROBOT_DWA only)");
    if (policy != CN_ROBOT_DWA || !g->dwa)
        return set_err(CN_EINVAL, "regret rows: policy CN_ROBOT_DWA on an engine cn_scripted_dwa enabled it for required");
    return CN_OK;
}

// cn_robot_act with the controller's regret kernel in place of the plain one: the same launch count.
int cn_robot_act_regret(cn_engine *g, void *stream, int policy, float *actions, float *regret)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (!actions || !regret) return set_err(CN_EINVAL, "cn_robot_act_regret: actions and regret required");
    const int rc = regret_policy_check(g, policy);
    if (rc) return rc;
    return robot_act_checked(g, stream, policy, actions, regret);
}

// By value through a kernel, as cn_rollout_noisy hands its block over: stream-ordered, a kernel node when captured.
int cn_mix_ctl_set(void *stream, cn_mix_ctl *dev, const cn_mix_ctl *value)
{
    if (!dev || !value) return set_err(CN_EINVAL, "cn_mix_ctl_set: dev and value required");
    if (!(value->beta >= 0.0f && value->beta <= 1.0f))   // (a NaN fails both)
        return set_err(CN_EINVAL, "cn_mix_ctl_set: beta in [0, 1] required");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_mix_ctl_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dev, *value);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

// cn_robot_act into `label` (its checks, its launches, a mixed engine's fork and join), then one launch over all E
// rows on the caller's stream.
static int robot_mix_checked(cn_engine *g, void *stream, int policy, const float *learner, const cn_mix_ctl *ctl,
                             int32_t t, float *label, float *executed, uint8_t *flags, float *regret)
{
    if (!learner || !ctl || !label || !executed || !flags || t < 0)
        return set_err(CN_EINVAL, "cn_robot_mix: learner, ctl, label, executed, flags and t >= 0 required");
    const int rc = robot_act_checked(g, stream, policy, label, regret);   // (every check of it comes before its first launch)
    if (rc) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_robot_mix_kernel, dim3((unsigned)((g->E + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint2 *)learner, ctl, t, (uint32_t)(uint64_t)g->c.env_offset, (int)g->E,
                       (const uint2 *)label, (uint2 *)executed, flags);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

int cn_robot_mix(cn_engine *g, void *stream, int policy, const float *learner, const cn_mix_ctl *ctl, int32_t t,
                 float *label, float *executed, uint8_t *flags)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    return robot_mix_checked(g, stream, policy, learner, ctl, t, label, executed, flags, nullptr);
}

// cn_robot_mix with cn_robot_act_regret's launch(es) in place of cn_robot_act's
int cn_robot_mix_regret(cn_engine *g, void *stream, int policy, const float *learner, const cn_mix_ctl *ctl, int32_t t,
                        float *label, float *executed, uint8_t *flags, float *regret)
{
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (!regret) return set_err(CN_EINVAL, "cn_robot_mix_regret: regret required");
    if (!learner || !ctl || !label || !executed || !flags || t < 0)
        return set_err(CN_EINVAL, "cn_robot_mix_regret: learner, ctl, label, executed, flags and t >= 0 required");
    const int rc = regret_policy_check(g, policy);
    if (rc) return rc;
    return robot_mix_checked(g, stream, policy, learner, ctl, t, label, executed, flags, regret);
}

// cn_visible_mask's launch for a plain engine or a group of a mixed engine (its envs' rows of the [E][NS] buffer)
static int visible_mask_launch(const cn_engine *g, hipStream_t st, float *mask)
{
    const cn_config &c = g->c;
    const int64_t n = (int64_t)g->E * g->NS;
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    const dim3 grid((unsigned)((n + 63) / 64));
    const int holo = c.kinematics == CN_HOLONOMIC ? 1 : 0;
    if (g->rows)
        hipLaunchKernelGGL(cn_visible_mask_kernel<true>, grid, dim3(64), 0, st, g->s, g->E, g->N, g->NS, holo, c.robot_fov,
                           cos(c.robot_fov / 2), mask, g->rows);
    else
        hipLaunchKernelGGL(cn_visible_mask_kernel<false>, grid, dim3(64), 0, st, g->s, g->E, g->N, g->NS, holo,
                           c.robot_fov, cos(c.robot_fov / 2), mask, (const int32_t *)nullptr);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

// One launch (a mixed engine: one per group, side by side like the groups' step launches); no engine state changes.
int cn_visible_mask(cn_engine *g, void *stream, float *mask)
{
    if (!g || !mask) return set_err(CN_EINVAL, "cn_visible_mask: engine and mask required");
    const hipStream_t st = (hipStream_t)stream;
    if (!g->ngroups) return visible_mask_launch(g, st, mask);
    int rc = mix_fork(g, st);
    if (rc) return rc;
    for (int k = 0; k < g->ngroups && !rc; ++k) rc = visible_mask_launch(g->grp[k], mix_stream(g, k, st), mask);
    const int rj = mix_join(g, st);
    return rc ? rc : rj;
}

// Steps [t0, t1) of a rollout call of T steps for g, a plain engine or a group of a mixed engine on its own stream:
// cn_robot_act + cn_step with every step recorded at row t of the caller's (T, ER, ..) buffers (ER = NS-strided rows
// of the whole engine; the group's envs at their own rows). Fused (the ROBOT kernels: up to seq_chunk steps per
// launch, the controller inside the step workgroups) where `fuse` allows, cn_step_seq's multi-step launches apply and
// the controller fits the step workgroup; launch pairs otherwise, the first step after cn_reset / cn_set_state
// included. The rule reads g's own human count.
// nz (cn_rollout_noisy, sigma > 0; null: cn_rollout): the step takes the perturbed action. The fused launches carry
// CN_ROLLOUT_NOISY and their first step's k in StepArgs::rollout and read the rest from the engine's RolloutNoise
// block, written once per call on the stream before the first of them; elsewhere cn_action_noise_kernel runs between
// the pair's two launches and the step reads the engine's scratch. Both key the noise by the global env index.
// ld (cn_rollout_lidar, plain engines; null: none): the state every step leaves goes to row t of ld's state rows -- the
// fused launches are the recording ROBOT kernels, told where through the engine's RolloutRows block (one small launch
// per call before the first of them); elsewhere cn_state_rows_kernel follows the step.
// mask (cn_rollout_masked; null: none; never with ld): the call's row 0 of the (T, ER, NS) visible_masks buffer (one
// row (ER, NS) without CN_ROLLOUT_OBS_EVERY_STEP). The fused launches are the mask-recording ROBOT kernels, handed
// their own row 0 in the kernel arguments (no launch added); elsewhere cn_visible_mask's launch follows the step, into
// the observation's row. *nl counts the launches.
static int rollout_steps(cn_engine *g, hipStream_t st, bool fuse, int policy, int t0, int t1, int T,
                         const cn_rollout_out *out, const cn_rollout_noise *nz, const struct cn_rollout_lidar *ld,
                         float *mask, int *nl)
{
    void *const stream = (void *)st;
    const int64_t E = g->ER, N = g->NS;
    const RolloutRows rows = {ld ? ld->robot_state : nullptr, ld ? ld->human_state : nullptr, out->actions, (int64_t)T};
    bool rows_set = false;
    const bool every = (out->flags & CN_ROLLOUT_OBS_EVERY_STEP) != 0;
    // the controller fits the step workgroup: social force (a lane per env) always, ORCA on its quad path, the
    // dynamic window (a wave per env) never
    const bool fits = policy == CN_ROBOT_SOCIAL_FORCE || (policy == CN_ROBOT_ORCA && g->N + 1 <= 10);
    const bool fusable = fuse && fits && g->seq_chunk > 1 && !g->devseq && !g->plan.kd;
    const int64_t rollout = (int64_t)policy | ((int64_t)(out->flags & CN_ROLLOUT_OBS_EVERY_STEP) << 8);
    bool block_set = false;
    for (int t = t0; t < t1;) {
        const int64_t ro = every ? t : 0;   // the observation's row
        float *const act = out->actions + t * E * 2;
        float *const rn = out->robot_node + ro * E * 7, *const te = out->temporal_edges + ro * E * 2;
        float *const se = out->spatial_edges + ro * E * N * 2;
        float *const mk = mask ? mask + ro * E * N : nullptr;
        float *const rw = out->reward ? out->reward + t * E : nullptr;
        uint8_t *const dn = out->done ? out->done + t * E : nullptr;
        int8_t *const ev = out->event ? out->event + t * E : nullptr;
        float *const inf = out->info ? out->info + t * E * CN_INFO_K : nullptr;
        double *const epr = out->ep_return ? out->ep_return + t * E : nullptr;
        int32_t *const epl = out->ep_len ? out->ep_len + t * E : nullptr;
        const uint32_t k = nz ? (uint32_t)(uint64_t)(nz->step0 + t) : 0u;   // the step's Philox counter
        int n = 1, rc;
        if (fusable && !g->pend_all) {
            n = t1 - t < g->seq_chunk ? t1 - t : g->seq_chunk;
            // (a launch never straddles the end of cn_profile's window: cn_step_seq)
            if (g->prof_on && g->prof_n < g->prof_cap && n > g->prof_cap - g->prof_n) n = g->prof_cap - g->prof_n;
            int64_t word = rollout;
            if (nz) {
                if (!block_set) {
                    const RolloutNoise v = {nz->sigma, nz->seed, nz->executed, out->actions};
                    (void)hipGetLastError();
                    hipLaunchKernelGGL(cn_noise_set_kernel, dim3(1), dim3(64), 0, st,
                                       (RolloutNoise *)(g->work_count + CN_NOISE_W), v);
                    HIPCHK(hipGetLastError());
                    block_set = true;
                    *nl += 1;
                }
                word |= CN_ROLLOUT_NOISY | ((int64_t)k << CN_ROLLOUT_K_SHIFT);
            }
            if (ld && !rows_set) {
                (void)hipGetLastError();
                hipLaunchKernelGGL(cn_rows_set_kernel, dim3(1), dim3(64), 0, st,
                                   (RolloutRows *)(g->work_count + CN_ROWS_W), rows);
                HIPCHK(hipGetLastError());
                rows_set = true;
                *nl += 1;
            }
            rc = step_launch(g, stream, act, n, 2 * E, rn, te, se, rw, dn, ev, inf, epr, epl, word, ld != nullptr, mk);
            *nl += 1;
        } else {
            rc = robot_act_launch(g, st, policy, act);
            if (rc) return rc;
            const float *stepped = act;
            if (nz) {
                (void)hipGetLastError();
                hipLaunchKernelGGL(cn_action_noise_kernel, dim3((unsigned)((g->E + 63) / 64)), dim3(64), 0, st, act,
                                   g->act_x, nz->executed ? nz->executed + t * E * 2 : nullptr, (int)g->E, nz->sigma,
                                   nz->seed, k, (uint32_t)(uint64_t)g->c.env_offset, (const int32_t *)g->rows);
                HIPCHK(hipGetLastError());
                stepped = g->act_x;
                *nl += 1;
            }
            rc = cn_step(g, stream, stepped, rn, te, se, rw, dn, ev, inf, epr, epl);
            *nl += 2;
            if (ld && !rc) {
                (void)hipGetLastError();
                hipLaunchKernelGGL(cn_state_rows_kernel, dim3((unsigned)((E + 63) / 64)), dim3(256), 0, st, g->s, rows,
                                   (int)E, (int)N, t * E);
                HIPCHK(hipGetLastError());
                *nl += 1;
            }
            if (mk && !rc) {
                rc = visible_mask_launch(g, st, mk);
                *nl += 1;
            }
        }
        if (rc) return rc;
        t += n;
    }
    return CN_OK;
}

// cn_rollout / cn_rollout_noisy / cn_rollout_lidar: the checks (all of them before any launch), then rollout_steps.
// A mixed engine: every group runs its whole T-step sequence on its own stream, fused chunks or launch pairs by its
// own count, between one fork and one join. While a cn_profile window is open on it, the mixed engine runs a step at a
// time instead (every group's launch pair or triple between a fork and a join per step), so the window counts steps.
// ld: one scan over the T * E state rows follows the last step.
static int rollout_run(cn_engine *g, void *stream, int policy, int T, const cn_rollout_out *out,
                       const cn_rollout_noise *nz, int32_t *num_launches, const struct cn_rollout_lidar *ld = nullptr,
                       float *mask = nullptr)
{
    if (num_launches) *num_launches = 0;
    if (!g) return set_err(CN_EINVAL, "null engine");
    const bool dwa = policy == CN_ROBOT_DWA && g->dwa;   // (without cn_scripted_dwa the id is unknown, as ever)
    if ((policy != CN_ROBOT_ORCA && policy != CN_ROBOT_SOCIAL_FORCE && !dwa) || T < 0 || !out || !out->actions ||
        !out->robot_node || !out->temporal_edges || !out->spatial_edges)
        return set_err(CN_EINVAL, "cn_rollout: policy CN_ROBOT_ORCA / CN_ROBOT_SOCIAL_FORCE, T >= 0, out with actions "
                                  "and the observation buffers required");
    if (g->ngroups && ld) return set_err(CN_EUNSUPPORTED, "cn_rollout: not on a mixed engine");
    if (g->ngroups && !g->scripted)
        return set_err(CN_EUNSUPPORTED, "cn_rollout: not on a mixed engine (unless cn_mixed_scripted enabled it)");
    if (!dwa && !all_holonomic(g) && !g->scripted_uni)
        return set_err(CN_EUNSUPPORTED, g->ngroups ? "cn_rollout: not on a unicycle mixed engine (the controllers return ActionXY)"
                                                   : "cn_rollout: the controllers return ActionXY (holonomic engines only)");
    const hipStream_t st = (hipStream_t)stream;
    int npts = 0;
    if (ld) {
        if (!ld->robot_state || !ld->human_state)
            return set_err(CN_EINVAL, "cn_rollout_lidar: lidar with obs, robot_state and human_state required");
        const int rc = lidar_scan_check(ld->beams, ld->max_range, ld->obs, &npts);
        if (rc) return rc;
    }
    int nl = 0, rc = CN_OK;
    if (!g->ngroups) {
        rc = rollout_steps(g, st, true, policy, 0, T, T, out, nz, ld, mask, &nl);
    } else if (g->prof_on && g->prof_n < g->prof_cap) {
        for (int t = 0; t < T && !rc; ++t) {
            const bool prof = g->prof_on && g->prof_n < g->prof_cap;
            if (prof && g->prof_n == 0) HIPCHK(hipEventRecord(g->ev[0], st));
            rc = mix_fork(g, st);
            if (rc) break;
            for (int k = 0; k < g->ngroups && !rc; ++k)
                rc = rollout_steps(g->grp[k], mix_stream(g, k, st), false, policy, t, t + 1, T, out, nz, nullptr, mask,
                                   &nl);
            const int rj = mix_join(g, st);
            if (!rc) rc = rj;
            if (!rc && prof && ++g->prof_n == g->prof_cap) HIPCHK(hipEventRecord(g->ev[1], st));
        }
    } else if (T > 0) {
        rc = mix_fork(g, st);
        if (rc) return rc;
        for (int k = 0; k < g->ngroups && !rc; ++k)
            rc = rollout_steps(g->grp[k], mix_stream(g, k, st), true, policy, 0, T, T, out, nz, nullptr, mask, &nl);
        const int rj = mix_join(g, st);
        if (!rc) rc = rj;
    }
    if (num_launches) *num_launches = nl;
    if (rc) return rc;
    if (ld && T > 0) {   // the observations of all T * E rows: the scan over a cn_state_ptrs aimed into the state rows
        const int64_t E = g->E, N = g->N;
        const int64_t RE = (int64_t)T * E;
        cn_state_ptrs P = g->s;
        double *const r = ld->robot_state, *const h = ld->human_state;
        P.r_px = r; P.r_py = r + RE; P.r_vx = r + 2 * RE; P.r_vy = r + 3 * RE; P.r_radius = r + 4 * RE;
        P.r_gx = r + 5 * RE; P.r_gy = r + 6 * RE; P.r_vpref = r + 7 * RE; P.r_theta = r + 8 * RE;
        P.h_px = h; P.h_py = h + RE * N; P.h_r = h + 2 * RE * N;
        rc = lidar_scan_launch(g, st, P, RE, ld->beams, npts, ld->max_range, ld->robot_radius, ld->obs, &nl);
        if (rc) return rc;
        if (num_launches) *num_launches = nl;
    }
    return CN_OK;
}

// sigma == 0: `executed` is a copy of the actions the rollout recorded (one launch)
static int executed_copy(const cn_engine *g, void *stream, int T, const cn_rollout_out *out,
                         const cn_rollout_noise *noise, int32_t *num_launches)
{
    const int64_t n = (int64_t)T * g->E * 2;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_copy32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       (const uint32_t *)out->actions, (uint32_t *)noise->executed);
    HIPCHK(hipGetLastError());
    if (num_launches) *num_launches += 1;
    return CN_OK;
}

int cn_rollout(cn_engine *g, void *stream, int policy, int T, const cn_rollout_out *out, int32_t *num_launches)
{
    return rollout_run(g, stream, policy, T, out, nullptr, num_launches);
}

int cn_rollout_noisy(cn_engine *g, void *stream, int policy, int T, const cn_rollout_out *out,
                     const cn_rollout_noise *noise, int32_t *num_launches)
{
    if (num_launches) *num_launches = 0;
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (!noise || !(noise->sigma >= 0.0f && noise->sigma <= 3.402823466e38f))   // (NaN fails both comparisons)
        return set_err(CN_EINVAL, "cn_rollout_noisy: noise with a finite sigma >= 0 required");
    if (noise->sigma > 0.0f) return rollout_run(g, stream, policy, T, out, noise, num_launches);
    // sigma == 0: cn_rollout itself; `executed` is a copy of the actions it recorded
    const int rc = rollout_run(g, stream, policy, T, out, nullptr, num_launches);
    if (rc || !noise->executed || T == 0) return rc;
    return executed_copy(g, stream, T, out, noise, num_launches);
}

int cn_rollout_lidar(cn_engine *g, void *stream, int policy, int T, const cn_rollout_out *out,
                     const cn_rollout_noise *noise, const struct cn_rollout_lidar *lidar, int32_t *num_launches)
{
    if (num_launches) *num_launches = 0;
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (!lidar) return set_err(CN_EINVAL, "cn_rollout_lidar: lidar required");
    if (noise && !(noise->sigma >= 0.0f && noise->sigma <= 3.402823466e38f))   // (NaN fails both comparisons)
        return set_err(CN_EINVAL, "cn_rollout_lidar: noise with a finite sigma >= 0 required");
    const bool noisy = noise && noise->sigma > 0.0f;
    const int rc = rollout_run(g, stream, policy, T, out, noisy ? noise : nullptr, num_launches, lidar);
    if (rc || noisy || !noise || !noise->executed || T == 0) return rc;
    // sigma == 0: cn_rollout_noisy's copy of the actions into `executed`
    return executed_copy(g, stream, T, out, noise, num_launches);
}

int cn_rollout_masked(cn_engine *g, void *stream, int policy, int T, const cn_rollout_out *out,
                      const cn_rollout_noise *noise, float *mask, int32_t *num_launches)
{
    if (num_launches) *num_launches = 0;
    if (!g) return set_err(CN_EINVAL, "null engine");
    if (!mask) return set_err(CN_EINVAL, "cn_rollout_masked: mask required");
    if (noise && !(noise->sigma >= 0.0f && noise->sigma <= 3.402823466e38f))   // (NaN fails both comparisons)
        return set_err(CN_EINVAL, "cn_rollout_masked: noise with a finite sigma >= 0 required");
    const bool noisy = noise && noise->sigma > 0.0f;
    const int rc = rollout_run(g, stream, policy, T, out, noisy ? noise : nullptr, num_launches, nullptr, mask);
    if (rc || noisy || !noise || !noise->executed || T == 0) return rc;
    return executed_copy(g, stream, T, out, noise, num_launches);   // sigma == 0: cn_rollout_noisy's copy
}

int cn_debug_disc_quad(void *stream, int64_t n, int mode, const double *px, const double *py, const double *r,
                       const double *qx, const double *qy, int32_t *out)
{
    if (n <= 0 || !px || !py || !r || !qx || !qy || !out) return set_err(CN_EINVAL, "cn_debug_disc_quad: n > 0 and buffers required");
    HIPCHK(circ_table_init());
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_disc_quad_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, mode,
                       px, py, r, qx, qy, out);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

int cn_debug_copy64(void *stream, int64_t n, int seg, const double *src, double *dst)
{
    if (n <= 0 || seg < 1 || seg > 64 || !src || !dst) return set_err(CN_EINVAL, "cn_debug_copy64: n > 0, 1 <= seg <= 64");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_copy64_kernel, dim3((unsigned)((n + seg - 1) / seg)), dim3(64), 0, (hipStream_t)stream, n, seg,
                       src, dst);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

int cn_debug_orca(void *stream, int64_t n, int A, const float *agents, const float *self, float neighbor_dist,
                  float time_horizon, float time_step, float *out)
{
    if (n <= 0 || !agents || !self || !out) return set_err(CN_EINVAL, "cn_debug_orca: n > 0 and buffers required");
    if (A < 1 || A > 10) return set_err(CN_EUNSUPPORTED, "cn_debug_orca: 1 <= A <= 10 (the quad path)");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_orca_kernel, dim3((unsigned)((n + 15) / 16)), dim3(64), 0, (hipStream_t)stream, n, A,
                       agents, self, neighbor_dist, time_horizon, time_step, out);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

int cn_orca_predict_kd(void *stream, int64_t n, int A, const float *agents, const float *self, float neighbor_dist,
                       float time_horizon, float time_step, uint8_t *perm, float *out)
{
    if (n <= 0 || !agents || !self || !out) return set_err(CN_EINVAL, "cn_orca_predict_kd: n > 0 and buffers required");
    if (A < 1 || A > CN_ORCA_MAXA) return set_err(CN_EUNSUPPORTED, "cn_orca_predict_kd: 1 <= A <= 64");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_orca_kd_kernel, dim3((unsigned)((n + 15) / 16)), dim3(64), orca_kd_lds(A), (hipStream_t)stream,
                       n, A, agents, self, neighbor_dist, time_horizon, time_step, perm, out);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

int cn_orca_predict(void *stream, int64_t n, int A, const float *agents, const float *self, float neighbor_dist,
                    float time_horizon, float time_step, float *out)
{
    if (A > 10)   // a fresh simulator per call: identity KdTree order
        return cn_orca_predict_kd(stream, n, A, agents, self, neighbor_dist, time_horizon, time_step, nullptr, out);
    return cn_debug_orca(stream, n, A, agents, self, neighbor_dist, time_horizon, time_step, out);
}

int cn_social_force_predict(void *stream, int64_t n, int M, const double *self, const double *others, double A,
                            double B, double KI, double time_step, double *out)
{
    if (n <= 0 || M < 0 || M > 64 || !self || (M && !others) || !out)
        return set_err(CN_EINVAL, "cn_social_force_predict: n > 0, 0 <= M <= 64 and buffers required");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_sf_predict_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, M,
                       self, others, A, B, KI, time_step, out);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

int cn_dwa_predict(void *stream, int64_t n, int M, const double *self, const double *v, const double *others,
                   double time_step, const cn_dwa_params *p, float *actions, int32_t *choice, double *costs)
{
    if (n <= 0 || n >= (1LL << 31) || M < 0 || M > 64 || !self || !v || (M && !others) || !actions)
        return set_err(CN_EINVAL, "cn_dwa_predict: 0 < n < 2^31, 0 <= M <= 64 and buffers required");
    if (!dwa_params_ok(p) || !(time_step > 0) || !isfinite(time_step))
        return set_err(CN_EINVAL, "cn_dwa_predict: horizon in [1, 16], d_safe > 0, finite weights and time_step > 0 required");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_dwa_predict_kernel, dim3((unsigned)((n + CN_DWA_WAVES - 1) / CN_DWA_WAVES)),
                       dim3(64 * CN_DWA_WAVES), 0, (hipStream_t)stream, n, M, self, v, others, time_step, *p, actions,
                       choice, costs);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

int cn_edge_features(void *stream, int64_t E, int N, const float *robot_node, const float *temporal_edges,
                     const float *spatial_edges, const float *Wt, const float *bt, const float *Ws, const float *bs,
                     const float *Wr, const float *br, const float *Wn, const float *bn, float *temporal_embed,
                     float *spatial_embed, float *node_embed)
{
    if (E <= 0 || N <= 0) return set_err(CN_EINVAL, "E, N must be > 0");
    const int64_t threads = E * (N + 2) * 16;
    const int64_t blocks = (threads + 255) / 256;
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_edge_features_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, E, N,
                       robot_node, temporal_edges, spatial_edges, Wt, bt, Ws, bs, Wr, br, Wn, bn, temporal_embed,
                       spatial_embed, node_embed);
    HIPCHK(hipGetLastError());
    return CN_OK;
}

}  // extern "C"
