// cn_engine.hip — MI355X (gfx950) batched CrowdSimDict engine: kernels + C ABI (include/crowdnav.h).
//
// Hot path: ONE kernel launch per cn_step (no host synchronisation, no second kernel):
//   cn_step_kernel, step workgroups: one lane per (env, human), 256-lane workgroups holding
//       floor(256/N) whole envs. Phases 0-4: SRNN.clip_action, the human policies (ORCA LP / social
//       force) on the PRE-move state, calc_reward, kinematics, observation, Monitor. Phase 5: the
//       workgroup's own RNG work, one wave per env needing it — goal changes (numpy-legacy MT19937 in
//       LDS) and the VecEnv auto-reset, which copies a spawn drawn ahead of time.
//   cn_step_kernel, spare workgroups: spawn waves. CrowdSimDict.reset is a pure function of the seed
//       schedule, so each env's NEXT episode is drawn (reseed + spawn with rejection) by these spare
//       workgroups right after its reset, concurrently with the step. On the kd-tree path they come
//       first in the grid so that they are dispatched first: a crowded spawn (25 humans in
//       square_crossing) runs ~1M cycles, longer than the step workgroups' rounds, and started last it
//       would add its whole latency to the launch. On the quad path (cheap spawns) they come last, so
//       the step workgroups start without waiting for their dispatch.
//   cn_reset_kernel: cn_reset (every env), one wave per env.
// Reference: crowd_sim/envs/crowd_sim_dict.py:105-271, crowd_sim/envs/crowd_sim.py:296-1161,
// crowd_sim/envs/utils/agent.py:172-218, crowd_nav/policy/{orca,social_force,srnn}.py; RVO2 v2.0
// (third-party) restated in float32. Numerics: see cn_math.h.
// This file holds wsync, CN_BLK and the two kernels, cn_step_kernel (with StepArgs) and cn_reset_kernel; everything
// they call is a section of this one translation unit in engine/*.h: the device core by topic (the table of sections
// below), then the stand-alone kernels and the host side (struct cn_engine, the C ABI), included at the end.
#include <hip/hip_runtime.h>
#include <vector>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/crowdnav.h"
#include "../../include/crowdnav_state.h"
#include "cn_math.h"

using namespace cn;

// LDS ordering among the lanes of ONE wave (kernel B workgroups are a single wave; the spawn waves of
// kernel A run independently of the other waves of their workgroup): no s_barrier needed, only the
// compiler/LDS ordering a release/acquire pair at wavefront scope gives.
__device__ __forceinline__ void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#define CN_BLK 256

// ------------------------------------------------------------------------------------------------
// The device core, by topic, in dependency order: sections of this one translation unit. The kernels follow.
// ------------------------------------------------------------------------------------------------
#include "engine/stamps.h"         // -DCN_STAMPS timeline instrumentation: stamp arrays, STAMP_* (no-ops when shipped)
#include "engine/plan.h"           // tunables, StepPlan / cn_step_plan, cn_goal_early_ok, the LDS views SL, RF / HF
#include "engine/quad.h"           // DPP quad helpers: quad_xor*, quad_min / max / or, qbc*
#include "engine/geometry.h"       // FOV, velocity rectangles, world box, norm zones, disc-quad SAT
#include "engine/orca_lp.h"        // RVO2's linear programs (LDS and register forms), orca_line, orca_lines_quad
#include "engine/rng.h"            // MT19937 ring / Philox stream: mt_gen_wave*, mt_dbl*, WRng
#include "engine/spawn.h"          // pending slots, spawn_env, reset_env, goal changes, the spawning waves (pend_waves)
#include "engine/robot.h"          // scripted robot controllers, rollout noise and rows, visible masks

// ------------------------------------------------------------------------------------------------
// kernel A
// ------------------------------------------------------------------------------------------------
struct StepArgs {
    cn_state_ptrs s;
    const float *actions;
    float *robot_node, *temporal, *spatial;
    float *reward;
    uint8_t *done;
    int8_t *event;
    float *info;
    double *ep_return;
    int32_t *ep_len;
    // graph mode (cn_set_graph_mode, the DEVSEQ kernels): the launch's position in the step sequence lives on the device (ctl =
    // the engine's work_count words: [CN_CTL_NSTEP] launches so far, [CN_CTL_ALL] draw every env's next
    // spawn, [CN_CTL_DONE] finished workgroups; the last workgroup of a launch advances them), so a launch
    // has no per-call arguments and a sequence of cn_step calls can be captured in a hipGraph and replayed;
    // the pointers below are then derived at the top of the kernel. Otherwise the host passes them.
    // Multi-step launches (the SEQ kernels, cn_step_seq; never in graph mode) keep their two arguments where the
    // struct has room, so that its size and every other member's place in the kernarg segment stay what the
    // single-step kernels were tuned with: the stride shares ctl's slot, nsteps fills the padding behind E.
    union {
        uint32_t *ctl;
        int64_t action_stride;   // SEQ: step t takes the actions at actions + t * action_stride
        // ROBOT (cn_rollout's launches; their action stride is always 2 * E): CN_ROBOT_* | cn_rollout_out::flags << 8;
        // cn_rollout_noisy's: | CN_ROLLOUT_NOISY | (uint32)k of the launch's first step << CN_ROLLOUT_K_SHIFT
        int64_t rollout;
    };
    uint32_t *plist_base;  // [3][E + 64][4] spawn lists: {env, reset_count, case_counter lo, hi} after the reset
    union {
        uint32_t *rlist_base;   // [3][2E + 64][4] parked-spawn lists (read by the DEVSEQ kernels only)
        // MASK (cn_rollout_masked's launches, never graph mode's): row 0 of the launch in the caller's mask buffer,
        // [nsteps][ER][NS] with CN_ROLLOUT_OBS_EVERY_STEP, one row [ER][NS] otherwise. In the kernarg segment and
        // not in a device block as RolloutRows is: the call then issues exactly cn_rollout's launches.
        float *mask;
    };
    uint32_t *plist_w;     // envs reset by this launch (their next spawn is drawn by the next launch); a multi-step
                            // launch keeps one entry per env and slot parity, the first E of them
    uint32_t *pcount_w;
    uint32_t *pcount_zero;  // the counter the NEXT launch appends to (triple-buffered), zeroed here
    uint32_t *rcount_zero;  // likewise for the parked-spawn list
    PendLaunch pend;        // spawn waves: the first or the last pend_blocks workgroups (pend.first)
    int64_t case_size;
    int E;
    int nsteps;             // SEQ: steps a step workgroup runs in this launch
    OutView ov;             // output rows / human stride (mixed engines); also pend.ov
    double cth_h, cth_r;    // cos(human_fov / 2), cos(robot_fov / 2): in_fov's thresholds
};
static_assert(sizeof(StepArgs) == 720, "StepArgs: the kernarg layout of the single-step kernels");

// phase 5 reads cn_config from the kernarg segment right after StepArgs (cn_step_kernel's RNG loop): the
// by-value arguments are laid out in order at their natural alignment (AMDHSA metadata: 0 / 720 today)
static_assert(alignof(StepArgs) >= alignof(cn_config) || sizeof(StepArgs) % alignof(cn_config) == 0,
              "cn_step_kernel's kernarg layout: cn_config follows StepArgs");

// observed agent of slot k seen by lane (human i of env base eb): position/velocity float32,
// frozen RVO2 radius; `vis` = visible now, `dm` = dummy at simulator creation
__device__ inline void slot_agent(const SL &sl, const cn_config &c, int eb, int el, int EPB, int N, int i, int k,
                                  uint32_t vis, uint32_t dm, float rdummy, float &x, float &y, float &vx, float &vy,
                                  float &r)
{
    const bool v = (vis >> k) & 1u;
    if (k < N - 1) {
        const int j = eb + (k < i ? k : k + 1);
        if (v) {
            x = (float)HF(sl, H_PX, j); y = (float)HF(sl, H_PY, j);
            vx = (float)HF(sl, H_VX, j); vy = (float)HF(sl, H_VY, j);
        } else { x = (float)CN_DUMMY_POS; y = (float)CN_DUMMY_POS; vx = 0.0f; vy = 0.0f; }
        r = ((dm >> k) & 1u) ? rdummy : sl.orad[j];
    } else {  // robot slot (robot.visible)
        if (v) {
            x = (float)RF(sl, R_PX, el, EPB); y = (float)RF(sl, R_PY, el, EPB);
            vx = (float)RF(sl, R_VX, el, EPB); vy = (float)RF(sl, R_VY, el, EPB);
        } else { x = (float)CN_DUMMY_POS; y = (float)CN_DUMMY_POS; vx = 0.0f; vy = 0.0f; }
        r = ((dm >> k) & 1u) ? (float)(c.robot_radius + 0.01 + c.orca_safety_space)
                             : (float)(RF(sl, R_RAD, el, EPB) + 0.01 + c.orca_safety_space);
    }
}

__device__ inline float bbox_dist(float x, float y, float mnx, float mxx, float mny, float mxy)
{
    const float a = (0.0f < mnx - x) ? mnx - x : 0.0f, b = (0.0f < x - mxx) ? x - mxx : 0.0f;
    const float cc = (0.0f < mny - y) ? mny - y : 0.0f, d = (0.0f < y - mxy) ? y - mxy : 0.0f;
    return a * a + b * b + cc * cc + d * d;
}

// KD: RVO2 kd-tree neighbour order (> 10 agents per simulator); PHX: c.rng_mode == CN_RNG_PHILOX, a
// template argument so that the MT19937 build carries no Philox registers
// MIX: a group of a mixed engine (outputs through g.ov); a plain engine's identity view is then a
// compile-time constant and costs no registers
// DEVSEQ: graph mode (StepArgs::devseq), a variant of its own so the default launches carry none of it
// SEQ: a multi-step launch (cn_step_seq's chunks): the step workgroups run g.nsteps steps of their own envs
// back to back (phases 0-5 in a loop, a workgroup barrier between steps), the spare workgroups draw spawns once
// per launch as ever. Envs are independent and belong to one workgroup for the whole launch, so no workgroup
// waits for another one: a slow step (a random-goal rejection, a reset next to goal changes on one wave) delays
// its own workgroup only, and over a chunk the workgroups' totals even out. Every step reads the state the
// previous one wrote through global memory (written by other waves of the same workgroup: visible after the
// barrier) and re-initialises every LDS word and register it uses, exactly as a launch of its own would.
// ROBOT: a launch of cn_rollout (a SEQ launch of 1..seq_chunk steps): before phase 0 of every step wave 0 computes
// the scripted robot's actions of the workgroup's envs from the state the previous step (or launch) left in global
// memory, with cn_robot_act's device functions (ORCA's quad path: one quad per env, EPB <= 16 envs; social force: one
// lane per env), stores them to row `step` of g.actions and hands them to phase 0 through LDS. Every step records
// its outputs at row `step` of [nsteps][E][..] buffers (the observation only with CN_ROLLOUT_OBS_EVERY_STEP;
// otherwise the launch's last step stores it to a single row, as the SEQ kernels do). A launch of cn_rollout_noisy
// (CN_ROLLOUT_NOISY in g.rollout, wave-uniform) perturbs the action on its way into LDS (rollout_noise, parameters
// from the engine's RolloutNoise block): row `step` of g.actions keeps the clean one, `executed` gets the perturbed.
// REC (ROBOT only): a launch of cn_rollout_lidar, which also records the state every step leaves (the twelve fields
// of the engine's RolloutRows block). While wave 0 runs the controller of step s >= 1, waves 1-3 copy the state
// step s - 1 left in global memory to its row; the launch's last step copies its own after its closing barrier.
// (The state before a launch's step 0 is the previous launch's last row.) A flag of its own, so that cn_rollout's
// kernels stay what they were.
// MASK (ROBOT only, never with REC): a launch of cn_rollout_masked, which also records which humans the robot sees in
// the state every step leaves (cn_visible_mask's row, visible_mask_slot) at row `step` of g.mask, in REC's places:
// waves 1-3 write row s - 1 while wave 0 runs the controller of step s >= 1, one lane per (env of the workgroup,
// slot), and the launch's last step writes its own after its closing barrier. Without CN_ROLLOUT_OBS_EVERY_STEP only
// that last row is written, to the single row. The mask lanes read no other lane and sit behind launch-uniform
// conditions. A flag of its own again, so that cn_rollout's kernels stay what they were.
template <bool KD, bool PHX, bool MIX, bool DEVSEQ = false, bool SEQ = false, bool ROBOT = false, bool REC = false,
          bool MASK = false>
__global__ void __launch_bounds__(CN_BLK, 3) cn_step_kernel(StepArgs g, cn_config c)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const OutView ov = MIX ? g.ov : OutView{nullptr, c.human_num};
    // the goal changes beside the state stores: multi-step launches of plain quad-path engines run the goal changes of
    // the envs that go on with their episode on waves 2 and 3 from phase 2's closing barrier on, beside the state
    // stores of waves 0 and 1, and phase 5 serves the resets alone (the A/B of DESIGN.md §4). These instantiations
    // alone, the others compile as without it
    constexpr bool GOAL_EARLY = SEQ && !ROBOT && !KD && !MIX;
    // linearProgram2 as a walk (lp2_r, orca_lp.h): the same instantiations, the ones its A/B measured
    constexpr bool LP2W = SEQ && !ROBOT && !KD && !MIX;
    // this launch's spawn / parked-spawn lists (triple-buffered: launch t appends to t % 3, reads (t - 1) % 3,
    // zeroes (t + 1) % 3) and id, from the device-side step counter
    const uint32_t ns = DEVSEQ ? g.ctl[CN_CTL_NSTEP] : 0u;
    if (DEVSEQ) {
        const int64_t kw = ns % 3u, kr = (ns + 2u) % 3u, kz = (ns + 1u) % 3u;
        const int64_t ls = 4 * ((int64_t)g.E + 64), rs = 4 * (2 * (int64_t)g.E + 64);
        g.plist_w = g.plist_base + kw * ls;
        g.pcount_w = g.ctl + 2 + kw;
        g.pcount_zero = g.ctl + 2 + kz;
        g.rcount_zero = g.ctl + 5 + kz;
        g.pend.list = g.plist_base + kr * ls;
        g.pend.count = g.ctl + 2 + kr;
        g.pend.rlist = g.rlist_base + kr * rs;
        g.pend.rcount = g.ctl + 5 + kr;
        g.pend.rlist_w = g.rlist_base + kw * rs;
        g.pend.rcount_w = g.ctl + 5 + kw;
        g.pend.launch_id = ((ns + 1u) % 0x7ffffffeu) + 1u;   // nonzero, differs from the neighbours'
        g.pend.all = (int)g.ctl[CN_CTL_ALL];
    }
    // the last workgroup to finish advances the sequence (every workgroup has read it by then)
    // (the atomic carries a register dependency on this workgroup's read of the counter, so the read has
    // completed before the count can reach the grid size)
    STAMP_R(0);
    auto finish = [&]() {
#ifdef CN_STAMPS
        __syncthreads();
        STAMP_R(1);
#endif
        if (!DEVSEQ) return;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t dep;
            asm volatile("v_mov_b32 %0, 0" : "=v"(dep) : "v"(ns));
            if (atomicAdd(g.ctl + CN_CTL_DONE, 1u + dep) == gridDim.x - 1) {
                g.ctl[CN_CTL_DONE] = 0u;
                g.ctl[CN_CTL_ALL] = 0u;
                g.ctl[CN_CTL_NSTEP] = ns + 1u;
            }
        }
    };
    // the spawn-list counter the NEXT launch appends to (neither read nor appended to by this launch)
    if (blockIdx.x == 0 && threadIdx.x == 0) { *g.pcount_zero = 0u; *g.rcount_zero = 0u; }
    const int sb = (int)blockIdx.x - (g.pend.first ? g.pend.pend_blocks : 0);   // step workgroup index
    if (sb < 0 || sb >= g.pend.step_blocks) {  // spare workgroups: draw upcoming episodes' spawns
        PendLaunch pl = g.pend;
        pl.ov = ov;
        pend_waves<PHX, KD, SEQ>(pl, g.s, c, g.E, smem);
        finish();
        return;
    }
    const int N = c.human_num;
    const StepPlan P = cn_step_plan(N, c.robot_visible);
    const int EPB = P.EPB, M = P.M, A = P.A;
    SL sl;
    sl.T = P.H;
    sl.r = (double *)(smem + P.o_renv);
    sl.act = (float *)(smem + P.o_racts);
    sl.rflag = (uint32_t *)(smem + P.o_rflag);
    sl.app = (uint32_t *)(smem + P.o_app);
    sl.rvr = (double *)(smem + P.o_rvr);
    sl.hvr = (double *)(smem + P.o_hvr);
    sl.hst = (double *)(smem + P.o_hst);
    sl.h = (double *)(smem + P.o_hum);
    sl.cd = (double *)(smem + P.o_lane);
    sl.lf = (uint32_t *)(smem + P.o_lane + P.H * 8);
    sl.orad = (float *)(smem + P.o_orad);
    sl.vis = (uint32_t *)(smem + P.o_vis);
    sl.dm = sl.vis + P.H;
    sl.vmax = (float *)(sl.vis + 2 * P.H);
    sl.npx = (double *)(smem + P.o_nv);
    sl.npy = sl.npx + P.H;
    sl.eg = (uint32_t *)(smem + P.o_eg);
    sl.lines = (float4 *)(smem + P.o_lines);
    sl.proj = (float4 *)(smem + P.o_proj);
    sl.nd = (float *)(smem + P.o_nd);
    sl.ns = (uint8_t *)(smem + P.o_ns);
    sl.perm = (uint8_t *)(smem + P.o_perm);
    const cn_state_ptrs &S = g.s;
    // human hh's velocity-rectangle corner k (x0..x3, y0..y3) and human_post's staged value f: [8][H] / [7][H]
    // arrays on the quad path, the human's own projected-line block on the kd-tree path (StepPlan)
    auto hvr_ref = [&](int hh, int k) -> double & {
        return KD ? ((double *)(sl.proj + hh * M))[k] : sl.hvr[k * 64 + hh];
    };
    auto hst_ref = [&](int hh, int f) -> double & {
        return KD ? ((double *)(sl.proj + hh * M))[f] : sl.hst[f * 64 + hh];
    };

    // SEQ: the spawn-list entry (index + 1; 0: none yet) this launch holds for each env and key parity (phase 5)
    if constexpr (SEQ) { if ((int)threadIdx.x < 2 * EPB) sl.app[threadIdx.x] = 0u; }
    int step = 0;
    do {   // one pass without SEQ: the condition folds and the single-step kernels compile as without the loop
           // (the body keeps the single step's indentation)
    int tid = threadIdx.x, sbk = sb;
    // SEQ: the lane and workgroup indices are opaque in every step, so that nothing derived from them (the ~40
    // per-lane state addresses above all) is step-invariant: hoisted out of the loop they stayed live across
    // the whole step (292 VGPRs spilled to scratch); now every step computes them at their uses, as a launch of
    // its own does
    if constexpr (SEQ) { asm volatile("" : "+v"(tid)); asm volatile("" : "+s"(sbk)); }
    // SEQ: the issue priority of the workgroup's waves rotates with the step. A CU's resident workgroups sit in
    // wave slots 0, 1, 2 of its SIMDs in the order they arrived (HW_REG_HW_ID's wave id), and at equal priority
    // the SIMD issues its oldest wave first: the first workgroup of a CU ran 32 steps in ~790 us, the second in
    // ~860, the third in ~940, launch after launch, and the launch ends with the third ("Where the
    // persistent groups come from"). With priority (slot + step) % 3 every workgroup spends a third of its steps
    // at each rank. For speed only: results do not depend on it.
    if constexpr (SEQ) {
        const unsigned ws = (unsigned)__builtin_amdgcn_s_getreg(4 | (3 << 11));   // HW_ID bits 3:0: the wave slot
        switch ((ws + (unsigned)step) % 3u) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        default: __builtin_amdgcn_s_setprio(2); break;
        }
    }
    // XCD-aware env placement: workgroup i runs on XCD i % 8 (round-robin dispatch; for speed only), so
    // give each XCD a contiguous run of env blocks. Neighbouring workgroups share the 128-B lines at the
    // ends of their SoA segments (a per-env field of one workgroup is only 48 B); on one XCD the second
    // reader hits in that XCD's L2 instead of fetching the line again.
    // (a leading pend_blocks is a multiple of 8, so step workgroup sb runs on XCD sb % 8 as well)
    const int nbk = g.pend.step_blocks, xq = nbk >> 3, xr = nbk & 7, xi = sbk & 7;
#if CN_LABEL_ROT
    // diagnostic (-DCN_STAMPS -DCN_LABEL_ROT=r, tools/probe_stamps.py xcd): the labels' runs of env blocks in the
    // order of (label + r) & 7, so that a slowness bound to the label can be told from one bound to the env range
    int blk = sbk >> 3;
    for (int y = 0; y < 8; ++y)
        if (((y + CN_LABEL_ROT) & 7) < ((xi + CN_LABEL_ROT) & 7)) blk += xq + (y < xr ? 1 : 0);
#else
    const int blk = xi * xq + min(xi, xr) + (sbk >> 3);
#endif
    const int e0 = blk * EPB;
    const int nenv_here = min(EPB, g.E - e0);
    const int el = tid / N, i = tid - el * N;
    const bool hl = el < nenv_here;               // human lane
    const int gh = (e0 + el) * N + i;                 // global human index (E*N < 2^31, cn_config_validate)
    // env lanes (robot / reward / bookkeeping): wave 1 on the quad path, so they run beside the human
    // lanes of wave 0 in phases 0, 3 and 4; the first lanes on the kd-tree path
    const int re = tid - 64;
    const bool rl = re >= 0 && re < nenv_here;
    const int ge = e0 + re;
    const bool holo = c.kinematics == CN_HOLONOMIC;
    const double dt = c.time_step;

    const float *actions = g.actions;
    // rows of one step in the caller's (T, E, ..) buffers: a group of a mixed engine records into the mixed engine's
    const int64_t erow = (MIX && ROBOT) ? (int64_t)((const int32_t *)g.pend.stats)[CN_ER_W - 8] : (int64_t)g.E;
    if constexpr (ROBOT) actions += (int64_t)step * (2 * erow);
    else if constexpr (SEQ) actions += (int64_t)step * g.action_stride;
    // SEQ: the caller reads the outputs of the launch's last step only (every step would overwrite them), so the
    // earlier steps neither convert nor store them (wave-uniform; state writes are not outputs and stay; the A/B
    // against storing in every step is in DESIGN.md §4)
    // ROBOT: every step's outputs are recorded, at row `step` (orw_e: its first env row; orw_o: the observation's,
    // row 0 of a single-row buffer without CN_ROLLOUT_OBS_EVERY_STEP, which then holds the last step's as above)
    const bool emit = !SEQ || ROBOT || step == g.nsteps - 1;
    const bool obs_rows = ROBOT && ((g.rollout >> 8) & CN_ROLLOUT_OBS_EVERY_STEP) != 0;
    const bool emit_obs = ROBOT ? (obs_rows || step == g.nsteps - 1) : emit;
    // SEQ (not ROBOT, which records every step): the values only the info row reads -- the velocity rectangles and
    // their intersection test (LF_VR), LF_NOTREACHED, R_JERK / R_SPD / R_SL / R_SR / R_SEP -- are computed in the step
    // that stores the row (wave-uniform; folds to true as emit does; the A/B of DESIGN.md §4). Everything the reward,
    // done or the state depend on (sl.cd, the collision index, LF_ENDGOAL, the NaN bit, R_D2G, R_BITS, last_ax /
    // last_ay) stays.
    const bool info_on = (SEQ && !ROBOT) ? emit : true;
    const int64_t orw_e = ROBOT ? (int64_t)step * erow : 0;
    const int64_t orw_o = obs_rows ? orw_e : 0;
    if constexpr (ROBOT) {
        // ---- the scripted robot: wave 0, from the global state (this workgroup's own envs; its previous step's
        // stores, an auto-reset's included, are visible after that step's closing barrier). The ORCA lines lie over
        // the step's ORCA scratch (16 envs x 9 float4 = 2304 B at o_lines, idle until phase 2 and smaller than one
        // RNG region, so SL::app behind the plan is out of reach). A quad is whole or absent (q < nenv_here).
        // On a unicycle engine (cn_scripted_unicycle) robot_unicycle_track reads r_theta and r_dv the same way: every
        // step stores both at its end, and an inline reset's come before the same barrier.
        if ((tid >> 6) == 0) {
            float *const arow = const_cast<float *>(actions);
            // cn_rollout_noisy's launches (wave-uniform): the step takes the perturbed action, the `actions` row keeps
            // the clean one, the `executed` row (same place in its buffer) gets the perturbed one
            const bool noisy = (g.rollout & CN_ROLLOUT_NOISY) != 0;
            RolloutNoise nz = {0.0f, 0u, nullptr, nullptr};
            if (noisy) nz = *(const RolloutNoise *)(g.pend.stats + (CN_NOISE_W - 8));
            const uint32_t nk = (uint32_t)(g.rollout >> CN_ROLLOUT_K_SHIFT) + (uint32_t)step;
            float *const xrow = nz.executed ? nz.executed + (arow - nz.actions) : nullptr;
            if ((int)(g.rollout & 0xff) == CN_ROBOT_SOCIAL_FORCE) {
                if (tid < nenv_here) {
                    double nx, ny, nn, vpref;   // (the clip and the rounding of cn_robot_sf_kernel)
                    robot_sf_velocity(S, e0 + tid, N, c.sf_A, c.sf_B, c.sf_KI, c.time_step, nx, ny, nn, vpref);
                    float ax, ay;
                    if (nn > vpref) { ax = (float)(ddiv(nx, nn) * vpref); ay = (float)(ddiv(ny, nn) * vpref); }
                    else { ax = (float)nx; ay = (float)ny; }
                    if (!holo) robot_unicycle_track(S, e0 + tid, ax, ay, ax, ay);   // (launch-uniform)
                    const int64_t oa = orow(ov, e0 + tid);   // the env's row in the caller's buffers (and noise key)
                    arow[2 * oa] = ax; arow[2 * oa + 1] = ay;
                    if (noisy) {
                        rollout_noise(nz.sigma, nz.seed, nk, (uint32_t)(c.env_offset + oa), ax, ay, ax, ay);
                        if (xrow) { xrow[2 * oa] = ax; xrow[2 * oa + 1] = ay; }
                    }
                    sl.act[tid] = ax; sl.act[EPB + tid] = ay;
                }
            } else {
                const int q = tid >> 2, sq = tid & 3;
                const bool act = q < nenv_here;
                const int64_t e = e0 + q;
                float4 *const Lq = sl.lines + q * 9;
                int cnt = 0;
                if (act)
                    cnt = robot_orca_lines(S, c.orca_safety_space, e, N, sq, (float)c.orca_neighbor_dist,
                                           (float)c.orca_time_horizon, (float)c.time_step, Lq);
                wsync();
                if (act) {
                    float rx, ry;
                    robot_orca_solve(S, e, cnt, sq, Lq, rx, ry);
                    if (sq == 0) {
                        // a unicycle engine (launch-uniform): the quad's lane 0 alone turns the velocity into the
                        // step's (dv, dtheta); no lane reads another's registers here
                        if (!holo) robot_unicycle_track(S, e, rx, ry, rx, ry);
                        const int64_t oa = orow(ov, e);   // (addresses only: the quad's lanes and flow are as ever)
                        arow[2 * oa] = rx; arow[2 * oa + 1] = ry;
                        if (noisy) {
                            rollout_noise(nz.sigma, nz.seed, nk, (uint32_t)(c.env_offset + oa), rx, ry, rx, ry);
                            if (xrow) { xrow[2 * oa] = rx; xrow[2 * oa + 1] = ry; }
                        }
                        sl.act[q] = rx; sl.act[EPB + q] = ry;
                    }
                }
            }
        } else if constexpr (REC) {
            if (step > 0) {   // (actions - rr.actions = row * 2 E: the row's first env without a division)
                const RolloutRows rr = *(const RolloutRows *)(g.pend.stats + (CN_ROWS_W - 8));
                state_rows_copy(S, rr, g.E, N, (actions - rr.actions) / 2 - g.E, e0, nenv_here, tid - 64, CN_BLK - 64);
            }
        } else if constexpr (MASK) {
            if (step > 0 && obs_rows)   // the mask of the state step - 1 left, into its row
                visible_mask_rows(S, ov, e0, nenv_here, N, holo ? 1 : 0, c.robot_fov, g.cth_r,
                                  g.mask + (orw_e - erow) * ov.NS, tid - 64, CN_BLK - 64);
        }
        __syncthreads();
    }
    STAMP_A(0);
    // ---- phase 0: load state into LDS -----------------------------------------------------------
    // values needed in later phases are loaded here, so their latency overlaps phase 0 (doubles parked
    // in LDS rather than registers across the ORCA phase)
    float pre_or = 0.0f, pre_vmax = 0.0f;
    uint32_t pre_dm = 0u;
    int32_t pre_epl = 0, pre_sc = 0;
    uint32_t pre_ovf = 0;
    // With a 360-degree robot FOV every human the robot can see is visible (only coincident agents are
    // not), so the previous belief is read only in that rare case, straight from the state in phase 4
    const bool rfull = c.robot_fov >= 2.0 * CN_PI;
    if (hl) {
        // every load issued before the first LDS store (the compiler otherwise waits on each load in turn)
        double hv[CN_HUM_F];
        pre_or = S.o_r[gh]; pre_vmax = S.o_vmax[gh]; pre_dm = S.o_dmask[gh];
        hv[H_PX] = S.h_px[gh]; hv[H_PY] = S.h_py[gh]; hv[H_GX] = S.h_gx[gh]; hv[H_GY] = S.h_gy[gh];
        hv[H_VX] = S.h_vx[gh]; hv[H_VY] = S.h_vy[gh]; hv[H_R] = S.h_r[gh]; hv[H_VP] = S.h_vpref[gh];
        hv[H_TH] = S.h_theta[gh];
        if (!rfull) {
            hv[H_BPX] = S.b_px[gh]; hv[H_BPY] = S.b_py[gh]; hv[H_BVX] = S.b_vx[gh]; hv[H_BVY] = S.b_vy[gh];
            hv[H_BR] = S.b_r[gh];
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int f = 0; f < H_BPX; ++f) HF(sl, f, tid) = hv[f];
        if (!rfull) {
#pragma unroll
            for (int f = H_BPX; f < CN_HUM_F; ++f) HF(sl, f, tid) = hv[f];
        }
    }
    STAMP_A(12);
    if (rl) {
        double rv[CN_RENV_F];
        rv[R_PX] = S.r_px[ge]; rv[R_PY] = S.r_py[ge]; rv[R_GX] = S.r_gx[ge]; rv[R_GY] = S.r_gy[ge];
        rv[R_VX] = S.r_vx[ge]; rv[R_VY] = S.r_vy[ge]; rv[R_TH] = S.r_theta[ge]; rv[R_RAD] = S.r_radius[ge];
        rv[R_VP] = S.r_vpref[ge]; rv[R_POT] = S.potential[ge]; rv[R_GT] = S.gtime[ge]; rv[R_DV] = S.r_dv[ge];
        rv[R_LAX] = S.last_ax[ge]; rv[R_LAY] = S.last_ay[ge]; rv[R_EPR] = S.ep_return[ge];
        const uint32_t fl = S.flags[ge];
        pre_epl = S.ep_len[ge]; pre_sc = S.scenario[ge]; pre_ovf = S.overflow[ge];
        const int64_t oa = orow(ov, ge);   // the env's row in the caller's buffers
        float a0, a1;
        if constexpr (ROBOT) { a0 = sl.act[re]; a1 = sl.act[EPB + re]; }   // (wave 0's, before the barrier above)
        else { a0 = actions[oa * 2]; a1 = actions[oa * 2 + 1]; }
        asm volatile("" ::: "memory");
        RF(sl, R_PX, re, EPB) = rv[R_PX]; RF(sl, R_PY, re, EPB) = rv[R_PY];
        RF(sl, R_GX, re, EPB) = rv[R_GX]; RF(sl, R_GY, re, EPB) = rv[R_GY];
        RF(sl, R_VX, re, EPB) = rv[R_VX]; RF(sl, R_VY, re, EPB) = rv[R_VY];
        RF(sl, R_TH, re, EPB) = rv[R_TH]; RF(sl, R_RAD, re, EPB) = rv[R_RAD];
        RF(sl, R_VP, re, EPB) = rv[R_VP]; RF(sl, R_POT, re, EPB) = rv[R_POT];
        RF(sl, R_GT, re, EPB) = rv[R_GT]; RF(sl, R_DV, re, EPB) = rv[R_DV];
        RF(sl, R_LAX, re, EPB) = rv[R_LAX]; RF(sl, R_LAY, re, EPB) = rv[R_LAY]; RF(sl, R_EPR, re, EPB) = rv[R_EPR];
        sl.rflag[re] = fl;
        STAMP_A(13);
        // ---- SRNN.clip_action (srnn.py:18-48) + unicycle integrator (crowd_sim_dict.py:211-217)
        if (holo) {
            const float n = np_norm2f(a0, a1);
            if ((double)n > RF(sl, R_VP, re, EPB)) {
                const float vp = (float)RF(sl, R_VP, re, EPB);
                a0 = fdiv(a0, n) * vp; a1 = fdiv(a1, n) * vp;
            }
        } else {
            a0 = np_clipf(a0, -0.1f, 0.1f);
            a1 = np_clipf(a1, -0.1f, 0.1f);
            const float vp = (float)RF(sl, R_VP, re, EPB);
            const float dv = np_clipf((float)RF(sl, R_DV, re, EPB) + a0, -vp, vp);
            RF(sl, R_DV, re, EPB) = dv;
            a0 = dv;
        }
        sl.act[re] = a0; sl.act[EPB + re] = a1;
        STAMP_A(10);
        STAMP_T(16, 64);
    }
    __syncthreads();
    STAMP_A(1);

    // per-human terms of calc_reward (crowd_sim.py:934-969), PRE-move, for human lane hh
    auto reward_terms = [&](int hh) {
        const int elh = hh / N;
        const double px = HF(sl, H_PX, hh), py = HF(sl, H_PY, hh);
        const double vx0 = HF(sl, H_VX, hh), vy0 = HF(sl, H_VY, hh), rad = HF(sl, H_R, hh);
        const double rdx = px - RF(sl, R_PX, elh, EPB), rdy = py - RF(sl, R_PY, elh, EPB);
        sl.cd[hh] = dsqrt(rdx * rdx + rdy * rdy) - rad - RF(sl, R_RAD, elh, EPB);
        uint32_t f = 0u;
        if (info_on) {   // the rectangle and the not-reached flag feed the info row alone
            double hcx[4], hcy[4];
            vel_rect(px, py, vx0, vy0, rad, false, hcx, hcy);
            for (int k = 0; k < 4; ++k) { hvr_ref(hh, k) = hcx[k]; hvr_ref(hh, 4 + k) = hcy[k]; }
            // (the path-violation test of this rectangle against the robot's runs in human_post, phase 2: the
            // robot's rectangle is computed beside this one, on wave 3)
            if (!(np_norm2(px - HF(sl, H_GX, hh), py - HF(sl, H_GY, hh)) < rad)) f |= LF_NOTREACHED;
        }
        sl.lf[hh] = f;
    };
    // robot VelocityRectangle (pre-move), phase 1 on wave 3
    auto robot_vr = [&](int q) {
        double cx[4], cy[4];
        vel_rect(RF(sl, R_PX, q, EPB), RF(sl, R_PY, q, EPB), RF(sl, R_VX, q, EPB), RF(sl, R_VY, q, EPB),
                 RF(sl, R_RAD, q, EPB), (sl.rflag[q] & CN_FLAG_ROBOT_F32) != 0, cx, cy);
        for (int k = 0; k < 4; ++k) { sl.rvr[k * EPB + q] = cx[k]; sl.rvr[(4 + k) * EPB + q] = cy[k]; }
    };
    // robot-only terms of calc_reward (crowd_sim.py:973-1030) and the robot's move (agent.py:172-212);
    // independent of the humans, so the quad path computes them in phase 1 on wave 2
    auto robot_terms = [&](int q) {
        const int64_t gq = e0 + q;
        const double rpx = RF(sl, R_PX, q, EPB), rpy = RF(sl, R_PY, q, EPB), rr = RF(sl, R_RAD, q, EPB);
        const double rgx = RF(sl, R_GX, q, EPB), rgy = RF(sl, R_GY, q, EPB);
        const bool rf32 = (sl.rflag[q] & CN_FLAG_ROBOT_F32) != 0;
        const float a0 = sl.act[q], a1 = sl.act[EPB + q];
        const bool reaching_goal = np_norm2(rpx - rgx, rpy - rgy) < rr;
        // commanded world-frame velocity; unicycle: theta + r is float32 (NEP 50)
        const float tr = (float)RF(sl, R_TH, q, EPB) + a1;
        const float th_new = np_modf(tr, (float)(2 * CN_PI));
        double cvx, cvy;
        if (holo) { cvx = a0; cvy = a1; }
        else { cvx = (double)(a0 * np_cosf(th_new)); cvy = (double)(a0 * np_sinf(th_new)); }
        // unicycle differential drive (agent.py:185-194)
        double upx = rpx, upy = rpy;
        if (!holo && !(fabsf(a1) < 0.0001f)) {
            const float w = fdiv(a1, (float)dt);
            const float R = fdiv(a0, w);
            const double th = RF(sl, R_TH, q, EPB);
            double t1x, t1y;
            if (rf32) { t1x = (double)(R * np_sinf((float)th)); t1y = (double)(R * np_cosf((float)th)); }
            else { t1x = (double)R * sin(th); t1y = (double)R * cos(th); }
            upx = rpx - t1x + (double)(R * np_sinf(tr));
            upy = rpy + t1y - (double)(R * np_cosf(tr));
        }
        double side_l = 0, side_r = 0, sep = 0;
        if (c.side_preference && info_on) {
            const int eb = q * N;
            double ex, ey;
            if (holo) { ex = rpx + (double)(a0 * (float)dt); ey = rpy + (double)(a1 * (float)dt); }
            else { ex = upx; ey = upy; }
            const double hy = HF(sl, H_PY, eb), hr = HF(sl, H_R, eb);
            if (ey <= hy + hr && ey >= hy - hr) { if (ex < HF(sl, H_PX, eb)) side_l = 1; else side_r = 1; }
            sep = np_norm2(HF(sl, H_PX, eb) - rpx, HF(sl, H_PY, eb) - rpy);
        }
        {   // jerk (crowd_sim.py:1002-1009), float32 like the reference's np.float32 action
            const float ax = (float)cvx - (float)RF(sl, R_VX, q, EPB), ay = (float)cvy - (float)RF(sl, R_VY, q, EPB);
            if (info_on) {
                const float dax = ax - (float)RF(sl, R_LAX, q, EPB), day = ay - (float)RF(sl, R_LAY, q, EPB);
                RF(sl, R_JERK, q, EPB) = (double)(dax * dax + day * day);
            }
            S.last_ax[gq] = ax; S.last_ay[gq] = ay;   // (state: kept every step)
        }
        RF(sl, R_D2G, q, EPB) = np_norm2(rpx - rgx, rpy - rgy);
        const bool inside = inside_world(rpx, rpy, rr, c.square_width / 2);
        if (info_on) {
            { const float fx = (float)cvx, fy = (float)cvy; RF(sl, R_SPD, q, EPB) = (double)fsqrt(fx * fx + fy * fy); }
            RF(sl, R_SL, q, EPB) = side_l; RF(sl, R_SR, q, EPB) = side_r; RF(sl, R_SEP, q, EPB) = sep;
        }
        RF(sl, R_BITS, q, EPB) = (double)((reaching_goal ? 1u : 0u) | (inside ? 2u : 0u));
        RF(sl, R_CVX, q, EPB) = cvx; RF(sl, R_CVY, q, EPB) = cvy; RF(sl, R_NTH, q, EPB) = th_new;
        if (holo) {
            RF(sl, R_NX, q, EPB) = rpx + (double)(a0 * (float)dt);
            RF(sl, R_NY, q, EPB) = rpy + (double)(a1 * (float)dt);
        } else { RF(sl, R_NX, q, EPB) = upx; RF(sl, R_NY, q, EPB) = upy; }
    };
    // ---- phase 1: visibility of the other agents to human i, frozen simulator parameters --------
    // (quad path: wave 1 computes the per-human reward terms, wave 2 the robot terms meanwhile)
    if (tid >= 64 && tid - 64 < nenv_here * N) reward_terms(tid - 64);
    STAMP_T(17, 64);
    if (tid >= 128 && tid - 128 < nenv_here) robot_terms(tid - 128);
    STAMP_T(18, 128);
    if (info_on && tid >= 192 && tid - 192 < nenv_here) robot_vr(tid - 192);
    const bool orca = c.human_policy == CN_POLICY_ORCA;
    uint32_t vis = 0, dm = 0;
    float my_vmax = 0.0f;
    bool frozen = true;
    if (hl) {
        const int eb = el * N;
        double fx = 0, fy = 0;
        bool have_dir = false;
        auto dir = [&]() {
            if (!have_dir) {
                if (holo) fov_dir64(atan2(HF(sl, H_VY, tid), HF(sl, H_VX, tid)), fx, fy);
                else fov_dir64(HF(sl, H_TH, tid), fx, fy);
                have_dir = true;
            }
        };
        const bool full = c.human_fov >= 2.0 * CN_PI;
        const bool hfin = holo ? (HF(sl, H_VX, tid) == HF(sl, H_VX, tid) && HF(sl, H_VY, tid) == HF(sl, H_VY, tid))
                               : isfinite(HF(sl, H_TH, tid));
        const double px = HF(sl, H_PX, tid), py = HF(sl, H_PY, tid);
        uint32_t undecided = 0;   // 360-degree FOV: decided without the heading except at |v|^2 extremes
        if (full) {
#pragma unroll 4
            for (int k = 0; k < N - 1; ++k) {
                const int j = eb + (k < i ? k : k + 1);
                const int v = vis360(hfin, px, py, HF(sl, H_PX, j), HF(sl, H_PY, j));
                if (v > 0) vis |= 1u << k;
                if (v < 0) undecided |= 1u << k;
            }
        } else undecided = (N - 1 >= 32) ? 0xffffffffu : ((1u << (N - 1)) - 1u);
        for (uint32_t um = undecided; um; um &= um - 1) {
            const int k = __ffs(um) - 1;
            const int j = eb + (k < i ? k : k + 1);
            dir();
            if (in_fov_fast(fx, fy, px, py, HF(sl, H_PX, j), HF(sl, H_PY, j), c.human_fov, g.cth_h)) vis |= 1u << k;
        }
        if (c.robot_visible) {
            int v = full ? vis360(hfin, px, py, RF(sl, R_PX, el, EPB), RF(sl, R_PY, el, EPB)) : -1;
            if (v < 0) {
                dir();
                v = in_fov_fast(fx, fy, px, py, RF(sl, R_PX, el, EPB), RF(sl, R_PY, el, EPB), c.human_fov, g.cth_h) ? 1 : 0;
            }
            if (v) vis |= 1u << (N - 1);
        }
        if (orca) {
            frozen = (sl.rflag[el] & CN_FLAG_ORCA_FROZEN) != 0;
            if (frozen) {
                sl.orad[tid] = pre_or;
                my_vmax = pre_vmax;
                dm = pre_dm;
            } else {  // first ORCA.predict of the episode creates the simulator (orca.py:85-109)
                sl.orad[tid] = (float)(HF(sl, H_R, tid) + 0.01 + c.orca_safety_space);
                my_vmax = (float)HF(sl, H_VP, tid);
                dm = ~vis & ((M >= 32) ? 0xffffffffu : ((1u << M) - 1u));
                S.o_r[gh] = sl.orad[tid];
                S.o_vmax[gh] = my_vmax;
                S.o_dmask[gh] = dm;
            }
        }
        sl.vis[tid] = vis; sl.dm[tid] = dm; sl.vmax[tid] = my_vmax;
    }
    STAMP_T(19, 0);
    __syncthreads();
    STAMP_A(2);

    // calc_reward ladder + Monitor (crowd_sim.py:907-1094) for env lane re: reads only phase-1 results (pre-move
    // distances / flags and the robot-only terms), so it runs inside phase 2 on the env lanes (wave 1, after
    // its own ORCA quads), in the slack while the slowest humans finish their linear programs. The robot's
    // kinematics update (which the ORCA simulators must not see yet) is applied after phase 2.
    bool ladder_done = false;   // the quad ORCA path runs it inside phase 2 (before the linearProgram3 tasks)
    auto ladder = [&]() {
        const double rr = RF(sl, R_RAD, re, EPB);
        const uint32_t flags = sl.rflag[re];
        const float a0 = sl.act[re], a1 = sl.act[EPB + re];
        const int eb = re * N;
        double dmin = INFINITY;
        bool collision = false, nz_viol = false;
        int agg = 0, kv = N;
        for (int k = 0; k < N; ++k) {
            const double cd = sl.cd[eb + k];
            if (cd < 0) { collision = true; kv = k; break; }
            else if (cd < dmin) dmin = cd;
            if (info_on) {
                const uint32_t f = sl.lf[eb + k];
                agg += (f & LF_NOTREACHED) ? 1 : 0;
            }
        }
        sl.rflag[2 * EPB + re] = (uint32_t)kv;   // the path violations of humans k < kv are counted after phase 2
        // the reference tests the norm zones inside the loop once human 0 is not a collision; the penalty
        // is read only on the no-collision branch of the ladder, where the loop ran past human 0, so
        // testing it here (outside the loop: the call's register saves only run when it is taken) is
        // the same
        if (c.norm_zones && !collision)
            nz_viol = robot_norm_zone_violation(RF(sl, R_PX, re, EPB), RF(sl, R_PY, re, EPB), RF(sl, R_VX, re, EPB),
                                                RF(sl, R_VY, re, EPB), rr, (flags & CN_FLAG_ROBOT_F32) != 0,
                                                c.norm_zone_lhs);
        const uint32_t bits = (uint32_t)RF(sl, R_BITS, re, EPB);
        const bool reaching_goal = (bits & 1u) != 0, inside = (bits & 2u) != 0;
        if (!reaching_goal) ++agg;
        const double dist_to_goal = RF(sl, R_D2G, re, EPB);
        const double gt = RF(sl, R_GT, re, EPB);
        double reward;
        int done, event;
        if (gt >= c.time_limit - 1) { reward = 0; done = 1; event = CN_EV_TIMEOUT; }
        else if (collision || !inside) { reward = c.collision_penalty; done = 1; event = CN_EV_COLLISION; }
        else if (reaching_goal) {
            reward = c.success_reward;
            if (c.time_factor) reward *= ddiv(c.time_limit - gt, c.time_limit);
            done = 1; event = CN_EV_REACHGOAL;
        } else if (dmin < c.discomfort_dist) {
            reward = (dmin - c.discomfort_dist) * c.discomfort_penalty_factor;
            done = 0; event = CN_EV_DANGER;
        } else {
            reward = c.potential_factor * (-fabs(dist_to_goal) - RF(sl, R_POT, re, EPB));
            RF(sl, R_POT, re, EPB) = -fabs(dist_to_goal);
            if (c.norm_zones && nz_viol) reward += c.norm_zone_penalty;
            done = 0; event = CN_EV_NOTHING;
        }
        if (!holo) {
            const float r_spin = -2.0f * (a1 * a1);
            const float r_back = a0 < 0 ? -2.0f * fabsf(a0) : 0.0f;
            if (event == CN_EV_DANGER || event == CN_EV_NOTHING) reward = reward + (double)r_spin + (double)r_back;
            else reward = (double)(((float)reward + r_spin) + r_back);
        }
        if (emit && g.info) {
            float *info = g.info + (orw_e + orow(ov, ge)) * CN_INFO_K;
            info[CN_INFO_AGG_NAV_TIME] = (float)agg;
            info[CN_INFO_PERSONAL_VIOLATION] = dmin < c.min_personal_space ? 1.0f : 0.0f;
            info[CN_INFO_JERK_COST] = (float)RF(sl, R_JERK, re, EPB);
            info[CN_INFO_DIST_TO_GOAL] = (float)dist_to_goal;
            info[CN_INFO_SPEED_VIOLATION] = RF(sl, R_SPD, re, EPB) > c.max_walking_speed ? 1.0f : 0.0f;
            info[CN_INFO_MIN_DIST] = (float)dmin;
            info[CN_INFO_SCENARIO] = (float)pre_sc;
            info[CN_INFO_SIDE_LEFT] = (float)RF(sl, R_SL, re, EPB);
            info[CN_INFO_SIDE_RIGHT] = (float)RF(sl, R_SR, re, EPB);
            info[CN_INFO_SEPARATION] = (float)RF(sl, R_SEP, re, EPB);
            info[CN_INFO_OVERFLOW] = (float)pre_ovf;
        }
        RF(sl, R_GT, re, EPB) = gt + dt;
        const double epr = RF(sl, R_EPR, re, EPB) + reward;
        const int32_t epl = pre_epl + 1;
        S.ep_return[ge] = epr; S.ep_len[ge] = epl;
        if (emit) {
            const int64_t oe = orw_e + orow(ov, ge);
            if (g.reward) g.reward[oe] = (float)reward;
            if (g.done) g.done[oe] = (uint8_t)done;
            if (g.event) g.event[oe] = (int8_t)event;
            if (g.ep_return) g.ep_return[oe] = epr;
            if (g.ep_len) g.ep_len[oe] = epl;
        }
        sl.rflag[EPB + re] = (uint32_t)done;   // aux word: done
    };
    // human kinematics, robot-FOV belief, observation and goal-reached detection of human hh from its new
    // velocity (agent.py:172-212 step, crowd_sim_dict.py:72-103 generate_ob): called by the lane that
    // produced the velocity as soon as it has it (ORCA: the quad's lane 0 after its linear programs)
    // path violation of human hh (crowd_sim.py:951-957): the robot's and the human's pre-move
    // VelocityRectangles intersect; quad version (4 lanes of the human's quad together) and a lane version
    auto path_vr_q = [&](int hh, int s4) -> bool {
        const int elh = hh / N;
        double rcx[4], rcy[4], hcx[4], hcy[4];
        for (int k = 0; k < 4; ++k) {
            rcx[k] = sl.rvr[k * EPB + elh]; rcy[k] = sl.rvr[(4 + k) * EPB + elh];
            hcx[k] = hvr_ref(hh, k); hcy[k] = hvr_ref(hh, 4 + k);
        }
        return quads_intersect_q(rcx, rcy, hcx, hcy, s4);
    };
    auto path_vr = [&](int hh) -> bool {
        const int elh = hh / N;
        double rcx[4], rcy[4], hcx[4], hcy[4];
        for (int k = 0; k < 4; ++k) {
            rcx[k] = sl.rvr[k * EPB + elh]; rcy[k] = sl.rvr[(4 + k) * EPB + elh];
            hcx[k] = hvr_ref(hh, k); hcy[k] = hvr_ref(hh, 4 + k);
        }
        return quads_intersect(rcx, rcy, hcx, hcy);
    };
    auto human_post = [&](int hh, double nvx, double nvy, bool vr) {
        const int elh = hh / N, ih = hh - elh * N;
        const int ghh = (e0 + elh) * N + ih;
        const double npx = HF(sl, H_PX, hh) + nvx * dt, npy = HF(sl, H_PY, hh) + nvy * dt;
        // detect_visible(robot, human, robot1=True) on the POST-move state (robot velocity now float32)
        const double rnx = RF(sl, R_NX, elh, EPB), rny = RF(sl, R_NY, elh, EPB);
        // the robot's post-move velocity / heading (agent.py:198-212, applied to the state after phase 2):
        // holonomic = the clipped action, unicycle = the commanded velocity and new heading of phase 1
        const float rvx = holo ? sl.act[elh] : (float)RF(sl, R_CVX, elh, EPB);
        const float rvy = holo ? sl.act[EPB + elh] : (float)RF(sl, R_CVY, elh, EPB);
        const float rth = holo ? 0.0f : (float)RF(sl, R_NTH, elh, EPB);
        const bool rfin = holo ? (rvx == rvx && rvy == rvy) : isfinite(rth);
        int rv = c.robot_fov >= 2.0 * CN_PI ? vis360(rfin, rnx, rny, npx, npy) : -1;
        if (rv < 0) {
            double fx, fy;
            if (holo) fov_dir32(atan2f(rvy, rvx), fx, fy);
            else fov_dir32(rth, fx, fy);
            rv = in_fov_fast(fx, fy, rnx, rny, npx, npy, c.robot_fov, g.cth_r) ? 1 : 0;
        }
        double bpx, bpy, bvx, bvy, br;
        if (rv) {
            bpx = npx; bpy = npy; bvx = nvx; bvy = nvy; br = HF(sl, H_R, hh);
        } else {
            if (rfull) {   // coincident with the robot (or a NaN state): the stored belief, extrapolated
                bvx = S.b_vx[ghh]; bvy = S.b_vy[ghh]; br = S.b_r[ghh];
                bpx = S.b_px[ghh] + bvx * dt; bpy = S.b_py[ghh] + bvy * dt;
            } else {
                bvx = HF(sl, H_BVX, hh); bvy = HF(sl, H_BVY, hh); br = HF(sl, H_BR, hh);
                bpx = HF(sl, H_BPX, hh) + bvx * dt; bpy = HF(sl, H_BPY, hh) + bvy * dt;
            }
        }
        // staged in LDS: the state / observation stores go out after phase 2 from consecutive lanes (one
        // lane per quad here would split every 128-B line of a field over several waves' partial writes:
        // +4 MB of HBM writes per C2 launch, measured)
        hst_ref(hh, 0) = nvx; hst_ref(hh, 1) = nvy;
        hst_ref(hh, 2) = bpx; hst_ref(hh, 3) = bpy; hst_ref(hh, 4) = bvx; hst_ref(hh, 5) = bvy;
        hst_ref(hh, 6) = br;
        uint32_t f = vr ? LF_VR : 0u;
        if (np_norm2(HF(sl, H_GX, hh) - npx, HF(sl, H_GY, hh) - npy) < HF(sl, H_R, hh)) f |= LF_ENDGOAL;
        if (!(npx == npx) || !(npy == npy)) f |= 0x80000000u;
        sl.eg[hh] = f;
        sl.npx[hh] = npx; sl.npy[hh] = npy;   // post-move positions for the goal changes (HF keeps the pre-move
                                              // ones: other humans' simulators may still be reading them)
    };
    // ---- phase 2: human policy (PRE-move state) -------------------------------------------------
    double nvx = 0.0, nvy = 0.0;
    {
        const int nh = nenv_here * N;
        if (orca) {
            // ORCA.predict for every human (orca.py:64-139), a quad of lanes per human. The neighbour list
            // (Agent::insertAgentNeighbor with maxNeighbors = M: every agent within neighborDist) is the
            // in-range slots stably sorted by distSq in the order RVO2's KdTree visits them. <= 10 agents:
            // one leaf, so that order is the simulator's agents_ order = slot order, and lane sq builds the
            // lines of slots sq, sq+4, sq+8 and ranks them itself. > 10 agents: lane 0 of the quad runs the
            // KdTree build (which also re-permutes the persisted agents_ order) and query, the quad then
            // builds the lines in neighbour order.
            const int h = tid >> 2, sq = tid & 3;
            {
                // lanes of quads past the last human (h >= nh) stay in step for the KdTree walk (whole
                // waves) and skip the per-human work; their LDS reads stay inside the [H] arrays
                const bool hq = h < nh;
                const int elq = h / N, iq = h - elq * N, eb = elq * N;
                const uint32_t visq = sl.vis[h], dmq = sl.dm[h];
                const double px = HF(sl, H_PX, h), py = HF(sl, H_PY, h);
                const float rdummy = (float)(c.human_radius + 0.01 + c.orca_safety_space);
                const float X0 = (float)px, Y0 = (float)py;
                const float VX0 = (float)HF(sl, H_VX, h), VY0 = (float)HF(sl, H_VY, h);
                const float R0 = sl.orad[h];
                const float rangeSq = (float)c.orca_neighbor_dist * (float)c.orca_neighbor_dist;
                const float invTH = fdiv(1.0f, (float)c.orca_time_horizon);
                const float invTS = fdiv(1.0f, (float)dt);
                // preferred velocity: unit vector to the goal only if farther than 1 (orca.py:118-122)
                double gdx = HF(sl, H_GX, h) - px, gdy = HF(sl, H_GY, h) - py;
                const double speed = np_norm2(gdx, gdy);
                if (speed > 1.0) { gdx = ddiv(gdx, speed); gdy = ddiv(gdy, speed); }
                float4 *Lb = sl.lines + h * M, *Pb = sl.proj + h * M;
                bool vr_kd = false;   // kd-tree path: path violation, tested before Pb is reused
                int cnt = 0;
                uint32_t inm = 0;
                if constexpr (!KD) {
                  if (hq)
                    cnt = orca_lines_quad(
                        [&](int k, float &x, float &y, float &vx, float &vy, float &r) {
                            slot_agent(sl, c, eb, elq, EPB, N, iq, k, visq, dmq, rdummy, x, y, vx, vy, r);
                        },
                        M, sq, X0, Y0, VX0, VY0, R0, rangeSq, invTH, invTS, Lb);
                } else {
                    // (1) the quad loads the persisted KdTree order and fills, in that order, the agents'
                    //     positions (XYP[q] = agent perm[q]: self = 0, slot k = k + 1; kept in the projected-
                    //     lines space, unused until linearProgram3) and each slot's distSq
                    // (0) the path-violation test reads this human's velocity rectangle from Pb, which the
                    //     KdTree exchange reuses below
                    if (hq && info_on) vr_kd = path_vr_q(h, sq);   // the whole quad
                    wsync();
                    const int HS = P.NH;   // LDS stride of the per-human slot / KdTree order arrays
                    float2 *XYP = (float2 *)Pb;          // [A] (x, y) in KdTree order, then the exchange space
                    float *D = (float *)Pb + 2 * A;      // [M] distSq of each slot (beside XYP in Pb)
                    uint8_t *perm = sl.perm, *tpos = sl.ns;
                    const bool frz = (sl.rflag[elq] & CN_FLAG_ORCA_FROZEN) != 0;
                    const int gq = (e0 + elq) * N + iq;
                    for (int q = sq; q < A && hq; q += 4) {
                        const int a = frz ? S.o_perm[gq * A + q] : q;
                        perm[q * HS + h] = (uint8_t)a;
                        if (a == 0) { XYP[q] = make_float2(X0, Y0); continue; }
                        float x, y, vx, vy, r;
                        slot_agent(sl, c, eb, elq, EPB, N, iq, a - 1, visq, dmq, rdummy, x, y, vx, vy, r);
                        XYP[q] = make_float2(x, y);
                        const float dx = X0 - x, dy = Y0 - y;
                        D[a - 1] = dx * dx + dy * dy;
                        if (D[a - 1] < rangeSq) inm |= 1u << (a - 1);
                    }
                    inm = (uint32_t)quad_or((int)inm);
                    wsync();
                    STAMP_A(15);
                    // (2) KdTree build (buildAgentTreeRecursive, which re-permutes the persisted agents_ order)
                    //     fused with the query's depth-first walk (queryAgentTreeRecursive: closer child first,
                    //     ties -> right). 4 lanes per human (lane sub holds positions sub, sub+4, ..., sub+28
                    //     of the agent order), all 16 humans of a wave at once (8 lanes and two rounds of 8
                    //     humans before: the walk's critical path was twice as long). Every node is partitioned
                    //     once: Hoare's two-pointer loop swaps the i-th element >= split left of the cut with the
                    //     i-th element < split counted from the right end, which ballots and popcounts give
                    //     directly (exchange through the human's projected-lines space). The children's
                    //     bounding boxes (exact min / max over the quad) give both the visiting order and
                    //     their own split. Pruned subtrees hold no agent within range, so walking them inserts
                    //     nothing: the in-range agents' visiting order tpos is the order
                    //     Agent::insertAgentNeighbor sees. The explicit stack (<= A - 9 entries) lives in the
                    //     sorted-lines space, written only after the walk.
                    //     The body is predicated rather than branched per element: every element's LDS write goes
                    //     to its slot or to a dummy slot of the human (tpos row M, perm row A, the exchange entry
                    //     XD past the distances), every read comes from a valid address and is selected, and the
                    //     group masks are quad ORs of per-lane bit sets (lane sub holds positions sub + 4u).
                    {
                        const int lane = tid & 63, grp = lane >> 2, sub = lane & 3;
                        const int wbase = (tid >> 6) * 16;
                        const uint32_t sbit = 1u << sub;
                        auto gmask = [&](const bool (&pr)[8]) -> uint32_t {
                            uint32_t m = 0;
#pragma unroll
                            for (int u = 0; u < 8; ++u) m |= pr[u] ? (sbit << (4 * u)) : 0u;
                            return (uint32_t)quad_or((int)m);
                        };
                        if (wbase + grp < nh) {   // 16 humans per wave, 4 lanes each, all at once
                            const int hw = wbase + grp;
                            const int elw = hw / N, iw = hw - elw * N;
                            const int gw = (e0 + elw) * N + iw;
                            int4 *stk = (int4 *)(sl.lines + hw * M);
                            // exchange: (x, y) of 2 x (A / 2) entries in Pb, their agent ids in perm (read once
                            // above); a slot's in-range test is bit (agent - 1) of the quad's inm
                            float2 *xch = (float2 *)(sl.proj + hw * M);
                            const int XD = (2 * A + M + 1) / 2;   // dummy exchange entry (floats [2A + M, 4M) are free)
                            uint8_t *permw = perm + hw, *tposw = tpos + hw;
                            const float SX = (float)HF(sl, H_PX, hw), SY = (float)HF(sl, H_PY, hw);
                            float px[8], py[8];
                            int pa[8];
                            bool inr[8];   // element u is an agent within range (bit pa - 1 of inm)
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                const int q = sub + 4 * u;
                                const bool v = q < A;
                                const float2 t = xch[v ? q : XD];
                                px[u] = v ? t.x : 0.0f; py[u] = v ? t.y : 0.0f;
                                const int a = permw[(v ? q : A) * HS];
                                pa[u] = v ? a : 0;
                                inr[u] = pa[u] != 0 && ((inm >> ((pa[u] - 1) & 31)) & 1u);
                            }
                            auto red = [&](int b0, int e1, float &mnx, float &mxx, float &mny, float &mxy) {
                                float a0 = INFINITY, a1 = -INFINITY, c0 = INFINITY, c1 = -INFINITY;
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int q = sub + 4 * u;
                                    const bool in = q >= b0 && q < e1;
                                    a1 = in && a1 < px[u] ? px[u] : a1; a0 = in && px[u] < a0 ? px[u] : a0;
                                    c1 = in && c1 < py[u] ? py[u] : c1; c0 = in && py[u] < c0 ? py[u] : c0;
                                }
                                mnx = quad_min(a0); mxx = quad_max(a1); mny = quad_min(c0); mxy = quad_max(c1);
                            };
                            // z: bit 0 = split on x, bit 1 = all points coincide (zero-extent box)
                            auto entry = [&](int b0, int e1, float mnx, float mxx, float mny, float mxy) {
                                const bool vert = (mxx - mnx > mxy - mny);
                                const float split = vert ? 0.5f * (mxx + mnx) : 0.5f * (mxy + mny);
                                const int deg = (mnx == mxx && mny == mxy) ? 2 : 0;
                                return make_int4(b0, e1, (vert ? 1 : 0) | deg, __float_as_int(split));
                            };
                            int sp = 0, tc = 0;
#ifdef CN_STAMPS
                            int dbg_it = 0;
#endif
                            {
                                float mnx, mxx, mny, mxy;
                                red(0, A, mnx, mxx, mny, mxy);
                                stk[0] = entry(0, A, mnx, mxx, mny, mxy);
                                sp = 1;
                            }
                            while (sp > 0) {
#ifdef CN_STAMPS
                                ++dbg_it;
#endif
                                const int4 en = stk[--sp];
                                const int b0 = en.x, e1 = en.y;
                                const bool leaf = e1 - b0 <= 10;           // RVO_MAX_LEAF_SIZE
                                const bool deg = !leaf && (en.z & 2) != 0;
                                // insertions of a leaf (positions [b0, e1) in order) or of a node whose points all
                                // coincide (e.g. the dummies of unseen humans, all at (7, 7)): no split separates
                                // them, so each level peels its first element into a one-agent leaf, nothing moves,
                                // and the equal-distance children are visited right first: positions [e1-10, e1) in
                                // order (set 1), then e1-11 down to b0 (set 2). Internal nodes insert nothing.
                                const int lo1 = leaf ? b0 : (deg ? e1 - 10 : e1), hi2 = deg ? e1 - 10 : b0;
                                bool s1[8], s2[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int q = sub + 4 * u;
                                    s1[u] = q >= lo1 && q < e1 && inr[u];
                                    s2[u] = q >= b0 && q < hi2 && inr[u];
                                }
                                const uint32_t b1 = gmask(s1), b2 = gmask(s2);
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int q = sub + 4 * u;
                                    const int r1 = tc + __popc(b1 & ((1u << q) - 1u));
                                    const int r2 = tc + __popc(b1) + __popc(b2 >> q >> 1);
                                    const bool w = s1[u] || s2[u];
                                    tposw[(w ? pa[u] - 1 : M) * HS] = (uint8_t)(s1[u] ? r1 : r2);
                                }
                                tc += __popc(b1) + __popc(b2);
                                if (leaf || deg) continue;
                                const float split = __int_as_float(en.w);
                                bool lt[8], pr[8], pL[8], pR[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int q = sub + 4 * u;
                                    lt[u] = ((en.z & 1) ? px[u] : py[u]) < split;
                                    pr[u] = q >= b0 && q < e1 && lt[u];
                                }
                                const int mid = b0 + __popc(gmask(pr));
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int q = sub + 4 * u;
                                    const bool in = q >= b0 && q < e1;
                                    pL[u] = in && q < mid && !lt[u];
                                    pR[u] = in && q >= mid && lt[u];
                                }
                                const uint32_t Lm = gmask(pL), Rm = gmask(pR);
                                if (Lm) {   // Hoare's swaps: the i-th misplaced left element with the i-th right one
                                    const int nsw = __popc(Lm);
                                    int src[8];
#pragma unroll
                                    for (int u = 0; u < 8; ++u) {
                                        const int q = sub + 4 * u;
                                        const bool mv = pL[u] || pR[u];
                                        const int slot = pL[u] ? __popc(Lm & ((1u << q) - 1u)) : nsw + __popc(Rm >> q >> 1);
                                        const int ws = mv ? slot : XD;
                                        xch[ws] = make_float2(px[u], py[u]);
                                        permw[(mv ? slot : A) * HS] = (uint8_t)pa[u];
                                        src[u] = mv ? (pL[u] ? slot + nsw : slot - nsw) : -1;
                                    }
                                    wsync();
#pragma unroll
                                    for (int u = 0; u < 8; ++u) {
                                        const bool mv = src[u] >= 0;
                                        const float2 t = xch[mv ? src[u] : XD];
                                        const int a = permw[(mv ? src[u] : A) * HS];
                                        px[u] = mv ? t.x : px[u]; py[u] = mv ? t.y : py[u];
                                        pa[u] = mv ? a : pa[u];
                                        inr[u] = pa[u] != 0 && ((inm >> ((pa[u] - 1) & 31)) & 1u);
                                    }
                                    wsync();
                                }
                                const int left = mid == b0 ? mid + 1 : mid;
                                float l0, l1, l2, l3, r0, r1, r2, r3;
                                red(b0, left, l0, l1, l2, l3);
                                red(left, e1, r0, r1, r2, r3);
                                const int4 cl = entry(b0, left, l0, l1, l2, l3), cr = entry(left, e1, r0, r1, r2, r3);
                                const float dl = bbox_dist(SX, SY, l0, l1, l2, l3);
                                const float dr = bbox_dist(SX, SY, r0, r1, r2, r3);
                                // (all 4 lanes store the same entries) left visited first when strictly closer
                                stk[sp] = dl < dr ? cr : cl;
                                stk[sp + 1] = dl < dr ? cl : cr;
                                sp += 2;
                                wsync();
                            }
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                const int q = sub + 4 * u;
                                if (q < A) S.o_perm[gw * A + q] = (uint8_t)pa[u];
                            }
#ifdef CN_STAMPS
                            if (threadIdx.x == 0 && blockIdx.x < 4096) cn_stamp_a[blockIdx.x * CN_NSTAMP + 13] = dbg_it;
#endif
                        }
                    }
                    wsync();
                    STAMP_A(14);
                    if (hq) {
                    // (3) neighbour rank = stable order of (distSq, visiting order): each lane ranks its slots
                    //     sq, sq+4, ... in one pass over the in-range slots, then writes their lines
                    float myD[8];
                    int myT[8], rk[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int k = sq + 4 * u;
                        const bool in = k < M && ((inm >> k) & 1u);
                        myD[u] = in ? D[k] : 0.0f;
                        myT[u] = in ? tpos[k * HS + h] : 0;
                        rk[u] = 0;
                    }
                    for (uint32_t mq = inm; mq; mq &= mq - 1) {
                        const int q = __ffs(mq) - 1;
                        const float dq = D[q];
                        const int tq = tpos[q * HS + h];
#pragma unroll
                        for (int u = 0; u < 8; ++u) rk[u] += (dq < myD[u] || (dq == myD[u] && tq < myT[u])) ? 1 : 0;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int k = sq + 4 * u;
                        if (k < M && ((inm >> k) & 1u)) {
                            float ox, oy, ovx, ovy, orr;
                            slot_agent(sl, c, eb, elq, EPB, N, iq, k, visq, dmq, rdummy, ox, oy, ovx, ovy, orr);
                            Lb[rk[u]] = orca_line(X0, Y0, VX0, VY0, R0, ox, oy, ovx, ovy, orr, invTH, invTS);
                        }
                    }
                    }
                    cnt = __popc(inm);
                }
                wsync();
                STAMP_A(7);
                STAMP_W(0);
                if constexpr (!KD) {   // <= 12 lines: register-resident linear programs
                    uint32_t *l3b = (uint32_t *)(smem + P.o_l3b);
                    float2 *l3r = (float2 *)(smem + P.o_l3r);
                    uint8_t *l3k = (uint8_t *)(smem + P.o_l3k);
                    float rx = 0.0f, ry = 0.0f;
                    int fail_at = 0;
                    float4 R[3];
#pragma unroll
                    for (int u = 0; u < 3; ++u)
                        R[u] = hq && sq + 4 * u < cnt ? Lb[sq + 4 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
#ifdef CN_STAMPS
                    LpCount lc2 = {0, 0}, lc3 = {0, 0};
                    if (hq) fail_at = lp2_r<3, LP2W>(R, cnt, sl.vmax[h], (float)gdx, (float)gdy, sq, rx, ry, Lb, &lc2);
                    {
                        int uni = 0, mx = 0;
                        lp_count_wave(lc2, uni, mx);
                        STAMP_WV(5, (unsigned long long)uni);
                        STAMP_WV(6, (unsigned long long)mx);
                    }
#else
                    if (hq) {
                        fail_at = lp2_r<3, LP2W>(R, cnt, sl.vmax[h], (float)gdx, (float)gdy, sq, rx, ry, Lb);
                    }
#endif
                    STAMP_A(8);
                    STAMP_W(1);
                    // linearProgram3 of the workgroup's infeasible humans: every sub-problem their loops may
                    // visit, solved by all quads (lp3_tasks), then each human's quad replays its loop
                    const bool l3 = hq && fail_at < cnt;
                    const int l3e = min(cnt, fail_at + CN_LP3_W);
                    if (sq == 0) l3b[h] = l3 ? (uint32_t)(fail_at | (l3e << 8)) : 0u;
                    // the calc_reward ladder here, while the waves wait for the slowest linearProgram2 at this
                    // barrier (after the linear programs it was the last item of its wave's phase 2: stamps of the
                    // driver's window put it at ~5 k of the slowest workgroups' ~63 k phase-2 cycles). It reads only
                    // phase-1 results and writes no value the linear programs or human_post read. Not with norm
                    // zones: their separating-axis tests make the ladder longer than that slack (C5 -1 %, A/B)
                    if (!c.norm_zones) {
                        if (rl) ladder();
                        ladder_done = true;
                    }
                    __syncthreads();
#ifdef CN_STAMPS
                    const unsigned long long tl3 = clock64();
                    STAMP_W(2);
                    lp3_tasks<3>(sl.lines, M, sl.vmax, l3b, l3r, l3k, tid, &lc3);
                    STAMP_W(3);
                    STAMP_WV(7, (unsigned long long)(lc3.bodies & 0xfff));
                    STAMP_WV(8, (unsigned long long)(lc3.bodies >> 12 & 0xfff));
                    STAMP_WV(9, (unsigned long long)(lc3.bodies >> 24));
#else
                    lp3_tasks<3>(sl.lines, M, sl.vmax, l3b, l3r, l3k, tid);
#endif
                    __syncthreads();
                    int l3vis = 0;
                    if (l3) l3vis = lp3_replay<3>(R, Lb, cnt, fail_at, l3e, sl.vmax[h], sq, l3r + h * 12, l3k + h * 12, rx, ry);
#ifdef CN_STAMPS
                    if (tid == 0 && (unsigned)sb < 4096) cn_stamp_a[sb * CN_NSTAMP + 23] = clock64() - tl3;
#endif
                    (void)l3vis;
                    STAMP_A(9);
                    if (hq) {
                        const bool vr = info_on && path_vr_q(h, sq);   // the whole quad
                        if (sq == 0) human_post(h, (double)rx, (double)ry, vr);
                    }
                    STAMP_W(4);
                } else if (hq) {
                    float rx, ry;
                    const float vmq = sl.vmax[h];
                    const int fail_at = lp2_q(Lb, cnt, vmq, (float)gdx, (float)gdy, sq, rx, ry);
                    STAMP_A(8);
                    if (fail_at < cnt) lp3_q(Lb, Pb, cnt, fail_at, vmq, sq, rx, ry);
                    STAMP_A(9);
                    wsync();   // the quad's last reads of Pb (linearProgram3) before human_post stages into it
                    if (sq == 0) human_post(h, (double)rx, (double)ry, vr_kd);
                }
            }
        } else if (hl) {
            const int eb = el * N;
            const double px = HF(sl, H_PX, tid), py = HF(sl, H_PY, tid);
            const double vx0 = HF(sl, H_VX, tid), vy0 = HF(sl, H_VY, tid);
            const double rad = HF(sl, H_R, tid), vpref = HF(sl, H_VP, tid);
            // SOCIAL_FORCE.predict (social_force.py:11-66)
            const double dx = HF(sl, H_GX, tid) - px, dy = HF(sl, H_GY, tid) - py;
            const double dist = dsqrt(dx * dx + dy * dy);
            const double dvx = ddiv(dx, dist) * vpref, dvy = ddiv(dy, dist) * vpref;
            const double cdx = c.sf_KI * (dvx - vx0), cdy = c.sf_KI * (dvy - vy0);
            double ix = 0.0, iy = 0.0;
            for (int k = 0; k < M; ++k) {
                double ox, oy, orr;
                const bool v = (vis >> k) & 1u;
                if (k < N - 1) {
                    const int j = eb + (k < i ? k : k + 1);
                    ox = v ? HF(sl, H_PX, j) : CN_DUMMY_POS; oy = v ? HF(sl, H_PY, j) : CN_DUMMY_POS;
                    orr = v ? HF(sl, H_R, j) : c.human_radius;
                } else {
                    ox = v ? RF(sl, R_PX, el, EPB) : CN_DUMMY_POS; oy = v ? RF(sl, R_PY, el, EPB) : CN_DUMMY_POS;
                    orr = v ? RF(sl, R_RAD, el, EPB) : c.robot_radius;
                }
                const double ddx = px - ox, ddy = py - oy;
                const double d = dsqrt(ddx * ddx + ddy * ddy);
                const double ex = exp(ddiv(rad + orr - d, c.sf_B));
                ix += c.sf_A * ex * ddiv(ddx, d);
                iy += c.sf_A * ex * ddiv(ddy, d);
            }
            const double tx = (cdx + ix) * dt, ty = (cdy + iy) * dt;
            const double nx = vx0 + tx, ny = vy0 + ty;
            const double n = np_norm2(nx, ny);
            if (n > vpref) { nvx = ddiv(nx, n) * vpref; nvy = ddiv(ny, n) * vpref; }
            else { nvx = nx; nvy = ny; }
            human_post(tid, nvx, nvy, info_on && path_vr(tid));
        }
        STAMP_T(21, 64);
        if (rl && !ladder_done) ladder();
        STAMP_T(20, 64);
    }
    __syncthreads();
    STAMP_A(3);

    // ---- human state / observation stores (human lanes, consecutive) beside the robot kinematics, state
    //      and observation stores and RNG needs (env lanes) ---------------------------------------------
    if (hl) {
        S.h_px[gh] = sl.npx[tid]; S.h_py[gh] = sl.npy[tid];
        S.h_vx[gh] = hst_ref(tid, 0); S.h_vy[gh] = hst_ref(tid, 1);
        const double bpx = hst_ref(tid, 2), bpy = hst_ref(tid, 3);
        S.b_px[gh] = bpx; S.b_py[gh] = bpy; S.b_vx[gh] = hst_ref(tid, 4); S.b_vy[gh] = hst_ref(tid, 5);
        S.b_r[gh] = hst_ref(tid, 6);
        if (emit_obs) {
            const int64_t oh = (orw_o + orow(ov, e0 + el)) * ov.NS + i;
            g.spatial[oh * 2] = (float)(bpx - RF(sl, R_NX, el, EPB));
            g.spatial[oh * 2 + 1] = (float)(bpy - RF(sl, R_NY, el, EPB));
        }
    }
    if (rl) {
        // robot kinematics (agent.py:198-212): the post-move state computed in phase 1
        const uint32_t flags = sl.rflag[re];
        const float a0 = sl.act[re], a1 = sl.act[EPB + re];
        if (holo) { RF(sl, R_VX, re, EPB) = a0; RF(sl, R_VY, re, EPB) = a1; }
        else {
            RF(sl, R_TH, re, EPB) = RF(sl, R_NTH, re, EPB);
            RF(sl, R_VX, re, EPB) = RF(sl, R_CVX, re, EPB); RF(sl, R_VY, re, EPB) = RF(sl, R_CVY, re, EPB);
        }
        sl.rflag[re] = flags | CN_FLAG_ROBOT_F32;
        const double nx = RF(sl, R_NX, re, EPB), ny = RF(sl, R_NY, re, EPB);
        S.r_px[ge] = nx; S.r_py[ge] = ny;
        S.r_vx[ge] = RF(sl, R_VX, re, EPB); S.r_vy[ge] = RF(sl, R_VY, re, EPB);
        S.r_theta[ge] = RF(sl, R_TH, re, EPB);
        S.r_dv[ge] = RF(sl, R_DV, re, EPB);
        S.potential[ge] = RF(sl, R_POT, re, EPB);
        const double gt = RF(sl, R_GT, re, EPB);
        S.gtime[ge] = gt;
        uint32_t flags2 = sl.rflag[re];
        if (orca) flags2 |= CN_FLAG_ORCA_FROZEN;
        bool endg = false, nan = false;
        int vr_viol = 0;
        const int kv = (int)sl.rflag[2 * EPB + re];
        for (int k = 0; k < N; ++k) {
            const uint32_t f = sl.eg[re * N + k];
            endg |= (f & LF_ENDGOAL) != 0;
            nan |= (f & 0x80000000u) != 0;
            vr_viol += (k < kv && (f & LF_VR)) ? 1 : 0;
        }
        if (emit && g.info) g.info[(orw_e + orow(ov, ge)) * CN_INFO_K + CN_INFO_PATH_VIOLATION] = (float)vr_viol;
        if (nan) flags2 |= CN_FLAG_NAN;
        S.flags[ge] = flags2;
        if (emit_obs) {
            const int64_t oe = orw_o + orow(ov, ge);
            float *rn = g.robot_node + oe * 7;
            rn[0] = (float)nx; rn[1] = (float)ny; rn[2] = (float)RF(sl, R_RAD, re, EPB);
            rn[3] = (float)RF(sl, R_GX, re, EPB); rn[4] = (float)RF(sl, R_GY, re, EPB);
            rn[5] = (float)RF(sl, R_VP, re, EPB); rn[6] = (float)RF(sl, R_TH, re, EPB);
            g.temporal[oe * 2] = (float)RF(sl, R_VX, re, EPB);
            g.temporal[oe * 2 + 1] = (float)RF(sl, R_VY, re, EPB);
            for (int k = N; k < ov.NS; ++k) {   // padding slots of a mixed engine (never-seen humans)
                g.spatial[(oe * ov.NS + k) * 2] = (float)(CN_PAD_POS - nx);
                g.spatial[(oe * ov.NS + k) * 2 + 1] = (float)(CN_PAD_POS - ny);
            }
        }
        // random numbers needed? (crowd_sim_dict.py:260-269, shmem_vec_env.py:166-167)
        // GOAL_EARLY: the word stays "done" (waves 2 and 3 are reading it for their goal items; phase 5 serves the
        // done envs alone)
        if constexpr (!GOAL_EARLY) {
            const bool done = sl.rflag[EPB + re] != 0;
            const bool rgoal = c.random_goal_changing && np_mod(gt, 5.0) == 0.0;
            const bool egoal = c.end_goal_changing && endg;
            sl.rflag[EPB + re] = (done ? 1u : 0u) | (rgoal ? 2u : 0u) | (egoal ? 4u : 0u);
        }
    }
    if ((tid >> 6) == 1) {   // the env lanes' wave: one mask of the envs with RNG work, for phase 5's item split
        const uint64_t bm = __ballot(rl && (GOAL_EARLY ? sl.rflag[EPB + re] : sl.rflag[EPB + re] & 7u) != 0u);
        if (tid == 64) { sl.rflag[3 * EPB] = (uint32_t)bm; sl.rflag[3 * EPB + 1] = (uint32_t)(bm >> 32); }
    }
    if constexpr (GOAL_EARLY) {
        // ---- waves 2 and 3, idle until the barrier below: the goal changes of the envs that go on with their episode,
        // beside the stores above. What decides them is final since phase 2's closing barrier: done (the ladder's
        // word, which the env lanes leave as it is), gtime as the ladder advanced it, the humans' LF_ENDGOAL. An item
        // reads the post-move positions, the humans' goals / radii / v_pref / headings and the robot's R_NX, R_NY,
        // R_GX, R_GY, R_RAD and the env's stream; it writes the goals, radii, v_pref (LDS and state) and the stream:
        // none of these is read or written by the stores above. Both waves work out the same list of envs and take
        // every other item of it, each in its own RNG region (2 and 3: over phase 2's neighbour distances and
        // linearProgram3 tables, clear of the staged values wave 0 is reading, cn_goal_early_ok). No wave waits
        // for another one but at the barriers.
        if ((tid >> 6) >= 2) {
            const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
            bool gneed = false, grand = false;
            if (lane < nenv_here) {
                bool endg = false;
                for (int k = 0; k < N; ++k) endg |= (sl.eg[lane * N + k] & LF_ENDGOAL) != 0;
                grand = c.random_goal_changing && np_mod(RF(sl, R_GT, lane, EPB), 5.0) == 0.0;
                gneed = sl.rflag[EPB + lane] == 0u && (grand || (c.end_goal_changing && endg));
            }
            const uint64_t gm = __ballot(gneed), grm = __ballot(grand);
            uint64_t mym = 0;
            {
                int jj = 0;
                for (uint64_t mm = gm; mm; mm &= mm - 1, ++jj)
                    if ((jj & 1) == w - 2) mym |= mm & (~mm + 1);
            }
            if (mym) {
                char *wb = smem + P.o_lines + w * P.rng_stride;
                WRng m;
                m.w = (uint32_t *)wb; m.off = 0; m.lane = lane; m.phx = PHX; m.edbg = -1;
                m.grid = P.rng_stride > CN_PEND_LDS ? wb + CN_PEND_LDS : nullptr;
                m.sl = (double *)(wb + 2 * CN_MT_N * 4 + 7 * 32 * 8);
                double *hb = (double *)(wb + 2 * CN_MT_N * 4);
                for (uint64_t mm = mym; mm; mm &= mm - 1) {
                    const int q = __builtin_ctzll(mm);
                    // (the kernel arguments from the kernarg segment, as in phase 5's loop below and for its reasons)
                    typedef const __attribute__((address_space(4))) char *KArgs;
                    typedef const __attribute__((address_space(4))) StepArgs *GArgs;
                    typedef const __attribute__((address_space(4))) cn_config *CArgs;
                    KArgs ks = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
                    asm volatile("" : "+s"(ks));
                    GArgs gq = (GArgs)ks;
                    CArgs cq = (CArgs)(ks + ((sizeof(StepArgs) + alignof(cn_config) - 1) & ~(alignof(cn_config) - 1)));
                    const StepArgs &G = *(const StepArgs *)gq;
                    const cn_config &C = *(const cn_config *)cq;
                    const int64_t e = e0 + q;
                    const int64_t se = CN_STAMP_ON ? e : -1;
                    (void)se;
                    STAMP_B(se, 0);
                    Env1 en;
                    const int b = q * N;
                    en.hpx = sl.npx + b; en.hpy = sl.npy + b; en.hgx = &HF(sl, H_GX, b);
                    en.hgy = &HF(sl, H_GY, b); en.hr = &HF(sl, H_R, b); en.hvp = &HF(sl, H_VP, b); en.hth = &HF(sl, H_TH, b);
                    en.rpx = RF(sl, R_NX, q, EPB); en.rpy = RF(sl, R_NY, q, EPB);
                    en.rgx = RF(sl, R_GX, q, EPB); en.rgy = RF(sl, R_GY, q, EPB); en.rr = RF(sl, R_RAD, q, EPB);
                    m.edbg = se;
                    goal_changes<KD>(C, G.s, e, en, m, ((grm >> q) & 1ull) != 0, C.end_goal_changing != 0, hb);
                }
            }
        }
    }
    STAMP_A(4);        // waves 0 and 1 at the barrier: their stores are issued (the barrier waits for them)
    STAMP_T(11, 64);
    __syncthreads();
    STAMP_A(5);

    // ---- phase 5: this workgroup's RNG work, one wave per env needing it --------------------------
    // Done envs auto-reset (VecEnv worker, shmem_vec_env.py:164-168) from the pending spawn drawn by an
    // earlier launch (reset_env: two slots per env, consumed only when an earlier launch completed the entry);
    // after cn_reset / cn_set_state, while this launch's spawn waves draw every env's entries, they draw inline.
    // GOAL_EARLY: the done envs alone (the mask holds no other), the goal changes having run beside the stores.
    bool rng_any = true;   // GOAL_EARLY: some env of the workgroup resets in this step (workgroup-uniform)
    {
        // the wave index is wave-uniform: readfirstlane keeps it (and every LDS pointer derived from it) in
        // SGPRs -- as a VGPR value the RNG block's preheader spilled it to scratch (HBM writes every launch)
        const int nw = P.rng_waves, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        char *wb = smem + P.o_lines + (w < nw ? w : 0) * P.rng_stride;   // over the ORCA scratch, dead after phase 2
        WRng m;
        m.w = (uint32_t *)wb; m.off = 0; m.lane = lane; m.phx = PHX; m.edbg = -1;
        m.grid = P.rng_stride > CN_PEND_LDS ? wb + CN_PEND_LDS : nullptr;
        m.sl = (double *)(wb + 2 * CN_MT_N * 4 + 7 * 32 * 8);
        double *hb = (double *)(wb + 2 * CN_MT_N * 4);
        // the RNG waves' goal loops end most of the slowest workgroups (kd-tree path): issue priority over
        // the other workgroups' waves on their SIMD (C3 460.3 / 461.6 -> 456.8 / 456.4 us per launch, A/B)
        if (KD && w < nw) __builtin_amdgcn_s_setprio(3);
        // waves without an env to serve skip the block entirely: the loop's preheader (values the
        // compiler hoists out of the RNG work, and their spill stores) then runs only where it is needed.
        // The envs with work, in env order, go round-robin to the RNG waves: this wave's share from the mask
        // wave 1 wrote (scalar bit loop, one LDS read instead of a dependent chain over the envs' flags)
        const uint64_t rm = ((uint64_t)__builtin_amdgcn_readfirstlane(sl.rflag[3 * EPB + 1]) << 32) |
                            (uint64_t)__builtin_amdgcn_readfirstlane(sl.rflag[3 * EPB]);
        uint64_t mym = 0;
        {
            int jj = 0;
            for (uint64_t mm = rm; mm; mm &= mm - 1, ++jj)
                if (jj % nw == w) mym |= mm & (~mm + 1);
        }
        if constexpr (GOAL_EARLY) rng_any = rm != 0;
        STAMP_T(22, 0);
        if (mym) {
        for (uint64_t mm = mym; mm; mm &= mm - 1) {
            const int q = __builtin_ctzll(mm);
            // the kernel arguments through pointers the compiler cannot see across iterations: their loads stay at
            // the uses in this body instead of a preheader that reloaded ~30 of them one by one and parked ~250
            // SGPR values in VGPR lanes before the first item (~4 k cycles on the slowest workgroups)
            // (read from the kernarg segment itself: taking the parameters' addresses would copy them to scratch;
            // by-value arguments in order at their natural alignment, StepArgs at 0, cn_config after it)
            typedef const __attribute__((address_space(4))) char *KArgs;
            typedef const __attribute__((address_space(4))) StepArgs *GArgs;
            typedef const __attribute__((address_space(4))) cn_config *CArgs;
            KArgs ks = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ks));
            GArgs gq = (GArgs)ks;
            CArgs cq = (CArgs)(ks + ((sizeof(StepArgs) + alignof(cn_config) - 1) & ~(alignof(cn_config) - 1)));
            const StepArgs &G = *(const StepArgs *)gq;
            const cn_config &C = *(const cn_config *)cq;
            ResetOut o;
            o.s = G.s; o.robot_node = G.robot_node; o.temporal = G.temporal; o.spatial = G.spatial;
            o.case_size = G.case_size; o.ov = ov;
            if constexpr (ROBOT) {   // the new episode's first observation goes to this step's row as well
                o.robot_node += orw_o * 7; o.temporal += orw_o * 2; o.spatial += orw_o * ov.NS * 2;
            }
            if (SEQ && !emit_obs) o.robot_node = nullptr;   // (write_reset<OBS_OPT>: no first observation)
            const uint32_t need = GOAL_EARLY ? 1u : sl.rflag[EPB + q] & 7u;
            const int64_t e = e0 + q;
            const int64_t se = CN_STAMP_ON ? e : -1;   // (the stamps' env: this step's items only)
            (void)se;
            STAMP_B(se, 0);
            Env1 en;
            if (need & 1u) {
                en.hpx = hb; en.hpy = hb + 32; en.hgx = hb + 64; en.hgy = hb + 96; en.hr = hb + 128; en.hvp = hb + 160;
                en.hth = hb + 192;
                // (pend.all, pend.launch_id, pcount_w and plist_w from the kernel's own copy g: graph mode (DEVSEQ)
                // rewrote them at the top from the device-side step counter; the kernarg segment holds the values of
                // the captured launch)
                const bool may = g.pend.all != PEND_BOTH;   // ready unless this launch redraws both
                // (no fences inside a step launch: write_pending's FENCE)
                reset_env<KD, false, SEQ>(o, G.pend.P, C, G.E, e, G.pend.counter_offset, may, g.pend.launch_id, m, en,
                                          G.pend.stats + 7);
                if (lane == 0) {
                    // the entry carries the counters this reset just wrote (its own stores, read back), so the
                    // next launch's spawn wave keys the spawn after next from them, never from a state that a
                    // later reset of the same env may be rewriting while it reads.
                    // A single-step launch resets an env at most once: at most E entries (k < E guarded all the
                    // same). A multi-step launch may reset an env several times, at keys rc, rc + 1, rc + 2, ...;
                    // their entries (spawns rc + 2, rc + 3, rc + 4, ...) would have spawns two keys apart share
                    // a pending slot and be written by two waves of the next launch. So the launch holds ONE
                    // entry per env and slot parity: a later reset of the same parity overwrites the entry its
                    // workgroup appended (sl.app: its index, kept across the steps; the list is read by the next
                    // launch only), which also keeps the key most likely to be needed. An entry that did not fit
                    // the list (k >= E: up to 2 E are attempted) is dropped for the launch; a dropped entry only
                    // costs an inline draw later.
                    const int64_t ccn = G.s.case_counter[e];
                    const int32_t rcn = G.s.reset_count[e];
                    uint32_t k;
                    if constexpr (SEQ) {
                        uint32_t *const aw = sl.app + 2 * q + (rcn & 1);
                        k = *aw;
                        if (k == 0u) {
                            k = atomicAdd(g.pcount_w, 1u);
                            *aw = k + 1u;
                        } else k -= 1u;
                    } else k = atomicAdd(g.pcount_w, 1u);
                    if (k < (uint32_t)G.E) {
                        uint32_t *q = g.plist_w + 4 * k;
                        q[0] = (uint32_t)e; q[1] = (uint32_t)rcn;
                        q[2] = (uint32_t)(uint64_t)ccn; q[3] = (uint32_t)((uint64_t)ccn >> 32);
                    }
                }
                STAMP_B(se, 5);
            } else {
                const int b = q * N;
                en.hpx = sl.npx + b; en.hpy = sl.npy + b; en.hgx = &HF(sl, H_GX, b);
                en.hgy = &HF(sl, H_GY, b); en.hr = &HF(sl, H_R, b); en.hvp = &HF(sl, H_VP, b); en.hth = &HF(sl, H_TH, b);
                en.rpx = RF(sl, R_NX, q, EPB); en.rpy = RF(sl, R_NY, q, EPB);
                en.rgx = RF(sl, R_GX, q, EPB); en.rgy = RF(sl, R_GY, q, EPB); en.rr = RF(sl, R_RAD, q, EPB);
                // update_human_goal checks every human AFTER the random changes (a new random goal may
                // land within reach of its own human), so it runs whenever end goal changing is on
                m.edbg = se;
                goal_changes<KD>(C, G.s, e, en, m, (need & 2u) != 0, C.end_goal_changing != 0, hb);
            }
        }
        }
        // back to normal priority for the epilogue (graph mode's finish barrier, stamps)
        if (KD && w < nw) __builtin_amdgcn_s_setprio(0);
    }
    // the next step's phase 0 reads the state (and the RNG streams) this step's resets and goal changes wrote
    // through other waves, and rewrites the LDS their RNG regions and agent tables use
    // GOAL_EARLY: without a reset in this step (the mask every wave read after the barrier above) phase 5 was empty and
    // that barrier, which every wave passed after its last goal item and its last store, already is this one
    if constexpr (SEQ) { if (!GOAL_EARLY || rng_any) __syncthreads(); }
#if defined(CN_STAMPS) && CN_STAMP_STEP >= 0
    if constexpr (SEQ) STAMP_A(6);   // the chosen step's end (the stamp behind the loop is the launch's)
#endif
    if constexpr (REC) {
        if (step == g.nsteps - 1) {
            const RolloutRows rr = *(const RolloutRows *)(g.pend.stats + (CN_ROWS_W - 8));
            state_rows_copy(S, rr, g.E, N, (actions - rr.actions) / 2, e0, nenv_here, tid, CN_BLK);
        }
    }
    if constexpr (MASK) {
        if (step == g.nsteps - 1)
            visible_mask_rows(S, ov, e0, nenv_here, N, holo ? 1 : 0, c.robot_fov, g.cth_r, g.mask + orw_o * ov.NS, tid,
                              CN_BLK);
    }
    } while (SEQ && ++step < g.nsteps);
#ifdef CN_STAMPS
    __syncthreads();
    STAMP_A(6);
#endif
    finish();
}

// cn_reset: CrowdSimDict.reset of every env, one wave (single-wave workgroup) per env
__global__ void __launch_bounds__(64) cn_reset_kernel(RngArgs g, cn_config c)
{
    __shared__ uint32_t mtw[2 * CN_MT_N];
    __shared__ double hbuf[7][32];
    __shared__ double slots[6 * 64];
    __shared__ __attribute__((aligned(16))) char gridbuf[CN_GRID_LDS];
    const int lane = threadIdx.x;
    for (int64_t e = blockIdx.x; e < g.E; e += gridDim.x) {
        Env1 en;
        en.hpx = hbuf[0]; en.hpy = hbuf[1]; en.hgx = hbuf[2]; en.hgy = hbuf[3]; en.hr = hbuf[4]; en.hvp = hbuf[5];
        en.hth = hbuf[6];
        WRng m;
        m.w = mtw; m.off = 0; m.lane = lane; m.sl = slots; m.phx = c.rng_mode == CN_RNG_PHILOX; m.edbg = -1;
        m.grid = gridbuf;
        reset_env<true>(g.o, g.pend, c, g.E, e, g.counter_offset, true, 0u, m, en);
        // and the spawns of the env's next two resets (both pending slots), so that the first step launches
        // find every spawn they need drawn (PEND_FRESH): keys = the counters the reset just wrote, advanced
        int64_t cc1 = g.o.s.case_counter[e];
        int32_t rc1 = g.o.s.reset_count[e];
        for (int k = 0; k < (g.draw_next ? 2 : 0); ++k) {
            double rth;
            uint32_t ovf;
            int sc;
            spawn_env<true>(c, c.env_offset + orow(g.o.ov, e), cc1, rc1, g.counter_offset, m, en, rth, ovf, sc);
            const bool in1 = !m.phx && m.p > CN_MT_N;
            write_pending<true>(g.pend, c, g.E, e, en, rth, sc, ovf, m.blk(in1 ? 1 : 0), in1 ? m.p - CN_MT_N : m.p, cc1,
                                rc1, lane, CN_OK_RESET, c.human_num);
            wsync();
            cc1 = (cc1 + c.nenv) % g.o.case_size;   // write_reset's counter update
            rc1 += 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The rest of this translation unit lives in engine/*.h: the stand-alone kernels and all host code. They are
// included here, after the device core above, because they use it (and must stay in this translation unit:
// the host code launches the kernels above; the order below is the kernels' order in the code object).
// ------------------------------------------------------------------------------------------------
#include "engine/edge_features.h"  // cn_edge_features_kernel
#include "engine/lidar.h"          // cn_lidar_obs_kernel, cn_lidar_scan_kernel
#include "engine/aux_kernels.h"    // debug / predictor kernels, cn_robot_act's kernels, ctl / key-snapshot kernels
#include "engine/host_engine.h"    // struct cn_engine, error text, the table of cn_step_kernel's instantiations
#include "engine/host_api.h"       // extern "C": the functions of include/crowdnav.h
