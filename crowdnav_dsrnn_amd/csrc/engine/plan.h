// plan.h -- the tunables, the step kernel's launch geometry and LDS plan (StepPlan, cn_step_plan, cn_goal_early_ok),
// its LDS views (SL, RF / HF) and the lane flag bits. Needs CN_BLK (cn_engine.hip); host and device.
#pragma once

#define CN_MAX_A 32
#ifndef CN_LP3_W
#define CN_LP3_W 12   // linearProgram3 sub-problems solved ahead per infeasible human (lp3_tasks); the rest inline
#endif
#define CN_DUMMY_POS 7.0
#define CN_CTL_NSTEP 12   // work_count words of the device-side step sequence (StepArgs::ctl)
#define CN_CTL_ALL 13
#define CN_CTL_DONE 14

// ------------------------------------------------------------------------------------------------
// launch geometry + LDS plan of kernel A
// ------------------------------------------------------------------------------------------------
struct StepPlan {
    int T;       // threads per workgroup (256)
    int H;       // human-lane stride (64: the humans of EPB envs sit on wave 0's lanes)
    int NH;      // per-human stride of the ORCA scratch arrays (kd-tree path: EPB * N humans; quad path: H)
    int EPB;     // envs per workgroup
    int M;       // observed slots per human (ORCA lines upper bound)
    int A;       // agents per RVO2 simulator
    int kd;      // A > 10: RVO2's KdTree order decides ties between equally distant neighbours
    // LDS byte offsets
    int o_renv, o_racts, o_rflag, o_rvr, o_hum, o_lane, o_orad, o_vis, o_nv, o_eg, o_lines, o_proj, o_nd, o_ns, o_perm,
        o_hvr, o_hst, o_l3b, o_l3r, o_l3k, o_app,
        total;
    int rng_waves;   // phase-5 RNG regions (rng_stride bytes each), laid over o_lines
    int rng_stride;  // CN_PEND_LDS, + CN_GRID_LDS when the plan has room for the spawn's DiscGrid
};

#define CN_RENV_F 27   // robot/env doubles per env in LDS
#define CN_HUM_F 14    // human doubles per lane in LDS
#define CN_PEND_LDS (2 * CN_MT_N * 4 + 7 * 32 * 8 + 6 * 64 * 8)   // per RNG wave: MT ring, agent table, try slots
#ifndef CN_QUAD_BUDGET
// the quad path's spawning waves park their spawns after this budget (and cn_reset pre-draws the next two
// spawns, as on the kd-tree path): round 6's timeline (stamps build without contended atomics) had the
// spawn workgroups end last in 78 % of steady C2 launches, one circle_crossing spawn being ~82 k cycles
#define CN_QUAD_BUDGET 70000   // clock cycles a quad-path spawning wave works per launch before parking
#endif
#ifndef CN_QUAD_SPAWN_WAVES
#define CN_QUAD_SPAWN_WAVES 128   // spawning waves of the quad path's spare workgroups
#endif
#ifndef CN_SEQ_CHUNK
// steps per launch of cn_step_seq (cn_debug_set_seq_chunk; 1: one cn_step launch per step). C2 sweep, us per step
// of the steady window: 1: 38.7, 4: 33.9, 8: 32.0, 16: 30.9, 32: 29.9, 64: 29.6 but with resets that no longer
// find their spawn drawn (a spawn queued in one launch is drawn by the next: > 1 inline draw per step at 64)
#define CN_SEQ_CHUNK 32
#endif
#define CN_GRID 16
#define CN_GRID_LDS (96 * 8 + CN_GRID * CN_GRID * 4 + 4 * 8 + 4 * 8)   // + spawn DiscGrid: agent table, masks, cover, box

__host__ __device__ inline int cn_align16(int x) { return (x + 15) & ~15; }

__host__ __device__ inline StepPlan cn_step_plan(int N, int robot_visible)
{
    StepPlan p;
    p.A = N + (robot_visible ? 1 : 0);
    p.M = p.A - 1;
    p.kd = p.A > 10;
    // 4 waves: the humans of EPB = 64 / N envs on wave 0's lanes for the per-human phases, the env lanes
    // on wave 1, all 256 lanes (4 per human) for ORCA. A > 10 adds the KdTree build / query (one lane of
    // each quad) that fixes RVO2's neighbour order.
    p.T = CN_BLK;
    p.H = 64;
    // at most 16 envs per workgroup: with 1-3 humans per env (side-preference scenarios) 64 / N envs would
    // put up to 64 env lanes' divergent reward / norm-zone work on one wave (C5: 16 -> +6 %; 8 -> -2 %)
    p.EPB = p.H / N < 16 ? p.H / N : 16;
    const int H = p.H;
    const int ML = p.M > 0 ? p.M : 1;
    // the kd-tree path sizes its ORCA scratch for the workgroup's EPB * N humans (quads past them never
    // touch it), so that three workgroups fit a CU's LDS
    p.NH = p.kd ? p.EPB * N : H;
    const int NH = p.NH;
    int o = 0;
    p.o_renv = o;  o = cn_align16(o + CN_RENV_F * p.EPB * 8);
    p.o_racts = o; o = cn_align16(o + 2 * p.EPB * 4);
    p.o_rflag = o; o = cn_align16(o + (3 * p.EPB + 2) * 4);   // + the 64-bit mask of envs with RNG work
    p.o_rvr = o;   o = cn_align16(o + 8 * p.EPB * 8);
    p.o_hum = o;   o = cn_align16(o + CN_HUM_F * H * 8);
    p.o_lane = o;  o = cn_align16(o + H * 8 + H * 4);      // closest distance (f64) + flag word
    p.o_orad = o;  o = cn_align16(o + H * 4);
    p.o_vis = o;   o = cn_align16(o + 3 * H * 4);          // visible mask, dummy mask, frozen max speed
    p.o_nv = o;    o = cn_align16(o + H * 16);             // post-move positions (x [H], y [H])
    p.o_eg = o;    o = cn_align16(o + H * 4);              // goal-reached / NaN flags
    // ORCA, per human: sorted lines [NH][M], projected lines [NH][M], neighbour distances (quad path); kd:
    // neighbour slots [M][NH], KdTree agent order [A][NH]
    p.o_lines = o; o = cn_align16(o + ML * NH * 16);
    p.o_proj = o;  o = cn_align16(o + ML * NH * 16);
    p.o_nd = o;    o = cn_align16(o + (p.kd ? 0 : ML * H * 4));
    p.o_ns = o;    o = cn_align16(o + (p.kd ? (ML + 1) * NH : 0));      // + a dummy row (the KdTree walk)
    p.o_perm = o;  o = cn_align16(o + (p.kd ? (p.A + 1) * NH : 0));     // + a dummy row
    // human velocity rectangles [8][H] (phases 1-2) + the human values human_post stages for the contiguous
    // state / observation stores after phase 2 [7][H]: over the quad path's projected-line / distance
    // scratch, unused there since the linear programs keep their lines in registers. The kd-tree path keeps
    // both in each human's own projected-line block instead (hvr_ref / hst_ref below): the rectangle is
    // consumed at the start of phase 2, before that block holds the KdTree exchange, and the staged values
    // are written after the human's linearProgram3, its last use of the block.
    if (p.kd) { p.o_hvr = p.o_proj; p.o_hst = p.o_proj; }
    else if ((p.o_ns - p.o_proj) >= 15 * H * 8) { p.o_hvr = p.o_proj; p.o_hst = p.o_proj + 8 * H * 8; }
    else { p.o_hvr = o; p.o_hst = o + 8 * H * 8; o = cn_align16(o + 15 * H * 8); }
    // quad path: the workgroup's linearProgram3 sub-problems (lp3_tasks): per human fail | n << 8, results
    // [H][12] (phase 2 only: under the RNG regions)
    p.o_l3b = o;   o = cn_align16(o + (p.kd ? 0 : H * 4));
    p.o_l3r = o;   o = cn_align16(o + (p.kd ? 0 : H * 12 * 8));
    p.o_l3k = o;   o = cn_align16(o + (p.kd ? 0 : H * 12));
    // one RNG wave per env of the workgroup, at most 4 (kd-tree path: EPB = 2 or 5 envs)
    p.rng_waves = p.EPB < 4 ? p.EPB : 4;
    // the DiscGrid region only where it costs no LDS (the kd-tree path's ORCA scratch is larger than the
    // RNG regions it hosts); the quad path keeps its 3 workgroups per CU
    p.rng_stride = p.o_lines + p.rng_waves * (CN_PEND_LDS + CN_GRID_LDS) <= o ? CN_PEND_LDS + CN_GRID_LDS : CN_PEND_LDS;
    const int rng_end = p.o_lines + p.rng_waves * p.rng_stride;
    p.total = o > rng_end ? o : rng_end;
    // multi-step launches: the spawn-list entries a workgroup holds for its envs (SL::app), kept across the steps,
    // so behind everything a step lays out (no other offset moves)
    p.o_app = p.total;
    p.total = cn_align16(p.total + 2 * p.EPB * 4);
    return p;
}

// cn_step_kernel's GOAL_EARLY, its condition on a quad-path plan: waves 2 and 3 run goal items in their RNG regions
// while waves 0 and 1 store the state, so the two regions must lie clear of what the store block reads:
// human_post's staged values (o_hst; everything else it reads lies below o_lines). It holds for every quad-path
// plan (N = 1..10 with and without robot_visible: the staged values end at most at o_lines + 19,200, region 2
// starts at o_lines + 19,712); cn_create refuses an engine whose plan breaks it.
__host__ __device__ inline bool cn_goal_early_ok(const StepPlan &p)
{
    const int lo = p.o_lines + 2 * p.rng_stride, hi = p.o_lines + 4 * p.rng_stride;
    return !p.kd && p.rng_waves == 4 && (p.o_hst + 7 * p.H * 8 <= lo || p.o_hst >= hi);
}

// kernel-A LDS views
struct SL {
    int T;            // lane stride of the per-lane arrays
    double *r;        // [CN_RENV_F][EPB]
    float *act;       // [2][EPB] clipped action (holonomic vx,vy / unicycle v,r)
    uint32_t *rflag;  // [EPB] flags ; [EPB] aux ; [EPB] humans the reward loop visited (first collision + 1)
    uint32_t *app;    // [EPB][2] multi-step launches: the env's spawn-list entry of each key parity (index + 1; 0: none)
    double *rvr;      // [8][EPB] robot VelocityRectangle corners
    double *hvr;      // [8][H] human VelocityRectangle corners (x0..x3, y0..y3)
    double *hst;      // [7][H] human_post's results (vx, vy, belief px, py, vx, vy, r), stored after phase 2
    double *h;        // [CN_HUM_F][T]
    double *cd;       // [T]
    uint32_t *lf;     // [T]
    float *orad;      // [T]
    uint32_t *vis;    // [H] visible-now mask of the human's observed slots (quad path)
    uint32_t *dm;     // [H] dummy-at-creation mask
    float *vmax;      // [H] frozen RVO2 max speed
    double *npx, *npy; // [H] each: post-move human positions (the phase-5 goal changes read them)
    uint32_t *eg;     // [H] goal reached (LF_ENDGOAL) / non-finite position (bit 31) after the move
    float4 *lines;    // [M][T]  (kd-tree path)
    float4 *proj;     // [M][T]  linearProgram3's projected lines (kd-tree path)
    float *nd;        // [M][T]
    uint8_t *ns;      // [M][T]
    uint8_t *perm;    // [A][T]
};
enum { R_PX, R_PY, R_GX, R_GY, R_VX, R_VY, R_TH, R_RAD, R_VP, R_POT, R_GT, R_DV, R_NX, R_NY, R_LAX, R_LAY, R_EPR,
       // robot terms of calc_reward / kinematics computed early (phase 1), applied in phase 3
       R_CVX, R_CVY, R_NTH, R_JERK, R_D2G, R_SPD, R_SL, R_SR, R_SEP, R_BITS };
enum { H_PX, H_PY, H_GX, H_GY, H_VX, H_VY, H_R, H_VP, H_TH, H_BPX, H_BPY, H_BVX, H_BVY, H_BR };
#define RF(sl, f, el, EPB) ((sl).r[(f) * (EPB) + (el)])
#define HF(sl, f, t) ((sl).h[(f) * (sl).T + (t)])

// lane flag bits
#define LF_VR 1u
#define LF_NOTREACHED 2u
#define LF_ENDGOAL 4u
