// robot.h -- the scripted robot's device functions (robot_* controllers), the rollouts' noise and recorded rows
// (state_row*, visible_mask_*). Needs plan.h, geometry.h, orca_lp.h and spawn.h (OutView).
#pragma once

// ------------------------------------------------------------------------------------------------
// the scripted robot's device functions (cn_robot_act's kernels below; cn_step_kernel's rollout variant)
// ------------------------------------------------------------------------------------------------
// Agent j of the robot's RVO2 simulator in float32 as ORCA._frame casts it (orca.py:91-115): j = 0 the robot,
// j >= 1 the belief of human j - 1; radius (float)((radius + 0.01) + safety_space).
__device__ __forceinline__ void robot_sim_agent(const cn_state_ptrs &S, double safety, int64_t e, int N, int j,
                                                float &x, float &y, float &vx, float &vy, float &r)
{
    if (j == 0) {
        x = (float)S.r_px[e]; y = (float)S.r_py[e]; vx = (float)S.r_vx[e]; vy = (float)S.r_vy[e];
        r = (float)((S.r_radius[e] + 0.01) + safety);
    } else {
        const int64_t h = e * N + (j - 1);
        x = (float)S.b_px[h]; y = (float)S.b_py[h]; vx = (float)S.b_vx[h]; vy = (float)S.b_vy[h];
        r = (float)((S.b_r[h] + 0.01) + safety);
    }
}

// maxSpeed and the preferred velocity (orca.py:118-122): float64 towards the goal, normalised only above
// speed 1 (np.linalg.norm), then float32
__device__ __forceinline__ void robot_pref_velocity(const cn_state_ptrs &S, int64_t e, float &vmax, float &ox, float &oy)
{
    const double vx = S.r_gx[e] - S.r_px[e], vy = S.r_gy[e] - S.r_py[e];
    const double speed = np_norm2(vx, vy);
    vmax = (float)S.r_vpref[e];
    if (speed > 1) { ox = (float)ddiv(vx, speed); oy = (float)ddiv(vy, speed); }
    else { ox = (float)vx; oy = (float)vy; }
}

// The unicycle robot's tracking law (this project's definition: the reference has no scripted unicycle robot).
// From a controller's ActionXY (ux, uy) -- the float32 pair the holonomic path writes -- and env e's heading
// theta = r_theta and speed v = r_dv, the (dv, dtheta) action cn_step takes on a unicycle engine: turn towards the
// velocity's direction by at most 0.1, and move the speed by at most 0.1 towards the velocity's projection on the
// heading the step will then have, never backwards. The limits are phase 0's clip of the action, which is therefore
// a no-op on the result. Float64, no contraction, one rounding to float32. One lane per env.
// Shared by cn_robot_act's kernels and cn_step_kernel's rollout variant: one arithmetic, bit for bit.
__device__ __forceinline__ void robot_unicycle_track(const cn_state_ptrs &S, int64_t e, float ux, float uy, float &a0,
                                                     float &a1)
{
    const double theta = S.r_theta[e], v = S.r_dv[e];
    const double s = np_norm2((double)ux, (double)uy);
    double turn = 0.0, target = 0.0;
    if (s != 0.0) {
        const double delta = remainder(atan2((double)uy, (double)ux) - theta, 2 * CN_PI);   // IEEE: in [-pi, pi]
        turn = delta < -0.1 ? -0.1 : (delta > 0.1 ? 0.1 : delta);
        const double along = cos(delta - turn);
        target = s * (along > 0.0 ? along : 0.0);
    }
    const double dv = target - v;
    a0 = (float)(dv < -0.1 ? -0.1 : (dv > 0.1 ? 0.1 : dv));
    a1 = (float)turn;
}

// The two halves of ORCA.predict on the quad path (N + 1 <= 10 agents), quad-cooperative, with a wave-level LDS
// ordering point (wsync) between them at the caller: the ORCA lines of env e's robot into Lq [<= 9] (returns
// their number), then RVO2's linear programs on them. Every lane of the quad gets the new velocity.
// Shared by cn_robot_orca_kernel and cn_step_kernel's rollout variant: one arithmetic, bit for bit.
__device__ __forceinline__ int robot_orca_lines(const cn_state_ptrs &S, double safety, int64_t e, int N, int sq, float nd,
                                                float th, float ts, float4 *Lq)
{
    float X0, Y0, VX0, VY0, R0;
    robot_sim_agent(S, safety, e, N, 0, X0, Y0, VX0, VY0, R0);
    return orca_lines_quad(
        [&](int k, float &x, float &y, float &vx, float &vy, float &r) {
            robot_sim_agent(S, safety, e, N, k + 1, x, y, vx, vy, r);
        },
        N, sq, X0, Y0, VX0, VY0, R0, nd * nd, fdiv(1.0f, th), fdiv(1.0f, ts), Lq);
}

__device__ __forceinline__ void robot_orca_solve(const cn_state_ptrs &S, int64_t e, int cnt, int sq, float4 *Lq, float &rx,
                                                 float &ry)
{
    float vmax, ox, oy;
    robot_pref_velocity(S, e, vmax, ox, oy);
    float4 R[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) R[u] = sq + 4 * u < cnt ? Lq[sq + 4 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int fail_at = lp2_r<3>(R, cnt, vmax, ox, oy, sq, rx, ry);
    if (fail_at < cnt) lp3_r<3>(R, Lq, cnt, fail_at, vmax, sq, rx, ry);
}

// SOCIAL_FORCE.predict (social_force.py:11-66) of env e's robot on its FullState and the N belief humans:
// cn_sf_predict_kernel's float64 arithmetic up to the new velocity (nx, ny), its norm nn and the robot's v_pref;
// the caller clips to v_pref and rounds the ActionXY to float32 (as cn_robot_sf_kernel does). One lane per env.
__device__ __forceinline__ void robot_sf_velocity(const cn_state_ptrs &S, int64_t e, int N, double A, double B, double KI,
                                                  double dt, double &nx, double &ny, double &nn, double &vpref)
{
    const double px = S.r_px[e], py = S.r_py[e], vx0 = S.r_vx[e], vy0 = S.r_vy[e], rad = S.r_radius[e];
    vpref = S.r_vpref[e];
    const double gdx = S.r_gx[e] - px, gdy = S.r_gy[e] - py;
    const double dg = dsqrt(gdx * gdx + gdy * gdy);
    const double dvx = ddiv(gdx, dg) * vpref, dvy = ddiv(gdy, dg) * vpref;
    const double cdx = KI * (dvx - vx0), cdy = KI * (dvy - vy0);
    double ix = 0.0, iy = 0.0;
    for (int k = 0; k < N; ++k) {
        const int64_t h = e * N + k;
        const double ddx = px - S.b_px[h], ddy = py - S.b_py[h];
        const double d = dsqrt(ddx * ddx + ddy * ddy);
        const double ex = exp(ddiv(rad + S.b_r[h] - d, B));
        ix += A * ex * ddiv(ddx, d);
        iy += A * ex * ddiv(ddy, d);
    }
    nx = vx0 + (cdx + ix) * dt; ny = vy0 + (cdy + iy) * dt;
    nn = np_norm2(nx, ny);
}

// cn_rollout_noisy: the executed action x = a + sigma * n of env G (global index) at step k of the caller's noise
// sequence, n uniform in [-1, 1) from the words x, y of philox(counter k, key (seed, G)). (w >> 8) * 2^-24 and
// 2 u - 1 are exact in float32; the product and the sum round once each (no contraction). One lane per env.
// Shared by cn_action_noise_kernel and cn_step_kernel's rollout variant: one arithmetic, bit for bit.
__device__ __forceinline__ void rollout_noise(float sigma, uint32_t seed, uint32_t k, uint32_t G, float ax, float ay,
                                              float &x0, float &x1)
{
    const uint4 w = philox4x32_10(k, seed, G);
    const float n0 = __fsub_rn(__fmul_rn(2.0f, __fmul_rn((float)(w.x >> 8), 0x1p-24f)), 1.0f);
    const float n1 = __fsub_rn(__fmul_rn(2.0f, __fmul_rn((float)(w.y >> 8), 0x1p-24f)), 1.0f);
    x0 = __fadd_rn(ax, __fmul_rn(sigma, n0));
    x1 = __fadd_rn(ay, __fmul_rn(sigma, n1));
}

// The engine's device block of a cn_rollout_noisy call (behind the control words: cn_engine::work_count + CN_NOISE_W,
// reached in the kernel from PendLaunch::stats), written on the stream before the call's fused launches.
// `executed` (or null) and `actions` are the call's row 0: a launch's row of `executed` lies where its row of
// `actions` lies.
struct RolloutNoise {
    float sigma;
    uint32_t seed;
    float *executed;
    const float *actions;
};
#define CN_NOISE_W 16   // in uint32 words from work_count (PendLaunch::stats = work_count + 8)
// StepArgs::rollout of a perturbed launch: CN_ROLLOUT_NOISY, and (uint32)k of the launch's first step above it (the
// word stays >= 0, which is how step_launch tells a rollout launch)
#define CN_ROLLOUT_NOISY (1ll << 16)
#define CN_ROLLOUT_K_SHIFT 17

// The engine's device block of a cn_rollout_lidar call (behind the RolloutNoise block: work_count + CN_ROWS_W),
// written on the stream before the call's fused launches. The state rows are field-major over the call's `rows`
// steps: robot_state [9][rows][E] (r_px, r_py, r_vx, r_vy, r_radius, r_gx, r_gy, r_vpref, r_theta), human_state
// [3][rows][E][N] (h_px, h_py, h_r) -- the twelve fields cn_lidar_scan_kernel reads, so a cn_state_ptrs aimed into
// them makes the scan run over rows * E "envs". `actions` is the call's row 0: a launch finds its row from its own.
struct RolloutRows {
    double *robot_state;
    double *human_state;
    const float *actions;
    int64_t rows;
};
#define CN_ROWS_W 22   // in uint32 words from work_count
// A group of a mixed engine: the envs of the whole engine, i.e. the rows of one step in the (T, E, ..) buffers of a
// rollout launch (word CN_ER_W of the group's work_count, behind the RolloutRows block; written once by
// cn_create_mixed). A plain engine's rows are its own E and the word is not read.
#define CN_ER_W 30

// field f of the state rows: its array in the blob
__device__ __forceinline__ const double *state_row_robot_field(const cn_state_ptrs &S, int f)
{
    switch (f) {
    case 0: return S.r_px;
    case 1: return S.r_py;
    case 2: return S.r_vx;
    case 3: return S.r_vy;
    case 4: return S.r_radius;
    case 5: return S.r_gx;
    case 6: return S.r_gy;
    case 7: return S.r_vpref;
    default: return S.r_theta;
    }
}
__device__ __forceinline__ const double *state_row_human_field(const cn_state_ptrs &S, int f)
{
    return f == 0 ? S.h_px : (f == 1 ? S.h_py : S.h_r);
}

// The blob's twelve fields of envs [e0, e0 + ne) copied to row `row_e / E` of the state rows (bits, no arithmetic), by
// thread k of nthr. Shared by cn_state_rows_kernel and cn_step_kernel's recording rollout variant.
__device__ __forceinline__ void state_rows_copy(const cn_state_ptrs &S, const RolloutRows &R, int64_t E, int N,
                                                int64_t row_e, int e0, int ne, int k, int nthr)
{
    const int64_t RE = R.rows * E, d0 = row_e + e0;   // row_e: the row's first env, row * E
#pragma unroll
    for (int f = 0; f < 9; ++f) {
        const double *const src = state_row_robot_field(S, f) + e0;
        double *const dst = R.robot_state + (f * RE + d0);
        for (int q = k; q < ne; q += nthr) dst[q] = src[q];
    }
    const int nh = ne * N;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const double *const src = state_row_human_field(S, f) + (int64_t)e0 * N;
        double *const dst = R.human_state + (f * RE + d0) * N;
        for (int q = k; q < nh; q += nthr) dst[q] = src[q];
    }
}

// cn_visible_mask's decision for slot k of env e (k >= N: a padded slot, 0): the step's own FOV test on the blob's
// r_px, r_py, r_vx, r_vy, r_theta, flags, h_px, h_py (aux_kernels.h: cn_visible_mask_kernel). Shared by that kernel
// and cn_step_kernel's mask-recording rollout variant: one arithmetic, so the rows are the same by construction.
// Reads no other lane.
__device__ __forceinline__ float visible_mask_slot(const cn_state_ptrs &S, int64_t e, int k, int N, int holo, double fov,
                                                   double cth)
{
    int rv = 0;
    if (k < N) {
        const int64_t h = e * N + k;
        const double rpx = S.r_px[e], rpy = S.r_py[e], px = S.h_px[h], py = S.h_py[h];
        const bool full = fov >= 2.0 * CN_PI;
        if (S.flags[e] & CN_FLAG_ROBOT_F32) {
            const float rvx = (float)S.r_vx[e], rvy = (float)S.r_vy[e];
            const float rth = holo ? 0.0f : (float)S.r_theta[e];
            const bool rfin = holo ? (rvx == rvx && rvy == rvy) : isfinite(rth);
            rv = full ? vis360(rfin, rpx, rpy, px, py) : -1;
            if (rv < 0) {
                double fx, fy;
                if (holo) fov_dir32(atan2f(rvy, rvx), fx, fy);
                else fov_dir32(rth, fx, fy);
                rv = in_fov_fast(fx, fy, rpx, rpy, px, py, fov, cth) ? 1 : 0;
            }
        } else {
            const double th0 = holo ? 0.0 : S.r_theta[e];
            rv = full ? vis360(isfinite(th0), rpx, rpy, px, py) : -1;
            if (rv < 0) rv = reset_fov_test(th0, rpx, rpy, px, py, fov);
        }
    }
    return rv ? 1.0f : 0.0f;
}

// The mask rows of envs [e0, e0 + ne) of a step workgroup into `row` (one step's [ER][NS] rows of the caller's
// buffer; the envs at orow(ov, e)), one (env, slot) per pass of thread k of nthr.
__device__ __forceinline__ void visible_mask_rows(const cn_state_ptrs &S, const OutView &ov, int e0, int ne, int N,
                                                  int holo, double fov, double cth, float *__restrict__ row, int k,
                                                  int nthr)
{
    const int NS = ov.NS, n = ne * NS;
    for (int q = k; q < n; q += nthr) {
        const int el = q / NS, s = q - el * NS;
        const int64_t e = e0 + el;
        row[orow(ov, e) * NS + s] = visible_mask_slot(S, e, s, N, holo, fov, cth);
    }
}
