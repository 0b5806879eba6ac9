// lidar.h -- the two LiDAR kernels of the ConvGRU observation: the scan as the reference ships it (taken at
// reset only, cn_lidar_obs) and the live per-step scan (cn_lidar_scan). Reference: crowd_sim_dict.py:96-101,
// 174-191, 224-251; crowd_sim/envs/utils/lidarv2.py. Part of cn_engine.hip's translation unit: included there
// after the device core (cn_state_ptrs, cn_math.h's float64 helpers).
#pragma once

// ------------------------------------------------------------------------------------------------
// LiDAR observation of the ConvGRU policy: CrowdSimDict.generate_ob's 'convgru' branch
// (crowd_sim_dict.py:96-101) over LidarSensor.sensor_spin (crowd_sim/envs/utils/lidarv2.py:398-427).
// As shipped, the reference computes the scan only inside reset() (crowd_sim_dict.py:174-191, robot
// heading atan2(0, 0) = 0, and only the LAST human is parsed: the append sits outside the loop), AFTER the
// reset observation was built (:166), and step() never refreshes lidar_rel_dist. So the observation that
// reset() returns carries the previous scan (zeros before the first), and every step of the episode
// carries the scan taken at its reset. One 64-lane wave per env, three beams per lane, float64 as the
// reference; the observation row is
//   [clip(robot (px, py, r, gx, gy, v_pref, theta) / max_range, 0, 1), |1 - clip(dist / max_range, 0, 1)|].
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double np_rem(double a, double b)   // numpy float remainder (sign of divisor)
{
    double m = fmod(a, b);
    if (m != 0.0) { if ((b < 0) != (m < 0)) m += b; }
    else m = copysign(0.0, b);
    return m;
}
__device__ __forceinline__ double rescale_angle(double t) { return np_rem(t + 2.0 * CN_PI, 2.0 * CN_PI); }

__device__ __forceinline__ int seg_orient(double px, double py, double qx, double qy, double rx, double ry)
{   // get_intersect.py:25-37
    const double v = ((qy - py) * (rx - qx)) - ((qx - px) * (ry - qy));
    return v > 0 ? 1 : (v < 0 ? 2 : 0);
}
__device__ __forceinline__ bool on_seg(double px, double py, double qx, double qy, double rx, double ry)
{   // get_intersect.py:12-21
    return qx <= fmax(px, rx) && qx >= fmin(px, rx) && qy <= fmax(py, ry) && qy >= fmin(py, ry);
}

__global__ void __launch_bounds__(256) cn_lidar_obs_kernel(cn_state_ptrs S, int E, int N, double half_world,
                                                           const uint8_t *__restrict__ reset_mask, int enable,
                                                           int beams, double max_range, double robot_r,
                                                           float *__restrict__ lidar, float *__restrict__ obs)
{
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= E) return;
    const int D = 7 + beams;
    float *o = obs + (int64_t)e * D;
    if (lane < 7) {
        double v;
        switch (lane) {
        case 0: v = S.r_px[e]; break;
        case 1: v = S.r_py[e]; break;
        case 2: v = S.r_radius[e]; break;
        case 3: v = S.r_gx[e]; break;
        case 4: v = S.r_gy[e]; break;
        case 5: v = S.r_vpref[e]; break;
        default: v = S.r_theta[e]; break;
        }
        v = v / max_range;
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);   // np.clip
        o[lane] = (float)v;
    }
    float *L = lidar + (int64_t)e * beams;
    const bool fresh = reset_mask == nullptr || reset_mask[e] != 0;
    if (fresh) {
        if (enable) {
            const double sx = S.r_px[e], sy = S.r_py[e];
            const int hl = e * N + (N - 1);                 // the last human only (see above)
            const double hx = S.h_px[hl], hy = S.h_py[hl], hr = S.h_r[hl];
            // get_valid_angles (lidarv2.py:17-52) for the one obstacle, sorted (min, max)
            const double rlx = hx - sx, rly = hy - sy;
            const double hd = rescale_angle(atan2(rly, rlx));
            const double ddx = hr * sin(hd), ddy = hr * cos(hd);
            const double m0 = rescale_angle(atan2(rly - ddy, rlx + ddx));
            const double m1 = rescale_angle(atan2(rly + ddy, rlx - ddx));
            const double lo0 = m0 < m1 ? m0 : m1, up0 = m0 < m1 ? m1 : m0;
            const double bstep = (2.0 * CN_PI) / (double)(beams - 1);   // np.linspace(0, 2 pi, beams)
            const int npts = 500;                                         // max_range / 0.01 samples (+ endpoint)
            const double sstep = max_range / (double)(npts - 1);
            for (int b = lane; b < beams; b += 64) {
                const double th0 = (b == beams - 1) ? 2.0 * CN_PI : (double)b * bstep;
                const double th = rescale_angle(th0 + 0.0);
                // get_valid_angle_idx (lidarv2.py:55-75) mutates the caller's (min, max) arrays in place and
                // they are reused for every beam: replay the mutation sequence up to this beam
                double lo = lo0, up = up0, tt = th;
                for (int q = 0; q <= b; ++q) {
                    const bool wide = up - lo >= CN_PI;
                    double tq = th;
                    if (wide) { const double nu = up - 2.0 * CN_PI; up = lo; lo = nu; tq -= 2.0 * CN_PI; }
                    if (q == b) tt = tq;
                }
                const bool valid = np_rem(tt - lo, 2.0 * CN_PI) < np_rem(up - lo, 2.0 * CN_PI);
                const double c = cos(th), sn = sin(th);
                double ex = c * max_range + sx, ey = sn * max_range + sy;   // beam_end
                bool hit = false;
                if (valid) {   // check_dist_collision_polygon (lidarv2.py:164-198): first sample inside the disc
                    const double wx = hx - sx, wy = hy - sy;
                    const double proj = wx * c + wy * sn, perp2 = wx * wx + wy * wy - proj * proj;
                    const double r2 = hr * hr;
                    if (perp2 <= r2 * (1.0 + 1e-9) + 1e-12) {
                        const double hw = sqrt(fmax(r2 - perp2, 0.0));
                        const double s_in = proj - hw, s_out = proj + hw;
                        int k0 = (int)floor(s_in / sstep) - 2, k1 = (int)ceil(s_out / sstep) + 2;
                        k0 = k0 < 0 ? 0 : k0;
                        k1 = k1 > npts - 1 ? npts - 1 : k1;
                        for (int k = k0; k <= k1 && !hit; ++k) {
                            const double sk = (k == npts - 1) ? max_range : (double)k * sstep;
                            const double bx = c * sk + sx, by = sn * sk + sy;
                            const double ax = hx - bx, ay = hy - by;
                            if (sqrt(ax * ax + ay * ay) < hr) { ex = bx; ey = by; hit = true; }
                        }
                    }
                }
                if (!hit) {    // walls (lidarv2.py:261-275): first intersecting wall, kept if within range
                    const double t = half_world;
                    const double wxs[5] = {-t, t, t, -t, -t}, wys[5] = {-t, -t, t, t, -t};
                    const double p1x = sx, p1y = sy, q1x = ex, q1y = ey;
                    for (int j = 0; j < 4; ++j) {
                        const double p2x = wxs[j], p2y = wys[j], q2x = wxs[j + 1], q2y = wys[j + 1];
                        const int o1 = seg_orient(p1x, p1y, q1x, q1y, p2x, p2y);
                        const int o2 = seg_orient(p1x, p1y, q1x, q1y, q2x, q2y);
                        const int o3 = seg_orient(p2x, p2y, q2x, q2y, p1x, p1y);
                        const int o4 = seg_orient(p2x, p2y, q2x, q2y, q1x, q1y);
                        const bool inter = (o1 != o2 && o3 != o4) || (o1 == 0 && on_seg(p1x, p1y, p2x, p2y, q1x, q1y)) ||
                                           (o2 == 0 && on_seg(p1x, p1y, q2x, q2y, q1x, q1y)) ||
                                           (o3 == 0 && on_seg(p2x, p2y, p1x, p1y, q2x, q2y)) ||
                                           (o4 == 0 && on_seg(p2x, p2y, q1x, q1y, q2x, q2y));
                        if (!inter) continue;
                        // line_intersection (get_intersect.py:72-89)
                        const double xd0 = p1x - q1x, xd1 = p2x - q2x, yd0 = p1y - q1y, yd1 = p2y - q2y;
                        const double div = xd0 * yd1 - xd1 * yd0;
                        if (div != 0.0) {
                            const double d0 = p1x * q1y - p1y * q1x, d1 = p2x * q2y - p2y * q2x;
                            const double ix = (d0 * xd1 - d1 * xd0) / div, iy = (d0 * yd1 - d1 * yd0) / div;
                            if (np_norm2(ix - sx, iy - sy) <= max_range) { ex = ix; ey = iy; }
                        }
                        break;
                    }
                }
                if (np_norm2(ex - sx, ey - sy) < robot_r) {   // beams cannot end inside the robot
                    ex = sx + robot_r * cos(th);
                    ey = sy + robot_r * sin(th);
                }
                const double rx = ex - sx, ry = ey - sy;
                double rd = sqrt(rx * rx + ry * ry) / max_range;
                rd = rd < 0.0 ? 0.0 : (rd > 1.0 ? 1.0 : rd);
                o[7 + b] = L[b];                 // the reset observation keeps the previous scan
                L[b] = (float)fabs(1.0 - rd);
            }
            return;
        }
        for (int b = lane; b < beams; b += 64) { o[7 + b] = L[b]; L[b] = 0.0f; }
        return;
    }
    for (int b = lane; b < beams; b += 64) o[7 + b] = L[b];
}

// ------------------------------------------------------------------------------------------------
// Live LiDAR scan (cn_lidar_scan): the scan CrowdSimDict.step() computes every step and then discards
// (crowd_sim_dict.py:224-251) — LidarSensor.sensor_spin at the robot's position, heading atan2(vy, vx),
// against ALL humans (index order) and the world walls — written into the observation row of the current
// state. float64 like the reference. One workgroup serves G consecutive envs (G chosen by the host so that
// G * beams fills the 256 lanes): phase 1 stages every obstacle of the G envs in LDS once (centre, radius,
// centre distance, angular window), phase 2 spreads the G * beams beams flat over the lanes, so neither a
// small N nor a beam count off a multiple of 64 idles lanes.
//
// get_valid_angle_idx (lidarv2.py:55-75) flips a window that is at least pi wide IN PLACE, and the flipped
// window serves every later beam. The flips do not depend on the beam, so phase 1 runs each obstacle's flip
// sequence once: nflip flips until the window is narrower than pi (0 or 1 but for a window of exactly pi,
// which flips back and forth: capped at the beam count). Beam b >= nflip sees the settled window and its own
// angle; beam b < nflip replays b + 1 flips and tests its angle - 2 pi, as the reference does on a flip.
// ------------------------------------------------------------------------------------------------
#define CN_LIDAR_G 8   // envs per workgroup at most (LDS: 8 * 31 obstacles * 80 B = 19.4 KB)

struct LidarObst {
    double x, y, r, dist;     // centre, radius, |centre - sensor| (np.linalg.norm(axis=1): no fused multiply-add)
    double lo, up, width;     // the settled window and np.remainder(up - lo, 2 pi)
    double lo0, up0;          // the window before any flip
    int nflip, pad;
};

// fmod(a, 2 pi) for |a| < 8 pi by exact subtractions (Sterbenz: x - b is exact for b <= x <= 2 b), then
// numpy's sign rule: np.remainder(a, 2 pi). Falls back to fmod outside that range.
__device__ __forceinline__ double np_rem_2pi(double a)
{
    const double b = 2.0 * CN_PI;
    double x = fabs(a);
    if (!(x < 4.0 * b)) return np_rem(a, b);
    if (x >= 2.0 * b) x -= 2.0 * b;
    if (x >= b) x -= b;
    if (x == 0.0) return 0.0;
    return a < 0.0 ? b - x : x;     // fmod keeps the sign of a; numpy then adds b: -x + b
}

__global__ void __launch_bounds__(256) cn_lidar_scan_kernel(cn_state_ptrs S, int E, int N, int G, double half_world,
                                                            int beams, int npts, double max_range, double robot_r,
                                                            float *__restrict__ obs)
{
    __shared__ LidarObst ob[CN_LIDAR_G * 31];
    __shared__ double hd[CN_LIDAR_G][3];     // sensor x, y, heading
    const int tid = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = min(G, E - e0);
    const int D = 7 + beams;
    const double TWO_PI = 2.0 * CN_PI;

    for (int t = tid; t < ne * 7; t += 256) {          // the robot part of the row
        const int e = e0 + t / 7, f = t % 7;
        double v;
        switch (f) {
        case 0: v = S.r_px[e]; break;
        case 1: v = S.r_py[e]; break;
        case 2: v = S.r_radius[e]; break;
        case 3: v = S.r_gx[e]; break;
        case 4: v = S.r_gy[e]; break;
        case 5: v = S.r_vpref[e]; break;
        default: v = S.r_theta[e]; break;
        }
        v = v / max_range;
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);   // np.clip
        obs[(int64_t)e * D + f] = (float)v;
    }
    if (tid < ne) {
        const int e = e0 + tid;
        hd[tid][0] = S.r_px[e];
        hd[tid][1] = S.r_py[e];
        // float64 arctangent. (While the robot's velocity holds np.float32 values the reference's np.arctan2 is
        // a float32 one, whose last ulp depends on the host's SIMD math library: within 1.2e-7 rad of this.)
        hd[tid][2] = atan2(S.r_vy[e], S.r_vx[e]);
    }
    for (int t = tid; t < ne * N; t += 256) {          // phase 1: obstacles -> LDS
        const int le = t / N, i = t % N, e = e0 + le;
        const double sx = S.r_px[e], sy = S.r_py[e];
        const int hi = e * N + i;
        LidarObst o;
        o.x = S.h_px[hi]; o.y = S.h_py[hi]; o.r = S.h_r[hi];
        // get_valid_angles (lidarv2.py:17-52): sorted (min, max)
        const double rlx = o.x - sx, rly = o.y - sy;
        o.dist = sqrt(rlx * rlx + rly * rly);
        const double ha = rescale_angle(atan2(rly, rlx));
        const double ddx = o.r * sin(ha), ddy = o.r * cos(ha);
        const double m0 = rescale_angle(atan2(rly - ddy, rlx + ddx));
        const double m1 = rescale_angle(atan2(rly + ddy, rlx - ddx));
        o.lo0 = m0 < m1 ? m0 : m1;
        o.up0 = m0 < m1 ? m1 : m0;
        double lo = o.lo0, up = o.up0;
        int nf = 0;
        while (up - lo >= CN_PI && nf < beams) { const double nu = up - TWO_PI; up = lo; lo = nu; ++nf; }
        o.lo = lo; o.up = up; o.nflip = nf; o.pad = 0;
        o.width = np_rem(up - lo, TWO_PI);
        ob[t] = o;
    }
    __syncthreads();

    const double bstep = TWO_PI / (double)(beams - 1);          // np.linspace(0, 2 pi, beams)
    const double sstep = max_range / (double)(npts - 1);        // np.linspace(0, max_range, npts)
    for (int item = tid; item < ne * beams; item += 256) {      // phase 2: one beam per lane
        const int le = item / beams, b = item - le * beams, e = e0 + le;
        const double sx = hd[le][0], sy = hd[le][1];
        const double th0 = (b == beams - 1) ? TWO_PI : (double)b * bstep;
        const double th = rescale_angle(th0 + hd[le][2]);
        const double c = cos(th), sn = sin(th);
        // the obstacle with the nearest centre among those whose window holds the beam (first on ties)
        const LidarObst *O = ob + le * N;
        int best = -1;
        double bestd = 0.0;
        for (int i = 0; i < N; ++i) {
            double lo = O[i].lo, up = O[i].up, tt = th, width = O[i].width;
            if (b < O[i].nflip) {
                lo = O[i].lo0; up = O[i].up0;
                for (int q = 0; q <= b; ++q) { const double nu = up - TWO_PI; up = lo; lo = nu; }
                tt = th - TWO_PI;
                width = np_rem(up - lo, TWO_PI);
            }
            const bool valid = np_rem_2pi(tt - lo) < width;
            const double d = O[i].dist;
            if (valid && (best < 0 || d < bestd)) { best = i; bestd = d; }
        }
        double ex = c * max_range + sx, ey = sn * max_range + sy;   // beam_end
        bool hit = false;
        if (best >= 0) {   // check_dist_collision_polygon (lidarv2.py:164-198): first sample inside the disc,
                           // searched in a window around the analytic entry point
            const double hx = O[best].x, hy = O[best].y, hr = O[best].r;
            const double wx = hx - sx, wy = hy - sy;
            const double proj = wx * c + wy * sn, perp2 = wx * wx + wy * wy - proj * proj;
            const double r2 = hr * hr;
            if (perp2 <= r2 * (1.0 + 1e-9) + 1e-12) {
                const double hw = sqrt(fmax(r2 - perp2, 0.0));
                const double k_in = floor((proj - hw) / sstep) - 2.0, k_out = ceil((proj + hw) / sstep) + 2.0;
                const int k0 = k_in > 0.0 ? (k_in < (double)npts ? (int)k_in : npts) : 0;
                const int k1 = k_out < (double)(npts - 1) ? (k_out > -1.0 ? (int)k_out : -1) : npts - 1;
                for (int k = k0; k <= k1 && !hit; ++k) {
                    const double sk = (k == npts - 1) ? max_range : (double)k * sstep;
                    const double bx = c * sk + sx, by = sn * sk + sy;
                    const double ax = hx - bx, ay = hy - by;
                    if (sqrt(ax * ax + ay * ay) < hr) { ex = bx; ey = by; hit = true; }
                }
            }
        }
        if (!hit) {    // walls (lidarv2.py:261-275): first intersecting wall, kept if within range
            const double t = half_world;
            const double wxs[5] = {-t, t, t, -t, -t}, wys[5] = {-t, -t, t, t, -t};
            const double p1x = sx, p1y = sy, q1x = ex, q1y = ey;
            for (int j = 0; j < 4; ++j) {
                const double p2x = wxs[j], p2y = wys[j], q2x = wxs[j + 1], q2y = wys[j + 1];
                const int o1 = seg_orient(p1x, p1y, q1x, q1y, p2x, p2y);
                const int o2 = seg_orient(p1x, p1y, q1x, q1y, q2x, q2y);
                const int o3 = seg_orient(p2x, p2y, q2x, q2y, p1x, p1y);
                const int o4 = seg_orient(p2x, p2y, q2x, q2y, q1x, q1y);
                const bool inter = (o1 != o2 && o3 != o4) || (o1 == 0 && on_seg(p1x, p1y, p2x, p2y, q1x, q1y)) ||
                                   (o2 == 0 && on_seg(p1x, p1y, q2x, q2y, q1x, q1y)) ||
                                   (o3 == 0 && on_seg(p2x, p2y, p1x, p1y, q2x, q2y)) ||
                                   (o4 == 0 && on_seg(p2x, p2y, q1x, q1y, q2x, q2y));
                if (!inter) continue;
                // line_intersection (get_intersect.py:72-89)
                const double xd0 = p1x - q1x, xd1 = p2x - q2x, yd0 = p1y - q1y, yd1 = p2y - q2y;
                const double div = xd0 * yd1 - xd1 * yd0;
                if (div != 0.0) {
                    const double d0 = p1x * q1y - p1y * q1x, d1 = p2x * q2y - p2y * q2x;
                    const double ix = (d0 * xd1 - d1 * xd0) / div, iy = (d0 * yd1 - d1 * yd0) / div;
                    if (np_norm2(ix - sx, iy - sy) <= max_range) { ex = ix; ey = iy; }
                }
                break;
            }
        }
        if (np_norm2(ex - sx, ey - sy) < robot_r) {   // beams cannot end inside the robot
            ex = sx + robot_r * c;
            ey = sy + robot_r * sn;
        }
        const double rx = ex - sx, ry = ey - sy;
        double rd = sqrt(rx * rx + ry * ry) / max_range;
        rd = rd < 0.0 ? 0.0 : (rd > 1.0 ? 1.0 : rd);
        obs[(int64_t)e * D + 7 + b] = (float)fabs(1.0 - rd);
    }
}
