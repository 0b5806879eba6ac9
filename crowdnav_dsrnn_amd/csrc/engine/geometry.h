// geometry.h -- FOV tests, velocity rectangles and their intersection, the world box, the social-norm zones and
// the disc-quad SAT family (robot_norm_zone_*). Needs cn_math.h and quad.h (quad_or).
#pragma once

// ------------------------------------------------------------------------------------------------
// FOV (CrowdSim.detect_visible, crowd_sim.py:820-847)
// With fov >= 2*pi (the reference default, FOV = 2) the arccos test always passes: an agent is visible
// iff the normalised dot product is not NaN. Away from under/overflow of |v|^2 that is "heading finite
// and the agents not coincident", decided without atan2/cos/sin/sqrt/division; `vis360` returns -1
// where the full computation must decide (|v|^2 outside [1e-300, 1e300]).
// ------------------------------------------------------------------------------------------------
// unit FOV direction of an agent with float64 heading
__device__ inline void fov_dir64(double th, double &fx, double &fy)
{
    fx = cos(th); fy = sin(th);
    const double nf = np_norm2(fx, fy);
    fx = ddiv(fx, nf); fy = ddiv(fy, nf);
}
// float32 heading (np.float32 robot state): float32 cos/sin/norm, promoted for the dot
__device__ inline void fov_dir32(float th, double &fx, double &fy)
{
    float cx = np_cosf(th), cy = np_sinf(th);
    const float nf = np_norm2f(cx, cy);
    fx = (double)fdiv(cx, nf); fy = (double)fdiv(cy, nf);
}
__device__ __forceinline__ int vis360(bool heading_finite, double px1, double py1, double px2, double py2)
{
    if (!heading_finite) return 0;
    const double dx = px2 - px1, dy = py2 - py1;
    const double n2 = __fma_rn(dy, dy, dx * dx);
    return (n2 > 1e-300 && n2 < 1e300) ? 1 : -1;
}
// arccos(d) <= fov / 2, the reference's test, out of line: only cosines within the band below reach it
__device__ __noinline__ bool acos_within(double d, double fov) { return fabs(acos(d)) <= fov / 2; }
// `cth` = cos(fov / 2) (any accurate evaluation): arccos is decreasing with |d arccos / dd| >= 1, so for
// |d - cth| > 1e-12 the arccos of d is farther than 1e-12 from fov / 2 -- orders of magnitude beyond the
// few-ulp error of any arccos or cosine -- and the comparison of d with cth gives the arccos test's
// answer; only the 2e-12-wide band around cth evaluates the arccos itself.
__device__ inline bool in_fov(double fx, double fy, double px1, double py1, double px2, double py2, double fov,
                              double cth)
{
    double vx = px2 - px1, vy = py2 - py1;
    const double nv = np_norm2(vx, vy);
    vx = ddiv(vx, nv); vy = ddiv(vy, nv);
    double d = np_dot2(fx, fy, vx, vy);
    if (d != d) return false;  // coincident agents: arccos(nan) -> not visible
    if (fov >= 2.0 * CN_PI) return true;
    d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
    if (d > cth + 1e-12) return true;
    if (d < cth - 1e-12) return false;
    return acos_within(d, fov);
}

// in_fov decided without square roots or divisions where that is exact (FOV < 2 pi; the pair loops of
// phase 1 and the robot's belief test): d = (f . v) / |v| against thresholds 4e-12 either side of cth, as
// sign tests of dp = f . v and of dp^2 - t^2 |v|^2 (d > t <=> dp > t |v|). These are within a few 1e-16 of
// the exact values, and the reference's d (correctly rounded norm, divisions and dot product, in_fov)
// within a few 1e-16 of the exact d too, so outside the +-4e-12 band both sides of cth are decided alike;
// inside it (and for |v|^2 near under/overflow or zero: coincident agents) in_fov itself runs.
__device__ inline bool in_fov_fast(double fx, double fy, double px1, double py1, double px2, double py2, double fov,
                                   double cth)
{
    const double dx = px2 - px1, dy = py2 - py1;
    const double n2 = __fma_rn(dy, dy, dx * dx);
    if (n2 > 1e-200 && n2 < 1e200) {
        const double dp = __fma_rn(fy, dy, fx * dx), dp2 = dp * dp;
        const double hi = cth + 4e-12, lo = cth - 4e-12;
        const bool above = hi >= 0.0 ? (dp > 0.0 && dp2 > hi * hi * n2) : (dp >= 0.0 || dp2 < hi * hi * n2);
        if (above) return true;
        const bool below = lo > 0.0 ? (dp <= 0.0 || dp2 < lo * lo * n2) : (dp < 0.0 && dp2 > lo * lo * n2);
        if (below) return false;
    }
    return in_fov(fx, fy, px1, py1, px2, py2, fov, cth);
}

// the robot's FOV test of a freshly spawned human (generate_ob(reset=True)), out of line: inlined into the
// step kernel's RNG phase, the acos polynomial's f64 constants were hoisted to the loop preheader and
// spilled to scratch by every wave with RNG work; only FOV < 2 pi configurations call it
__device__ __noinline__ int reset_fov_test(double th, double rpx, double rpy, double px, double py, double fov)
{
    double fx, fy;
    fov_dir64(th, fx, fy);
    return in_fov(fx, fy, rpx, rpy, px, py, fov, cos(fov / 2)) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// shapely restatements (parity unpinned)
// ------------------------------------------------------------------------------------------------
__device__ inline void vel_rect(double px, double py, double vx, double vy, double r, bool f32, double *cx,
                                double *cy)
{
    const double w = 2 * r * 1;
    double len, dth, xos, yos;
    if (f32) {
        const float fvx = (float)vx, fvy = (float)vy;
        len = (double)(3.0f * fsqrt(fvx * fvx + fvy * fvy));
        const float h = atan2f(fvy, fvx);
        dth = (double)(h - (float)(CN_PI / 2));
        xos = px + (double)((float)r * np_cosf(h));
        yos = py + (double)((float)r * np_sinf(h));
    } else {
        len = 3 * dsqrt(vx * vx + vy * vy);
        const double heading = atan2(vy, vx);
        dth = heading - CN_PI / 2;
        xos = px + r * cos(heading);
        yos = py + r * sin(heading);
    }
    double c = cos(dth), s = sin(dth);
    if (fabs(c) < 2.5e-16) c = 0.0;
    if (fabs(s) < 2.5e-16) s = 0.0;
    const double bx[4] = {w / 2, w / 2, -w / 2, -w / 2};
    const double by0[4] = {-len / 2, len / 2, len / 2, -len / 2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double x = bx[k], y = by0[k] + len / 2;
        cx[k] = (c * x - s * y) + xos;
        cy[k] = (s * x + c * y) + yos;
    }
}

__device__ inline bool quads_intersect(const double *ax, const double *ay, const double *bx, const double *by)
{
    for (int p = 0; p < 2; ++p) {
        const double *qx = p ? bx : ax, *qy = p ? by : ay;
        for (int k = 0; k < 4; ++k) {
            const double ex = qx[(k + 1) & 3] - qx[k], ey = qy[(k + 1) & 3] - qy[k];
            if (ex == 0.0 && ey == 0.0) continue;
            for (int t = 0; t < 2; ++t) {
                const double nx = t ? ex : -ey, ny = t ? ey : ex;
                double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double pa = ax[v] * nx + ay[v] * ny, pb = bx[v] * nx + by[v] * ny;
                    amin = pa < amin ? pa : amin; amax = pa > amax ? pa : amax;
                    bmin = pb < bmin ? pb : bmin; bmax = pb > bmax ? pb : bmax;
                }
                if (amax < bmin || bmax < amin) return false;
            }
        }
    }
    return true;
}

// quads_intersect split over the 4 lanes of a quad: lane s tests the 4 axes of edges 2(s & 1), 2(s & 1) + 1 of
// quad s >> 1 and the quad ORs "separated" (a separating axis exists iff some lane found one: the same
// boolean as the sequential early-out loop). Lanes of the quad must run it together.
__device__ __forceinline__ bool quads_intersect_q(const double *ax, const double *ay, const double *bx, const double *by,
                                                  int s)
{
    // the lane's quad and edges by register selects (no lane-dependent indexing)
    const bool qb = (s >> 1) != 0, hi = (s & 1) != 0;
    double Qx[4], Qy[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) { Qx[v] = qb ? bx[v] : ax[v]; Qy[v] = qb ? by[v] : ay[v]; }
    double ex[2], ey[2];
    ex[0] = hi ? Qx[3] - Qx[2] : Qx[1] - Qx[0]; ey[0] = hi ? Qy[3] - Qy[2] : Qy[1] - Qy[0];   // edge k0
    ex[1] = hi ? Qx[0] - Qx[3] : Qx[2] - Qx[1]; ey[1] = hi ? Qy[0] - Qy[3] : Qy[2] - Qy[1];   // edge k0 + 1
    int sep = 0;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        if (ex[kk] == 0.0 && ey[kk] == 0.0) continue;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const double nx = t ? ex[kk] : -ey[kk], ny = t ? ey[kk] : ex[kk];
            double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const double pa = ax[v] * nx + ay[v] * ny, pb = bx[v] * nx + by[v] * ny;
                amin = pa < amin ? pa : amin; amax = pa > amax ? pa : amax;
                bmin = pb < bmin ? pb : bmin; bmax = pb > bmax ? pb : bmax;
            }
            if (amax < bmin || bmax < amin) sep = 1;
        }
    }
    return quad_or(sep) == 0;
}

__device__ inline bool inside_world(double px, double py, double r, double half)
{
    const bool right = (px + r >= half) && (px - r <= half);
    const bool left = (px - r <= -half) && (px + r >= -half);
    const bool top = (py + r >= half) && (py - r <= half);
    const bool bottom = (py - r <= -half) && (py + r >= -half);
    return !(right || left || top || bottom);
}

// The robot's heading frame of its norm zones (both zones share it): offset point and rotation by dth
struct ZoneFrame {
    double dth, xos, yos, c, s;
};

__device__ __forceinline__ ZoneFrame zone_frame(double px, double py, double vx, double vy, double r, bool f32)
{
    ZoneFrame f;
    if (f32) {
        const float h = atan2f((float)vy, (float)vx);
        f.dth = (double)(h - (float)(CN_PI / 2));
        f.xos = px + (double)((float)r * np_cosf(h));
        f.yos = py + (double)((float)r * np_sinf(h));
    } else {
        const double heading = atan2(vy, vx);
        f.dth = heading - CN_PI / 2;
        f.xos = px + r * cos(heading);
        f.yos = py + r * sin(heading);
    }
    f.c = cos(f.dth); f.s = sin(f.dth);
    if (fabs(f.c) < 2.5e-16) f.c = 0.0;
    if (fabs(f.s) < 2.5e-16) f.s = 0.0;
    return f;
}

__device__ inline void norm_zone(const ZoneFrame &f, double r, int lhs, int left, double *cx, double *cy)
{
    const double w = 2 * r * 1.5, len = 1.5 * 1.2;
    const double xos = f.xos, yos = f.yos, c = f.c, s = f.s;
    double tx, ty;
    if (lhs) { if (left) { tx = -w / 2; ty = len / 2 + 0.6; } else { tx = w / 2; ty = len / 2; } }
    else { if (left) { tx = -w / 2; ty = len / 2; } else { tx = w / 2; ty = len / 2 + 0.6; } }
    const double bx[4] = {w / 2, w / 2, -w / 2, -w / 2};
    const double by[4] = {-len / 2, len / 2, len / 2, -len / 2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double x = bx[k] + tx, y = by[k] + ty;
        cx[k] = (c * x - s * y) + xos;
        cy[k] = (s * x + c * y) + yos;
    }
}

// robot disc (GEOS 64-gon buffer) vs convex quad; unit circle table precomputed on the host
__constant__ double c_circ_cos[64];
__constant__ double c_circ_sin[64];

// GEOS's 64-gon buffer of the robot disc (Point.buffer(r)): vertex k at angle -k*pi/32
__device__ __forceinline__ double gon_x(double px, double r, int k)
{
    k &= 63;
    return k == 0 ? px + r : px + r * c_circ_cos[k];
}
__device__ __forceinline__ double gon_y(double py, double r, int k)
{
    k &= 63;
    return k == 0 ? py : py + r * c_circ_sin[k];
}

// Extents of the 64-gon on axis n: the vertex projections V_k.n = P.n + r|n|cos(theta_k - phi) peak at
// the vertex nearest phi (kmax) and bottom out opposite (kmax + 32); vertices two or more steps away
// are smaller by >= ~r|n|*pi^2/1024 relative to the extreme, ~10^12 times any rounding of a projection,
// so the extremes over a +-2 window equal those over all 64 vertices exactly (min / max are
// order-independent).
__device__ __forceinline__ void gon_extent(double px, double py, double r, double nx, double ny, int kmax,
                                           double &amin, double &amax)
{
    amin = INFINITY; amax = -INFINITY;
#pragma unroll
    for (int d = -2; d <= 2; ++d) {
        const double t = gon_x(px, r, kmax + d) * nx + gon_y(py, r, kmax + d) * ny;
        const double u = gon_x(px, r, kmax + 32 + d) * nx + gon_y(py, r, kmax + 32 + d) * ny;
        amax = t > amax ? t : amax;
        amin = u < amin ? u : amin;
    }
}

// One 64-gon edge axis of disc_quad_sat's second loop (edge k -> k + 1, extents over the +-2 vertex windows
// of gon_extent): true if it separates the 64-gon from the quad. Same vertices, same operations as the loop.
__device__ __forceinline__ bool gon_axis_separates(double px, double py, double r, const double *qx, const double *qy, int k)
{
    auto vx = [&](int idx) { idx &= 63; return idx == 0 ? px + r : px + r * c_circ_cos[idx]; };
    auto vy = [&](int idx) { idx &= 63; return idx == 0 ? py : py + r * c_circ_sin[idx]; };
    const double ex = vx(k + 1) - vx(k), ey = vy(k + 1) - vy(k);
    if (ex == 0.0 && ey == 0.0) return false;
    const double nx = -ey, ny = ex;
    double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const double t = vx(k - 2 + d) * nx + vy(k - 2 + d) * ny;
        const double u = vx(k + 30 + d) * nx + vy(k + 30 + d) * ny;
        amax = t > amax ? t : amax;
        amin = u < amin ? u : amin;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) { const double t = qx[v] * nx + qy[v] * ny; bmin = t < bmin ? t : bmin; bmax = t > bmax ? t : bmax; }
    return amax < bmin || bmax < amin;
}

// Separating-axis test over the edge normals of the quad and of the 64-gon (the predicate the oracle,
// oracle/cpu_ref.c:disc_quad_intersect, evaluates with all 64 vertices per axis): identical boolean. Only the
// fallback for degenerate quads / radii (and the test hook's mode 1), so written for few registers: loops
// not unrolled.
__device__ __forceinline__ bool disc_quad_sat(double px, double py, double r, const double *qx, const double *qy)
{
    const double step = CN_PI / 32;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {   // quad edges: the 64-gon's extreme vertex from the axis angle
        const int k1 = (k + 1) & 3;
        const double ex = qx[k1] - qx[k], ey = qy[k1] - qy[k];
        if (ex == 0.0 && ey == 0.0) continue;
        const double nx = -ey, ny = ex;
        const int kmax = ((int)rint(-atan2(ny, nx) / step) % 64 + 64) % 64;
        double amin, amax, bmin = INFINITY, bmax = -INFINITY;
        gon_extent(px, py, r, nx, ny, kmax, amin, amax);
#pragma unroll
        for (int v = 0; v < 4; ++v) { const double t = qx[v] * nx + qy[v] * ny; bmin = t < bmin ? t : bmin; bmax = t > bmax ? t : bmax; }
        if (amax < bmin || bmax < amin) return false;
    }
#pragma unroll 1
    for (int k = 0; k < 64; ++k)   // 64-gon edge k -> k+1 (its normal points at -(k + 1/2) pi/32)
        if (gon_axis_separates(px, py, r, qx, qy, k)) return false;
    return true;
}

// disc_quad_sat for a centre P OUTSIDE the quad within the boundary band (r cos(pi/64) - eps <= d <= r + eps,
// d = |c - P|, c the quad's closest point, (cx, cy) = c - P): the same boolean from the 4 quad axes and only
// the 64-gon edge axes whose direction lies within 3 steps of c - P or of P - c. Why no other axis can
// separate: an axis of unit direction u separates (amax < bmin) only if min_q (q - P).u exceeds the 64-gon's
// support (v - P).u, which is at least the apothem r cos(pi/64) for every u; but min_q (q - P).u <=
// (c - P).u = d cos(angle(u, c - P)) <= (r + eps) cos(angle). Edge k's normal points at -(k + 1/2) pi/32;
// ks, the nearest such edge to c - P, is within pi/64 (+ rounding of atan2 / rint) of it, so an edge 4 or
// more steps away is >= 3.5 pi/32 off: (r + eps) cos(3.5 pi/32) = 0.941 (r + eps) < 0.9988 r -- a margin of
// ~0.057 r against eps = 1e-9 and the ~1e-15 r rounding of the projections (r > 1e-6 here). The other
// condition (bmax < amin) is separation along -u: the window around ks + 32. SURVEY §9-7; the 100 k predicate
// cases of tests/test_norm_zone.py (the zones' corner-on-circle geometry included) check it against the
// oracle's all-axes test.
// kq >= 0: the quad is a norm zone (a rectangle rotated by dth, norm_zone), whose edge k's normal points at
// dth + pi + k pi/2, so the 64-gon's extreme vertex for it is (kq - 16 k) & 63 with kq = rint(-dth / step) - 32
// -- the vertex nearest the normal up to one step where the rounded edge vector's atan2 would round the other
// way, which gon_extent's +-2 window absorbs (its extremes are those of all 64 vertices for any kmax within one
// step of the nearest vertex): the same amin / amax, without four f64 atan2. kq < 0: atan2 per edge.
__device__ __forceinline__ bool disc_quad_sat_band(double px, double py, double r, const double *qx, const double *qy,
                                                   double cx, double cy, int kq)
{
    const double step = CN_PI / 32;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {   // quad edges, as in disc_quad_sat
        const int k1 = (k + 1) & 3;
        const double ex = qx[k1] - qx[k], ey = qy[k1] - qy[k];
        if (ex == 0.0 && ey == 0.0) continue;
        const double nx = -ey, ny = ex;
        const int kmax = kq >= 0 ? (kq - 16 * k) & 63 : ((int)rint(-atan2(ny, nx) / step) % 64 + 64) % 64;
        double amin, amax, bmin = INFINITY, bmax = -INFINITY;
        gon_extent(px, py, r, nx, ny, kmax, amin, amax);
#pragma unroll
        for (int v = 0; v < 4; ++v) { const double t = qx[v] * nx + qy[v] * ny; bmin = t < bmin ? t : bmin; bmax = t > bmax ? t : bmax; }
        if (amax < bmin || bmax < amin) return false;
    }
    const int ks = (int)rint(-atan2(cy, cx) / step - 0.5);
#pragma unroll 1
    for (int j = -3; j <= 3; ++j) {
        if (gon_axis_separates(px, py, r, qx, qy, (ks + j) & 63)) return false;
        if (gon_axis_separates(px, py, r, qx, qy, (ks + 32 + j) & 63)) return false;
    }
    return true;
}

__device__ __forceinline__ int disc_quad_classify(double px, double py, double r, const double *qx, const double *qy,
                                                  double sgn, double eps, double &cx, double &cy)
{
    bool inside = true;
    double d2 = INFINITY;   // squared distance from P to the quad's boundary segments
    cx = 0.0; cy = 0.0;     // closest boundary point - P
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const double ex = qx[k1] - qx[k], ey = qy[k1] - qy[k];
        const double wx = px - qx[k], wy = py - qy[k];
        if (sgn * (ex * wy - ey * wx) < 0) inside = false;
        const double ee = ex * ex + ey * ey;
        double t = ee > 0 ? (wx * ex + wy * ey) / ee : 0.0;
        t = t < 0 ? 0 : (t > 1 ? 1 : t);
        const double dx = wx - t * ex, dy = wy - t * ey;
        const double dd = dx * dx + dy * dy;
        if (dd < d2) { d2 = dd; cx = -dx; cy = -dy; }
    }
    if (inside) return 1;
    const double d = sqrt(d2);
    if (d < r * 0.99879545620517241 - eps) return 1;   // cos(pi/64)
    if (d > r + eps) return 0;
    return -1;
}

// robot 64-gon vs a norm-zone quad (Point.buffer(r).intersects(zone), crowd_sim.py norm-zone penalty).
// Away from the boundary the answer is geometric: the 64-gon lies between the discs of radius
// r cos(pi/64) and r about P, so a centre distance to the (convex) quad below r cos(pi/64) - eps means
// intersecting and above r + eps disjoint (eps = 1e-9 >> rounding of the inputs); only the thin band in
// between runs the separating-axis test (disc_quad_sat_band's axes). Returns 1 / 0, or -1 for a degenerate
// quad or radius, which the full separating-axis test (disc_quad_sat) decides.
__device__ __forceinline__ int disc_quad_intersect3(double px, double py, double r, const double *qx, const double *qy,
                                                    int kq = -1)
{
    const double eps = 1e-9;
    double area2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) area2 += qx[k] * qy[(k + 1) & 3] - qx[(k + 1) & 3] * qy[k];
    if (!(fabs(area2) > 1e-12 && r > 1e-6)) return -1;
    double cx, cy;
    // 1 / 0 decided by the distance classification, -1: the centre is in the band, outside the quad
    const int cls = disc_quad_classify(px, py, r, qx, qy, area2 > 0 ? 1.0 : -1.0, eps, cx, cy);
    return cls >= 0 ? cls : (int)disc_quad_sat_band(px, py, r, qx, qy, cx, cy, kq);
}

__device__ __forceinline__ bool disc_quad_intersect(double px, double py, double r, const double *qx, const double *qy)
{
    const int v = disc_quad_intersect3(px, py, r, qx, qy);
    return v >= 0 ? v != 0 : disc_quad_sat(px, py, r, qx, qy);
}

// crowd_sim.py:918-926,957-960 (norm zones on): both zones are built around the robot and
// tested against its own disc. Out of line: the separating-axis tests would otherwise raise the step
// kernel's register pressure (and scratch) for every workload, norm zones on or off. Returns 1 / 0, or -1
// when a zone is degenerate (a robot radius <= 1e-6): robot_norm_zone_violation then decides with the full
// separating-axis test. Two callees, each without calls of its own: a callee's VGPR count (the highest
// register it touches, callee-saved ones included when it calls further) is charged to every kernel that
// calls it, beyond the kernel's launch bounds.
__device__ __noinline__ int robot_norm_zone_fast(double px, double py, double vx, double vy, double rr, bool f32, int lhs)
{
    double zx[4], zy[4];
    const ZoneFrame f = zone_frame(px, py, vx, vy, rr, f32);   // the heading's trigonometry once for both zones
    const int kq = ((int)rint(-f.dth / (CN_PI / 32)) - 32) & 63;
#pragma unroll 1
    for (int z = 0; z < 2; ++z) {
        norm_zone(f, rr, lhs, z == 0, zx, zy);
        const int v = disc_quad_intersect3(px, py, rr, zx, zy, kq);
        if (v != 0) return v;
    }
    return 0;
}

__device__ __noinline__ bool robot_norm_zone_full(double px, double py, double vx, double vy, double rr, bool f32, int lhs)
{
    double zx[4], zy[4];
    const ZoneFrame f = zone_frame(px, py, vx, vy, rr, f32);
#pragma unroll 1
    for (int z = 0; z < 2; ++z) {
        norm_zone(f, rr, lhs, z == 0, zx, zy);
        if (disc_quad_sat(px, py, rr, zx, zy)) return true;
    }
    return false;
}

__device__ __forceinline__ bool robot_norm_zone_violation(double px, double py, double vx, double vy, double rr, bool f32,
                                                          int lhs)
{
    const int v = robot_norm_zone_fast(px, py, vx, vy, rr, f32, lhs);
    return v >= 0 ? v != 0 : robot_norm_zone_full(px, py, vx, vy, rr, f32, lhs);
}
