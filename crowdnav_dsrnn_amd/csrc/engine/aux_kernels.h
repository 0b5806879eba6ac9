// aux_kernels.h -- the small stand-alone kernels: the debug / predictor kernels that expose the step kernel's
// device functions on caller-given inputs (cn_disc_quad, cn_copy64, cn_orca, cn_orca_kd with RVO2's sequential
// KdTree, cn_sf_predict, cn_dwa_predict), cn_robot_act's kernels (ORCA, social force, the dynamic window), cn_rollout_noisy's (cn_action_noise_kernel,
// cn_noise_set_kernel, cn_copy32_kernel), cn_robot_mix's (cn_robot_mix_kernel, cn_mix_ctl_set_kernel), cn_rollout_lidar's (cn_rows_set_kernel, cn_state_rows_kernel), and the
// two stream-ordered helpers of the host API (cn_ctl_set_kernel, cn_keysnap_kernel), cn_visible_mask's, and last cn_robot_act_regret's two (the dynamic window with its regret row). Part of cn_engine.hip's translation unit: included there after the device core, whose
// geometry, ORCA and scripted-robot functions these kernels call.
#pragma once

__global__ void __launch_bounds__(64) cn_disc_quad_kernel(int64_t n, int mode, const double *px, const double *py,
                                                          const double *r, const double *qx, const double *qy,
                                                          int32_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 2)   // the robot's norm-zone penalty predicate: qx[i] = {vx, f32, ...}, qy[i] = {vy, lhs, ...}
        out[i] = robot_norm_zone_violation(px[i], py[i], qx[4 * i], qy[4 * i], r[i], qx[4 * i + 1] != 0.0,
                                           (int)qy[4 * i + 1]);
    else
        out[i] = mode ? disc_quad_sat(px[i], py[i], r[i], qx + 4 * i, qy + 4 * i)
                      : disc_quad_intersect(px[i], py[i], r[i], qx + 4 * i, qy + 4 * i);
}

// cn_debug_copy64: one wave per segment of `seg` doubles
__global__ void __launch_bounds__(64) cn_copy64_kernel(int64_t n, int seg, const double *__restrict__ src,
                                                       double *__restrict__ dst)
{
    const int64_t k = (int64_t)blockIdx.x * seg + threadIdx.x;
    if ((int)threadIdx.x < seg && k < n) dst[k] = src[k];
}

// cn_debug_orca: one quad per simulator (16 per 64-lane workgroup), the step kernel's quad-path functions
__global__ void __launch_bounds__(64) cn_orca_kernel(int64_t n, int A, const float *__restrict__ ag,
                                                     const float *__restrict__ self, float nd, float th, float ts,
                                                     float *__restrict__ out)
{
    __shared__ float4 Ls[16][9];
    const int q = threadIdx.x >> 2, sq = threadIdx.x & 3;
    const int64_t i = (int64_t)blockIdx.x * 16 + q;
    const bool act = i < n;
    const float *a = ag + (act ? i : 0) * A * 5;
    const int M = A - 1;
    int cnt = 0;
    if (act)
        cnt = orca_lines_quad(
            [&](int k, float &x, float &y, float &vx, float &vy, float &r) {
                const float *o = a + (k + 1) * 5;
                x = o[0]; y = o[1]; vx = o[2]; vy = o[3]; r = o[4];
            },
            M, sq, a[0], a[1], a[2], a[3], a[4], nd * nd, fdiv(1.0f, th), fdiv(1.0f, ts), Ls[q]);
    wsync();
    if (act) {
        const float vmax = self[3 * i], ox = self[3 * i + 1], oy = self[3 * i + 2];
        float rx, ry;
        float4 R[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) R[u] = sq + 4 * u < cnt ? Ls[q][sq + 4 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
        const int fail_at = lp2_r<3, true>(R, cnt, vmax, ox, oy, sq, rx, ry, Ls[q]);   // the walk: tests/test_lp_walk.py
        if (fail_at < cnt) lp3_r<3>(R, Ls[q], cnt, fail_at, vmax, sq, rx, ry);
        if (sq == 0) {
            out[4 * i] = rx; out[4 * i + 1] = ry; out[4 * i + 2] = (float)fail_at; out[4 * i + 3] = (float)cnt;
        }
    }
}

// cn_orca_predict_kd: ORCA.predict of simulators of any size up to CN_ORCA_MAXA agents, with RVO2's KdTree
// (MAX_LEAF_SIZE 10) and its persisted agents_ order. One quad per simulator (16 per 64-lane workgroup):
// lane 0 of the quad builds the tree (buildAgentTreeRecursive, which re-permutes agents_ in place) and runs
// the query (queryAgentTreeRecursive + insertAgentNeighbor with maxNeighbors = A - 1), both sequential as
// in RVO2 -- the plugin serves one predict per agent per env step, off the batched step path, which has its
// own ballot-partitioned walk; then the quad builds the ORCA lines in neighbour order and runs the quad
// linear programs of the step kernel. Oracle: cpu_ref.c:kd_build / kd_query / rvo2_agent0.
#define CN_ORCA_MAXA 64
// 20 B per node: ranges and child indices fit bytes (A <= 64 agents, < 2A nodes); the build / query stacks
// below are bytes too -- the per-lane private arrays were 5.7 KB of scratch per lane with ints, 3.3 KB now
struct KdNodeS { uint8_t begin, end, left, right; float minX, maxX, minY, maxY; };

__device__ __forceinline__ float kd_bdist(const KdNodeS &t, float x, float y)
{
    const float a = (0.0f < t.minX - x) ? t.minX - x : 0.0f, b = (0.0f < x - t.maxX) ? x - t.maxX : 0.0f;
    const float cc = (0.0f < t.minY - y) ? t.minY - y : 0.0f, d = (0.0f < y - t.maxY) ? y - t.maxY : 0.0f;
    return a * a + b * b + cc * cc + d * d;
}

// lane-sequential KdTree build + query over X / Y [A] (LDS), perm [A] (LDS, updated in place); writes the
// neighbours of agent 0 in insertion-sorted order to nb [A - 1] (agent ids) and returns their count
__device__ int kd_neighbors_seq(int A, const float *X, const float *Y, uint8_t *perm, float rangeSq, uint8_t *nb)
{
    KdNodeS T[2 * CN_ORCA_MAXA];
    uint8_t stk[CN_ORCA_MAXA + 2][3];
    int sp = 0;
    stk[sp][0] = 0; stk[sp][1] = (uint8_t)A; stk[sp][2] = 0; ++sp;
    while (sp > 0) {   // any order of the recursive calls gives the same tree: children own disjoint ranges
        --sp;
        const int begin = stk[sp][0], end = stk[sp][1], node = stk[sp][2];
        KdNodeS t;
        t.begin = (uint8_t)begin; t.end = (uint8_t)end; t.left = t.right = 0;
        t.minX = t.maxX = X[perm[begin]];
        t.minY = t.maxY = Y[perm[begin]];
        for (int i = begin + 1; i < end; ++i) {
            const float x = X[perm[i]], y = Y[perm[i]];
            t.maxX = t.maxX < x ? x : t.maxX; t.minX = x < t.minX ? x : t.minX;
            t.maxY = t.maxY < y ? y : t.maxY; t.minY = y < t.minY ? y : t.minY;
        }
        if (end - begin > 10) {
            const bool vert = t.maxX - t.minX > t.maxY - t.minY;
            const float split = vert ? 0.5f * (t.maxX + t.minX) : 0.5f * (t.maxY + t.minY);
            int left = begin, right = end;
            while (left < right) {
                while (left < right && (vert ? X[perm[left]] : Y[perm[left]]) < split) ++left;
                while (right > left && (vert ? X[perm[right - 1]] : Y[perm[right - 1]]) >= split) --right;
                if (left < right) {
                    const uint8_t s = perm[left]; perm[left] = perm[right - 1]; perm[right - 1] = s;
                    ++left; --right;
                }
            }
            if (left == begin) { ++left; ++right; }
            t.left = (uint8_t)(node + 1);
            t.right = (uint8_t)(node + 2 * (left - begin));
            stk[sp][0] = (uint8_t)left; stk[sp][1] = (uint8_t)end; stk[sp][2] = t.right; ++sp;
            stk[sp][0] = (uint8_t)begin; stk[sp][1] = (uint8_t)left; stk[sp][2] = t.left; ++sp;
        }
        T[node] = t;
    }
    // query: a node popped with distance d is walked only if d < rangeSq at that moment (the recursion tests
    // the nearer child at once and the farther one after the nearer subtree; ties visit the right first)
    const int maxN = A - 1;
    float nd[CN_ORCA_MAXA];
    int cnt = 0;
    float dst[CN_ORCA_MAXA + 2];
    uint8_t nst[CN_ORCA_MAXA + 2];
    sp = 0;
    nst[0] = 0; dst[0] = -1.0f; sp = 1;
    const float x0 = X[0], y0 = Y[0];
    while (sp > 0) {
        --sp;
        const int node = nst[sp];
        if (!(dst[sp] < rangeSq)) continue;
        const KdNodeS &t = T[node];
        if (t.end - t.begin <= 10) {
            for (int i = t.begin; i < t.end; ++i) {   // Agent::insertAgentNeighbor
                const int a = perm[i];
                if (a == 0) continue;
                const float dx = x0 - X[a], dy = y0 - Y[a];
                const float distSq = dx * dx + dy * dy;
                if (distSq < rangeSq) {
                    if (cnt < maxN) { nd[cnt] = distSq; nb[cnt] = (uint8_t)a; ++cnt; }
                    int k = cnt - 1;
                    while (k != 0 && distSq < nd[k - 1]) { nd[k] = nd[k - 1]; nb[k] = nb[k - 1]; --k; }
                    nd[k] = distSq; nb[k] = (uint8_t)a;
                    if (cnt == maxN) rangeSq = nd[cnt - 1];
                }
            }
            continue;
        }
        const float dl = kd_bdist(T[t.left], x0, y0), dr = kd_bdist(T[t.right], x0, y0);
        if (dl < dr) { nst[sp] = t.right; dst[sp] = dr; nst[sp + 1] = t.left; dst[sp + 1] = dl; }
        else { nst[sp] = t.left; dst[sp] = dl; nst[sp + 1] = t.right; dst[sp + 1] = dr; }
        sp += 2;
    }
    return cnt;
}

// LDS of one cn_orca_kd_kernel workgroup, sized by the simulators' agent count A (dynamic): 16 quads' lines
// and projected lines [A - 1] float4 each, positions [A] float x 2, agents_ order and neighbours [A] bytes, counts.
// (Sized for CN_ORCA_MAXA it was 42.5 KB, 3 one-wave workgroups per CU; at A = 26, 17 KB: 9.)
__host__ __device__ inline int orca_kd_lds(int A)
{
    return 16 * (2 * 16 * (A - 1) + 2 * 4 * A) + ((2 * 16 * A + 15) & ~15) + 16 * 4;
}

__global__ void __launch_bounds__(64) cn_orca_kd_kernel(int64_t n, int A, const float *__restrict__ ag,
                                                        const float *__restrict__ self, float nd, float th, float ts,
                                                        uint8_t *__restrict__ perm_io, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char kd_smem[];
    const int q = threadIdx.x >> 2, sq = threadIdx.x & 3;
    float4 *Lq = (float4 *)kd_smem + q * (A - 1);                 // [16][A - 1]
    float4 *Pq = (float4 *)kd_smem + 16 * (A - 1) + q * (A - 1);  // [16][A - 1]
    float *Xq = (float *)(kd_smem + 16 * 2 * 16 * (A - 1)) + q * A;
    float *Yq = (float *)(kd_smem + 16 * 2 * 16 * (A - 1)) + 16 * A + q * A;
    uint8_t *Pmq = (uint8_t *)(kd_smem + 16 * (2 * 16 * (A - 1) + 2 * 4 * A)) + q * A;
    uint8_t *Nbq = (uint8_t *)(kd_smem + 16 * (2 * 16 * (A - 1) + 2 * 4 * A)) + 16 * A + q * A;
    int *Cn = (int *)(kd_smem + orca_kd_lds(A) - 16 * 4);
    const int64_t i = (int64_t)blockIdx.x * 16 + q;
    const bool act = i < n;
    const float *a = ag + (act ? i : 0) * A * 5;
    if (act)
        for (int k = sq; k < A; k += 4) {
            Xq[k] = a[k * 5]; Yq[k] = a[k * 5 + 1];
            Pmq[k] = perm_io ? perm_io[i * A + k] : (uint8_t)k;
        }
    wsync();
    if (act && sq == 0) Cn[q] = A > 1 ? kd_neighbors_seq(A, Xq, Yq, Pmq, nd * nd, Nbq) : 0;
    wsync();
    if (act) {
        const int cnt = Cn[q];
        const float invTH = fdiv(1.0f, th), invTS = fdiv(1.0f, ts);
        for (int k = sq; k < cnt; k += 4) {
            const float *o = a + Nbq[k] * 5;
            Lq[k] = orca_line(a[0], a[1], a[2], a[3], a[4], o[0], o[1], o[2], o[3], o[4], invTH, invTS);
        }
        if (perm_io)
            for (int k = sq; k < A; k += 4) perm_io[i * A + k] = Pmq[k];
    }
    wsync();
    if (act) {
        const int cnt = Cn[q];
        const float vmax = self[3 * i], ox = self[3 * i + 1], oy = self[3 * i + 2];
        float rx, ry;
        const int fail_at = lp2_q<uint64_t>(Lq, cnt, vmax, ox, oy, sq, rx, ry);
        if (fail_at < cnt) lp3_q<uint64_t>(Lq, Pq, cnt, fail_at, vmax, sq, rx, ry);
        if (sq == 0) {
            out[4 * i] = rx; out[4 * i + 1] = ry; out[4 * i + 2] = (float)fail_at; out[4 * i + 3] = (float)cnt;
        }
    }
}

// cn_social_force_predict: SOCIAL_FORCE.predict (social_force.py:11-66) for n agents, one lane each, f64 in
// the reference's operation order (the step kernel's phase 2 on caller-given states)
__global__ void __launch_bounds__(64) cn_sf_predict_kernel(int64_t n, int M, const double *__restrict__ self,
                                                           const double *__restrict__ others, double A, double B,
                                                           double KI, double dt, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *s = self + 9 * i;   // px, py, vx, vy, radius, gx, gy, v_pref, theta
    const double px = s[0], py = s[1], vx0 = s[2], vy0 = s[3], rad = s[4], vpref = s[7];
    const double gdx = s[5] - px, gdy = s[6] - py;
    const double dg = dsqrt(gdx * gdx + gdy * gdy);
    const double dvx = ddiv(gdx, dg) * vpref, dvy = ddiv(gdy, dg) * vpref;
    const double cdx = KI * (dvx - vx0), cdy = KI * (dvy - vy0);
    double ix = 0.0, iy = 0.0;
    for (int k = 0; k < M; ++k) {
        const double *o = others + (i * M + k) * 5;   // px, py, vx, vy, radius
        const double ddx = px - o[0], ddy = py - o[1];
        const double d = dsqrt(ddx * ddx + ddy * ddy);
        const double ex = exp(ddiv(rad + o[4] - d, B));
        ix += A * ex * ddiv(ddx, d);
        iy += A * ex * ddiv(ddy, d);
    }
    const double nx = vx0 + (cdx + ix) * dt, ny = vy0 + (cdy + iy) * dt;
    const double nn = np_norm2(nx, ny);
    if (nn > vpref) { out[2 * i] = ddiv(nx, nn) * vpref; out[2 * i + 1] = ddiv(ny, nn) * vpref; }
    else { out[2 * i] = nx; out[2 * i + 1] = ny; }
}

// ------------------------------------------------------------------------------------------------
// cn_robot_act: the scripted robot (ORCA / social force) on the engine's CURRENT state, read straight from
// the blob: policy_factory[name](config).predict(JointState(robot FullState, [ObservableState(b_px, b_py,
// b_vx, b_vy, b_r) of the N humans in index order])) of a fresh policy object per env, rounded to float32.
// Pure functions of the state (nothing held between calls), one launch each (a mixed engine: one per group).
// Each has a twin for a group of a mixed engine (cn_robot_*_mix_kernel: the same body with MIX), where env e's action
// goes to row rows[e] of `actions`. The map changes that address alone, never which lanes run; the plain kernels
// carry no argument for it and compile as before.
// uni (launch-uniform: the engine's kinematics is unicycle, served after cn_scripted_unicycle): the lane that stores
// the action first turns the controller's velocity into the step's (dv, dtheta) with robot_unicycle_track. Which
// lanes run, and the quads' control flow up to that store, do not depend on it.
// ------------------------------------------------------------------------------------------------
// (robot_sim_agent, robot_pref_velocity, robot_orca_lines / robot_orca_solve and robot_sf_velocity are defined above
// cn_step_kernel, whose rollout variant computes the same actions inside its multi-step launches)
// ORCA, N + 1 <= 10 agents: cn_orca_kernel's quad path (one quad per env, 16 envs per 64-lane workgroup).
// `act` depends on the quad alone, so a quad is whole or absent and its control flow uniform (DESIGN.md §4,
// "Cross-lane reads"): the quad's 4 lanes read the same state words.
__global__ void __launch_bounds__(64) cn_robot_orca_kernel(cn_state_ptrs S, int E, int N, double safety, float nd,
                                                           float th, float ts, float *__restrict__ actions, int uni)
{
    __shared__ float4 Ls[16][9];
    const int q = threadIdx.x >> 2, sq = threadIdx.x & 3;
    const int64_t e = (int64_t)blockIdx.x * 16 + q;
    const bool act = e < E;
    int cnt = 0;
    if (act) cnt = robot_orca_lines(S, safety, e, N, sq, nd, th, ts, Ls[q]);
    wsync();
    if (act) {
        float rx, ry;
        robot_orca_solve(S, e, cnt, sq, Ls[q], rx, ry);
        if (sq == 0) {
            if (uni) robot_unicycle_track(S, e, rx, ry, rx, ry);   // (launch-uniform; lane 0 of the quad alone)
            actions[2 * e] = rx; actions[2 * e + 1] = ry;
        }
    }
}
// (the twin restates the dozen lines above: as a shared body the plain kernel came out with other registers)
__global__ void __launch_bounds__(64) cn_robot_orca_mix_kernel(cn_state_ptrs S, int E, int N, double safety, float nd,
                                                               float th, float ts, float *__restrict__ actions,
                                                               const int32_t *__restrict__ rows, int uni)
{
    __shared__ float4 Ls[16][9];
    const int q = threadIdx.x >> 2, sq = threadIdx.x & 3;
    const int64_t e = (int64_t)blockIdx.x * 16 + q;
    const bool act = e < E;
    int cnt = 0;
    if (act) cnt = robot_orca_lines(S, safety, e, N, sq, nd, th, ts, Ls[q]);
    wsync();
    if (act) {
        float rx, ry;
        robot_orca_solve(S, e, cnt, sq, Ls[q], rx, ry);
        if (sq == 0) {
            if (uni) robot_unicycle_track(S, e, rx, ry, rx, ry);
            const int64_t o = rows[e];
            actions[2 * o] = rx; actions[2 * o + 1] = ry;
        }
    }
}

// ORCA, N + 1 > 10 agents: cn_orca_kd_kernel's path with a fresh simulator's identity agent order (LDS sized by
// A = N + 1: orca_kd_lds)
template <bool MIX>
__device__ __forceinline__ void robot_orca_kd_body(const cn_state_ptrs &S, int E, int N, double safety, float nd,
                                                   float th, float ts, float *__restrict__ actions,
                                                   const int32_t *__restrict__ rows, int uni)
{
    extern __shared__ __attribute__((aligned(16))) char kd_smem[];
    const int A = N + 1;
    const int q = threadIdx.x >> 2, sq = threadIdx.x & 3;
    float4 *Lq = (float4 *)kd_smem + q * (A - 1);                 // [16][A - 1]
    float4 *Pq = (float4 *)kd_smem + 16 * (A - 1) + q * (A - 1);  // [16][A - 1]
    float *Xq = (float *)(kd_smem + 16 * 2 * 16 * (A - 1)) + q * A;
    float *Yq = (float *)(kd_smem + 16 * 2 * 16 * (A - 1)) + 16 * A + q * A;
    uint8_t *Pmq = (uint8_t *)(kd_smem + 16 * (2 * 16 * (A - 1) + 2 * 4 * A)) + q * A;
    uint8_t *Nbq = (uint8_t *)(kd_smem + 16 * (2 * 16 * (A - 1) + 2 * 4 * A)) + 16 * A + q * A;
    int *Cn = (int *)(kd_smem + orca_kd_lds(A) - 16 * 4);
    const int64_t e = (int64_t)blockIdx.x * 16 + q;
    const bool act = e < E;
    if (act)
        for (int k = sq; k < A; k += 4) {
            float x, y, vx, vy, r;
            robot_sim_agent(S, safety, e, N, k, x, y, vx, vy, r);
            Xq[k] = x; Yq[k] = y;
            Pmq[k] = (uint8_t)k;
        }
    wsync();
    if (act && sq == 0) Cn[q] = kd_neighbors_seq(A, Xq, Yq, Pmq, nd * nd, Nbq);
    wsync();
    if (act) {
        const int cnt = Cn[q];
        const float invTH = fdiv(1.0f, th), invTS = fdiv(1.0f, ts);
        float X0, Y0, VX0, VY0, R0;
        robot_sim_agent(S, safety, e, N, 0, X0, Y0, VX0, VY0, R0);
        for (int k = sq; k < cnt; k += 4) {
            float x, y, vx, vy, r;
            robot_sim_agent(S, safety, e, N, Nbq[k], x, y, vx, vy, r);
            Lq[k] = orca_line(X0, Y0, VX0, VY0, R0, x, y, vx, vy, r, invTH, invTS);
        }
    }
    wsync();
    if (act) {
        const int cnt = Cn[q];
        float vmax, ox, oy, rx, ry;
        robot_pref_velocity(S, e, vmax, ox, oy);
        const int fail_at = lp2_q<uint64_t>(Lq, cnt, vmax, ox, oy, sq, rx, ry);
        if (fail_at < cnt) lp3_q<uint64_t>(Lq, Pq, cnt, fail_at, vmax, sq, rx, ry);
        if (sq == 0) {
            if (uni) robot_unicycle_track(S, e, rx, ry, rx, ry);
            const int64_t o = MIX ? (int64_t)rows[e] : e;
            actions[2 * o] = rx; actions[2 * o + 1] = ry;
        }
    }
}
__global__ void __launch_bounds__(64) cn_robot_orca_kd_kernel(cn_state_ptrs S, int E, int N, double safety, float nd,
                                                              float th, float ts, float *__restrict__ actions, int uni)
{
    robot_orca_kd_body<false>(S, E, N, safety, nd, th, ts, actions, nullptr, uni);
}
__global__ void __launch_bounds__(64) cn_robot_orca_kd_mix_kernel(cn_state_ptrs S, int E, int N, double safety, float nd,
                                                                  float th, float ts, float *__restrict__ actions,
                                                                  const int32_t *__restrict__ rows, int uni)
{
    robot_orca_kd_body<true>(S, E, N, safety, nd, th, ts, actions, rows, uni);
}

// Social force: cn_sf_predict_kernel's float64 arithmetic on the robot's FullState and the N belief humans,
// one lane per env; the ActionXY rounded to float32
template <bool MIX>
__device__ __forceinline__ void robot_sf_body(const cn_state_ptrs &S, int E, int N, double A, double B, double KI,
                                              double dt, float *__restrict__ actions, const int32_t *__restrict__ rows,
                                              int uni)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double nx, ny, nn, vpref;
    robot_sf_velocity(S, e, N, A, B, KI, dt, nx, ny, nn, vpref);
    const int64_t o = MIX ? (int64_t)rows[e] : e;
    float ax, ay;
    if (nn > vpref) { ax = (float)(ddiv(nx, nn) * vpref); ay = (float)(ddiv(ny, nn) * vpref); }
    else { ax = (float)nx; ay = (float)ny; }
    if (uni) robot_unicycle_track(S, e, ax, ay, ax, ay);
    actions[2 * o] = ax; actions[2 * o + 1] = ay;
}
__global__ void __launch_bounds__(64) cn_robot_sf_kernel(cn_state_ptrs S, int E, int N, double A, double B, double KI,
                                                         double dt, float *__restrict__ actions, int uni)
{
    robot_sf_body<false>(S, E, N, A, B, KI, dt, actions, nullptr, uni);
}
__global__ void __launch_bounds__(64) cn_robot_sf_mix_kernel(cn_state_ptrs S, int E, int N, double A, double B, double KI,
                                                             double dt, float *__restrict__ actions,
                                                             const int32_t *__restrict__ rows, int uni)
{
    robot_sf_body<true>(S, E, N, A, B, KI, dt, actions, rows, uni);
}

// ------------------------------------------------------------------------------------------------
// The dynamic-window controller of the unicycle robot (include/crowdnav.h, cn_dwa_predict: this project's
// definition). One 64-lane wave per env, lane c = candidate c = 8a + b of the step's 8 x 8 action grid: every lane
// walks its own arc over the horizon against the constant-velocity forecast of the M humans, in float64 without
// contraction, then the wave takes the lexicographic minimum of (J, c) by a shuffle butterfly (ties: the lowest c).
// The env, and with it every human word, is wave-uniform (the caller forms the env index through readfirstlane), so
// the humans are read at one address per wave. A lane that reaches the goal stops walking (`go`), the others go on:
// the loops themselves stay wave-uniform. No LDS, no atomics, no barrier: a wave past the last env returns whole.
// Shared by cn_dwa_predict's kernel and cn_robot_act's two: one arithmetic, bit for bit.
// ------------------------------------------------------------------------------------------------
#define CN_DWA_WAVES 4   // envs per 256-lane workgroup

__device__ __forceinline__ double dwa_grid(int k) { return ddiv(0.1 * (double)(2 * k - 7), 7.0); }

// human(i, bx, by, bvx, bvy, br): belief human i of this wave's env. Returns the lane's cost J; best = the wave's choice.
template <class Human>
__device__ __forceinline__ double dwa_choose(Human human, int M, double px, double py, double theta, double v, double r,
                                             double gx, double gy, double vpref, double dt, const cn_dwa_params &p,
                                             int lane, int &best)
{
    const int H = p.horizon;
    const double dv = dwa_grid(lane >> 3), dth = dwa_grid(lane & 7);
    const double sv = v + dv;
    const double v1 = sv < -vpref ? -vpref : (sv > vpref ? vpref : sv);
    const double R = ddiv(v1, ddiv(dth, dt));
    const double cx = px - R * sin(theta), cy = py + R * cos(theta);   // the arc's centre
    double cmin = __builtin_inf(), gterm = 0.0;
    int hit = 0;
    bool go = true;
    for (int k = 1; k <= H; ++k) {
        const double phi = theta + (double)k * dth;
        const double x = cx + R * sin(phi), y = cy - R * cos(phi);
        const double kt = (double)k * dt;
        double ck = __builtin_inf();
        for (int i = 0; i < M; ++i) {
            double bx, by, bvx, bvy, br;
            human(i, bx, by, bvx, bvy, br);
            const double ddx = x - (bx + kt * bvx), ddy = y - (by + kt * bvy);
            const double c = dsqrt(ddx * ddx + ddy * ddy) - r - br;
            ck = c < ck ? c : ck;
        }
        const double gdx = x - gx, gdy = y - gy;
        const double gk = dsqrt(gdx * gdx + gdy * gdy);
        if (go) {
            cmin = ck < cmin ? ck : cmin;
            if (ck < 0.0 && hit == 0) hit = H + 1 - k;
            gterm = gk;
            if (gk < r) { gterm = 0.0; go = false; }
        }
    }
    const double short_of = p.d_safe - cmin;
    const double J = (p.w_goal * gterm + ddiv(p.w_clear * (short_of > 0.0 ? short_of : 0.0), p.d_safe))
                     + p.w_col * (double)hit;
    double bj = J;
    int bc = lane;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oj = __shfl_xor(bj, m, 64);
        const int oc = __shfl_xor(bc, m, 64);
        if (oj < bj || (oj == bj && oc < bc)) { bj = oj; bc = oc; }
    }
    best = bc;
    return J;
}

// cn_dwa_predict: the controller on caller-given arrays, env i on wave i
__global__ void __launch_bounds__(64 * CN_DWA_WAVES) cn_dwa_predict_kernel(int64_t n, int M, const double *__restrict__ self,
                                                                          const double *__restrict__ v,
                                                                          const double *__restrict__ others, double dt,
                                                                          cn_dwa_params p, float *__restrict__ actions,
                                                                          int32_t *__restrict__ choice,
                                                                          double *__restrict__ costs)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * CN_DWA_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= n) return;
    const double *s = self + 9 * i;   // px, py, vx, vy, radius, gx, gy, v_pref, theta
    const double *o = others + i * M * 5;
    int best;
    const double J = dwa_choose(
        [&](int k, double &bx, double &by, double &bvx, double &bvy, double &br) {
            bx = o[5 * k]; by = o[5 * k + 1]; bvx = o[5 * k + 2]; bvy = o[5 * k + 3]; br = o[5 * k + 4];
        },
        M, s[0], s[1], s[8], v[i], s[4], s[5], s[6], s[7], dt, p, lane, best);
    if (costs) costs[64 * i + lane] = J;
    if (lane == 0) {
        actions[2 * i] = (float)dwa_grid(best >> 3); actions[2 * i + 1] = (float)dwa_grid(best & 7);
        if (choice) choice[i] = best;
    }
}

// cn_robot_act's: the controller on the engine's state, read in place (the robot's FullState with v = r_dv and the N
// belief humans); a plain kernel and the twin of a mixed engine's group, whose action goes to row rows[e]
// REGRET (cn_robot_act_regret's two kernels, at the end of this file): every lane also stores its candidate's regret
// (float)(J - J_best) to row o of `regret`, one coalesced 256-byte store per wave. J_best is the chosen lane's own J,
// read by one shuffle at the wave-uniform `best` (every lane of the wave is active: the wave past the last env left
// whole above), so the chosen lane subtracts its J from itself: +0.0 exactly. Without REGRET nothing is added.
template <bool MIX, bool REGRET>
__device__ __forceinline__ void robot_dwa_body(const cn_state_ptrs &S, int E, int N, double dt, const cn_dwa_params &p,
                                               float *__restrict__ actions, const int32_t *__restrict__ rows,
                                               float *__restrict__ regret)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * CN_DWA_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (e >= E) return;
    const int64_t h0 = e * N;
    int best;
    const double J = dwa_choose(
        [&](int k, double &bx, double &by, double &bvx, double &bvy, double &br) {
            bx = S.b_px[h0 + k]; by = S.b_py[h0 + k]; bvx = S.b_vx[h0 + k]; bvy = S.b_vy[h0 + k]; br = S.b_r[h0 + k];
        },
        N, S.r_px[e], S.r_py[e], S.r_theta[e], S.r_dv[e], S.r_radius[e], S.r_gx[e], S.r_gy[e], S.r_vpref[e], dt, p, lane,
        best);
    if (REGRET) {
        const int64_t o = MIX ? (int64_t)rows[e] : e;
        regret[64 * o + lane] = (float)(J - __shfl(J, best, 64));
    }
    if (lane == 0) {
        const int64_t o = MIX ? (int64_t)rows[e] : e;
        actions[2 * o] = (float)dwa_grid(best >> 3); actions[2 * o + 1] = (float)dwa_grid(best & 7);
    }
}
__global__ void __launch_bounds__(64 * CN_DWA_WAVES) cn_robot_dwa_kernel(cn_state_ptrs S, int E, int N, double dt,
                                                                        cn_dwa_params p, float *__restrict__ actions)
{
    robot_dwa_body<false, false>(S, E, N, dt, p, actions, nullptr, nullptr);
}
__global__ void __launch_bounds__(64 * CN_DWA_WAVES) cn_robot_dwa_mix_kernel(cn_state_ptrs S, int E, int N, double dt,
                                                                            cn_dwa_params p, float *__restrict__ actions,
                                                                            const int32_t *__restrict__ rows)
{
    robot_dwa_body<true, false>(S, E, N, dt, p, actions, rows, nullptr);
}

// cn_rollout_noisy outside the fused launches: the perturbation between cn_robot_act's kernel and the step. `act` is
// the clean row the robot kernel wrote, `x` the engine's (E, 2) scratch the step reads, `executed` the caller's row
// or null; rollout_noise's arithmetic, one lane per env. A group of a mixed engine (`rows`; null: the identity)
// works on its envs' rows of the three buffers, all of the mixed engine's E rows, and keys the noise by the row: the
// global env index, as the fused launches do.
__global__ void __launch_bounds__(64) cn_action_noise_kernel(const float *__restrict__ act, float *__restrict__ x,
                                                             float *__restrict__ executed, int E, float sigma,
                                                             uint32_t seed, uint32_t k, uint32_t G0,
                                                             const int32_t *__restrict__ rows)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t o = rows ? (int64_t)rows[e] : (int64_t)e;
    float x0, x1;
    rollout_noise(sigma, seed, k, G0 + (uint32_t)o, act[2 * o], act[2 * o + 1], x0, x1);
    x[2 * o] = x0; x[2 * o + 1] = x1;
    if (executed) { executed[2 * o] = x0; executed[2 * o + 1] = x1; }
}

// cn_rollout_noisy's device block for the fused launches that follow on the stream (a kernel for the reason
// cn_ctl_set_kernel is one)
__global__ void cn_noise_set_kernel(RolloutNoise *w, RolloutNoise v)
{
    if (threadIdx.x == 0) *w = v;
}

// cn_robot_mix: the coin between the learner's action and the controller's label, one lane per env of all E rows (a
// mixed engine: after the groups' join, its rows are the global order already). `ctl` is the caller's device block:
// the address is a kernel argument, so the three words arrive as wave-uniform (scalar) loads; only t is baked
// into a captured launch. The coin is word z of rollout_noise's Philox block (x and y are the noise's), the pairs
// move as 8-byte words (bits, no arithmetic). No LDS, no cross-lane reads, no barrier.
__global__ void __launch_bounds__(256) cn_robot_mix_kernel(const uint2 *__restrict__ learner,
                                                           const cn_mix_ctl *__restrict__ ctl, int32_t t, uint32_t G0,
                                                           int E, const uint2 *__restrict__ label,
                                                           uint2 *__restrict__ executed, uint8_t *__restrict__ flags)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const float beta = ctl->beta;
    const uint32_t seed = ctl->seed, k = (uint32_t)(uint64_t)(ctl->step0 + t);
    const uint4 w = philox4x32_10(k, seed, G0 + (uint32_t)e);
    const float u = (float)(w.z >> 8) * 5.9604644775390625e-08f;   // 2^-24: exact, in [0, 1)
    const bool took = u < beta;
    const uint2 l = label[e], a = learner[e];
    executed[e] = took ? l : a;
    flags[e] = (uint8_t)((took ? 1u : 0u) | ((l.x == a.x && l.y == a.y) ? 2u : 0u));
}

// cn_mix_ctl_set: the caller's device block from the stream (a kernel for the reason cn_ctl_set_kernel is one)
__global__ void cn_mix_ctl_set_kernel(cn_mix_ctl *w, cn_mix_ctl v)
{
    if (threadIdx.x == 0) *w = v;
}

// cn_rollout_lidar's device block for the fused launches that follow on the stream
__global__ void cn_rows_set_kernel(RolloutRows *w, RolloutRows v)
{
    if (threadIdx.x == 0) *w = v;
}

// cn_rollout_lidar outside the fused launches: the state a step (a launch pair or triple) left, copied to row
// row_e / E of the state rows. A workgroup per 64 consecutive envs, state_rows_copy as in the recording step kernel.
__global__ void __launch_bounds__(256) cn_state_rows_kernel(cn_state_ptrs S, RolloutRows R, int E, int N, int64_t row_e)
{
    const int e0 = blockIdx.x * 64;
    state_rows_copy(S, R, E, N, row_e, e0, min(64, E - e0), threadIdx.x, 256);
}

// cn_rollout_noisy at sigma == 0: `executed` is a copy of `actions` (bits, no arithmetic); n words
__global__ void __launch_bounds__(256) cn_copy32_kernel(int64_t n, const uint32_t *__restrict__ src,
                                                        uint32_t *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// One control word of the engine set from the stream (graph mode's draw-all flag after cn_reset /
// cn_set_state). A kernel, not hipMemsetAsync: captured into a hipGraph it is a kernel node, and this
// runtime replays memset nodes with stale bytes (cn_graph_node_counts).
__global__ void cn_ctl_set_kernel(uint32_t *w, uint32_t v)
{
    if (threadIdx.x == 0) *w = v;
}

// Key snapshot for a PEND_BOTH launch (after cn_set_state): every env's
// {e, reset_count, case_counter lo, hi} into the spawn list the next step launch reads (kr = (t + 2) % 3 for
// launch t: the host's sequence number, or graph mode's device word). That launch's spawn waves key both of an
// env's pending spawns from this entry, not from the state its own step workgroups rewrite when a terminal env
// resets inline (crowd_sim_dict.py:147-164: the seed of the k-th reset is offset + case_counter + thisSeed).
__global__ void cn_keysnap_kernel(const int32_t *__restrict__ reset_count, const int64_t *__restrict__ case_counter,
                                  uint32_t *plist_base, const uint32_t *ctl, int host_kr, int E)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t kr = host_kr >= 0 ? host_kr : (int64_t)((ctl[CN_CTL_NSTEP] + 2u) % 3u);
    uint32_t *q = plist_base + kr * 4 * ((int64_t)E + 64) + 4 * (int64_t)e;
    const uint64_t cc = (uint64_t)case_counter[e];
    const uint4 v = make_uint4((uint32_t)e, (uint32_t)reset_count[e], (uint32_t)cc, (uint32_t)(cc >> 32));
    *(uint4 *)q = v;
}

// ------------------------------------------------------------------------------------------------
// cn_visible_mask: which humans the robot sees in the state the engine now holds, one lane per (env, slot of the
// padded stride NS). It is the decision the step made when it wrote that state's belief -- human_post's in phase 4 of
// cn_step_kernel once the robot carries its float32 state (CN_FLAG_ROBOT_F32: heading atan2f of the float32 velocity
// for a holonomic robot, the float32 r_theta for a unicycle), write_reset's float64 path before that -- recomputed
// from the blob's r_px, r_py, r_vx, r_vy, r_theta, flags, h_px, h_py with the same device functions on the same
// words, so the booleans are the step's by construction. The belief itself does not determine it: an invisible human
// that keeps its velocity is extrapolated exactly. A group of a mixed engine (MIX) writes its envs' rows rows[e] of the
// caller's [E][NS] buffer, the padded slots k >= N as 0. No LDS, no cross-lane reads, no barrier.
// ------------------------------------------------------------------------------------------------
template <bool MIX>
__global__ void __launch_bounds__(64) cn_visible_mask_kernel(cn_state_ptrs S, int E, int N, int NS, int holo, double fov,
                                                             double cth, float *__restrict__ mask,
                                                             const int32_t *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = i / NS;
    if (e >= E) return;
    const int k = (int)(i - e * NS);
    const int64_t o = MIX ? (int64_t)rows[e] : e;
    mask[o * NS + k] = visible_mask_slot(S, e, k, N, holo, fov, cth);   // (robot.h: the rollout kernels' too)
}

// ------------------------------------------------------------------------------------------------
// cn_robot_act_regret's: cn_robot_dwa_kernel / cn_robot_dwa_mix_kernel with the regret row beside the action
// (robot_dwa_body with REGRET: the same dwa_choose, so the action is the plain kernels' bit for bit). The wave of env
// e (a group of a mixed engine: of row rows[e]) writes the 64 floats regret[64 * row .. 64 * row + 63] and nothing
// else of that buffer. The shape rules are the controller's: a wave past the last env leaves whole before any
// cross-lane read; no LDS, no atomics, no barrier. Last in the file: the kernels above keep their places in the
// code object.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * CN_DWA_WAVES) cn_robot_dwa_regret_kernel(cn_state_ptrs S, int E, int N, double dt,
                                                                               cn_dwa_params p,
                                                                               float *__restrict__ actions,
                                                                               float *__restrict__ regret)
{
    robot_dwa_body<false, true>(S, E, N, dt, p, actions, nullptr, regret);
}
__global__ void __launch_bounds__(64 * CN_DWA_WAVES) cn_robot_dwa_regret_mix_kernel(cn_state_ptrs S, int E, int N,
                                                                                   double dt, cn_dwa_params p,
                                                                                   float *__restrict__ actions,
                                                                                   const int32_t *__restrict__ rows,
                                                                                   float *__restrict__ regret)
{
    robot_dwa_body<true, true>(S, E, N, dt, p, actions, rows, regret);
}
