// orca_lp.h -- RVO2's linear programs in float32 (lines in LDS: lp1/2/3_q; in registers: lp1/2_r, lp3_sub / _r /
// _tasks / _replay) and the ORCA lines themselves (orca_line, orca_lines_quad). Needs cn_math.h, wsync and quad.h.
#pragma once

// ------------------------------------------------------------------------------------------------
// RVO2 v2.0 agent-0 solve (float32) with ORCA lines in LDS ([line][lane] float4: point.xy, dir.xy)
// ------------------------------------------------------------------------------------------------
#define RVO_EPSILON 0.00001f

__device__ inline float det2(float ax, float ay, float bx, float by) { return ax * by - ay * bx; }

// a / b, IEEE-rounded, for the linear programs' quotients: |b| > RVO_EPSILON (the callers ignore the
// quotient when |b| <= RVO_EPSILON, RVO2's parallel-line branch) and |b| <= 2 (determinants of unit
// direction vectors). This is the compiler's correctly rounded f32 division (v_div_scale, rcp, one
// reciprocal and two quotient refinements by FMA, v_div_fmas, v_div_fixup) without the steps that are
// identities on that domain: v_div_scale only rescales a denormal divisor or an exponent gap of >= 96
// (so VCC = 0 and v_div_fmas is a plain FMA), and v_div_fixup only rewrites zero / inf / NaN operands and
// over/underflowed quotients. The FMA residuals a - b*q are exact only while they stay above the denormal
// range, i.e. for |a| >= ~2^-100: a numerator below 2^-96 (zero included) takes the full division instead
// (a rarely taken branch). tools/fdiv_lp_check.hip compares this with `/` bit for bit over numerators of
// every exponent (denormals included) and that divisor domain.
__device__ __forceinline__ float fdiv_lp(float a, float b)
{
    if (__builtin_expect(__builtin_fabsf(a) < 0x1p-96f, 0)) return a / b;
    const float y0 = __builtin_amdgcn_rcpf(b);
    const float y1 = __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0);
    const float q0 = a * y1;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-b, q0, a), y1, q0);
    return __builtin_fmaf(__builtin_fmaf(-b, q1, a), y1, q1);
}

// projected line of LP3's line li against lj (`valid` false when RVO2 skips it: parallel, same direction)
__device__ __forceinline__ float4 proj_line(const float4 li, const float4 lj, bool &valid)
{
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    const float determinant = det2(li.z, li.w, lj.z, lj.w);
    valid = true;
    if (fabsf(determinant) <= RVO_EPSILON) {
        if (li.z * lj.z + li.w * lj.w > 0.0f) { valid = false; return r; }
        r.x = 0.5f * (li.x + lj.x);
        r.y = 0.5f * (li.y + lj.y);
    } else {
        const float s = fdiv_lp(det2(lj.z, lj.w, li.x - lj.x, li.y - lj.y), determinant);
        r.x = li.x + s * li.z;
        r.y = li.y + s * li.w;
    }
    const float ddx = lj.z - li.z, ddy = lj.w - li.w;
    const float inv = fdiv(1.0f, fsqrt(ddx * ddx + ddy * ddy));
    r.z = ddx * inv; r.w = ddy * inv;
    return r;
}

// ------------------------------------------------------------------------------------------------
// ORCA linear programs on a QUAD of lanes per human (A <= 10). The lines live in LDS ([human][M]);
// every quad-uniform quantity (the result, loop indices, branch conditions) is computed redundantly by
// the 4 lanes, and the inner loop of linearProgram1 over the earlier lines is split across them: lane s
// takes lines s, s+4, ... and the quad combines tLeft = max, tRight = min and the parallel-line failure.
// tLeft only grows and tRight only shrinks in RVO2's sequential loop, and its exits ("tLeft > tRight",
// "parallel line with numerator < 0") are order independent, so the combined result is RVO2's.
// ------------------------------------------------------------------------------------------------

// linearProgram1 on line `no` of Lb (valid lines: bits of vmask), quad-cooperative. MT: the line mask type
// (uint32_t: <= 32 lines, the step kernel; uint64_t: <= 64, the plugin's large simulators)
template <typename MT = uint32_t>
__device__ __forceinline__ bool lp1_q(const float4 *Lb, MT vmask, int no, float radius, int s, float &tL,
                                      float &tR)
{
    const float4 ln = Lb[no];
    const float dot = ln.x * ln.z + ln.y * ln.w;
    const float disc = dot * dot + radius * radius - (ln.x * ln.x + ln.y * ln.y);
    const float sd = fsqrt(disc);
    float ptl = -INFINITY, ptr = INFINITY;
    for (int j = s; j < no; j += 4) {
        if (!((vmask >> j) & (MT)1)) continue;
        const float4 li = Lb[j];
        const float den = det2(ln.z, ln.w, li.z, li.w);
        const float num = det2(li.z, li.w, ln.x - li.x, ln.y - li.y);
        const bool par = fabsf(den) <= RVO_EPSILON;
        const float t = fdiv_lp(num, den);
        if (!par && den >= 0.0f && t < ptr) ptr = t;
        if (!par && !(den >= 0.0f) && ptl < t) ptl = t;
        if (par && num < 0.0f) ptl = INFINITY;   // RVO2's parallel-line failure (as in lp1_r)
    }
    ptr = quad_min(ptr);
    ptl = quad_max(ptl);
    float tr = -dot + sd, tl = -dot - sd;
    tr = ptr < tr ? ptr : tr;
    tl = tl < ptl ? ptl : tl;
    tL = tl; tR = tr;
    return !(disc < 0.0f || tl > tr);
}

// linearProgram2 (optimize closest to (ox, oy)); returns the index of the failing line or n
template <typename MT = uint32_t>
__device__ __forceinline__ int lp2_q(const float4 *Lb, int n, float radius, float ox, float oy, int s, float &rx,
                                     float &ry)
{
    if (ox * ox + oy * oy > radius * radius) {
        const float inv = fdiv(1.0f, fsqrt(ox * ox + oy * oy));
        rx = (ox * inv) * radius; ry = (oy * inv) * radius;
    } else { rx = ox; ry = oy; }
    for (int i = 0; i < n; ++i) {
        const float4 li = Lb[i];
        if (det2(li.z, li.w, li.x - rx, li.y - ry) > 0.0f) {
            float tL, tR;
            if (!lp1_q<MT>(Lb, ~(MT)0, i, radius, s, tL, tR)) return i;
            const float t = li.z * (ox - li.x) + li.w * (oy - li.y);
            if (t < tL) { rx = li.x + tL * li.z; ry = li.y + tL * li.w; }
            else if (t > tR) { rx = li.x + tR * li.z; ry = li.y + tR * li.w; }
            else { rx = li.x + t * li.z; ry = li.y + t * li.w; }
        }
    }
    return n;
}

// linearProgram3 from line `begin` (agents only); Pb = the human's projected-line scratch
template <typename MT = uint32_t>
__device__ __forceinline__ void lp3_q(const float4 *Lb, float4 *Pb, int n, int begin, float radius, int s, float &rx,
                                      float &ry)
{
    float distance = 0.0f;
    for (int i = begin; i < n; ++i) {
        const float4 li = Lb[i];
        if (det2(li.z, li.w, li.x - rx, li.y - ry) > distance) {
            MT pv = 0;
            for (int j = s; j < i; j += 4) {
                bool v;
                const float4 pj = proj_line(li, Lb[j], v);
                Pb[j] = pj;
                if (v) pv |= (MT)1 << j;
            }
            pv = quad_or_m(pv);
            wsync();
            const float tx = rx, ty = ry;
            const float ox = -li.w, oy = li.z;   // linearProgram2(projLines, radius, (-d.y, d.x), true)
            rx = ox * radius; ry = oy * radius;
            bool fail = false;
            for (int k = 0; k < i && !fail; ++k) {
                if (!((pv >> k) & (MT)1)) continue;
                const float4 pk = Pb[k];
                if (det2(pk.z, pk.w, pk.x - rx, pk.y - ry) > 0.0f) {
                    float tL, tR;
                    if (!lp1_q<MT>(Pb, pv, k, radius, s, tL, tR)) fail = true;
                    else if (ox * pk.z + oy * pk.w > 0.0f) { rx = pk.x + tR * pk.z; ry = pk.y + tR * pk.w; }
                    else { rx = pk.x + tL * pk.z; ry = pk.y + tL * pk.w; }
                }
            }
            if (fail) { rx = tx; ry = ty; }
            distance = det2(li.z, li.w, li.x - rx, li.y - ry);
            wsync();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same linear programs with the lines in REGISTERS (quad path, <= 4 * NU lines): lane s of the quad
// holds lines s, s+4, ..., s+4(NU-1) (R[u] = line s + 4u) and line i reaches the whole quad by a DPP
// quad_perm broadcast from lane i & 3 -- the loops over lines are unrolled, so every broadcast has a
// compile-time source lane and no LDS round trip sits on the linear programs' dependent chain. Same
// operations in the same order as lp1_q / lp2_q / lp3_q, so the same bits.
// ------------------------------------------------------------------------------------------------

// -DCN_STAMPS: the linearProgram1 bodies a quad's linear program ran (count, and their line indices as a mask).
// A wave runs the unrolled forms' body of index i when any of its quads does (lp_count_wave's `uni`: distinct
// indices over the wave) and a walk's body once per trip (`mx`: the largest count of one quad).
#ifdef CN_STAMPS
struct LpCount { int bodies; uint32_t lines; };
#define LP_COUNT_ARG , LpCount *lc = nullptr
#define LP_COUNT(i) do { if (lc) { ++lc->bodies; lc->lines |= 1u << (i); } } while (0)
__device__ __forceinline__ void lp_count_wave(const LpCount &lc, int &uni, int &mx)   // over the active lanes
{
    int m = 0;
    for (int k = 0; k < 12; ++k) {
        if (__ballot((lc.lines >> k) & 1u)) ++uni;
        if (__ballot(lc.bodies > k)) m = k + 1;
    }
    mx += m;
}
#else
#define LP_COUNT_ARG
#define LP_COUNT(i) do { } while (0)
#endif

// linearProgram1 on line `no` (= ln, already broadcast) against the valid (vmask) lines j < no of R
template <int NU>
__device__ __forceinline__ bool lp1_r(const float4 (&R)[NU], uint32_t vmask, int no, const float4 ln, float radius,
                                      int s, float &tL, float &tR)
{
    const float dot = ln.x * ln.z + ln.y * ln.w;
    const float disc = dot * dot + radius * radius - (ln.x * ln.x + ln.y * ln.y);
    const float sd = fsqrt(disc);
    float ptl = -INFINITY, ptr = INFINITY;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int j = s + 4 * u;
        if (j < no && ((vmask >> j) & 1u)) {
            const float4 li = R[u];
            const float den = det2(ln.z, ln.w, li.z, li.w);
            const float num = det2(li.z, li.w, ln.x - li.x, ln.y - li.y);
            const bool par = fabsf(den) <= RVO_EPSILON;
            const float t = fdiv_lp(num, den);
            if (!par && den >= 0.0f && t < ptr) ptr = t;
            if (!par && !(den >= 0.0f) && ptl < t) ptl = t;
            // RVO2 fails on a parallel line with numerator < 0: tLeft = +inf (> any tRight, t is finite)
            // fails the same test below, and rides the max reduction instead of a third quad reduction
            if (par && num < 0.0f) ptl = INFINITY;
        }
    }
    ptr = quad_min(ptr);
    ptl = quad_max(ptl);
    float tr = -dot + sd, tl = -dot - sd;
    tr = ptr < tr ? ptr : tr;
    tl = tl < ptl ? ptl : tl;
    tL = tl; tR = tr;
    return !(disc < 0.0f || tl > tr);
}

// linearProgram2 (optimize closest to (ox, oy)) over the n lines of R; returns the failing line or n.
// RVO2's loop acts only at a line the current result violates, and the result changes only there, so the lines a
// quad acts on are "the lowest index above the last one whose line the current result violates". The unrolled form
// (WALK false) steps through all indices in lockstep, and a wave runs linearProgram1 at index i when ANY of its 16
// quads has line i violated: the union of their indices. The walk (WALK true; Lb: the LDS copy of the lines) lets
// each quad jump to its own next violated line: per trip every lane tests its own lines against the result (the
// loop's own test, same operands), the quad ORs the bits, masks them to the indices above the last line acted on
// and takes the lowest; line i, a run-time index now, is read from Lb. A wave makes as many trips as its busiest
// quad has lines to act on (C2: 3.2 instead of 5.8 linearProgram1 bodies per wave and step). Every arithmetic
// operation of a quad is one the unrolled form performs, on the same operands in the same order: the same bits.
// The loop's control flow is quad-uniform (vm, i and the failure are), so every DPP runs with whole quads.
// The walk serves the instantiations its A/B measured: the plain multi-step step kernels and
// cn_debug_orca, through which tests/test_lp_walk.py pins it to the oracle; the others keep the unrolled form.
template <int NU, bool WALK = false>
__device__ __forceinline__ int lp2_r(const float4 (&R)[NU], int n, float radius, float ox, float oy, int s, float &rx,
                                     float &ry, const float4 *Lb = nullptr LP_COUNT_ARG)
{
    if (ox * ox + oy * oy > radius * radius) {
        const float inv = fdiv(1.0f, fsqrt(ox * ox + oy * oy));
        rx = (ox * inv) * radius; ry = (oy * inv) * radius;
    } else { rx = ox; ry = oy; }
    int fail = n;
    if constexpr (WALK) {
        uint32_t above = ~0u;   // the indices above the last line acted on
        for (;;) {
            uint32_t vm = 0;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const float4 lu = R[u];
                if (s + 4 * u < n && det2(lu.z, lu.w, lu.x - rx, lu.y - ry) > 0.0f) vm |= 1u << (s + 4 * u);
            }
            vm = (uint32_t)quad_or((int)vm) & above;
            if (vm == 0) break;   // quad-uniform: no line left
            const int i = __ffs(vm) - 1;
            above = ~1u << i;
            const float4 li = Lb[i];
            LP_COUNT(i);
            float tL, tR;
            if (!lp1_r<NU>(R, ~0u, i, li, radius, s, tL, tR)) { fail = i; break; }
            const float t = li.z * (ox - li.x) + li.w * (oy - li.y);
            if (t < tL) { rx = li.x + tL * li.z; ry = li.y + tL * li.w; }
            else if (t > tR) { rx = li.x + tR * li.z; ry = li.y + tR * li.w; }
            else { rx = li.x + t * li.z; ry = li.y + t * li.w; }
        }
        return fail;
    }
#pragma unroll
    for (int i = 0; i < 4 * NU; ++i) {
        if (i < n && fail == n) {   // quad-uniform
            const float4 li = qbc4(R[i >> 2], i);
            if (det2(li.z, li.w, li.x - rx, li.y - ry) > 0.0f) {
                float tL, tR;
                LP_COUNT(i);
                if (!lp1_r<NU>(R, ~0u, i, li, radius, s, tL, tR)) fail = i;
                else {
                    const float t = li.z * (ox - li.x) + li.w * (oy - li.y);
                    if (t < tL) { rx = li.x + tL * li.z; ry = li.y + tL * li.w; }
                    else if (t > tR) { rx = li.x + tR * li.z; ry = li.y + tR * li.w; }
                    else { rx = li.x + t * li.z; ry = li.y + t * li.w; }
                }
            }
        }
    }
    return fail;
}

// RVO2 linearProgram3's sub-problem for line i: linearProgram2 over the projections of lines 0..i-1 onto
// line i (R: lane s holds lines s + 4u), optimising direction (-d.y, d.x) from result = opt * radius.
// Depends on the lines only. Returns false when it fails (RVO2 then keeps the result it had).
template <int NU>
__device__ __forceinline__ bool lp3_sub(const float4 (&R)[NU], const float4 li, int i, float radius, int s, float &rx,
                                        float &ry LP_COUNT_ARG)
{
    float4 P[NU];
    uint32_t pv = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int j = s + 4 * u;
        P[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < i) {
            bool v;
            P[u] = proj_line(li, R[u], v);
            if (v) pv |= 1u << j;
        }
    }
    pv = (uint32_t)quad_or((int)pv);
    const float ox = -li.w, oy = li.z;   // linearProgram2(projLines, radius, (-d.y, d.x), true)
    rx = ox * radius; ry = oy * radius;
    bool fail = false;
#pragma unroll
    for (int k = 0; k < 4 * NU; ++k) {
        if (k < i && !fail && ((pv >> k) & 1u)) {   // quad-uniform
            const float4 pk = qbc4(P[k >> 2], k);
            if (det2(pk.z, pk.w, pk.x - rx, pk.y - ry) > 0.0f) {
                float tL, tR;
                LP_COUNT(k);
                if (!lp1_r<NU>(P, pv, k, pk, radius, s, tL, tR)) fail = true;
                else if (ox * pk.z + oy * pk.w > 0.0f) { rx = pk.x + tR * pk.z; ry = pk.y + tR * pk.w; }
                else { rx = pk.x + tL * pk.z; ry = pk.y + tL * pk.w; }
            }
        }
    }
    return !fail;
}

// linearProgram3 from line `begin`; Lb = the same lines in LDS (line i of the outer loop is read from
// there: its index is dynamic), the projected lines stay in registers (lane s: j = s + 4u)
template <int NU>
__device__ __forceinline__ void lp3_r(const float4 (&R)[NU], const float4 *Lb, int n, int begin, float radius, int s,
                                      float &rx, float &ry)
{
    float distance = 0.0f;
    for (int i = begin; i < n; ++i) {
        const float4 li = Lb[i];
        if (det2(li.z, li.w, li.x - rx, li.y - ry) > distance) {
            float qx, qy;
            if (lp3_sub<NU>(R, li, i, radius, s, qx, qy)) { rx = qx; ry = qy; }
            distance = det2(li.z, li.w, li.x - rx, li.y - ry);
        }
    }
}

// The linearProgram3 sub-problems of a whole workgroup, spread over all its quads (the quad path's step
// kernel). Sub-problem (h, i) -- human h's line i -- depends on h's lines only, not on the result RVO2's
// loop has reached when it visits line i, so every one that the loop may visit (i in [fail, n) of each
// human whose linearProgram2 failed at `fail`) is solved up front, by any quad: sorted by i (descending),
// so the 16 quads of a wave run sub-problems of about the same size side by side, and one human's
// sub-problems run on different quads at once. Each human's quad then replays RVO2's loop (lp3_replay).
// The serial version puts a human's whole loop on its own quad, and the wave runs the union of its 16
// humans' control flow: for crowded circle crossings that was half of the C2 launch.
// bn[h] = fail | n << 8 (0: no linearProgram3); results to res / rok [h][12].
template <int NU>
__device__ __forceinline__ void lp3_tasks(const float4 *lines, int M, const float *vmax, const uint32_t *bn,
                                          float2 *res, uint8_t *rok, int tid LP_COUNT_ARG)
{
    const int q = tid >> 2, sq = tid & 3;
    const uint32_t b = bn[tid & 63];
    const int b0 = (int)(b & 0xffu), b1 = (int)(b >> 8);
    uint64_t mk[4 * NU];
    int cn[4 * NU], T = 0;
#pragma unroll
    for (int i = 0; i < 4 * NU; ++i) {   // humans with sub-problem i (wave-uniform)
        mk[i] = __ballot(b0 <= i && i < b1);
        cn[i] = __popcll(mk[i]);
        T += cn[i];
    }
    for (int t = q; t < T; t += 64) {   // quad-uniform
        int i = 0, k = 0, acc = 0;
        uint64_t m = 0;
        bool found = false;
#pragma unroll
        for (int ii = 4 * NU - 1; ii >= 0; --ii) {
            if (!found && t < acc + cn[ii]) { found = true; i = ii; k = t - acc; m = mk[ii]; }
            acc += cn[ii];
        }
        for (int z = 0; z < k; ++z) m &= m - 1;   // the k-th human with sub-problem i
        const int h = __ffsll((long long)m) - 1;
        const float4 *Lh = lines + h * M;
        float4 R[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) R[u] = sq + 4 * u < i ? Lh[sq + 4 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
        float qx, qy;
#ifdef CN_STAMPS
        LpCount l1 = {0, 0};   // per round: lc->bodies += its distinct indices | largest quad count << 12 | 1 << 24
        const bool ok = lp3_sub<NU>(R, Lh[i], i, vmax[h], sq, qx, qy, &l1);
        int uni = 0, mx = 0;
        lp_count_wave(l1, uni, mx);
        if (lc) lc->bodies += uni | mx << 12 | 1 << 24;
#else
        const bool ok = lp3_sub<NU>(R, Lh[i], i, vmax[h], sq, qx, qy);
#endif
        if (sq == 0) { res[h * 12 + i] = make_float2(qx, qy); rok[h * 12 + i] = ok ? 1 : 0; }
    }
}

// RVO2's linearProgram3 loop over the sub-problems lp3_tasks solved (lines < `end`), quad-uniform; a visited
// line >= end has its sub-problem solved here, by the human's own quad (R: its lines, lane s: s + 4u)
template <int NU>
__device__ __forceinline__ int lp3_replay(const float4 (&R)[NU], const float4 *Lb, int n, int begin, int end,
                                          float radius, int s, const float2 *res, const uint8_t *rok, float &rx,
                                          float &ry)
{
    float distance = 0.0f;
    int vis = 0;
    for (int i = begin; i < n; ++i) {
        const float4 li = Lb[i];
        if (det2(li.z, li.w, li.x - rx, li.y - ry) > distance) {
            ++vis;
            if (i < end) {
                if (rok[i]) { const float2 r2 = res[i]; rx = r2.x; ry = r2.y; }
            } else {
                float qx, qy;
                if (lp3_sub<NU>(R, li, i, radius, s, qx, qy)) { rx = qx; ry = qy; }
            }
            distance = det2(li.z, li.w, li.x - rx, li.y - ry);
        }
    }
    return vis;
}

// one ORCA line (Agent::computeNewVelocity, agent branch) of self vs another agent
__device__ __forceinline__ float4 orca_line(float X0, float Y0, float VX0, float VY0, float R0, float ox, float oy,
                                           float ovx, float ovy, float orr, float invTH, float invTS)
{
    const float rpx = ox - X0, rpy = oy - Y0;
    const float rvx = VX0 - ovx, rvy = VY0 - ovy;
    const float distSq = rpx * rpx + rpy * rpy;
    const float cr = R0 + orr;
    const float crSq = cr * cr;
    float ux, uy, dx, dy;
    if (distSq > crSq) {
        const float wx = rvx - invTH * rpx, wy = rvy - invTH * rpy;
        const float wLenSq = wx * wx + wy * wy;
        const float dot1 = wx * rpx + wy * rpy;
        if (dot1 < 0.0f && dot1 * dot1 > crSq * wLenSq) {
            const float wLen = fsqrt(wLenSq);
            const float inv = fdiv(1.0f, wLen);
            const float uwx = wx * inv, uwy = wy * inv;
            dx = uwy; dy = -uwx;
            const float s = cr * invTH - wLen;
            ux = s * uwx; uy = s * uwy;
        } else {
            const float leg = fsqrt(distSq - crSq);
            const float inv = fdiv(1.0f, distSq);
            if (det2(rpx, rpy, wx, wy) > 0.0f) {
                dx = (rpx * leg - rpy * cr) * inv;
                dy = (rpx * cr + rpy * leg) * inv;
            } else {
                dx = -((rpx * leg + rpy * cr) * inv);
                dy = -((-rpx * cr + rpy * leg) * inv);
            }
            const float dot2 = rvx * dx + rvy * dy;
            ux = dot2 * dx - rvx; uy = dot2 * dy - rvy;
        }
    } else {
        const float wx = rvx - invTS * rpx, wy = rvy - invTS * rpy;
        const float wLen = fsqrt(wx * wx + wy * wy);
        const float inv = fdiv(1.0f, wLen);
        const float uwx = wx * inv, uwy = wy * inv;
        dx = uwy; dy = -uwx;
        const float s = cr * invTS - wLen;
        ux = s * uwx; uy = s * uwy;
    }
    return make_float4(VX0 + 0.5f * ux, VY0 + 0.5f * uy, dx, dy);
}

// Agent::computeNeighbors + the agent loop of Agent::computeNewVelocity for a simulator of <= 13 agents
// (RVO2's KdTree is a single leaf for <= 10: the neighbours are the in-range slots stably sorted by distSq
// in slot order), quad-cooperative: lane sq builds the lines of slots sq, sq+4, sq+8 and ranks them itself
// against the quad's distances, gathered by DPP broadcasts (no LDS round trip).
// `slot(k, x, y, vx, vy, r)` gives observed slot k (agent k + 1) in float32. Lines land in Lb[rank].
// Returns the number of lines. Shared by cn_step_kernel and cn_debug_orca.
template <typename SlotF>
__device__ __forceinline__ int orca_lines_quad(const SlotF &slot, int M, int sq, float X0, float Y0, float VX0,
                                               float VY0, float R0, float rangeSq, float invTH, float invTS,
                                               float4 *Lb)
{
    float4 rawv[3];
    float dv[3];
    uint32_t inm = 0;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int k = sq + 4 * u;
        rawv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        dv[u] = 0.0f;
        if (k < M) {
            float x, y, vx, vy, r;
            slot(k, x, y, vx, vy, r);
            const float dx = X0 - x, dy = Y0 - y;
            dv[u] = dx * dx + dy * dy;
            if (dv[u] < rangeSq) inm |= 1u << k;
            rawv[u] = orca_line(X0, Y0, VX0, VY0, R0, x, y, vx, vy, r, invTH, invTS);
        }
    }
    inm = (uint32_t)quad_or((int)inm);
    float dq[12];   // distSq of slot q = 4u + t (lane t's dv[u]), broadcast with the whole quad active
#pragma unroll
    for (int q = 0; q < 12; ++q) dq[q] = qbcf(dv[q >> 2], q);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int k = sq + 4 * u;
        if (k < M && ((inm >> k) & 1u)) {
            int rank = 0;
#pragma unroll
            for (int q = 0; q < 12; ++q)
                if (((inm >> q) & 1u) && (dq[q] < dv[u] || (dq[q] == dv[u] && q < k))) ++rank;
            Lb[rank] = rawv[u];
        }
    }
    return __popc(inm);
}
