// spatial_attn.h -- the whole spatial-edge attention in one pass: cn_spatial_attn_fwd / _bwd kernels and their _var
// pair (a per-row human count). Needs nothing before it.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// Whole spatial-edge attention of EdgeAttention.forward (srnn_model.py:256-333) in one pass over hs:
//   score[r][n] = scale * sum_k te[r][k] (Ws hs[r][n] + bs)[k]  = scale * (hs[r][n] . u[r] + c[r]),
//   u = te Ws (R x H), c = te . bs (host GEMM / GEMV, R x A x H: 1/10 of the reference's R*N x H x A),
//   attn = softmax_n(score), out[r] = sum_n attn[r][n] hs[r][n].
// The reference materialises spatial_embed (R*N x 64), the product with temporal_embed and its sum,
// then reads hs again for the pooling; here hs is read once (the first 16 of a row's N vectors stay in
// registers between the score and pooling passes). Same quantity, reassociated (fp32 rounding level).
// One thread per (row, 4 consecutive h): HQ = H / 4 lanes per row, rows never straddle a wave; the
// row's scores go through LDS (lane 0 of the row writes, the row's lanes read after a barrier).
// ------------------------------------------------------------------------------------------------
#define CN_SA_MAXN 64
// NR: a row's first NR edge vectors stay in registers between the two passes (the rest are read again).
// Instantiated for NR = 10 (N <= 10: C4's rows; backward 79 instead of 103 VGPRs, 6 instead of 4 waves per
// SIMD: 2.05 -> 1.65 ms at C4's 262,144 x 10 x 256, 3.0 -> 3.75 TB/s; forward 0.90 -> 0.85 ms,
// tools/probe_attn.py) and NR = 16.

template <int HQ, int NR>
__global__ __launch_bounds__(256) void cn_spatial_attn_fwd_kernel(int64_t R, int N, float scale,
                                                                  const float *__restrict__ hs,
                                                                  const float *__restrict__ u,
                                                                  const float *__restrict__ c,
                                                                  float *__restrict__ out, float *__restrict__ attn)
{
    constexpr int H = HQ * 4, RB = 256 / HQ;
    __shared__ float sc[RB][CN_SA_MAXN];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / HQ;
    const int q = (int)(i - r * HQ), rl = (int)threadIdx.x / HQ;
    const bool ok = r < R;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 uu = ok ? *(const float4 *)(u + r * H + q * 4) : z4;
    const float cr = ok ? c[r] : 0.f;
    const float *hr = hs + (ok ? r : 0) * (int64_t)N * H + q * 4;
    float4 vc[NR];
    float mx = -INFINITY;
    auto score = [&](int n, const float4 &v) {
        float part = ((uu.x * v.x + uu.y * v.y) + uu.z * v.z) + uu.w * v.w;
#pragma unroll
        for (int o = HQ / 2; o; o >>= 1) part += __shfl_xor(part, o);
        const float s = (part + cr) * scale;
        if (q == 0) sc[rl][n] = s;
        mx = fmaxf(mx, s);
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < N) {
            vc[n] = ok ? *(const float4 *)(hr + n * H) : z4;
            score(n, vc[n]);
        }
    for (int n = NR; n < N; ++n) score(n, ok ? *(const float4 *)(hr + n * H) : z4);
    __syncthreads();
    float den = 0.f;
    for (int n = 0; n < N; ++n) den += expf(sc[rl][n] - mx);
    float4 acc = z4;
    auto pool = [&](int n, const float4 &v) {
        const float a = expf(sc[rl][n] - mx) / den;
        acc.x += v.x * a; acc.y += v.y * a; acc.z += v.z * a; acc.w += v.w * a;
        if (ok && q == 0) attn[r * N + n] = a;
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < N) pool(n, vc[n]);
    for (int n = NR; n < N; ++n) pool(n, ok ? *(const float4 *)(hr + n * H) : z4);
    if (ok) *(float4 *)(out + r * H + q * 4) = acc;
}

// Gradient: p[n] = dout[r] . hs[r][n] (+ the caller's d attn), s = sum_n attn[n] p[n],
// dscore[n] = scale * attn[n] (p[n] - s) (softmax backward), then
//   dhs[r][n] = attn[n] dout[r] + dscore[n] u[r],  du[r] = sum_n dscore[n] hs[r][n],  dc[r] = sum_n dscore[n].
// hs is read once (as forward); dhs written once (it is the spatial GRU output's whole gradient).
template <int HQ, int NR>
__global__ __launch_bounds__(256) void cn_spatial_attn_bwd_kernel(int64_t R, int N, float scale,
                                                                  const float *__restrict__ hs,
                                                                  const float *__restrict__ u,
                                                                  const float *__restrict__ attn,
                                                                  const float *__restrict__ dout,
                                                                  const float *__restrict__ dattn,
                                                                  float *__restrict__ dhs, float *__restrict__ du,
                                                                  int64_t ldu, float *__restrict__ dc, int64_t ldc)
{
    constexpr int H = HQ * 4, RB = 256 / HQ;
    __shared__ float sp[RB][CN_SA_MAXN];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / HQ;
    const int q = (int)(i - r * HQ), rl = (int)threadIdx.x / HQ;
    const bool ok = r < R;
    const int64_t rr = ok ? r : 0;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 g = ok ? *(const float4 *)(dout + r * H + q * 4) : z4;
    const float4 uu = ok ? *(const float4 *)(u + r * H + q * 4) : z4;
    const float *hr = hs + rr * (int64_t)N * H + q * 4;
    float4 vc[NR];
    float s = 0.f;
    auto grad = [&](int n, const float4 &v) {
        float part = ((g.x * v.x + g.y * v.y) + g.z * v.z) + g.w * v.w;
#pragma unroll
        for (int o = HQ / 2; o; o >>= 1) part += __shfl_xor(part, o);
        if (dattn) part += dattn[rr * N + n];
        if (q == 0) sp[rl][n] = part;
        s += attn[rr * N + n] * part;
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < N) {
            vc[n] = ok ? *(const float4 *)(hr + n * H) : z4;
            grad(n, vc[n]);
        }
    for (int n = NR; n < N; ++n) grad(n, ok ? *(const float4 *)(hr + n * H) : z4);
    __syncthreads();
    float4 acc = z4;
    float dcs = 0.f;
    float *dr = dhs + rr * (int64_t)N * H + q * 4;
    auto back = [&](int n, const float4 &v) {
        const float a = attn[rr * N + n];
        const float ds = scale * (a * (sp[rl][n] - s));
        acc.x += ds * v.x; acc.y += ds * v.y; acc.z += ds * v.z; acc.w += ds * v.w;
        dcs += ds;
        if (ok)
            *(float4 *)(dr + n * H) = make_float4(a * g.x + ds * uu.x, a * g.y + ds * uu.y, a * g.z + ds * uu.z,
                                                  a * g.w + ds * uu.w);
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < N) back(n, vc[n]);
    for (int n = NR; n < N; ++n) back(n, ok ? *(const float4 *)(hr + n * H) : z4);
    if (ok) {
        *(float4 *)(du + r * ldu + q * 4) = acc;
        if (q == 0) dc[r * ldc] = dcs;
    }
}

// ------------------------------------------------------------------------------------------------
// The same attention with a per-row human count (a policy over crowds of varying size; rows of a mixed
// engine are padded to the largest count): row r attends to its first count[r] of the N slots with its own
// temperature row_scale[r], and is computed as cn_spatial_attn_fwd / _bwd compute a row at N = count[r],
// scale = row_scale[r] -- the same operations in the same order, so a row of full count is today's row.
// attn[r][n] and dhs[r][n][:] of the padded slots n >= count[r] are written as zeros (by all of the row's
// lanes, one slot each per round); hs[r][n] and dattn[r][n] of those slots are never read.
// Mapping as above: HQ lanes per row, rows never straddle a wave, the first NR vectors in registers,
// scores through LDS. The loop bound is row-uniform instead of launch-uniform. Cross-lane reads: the
// __shfl_xor reductions use offsets < HQ, so a lane reads only lanes of its own row, and all HQ lanes of a
// row run the same trip count (cnt depends on r alone): every lane a reduction reads is active at that
// instruction, whatever the other rows of the wave do. The workgroup barrier is outside every loop and
// reached by all 256 threads. Rows past R get cnt = 0: no loads, no stores.
// ------------------------------------------------------------------------------------------------
template <int HQ, int NR>
__global__ __launch_bounds__(256) void cn_spatial_attn_var_fwd_kernel(int64_t R, int N,
                                                                      const int32_t *__restrict__ count,
                                                                      const float *__restrict__ row_scale,
                                                                      const float *__restrict__ hs,
                                                                      const float *__restrict__ u,
                                                                      const float *__restrict__ c,
                                                                      float *__restrict__ out,
                                                                      float *__restrict__ attn)
{
    constexpr int H = HQ * 4, RB = 256 / HQ;
    __shared__ float sc[RB][CN_SA_MAXN];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / HQ;
    const int q = (int)(i - r * HQ), rl = (int)threadIdx.x / HQ;
    const bool ok = r < R;
    // (the clamp keeps a count outside the caller's contract inside the row's own N slots)
    const int cnt = ok ? min(max(count[r], 0), N) : 0;
    const float scale = ok ? row_scale[r] : 0.f;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 uu = z4;
    if (ok) uu = *(const float4 *)(u + r * H + q * 4);
    const float cr = ok ? c[r] : 0.f;
    const float *hr = hs + (ok ? r : 0) * (int64_t)N * H + q * 4;
    float4 vc[NR];
    float mx = -INFINITY;
    auto score = [&](int n, const float4 &v) {
        float part = ((uu.x * v.x + uu.y * v.y) + uu.z * v.z) + uu.w * v.w;
#pragma unroll
        for (int o = HQ / 2; o; o >>= 1) part += __shfl_xor(part, o);
        const float s = (part + cr) * scale;
        if (q == 0) sc[rl][n] = s;
        mx = fmaxf(mx, s);
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < cnt) {
            vc[n] = *(const float4 *)(hr + n * H);
            score(n, vc[n]);
        }
    for (int n = NR; n < cnt; ++n) score(n, *(const float4 *)(hr + n * H));
    __syncthreads();
    float den = 0.f;
    for (int n = 0; n < cnt; ++n) den += expf(sc[rl][n] - mx);
    float4 acc = z4;
    auto pool = [&](int n, const float4 &v) {
        const float a = expf(sc[rl][n] - mx) / den;
        acc.x += v.x * a; acc.y += v.y * a; acc.z += v.z * a; acc.w += v.w * a;
        if (q == 0) attn[r * N + n] = a;
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < cnt) pool(n, vc[n]);
    for (int n = NR; n < cnt; ++n) pool(n, *(const float4 *)(hr + n * H));
    if (ok) {
        for (int n = cnt + q; n < N; n += HQ) attn[r * N + n] = 0.f;
        *(float4 *)(out + r * H + q * 4) = acc;
    }
}

template <int HQ, int NR>
__global__ __launch_bounds__(256) void cn_spatial_attn_var_bwd_kernel(int64_t R, int N,
                                                                      const int32_t *__restrict__ count,
                                                                      const float *__restrict__ row_scale,
                                                                      const float *__restrict__ hs,
                                                                      const float *__restrict__ u,
                                                                      const float *__restrict__ attn,
                                                                      const float *__restrict__ dout,
                                                                      const float *__restrict__ dattn,
                                                                      float *__restrict__ dhs, float *__restrict__ du,
                                                                      int64_t ldu, float *__restrict__ dc, int64_t ldc)
{
    constexpr int H = HQ * 4, RB = 256 / HQ;
    __shared__ float sp[RB][CN_SA_MAXN];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / HQ;
    const int q = (int)(i - r * HQ), rl = (int)threadIdx.x / HQ;
    const bool ok = r < R;
    const int64_t rr = ok ? r : 0;
    const int cnt = ok ? min(max(count[r], 0), N) : 0;
    const float scale = ok ? row_scale[r] : 0.f;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g = z4;
    if (ok) g = *(const float4 *)(dout + r * H + q * 4);
    float4 uu = z4;
    if (ok) uu = *(const float4 *)(u + r * H + q * 4);
    const float *hr = hs + rr * (int64_t)N * H + q * 4;
    float4 vc[NR];
    float s = 0.f;
    auto grad = [&](int n, const float4 &v) {
        float part = ((g.x * v.x + g.y * v.y) + g.z * v.z) + g.w * v.w;
#pragma unroll
        for (int o = HQ / 2; o; o >>= 1) part += __shfl_xor(part, o);
        if (dattn) part += dattn[rr * N + n];
        if (q == 0) sp[rl][n] = part;
        s += attn[rr * N + n] * part;
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < cnt) {
            vc[n] = *(const float4 *)(hr + n * H);
            grad(n, vc[n]);
        }
    for (int n = NR; n < cnt; ++n) grad(n, *(const float4 *)(hr + n * H));
    __syncthreads();
    float4 acc = z4;
    float dcs = 0.f;
    float *dr = dhs + rr * (int64_t)N * H + q * 4;
    auto back = [&](int n, const float4 &v) {
        const float a = attn[rr * N + n];
        const float ds = scale * (a * (sp[rl][n] - s));
        acc.x += ds * v.x; acc.y += ds * v.y; acc.z += ds * v.z; acc.w += ds * v.w;
        dcs += ds;
        *(float4 *)(dr + n * H) = make_float4(a * g.x + ds * uu.x, a * g.y + ds * uu.y, a * g.z + ds * uu.z,
                                              a * g.w + ds * uu.w);
    };
#pragma unroll
    for (int n = 0; n < NR; ++n)
        if (n < cnt) back(n, vc[n]);
    for (int n = NR; n < cnt; ++n) back(n, *(const float4 *)(hr + n * H));
    if (ok) {
        for (int n = cnt; n < N; ++n) *(float4 *)(dr + n * H) = z4;
        *(float4 *)(du + r * ldu + q * 4) = acc;
        if (q == 0) dc[r * ldc] = dcs;
    }
}

}  // namespace
