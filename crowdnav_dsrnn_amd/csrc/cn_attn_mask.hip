// Spatial-edge attention over the humans the robot currently sees (cn_spatial_attn_mask_fwd / _bwd).
//
// cn_gru.hip's cn_spatial_attn_var_fwd / _bwd let a row attend to a prefix of its N slots; here the subset is any:
// mask [R][N] float, nonzero and not NaN = visible (cn_visible_mask's output, possibly ANDed with a count by the
// caller). Row r visits its visible slots in ascending slot order and performs on them exactly the operations the
// _var pair performs on a row that holds those slots compacted to the front -- score, max, denominator, pooling, s,
// ds, du, dc, in that order -- so a full mask gives cn_spatial_attn_fwd's row, a prefix mask the _var row of that
// count, and any mask the _var row of the compacted input, bit for bit (-ffp-contract=off in every unit).
// attn[r][n] and dhs[r][n][:] of masked slots are written as exact zeros; hs[r][n] and dattn[r][n] are never read
// there. A row without a visible slot gives out = 0, attn = 0, du = 0, dc = 0, dhs = 0.
//
// A translation unit of its own, not a section of cn_gru.hip under policy/: the code object of cn_gru.hip does not
// move (its kernels' placement has measured 0.4 - 0.8 % on the training workload with byte-identical kernels).
//
// Mapping as the _var pair: one thread per (row, 4 consecutive h), HQ = H / 4 lanes per row, rows never straddle a
// wave, scores through LDS at the COMPACT index k (the k-th visible slot), the first NR VISIBLE vectors stay in
// registers between the two passes. The row's visibility is a 64-bit word `vm` (bit n = slot n), built by wave
// ballots over a launch-uniform loop (ceil(N / HQ) rounds, every lane of the wave executes every ballot; a lane takes
// the HQ bits of its own row); the walk takes the lowest set bit and clears it.
// Cross-lane reads: the ballots run before any divergent code with all 64 lanes active; the __shfl_xor reductions
// use offsets < HQ, so a lane reads only lanes of its own row, and all HQ lanes of a row hold the same vm, hence run
// the same trip count and visit the same slots: every lane a reduction reads is active at that instruction, whatever
// the other rows of the wave do. The workgroup barrier is outside every loop and reached by all 256 threads. Rows
// past R get vm = 0: no loads, no stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

#include "../../include/crowdnav.h"
#include "cn_host.h"   // cn_set_error, grid_for, launch_status, CN_SA_LAUNCH (the (H, N) ladder of cn_gru.hip's kernels)

namespace {

#define CN_SAM_MAXN 64

// visibility word of row r (all HQ lanes of the row return the same word); called by all 256 threads
template <int HQ>
__device__ __forceinline__ uint64_t row_mask(const float *__restrict__ mask, int64_t r, int N, int q, bool ok)
{
    const int rowbase = ((int)threadIdx.x & 63) & ~(HQ - 1);
    uint64_t vm = 0;
    for (int b = 0; b < N; b += HQ) {
        const int n = b + q;
        bool p = false;
        if (ok && n < N) {
            const float m = mask[r * N + n];
            p = m != 0.0f && m == m;
        }
        const uint64_t bal = __ballot(p);
        const uint64_t bits = HQ == 64 ? bal : ((bal >> rowbase) & ((1ull << (HQ & 63)) - 1ull));
        vm |= bits << b;
    }
    return vm;
}

__device__ __forceinline__ int pop_low(uint64_t &w)
{
    const int n = __builtin_ctzll(w);
    w &= w - 1;
    return n;
}

template <int HQ, int NR>
__global__ __launch_bounds__(256) void cn_spatial_attn_mask_fwd_kernel(int64_t R, int N,
                                                                       const float *__restrict__ mask,
                                                                       const float *__restrict__ row_scale,
                                                                       const float *__restrict__ hs,
                                                                       const float *__restrict__ u,
                                                                       const float *__restrict__ c,
                                                                       float *__restrict__ out,
                                                                       float *__restrict__ attn)
{
    constexpr int H = HQ * 4, RB = 256 / HQ;
    __shared__ float sc[RB][CN_SAM_MAXN];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / HQ;
    const int q = (int)(i - r * HQ), rl = (int)threadIdx.x / HQ;
    const bool ok = r < R;
    const uint64_t vm = row_mask<HQ>(mask, r, N, q, ok);
    const int cnt = __popcll(vm);
    const float scale = ok ? row_scale[r] : 0.f;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 uu = z4;
    if (ok) uu = *(const float4 *)(u + r * H + q * 4);
    const float cr = ok ? c[r] : 0.f;
    const float *hr = hs + (ok ? r : 0) * (int64_t)N * H + q * 4;
    float4 vc[NR];
    float mx = -INFINITY;
    auto score = [&](int k, const float4 &v) {
        float part = ((uu.x * v.x + uu.y * v.y) + uu.z * v.z) + uu.w * v.w;
#pragma unroll
        for (int o = HQ / 2; o; o >>= 1) part += __shfl_xor(part, o);
        const float s = (part + cr) * scale;
        if (q == 0) sc[rl][k] = s;
        mx = fmaxf(mx, s);
    };
    uint64_t w = vm;
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if (k < cnt) {
            vc[k] = *(const float4 *)(hr + pop_low(w) * H);
            score(k, vc[k]);
        }
    for (int k = NR; k < cnt; ++k) score(k, *(const float4 *)(hr + pop_low(w) * H));
    __syncthreads();
    float den = 0.f;
    for (int k = 0; k < cnt; ++k) den += expf(sc[rl][k] - mx);
    float4 acc = z4;
    auto pool = [&](int k, int n, const float4 &v) {
        const float a = expf(sc[rl][k] - mx) / den;
        acc.x += v.x * a; acc.y += v.y * a; acc.z += v.z * a; acc.w += v.w * a;
        if (q == 0) attn[r * N + n] = a;
    };
    w = vm;
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if (k < cnt) pool(k, pop_low(w), vc[k]);
    for (int k = NR; k < cnt; ++k) {
        const int n = pop_low(w);
        pool(k, n, *(const float4 *)(hr + n * H));
    }
    if (ok) {
        for (int n = q; n < N; n += HQ)
            if (!((vm >> n) & 1ull)) attn[r * N + n] = 0.f;
        *(float4 *)(out + r * H + q * 4) = acc;
    }
}

template <int HQ, int NR>
__global__ __launch_bounds__(256) void cn_spatial_attn_mask_bwd_kernel(int64_t R, int N,
                                                                       const float *__restrict__ mask,
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
    __shared__ float sp[RB][CN_SAM_MAXN];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / HQ;
    const int q = (int)(i - r * HQ), rl = (int)threadIdx.x / HQ;
    const bool ok = r < R;
    const int64_t rr = ok ? r : 0;
    const uint64_t vm = row_mask<HQ>(mask, r, N, q, ok);
    const int cnt = __popcll(vm);
    const float scale = ok ? row_scale[r] : 0.f;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g = z4;
    if (ok) g = *(const float4 *)(dout + r * H + q * 4);
    float4 uu = z4;
    if (ok) uu = *(const float4 *)(u + r * H + q * 4);
    const float *hr = hs + rr * (int64_t)N * H + q * 4;
    float4 vc[NR];
    float s = 0.f;
    auto grad = [&](int k, int n, const float4 &v) {
        float part = ((g.x * v.x + g.y * v.y) + g.z * v.z) + g.w * v.w;
#pragma unroll
        for (int o = HQ / 2; o; o >>= 1) part += __shfl_xor(part, o);
        if (dattn) part += dattn[rr * N + n];
        if (q == 0) sp[rl][k] = part;
        s += attn[rr * N + n] * part;
    };
    uint64_t w = vm;
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if (k < cnt) {
            const int n = pop_low(w);
            vc[k] = *(const float4 *)(hr + n * H);
            grad(k, n, vc[k]);
        }
    for (int k = NR; k < cnt; ++k) {
        const int n = pop_low(w);
        grad(k, n, *(const float4 *)(hr + n * H));
    }
    __syncthreads();
    float4 acc = z4;
    float dcs = 0.f;
    float *dr = dhs + rr * (int64_t)N * H + q * 4;
    auto back = [&](int k, int n, const float4 &v) {
        const float a = attn[rr * N + n];
        const float ds = scale * (a * (sp[rl][k] - s));
        acc.x += ds * v.x; acc.y += ds * v.y; acc.z += ds * v.z; acc.w += ds * v.w;
        dcs += ds;
        *(float4 *)(dr + n * H) = make_float4(a * g.x + ds * uu.x, a * g.y + ds * uu.y, a * g.z + ds * uu.z,
                                              a * g.w + ds * uu.w);
    };
    w = vm;
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if (k < cnt) back(k, pop_low(w), vc[k]);
    for (int k = NR; k < cnt; ++k) {
        const int n = pop_low(w);
        back(k, n, *(const float4 *)(hr + n * H));
    }
    if (ok) {
        for (int n = 0; n < N; ++n)
            if (!((vm >> n) & 1ull)) *(float4 *)(dr + n * H) = z4;
        *(float4 *)(du + r * ldu + q * 4) = acc;
        if (q == 0) dc[r * ldc] = dcs;
    }
}

int sam_check(const char *who, int64_t R, int N, int H, std::initializer_list<const void *> vec,
              std::initializer_list<const void *> other)
{
    if (R <= 0 || N <= 0 || N > CN_SAM_MAXN || !(H == 256 || H == 128 || H == 64) ||
        R * (H / 4) > (int64_t)0x7fffffff * 256)
        return cn_set_error(CN_EINVAL, who);
    for (const void *p : vec)
        if (!p || ((uintptr_t)p & 15)) return cn_set_error(CN_EINVAL, who);
    for (const void *p : other)
        if (!p) return cn_set_error(CN_EINVAL, who);
    return CN_OK;
}

}  // namespace

extern "C" {

int cn_spatial_attn_mask_fwd(void *stream, int64_t R, int N, int H, const float *mask, const float *row_scale,
                             const float *hs, const float *u, const float *c, float *out, float *attn)
{
    if (sam_check("cn_spatial_attn_mask_fwd: H in {64, 128, 256}, 1 <= N <= 64, non-null operands, hs / u / out "
                  "16-byte aligned", R, N, H, {hs, u, out}, {mask, row_scale, c, attn}))
        return CN_EINVAL;
    const unsigned grid = grid_for(R, H);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    CN_SA_LAUNCH(cn_spatial_attn_mask_fwd_kernel, H, N, grid, (hipStream_t)stream, R, N, mask, row_scale,
                 hs, u, c, out, attn);
    return launch_status();
}

int cn_spatial_attn_mask_bwd(void *stream, int64_t R, int N, int H, const float *mask, const float *row_scale,
                             const float *hs, const float *u, const float *attn, const float *dout, const float *dattn,
                             float *dhs, float *du, int64_t ldu, float *dc, int64_t ldc)
{
    if (sam_check("cn_spatial_attn_mask_bwd: H in {64, 128, 256}, 1 <= N <= 64, non-null operands, hs / u / dout / "
                  "dhs / du 16-byte aligned, ldu >= H and a multiple of 4, ldc >= 1", R, N, H, {hs, u, dout, dhs, du},
                  {mask, row_scale, attn, dc}) || ldu < H || (ldu & 3) || ldc < 1)
        return cn_set_error(CN_EINVAL, "cn_spatial_attn_mask_bwd: bad shape, stride or operand");
    const unsigned grid = grid_for(R, H);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    CN_SA_LAUNCH(cn_spatial_attn_mask_bwd_kernel, H, N, grid, (hipStream_t)stream, R, N, mask, row_scale,
                 hs, u, attn, dout, dattn, dhs, du, ldu, dc, ldc);
    return launch_status();
}

}  // extern "C"
