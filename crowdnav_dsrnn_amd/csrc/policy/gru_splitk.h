// gru_splitk.h -- the split-K forms of the fused GRU step for launches with few rows (32-row tiles), and the choice
// between the two forms: device_cus, use_split_k, row_tile. Needs gru_cell.h and gru_fused.h (GfArgs, GbArgs, GF_*).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// Split-K variants for launches with few rows (the DSRNN node GRU: 2,048 x 128 per PPO minibatch, the
// rollout's 4,096-row node step): with 128-row tiles such a launch has fewer workgroups than CUs and each
// wave runs the whole K chain (node GRU: 16 row tiles x 4 unit tiles = 64 workgroups, 5 us of MFMA per
// wave). Here a workgroup owns 32 rows x 32 hidden units and its 4 waves split K (wave w takes K chunks
// w, w + 4, ...), loading their MFMA operands straight from global memory into registers in the
// instruction's layout (lane (i, p) holds row / unit i at k = 8q + 4p .. + 3 of chunk q: no LDS staging);
// the 4 partial tiles are summed through LDS in wave order (deterministic), then the same epilogue
// arithmetic as the 128-row kernels runs with one output row x 4 units per thread.
// ------------------------------------------------------------------------------------------------
constexpr int SK_BM = 32;

template <bool XM>
__global__ __launch_bounds__(256) void cn_gru_fused_sk_kernel(const GfArgs P)
{
    __shared__ float sP[4][XM ? 4 : 3][SK_BM][33];
    const int bid = blockIdx.x;
    const int xcd = bid & 7, k = bid >> 3;
    const int unit_tiles = P.unit_tiles, H = P.H;
    const int ut = k % unit_tiles;
    int rt = (k / unit_tiles) * 8 + xcd;
    if (rt >= P.rt_total) return;  // grid padding (whole workgroup, before any barrier)
    const bool second = rt >= P.rt0;
    const GfSeg S = second ? P.s1 : P.s0;
    if (second) rt -= P.rt0;
    const int64_t B = S.B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, p4 = (lane >> 5) * 4;
    const int64_t row0 = (int64_t)rt * SK_BM;
    const int u0 = ut * GF_BU;
    // epilogue map: thread -> row er, units u0 + lc .. + 3; its operands are requested first
    const int er = tid >> 3, lc = (tid & 7) * 4;
    const int64_t eb = min(row0 + er, B - 1);
    float4 eg[3];
    if (!XM) {
#pragma unroll
        for (int g = 0; g < 3; ++g) eg[g] = *(const float4 *)(S.gi + eb * 3 * H + g * H + u0 + lc);
    }
    const float4 hp = *(const float4 *)(S.hm + eb * H + u0 + lc);

    // XM: chunks 0 .. F/32 - 1 are x against W_ih (n into acc[3]), then hm against W_hh
    gf_f32x16 acc[XM ? 4 : 3];
#pragma unroll
    for (int g = 0; g < (XM ? 4 : 3); ++g)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[g][e] = 0.0f;
    const float *pa = S.hm + min(row0 + li, B - 1) * H + p4;
    const float *pb = S.w_hh + (int64_t)(u0 + li) * H + p4;
    const int64_t b_step = (int64_t)H * H;
    const int nch = H / GF_KC;
    const int64_t F = XM ? S.F : 0;
    const int ncx = (int)(F / GF_KC);
    const float *xa = XM ? S.x + min(row0 + li, B - 1) * F + p4 : nullptr;
    const float *xb = XM ? S.w_ih + (int64_t)(u0 + li) * F + p4 : nullptr;
    for (int c = wave; c < ncx + nch; c += 4) {
        const bool isx = c < ncx;
        const float *ap = isx ? xa + c * GF_KC : pa + (c - ncx) * GF_KC;
        const float *bp = isx ? xb + c * GF_KC : pb + (c - ncx) * GF_KC;
        const int64_t bs = isx ? (int64_t)H * F : b_step;
        float4 a[4], b[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = *(const float4 *)(ap + 8 * q);
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) b[g][q] = *(const float4 *)(bp + g * bs + 8 * q);
        if (XM && isx) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[0][q].x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[1][q].x, acc[1], 0, 0, 0);
                acc[XM ? 3 : 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[2][q].x, acc[XM ? 3 : 2], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[0][q].y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[1][q].y, acc[1], 0, 0, 0);
                acc[XM ? 3 : 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[2][q].y, acc[XM ? 3 : 2], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[0][q].z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[1][q].z, acc[1], 0, 0, 0);
                acc[XM ? 3 : 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[2][q].z, acc[XM ? 3 : 2], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[0][q].w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[1][q].w, acc[1], 0, 0, 0);
                acc[XM ? 3 : 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[2][q].w, acc[XM ? 3 : 2], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[g][q].x, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[g][q].y, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[g][q].z, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[g][q].w, acc[g], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < (XM ? 4 : 3); ++g)
#pragma unroll
        for (int e = 0; e < 16; ++e) sP[wave][g][(e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)][li] = acc[g][e];
    __syncthreads();
    const int64_t b = row0 + er;
    if (b >= B) return;
    float cs[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            cs[g][j] = ((sP[0][g][er][lc + j] + sP[1][g][er][lc + j]) + sP[2][g][er][lc + j]) + sP[3][g][er][lc + j];
    const float4 cr = make_float4(cs[0][0], cs[0][1], cs[0][2], cs[0][3]);
    const float4 cz = make_float4(cs[1][0], cs[1][1], cs[1][2], cs[1][3]);
    const float4 cn = make_float4(cs[2][0], cs[2][1], cs[2][2], cs[2][3]);
    const float *b_hh = S.b_hh;
    const float4 br = *(const float4 *)(b_hh + u0 + lc), bz = *(const float4 *)(b_hh + H + u0 + lc),
                 bn = *(const float4 *)(b_hh + 2 * H + u0 + lc);
    if (XM) {
        const float *b_ih = S.b_ih;
        float ci[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ci[j] = ((sP[0][XM ? 3 : 0][er][lc + j] + sP[1][XM ? 3 : 0][er][lc + j]) +
                                             sP[2][XM ? 3 : 0][er][lc + j]) + sP[3][XM ? 3 : 0][er][lc + j];
        const float4 bin = *(const float4 *)(b_ih + 2 * H + u0 + lc);
        eg[0] = *(const float4 *)(b_ih + u0 + lc);
        eg[1] = *(const float4 *)(b_ih + H + u0 + lc);
        eg[2] = make_float4(ci[0] + bin.x, ci[1] + bin.y, ci[2] + bin.z, ci[3] + bin.w);
    }
    const float4 ir = eg[0], iz = eg[1], in = eg[2];
    float4 hr, hz, hn, r, z, n, h;
    CN_GATE_B(x) CN_GATE_B(y) CN_GATE_B(z) CN_GATE_B(w)
    const int64_t o = b * H + u0 + lc;
    *(float4 *)(S.h_out + o) = h;
    if (S.h_out2) {
        float *d = S.h_out2 + (b / S.g2) * S.ld2 + (b % S.g2) * H + u0 + lc;
        d[0] = h.x;
        d[1] = h.y;
        d[2] = h.z;
        d[3] = h.w;
    }
    if (S.hm_next) {
        const float m = S.m_next ? S.m_next[b] : 1.0f;
        *(float4 *)(S.hm_next + o) = make_float4(h.x * m, h.y * m, h.z * m, h.w * m);
    }
    if (S.save) {
        float *sv = S.save + b * 4 * H + u0 + lc;
        *(float4 *)(sv) = r;
        *(float4 *)(sv + H) = z;
        *(float4 *)(sv + 2 * H) = n;
        *(float4 *)(sv + 3 * H) = hn;
    }
}

__global__ __launch_bounds__(256) void cn_gru_bwd_sk_kernel(const GbArgs P)
{
    __shared__ float sP[4][SK_BM][33];
    __shared__ float red[256 * 16];
    const int bid = blockIdx.x;
    const int xcd = bid & 7, k = bid >> 3;
    const int unit_tiles = P.unit_tiles, H = P.H;
    const int ut = k % unit_tiles;
    int rt = (k / unit_tiles) * 8 + xcd;
    if (rt >= P.rt_total) return;  // grid padding (whole workgroup, before any barrier)
    const bool second = rt >= P.rt0;
    const GbSeg S = second ? P.s1 : P.s0;
    if (second) rt -= P.rt0;
    const int64_t B = S.B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, p4 = (lane >> 5) * 4;
    const int64_t row0 = (int64_t)rt * SK_BM;
    const int u0 = ut * GF_BU;
    const int er = tid >> 3, lc = (tid & 7) * 4;
    const int64_t eb = min(row0 + er, B - 1);
    const bool gates = S.g != nullptr;
    const int64_t eo = eb * H + u0 + lc;
    // epilogue operands first (they do not depend on the GEMM)
    const float4 ai = *(const float4 *)(S.a + eo);
    float4 es[4], d = make_float4(0.f, 0.f, 0.f, 0.f), hp = d;
    float m = 1.0f;
    if (gates) {
        const float *sv = S.save + eb * 4 * H + u0 + lc;
#pragma unroll
        for (int q = 0; q < 4; ++q) es[q] = *(const float4 *)(sv + q * H);
        hp = *(const float4 *)(S.hm + eo);
        if (S.dout) d = *(const float4 *)(S.dout + eo);
        if (S.m_next) m = S.m_next[eb];
    }
    gf_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    if (S.gk) {
        const int K3 = 3 * H;
        const float *pa = S.gk + min(row0 + li, B - 1) * 4 * H + H + p4;
        const float *pb = S.wt + (int64_t)(u0 + li) * K3 + p4;
        const int nch = K3 / GF_KC;
        for (int c = wave; c < nch; c += 4) {
            const int kc = c * GF_KC;
            float4 a[4], bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = *(const float4 *)(pa + kc + 8 * q);
                bv[q] = *(const float4 *)(pb + kc + 8 * q);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, bv[q].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, bv[q].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, bv[q].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, bv[q].w, acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) sP[wave][(e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)][li] = acc[e];
    __syncthreads();
    const int64_t b = row0 + er;
    const bool live = b < B;
    float4 sr = make_float4(0.f, 0.f, 0.f, 0.f), sz = sr, sn = sr, shn = sr;
    if (live) {
        float cs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] = ((sP[0][er][lc + j] + sP[1][er][lc + j]) + sP[2][er][lc + j]) + sP[3][er][lc + j];
        const float4 v = make_float4(cs[0] + ai.x, cs[1] + ai.y, cs[2] + ai.z, cs[3] + ai.w);
        const int64_t o = b * H + u0 + lc;
        if (!gates) {
            *(float4 *)(S.a + o) = v;
        } else {
            const float4 r = es[0], z = es[1], n = es[2], hn = es[3];
            float4 a, dr, dz, dn, dhn;
#define GB(c) CN_GBWD(c, v.c * m + d.c) CN_GSUM(c, =)
            GB(x) GB(y) GB(z) GB(w)
#undef GB
            *(float4 *)(S.a + o) = a;
            float *gr = S.g + b * 4 * H + u0 + lc;
            *(float4 *)(gr) = dn;
            *(float4 *)(gr + H) = dr;
            *(float4 *)(gr + 2 * H) = dz;
            *(float4 *)(gr + 3 * H) = dhn;
        }
    }
    if (!gates) return;
    // column sums of the tile (32 units x 4 gates) over its 32 rows, in row order through LDS
    float *rw = red + tid * 16;
    *(float4 *)(rw) = sr;
    *(float4 *)(rw + 4) = sz;
    *(float4 *)(rw + 8) = sn;
    *(float4 *)(rw + 12) = shn;
    __syncthreads();
    if (tid >= 4 * GF_BU) return;
    const int q = tid / GF_BU, cu = tid - q * GF_BU;
    const float *src = red + (cu >> 2) * 16 + q * 4 + (cu & 3);
    float s = 0.0f;
    for (int r = 0; r < SK_BM; ++r) s += src[r * 8 * 16];
    S.part[(int64_t)rt * 4 * H + q * H + u0 + cu] = s;
}

// CUs of the current device (256 on the MI355X), read once per device: the split-K choice below, and with
// it the workspace sizing of cn_gru_bwd_seq_work_elems, follows the part it runs on
static int device_cus()
{
    static int cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// 128-row tiles unless that leaves fewer workgroups than CUs (then the split-K kernels, 32-row tiles)
static inline bool use_split_k(int64_t rows, int H)
{
    return (rows + GF_BM - 1) / GF_BM * (H / GF_BU) < device_cus();
}
static inline int64_t row_tile(int64_t rows_total, int H) { return use_split_k(rows_total, H) ? SK_BM : GF_BM; }

}  // namespace
