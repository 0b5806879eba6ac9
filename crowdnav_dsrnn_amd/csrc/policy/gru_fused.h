// gru_fused.h -- the fused GRU step on the matrix cores, 128-row tiles: GfSeg / GfArgs and cn_gru_fused_kernel, GbSeg /
// GbArgs and cn_gru_bwd_fused_kernel. Needs gru_cell.h (sigm, CN_GATE, CN_GBWD).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// Fused recurrent step: gh = hm W_hh^T + b_hh on the f32-input matrix cores with the gate arithmetic of
// cn_gru_fwd_kernel in the epilogue, so gh ([B][3H], 63 MB at C4's 20,480 x 256) never goes to HBM.
// Workgroup tile: GF_BM = 128 rows x GF_BU = 32 hidden units, i.e. the r, z and n columns of those units
// (96 of W_hh's rows); 4 waves, wave w owns rows 32w .. 32w + 31 and one 32x32 accumulator per gate
// (v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulation). K (= H) streams through LDS in chunks
// of 32: the next chunk's global loads are in flight while the current one is multiplied.
// The k pair of an MFMA is a permutation of K (lane half p of step (c, q) holds k = 8c + 4p + q for A
// and B alike), so every lane reads 16-byte LDS vectors. Rows are padded to 36 floats in LDS (the 32 rows
// of a b128 read land on distinct bank groups).
// Grid: XCD-aware -- workgroup id x runs on XCD x % 8; the 8 unit tiles (H = 256) of one row tile are
// given consecutive ids on the same XCD, so the row tile's hm rows are fetched into that XCD's L2 once.
// ------------------------------------------------------------------------------------------------
constexpr int GF_BM = 128, GF_BU = 32, GF_KC = 32, GF_LD = GF_KC + 4;
typedef float gf_f32x16 __attribute__((ext_vector_type(16)));

// One GRU (segment) of a fused-step launch: two independent GRUs with the same H (the DSRNN's spatial and
// temporal edge RNNs) share one launch, the row tiles of the second following the first's.
struct GfSeg {
    int64_t B;
    const float *gi, *hm, *w_hh, *b_hh, *m_next;
    float *h_out, *hm_next, *save, *h_out2;
    int64_t g2, ld2;
    // input projection in the kernel (template XM): gi = x W_ih^T + b_ih from x [B][F], w_ih [3H][F], b_ih [3H]
    const float *x, *w_ih, *b_ih;
    int64_t F;
};
struct GfArgs {
    GfSeg s0, s1;
    int rt0, rt_total, unit_tiles, H;
};
// XM (input projection in the kernel): the K loop first runs the F / 32 chunks of x against W_ih (r and z into
// the same accumulators as their recurrent parts, n into a fourth one: gi_n stays separate from gh_n), then
// the H / 32 chunks of hm against W_hh; the epilogue adds b_ih and b_hh. gi ([B][3H], 3 of the 10 floats the
// step moves per output, and its T * B * 3H buffer) is never materialised.
template <bool XM>
__global__ __launch_bounds__(256, 3) void cn_gru_fused_kernel(const GfArgs P)
{
    // LDS: one A / B chunk buffer during the K loop, then the three gate accumulators of the tile
    // (sC[g][row][unit], rows padded to LDC = 33) for the epilogue's row-major pass. 50.7 KB in all, so three
    // workgroups fit per CU: another workgroup's MFMAs cover one's barriers and epilogue (measured 92 us vs
    // 99 us for the double-buffered 64.5 KB form at two per CU).
    constexpr int SA = GF_BM * GF_LD, SB = 3 * GF_BU * GF_LD, LDC = 33;
    constexpr int SMEM = (SA + SB) > 3 * GF_BM * LDC ? (SA + SB) : 3 * GF_BM * LDC;
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    float *const sA0 = smem, *const sB0 = smem + SA;
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
    const float *__restrict__ gi = S.gi, *__restrict__ hm = S.hm, *__restrict__ w_hh = S.w_hh,
                                  *__restrict__ b_hh = S.b_hh, *__restrict__ m_next = S.m_next;
    float *__restrict__ h_out = S.h_out, *__restrict__ hm_next = S.hm_next, *__restrict__ save = S.save,
                        *__restrict__ h_out2 = S.h_out2;
    const int64_t g2 = S.g2, ld2 = S.ld2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)rt * GF_BM;
    const int u0 = ut * GF_BU;

    // global -> register staging: A = 128 rows x 32 floats (4 float4 per thread), B = 96 rows (3 per thread).
    // Plain scalars (no captured arrays): the loads must stay in flight across the chunk's MFMAs. The same
    // thread -> (row, 4 columns) map serves the epilogue: thread t owns units u0 + lc .. + 3 of rows lr + 32 i.
    const int lc = (tid & 7) * 4, lr = tid >> 3;
    // rows past B (last row tile) read row B - 1 instead: rows are independent and those are never stored
    int64_t ar[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ar[i] = min(row0 + lr + 32 * i, B - 1);
    const float *pa0 = hm + ar[0] * H + lc, *pa1 = hm + ar[1] * H + lc, *pa2 = hm + ar[2] * H + lc,
                *pa3 = hm + ar[3] * H + lc;
    const float *pb0 = w_hh + (int64_t)(u0 + lr) * H + lc;
    const int64_t b_step = (int64_t)H * H;
    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2;
#define GF_GLOAD(kc)                                                         \
    ra0 = *(const float4 *)(pa0 + (kc));                                     \
    ra1 = *(const float4 *)(pa1 + (kc));                                     \
    ra2 = *(const float4 *)(pa2 + (kc));                                     \
    ra3 = *(const float4 *)(pa3 + (kc));                                     \
    rb0 = *(const float4 *)(pb0 + (kc));                                     \
    rb1 = *(const float4 *)(pb0 + b_step + (kc));                            \
    rb2 = *(const float4 *)(pb0 + 2 * b_step + (kc));
#define GF_LSTORE(buf)                                                                    \
    {                                                                                     \
        float *da = sA0 + (buf) * SA + lr * GF_LD + lc, *db = sB0 + (buf) * SB + lr * GF_LD + lc; \
        *(float4 *)(da) = ra0;                                                            \
        *(float4 *)(da + 32 * GF_LD) = ra1;                                               \
        *(float4 *)(da + 64 * GF_LD) = ra2;                                               \
        *(float4 *)(da + 96 * GF_LD) = ra3;                                               \
        *(float4 *)(db) = rb0;                                                            \
        *(float4 *)(db + GF_BU * GF_LD) = rb1;                                            \
        *(float4 *)(db + 2 * GF_BU * GF_LD) = rb2;                                        \
    }
    const int li = lane & 31, p4 = (lane >> 5) * 4;
#define GF_MMA(buf, A2)                                                                                      \
    {                                                                                                        \
        const float *a_base = sA0 + (buf) * SA + (wave * 32 + li) * GF_LD + p4;                              \
        const float *b_base = sB0 + (buf) * SB + li * GF_LD + p4;                                            \
        _Pragma("unroll") for (int c = 0; c < GF_KC / 8; ++c)                                                \
        {                                                                                                    \
            const float4 a = *(const float4 *)(a_base + 8 * c);                                              \
            float4 bv[3];                                                                                    \
            _Pragma("unroll") for (int g = 0; g < 3; ++g) bv[g] = *(const float4 *)(b_base + g * GF_BU * GF_LD + 8 * c); \
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv[0].x, acc[0], 0, 0, 0);                   \
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv[1].x, acc[1], 0, 0, 0);                   \
            A2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv[2].x, A2, 0, 0, 0);                           \
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv[0].y, acc[0], 0, 0, 0);                   \
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv[1].y, acc[1], 0, 0, 0);                   \
            A2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv[2].y, A2, 0, 0, 0);                           \
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv[0].z, acc[0], 0, 0, 0);                   \
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv[1].z, acc[1], 0, 0, 0);                   \
            A2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv[2].z, A2, 0, 0, 0);                           \
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv[0].w, acc[0], 0, 0, 0);                   \
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv[1].w, acc[1], 0, 0, 0);                   \
            A2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv[2].w, A2, 0, 0, 0);                           \
        }                                                                                                    \
    }

    gf_f32x16 acc[3], acc_in;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[g][e] = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc_in[e] = 0.0f;

    const int nch = H / GF_KC;
    float4 eg[4][3], eh[4];
#define GF_EPI_LOAD()                                                                    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                       \
    {                                                                                    \
        if (!XM) {                                                                       \
            const float *gib = gi + ar[i] * 3 * H + u0 + lc;                             \
            _Pragma("unroll") for (int g = 0; g < 3; ++g) eg[i][g] = *(const float4 *)(gib + g * H); \
        }                                                                                \
        eh[i] = *(const float4 *)(hm + ar[i] * H + u0 + lc);                             \
    }
    if (XM) {
        // x chunks first (A = x rows, B = W_ih rows; n into acc_in), then the recurrent ones. Two loops, and
        // the x addresses formed per load, so no second address set stays live across the recurrent chunks.
        const int64_t F = S.F;
        const int ncx = (int)(F / GF_KC);
        const float *__restrict__ xx = S.x, *__restrict__ wih = S.w_ih;
#define GF_GLOAD_X(kc)                                                                        \
    {                                                                                         \
        ra0 = *(const float4 *)(xx + ar[0] * F + lc + (kc));                                  \
        ra1 = *(const float4 *)(xx + ar[1] * F + lc + (kc));                                  \
        ra2 = *(const float4 *)(xx + ar[2] * F + lc + (kc));                                  \
        ra3 = *(const float4 *)(xx + ar[3] * F + lc + (kc));                                  \
        const float *xb = wih + (int64_t)(u0 + lr) * F + lc + (kc);                           \
        rb0 = *(const float4 *)(xb);                                                          \
        rb1 = *(const float4 *)(xb + (int64_t)H * F);                                         \
        rb2 = *(const float4 *)(xb + (int64_t)2 * H * F);                                     \
    }
        GF_GLOAD_X(0)
        GF_LSTORE(0)
        __syncthreads();
        for (int ch = 0; ch < ncx; ++ch) {
            if (ch + 1 < ncx) {
                GF_GLOAD_X((ch + 1) * GF_KC)
            } else {
                GF_GLOAD(0)   // the first recurrent chunk
            }
            GF_MMA(0, acc_in)
            __syncthreads();
            GF_LSTORE(0)
            __syncthreads();
        }
#undef GF_GLOAD_X
    } else {
        GF_GLOAD(0)
        GF_LSTORE(0)
        __syncthreads();
    }
    for (int ch = 0; ch + 1 < nch; ++ch) {
        GF_GLOAD((ch + 1) * GF_KC)  // in flight during this chunk's MFMAs
        GF_MMA(0, acc[2])
        __syncthreads();
        GF_LSTORE(0)
        __syncthreads();
    }
    // last chunk (a recurrent one): the epilogue's operands (gi's three gate blocks unless XM, and hm of this
    // thread's 4 x 4 outputs) are fetched while its MFMAs run
    GF_EPI_LOAD()
#undef GF_EPI_LOAD
    GF_MMA(0, acc[2])
    __syncthreads();  // every wave is done reading the chunk buffers before sC overwrites them
#undef GF_GLOAD
#undef GF_LSTORE
#undef GF_MMA

    // accumulators -> LDS: lane holds unit li of rows (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of its wave's 32.
    // XM: the input part of n (acc_in) goes through region 2 first; gi_r / gi_z are b_ih alone (their x parts
    // are in acc r / z) and gi_n = acc_in + b_ih_n
#define GF_TO_LDS(g, A)                                                                                        \
    _Pragma("unroll") for (int e = 0; e < 16; ++e)                                                           \
        smem[((g) * GF_BM + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) * LDC + li] = (A)[e];
    GF_TO_LDS(0, acc[0])
    GF_TO_LDS(1, acc[1])
    if (XM) {
        GF_TO_LDS(2, acc_in)
        __syncthreads();
        const float *b_ih = S.b_ih;
        const float4 bir = *(const float4 *)(b_ih + u0 + lc), biz = *(const float4 *)(b_ih + H + u0 + lc),
                     bin = *(const float4 *)(b_ih + 2 * H + u0 + lc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float *pc = smem + (2 * GF_BM + lr + 32 * i) * LDC + lc;
            eg[i][0] = bir;
            eg[i][1] = biz;
            eg[i][2] = make_float4(pc[0] + bin.x, pc[1] + bin.y, pc[2] + bin.z, pc[3] + bin.w);
        }
        __syncthreads();
    }
    GF_TO_LDS(2, acc[2])
#undef GF_TO_LDS
    __syncthreads();

    const float4 br = *(const float4 *)(b_hh + u0 + lc), bz = *(const float4 *)(b_hh + H + u0 + lc),
                 bn = *(const float4 *)(b_hh + 2 * H + u0 + lc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = lr + 32 * i;
        const int64_t b = row0 + row;
        if (b >= B) continue;
        const float *pcr = smem + (0 * GF_BM + row) * LDC + lc;
        const float4 cr = make_float4(pcr[0], pcr[1], pcr[2], pcr[3]);
        const float *pcz = smem + (1 * GF_BM + row) * LDC + lc;
        const float4 cz = make_float4(pcz[0], pcz[1], pcz[2], pcz[3]);
        const float *pcn = smem + (2 * GF_BM + row) * LDC + lc;
        const float4 cn = make_float4(pcn[0], pcn[1], pcn[2], pcn[3]);
        const float4 ir = eg[i][0], iz = eg[i][1], in = eg[i][2], hp = eh[i];
        float4 hr, hz, hn, r, z, n, h;
        CN_GATE_B(x) CN_GATE_B(y) CN_GATE_B(z) CN_GATE_B(w)
        const int64_t o = b * H + u0 + lc;
        *(float4 *)(h_out + o) = h;
        if (h_out2) {
            float *d = h_out2 + (b / g2) * ld2 + (b % g2) * H + u0 + lc;
            d[0] = h.x;
            d[1] = h.y;
            d[2] = h.z;
            d[3] = h.w;
        }
        if (hm_next) {
            const float m = m_next ? m_next[b] : 1.0f;
            *(float4 *)(hm_next + o) = make_float4(h.x * m, h.y * m, h.z * m, h.w * m);
        }
        if (save) {
            float *sv = save + b * 4 * H + u0 + lc;
            *(float4 *)(sv) = r;
            *(float4 *)(sv + H) = z;
            *(float4 *)(sv + 2 * H) = n;
            *(float4 *)(sv + 3 * H) = hn;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Fused backward step: the recurrent GEMM of step t, acc_t = a_t + g_t[:, H:4H] W_hh (K = 3H; a_t = the
// direct path dL/dh_t * z_t), on the f32 matrix cores with the gate gradients of step t - 1 in its epilogue:
//   gacc = acc_t * m_t + dout_{t-1}                       (dL/dh_{t-1})
//   dn = gacc (1 - z) (1 - n^2), dz = gacc (hm - n) z (1 - z), dr = dn gh_n r (1 - r), dhn = dn r
//   a_{t-1} = gacc z;  g_{t-1} = [dn | dr | dz | dhn];  column sums of dr | dz | dn | dhn -> part
// so acc_t never goes to HBM and the backward is one launch per step (cn_gru_bwd_seq). Modes per launch: no
// GEMM (gk = null: the first step, acc = dL/dh_{T-1} comes in through a) and no gates (g = null: the last
// step, a <- acc_0 = dL/dhm_0). Same tiling as cn_gru_fused_kernel: 128 rows x 32 hidden units per
// workgroup, wave w owns rows 32w .. 32w + 31 with one 32x32 accumulator (v_mfma_f32_32x32x2_f32), K in
// chunks of 32 through double-buffered LDS (46 KB: three workgroups per CU), XCD-aware tile order.
// The B operand is W_hh^T [H][3H] (row u = unit u's weights over the 3H gate gradients, contiguous in K).
// ------------------------------------------------------------------------------------------------
struct GbSeg {
    int64_t B;
    const float *gk;      // g_t [B][4H]: the K operand is its columns H .. 4H (dr | dz | dhn); null: no GEMM
    const float *wt;      // W_hh^T [H][3H]
    float *a;             // [B][H]: in a_t (or dL/dh_{T-1}), out a_{t-1} (gates) or acc_t (no gates)
    const float *m_next;  // [B] m_t, or null (= 1)
    const float *dout;    // [B][H] dL/d out_{t-1}, or null
    const float *save;    // [B][4H] r | z | n | gh_n of step t - 1
    const float *hm;      // [B][H] masked state entering step t - 1
    float *g;             // [B][4H] out g_{t-1}, or null: no gates
    float *part;          // [row tiles][4H] out: the workgroup's column sums
};
struct GbArgs {
    GbSeg s0, s1;
    int rt0, rt_total, unit_tiles, H;
};

__global__ __launch_bounds__(256, 3) void cn_gru_bwd_fused_kernel(const GbArgs P)
{
    constexpr int SA = GF_BM * GF_LD, SB = GF_BU * GF_LD, LDC = 33;
    __shared__ __attribute__((aligned(16))) float smem[2 * (SA + SB)];
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
    const int64_t row0 = (int64_t)rt * GF_BM;
    const int u0 = ut * GF_BU;
    const int lc = (tid & 7) * 4, lr = tid >> 3;
    const int li = lane & 31, p4 = (lane >> 5) * 4;
    int64_t ar[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ar[i] = min(row0 + lr + 32 * i, B - 1);

    gf_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    // the gate records of the epilogue's 4 x 4 outputs (thread: units u0 + lc .. + 3 of rows lr + 32 i) are
    // fetched during the last chunk; the other operands (a, dout, hm: one float4 per row each) in the epilogue
    float4 es[4][4];
    const bool gates = S.g != nullptr;
#define GB_EPI_LOAD()                                                                                   \
    if (gates) {                                                                                        \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                  \
        {                                                                                               \
            const float *sv = S.save + ar[i] * 4 * H + u0 + lc;                                         \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) es[i][q] = *(const float4 *)(sv + q * H);    \
        }                                                                                               \
    }

    if (S.gk) {
        const int K3 = 3 * H, ldg = 4 * H;
        const float *pa0 = S.gk + ar[0] * ldg + H + lc, *pa1 = S.gk + ar[1] * ldg + H + lc,
                    *pa2 = S.gk + ar[2] * ldg + H + lc, *pa3 = S.gk + ar[3] * ldg + H + lc;
        const float *pb = S.wt + (int64_t)(u0 + lr) * K3 + lc;
        float4 ra0, ra1, ra2, ra3, rb;
#define GB_GLOAD(kc)                           \
    ra0 = *(const float4 *)(pa0 + (kc));       \
    ra1 = *(const float4 *)(pa1 + (kc));       \
    ra2 = *(const float4 *)(pa2 + (kc));       \
    ra3 = *(const float4 *)(pa3 + (kc));       \
    rb = *(const float4 *)(pb + (kc));
#define GB_LSTORE(buf)                                                                          \
    {                                                                                           \
        float *da = smem + (buf) * SA + lr * GF_LD + lc, *db = smem + 2 * SA + (buf) * SB + lr * GF_LD + lc; \
        *(float4 *)(da) = ra0;                                                                  \
        *(float4 *)(da + 32 * GF_LD) = ra1;                                                     \
        *(float4 *)(da + 64 * GF_LD) = ra2;                                                     \
        *(float4 *)(da + 96 * GF_LD) = ra3;                                                     \
        *(float4 *)(db) = rb;                                                                   \
    }
#define GB_MMA(buf)                                                                             \
    {                                                                                           \
        const float *a_base = smem + (buf) * SA + (wave * 32 + li) * GF_LD + p4;                \
        const float *b_base = smem + 2 * SA + (buf) * SB + li * GF_LD + p4;                     \
        _Pragma("unroll") for (int c = 0; c < GF_KC / 8; ++c)                                   \
        {                                                                                       \
            const float4 av = *(const float4 *)(a_base + 8 * c);                                \
            const float4 bv = *(const float4 *)(b_base + 8 * c);                                \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);               \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);               \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);               \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);               \
        }                                                                                       \
    }
        const int nch = K3 / GF_KC;
        GB_GLOAD(0)
        GB_LSTORE(0)
        __syncthreads();
        for (int ch = 0; ch + 1 < nch; ++ch) {
            GB_GLOAD((ch + 1) * GF_KC)  // in flight during this chunk's MFMAs
            GB_MMA(ch & 1)
            GB_LSTORE((ch + 1) & 1)     // the other buffer: its last readers passed the previous barrier
            __syncthreads();
        }
        GB_EPI_LOAD()
        GB_MMA((nch - 1) & 1)
        __syncthreads();  // every wave is done reading the chunk buffers before sC overwrites them
#undef GB_GLOAD
#undef GB_LSTORE
#undef GB_MMA
    } else {
        GB_EPI_LOAD()
    }
#undef GB_EPI_LOAD
    // accumulator -> LDS (sC [128][LDC]): lane holds unit li of rows (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    float *const sC = smem;
#pragma unroll
    for (int e = 0; e < 16; ++e) sC[(wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) * LDC + li] = acc[e];
    __syncthreads();

    float4 sr = make_float4(0.f, 0.f, 0.f, 0.f), sz = sr, sn = sr, shn = sr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = lr + 32 * i;
        const int64_t b = row0 + row;
        if (b >= B) continue;
        const int64_t o = b * H + u0 + lc;
        const float *pc = sC + row * LDC + lc;
        const float4 ai = *(const float4 *)(S.a + o);
        const float4 v = make_float4(pc[0] + ai.x, pc[1] + ai.y, pc[2] + ai.z, pc[3] + ai.w);
        if (!gates) {
            *(float4 *)(S.a + o) = v;
            continue;
        }
        const float m = S.m_next ? S.m_next[b] : 1.0f;
        const float4 d = S.dout ? *(const float4 *)(S.dout + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 hp = *(const float4 *)(S.hm + o);
        const float4 r = es[i][0], z = es[i][1], n = es[i][2], hn = es[i][3];
        float4 a, dr, dz, dn, dhn;
#define GB(c) CN_GBWD(c, v.c * m + d.c) CN_GSUM(c, +=)
        GB(x) GB(y) GB(z) GB(w)
#undef GB
        *(float4 *)(S.a + o) = a;
        float *gr = S.g + b * 4 * H + u0 + lc;
        *(float4 *)(gr) = dn;
        *(float4 *)(gr + H) = dr;
        *(float4 *)(gr + 2 * H) = dz;
        *(float4 *)(gr + 3 * H) = dhn;
    }
    if (!gates) return;
    // column sums of the tile (32 units x 4 gates) over its 128 rows: thread rows in order through LDS
    float *const red = smem + GF_BM * LDC;
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
    for (int r = 0; r < 32; ++r) s += src[r * 8 * 16];
    S.part[(int64_t)rt * 4 * H + q * H + u0 + cu] = s;
}

}  // namespace
