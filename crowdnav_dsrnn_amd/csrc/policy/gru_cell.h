// gru_cell.h -- the element-wise GRU step: sigm, the gate arithmetic CN_GATE / CN_GBWD, the forward, backward and
// backward-with-bias kernels, the bias reductions. Needs nothing before it.
#pragma once

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// The gate arithmetic of one hidden unit, written once for every kernel of this unit: component c of the float4s
// named as below at the place of use.
// CN_GATE: r, z, n, h from the input parts ir / iz / in, the recurrent parts hr / hz / hn and the previous state hp.
#define CN_GATE(c)                                 \
    r.c = sigm(hr.c + ir.c);                       \
    z.c = sigm(hz.c + iz.c);                       \
    n.c = tanhf(in.c + hn.c * r.c);                \
    h.c = (hp.c - n.c) * z.c + n.c;
// CN_GATE_B: the fused kernels' form, the recurrent parts first from the GEMM's sums cr / cz / cn and b_hh (br / bz / bn).
#define CN_GATE_B(c)                               \
    hr.c = cr.c + br.c;                            \
    hz.c = cz.c + bz.c;                            \
    hn.c = cn.c + bn.c;                            \
    CN_GATE(c)
// CN_GBWD: the gate gradients a (direct path), dr, dz, dn, dhn from G = dL/dh of the component and the saved
// r, z, n, hn, hp. CN_GSUM: the column sums sr / sz / sn / shn take them (OP: += over a thread's rows, = for its one row).
#define CN_GBWD(c, G)                                             \
    {                                                             \
        const float gc = (G);                                     \
        const float dnc = gc * (1.0f - z.c) * (1.0f - n.c * n.c); \
        const float dzc = gc * (hp.c - n.c) * z.c * (1.0f - z.c); \
        const float drc = dnc * hn.c * r.c * (1.0f - r.c);        \
        a.c = gc * z.c;                                           \
        dr.c = drc;                                               \
        dz.c = dzc;                                               \
        dn.c = dnc;                                               \
        dhn.c = dnc * r.c;                                        \
    }
#define CN_GSUM(c, OP) sr.c OP dr.c; sz.c OP dz.c; sn.c OP dn.c; shn.c OP dhn.c;

// gi, gh: [B][3H] (r | z | n blocks); hm: [B][H] the masked previous state; m_next: [B] or null;
// h_out: [B][H]; hm_next: [B][H] or null (= h_out * m_next); save: [B][4H] (r | z | n | gh_n) or null;
// h_out2: a second copy of h_out in a grouped row layout (row b at (b / g2) * ld2 + (b % g2) * H), or null.
__global__ __launch_bounds__(256) void cn_gru_fwd_kernel(int64_t B, int H, const float *__restrict__ gi,
                                                         const float *__restrict__ gh,
                                                         const float *__restrict__ hm,
                                                         const float *__restrict__ m_next, float *__restrict__ h_out,
                                                         float *__restrict__ hm_next, float *__restrict__ save,
                                                         float *__restrict__ h_out2, int64_t g2, int64_t ld2)
{
    const int H4 = H >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H4) return;
    const int64_t b = i / H4;
    const int j = (int)(i - b * H4) * 4;
    const float4 ir = *(const float4 *)(gi + b * 3 * H + j);
    const float4 iz = *(const float4 *)(gi + b * 3 * H + H + j);
    const float4 in = *(const float4 *)(gi + b * 3 * H + 2 * H + j);
    const float4 hr = *(const float4 *)(gh + b * 3 * H + j);
    const float4 hz = *(const float4 *)(gh + b * 3 * H + H + j);
    const float4 hn = *(const float4 *)(gh + b * 3 * H + 2 * H + j);
    const float4 hp = *(const float4 *)(hm + b * H + j);
    float4 r, z, n, h;
    CN_GATE(x) CN_GATE(y) CN_GATE(z) CN_GATE(w)
    *(float4 *)(h_out + b * H + j) = h;
    if (h_out2) *(float4 *)(h_out2 + (b / g2) * ld2 + (b % g2) * H + j) = h;
    if (hm_next) {
        const float m = m_next ? m_next[b] : 1.0f;
        *(float4 *)(hm_next + b * H + j) = make_float4(h.x * m, h.y * m, h.z * m, h.w * m);
    }
    if (save) {
        float *s = save + b * 4 * H + j;
        *(float4 *)(s) = r;
        *(float4 *)(s + H) = z;
        *(float4 *)(s + 2 * H) = n;
        *(float4 *)(s + 3 * H) = hn;
    }
}

// Gradient of step t. g = acc * m_next + dout_t is dL/dh_t (acc = dL/dhm_{t+1} from the later step, or
// dL/dh_T at the last step with m_next = null). Writes dgi_t, dgh_t [B][3H] and acc <- g * z (the direct
// path of dL/dhm_t; the caller adds dgh_t @ W_hh).
__global__ __launch_bounds__(256) void cn_gru_bwd_kernel(int64_t B, int H, float *__restrict__ acc,
                                                         const float *__restrict__ m_next,
                                                         const float *__restrict__ dout,
                                                         const float *__restrict__ save,
                                                         const float *__restrict__ hm, float *__restrict__ dgi,
                                                         float *__restrict__ dgh)
{
    const int H4 = H >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H4) return;
    const int64_t b = i / H4;
    const int j = (int)(i - b * H4) * 4;
    const float m = m_next ? m_next[b] : 1.0f;
    float4 g = *(const float4 *)(acc + b * H + j);
    g = make_float4(g.x * m, g.y * m, g.z * m, g.w * m);
    if (dout) {
        const float4 d = *(const float4 *)(dout + b * H + j);
        g = make_float4(g.x + d.x, g.y + d.y, g.z + d.z, g.w + d.w);
    }
    const float *s = save + b * 4 * H + j;
    const float4 r = *(const float4 *)(s), z = *(const float4 *)(s + H), n = *(const float4 *)(s + 2 * H),
                 hn = *(const float4 *)(s + 3 * H);
    const float4 hp = *(const float4 *)(hm + b * H + j);
    float4 a, dr, dz, dn, dhn;
    CN_GBWD(x, g.x) CN_GBWD(y, g.y) CN_GBWD(z, g.z) CN_GBWD(w, g.w)
    *(float4 *)(acc + b * H + j) = a;
    *(float4 *)(dgi + b * 3 * H + j) = dr;
    *(float4 *)(dgi + b * 3 * H + H + j) = dz;
    *(float4 *)(dgi + b * 3 * H + 2 * H + j) = dn;
    *(float4 *)(dgh + b * 3 * H + j) = dr;
    *(float4 *)(dgh + b * 3 * H + H + j) = dz;
    *(float4 *)(dgh + b * 3 * H + 2 * H + j) = dhn;
}

// The same step with the bias gradients folded in (the reference's autograd sums dgi / dgh over all T*B
// rows for b_ih / b_hh: two passes over [T][B][3H] each). Workgroup = CN_GB_RW rows x H columns, thread
// (row slot, 4 columns); besides dgi / dgh it writes the workgroup's column sums of dr | dz | dn | dhn to
// part [blocks][4H] (row slots summed in order through LDS); cn_gru_bias_reduce adds the partials of all
// steps in order (deterministic).
#define CN_GB_RW 16
// COMB: the gate gradients go once to g = [dn | dr | dz | dhn] per row (4H; dgi's r / z columns equal dgh's,
// so dgh = g[:, H:4H] and dgi = g[:, 0:3H] with the input weights' rows taken in the order n, r, z) instead of
// the separate [dr | dz | dn] and [dr | dz | dhn] (6H): 2H fewer floats written per row and step
template <bool COMB>
__global__ __launch_bounds__(256) void cn_gru_bwd_bias_kernel(int64_t B, int H, float *__restrict__ acc,
                                                              const float *__restrict__ m_next,
                                                              const float *__restrict__ dout,
                                                              const float *__restrict__ save,
                                                              const float *__restrict__ hm, float *__restrict__ dgi,
                                                              float *__restrict__ dgh, float *__restrict__ part)
{
    __shared__ float4 red[256][4];
    const int H4 = H >> 2, slots = 256 / H4;   // H in {64, 128, 256}: 16 / 8 / 4 row slots
    const int rs = (int)threadIdx.x / H4, j = ((int)threadIdx.x - rs * H4) * 4;
    float4 sr = make_float4(0.f, 0.f, 0.f, 0.f), sz = sr, sn = sr, shn = sr;
    const int64_t b0 = (int64_t)blockIdx.x * CN_GB_RW;
    for (int k = rs; k < CN_GB_RW; k += slots) {
        const int64_t b = b0 + k;
        if (b >= B) break;
        const float m = m_next ? m_next[b] : 1.0f;
        float4 g = *(const float4 *)(acc + b * H + j);
        g = make_float4(g.x * m, g.y * m, g.z * m, g.w * m);
        if (dout) {
            const float4 d = *(const float4 *)(dout + b * H + j);
            g = make_float4(g.x + d.x, g.y + d.y, g.z + d.z, g.w + d.w);
        }
        const float *s = save + b * 4 * H + j;
        const float4 r = *(const float4 *)(s), z = *(const float4 *)(s + H), n = *(const float4 *)(s + 2 * H),
                     hn = *(const float4 *)(s + 3 * H);
        const float4 hp = *(const float4 *)(hm + b * H + j);
        float4 a, dr, dz, dn, dhn;
#define GB(c) CN_GBWD(c, g.c) CN_GSUM(c, +=)
        GB(x) GB(y) GB(z) GB(w)
#undef GB
        *(float4 *)(acc + b * H + j) = a;
        if (COMB) {
            float *gr = dgi + b * 4 * H + j;
            *(float4 *)(gr) = dn;
            *(float4 *)(gr + H) = dr;
            *(float4 *)(gr + 2 * H) = dz;
            *(float4 *)(gr + 3 * H) = dhn;
        } else {
            *(float4 *)(dgi + b * 3 * H + j) = dr;
            *(float4 *)(dgi + b * 3 * H + H + j) = dz;
            *(float4 *)(dgi + b * 3 * H + 2 * H + j) = dn;
            *(float4 *)(dgh + b * 3 * H + j) = dr;
            *(float4 *)(dgh + b * 3 * H + H + j) = dz;
            *(float4 *)(dgh + b * 3 * H + 2 * H + j) = dhn;
        }
    }
    red[threadIdx.x][0] = sr; red[threadIdx.x][1] = sz; red[threadIdx.x][2] = sn; red[threadIdx.x][3] = shn;
    __syncthreads();
    if (rs != 0) return;
    for (int q = 1; q < slots; ++q) {
        const float4 *o = red[q * H4 + threadIdx.x];
        sr.x += o[0].x; sr.y += o[0].y; sr.z += o[0].z; sr.w += o[0].w;
        sz.x += o[1].x; sz.y += o[1].y; sz.z += o[1].z; sz.w += o[1].w;
        sn.x += o[2].x; sn.y += o[2].y; sn.z += o[2].z; sn.w += o[2].w;
        shn.x += o[3].x; shn.y += o[3].y; shn.z += o[3].z; shn.w += o[3].w;
    }
    float *pw = part + (int64_t)blockIdx.x * 4 * H + j;
    *(float4 *)(pw) = sr;
    *(float4 *)(pw + H) = sz;
    *(float4 *)(pw + 2 * H) = sn;
    *(float4 *)(pw + 3 * H) = shn;
}

// db_ih = (sum dr, sum dz, sum dn), db_hh = (sum dr, sum dz, sum dhn) over the rows of part [rows][4H]
// (every step's workgroup partials), in two deterministic passes: CN_GB_RC row chunks x 64-column slices
// (thread = column, the workgroup's 4 waves stride the chunk's rows, LDS sum in wave order) into
// work [CN_GB_RC][4H], then the chunks in order.
#define CN_GB_RC 64
__global__ __launch_bounds__(256) void cn_gru_bias_part2_kernel(int64_t rows, int H, const float *__restrict__ part,
                                                                float *__restrict__ work)
{
    __shared__ float red[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6, rc = blockIdx.y;
    const int64_t chunk = (rows + CN_GB_RC - 1) / CN_GB_RC, r0 = rc * chunk;
    const int64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
    float s = 0.0f;
    if (col < 4 * H)
        for (int64_t r = r0 + w; r < r1; r += 4) s += part[r * 4 * H + col];
    red[w][threadIdx.x & 63] = s;
    __syncthreads();
    if (w != 0 || col >= 4 * H) return;
    work[(int64_t)rc * 4 * H + col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void cn_gru_bias_final_kernel(int H, const float *__restrict__ work,
                                                                float *__restrict__ db_ih, float *__restrict__ db_hh)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= 4 * H) return;
    float s = 0.0f;
    for (int rc = 0; rc < CN_GB_RC; ++rc) s += work[rc * 4 * H + col];
    const int gate = col / H, u = col - gate * H;
    if (gate < 2) { db_ih[col] = s; db_hh[col] = s; }
    else if (gate == 2) db_ih[2 * H + u] = s;
    else db_hh[2 * H + u] = s;
}

}  // namespace
