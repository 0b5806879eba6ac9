// wgrad.h -- skinny weight gradients: cn_wgrad_part_kernel, cn_wgrad_sum_kernel, wgrad_grid. Needs nothing before
// it.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// Skinny weight gradient of a Linear layer applied to K >> 1 rows (PPO minibatch: T*B or T*B*N rows):
//   dW[a][j] = sum_k dy'[k][a] x[k][j],  db[a] = sum_k dy'[k][a],  dy' = dy * (relu_out > 0) if given
// for layers whose output or input width is tiny (the DSRNN input encoders: 2 / 3 / 7 inputs; the action
// mean and value heads: 2 / 1 outputs), where a library GEMM walks all of K with a handful of output
// tiles (4.1 ms for the spatial encoder's 64 x 2 gradient over 2.6 M rows). HBM-bound:
// one pass over dy (+ the ReLU output) and x. Each workgroup owns a contiguous run of rows and keeps the
// m*n + m sums of its rows in registers (thread t: slots t, t + 256, ...); the per-workgroup partials are
// then summed in workgroup order by a second kernel (deterministic, no atomics).
// ------------------------------------------------------------------------------------------------
#define CN_WG_MAXSLOT 1024
#define CN_WG_NARROW 8

// Layout: each thread owns VEC consecutive columns of the WIDE operand (dy if DYWIDE, else x; <= 256
// columns, TW = ceil(wide / VEC) threads per row, 256 / TW rows in flight) and all columns of the NARROW
// one (<= 8); rows are read as coalesced vectors. The 256 / TW row slots are summed through LDS in slot
// order, then one partial row of m * n + m sums per workgroup.
template <int VEC, bool DYWIDE>
__global__ __launch_bounds__(256) void cn_wgrad_part_kernel(int64_t K, int m, int n, int TW, int64_t rows,
                                                            const float *__restrict__ dy,
                                                            const float *__restrict__ mo,
                                                            const float *__restrict__ x,
                                                            float *__restrict__ part)
{
    __shared__ float red[256 * (VEC * CN_WG_NARROW + CN_WG_NARROW)];
    constexpr int NA = CN_WG_NARROW, NB = VEC > NA ? VEC : NA;
    const int wide = DYWIDE ? m : n, nar = DYWIDE ? n : m;
    const int RP = 256 / TW, tr = (int)threadIdx.x / TW, tc = (int)threadIdx.x - tr * TW;
    const int c0 = tc * VEC;
    const bool act = tr < RP && c0 < wide;
    const int64_t k0 = (int64_t)blockIdx.x * rows;
    const int64_t k1 = k0 + rows < K ? k0 + rows : K;
    float acc[VEC][NA], dbs[NB];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
        for (int u = 0; u < NA; ++u) acc[v][u] = 0.0f;
#pragma unroll
    for (int u = 0; u < NB; ++u) dbs[u] = 0.0f;
    if (act) {
        for (int64_t k = k0 + tr; k < k1; k += RP) {
            float w[VEC], q[NA];
            const float *wr = DYWIDE ? dy + k * m : x + k * n;
            if (VEC == 4) {
                const float4 t = *(const float4 *)(wr + c0);
                w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
                if (DYWIDE && mo) {
                    const float4 o = *(const float4 *)(mo + k * m + c0);
                    w[0] = o.x > 0.0f ? w[0] : 0.0f; w[1] = o.y > 0.0f ? w[1] : 0.0f;
                    w[2] = o.z > 0.0f ? w[2] : 0.0f; w[3] = o.w > 0.0f ? w[3] : 0.0f;
                }
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    w[v] = c0 + v < wide ? wr[c0 + v] : 0.0f;
                    if (DYWIDE && mo && c0 + v < wide && !(mo[k * m + c0 + v] > 0.0f)) w[v] = 0.0f;
                }
            }
            const float *qr = DYWIDE ? x + k * n : dy + k * m;
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                q[u] = u < nar ? qr[u] : 0.0f;
                if (!DYWIDE && mo && u < nar && !(mo[k * m + u] > 0.0f)) q[u] = 0.0f;
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v)
#pragma unroll
                for (int u = 0; u < NA; ++u) acc[v][u] += w[v] * q[u];
            if (DYWIDE) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) dbs[v] += w[v];
            } else {
#pragma unroll
                for (int u = 0; u < NA; ++u) dbs[u] += q[u];
            }
        }
    }
    // sum the RP row slots in slot order: thread (tr, tc) stores its sums, then thread tc of slot 0 adds up
    constexpr int SL = VEC * NA + NA;
    float *mine = red + threadIdx.x * SL;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
        for (int u = 0; u < NA; ++u) mine[v * NA + u] = acc[v][u];
#pragma unroll
    for (int u = 0; u < NA; ++u) mine[VEC * NA + u] = u < NB ? dbs[u] : 0.0f;
    __syncthreads();
    if (tr != 0 || c0 >= wide) return;
    for (int r = 1; r < RP; ++r) {
        const float *o = red + (r * TW + tc) * SL;
#pragma unroll
        for (int v = 0; v < VEC; ++v)
#pragma unroll
            for (int u = 0; u < NA; ++u) acc[v][u] += o[v * NA + u];
#pragma unroll
        for (int u = 0; u < NB; ++u) dbs[u] += o[VEC * NA + u];
    }
    const int P = m * n;
    float *pw = part + (int64_t)blockIdx.x * (P + m);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        if (c0 + v >= wide) continue;
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            if (u >= nar) continue;
            if (DYWIDE) pw[(c0 + v) * n + u] = acc[v][u];   // dW[a = c0 + v][j = u]
            else pw[u * n + c0 + v] = acc[v][u];            // dW[a = u][j = c0 + v]
        }
        if (DYWIDE) pw[P + c0 + v] = dbs[v];
    }
    if (!DYWIDE && tc == 0)
        for (int u = 0; u < nar; ++u) pw[P + u] = dbs[u];
}

// out[p] = sum over the G workgroup partials in workgroup order (one workgroup per output: strided
// sequential sums, then a fixed-order LDS tree)
__global__ __launch_bounds__(256) void cn_wgrad_sum_kernel(int G, int m, int n, const float *__restrict__ part,
                                                           float *__restrict__ dW, float *__restrict__ db)
{
    __shared__ float red[256];
    const int P = m * n, S = P + m;
    const int p = blockIdx.x;
    float s = 0.0f;
    for (int g = threadIdx.x; g < G; g += 256) s += part[(int64_t)g * S + p];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (p < P) dW[p] = red[0];
        else if (db) db[p - P] = red[0];
    }
}

// rows per workgroup and workgroup count of cn_wgrad for K rows (about four workgroups per CU)
static inline void wgrad_grid(int64_t K, int64_t &rows, int &G)
{
    rows = (K + 1023) / 1024;
    if (rows < 64) rows = 64;
    G = (int)((K + rows - 1) / rows);
}

}  // namespace
