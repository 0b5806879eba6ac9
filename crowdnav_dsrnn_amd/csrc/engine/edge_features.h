// edge_features.h -- cn_edge_features' kernel: the three input embeddings of the DSRNN policy (robot node,
// temporal edge, spatial edges) assembled in one launch (srnn_model.py:160-161, 210-211, 466).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ------------------------------------------------------------------------------------------------
// fused DSRNN edge-feature assembly (srnn_model.py:160-161, 210-211, 466)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cn_edge_features_kernel(int64_t E, int N, const float *__restrict__ robot_node,
                                                               const float *__restrict__ temporal,
                                                               const float *__restrict__ spatial,
                                                               const float *__restrict__ Wt, const float *__restrict__ bt,
                                                               const float *__restrict__ Ws, const float *__restrict__ bs,
                                                               const float *__restrict__ Wr, const float *__restrict__ br,
                                                               const float *__restrict__ Wn, const float *__restrict__ bn,
                                                               float *__restrict__ t_out, float *__restrict__ s_out,
                                                               float *__restrict__ n_out)
{
    // one thread per (row, 4 output features); rows = E temporal + E*N spatial + E node
    const int64_t rows = E * (N + 2);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = idx >> 4;
    const int q = (int)(idx & 15) * 4;
    if (row >= rows) return;
    float o[4];
    if (row < E) {  // temporal edge: relu(Wt x + bt), x = robot velocity
        const float x0 = temporal[row * 2], x1 = temporal[row * 2 + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fmaxf(__fmaf_rn(Wt[(q + k) * 2 + 1], x1, __fmaf_rn(Wt[(q + k) * 2], x0, bt[q + k])), 0.0f);
        *(float4 *)(t_out + row * 64 + q) = make_float4(o[0], o[1], o[2], o[3]);
    } else if (row < E + E * N) {  // spatial edges
        const int64_t r = row - E;
        const float x0 = spatial[r * 2], x1 = spatial[r * 2 + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fmaxf(__fmaf_rn(Ws[(q + k) * 2 + 1], x1, __fmaf_rn(Ws[(q + k) * 2], x0, bs[q + k])), 0.0f);
        *(float4 *)(s_out + r * 64 + q) = make_float4(o[0], o[1], o[2], o[3]);
    } else {  // robot node: relu(Wn (Wr x + br) + bn)
        const int64_t r = row - E - E * N;
        float h[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float a = br[j];
#pragma unroll
            for (int k = 0; k < 7; ++k) a = __fmaf_rn(Wr[j * 7 + k], robot_node[r * 7 + k], a);
            h[j] = a;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a = bn[q + k];
#pragma unroll
            for (int j = 0; j < 3; ++j) a = __fmaf_rn(Wn[(q + k) * 3 + j], h[j], a);
            o[k] = fmaxf(a, 0.0f);
        }
        *(float4 *)(n_out + r * 64 + q) = make_float4(o[0], o[1], o[2], o[3]);
    }
}
