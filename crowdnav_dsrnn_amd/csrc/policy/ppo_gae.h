// ppo_gae.h -- cn_gae_kernel, generalized advantage estimation. Needs nothing before it. Not in one header with
// ppo_act.h: the kernels keep their places in the unit's code object, this one behind the split-K kernels.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// Generalized advantage estimation (storage.py:132-177, use_gae with use_proper_time_limits): one thread per
// env scans the steps backwards with the reference's float32 operation order
//   delta = ((r[s] + (gamma * v[s+1]) * m[s+1]) - v[s]);  gae = delta + (gl * m[s+1]) * gae;  gae *= bm[s+1]
//   ret[s] = gae + v[s]
// (gl = gamma * gae_lambda rounded once to float, as torch's scalar operands are): ~11 tiny torch launches
// per step (1,400 per rollout) in one.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cn_gae_kernel(int T, int64_t E, float gamma, float gl, int time_limits,
                                                     const float *__restrict__ r, const float *__restrict__ v,
                                                     const float *__restrict__ m, const float *__restrict__ bm,
                                                     float *__restrict__ ret)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float gae = 0.0f;
    for (int s = T - 1; s >= 0; --s) {
        const float v1 = v[(int64_t)(s + 1) * E + e], m1 = m[(int64_t)(s + 1) * E + e], v0 = v[(int64_t)s * E + e];
        const float delta = (r[(int64_t)s * E + e] + (gamma * v1) * m1) - v0;
        gae = delta + (gl * m1) * gae;
        if (time_limits) gae = gae * bm[(int64_t)(s + 1) * E + e];
        ret[(int64_t)s * E + e] = gae + v0;
    }
}

}  // namespace
