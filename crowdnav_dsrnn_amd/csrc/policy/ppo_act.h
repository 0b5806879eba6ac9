// ppo_act.h -- cn_gaussian_act_kernel, the act() tail of the Box-action policy. Needs nothing before it. Not in one
// header with ppo_gae.h: the kernels keep their places in the unit's code object, this one before the split-K kernels.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// The act() tail of the Box-action policy (distributions.py:74-94 DiagGaussian + FixedNormal, with the
// reference's operation order and torch's float32 arithmetic): std = exp(0 + logstd) (AddBias on zeros),
// action = eps * std + mean (sample; eps = torch.randn) or mean (mode), and
//   log_prob = sum_a [ -((action - mean)^2) / (2 std^2) - log(std) - log(sqrt(2 pi)) ]
// one thread per env: ~15 tiny torch launches per act() in one (the HIP-graph rollout replays them all).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cn_gaussian_act_kernel(int64_t E, int A, const float *__restrict__ mean,
                                                              const float *__restrict__ logstd,
                                                              const float *__restrict__ eps,
                                                              float *__restrict__ action, float *__restrict__ logp)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float c = 0.9189385332046727f;   // math.log(math.sqrt(2 * math.pi)) as torch's float32 scalar
    float lp = 0.0f;
    for (int a = 0; a < A; ++a) {
        const float sd = expf(0.0f + logstd[a]);
        const float mu = mean[e * A + a];
        const float x = eps ? eps[e * A + a] * sd + mu : mu;
        action[e * A + a] = x;
        const float d = x - mu;
        const float var = sd * sd;
        const float t = -(d * d) / (2.0f * var) - logf(sd) - c;
        lp = a ? lp + t : t;
    }
    logp[e] = lp;
}

}  // namespace
