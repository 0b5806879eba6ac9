// The lattice action head of the unicycle robot (cn_lattice_act / cn_lattice_eval_fwd / cn_lattice_eval_bwd): a
// categorical distribution over cn_dwa_predict's 64 candidate actions, defined in include/crowdnav.h; and its soft-label
// loss against the controller's regret rows (cn_lattice_soft_fwd / cn_lattice_soft_bwd).
//
// One shape for the five kernels: a 64-lane wavefront owns a row of 64 logits, lane c holds candidate c; a 256-thread
// workgroup serves 4 consecutive rows. Maximum, sum and entropy are xor butterflies (every lane ends with the same
// bits: each level adds the same two partial sums in both partners), the inclusive prefix sums a 6-step shuffle
// scan, the lowest / highest lane of a predicate a ballot. No LDS, no scratch, no atomics, no memset; a row's wave
// reads and writes that row only, so a launch is stream-ordered and graph-capturable like any other.
// Cross-lane reads: a wave whose row lies past the end leaves as a whole (the row index is wave-uniform) before the
// first shuffle and there is no other branch around one, so every lane a shuffle or ballot reads is active.
//
// A translation unit of its own: the code objects of cn_engine.hip and cn_gru.hip do not move.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

#include "../../include/crowdnav.h"
#include "cn_host.h"   // cn_set_error, launch_status

namespace {

constexpr int ROWS = 4;   // rows (wavefronts) per 256-thread workgroup

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// inclusive prefix sums over the 64 lanes
__device__ __forceinline__ float wave_scan(float v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// the row's softmax pieces in lane `lane`: p = expf(l - m), Z, logp = (l - m) - logf(Z)
struct Row {
    float m, p, Z, logp;
};

__device__ __forceinline__ Row softmax_row(float l)
{
    Row r;
    r.m = wave_max(l);
    const float d = l - r.m;
    r.p = expf(d);
    r.Z = wave_sum(r.p);
    r.logp = d - logf(r.Z);
    return r;
}

// H = -sum over p_j > 0 of (p_j / Z) * logp_j
__device__ __forceinline__ float entropy_row(const Row &r)
{
    return -wave_sum(r.p > 0.0f ? (r.p / r.Z) * r.logp : 0.0f);
}

// candidate c = 8 a + b -> (dv, dth): cn_dwa_predict's values
__device__ __forceinline__ float lattice_value(int k) { return (float)((0.1 * (double)(2 * k - 7)) / 7.0); }

// nearest lattice coordinate of one action component (NaN -> 0)
__device__ __forceinline__ int lattice_coord(float x)
{
    const float r = rintf((x * 70.0f + 7.0f) * 0.5f);
    return (int)fminf(fmaxf(r, 0.0f), 7.0f);
}

__device__ __forceinline__ int lowest(uint64_t w) { return __builtin_ctzll(w); }
__device__ __forceinline__ int highest(uint64_t w) { return 63 - __builtin_clzll(w); }

__global__ __launch_bounds__(256) void cn_lattice_act_kernel(int64_t E, const float *__restrict__ logits,
                                                             const float *__restrict__ u,
                                                             float *__restrict__ action, float *__restrict__ logp,
                                                             int32_t *__restrict__ choice)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * ROWS + ((int)threadIdx.x >> 6);
    if (e >= E) return;   // wave-uniform
    const float l = logits[e * 64 + lane];
    const Row r = softmax_row(l);
    int c;
    if (u) {
        const float S = wave_scan(r.p, lane);
        const float thr = u[e] * __shfl(S, 63);
        // the scan's sums need not be monotonic in their last bits: p > 0 is part of the rule, not implied by it
        const uint64_t over = __ballot(S > thr && r.p > 0.0f);
        const uint64_t live = __ballot(r.p > 0.0f);
        c = over ? lowest(over) : (live ? highest(live) : 0);
    } else {
        const uint64_t top = __ballot(l == r.m);
        c = top ? lowest(top) : 0;   // (a NaN row has no defined mode)
    }
    const float lp = __shfl(r.logp, c);
    if (lane == 0) {
        action[e * 2] = lattice_value(c >> 3);
        action[e * 2 + 1] = lattice_value(c & 7);
        logp[e] = lp;
        if (choice) choice[e] = c;
    }
}

__global__ __launch_bounds__(256) void cn_lattice_eval_fwd_kernel(int64_t B, const float *__restrict__ logits,
                                                                  const float *__restrict__ actions,
                                                                  float *__restrict__ logp,
                                                                  float *__restrict__ entropy,
                                                                  int32_t *__restrict__ choice)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;   // wave-uniform
    const Row r = softmax_row(logits[e * 64 + lane]);
    const float H = entropy_row(r);
    const int c = 8 * lattice_coord(actions[e * 2]) + lattice_coord(actions[e * 2 + 1]);
    const float lp = __shfl(r.logp, c);
    if (lane == 0) {
        logp[e] = lp;
        entropy[e] = H;
        choice[e] = c;
    }
}

__global__ __launch_bounds__(256) void cn_lattice_eval_bwd_kernel(int64_t B, const float *__restrict__ logits,
                                                                  const int32_t *__restrict__ choice,
                                                                  const float *__restrict__ g_logp,
                                                                  const float *__restrict__ g_entropy,
                                                                  float *__restrict__ dlogits)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;   // wave-uniform
    const Row r = softmax_row(logits[e * 64 + lane]);
    const float H = entropy_row(r);
    const float q = r.p / r.Z;
    const float glp = g_logp[e], gH = g_entropy[e];
    const float onehot = lane == choice[e] ? 1.0f : 0.0f;   // (compared only, never an index)
    float d = glp * onehot;
    if (q != 0.0f) d = glp * (onehot - q) - gH * q * (r.logp + H);
    dlogits[e * 64 + lane] = d;
}

// ------------------------------------------------------------------------------------------------
// Soft labels (cn_lattice_soft_fwd / cn_lattice_soft_bwd, include/crowdnav.h): the cross-entropy of the row's softmax
// against the target the expert's 64 regrets define at temperature tau, q = softmax(-(r - min r) / tau). The same
// shape as the three kernels above, which they follow in this file so that those keep their places in the code object.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// the target's pieces in lane `lane`: a = r - min r, x = -(a * inv_tau), t = expf(x), Zt = sum t, q = t / Zt
struct Target {
    float a, x, Zt, q;
};

__device__ __forceinline__ Target target_row(float r, float inv_tau)
{
    Target g;
    g.a = r - wave_min(r);
    g.x = -(g.a * inv_tau);
    const float t = expf(g.x);
    g.Zt = wave_sum(t);
    g.q = t / g.Zt;
    return g;
}

__global__ __launch_bounds__(256) void cn_lattice_soft_fwd_kernel(int64_t B, const float *__restrict__ logits,
                                                                  const float *__restrict__ regret, float inv_tau,
                                                                  float *__restrict__ ce, float *__restrict__ kl,
                                                                  float *__restrict__ logp_best)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;   // wave-uniform
    const Row r = softmax_row(logits[e * 64 + lane]);
    const Target g = target_row(regret[e * 64 + lane], inv_tau);
    const bool on = g.q > 0.0f;
    const float c = -wave_sum(on ? g.q * r.logp : 0.0f);
    const float Hq = -wave_sum(on ? g.q * (g.x - logf(g.Zt)) : 0.0f);
    const uint64_t zero = __ballot(g.a == 0.0f);
    const float lb = __shfl(r.logp, zero ? lowest(zero) : 0);   // (a NaN row has no best candidate)
    if (lane == 0) {
        ce[e] = c;
        if (kl) kl[e] = c - Hq;
        if (logp_best) logp_best[e] = lb;
    }
}

__global__ __launch_bounds__(256) void cn_lattice_soft_bwd_kernel(int64_t B, const float *__restrict__ logits,
                                                                  const float *__restrict__ regret, float inv_tau,
                                                                  const float *__restrict__ g_ce,
                                                                  float *__restrict__ dlogits)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * ROWS + ((int)threadIdx.x >> 6);
    if (e >= B) return;   // wave-uniform
    const Row r = softmax_row(logits[e * 64 + lane]);
    const Target g = target_row(regret[e * 64 + lane], inv_tau);
    dlogits[e * 64 + lane] = g_ce[e] * (r.p / r.Z - g.q);
}

int lattice_check(const char *who, int64_t rows, std::initializer_list<const void *> need)
{
    if (rows <= 0 || rows > (int64_t)0x7fffffff * ROWS) return cn_set_error(CN_EINVAL, who);
    for (const void *p : need)
        if (!p) return cn_set_error(CN_EINVAL, who);
    return CN_OK;
}

inline unsigned row_grid(int64_t rows) { return (unsigned)((rows + ROWS - 1) / ROWS); }

}  // namespace

extern "C" {

int cn_lattice_act(void *stream, int64_t E, const float *logits, const float *u, float *action, float *logp,
                   int32_t *choice)
{
    if (lattice_check("cn_lattice_act: E > 0 and non-null logits, action, logp required", E, {logits, action, logp}))
        return CN_EINVAL;
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_lattice_act_kernel, dim3(row_grid(E)), dim3(256), 0, (hipStream_t)stream, E, logits, u,
                       action, logp, choice);
    return launch_status();
}

int cn_lattice_eval_fwd(void *stream, int64_t B, const float *logits, const float *actions, float *logp,
                        float *entropy, int32_t *choice)
{
    if (lattice_check("cn_lattice_eval_fwd: B > 0 and non-null logits, actions, logp, entropy, choice required", B,
                      {logits, actions, logp, entropy, choice}))
        return CN_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_lattice_eval_fwd_kernel, dim3(row_grid(B)), dim3(256), 0, (hipStream_t)stream, B, logits,
                       actions, logp, entropy, choice);
    return launch_status();
}

int cn_lattice_eval_bwd(void *stream, int64_t B, const float *logits, const int32_t *choice, const float *g_logp,
                        const float *g_entropy, float *dlogits)
{
    if (lattice_check("cn_lattice_eval_bwd: B > 0 and non-null logits, choice, g_logp, g_entropy, dlogits required", B,
                      {logits, choice, g_logp, g_entropy, dlogits}))
        return CN_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_lattice_eval_bwd_kernel, dim3(row_grid(B)), dim3(256), 0, (hipStream_t)stream, B, logits,
                       choice, g_logp, g_entropy, dlogits);
    return launch_status();
}

int cn_lattice_soft_fwd(void *stream, int64_t B, const float *logits, const float *regret, float inv_tau, float *ce,
                        float *kl, float *logp_best)
{
    if (lattice_check("cn_lattice_soft_fwd: B > 0 and non-null logits, regret, ce required", B, {logits, regret, ce}))
        return CN_EINVAL;
    if (!(inv_tau > 0.0f && inv_tau < __builtin_inff()))   // (a NaN fails both)
        return cn_set_error(CN_EINVAL, "cn_lattice_soft_fwd: a finite inv_tau > 0 required");
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_lattice_soft_fwd_kernel, dim3(row_grid(B)), dim3(256), 0, (hipStream_t)stream, B, logits,
                       regret, inv_tau, ce, kl, logp_best);
    return launch_status();
}

int cn_lattice_soft_bwd(void *stream, int64_t B, const float *logits, const float *regret, float inv_tau,
                        const float *g_ce, float *dlogits)
{
    if (lattice_check("cn_lattice_soft_bwd: B > 0 and non-null logits, regret, g_ce, dlogits required", B,
                      {logits, regret, g_ce, dlogits}))
        return CN_EINVAL;
    if (!(inv_tau > 0.0f && inv_tau < __builtin_inff()))
        return cn_set_error(CN_EINVAL, "cn_lattice_soft_bwd: a finite inv_tau > 0 required");
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_lattice_soft_bwd_kernel, dim3(row_grid(B)), dim3(256), 0, (hipStream_t)stream, B, logits,
                       regret, inv_tau, g_ce, dlogits);
    return launch_status();
}

}  // extern "C"
