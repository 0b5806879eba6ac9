// policy_api.h -- extern "C": the policy functions of include/crowdnav.h that this unit serves, by topic. Needs every
// section before it and cn_host.h (cn_set_error, grid_for, aligned16, launch_status, CN_SA_LAUNCH).
#pragma once

namespace {

static int launch_fwd_fused(hipStream_t st, GfArgs &P, int64_t B0, int64_t B1, int H)
{
    const int64_t bm = row_tile(B0 + B1, H);
    const int64_t rt0 = (B0 + bm - 1) / bm, rt1 = (B1 + bm - 1) / bm;
    const int ut = H / GF_BU;
    const int64_t grid = (rt0 + rt1 + 7) / 8 * 8 * ut;
    if (grid > 0x7fffffff) return cn_set_error(CN_EINVAL, "fused GRU step: B too large");
    P.rt0 = (int)rt0;
    P.rt_total = (int)(rt0 + rt1);
    P.unit_tiles = ut;
    P.H = H;
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    const bool xm = P.s0.x != nullptr;
    if (bm == SK_BM) {
        if (xm)
            hipLaunchKernelGGL(cn_gru_fused_sk_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL(cn_gru_fused_sk_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, P);
    } else {
        if (xm)
            hipLaunchKernelGGL(cn_gru_fused_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL(cn_gru_fused_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, P);
    }
    return launch_status();
}

}  // namespace

extern "C" {

// ---- GRU: the element-wise steps, the fused steps and sequences, the bias reductions ----

int cn_gru_fwd_step(void *stream, int64_t B, int H, const float *gi, const float *gh, const float *hm,
                    const float *m_next, float *h_out, float *hm_next, float *save)
{
    return cn_gru_fwd_step_scatter(stream, B, H, gi, gh, hm, m_next, h_out, hm_next, save, nullptr, 1, 0);
}

int cn_gru_fwd_step_scatter(void *stream, int64_t B, int H, const float *gi, const float *gh, const float *hm,
                         const float *m_next, float *h_out, float *hm_next, float *save, float *h_out2, int64_t g2,
                         int64_t ld2)
{
    if (B <= 0 || H <= 0 || (H & 3)) return cn_set_error(CN_EINVAL, "cn_gru_fwd_step: B > 0 and H % 4 == 0 required");
    if (!gi || !gh || !hm || !h_out) return cn_set_error(CN_EINVAL, "cn_gru_fwd_step: null operand");
    if (B * (H / 4) > (int64_t)0xffffffff * 256) return cn_set_error(CN_EINVAL, "cn_gru_fwd_step: B too large");
    if (h_out2 && (g2 <= 0 || ld2 < g2 * H || (ld2 & 3) || ((uintptr_t)h_out2 & 15)))
        return cn_set_error(CN_EINVAL, "cn_gru_fwd_step_scatter: g2 > 0, ld2 >= g2 * H, ld2 % 4 == 0, 16-byte aligned h_out2");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_gru_fwd_kernel, dim3(grid_for(B, H)), dim3(256), 0, (hipStream_t)stream, B, H, gi, gh,
                       hm, m_next, h_out, hm_next, save, h_out2, h_out2 ? g2 : (int64_t)1, ld2);
    return launch_status();
}

int cn_gru_fwd_fused(void *stream, int64_t B, int H, const float *gi, const float *hm, const float *w_hh,
                     const float *b_hh, const float *m_next, float *h_out, float *hm_next, float *save, float *h_out2,
                     int64_t g2, int64_t ld2)
{
    if (B <= 0 || H <= 0 || H % GF_BU) return cn_set_error(CN_EINVAL, "cn_gru_fwd_fused: B > 0 and H % 32 == 0 required");
    if (!gi || !hm || !w_hh || !b_hh || !h_out) return cn_set_error(CN_EINVAL, "cn_gru_fwd_fused: null operand");
    // every operand the kernel touches with 16-byte vectors (float4 loads of hm, w_hh, gi, b_hh; float4 stores
    // of h_out, hm_next, save); h_out2 is checked below
    if ((((uintptr_t)hm) | ((uintptr_t)w_hh) | ((uintptr_t)gi) | ((uintptr_t)b_hh) | ((uintptr_t)h_out) |
         ((uintptr_t)hm_next) | ((uintptr_t)save)) & 15)
        return cn_set_error(CN_EINVAL, "cn_gru_fwd_fused: hm, w_hh, gi, b_hh, h_out, hm_next and save must be 16-byte aligned");
    if (h_out2 && (g2 <= 0 || ld2 < g2 * H))
        return cn_set_error(CN_EINVAL, "cn_gru_fwd_fused: g2 > 0 and ld2 >= g2 * H required");
    GfArgs P{};
    P.s0 = GfSeg{B, gi, hm, w_hh, b_hh, m_next, h_out, hm_next, save, h_out2, h_out2 ? g2 : (int64_t)1, ld2,
                 nullptr, nullptr, nullptr, 0};
    P.s1 = P.s0;
    return launch_fwd_fused((hipStream_t)stream, P, B, 0, H);
}

int cn_gru_fwd_step_group(void *stream, int H, int nseg, const cn_gru_step_seg *segs)
{
    if (H <= 0 || H % GF_BU || nseg < 1 || nseg > 2 || !segs)
        return cn_set_error(CN_EINVAL, "cn_gru_fwd_step_group: H % 32 == 0 and 1 <= nseg <= 2 required");
    GfArgs P{};
    for (int s = 0; s < nseg; ++s) {
        const cn_gru_step_seg &q = segs[s];
        if (q.B <= 0 || !q.hm || !q.w_hh || !q.b_hh || !q.h_out)
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_step_group: B > 0 and hm, w_hh, b_hh, h_out required");
        if ((q.x != nullptr) != (segs[0].x != nullptr))
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_step_group: every GRU of a call passes gi, or every GRU x");
        if (q.x ? (!q.w_ih || !q.b_ih || q.F <= 0 || q.F % GF_KC) : !q.gi)
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_step_group: gi, or x with w_ih, b_ih and F % 32 == 0, required");
        if (!aligned16({q.gi, q.x, q.w_ih, q.b_ih, q.hm, q.w_hh, q.b_hh, q.h_out}))
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_step_group: every array must be 16-byte aligned");
        if (q.h_out2 && (q.g2 <= 0 || q.ld2 < q.g2 * H))
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_step_group: g2 > 0 and ld2 >= g2 * H required");
        GfSeg g{q.B, q.gi, q.hm, q.w_hh, q.b_hh, nullptr, q.h_out, nullptr, nullptr, q.h_out2,
                q.h_out2 ? q.g2 : (int64_t)1, q.ld2, q.x, q.w_ih, q.b_ih, q.F};
        (s ? P.s1 : P.s0) = g;
    }
    if (nseg == 1) P.s1 = P.s0;
    return launch_fwd_fused((hipStream_t)stream, P, segs[0].B, nseg > 1 ? segs[1].B : 0, H);
}

int cn_gru_fwd_seq(void *stream, int T, int H, int nseg, const cn_gru_seq_fwd *segs)
{
    if (T <= 0 || H <= 0 || H % GF_BU || nseg < 1 || nseg > 2 || !segs)
        return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: T > 0, H % 32 == 0 and 1 <= nseg <= 2 required");
    for (int s = 0; s < nseg; ++s) {
        const cn_gru_seq_fwd &q = segs[s];
        if (q.B <= 0 || q.nh < 1 || q.nh > T) return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: B > 0 and 1 <= nh <= T required");
        // step t reads hm[t % nh] in every workgroup while others write their columns of hm[(t + 1) % nh]: with
        // nh == 1 and T > 1 those are the same rows (a cross-workgroup race); the backward reads hm of every step
        if (T > 1 && q.nh < 2) return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: nh >= 2 required when T > 1");
        if (q.save && q.nh != T) return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: nh == T required with save");
        if (!q.w_hh || !q.b_hh || !q.m || !q.out || !q.hm) return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: null operand");
        if ((q.x != nullptr) != (segs[0].x != nullptr))
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: every GRU of a call passes gi, or every GRU x / w_ih / b_ih");
        if (q.x ? (!q.w_ih || !q.b_ih || q.F <= 0 || q.F % GF_KC) : !q.gi)
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: gi, or x with w_ih, b_ih and F % 32 == 0, required");
        if (!aligned16({q.gi, q.w_hh, q.b_hh, q.out, q.hm, q.save, q.x, q.w_ih, q.b_ih}))
            return cn_set_error(CN_EINVAL, "cn_gru_fwd_seq: every array must be 16-byte aligned");
    }
    const int64_t B1 = nseg > 1 ? segs[1].B : 0;
    for (int t = 0; t < T; ++t) {
        GfArgs P{};
        for (int s = 0; s < nseg; ++s) {
            const cn_gru_seq_fwd &q = segs[s];
            const bool last = t + 1 == T;
            const int64_t BH = q.B * H;
            GfSeg g{q.B, q.gi ? q.gi + t * 3 * BH : nullptr, q.hm + (t % q.nh) * BH, q.w_hh, q.b_hh,
                    last ? nullptr : q.m + (t + 1) * q.B, q.out + t * BH,
                    last ? nullptr : q.hm + ((t + 1) % q.nh) * BH, q.save ? q.save + t * 4 * BH : nullptr, nullptr,
                    1, 0,
                    q.x ? q.x + t * q.B * q.F : nullptr, q.w_ih, q.b_ih, q.F};
            (s ? P.s1 : P.s0) = g;
        }
        if (nseg == 1) P.s1 = P.s0;
        const int rc = launch_fwd_fused((hipStream_t)stream, P, segs[0].B, B1, H);
        if (rc) return rc;
    }
    return CN_OK;
}

// workspace of cn_gru_bwd_seq: per GRU the bias partials [T][row tiles][4H], then cn_gru_bias_reduce's work
static int64_t bwd_part_rows(int64_t B, int64_t bm) { return (B + bm - 1) / bm; }

int64_t cn_gru_bwd_seq_work_elems(int T, int H, int nseg, const cn_gru_seq_bwd *segs)
{
    if (T <= 0 || H <= 0 || nseg < 1 || nseg > 2 || !segs) return 0;
    const int64_t rows = segs[0].B + (nseg > 1 ? segs[1].B : 0);
    const int64_t bm = row_tile(rows, H);
    int64_t n = (int64_t)CN_GB_RC * 4 * H;
    for (int s = 0; s < nseg; ++s) n += (int64_t)T * bwd_part_rows(segs[s].B, bm) * 4 * H;
    return n;
}

int cn_gru_bwd_seq(void *stream, int T, int H, int nseg, const cn_gru_seq_bwd *segs, float *work, int64_t work_elems)
{
    if (T <= 0 || H <= 0 || H % GF_BU || nseg < 1 || nseg > 2 || !segs)
        return cn_set_error(CN_EINVAL, "cn_gru_bwd_seq: T > 0, H % 32 == 0 and 1 <= nseg <= 2 required");
    if (!work) return cn_set_error(CN_EINVAL, "cn_gru_bwd_seq: null workspace");
    for (int s = 0; s < nseg; ++s) {
        const cn_gru_seq_bwd &q = segs[s];
        if (q.B <= 0) return cn_set_error(CN_EINVAL, "cn_gru_bwd_seq: B > 0 required");
        if (!q.w_hh_t || !q.m || !q.save || !q.hm || !q.acc || !q.g || !q.db_ih || !q.db_hh)
            return cn_set_error(CN_EINVAL, "cn_gru_bwd_seq: null operand");
        if (!aligned16({q.w_hh_t, q.dout, q.save, q.hm, q.acc, q.g}))
            return cn_set_error(CN_EINVAL, "cn_gru_bwd_seq: w_hh_t, dout, save, hm, acc and g must be 16-byte aligned");
    }
    // the row tiling (and with it the workspace) follows the CU count of the CURRENT device: a workspace sized on
    // another device may be too small for this one's choice
    if (work_elems < cn_gru_bwd_seq_work_elems(T, H, nseg, segs))
        return cn_set_error(CN_EINVAL, "cn_gru_bwd_seq: workspace smaller than cn_gru_bwd_seq_work_elems on this device");
    const int ut = H / GF_BU;
    const int64_t bm = row_tile(segs[0].B + (nseg > 1 ? segs[1].B : 0), H);
    const int64_t rt0 = bwd_part_rows(segs[0].B, bm), rt1 = nseg > 1 ? bwd_part_rows(segs[1].B, bm) : 0;
    const int64_t grid = (rt0 + rt1 + 7) / 8 * 8 * ut;
    if (grid > 0x7fffffff) return cn_set_error(CN_EINVAL, "cn_gru_bwd_seq: B too large");
    float *part[2] = {work, work + (int64_t)T * rt0 * 4 * H};
    float *red = part[1] + (int64_t)T * rt1 * 4 * H;
    // launch j = 0 .. T: the GEMM of step T - j (none at j = 0) and the gates of step T - 1 - j (none at j = T)
    for (int j = 0; j <= T; ++j) {
        GbArgs P{};
        P.rt0 = (int)rt0;
        P.rt_total = (int)(rt0 + rt1);
        P.unit_tiles = ut;
        P.H = H;
        for (int s = 0; s < nseg; ++s) {
            const cn_gru_seq_bwd &q = segs[s];
            const int64_t BH = q.B * H, rt = s ? rt1 : rt0;
            const int tk = T - j, tg = T - 1 - j;
            const bool gates = tg >= 0;
            GbSeg g{q.B,
                    j ? q.g + tk * 4 * BH : nullptr,
                    q.w_hh_t,
                    q.acc,
                    (gates && tg + 1 < T) ? q.m + (tg + 1) * q.B : nullptr,
                    (gates && q.dout) ? q.dout + tg * BH : nullptr,
                    gates ? q.save + tg * 4 * BH : nullptr,
                    gates ? q.hm + tg * BH : nullptr,
                    gates ? q.g + tg * 4 * BH : nullptr,
                    gates ? part[s] + tg * rt * 4 * H : nullptr};
            (s ? P.s1 : P.s0) = g;
        }
        if (nseg == 1) P.s1 = P.s0;
        (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
        if (bm == SK_BM)
            hipLaunchKernelGGL(cn_gru_bwd_sk_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, P);
        else
            hipLaunchKernelGGL(cn_gru_bwd_fused_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, P);
        if (const int rc = launch_status()) return rc;
    }
    // bias gradients: every step's workgroup partials of each GRU, summed in a fixed order
    for (int s = 0; s < nseg; ++s) {
        const int rc = cn_gru_bias_reduce(stream, (int64_t)T * (s ? rt1 : rt0), H, part[s], segs[s].db_ih,
                                          segs[s].db_hh, red);
        if (rc) return rc;
    }
    return CN_OK;
}

int64_t cn_gru_bias_blocks(int64_t B) { return (B + CN_GB_RW - 1) / CN_GB_RW; }

int cn_gru_bwd_step_bias(void *stream, int64_t B, int H, float *acc, const float *m_next, const float *dout,
                         const float *save, const float *hm, float *dgi, float *dgh, float *part)
{
    if (B <= 0 || !(H == 64 || H == 128 || H == 256)) return cn_set_error(CN_EINVAL, "cn_gru_bwd_step_bias: H in {64, 128, 256}");
    if (!acc || !save || !hm || !dgi || !dgh || !part) return cn_set_error(CN_EINVAL, "cn_gru_bwd_step_bias: null operand");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_gru_bwd_bias_kernel<false>, dim3((unsigned)cn_gru_bias_blocks(B)), dim3(256), 0, (hipStream_t)stream,
                       B, H, acc, m_next, dout, save, hm, dgi, dgh, part);
    return launch_status();
}

int cn_gru_bwd_step_gates(void *stream, int64_t B, int H, float *acc, const float *m_next, const float *dout,
                          const float *save, const float *hm, float *g, float *part)
{
    if (B <= 0 || !(H == 64 || H == 128 || H == 256)) return cn_set_error(CN_EINVAL, "cn_gru_bwd_step_gates: H in {64, 128, 256}");
    if (!acc || !save || !hm || !g || !part) return cn_set_error(CN_EINVAL, "cn_gru_bwd_step_gates: null operand");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_gru_bwd_bias_kernel<true>, dim3((unsigned)cn_gru_bias_blocks(B)), dim3(256), 0, (hipStream_t)stream,
                       B, H, acc, m_next, dout, save, hm, g, nullptr, part);
    return launch_status();
}

int64_t cn_gru_bias_work_elems(int H) { return (int64_t)CN_GB_RC * 4 * H; }

int cn_gru_bias_reduce(void *stream, int64_t rows, int H, const float *part, float *db_ih, float *db_hh,
                       float *work)
{
    if (rows <= 0 || H <= 0 || (H & 3)) return cn_set_error(CN_EINVAL, "cn_gru_bias_reduce: bad shape");
    if (!part || !db_ih || !db_hh || !work) return cn_set_error(CN_EINVAL, "cn_gru_bias_reduce: null operand");
    (void)hipGetLastError();
    hipLaunchKernelGGL(cn_gru_bias_part2_kernel, dim3((unsigned)((4 * H + 63) / 64), CN_GB_RC), dim3(256), 0,
                       (hipStream_t)stream, rows, H, part, work);
    hipLaunchKernelGGL(cn_gru_bias_final_kernel, dim3((unsigned)((4 * H + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, H, (const float *)work, db_ih, db_hh);
    return launch_status();
}

int cn_gru_bwd_step(void *stream, int64_t B, int H, float *acc, const float *m_next, const float *dout,
                    const float *save, const float *hm, float *dgi, float *dgh)
{
    if (B <= 0 || H <= 0 || (H & 3)) return cn_set_error(CN_EINVAL, "cn_gru_bwd_step: B > 0 and H % 4 == 0 required");
    if (!acc || !save || !hm || !dgi || !dgh) return cn_set_error(CN_EINVAL, "cn_gru_bwd_step: null operand");
    if (B * (H / 4) > (int64_t)0xffffffff * 256) return cn_set_error(CN_EINVAL, "cn_gru_bwd_step: B too large");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_gru_bwd_kernel, dim3(grid_for(B, H)), dim3(256), 0, (hipStream_t)stream, B, H, acc,
                       m_next, dout, save, hm, dgi, dgh);
    return launch_status();
}

// ---- PPO: GAE, the Gaussian act() tail ----

int cn_gae(void *stream, int T, int64_t E, float gamma, float gamma_lambda, int use_proper_time_limits,
           const float *rewards, const float *values, const float *masks, const float *bad_masks, float *returns)
{
    if (T <= 0 || E <= 0) return cn_set_error(CN_EINVAL, "cn_gae: T > 0 and E > 0 required");
    if (!rewards || !values || !masks || !returns || (use_proper_time_limits && !bad_masks))
        return cn_set_error(CN_EINVAL, "cn_gae: null operand");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_gae_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, E, gamma,
                       gamma_lambda, use_proper_time_limits, rewards, values, masks, bad_masks, returns);
    return launch_status();
}

int cn_gaussian_act(void *stream, int64_t E, int A, const float *mean, const float *logstd, const float *eps,
                    float *action, float *logp)
{
    if (E <= 0 || A <= 0 || A > 64) return cn_set_error(CN_EINVAL, "cn_gaussian_act: E > 0 and 0 < A <= 64 required");
    if (!mean || !logstd || !action || !logp) return cn_set_error(CN_EINVAL, "cn_gaussian_act: null operand");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_gaussian_act_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       E, A, mean, logstd, eps, action, logp);
    return launch_status();
}

// ---- weight gradients ----

int64_t cn_wgrad_work_elems(int64_t K, int m, int n)
{
    if (K <= 0 || m <= 0 || n <= 0) return 0;
    int64_t rows;
    int G;
    wgrad_grid(K, rows, G);
    return (int64_t)G * (m * n + m);
}

int cn_wgrad(void *stream, int64_t K, int m, int n, const float *dy, const float *relu_out, const float *x,
             float *dW, float *db, float *work)
{
    if (K <= 0 || m <= 0 || n <= 0 || m * n + m > CN_WG_MAXSLOT || (m < n ? m : n) > CN_WG_NARROW ||
        (m > n ? m : n) > 256)
        return cn_set_error(CN_EINVAL, "cn_wgrad: need K > 0, min(m, n) <= 8, max(m, n) <= 256");
    if (!dy || !x || !dW || !work) return cn_set_error(CN_EINVAL, "cn_wgrad: null operand");
    int64_t rows;
    int G;
    wgrad_grid(K, rows, G);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    const bool dywide = m >= n;
    const int wide = dywide ? m : n;
    const bool v4 = (wide & 3) == 0 && ((uintptr_t)(dywide ? dy : x) & 15) == 0 &&
                    (!dywide || !relu_out || ((uintptr_t)relu_out & 15) == 0);
    const int TW = v4 ? wide / 4 : wide;
    if (dywide && v4)
        hipLaunchKernelGGL((cn_wgrad_part_kernel<4, true>), dim3(G), dim3(256), 0, (hipStream_t)stream, K, m, n, TW,
                           rows, dy, relu_out, x, work);
    else if (dywide)
        hipLaunchKernelGGL((cn_wgrad_part_kernel<1, true>), dim3(G), dim3(256), 0, (hipStream_t)stream, K, m, n, TW,
                           rows, dy, relu_out, x, work);
    else if (v4)
        hipLaunchKernelGGL((cn_wgrad_part_kernel<4, false>), dim3(G), dim3(256), 0, (hipStream_t)stream, K, m, n, TW,
                           rows, dy, relu_out, x, work);
    else
        hipLaunchKernelGGL((cn_wgrad_part_kernel<1, false>), dim3(G), dim3(256), 0, (hipStream_t)stream, K, m, n, TW,
                           rows, dy, relu_out, x, work);
    hipLaunchKernelGGL(cn_wgrad_sum_kernel, dim3(m * n + m), dim3(256), 0, (hipStream_t)stream, G, m, n,
                       (const float *)work, dW, db);
    return launch_status();
}

// ---- attention pooling ----

int cn_attn_pool_fwd(void *stream, int64_t R, int N, int H, const float *hs, const float *attn, float *out)
{
    if (R <= 0 || N <= 0 || H <= 0 || (H & 3)) return cn_set_error(CN_EINVAL, "cn_attn_pool_fwd: bad shape");
    if (!hs || !attn || !out) return cn_set_error(CN_EINVAL, "cn_attn_pool_fwd: null operand");
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    hipLaunchKernelGGL(cn_attn_pool_fwd_kernel, dim3(grid_for(R, H)), dim3(256), 0, (hipStream_t)stream, R, N, H, hs,
                       attn, out);
    return launch_status();
}

int cn_attn_pool_bwd(void *stream, int64_t R, int N, int H, const float *hs, const float *attn, const float *dout,
                     float *dhs, float *dattn)
{
    if (R <= 0 || N <= 0 || !(H == 256 || H == 128 || H == 64))
        return cn_set_error(CN_EINVAL, "cn_attn_pool_bwd: H must be 64, 128 or 256");
    if (!hs || !attn || !dout || !dhs || !dattn) return cn_set_error(CN_EINVAL, "cn_attn_pool_bwd: null operand");
    const unsigned grid = grid_for(R, H);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    if (H == 256)
        hipLaunchKernelGGL(cn_attn_pool_bwd_kernel<64>, dim3(grid), dim3(256), 0, (hipStream_t)stream, R, N, hs, attn,
                           dout, dhs, dattn);
    else if (H == 128)
        hipLaunchKernelGGL(cn_attn_pool_bwd_kernel<32>, dim3(grid), dim3(256), 0, (hipStream_t)stream, R, N, hs, attn,
                           dout, dhs, dattn);
    else
        hipLaunchKernelGGL(cn_attn_pool_bwd_kernel<16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, R, N, hs, attn,
                           dout, dhs, dattn);
    return launch_status();
}

// ---- spatial attention ----

static int sa_check(const char *who, int64_t R, int N, int H, std::initializer_list<const void *> vec,
                    std::initializer_list<const void *> other)
{
    if (R <= 0 || N <= 0 || N > CN_SA_MAXN || !(H == 256 || H == 128 || H == 64))
        return cn_set_error(CN_EINVAL, who);
    for (const void *p : vec)
        if (!p || ((uintptr_t)p & 15)) return cn_set_error(CN_EINVAL, who);
    for (const void *p : other)
        if (!p) return cn_set_error(CN_EINVAL, who);
    return CN_OK;
}

int cn_spatial_attn_fwd(void *stream, int64_t R, int N, int H, float scale, const float *hs, const float *u,
                        const float *c, float *out, float *attn)
{
    if (sa_check("cn_spatial_attn_fwd: H in {64, 128, 256}, 1 <= N <= 64, non-null operands, hs / u / out "
                 "16-byte aligned", R, N, H, {hs, u, out}, {c, attn}))
        return CN_EINVAL;
    const unsigned grid = grid_for(R, H);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    CN_SA_LAUNCH(cn_spatial_attn_fwd_kernel, H, N, grid, (hipStream_t)stream, R, N, scale, hs, u, c, out, attn);
    return launch_status();
}

int cn_spatial_attn_bwd(void *stream, int64_t R, int N, int H, float scale, const float *hs, const float *u,
                        const float *attn, const float *dout, const float *dattn, float *dhs, float *du, int64_t ldu,
                        float *dc, int64_t ldc)
{
    if (sa_check("cn_spatial_attn_bwd: H in {64, 128, 256}, 1 <= N <= 64, non-null operands, hs / u / dout / "
                 "dhs / du 16-byte aligned, ldu >= H and a multiple of 4, ldc >= 1", R, N, H, {hs, u, dout, dhs, du},
                 {attn, dc}) || ldu < H || (ldu & 3) || ldc < 1)
        return cn_set_error(CN_EINVAL, "cn_spatial_attn_bwd: bad shape, stride or operand");
    const unsigned grid = grid_for(R, H);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    CN_SA_LAUNCH(cn_spatial_attn_bwd_kernel, H, N, grid, (hipStream_t)stream, R, N, scale, hs, u, attn,
                 dout, dattn, dhs, du, ldu, dc, ldc);
    return launch_status();
}

int cn_spatial_attn_var_fwd(void *stream, int64_t R, int N, int H, const int32_t *count, const float *row_scale,
                            const float *hs, const float *u, const float *c, float *out, float *attn)
{
    if (sa_check("cn_spatial_attn_var_fwd: H in {64, 128, 256}, 1 <= N <= 64, non-null operands, hs / u / out "
                 "16-byte aligned", R, N, H, {hs, u, out}, {count, row_scale, c, attn}))
        return CN_EINVAL;
    const unsigned grid = grid_for(R, H);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    CN_SA_LAUNCH(cn_spatial_attn_var_fwd_kernel, H, N, grid, (hipStream_t)stream, R, N, count, row_scale,
                 hs, u, c, out, attn);
    return launch_status();
}

int cn_spatial_attn_var_bwd(void *stream, int64_t R, int N, int H, const int32_t *count, const float *row_scale,
                            const float *hs, const float *u, const float *attn, const float *dout, const float *dattn,
                            float *dhs, float *du, int64_t ldu, float *dc, int64_t ldc)
{
    if (sa_check("cn_spatial_attn_var_bwd: H in {64, 128, 256}, 1 <= N <= 64, non-null operands, hs / u / dout / "
                 "dhs / du 16-byte aligned, ldu >= H and a multiple of 4, ldc >= 1", R, N, H, {hs, u, dout, dhs, du},
                 {count, row_scale, attn, dc}) || ldu < H || (ldu & 3) || ldc < 1)
        return cn_set_error(CN_EINVAL, "cn_spatial_attn_var_bwd: bad shape, stride or operand");
    const unsigned grid = grid_for(R, H);
    (void)hipGetLastError();   // a stale error of an earlier call (any library) is not this launch's
    CN_SA_LAUNCH(cn_spatial_attn_var_bwd_kernel, H, N, grid, (hipStream_t)stream, R, N, count, row_scale,
                 hs, u, attn, dout, dattn, dhs, du, ldu, dc, ldc);
    return launch_status();
}

}  // extern "C"
