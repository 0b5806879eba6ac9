// cn_host.h -- host-side helpers of the policy units (cn_gru.hip, cn_attn_mask.hip, cn_lattice.hip): the error
// channel of cn_engine.hip, the checks and launch grids their extern "C" functions share. No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

#include "../../include/crowdnav.h"

int cn_set_error(int code, const char *msg);   // cn_engine.hip: records cn_last_error()'s text, returns code

namespace {

// one thread per (row, 4 consecutive hidden units), 256-thread workgroups
inline unsigned grid_for(int64_t B, int H) { return (unsigned)((B * (H / 4) + 255) / 256); }

inline bool aligned16(std::initializer_list<const void *> ps)
{
    for (const void *p : ps)
        if ((uintptr_t)p & 15) return false;
    return true;
}

// the end of a function that launched: the launches' status as the function's return code. (Before its first launch
// the function drops a stale error of an earlier call, of any library, with `(void)hipGetLastError()`.)
inline int launch_status()
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CN_OK : cn_set_error(CN_EHIP, hipGetErrorString(e));
}

// The (H, N) ladder of the spatial-attention kernel templates <HQ, NR>: HQ = H / 4 lanes per row for H in
// {256, 128, 64}; a row's first NR vectors stay in registers, NR = 10 for N <= 10 and 16 otherwise. KERNEL is the
// template's name, the arguments after `stream` are the kernel's.
#define CN_SA_LAUNCH1(KERNEL, HQ, NR, grid, stream, ...) \
    hipLaunchKernelGGL((KERNEL<HQ, NR>), dim3(grid), dim3(256), 0, stream, __VA_ARGS__)
#define CN_SA_LAUNCH(KERNEL, H, N, grid, stream, ...)                                       \
    do {                                                                                    \
        if ((N) <= 10) {                                                                    \
            if ((H) == 256) CN_SA_LAUNCH1(KERNEL, 64, 10, grid, stream, __VA_ARGS__);       \
            else if ((H) == 128) CN_SA_LAUNCH1(KERNEL, 32, 10, grid, stream, __VA_ARGS__);  \
            else CN_SA_LAUNCH1(KERNEL, 16, 10, grid, stream, __VA_ARGS__);                  \
        } else {                                                                            \
            if ((H) == 256) CN_SA_LAUNCH1(KERNEL, 64, 16, grid, stream, __VA_ARGS__);       \
            else if ((H) == 128) CN_SA_LAUNCH1(KERNEL, 32, 16, grid, stream, __VA_ARGS__);  \
            else CN_SA_LAUNCH1(KERNEL, 16, 16, grid, stream, __VA_ARGS__);                  \
        }                                                                                   \
    } while (0)

}  // namespace
