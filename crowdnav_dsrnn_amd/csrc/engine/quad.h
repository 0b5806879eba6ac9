// quad.h -- DPP helpers over the 4 lanes of a quad: exchange (quad_xor*), min / max / OR, and the broadcast of
// one lane's value to the quad (qbc*). Needs nothing.
#pragma once

__device__ __forceinline__ float quad_xor1(float x)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, false));  // quad_perm 1,0,3,2
}
__device__ __forceinline__ float quad_xor2(float x)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xF, 0xF, false));  // quad_perm 2,3,0,1
}
__device__ __forceinline__ int quad_xor1i(int x) { return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false); }
__device__ __forceinline__ int quad_xor2i(int x) { return __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, false); }
__device__ __forceinline__ float quad_min(float x)
{
    float y = quad_xor1(x); x = y < x ? y : x;
    y = quad_xor2(x); return y < x ? y : x;
}
__device__ __forceinline__ float quad_max(float x)
{
    float y = quad_xor1(x); x = x < y ? y : x;
    y = quad_xor2(x); return x < y ? y : x;
}
__device__ __forceinline__ int quad_or(int x)
{
    x |= quad_xor1i(x);
    return x | quad_xor2i(x);
}

// 64-bit quad OR (MT = uint64_t masks: simulators of more than 32 agents, cn_orca_predict_kd only)
__device__ __forceinline__ uint32_t quad_or_m(uint32_t x) { return (uint32_t)quad_or((int)x); }
__device__ __forceinline__ uint64_t quad_or_m(uint64_t x)
{
    return (uint64_t)(uint32_t)quad_or((int)(uint32_t)x) | ((uint64_t)(uint32_t)quad_or((int)(uint32_t)(x >> 32)) << 32);
}

template <int T>
__device__ __forceinline__ float qbc(float x)   // quad_perm(T, T, T, T): lane T of the quad to all four
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), T * 0x55, 0xF, 0xF, false));
}
__device__ __forceinline__ float4 qbc4(const float4 v, int t)   // t folds to a constant once unrolled
{
    switch (t & 3) {
    case 0: return make_float4(qbc<0>(v.x), qbc<0>(v.y), qbc<0>(v.z), qbc<0>(v.w));
    case 1: return make_float4(qbc<1>(v.x), qbc<1>(v.y), qbc<1>(v.z), qbc<1>(v.w));
    case 2: return make_float4(qbc<2>(v.x), qbc<2>(v.y), qbc<2>(v.z), qbc<2>(v.w));
    default: return make_float4(qbc<3>(v.x), qbc<3>(v.y), qbc<3>(v.z), qbc<3>(v.w));
    }
}
__device__ __forceinline__ float qbcf(const float v, int t)
{
    switch (t & 3) {
    case 0: return qbc<0>(v);
    case 1: return qbc<1>(v);
    case 2: return qbc<2>(v);
    default: return qbc<3>(v);
    }
}
