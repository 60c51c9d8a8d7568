// What the fused optimizer kernels (sgd.hip, adam.hip) share: the 16-byte streaming accesses of their matrix mode and the
// max |w_new| by-product (IEEE bit patterns; per row through a wave-wide maximum, per column in registers).
#pragma once
#include <hip/hip_runtime.h>

namespace {

#ifndef CIM_SGD_NT
#define CIM_SGD_NT 1            // 1 = nontemporal stores of the updated parameter / history (matrix mode)
#endif
typedef float sgd_v4 __attribute__((ext_vector_type(4)));
#ifndef CIM_SGD_NTL
#define CIM_SGD_NTL 0           // 1 = nontemporal loads too: measured slower (0.919 vs 0.864 ms at cfg2)
#endif
__device__ __forceinline__ float4 sgd_load(const float* p) {
#if CIM_SGD_NTL
    const sgd_v4 v = __builtin_nontemporal_load(reinterpret_cast<const sgd_v4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *reinterpret_cast<const float4*>(p);
#endif
}
__device__ __forceinline__ void sgd_store(float* p, const float4& v) {
#if CIM_SGD_NT
    __builtin_nontemporal_store(sgd_v4{v.x, v.y, v.z, v.w}, reinterpret_cast<sgd_v4*>(p));
#else
    *reinterpret_cast<float4*>(p) = v;
#endif
}

// wave-wide maximum on the VALU (see amax_wave in gemm_f32.hip): valid in lane 63
__device__ __forceinline__ unsigned sgd_wave_max(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true));
    return v;
}

}  // namespace
