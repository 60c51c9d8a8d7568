// The integer / compare-only wave and workgroup helpers that the exactness contracts rest on (stable
// descending order, first-index arg-max), one definition each for mining.hip, detect.hip, losses.hip and the evaluators
// (eval_match.h).  Nothing here adds floats, so no summation order depends on this file; the float and double sums stay with
// the kernels whose contracts fix their order.  Included once per translation unit; everything has internal linkage.
#pragma once
#include "common.h"

namespace {

// A float as an unsigned key in IEEE order for every non-NaN value, -0 == +0 (NumPy's comparison sorts)
__device__ __forceinline__ uint32_t orderable(float f) {
    if (f == 0.0f) f = 0.0f;  // -0 == +0 for the comparison sort
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float orderable_inverse(uint32_t o) {         // (of -0: +0)
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

template <typename T>
__device__ T block_exclusive_scan(T v, T* part, T* total) {                      // 1024 lanes; returns the exclusive prefix
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;       // wave scans in registers, 16 wave totals through LDS:
    T incl = v;                                                          // two barriers instead of the 20 of an all-LDS scan
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    __syncthreads();                                                     // (part[] of the previous scan has been read)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    T woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const T p = part[w];
        tot += p;
        woff += (w < wave) ? p : 0;
    }
    *total = tot;
    return woff + incl - v;
}

// First-index arg-max: the greater value wins, an equal value takes the lower index (the first maximum; NaN never wins)
__device__ __forceinline__ bool argmax_takes(float ov, int oi, float v, int i) { return ov > v || (ov == v && oi < i); }

// (value, index) max over the 64 lanes
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (argmax_takes(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// ... with 32 bits that travel with the winner
__device__ __forceinline__ void wave_argmax(float& v, int& i, int& payload) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        const int op = __shfl_xor(payload, o);
        if (argmax_takes(ov, oi, v, i)) { v = ov; i = oi; payload = op; }
    }
}

}  // namespace
