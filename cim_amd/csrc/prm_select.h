// The exact lower median of a map, shared by prm.hip (maps in memory) and prm_train.hip (maps in LDS): integer work only.
#pragma once
#include "common.h"

namespace cim {

constexpr int PRM_THREADS = 256;

// Order-preserving 32-bit keys: ascending key order is ascending float order with -0.0 below +0.0 (integer work only).
__device__ __forceinline__ unsigned prm_key(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned prm_unkey(unsigned k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

// The element of rank (n - 1) / 2 of the n bit patterns at `bits` (global memory or LDS), most significant byte first: four
// histogram passes of one PRM_THREADS workgroup.  hist [256] and sel [2] are LDS; *s_nan (LDS, zeroed by the caller before its
// last barrier) is set when a value is a NaN.  Every thread returns the same bit pattern; ends behind a barrier.
__device__ __forceinline__ unsigned prm_lower_median_bits(const unsigned* __restrict__ bits, int n, int* hist, int* sel, int* s_nan) {
    const int tid = threadIdx.x;
    unsigned prefix = 0u, mask = 0u;
    int k = (n - 1) >> 1;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        bool nan = false;
        for (int i = tid; i < n; i += PRM_THREADS) {
            const unsigned u = bits[i];
            nan = nan || (u & 0x7fffffffu) > 0x7f800000u;
            const unsigned key = prm_key(u);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        if (shift == 24 && nan) *s_nan = 1;
        __syncthreads();
        if (tid == 0) {
            int c = 0, b = 0;
            for (; b < 255; ++b) {
                const int hb = hist[b];
                if (k < c + hb) break;
                c += hb;
            }
            sel[0] = b;
            sel[1] = k - c;
        }
        __syncthreads();
        prefix |= (unsigned)sel[0] << shift;
        mask |= 255u << shift;
        k = sel[1];
    }
    return prm_unkey(prefix);
}

// ConstantPad2d(1, -inf) around a map
__device__ __forceinline__ float prm_at(const float* __restrict__ map, int H, int W, int y, int x) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? map[y * W + x] : -INFINITY;
}

// max_pool2d keeps the FIRST maximum of the 3 x 3 window (val > max): earlier neighbours strictly less, later ones <=
__device__ __forceinline__ bool prm_is_peak(const float* __restrict__ map, int H, int W, int y, int x, float v, float med) {
    return v >= med && prm_at(map, H, W, y - 1, x - 1) < v && prm_at(map, H, W, y - 1, x) < v && prm_at(map, H, W, y - 1, x + 1) < v &&
           prm_at(map, H, W, y, x - 1) < v && prm_at(map, H, W, y, x + 1) <= v && prm_at(map, H, W, y + 1, x - 1) <= v &&
           prm_at(map, H, W, y + 1, x) <= v && prm_at(map, H, W, y + 1, x + 1) <= v;
}

}  // namespace cim
