// The mixed 4 + 3 Winograd tiling of a 7 x 7 map: its geometry, the pair-image store and the input tile transform B^T d B.
// Shared by winograd.hip (wino7_input_pair_kernel: d from global memory) and roi_align.hip (the fused ROIAlign -> Winograd
// forward: d from its LDS patch), whose images must agree bit for bit.  No contraction pragma here: the transform uses explicit
// fmaf, and the one product a compiler may fuse (w7_store_pair) is exact, so both includers get the same bits.
#pragma once
#include "common.h"
#include "wino43_mats.h"

struct W7 {
    static constexpr int NP[2] = {6, 5};      // positions per axis
    static constexpr int OUT[2] = {4, 3};     // outputs per axis
    static constexpr int IN0[2] = {-1, 3};    // first input row / column of the tile's patch
    static constexpr int OUT0[2] = {0, 4};    // first output row / column
    static constexpr int QOFF[4] = {0, 36, 66, 96};   // first position of tile type ka * 2 + kb (121 in total)
};

// A tile type as a compile-time pair, and the ONE dispatch from a runtime tile type t = ka * 2 + kb (QOFF's index: a grid index,
// a wave index) to it: f(W7Type<KA, KB>{}) with f a generic always-inline lambda, so that each call site inlines four bodies.
template <int KA_, int KB_> struct W7Type { static constexpr int KA = KA_, KB = KB_; };
template <typename F> __device__ __forceinline__ void w7_for_tile(int t, F&& f) {
    switch (t) {
        case 0: f(W7Type<0, 0>{}); break;
        case 1: f(W7Type<0, 1>{}); break;
        case 2: f(W7Type<1, 0>{}); break;
        default: f(W7Type<1, 1>{}); break;
    }
}
// all four tile types, in position order
template <typename F> __device__ __forceinline__ void w7_for_all_tiles(F&& f) {
    f(W7Type<0, 0>{});
    f(W7Type<0, 1>{});
    f(W7Type<1, 0>{});
    f(W7Type<1, 1>{});
}

__device__ __forceinline__ void fma4(float4& a, float s, float4 v) {
    a.x = fmaf(s, v.x, a.x); a.y = fmaf(s, v.y, a.y); a.z = fmaf(s, v.z, a.z); a.w = fmaf(s, v.w, a.w);
}

// ---- pair-image output (f16x2p GEMM engine, gemm_pair.hip) ------------------------------------------------------------
// A lane holds 4 consecutive channels c .. c+3 (c = 4 x its index along C), its neighbour (lane ^ 1) the other half of the
// 8-channel chunk [h: 8 x f16 | l: 8 x f16].  The even lane hands its two l words to the odd lane and receives the odd lane's
// two h words (one quad_perm DPP move each way), so both store 16 contiguous bytes - the even lane the h half, the odd lane
// the l half - at the byte offset the fp32 float4 would have gone to: pair images keep the fp32 tensor's addressing.
// Callers keep lanes along C, four channels per lane (threadIdx.x & 1 pairs adjacent lanes).
// s is a power of two (cim::pair_scale_of), so v * s is exact: fused into pair_split2's subtraction or not, the bits are the same.
typedef unsigned w7_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned w7_swap1(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
}
__device__ __forceinline__ void w7_store_pair(float* p, const float4& v, float s) {
    unsigned h0, l0, h1, l1;
    cim::pair_split2(v.x * s, v.y * s, h0, l0);
    cim::pair_split2(v.z * s, v.w * s, h1, l1);
    const bool odd = (threadIdx.x & 1) != 0;
    const unsigned r0 = w7_swap1(odd ? h0 : l0), r1 = w7_swap1(odd ? h1 : l1);
    const w7_u4 o = odd ? w7_u4{r0, r1, l0, l1} : w7_u4{h0, h1, r0, r1};
    __builtin_nontemporal_store(o, reinterpret_cast<w7_u4*>(p));
}

// One input tile of type (KA, KB) for the lane's 4 channels: d[i][j] = fetch(iy, ix) inside the 7 x 7 map, 0 outside ->
// B^T d B -> pair image positions Q0 .. Q0 + NA NB of V (position stride MC floats) at element offset `off`; scale [121].
template <int KA, int KB, typename Fetch>
__device__ __forceinline__ void w7_input_tile_regs(Fetch fetch, float* __restrict__ V, size_t MC, size_t off,
                                                   const float* __restrict__ scale) {
    constexpr int NA = W7::NP[KA], NB = W7::NP[KB], P = 7, Q0 = W7::QOFF[KA * 2 + KB];
    float4 d[NA][NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int iy = W7::IN0[KA] + i;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int ix = W7::IN0[KB] + j;
            if ((unsigned)iy < (unsigned)P && (unsigned)ix < (unsigned)P) d[i][j] = fetch(iy, ix);
            else d[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        float4 trow[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            trow[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < NA; ++k)
                if (W7_BT[KA][i][k] != 0.0f) fma4(trow[j], W7_BT[KA][i][k], d[k][j]);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < NB; ++k)
                if (W7_BT[KB][j][k] != 0.0f) fma4(v, W7_BT[KB][j][k], trow[k]);
            w7_store_pair(V + (size_t)(Q0 + i * NB + j) * MC + off, v, scale[Q0 + i * NB + j]);
        }
    }
}
