// The ONE copy of what the fused optimizer kernels share (sgd.hip, adam.hip; grad_clip.hip takes the load helper and the grid
// rule): the walk over the two device tables - `chunks` (cim_sgd_chunk) and one record per tensor - with its flat chunks and
// its matrix-mode tiles, the 16-byte streaming accesses and the max |w_new| by-product (IEEE bit patterns; per row through a
// wave-wide maximum, per column in registers).  An optimizer is a RULE:
//     struct Rule {
//         static constexpr int NS;                     // state arrays per tensor (SGD 1, Adam 2)
//         using record = ...;                          // the tensor record: p, g, n, rows, cols, row_amax, col_amax + its own
//         using consts = ...;                          // what the launch takes once for all tensors
//         static uint64_t state(const record&, int k); // where the record keeps state array k
//         Rule(const consts&, const record&);          // reads the per-tensor constants
//         void operator()(float& p, float g, float (&s)[NS]) const;   // updates ONE element
//     };
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/cim_hip.h"

namespace {

#ifndef CIM_SGD_NT
#define CIM_SGD_NT 1            // 1 = nontemporal stores of the updated parameter / state (matrix mode)
#endif
typedef float stream_v4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 stream_load(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void stream_store(float* p, const float4& v) {
#if CIM_SGD_NT
    __builtin_nontemporal_store(stream_v4{v.x, v.y, v.z, v.w}, reinterpret_cast<stream_v4*>(p));
#else
    *reinterpret_cast<float4*>(p) = v;
#endif
}

// wave-wide maximum on the VALU (as amax_wave of experiments/csrc/gemm_engines.hip): valid in lane 63
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true));
    return v;
}

// max_workgroups of the C entry points: 0 = one workgroup per chunk, else at most that many, each walking chunks b, b + grid, ...
inline int optim_grid(int n_chunks, int max_workgroups) {
    return max_workgroups > 0 && max_workgroups < n_chunks ? max_workgroups : n_chunks;
}

// the rule on 4 consecutive elements: the float4 form and the scalar tail run the same operator()
template <class Rule>
__device__ __forceinline__ void update4(const Rule& rule, float4& pv, const float4& gv, float4 (&sv)[Rule::NS]) {
#define CIM_OPTIM_LANE(e)                                        \
    {                                                            \
        float s[Rule::NS];                                       \
        _Pragma("unroll") for (int k = 0; k < Rule::NS; ++k) s[k] = sv[k].e; \
        rule(pv.e, gv.e, s);                                     \
        _Pragma("unroll") for (int k = 0; k < Rule::NS; ++k) sv[k].e = s[k]; \
    }
    CIM_OPTIM_LANE(x) CIM_OPTIM_LANE(y) CIM_OPTIM_LANE(z) CIM_OPTIM_LANE(w)
#undef CIM_OPTIM_LANE
}

// R rows of a matrix-mode tile: all (2 + NS) R loads of a lane are issued before the first update.  m[i] = max |p_new| of the
// lane's 4 columns of row i, cm = running column maxima.  (No __restrict__ on these parameters - the walker's own pointers
// carry it: with it here the compiler drops the nontemporal hint from the single-row form's store of p.)
template <class Rule, int R>
__device__ __forceinline__ void tile_rows(const Rule& rule, float* p, const float* g,
                                          float* const (&s)[Rule::NS], size_t ld, uint4& cm, unsigned (&m)[R]) {
    float4 pv[R], gv[R], sv[R][Rule::NS];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        pv[i] = stream_load(p + i * ld);
        gv[i] = stream_load(g + i * ld);
#pragma unroll
        for (int k = 0; k < Rule::NS; ++k) sv[i][k] = stream_load(s[k] + i * ld);
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        update4(rule, pv[i], gv[i], sv[i]);
#pragma unroll
        for (int k = 0; k < Rule::NS; ++k) stream_store(s[k] + i * ld, sv[i][k]);
        stream_store(p + i * ld, pv[i]);
        const unsigned ax = __float_as_uint(pv[i].x) & 0x7fffffffu, ay = __float_as_uint(pv[i].y) & 0x7fffffffu;
        const unsigned az = __float_as_uint(pv[i].z) & 0x7fffffffu, aw = __float_as_uint(pv[i].w) & 0x7fffffffu;
        cm.x = max(cm.x, ax); cm.y = max(cm.y, ay); cm.z = max(cm.z, az); cm.w = max(cm.w, aw);
        m[i] = max(max(ax, ay), max(az, aw));
    }
}

// tile_rows for the lanes inside the matrix, then the R row maxima of the wave into row_amax[0..R)
template <class Rule, int R>
__device__ __forceinline__ void tile_step(const Rule& rule, float* p, const float* g,
                                          float* const (&s)[Rule::NS], size_t ld, bool cin, bool lead, unsigned* row_amax, uint4& cm) {
    unsigned m[R] = {};
    if (cin) tile_rows<Rule, R>(rule, p, g, s, ld, cm, m);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const unsigned mm = wave_max_u32(m[i]);
        if (lead) atomicMax(row_amax + i, mm);
    }
}

// A launch of fewer workgroups than chunks WALKS over them (workgroup b takes chunks b, b + grid, ...): max_workgroups of the
// entry points - an update that runs beside another stream's latency-bound launches (FusedOptimizer.overlap_update: under the
// next step's backbone forward) then holds ONE or TWO of a CU's workgroup slots instead of all of them, and those launches'
// workgroups are placed at once instead of queueing behind 15 k chunk workgroups.  256 lanes per workgroup.
template <class Rule>
__device__ __forceinline__ void walk_chunks(const typename Rule::record* __restrict__ tensors, const cim_sgd_chunk* __restrict__ chunks,
                                            int n_chunks, const typename Rule::consts& k) {
  constexpr int NS = Rule::NS;
  for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    const cim_sgd_chunk ch = chunks[ci];
    const typename Rule::record t = tensors[ch.tensor];
    const Rule rule(k, t);
    const bool matrix = t.cols > 0;
    // matrix mode ([rows][cols] weights of the MaskFuse contractions): a 64-row x 1024-column tile per workgroup, a lane owns 4
    // consecutive columns - the update of the flat mode plus the per-row / per-column max |w_new| the f16x2 GEMM engine needs
    // as operand scales (saves its pass over the 822 MB fc1 weight).  ch.offset = first row, ch.n = first column.
    const int r0 = (int)ch.offset, r1 = min((int)t.rows, r0 + 64);
    const int c = ch.n + threadIdx.x * 4;
    const bool cin = c < t.cols;
    const size_t ld = (size_t)t.cols;
    const size_t base = matrix ? (size_t)r0 * ld + (cin ? c : 0) : (size_t)ch.offset;
    float* __restrict__ p = reinterpret_cast<float*>(t.p) + base;
    const float* __restrict__ g = reinterpret_cast<const float*>(t.g) + base;
    float* s[NS];
    uint64_t all = t.p | t.g;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        s[j] = reinterpret_cast<float*>(Rule::state(t, j)) + base;
        all |= Rule::state(t, j);
    }
    if (matrix) {
        unsigned* row_amax = reinterpret_cast<unsigned*>(t.row_amax);
        unsigned* col_amax = reinterpret_cast<unsigned*>(t.col_amax);
        const bool lead = (threadIdx.x & 63) == 63;
        uint4 cm = make_uint4(0, 0, 0, 0);
        int r = r0;
        for (; r + 4 <= r1; r += 4) {                    // 4 rows = 4 (2 + NS) x 16 B loads in flight per lane
            tile_step<Rule, 4>(rule, p, g, s, ld, cin, lead, row_amax + r, cm);
            p += 4 * ld; g += 4 * ld;
#pragma unroll
            for (int j = 0; j < NS; ++j) s[j] += 4 * ld;
        }
        for (; r < r1; ++r) {
            tile_step<Rule, 1>(rule, p, g, s, ld, cin, lead, row_amax + r, cm);
            p += ld; g += ld;
#pragma unroll
            for (int j = 0; j < NS; ++j) s[j] += ld;
        }
        if (cin) {
            atomicMax(col_amax + c, cm.x); atomicMax(col_amax + c + 1, cm.y);
            atomicMax(col_amax + c + 2, cm.z); atomicMax(col_amax + c + 3, cm.w);
        }
        continue;
    }
    const int n = min(ch.n, (int)(t.n - ch.offset));
    // 16-byte accesses need every chunk base aligned (chunk offsets are multiples of 4 elements); plain stores: flat tensors are small
    const int n4 = (all & 15) == 0 ? (n & ~3) : 0;
    for (int i = threadIdx.x * 4; i < n4; i += 256 * 4) {
        float4 pv = stream_load(p + i), sv[NS];
        const float4 gv = stream_load(g + i);
#pragma unroll
        for (int j = 0; j < NS; ++j) sv[j] = stream_load(s[j] + i);
        update4(rule, pv, gv, sv);
#pragma unroll
        for (int j = 0; j < NS; ++j) *reinterpret_cast<float4*>(s[j] + i) = sv[j];
        *reinterpret_cast<float4*>(p + i) = pv;
    }
    for (int i = n4 + threadIdx.x; i < n; i += 256) {      // unaligned tensors / tails
        float pv = p[i], sv[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) sv[j] = s[j][i];
        rule(pv, g[i], sv);
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j][i] = sv[j];
        p[i] = pv;
    }
  }
}

}  // namespace
