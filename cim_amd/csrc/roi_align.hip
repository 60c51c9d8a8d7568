// ROIAlign forward / backward for gfx950, channels-last, optionally fused with the
// MaskFuse prologue (mask multiply + channel concat).
//
// Replaces mmcv.ops.RoIAlign as used at /root/reference/lib/modeling/model_builder.py:229-231
// and the elementwise prologue of MaskFuse.forward (/root/reference/lib/modeling/resnet50.py:131-134).
// Arithmetic follows SURVEY.md App. D; the forward is evaluated with FP contraction off and
// in the reference's sample order so it is bit-identical to oracle/roi_align_ref.c.
//
// Layout: feat [B,H,W,C], out [K,P,P,C] (or cat [K,P,P,2C]).  A workgroup owns one
// (roi, bin-row); its lanes run along C, so every global access is a contiguous
// 16 B/lane x 64-lane (1 KiB per wave) segment of one feature pixel's channel vector.
#include <cstdlib>
#include "common.h"
#include "wino7_tile.h"
#include "../../include/cim_hip.h"

namespace {

struct RoiGeom {
    float x1, y1, bw, bh, count;
    int gw, gh, b;
};

#pragma clang fp contract(off)
__device__ __forceinline__ RoiGeom roi_geom(const float* __restrict__ roi, float scale, int P, int sampling_ratio,
                                            int aligned) {
    RoiGeom g;
    const float off = aligned ? 0.5f : 0.0f;
    g.b = (int)roi[0];
    g.x1 = roi[1] * scale - off;
    g.y1 = roi[2] * scale - off;
    const float x2 = roi[3] * scale - off;
    const float y2 = roi[4] * scale - off;
    float rw = x2 - g.x1, rh = y2 - g.y1;
    if (!aligned) {
        rw = fmaxf(rw, 1.0f);
        rh = fmaxf(rh, 1.0f);
    }
    g.bh = rh / (float)P;
    g.bw = rw / (float)P;
    g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)P);
    g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)P);
    const int c = g.gh * g.gw;
    g.count = (float)(c > 1 ? c : 1);
    return g;
}

struct Tap {  // one axis of a bilinear sample
    int lo, hi;
    float l, h;
    bool valid;
};

__device__ __forceinline__ Tap make_tap(float v, int size) {
    Tap t;
    t.valid = !(v < -1.0f || v > (float)size);
    if (v <= 0.0f) v = 0.0f;
    t.lo = (int)v;
    if (t.lo >= size - 1) {
        t.hi = t.lo = size - 1;
        v = (float)t.lo;
    } else {
        t.hi = t.lo + 1;
    }
    t.l = v - (float)t.lo;
    t.h = 1.0f - t.l;
    return t;
}

template <int VEC> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<4> { using type = float4; };

__device__ __forceinline__ float vmul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 vmul(float a, float4 b) { return make_float4(a * b.x, a * b.y, a * b.z, a * b.w); }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float vdiv(float a, float b) { return a / b; }
__device__ __forceinline__ float4 vdiv(float4 a, float b) { return make_float4(a.x / b, a.y / b, a.z / b, a.w / b); }
__device__ __forceinline__ void vzero(float& a) { a = 0.0f; }
__device__ __forceinline__ void vzero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }

// The in-range samples of output bin (ph, pw), in the oracle's order: f(ty, tx) per sample (an out-of-range one contributes 0).
template <typename F>
__device__ __forceinline__ void for_each_sample(const RoiGeom& g, int ph, int pw, int H, int W, F f) {
    for (int iy = 0; iy < g.gh; ++iy) {
        const float y = g.y1 + ph * g.bh + (iy + 0.5f) * g.bh / (float)g.gh;
        const Tap ty = make_tap(y, H);
        for (int ix = 0; ix < g.gw; ++ix) {
            const float x = g.x1 + pw * g.bw + (ix + 0.5f) * g.bw / (float)g.gw;
            const Tap tx = make_tap(x, W);
            if (ty.valid && tx.valid) f(ty, tx);
        }
    }
}

// One output bin in the oracle's sample and operation order (FP contraction off: bit-identical to oracle/roi_align_ref.c) for the
// VEC channels at fc = feature map of the ROI's image + channel.
template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type sample_bin(const float* __restrict__ fc, const RoiGeom& g, int ph, int pw, int C,
                                                               int H, int W) {
    using V = typename VecT<VEC>::type;
    V acc;
    vzero(acc);
    for_each_sample(g, ph, pw, H, W, [&](const Tap& ty, const Tap& tx) {
        const V v1 = *reinterpret_cast<const V*>(fc + ((size_t)ty.lo * W + tx.lo) * C);
        const V v2 = *reinterpret_cast<const V*>(fc + ((size_t)ty.lo * W + tx.hi) * C);
        const V v3 = *reinterpret_cast<const V*>(fc + ((size_t)ty.hi * W + tx.lo) * C);
        const V v4 = *reinterpret_cast<const V*>(fc + ((size_t)ty.hi * W + tx.hi) * C);
        const float w1 = ty.h * tx.h, w2 = ty.h * tx.l, w3 = ty.l * tx.h, w4 = ty.l * tx.l;
        acc = vadd(acc, vadd(vadd(vadd(vmul(w1, v1), vmul(w2, v2)), vmul(w3, v3)), vmul(w4, v4)));
    });
    return vdiv(acc, g.count);
}

// grid = (K, P); block = 256 lanes along C.
template <int VEC, bool MASKCAT>
__global__ __launch_bounds__(256) void roi_align_fwd_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ rois,
                                                            const float* __restrict__ masks,
                                                            float* __restrict__ out, int C, int H, int W, int P,
                                                            float scale, int sampling_ratio, int aligned) {
    using V = typename VecT<VEC>::type;
    const int k = blockIdx.x, ph = blockIdx.y;
    const RoiGeom g = roi_geom(rois + 5 * (size_t)k, scale, P, sampling_ratio, aligned);
    const float* __restrict__ fb = feat + (size_t)g.b * H * W * C;
    const int OC = MASKCAT ? 2 * C : C;
    for (int c = threadIdx.x * VEC; c < C; c += blockDim.x * VEC) {
        for (int pw = 0; pw < P; ++pw) {
            const V o = sample_bin<VEC>(fb + c, g, ph, pw, C, H, W);
            float* dst = out + (((size_t)k * P + ph) * P + pw) * OC + c;
            *reinterpret_cast<V*>(dst) = o;
            if (MASKCAT) {
                const float m = masks[((size_t)k * P + ph) * P + pw];
                *reinterpret_cast<V*>(dst + C) = vmul(m, o);
            }
        }
    }
}

__device__ __forceinline__ void atomic_add_vec(float* p, float v) { atomicAdd(p, v); }
__device__ __forceinline__ void atomic_add_vec(float* p, float4 v) {
    atomicAdd(p + 0, v.x);
    atomicAdd(p + 1, v.y);
    atomicAdd(p + 2, v.z);
    atomicAdd(p + 3, v.w);
}

// Backward: scatter g*w/count to the 4 neighbours of every in-range sample
// (roi_align_kernel.cu:237-266 of the in-tree variant; mmcv does the same).
template <int VEC, bool MASKCAT>
__global__ __launch_bounds__(256) void roi_align_bwd_kernel(const float* __restrict__ grad_out,
                                                            const float* __restrict__ rois,
                                                            const float* __restrict__ masks,
                                                            float* __restrict__ grad_in, int C, int H, int W, int P,
                                                            float scale, int sampling_ratio, int aligned) {
    using V = typename VecT<VEC>::type;
    const int k = blockIdx.x, ph = blockIdx.y;
    const RoiGeom g = roi_geom(rois + 5 * (size_t)k, scale, P, sampling_ratio, aligned);
    float* __restrict__ gb = grad_in + (size_t)g.b * H * W * C;
    const int OC = MASKCAT ? 2 * C : C;
    for (int c = threadIdx.x * VEC; c < C; c += blockDim.x * VEC) {
        for (int pw = 0; pw < P; ++pw) {
            const float* src = grad_out + (((size_t)k * P + ph) * P + pw) * OC + c;
            V go = *reinterpret_cast<const V*>(src);
            if (MASKCAT) {
                const float m = masks[((size_t)k * P + ph) * P + pw];
                go = vadd(go, vmul(m, *reinterpret_cast<const V*>(src + C)));
            }
            for_each_sample(g, ph, pw, H, W, [&](const Tap& ty, const Tap& tx) {
                const float w1 = ty.h * tx.h, w2 = ty.h * tx.l, w3 = ty.l * tx.h, w4 = ty.l * tx.l;
                atomic_add_vec(gb + ((size_t)ty.lo * W + tx.lo) * C + c, vdiv(vmul(w1, go), g.count));
                atomic_add_vec(gb + ((size_t)ty.lo * W + tx.hi) * C + c, vdiv(vmul(w2, go), g.count));
                atomic_add_vec(gb + ((size_t)ty.hi * W + tx.lo) * C + c, vdiv(vmul(w3, go), g.count));
                atomic_add_vec(gb + ((size_t)ty.hi * W + tx.hi) * C + c, vdiv(vmul(w4, go), g.count));
            });
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Per-ROI tables (shared by the table-driven forward and the region backward).
//
// ROIAlign is linear and separable: with per-ROI weight tables
//   WY[ph][y] = sum over the bin-row's y-samples of the bilinear weight that sample puts on row y
//   WX[pw][x] = likewise for columns
// (a sample is dropped when either coordinate is out of range, which factorises too),
//   out[ph,pw,c] = (1/count) sum_y sum_x WY[ph][y] WX[pw][x] feat[y,x,c]
//   grad_in[y,x,c] += (1/count) * sum_ph WY[ph][y] * sum_pw WX[pw][x] * g[ph,pw,c].
// (Rounds 1-3 carried five more backward kernels built on them - an LDS-resident whole-map tile, a 16-channel pixel-owner form,
// a 3 x 4 pixel-block gather, and a producer / consumer variant of the region form - and two more forwards; all measured slower
// than the kernels below and removed in round 4: DESIGN.md section 4.2 keeps their numbers.)

// conservative [lo, hi] range of bins whose samples can touch position `pos` along one axis
__device__ __forceinline__ void bin_range(float start, float bin, int P, int pos, int& lo, int& hi) {
    if (bin > 0.0f) {
        const float inv = 1.0f / bin;
        lo = (int)floorf(((float)pos - 1.0f - start) * inv) - 1;
        hi = (int)floorf(((float)pos + 1.0f - start) * inv) + 1;
        lo = max(lo, 0);
        hi = min(hi, P - 1);
    } else {  // degenerate ROI: every bin sits at `start`
        lo = 0;
        hi = P - 1;
    }
}

// Per-ROI record written once per launch by roi_tables_kernel (when the caller provides a workspace):
//   wy [P][H] | wx [P][W] | yr [H] | xr [W] | ylo yhi xlo xhi | count | batch      (4-byte words)
// yr / xr: packed range of bins with a non-zero weight on that row / column: lo | hi << 8 | none << 16.
__host__ __device__ __forceinline__ int roi_rec_words(int P, int H, int W) { return ((P + 1) * (H + W) + 6 + 3) & ~3; }

// What the table-driven forwards read of ROI k's record.
struct RoiRec {
    const float* wy;      // [P][H]
    const float* wx;      // [P][W]
    const float* fb;      // feature map of the ROI's image
    int ylo, yhi, xlo, xhi, ncols;
    float inv_count;
};
__device__ __forceinline__ RoiRec roi_rec(const float* __restrict__ rec_all, const float* __restrict__ feat, int k, int C, int H,
                                          int W, int P) {
    RoiRec r;
    r.wy = rec_all + (size_t)k * roi_rec_words(P, H, W);
    r.wx = r.wy + P * H;
    const int* box = reinterpret_cast<const int*>(r.wy + (P + 1) * (H + W));
    r.ylo = box[0]; r.yhi = box[1]; r.xlo = box[2]; r.xhi = box[3];
    r.ncols = max(r.xhi - r.xlo + 1, 0);
    r.inv_count = 1.0f / reinterpret_cast<const float*>(box)[4];
    r.fb = feat + (size_t)box[5] * H * W * C;
    return r;
}

// The record is assembled in LDS (tables, packed ranges, bounding box through LDS atomics) and written to global memory
// once, as one contiguous run: the first version went through global memory between its three phases (three dependent
// round trips per workgroup: 16.7 us for 1000 ROIs; now ~5).  Dynamic LDS: roi_rec_words(P, H, W) words.
__global__ __launch_bounds__(256) void roi_tables_kernel(const float* __restrict__ rois, float* __restrict__ rec_all, int K,
                                                         int P, int H, int W, float scale, int sampling_ratio, int aligned) {
    extern __shared__ __attribute__((aligned(16))) float tsm[];
    const int k = blockIdx.x, tid = threadIdx.x;
    const RoiGeom g = roi_geom(rois + 5 * (size_t)k, scale, P, sampling_ratio, aligned);
    const int words = roi_rec_words(P, H, W);
    float* wy = tsm;
    float* wx = wy + P * H;
    int* yr = reinterpret_cast<int*>(wx + P * W);
    int* xr = yr + H;
    int* box = xr + W;
    if (tid < 4) box[tid] = (tid == 0) ? H : (tid == 2) ? W : -1;      // ylo yhi xlo xhi
    for (int e = tid; e < P * (H + W); e += 256) {
        const bool isy = e < P * H;
        const int e2 = isy ? e : e - P * H;
        const int size = isy ? H : W;
        const int pb = e2 / size, pos = e2 % size;
        const int gn = isy ? g.gh : g.gw;
        const float start = isy ? g.y1 : g.x1, bin = isy ? g.bh : g.bw;
        float acc = 0.0f;
        for (int is = 0; is < gn; ++is) {
            const float v = start + pb * bin + (is + 0.5f) * bin / (float)gn;
            const Tap t = make_tap(v, size);
            if (!t.valid) continue;
            if (t.lo == pos) acc += t.h;
            if (t.hi == pos) acc += t.l;
        }
        (isy ? wy : wx)[e2] = acc;
    }
    __syncthreads();
    for (int e = tid; e < H + W; e += 256) {
        const bool isy = e < H;
        const int pos = isy ? e : e - H, size = isy ? H : W;
        const float* tabp = isy ? wy : wx;
        int lo = P, hi = -1;
        for (int pb = 0; pb < P; ++pb)
            if (tabp[pb * size + pos] != 0.0f) { lo = min(lo, pb); hi = pb; }
        (isy ? yr : xr)[pos] = (hi < 0) ? 0x10000 : (lo | (hi << 8));
        if (hi >= 0) {
            atomicMin(&box[isy ? 0 : 2], pos);
            atomicMax(&box[isy ? 1 : 3], pos);
        }
    }
    if (tid == 0) {
        reinterpret_cast<float*>(box)[4] = g.count;
        box[5] = g.b;
    }
    __syncthreads();
    float* rec = rec_all + (size_t)k * words;
    for (int e = tid; e < (P + 1) * (H + W) + 6; e += 256) rec[e] = tsm[e];
}

// ---------------------------------------------------------------------------------------------
// Forward, aggregated-weight form (default when the caller provides the table workspace).
//
// out[ph,pw,c] = (1/count) sum_y sum_x WY[ph][y] WX[pw][x] feat[y,x,c]   with the per-ROI tables of
// roi_tables_kernel (the same ones the backward uses).  A bin touches (rows of bin ph) x (columns of bin pw)
// pixels ONCE each - (gh+1)(gw+1) 16 B loads per lane instead of the 4*gh*gw of the sample-by-sample kernels
// (2.5-3x fewer at the benchmark's ROI sizes: the tap kernels move 16x the algorithmic bytes through L1).
// The sum is reassociated, so the result differs from the oracle's sample order by a few ulp (tests state
// 1e-6 relative); the sample-order kernels above stay behind cim_roi_align_fwd / CIM_ROI_FWD_EXACT=1.
// The weight tables are built with FP contraction off (same values as the backward's).
// A workgroup owns one (roi, bin row): it flattens the bin row's (pixel offset, weight) pairs into LDS once,
// then every lane runs a flat, 4-way unrolled loop over them for its 4 channels.
typedef float ga_f2 __attribute__((ext_vector_type(2)));       // v_pk_fma_f32: two fp32 FMAs per instruction
__device__ __forceinline__ ga_f2 ga_lo(const float4& v) { return ga_f2{v.x, v.y}; }
__device__ __forceinline__ ga_f2 ga_hi(const float4& v) { return ga_f2{v.z, v.w}; }
__device__ __forceinline__ ga_f2 ga_fma(float w, ga_f2 v, ga_f2 a) { return __builtin_elementwise_fma(ga_f2{w, w}, v, a); }
constexpr int FW_MAXP = 8;      // bins per axis the table-driven forwards take
constexpr int AG_MAXE = 64;     // entries per (ph, pw) list kept in LDS; larger bins take the sample-order kernel

template <bool MASKCAT>
__global__ __launch_bounds__(256) void roi_align_fwd_agg_kernel(const float* __restrict__ feat,
                                                                const float* __restrict__ masks,
                                                                float* __restrict__ out, int C, int H, int W, int P,
                                                                const float* __restrict__ rec_all,
                                                                const float* __restrict__ rois, float scale,
                                                                int sampling_ratio, int aligned) {
    __shared__ int2 ent[FW_MAXP * AG_MAXE];      // {element offset of the pixel, weight bits}
    __shared__ int s_over;
    __shared__ int s_n[FW_MAXP], s_xlo[FW_MAXP], s_nx[FW_MAXP];
    __shared__ int s_rows[64];                   // rows with a non-zero weight in this bin row
    __shared__ int s_nrows;
    const int k = blockIdx.x, ph = blockIdx.y, tid = threadIdx.x, NTH = blockDim.x;
    const RoiRec R = roi_rec(rec_all, feat, k, C, H, W, P);
    const float* wy = R.wy + ph * H;
    const float* wx = R.wx;
    const int ylo = R.ylo, yhi = R.yhi, xlo = R.xlo, xhi = R.xhi;
    const float inv_count = R.inv_count;
    const float* __restrict__ fb = R.fb;
    if (tid == 0) {
        int n = 0;      // every row with a non-zero weight counts: more than s_rows holds takes the sample-order path below
        for (int y = ylo; y <= yhi; ++y)
            if (wy[y] != 0.0f) {
                if (n < 64) s_rows[n] = y;
                ++n;
            }
        s_nrows = n;
        s_over = n > 64;
    } else if (tid >= 64 && tid < 64 + P) {
        const int pw = tid - 64;
        int lo = xhi + 1, hi = xlo - 1;
        for (int x = xlo; x <= xhi; ++x)
            if (wx[pw * W + x] != 0.0f) { lo = min(lo, x); hi = x; }
        s_xlo[pw] = lo;
        s_nx[pw] = max(hi - lo + 1, 0);
    }
    __syncthreads();
    const int nrows = s_nrows;
    if (tid < P && nrows * s_nx[tid] > AG_MAXE) s_over = 1;      // benign race: every writer stores 1
    __syncthreads();
    const int OC = MASKCAT ? 2 * C : C;
    if (s_over) {      // block-uniform: a bin larger than the LDS list (ROI far larger than the map) -> sample by sample
        const RoiGeom g = roi_geom(rois + 5 * (size_t)k, scale, P, sampling_ratio, aligned);
        for (int c = tid * 4; c < C; c += NTH * 4) {
            for (int pw = 0; pw < P; ++pw) {
                const float4 o = sample_bin<4>(fb + c, g, ph, pw, C, H, W);
                float* dst = out + (((size_t)k * P + ph) * P + pw) * OC + c;
                *reinterpret_cast<float4*>(dst) = o;
                if (MASKCAT) *reinterpret_cast<float4*>(dst + C) = vmul(masks[((size_t)k * P + ph) * P + pw], o);
            }
        }
        return;
    }
    for (int e = tid; e < P * AG_MAXE; e += NTH) {
        const int pw = e / AG_MAXE, i = e % AG_MAXE;
        const int nx = s_nx[pw];
        const int n = nrows * nx;
        if (i == 0) s_n[pw] = n;
        if (i < n) {
            const int r = i / nx, x = s_xlo[pw] + (i - r * nx), y = s_rows[r];
            ent[e] = make_int2((y * W + x) * C, __float_as_int(wy[y] * inv_count * wx[pw * W + x]));
        }
    }
    __syncthreads();
    for (int c = tid * 4; c < C; c += NTH * 4) {
        const float* __restrict__ fc = fb + c;
        for (int pw = 0; pw < P; ++pw) {
            const int2* el = ent + pw * AG_MAXE;
            const int n = s_n[pw];
            ga_f2 al = {0.f, 0.f}, ah = {0.f, 0.f};
            int i = 0;
            for (; i + 8 <= n; i += 8) {      // 8 loads in flight per lane, then the 4 and 1 tails
                int2 e[8];
                float4 v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) e[j] = el[i + j];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float4*>(fc + e[j].x);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float w = __int_as_float(e[j].y);
                    al = ga_fma(w, ga_lo(v[j]), al);
                    ah = ga_fma(w, ga_hi(v[j]), ah);
                }
            }
            for (; i + 4 <= n; i += 4) {
                const int2 e0 = el[i], e1 = el[i + 1], e2 = el[i + 2], e3 = el[i + 3];
                const float4 v0 = *reinterpret_cast<const float4*>(fc + e0.x);
                const float4 v1 = *reinterpret_cast<const float4*>(fc + e1.x);
                const float4 v2 = *reinterpret_cast<const float4*>(fc + e2.x);
                const float4 v3 = *reinterpret_cast<const float4*>(fc + e3.x);
                const float w0 = __int_as_float(e0.y), w1 = __int_as_float(e1.y), w2 = __int_as_float(e2.y), w3 = __int_as_float(e3.y);
                al = ga_fma(w0, ga_lo(v0), al); ah = ga_fma(w0, ga_hi(v0), ah);
                al = ga_fma(w1, ga_lo(v1), al); ah = ga_fma(w1, ga_hi(v1), ah);
                al = ga_fma(w2, ga_lo(v2), al); ah = ga_fma(w2, ga_hi(v2), ah);
                al = ga_fma(w3, ga_lo(v3), al); ah = ga_fma(w3, ga_hi(v3), ah);
            }
            for (; i < n; ++i) {
                const int2 e0 = el[i];
                const float4 v0 = *reinterpret_cast<const float4*>(fc + e0.x);
                const float w0 = __int_as_float(e0.y);
                al = ga_fma(w0, ga_lo(v0), al); ah = ga_fma(w0, ga_hi(v0), ah);
            }
            const float4 acc = make_float4(al.x, al.y, ah.x, ah.y);
            float* dst = out + (((size_t)k * P + ph) * P + pw) * OC + c;
            typedef float ga_f4 __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(ga_f4{acc.x, acc.y, acc.z, acc.w}, reinterpret_cast<ga_f4*>(dst));
            if (MASKCAT) {
                const float4 mo = vmul(masks[((size_t)k * P + ph) * P + pw], acc);
                __builtin_nontemporal_store(ga_f4{mo.x, mo.y, mo.z, mo.w}, reinterpret_cast<ga_f4*>(dst + C));
            }
        }
    }
}

constexpr int RS_MAXD = 128;     // rows / columns of the map (round 6: was 64 - the reference's largest training scale gives 57 x 75 maps)

// The row-sum core, shared by roi_align_fwd_rowsum2_kernel and the fused roi_align_wino7_pair_kernel: the two write the same bits
// because they run these functions.
// s_wx[xi][pw] = WX[pw][xlo + xi], zero for pw >= P: the column weights of one column as one padded row (whole workgroup).
__device__ __forceinline__ void rs_fill_wx(float (*s_wx)[8], const RoiRec& R, int P, int W, int tid, int nth) {
    for (int e = tid; e < R.ncols * 8; e += nth) {
        const int xi = e >> 3, pw = e & 7;
        s_wx[xi][pw] = pw < P ? R.wx[pw * W + R.xlo + xi] : 0.0f;
    }
}

// The rows of the map with a non-zero weight in bin row ph0 or ph0 + 1, ascending, with their weights / count: a wave-wide
// compaction, run by ONE whole wave (an ROI spans up to RS_MAXD = 128 rows: two passes of the wave).  Returns their number.
__device__ __forceinline__ int rs_row_list(const RoiRec& R, int ph0, bool two, int H, int W, int lane, int* rows, float* wa,
                                           float* wb) {
    const float* wy0 = R.wy + ph0 * H;
    const float* wy1 = wy0 + H;
    int nrows = 0;
    for (int y0 = R.ylo; y0 <= R.yhi; y0 += 64) {
        const int y = y0 + lane;
        float a = 0.0f, b = 0.0f;
        if (y <= R.yhi) { a = wy0[y]; b = two ? wy1[y] : 0.0f; }
        const bool on = y <= R.yhi && (a != 0.0f || b != 0.0f);
        const unsigned long long m = __ballot(on);
        if (on) {
            const int n = nrows + __popcll(m & ((1ull << lane) - 1ull));
            rows[n] = y * W; wa[n] = a * R.inv_count; wb[n] = b * R.inv_count;
        }
        nrows += __popcll(m);
    }
    return nrows;
}

// The column walk for the lane's 4 channels at fc: a (bin row ph0) and b (ph0 + 1), low and high channel pair of the 7 bins.
__device__ __forceinline__ void rs_column_walk(const int* __restrict__ rows, const float* __restrict__ rwa,
                                               const float* __restrict__ rwb, int nrows, int ncols, int xlo, int C,
                                               const float* __restrict__ fc, const float (*s_wx)[8], ga_f2 (&al)[7], ga_f2 (&ah)[7],
                                               ga_f2 (&bl)[7], ga_f2 (&bh)[7]) {
#pragma unroll
    for (int pw = 0; pw < 7; ++pw) al[pw] = ah[pw] = bl[pw] = bh[pw] = ga_f2{0.f, 0.f};
    for (int xi = 0; xi < ncols; xi += 2) {
        const bool pair = xi + 1 < ncols;            // wave-uniform; the odd last column is loaded twice, weight 0
        const int x0 = (xlo + xi) * C, dx1 = pair ? C : 0;
        ga_f2 ta0l = {0.f, 0.f}, ta0h = {0.f, 0.f}, ta1l = {0.f, 0.f}, ta1h = {0.f, 0.f};
        ga_f2 tb0l = {0.f, 0.f}, tb0h = {0.f, 0.f}, tb1l = {0.f, 0.f}, tb1h = {0.f, 0.f};
        int r = 0;
        for (; r + 4 <= nrows; r += 4) {
            float4 v0[4], v1[4];
            float wa[4], wb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* src = fc + (size_t)rows[r + j] * C + x0;
                v0[j] = *reinterpret_cast<const float4*>(src);
                v1[j] = *reinterpret_cast<const float4*>(src + dx1);
                wa[j] = rwa[r + j];
                wb[j] = rwb[r + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ta0l = ga_fma(wa[j], ga_lo(v0[j]), ta0l); ta0h = ga_fma(wa[j], ga_hi(v0[j]), ta0h);
                ta1l = ga_fma(wa[j], ga_lo(v1[j]), ta1l); ta1h = ga_fma(wa[j], ga_hi(v1[j]), ta1h);
                tb0l = ga_fma(wb[j], ga_lo(v0[j]), tb0l); tb0h = ga_fma(wb[j], ga_hi(v0[j]), tb0h);
                tb1l = ga_fma(wb[j], ga_lo(v1[j]), tb1l); tb1h = ga_fma(wb[j], ga_hi(v1[j]), tb1h);
            }
        }
        for (; r < nrows; ++r) {
            const float* src = fc + (size_t)rows[r] * C + x0;
            const float4 v0 = *reinterpret_cast<const float4*>(src);
            const float4 v1 = *reinterpret_cast<const float4*>(src + dx1);
            const float wa = rwa[r], wb = rwb[r];
            ta0l = ga_fma(wa, ga_lo(v0), ta0l); ta0h = ga_fma(wa, ga_hi(v0), ta0h);
            ta1l = ga_fma(wa, ga_lo(v1), ta1l); ta1h = ga_fma(wa, ga_hi(v1), ta1h);
            tb0l = ga_fma(wb, ga_lo(v0), tb0l); tb0h = ga_fma(wb, ga_hi(v0), tb0h);
            tb1l = ga_fma(wb, ga_lo(v1), tb1l); tb1h = ga_fma(wb, ga_hi(v1), tb1h);
        }
        const int xj = pair ? xi + 1 : xi;
        const float4 wa0 = *reinterpret_cast<const float4*>(&s_wx[xi][0]), wb0 = *reinterpret_cast<const float4*>(&s_wx[xi][4]);
        const float4 wa1 = *reinterpret_cast<const float4*>(&s_wx[xj][0]), wb1 = *reinterpret_cast<const float4*>(&s_wx[xj][4]);
        const float m1 = pair ? 1.0f : 0.0f;
        const float w0[7] = {wa0.x, wa0.y, wa0.z, wa0.w, wb0.x, wb0.y, wb0.z};
        const float w1[7] = {m1 * wa1.x, m1 * wa1.y, m1 * wa1.z, m1 * wa1.w, m1 * wb1.x, m1 * wb1.y, m1 * wb1.z};
#pragma unroll
        for (int pw = 0; pw < 7; ++pw) {
            al[pw] = ga_fma(w0[pw], ta0l, al[pw]); ah[pw] = ga_fma(w0[pw], ta0h, ah[pw]);
            al[pw] = ga_fma(w1[pw], ta1l, al[pw]); ah[pw] = ga_fma(w1[pw], ta1h, ah[pw]);
            bl[pw] = ga_fma(w0[pw], tb0l, bl[pw]); bh[pw] = ga_fma(w0[pw], tb0h, bh[pw]);
            bl[pw] = ga_fma(w1[pw], tb1l, bl[pw]); bh[pw] = ga_fma(w1[pw], tb1h, bh[pw]);
        }
    }
}

// Forward, row-sum form of the same separable sum (default when P <= 7 and the map is at most 128 x 128):
//   out[ph,pw,c] = sum_x WX[pw][x] * ( sum_y WY[ph][y] / count * feat[y,x,c] ).
// A workgroup still owns one (roi, bin row), but walks the COLUMNS of the ROI once: the inner sum t(x) over the bin row's
// rows is formed once per column and fed to every bin whose WX[pw][x] is non-zero, so the pixels that neighbouring bins
// share (one or two columns per bin boundary) are loaded once - rows x (columns of the ROI) loads instead of
// rows x (sum of the bins' column counts), ~23 % fewer at the benchmark's ROI sizes.  Two columns are in flight per
// iteration (up to 8 loads per lane).  The 7 column weights of a column sit in LDS as one padded row (zero outside the
// bin's range), so the bin update is 7 unconditional packed FMAs.
// Round 4, measured and dropped: workgroup = one ROI x one 256-channel slice (four waves = the four bin-row pairs) with the slices
// pinned to XCDs, so that an XCD's L2 only sees its 1.45 MB of the 5.8 MB map (the calibrated FETCH_SIZE of this launch is 232 MB
// for that map: 38x).  0.152 vs 0.140 ms at cfg2, 0.287 vs 0.279 at 2000 ROIs (tools/bench_roi.py, same box): the re-fetches are
// served by the Infinity Cache and were not what bounds the kernel - the L1 -> L2 request rate is (section 4.2 of DESIGN.md).
// Two bin rows per workgroup: the rows of the map that bin rows ph and ph + 1 share (one or two of ~3.6)
// are loaded once as well; grid = (K, ceil(P / 2)).
template <bool MASKCAT>
__global__ __launch_bounds__(256) void roi_align_fwd_rowsum2_kernel(const float* __restrict__ feat,
                                                                    const float* __restrict__ masks,
                                                                    float* __restrict__ out, int C, int H, int W, int P,
                                                                    const float* __restrict__ rec_all) {
    __shared__ __attribute__((aligned(16))) float s_wx[RS_MAXD][8];
    __shared__ float s_wa[RS_MAXD], s_wb[RS_MAXD];
    __shared__ int s_rows[RS_MAXD];
    __shared__ int s_nrows;
    const int k = blockIdx.x, ph0 = blockIdx.y * 2, tid = threadIdx.x, NTH = blockDim.x;
    const bool two = ph0 + 1 < P;
    const RoiRec R = roi_rec(rec_all, feat, k, C, H, W, P);
    if (tid < 64) {      // wave 0
        const int n = rs_row_list(R, ph0, two, H, W, tid, s_rows, s_wa, s_wb);
        if (tid == 0) s_nrows = n;
    }
    rs_fill_wx(s_wx, R, P, W, tid, NTH);
    __syncthreads();
    const int nrows = s_nrows;
    const int OC = MASKCAT ? 2 * C : C;
    for (int c = tid * 4; c < C; c += NTH * 4) {
        ga_f2 al[7], ah[7], bl[7], bh[7];
        rs_column_walk(s_rows, s_wa, s_wb, nrows, R.ncols, R.xlo, C, R.fb + c, s_wx, al, ah, bl, bh);
        typedef float ga_f4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int pw = 0; pw < 7; ++pw) {
            if (pw >= P) break;
            float* dst = out + (((size_t)k * P + ph0) * P + pw) * OC + c;
            __builtin_nontemporal_store(ga_f4{al[pw].x, al[pw].y, ah[pw].x, ah[pw].y}, reinterpret_cast<ga_f4*>(dst));
            if (MASKCAT) {
                const float m = masks[((size_t)k * P + ph0) * P + pw];
                __builtin_nontemporal_store(ga_f4{m * al[pw].x, m * al[pw].y, m * ah[pw].x, m * ah[pw].y}, reinterpret_cast<ga_f4*>(dst + C));
            }
            if (two) {
                float* dst2 = dst + (size_t)P * OC;
                __builtin_nontemporal_store(ga_f4{bl[pw].x, bl[pw].y, bh[pw].x, bh[pw].y}, reinterpret_cast<ga_f4*>(dst2));
                if (MASKCAT) {
                    const float m = masks[((size_t)k * P + ph0 + 1) * P + pw];
                    __builtin_nontemporal_store(ga_f4{m * bl[pw].x, m * bl[pw].y, m * bh[pw].x, m * bh[pw].y}, reinterpret_cast<ga_f4*>(dst2 + C));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Forward, fused with the MaskFuse prologue AND the Winograd input transform of MaskFuse's convolution (round 5):
//   feat --ROIAlign--> box [7][7][C] --(box, box * mask)--> cat [7][7][2C] --B^T d B per tile--> V' [121][Rs][2C] pair image
// for /root/reference/lib/modeling/resnet50.py:121-135 (roi_xform -> mask multiply -> concat -> mask_branch's 3 x 3 convolution in
// the mixed 4 + 3 Winograd tiling of csrc/winograd.hip).  `cat` never exists: the two-kernel path wrote its 401 MB (cfg2), read
// them back in wino7_input_pair_kernel (0.288 ms) and wrote the 991 MB image; here the image is the only output.
// Workgroup = (ROI r, 256-channel slice), four waves.  Phase A: wave w computes the bin rows 2w, 2w + 1 of the ROI for the lane's
// 4 channels with the row-sum core of roi_align_fwd_rowsum2_kernel (the same functions: the values are the bits that kernel
// writes) into an LDS patch [49][256].  Phase B: wave t transforms tile type t (36 / 30 / 30 / 25 positions)
// of the patch - once as it is, once multiplied by the ROI's 7 x 7 mask - with w7_input_tile_regs of wino7_tile.h, the
// transform and split (h, l) fp16 store of wino7_input_pair_kernel (lane pairs exchange halves, 16 bytes per lane).  Rows r >= K (the pad up
// to a multiple of 32 rows the GEMM wants) are zero-filled.  The image is bit-identical to the two-kernel path's.
__global__ __launch_bounds__(256) void roi_align_wino7_pair_kernel(const float* __restrict__ feat, const float* __restrict__ masks,
                                                                   float* __restrict__ V, int C, int H, int W, int K, int Rs,
                                                                   const float* __restrict__ rec_all,
                                                                   const float* __restrict__ scale) {
    constexpr int P = 7;
    __shared__ __attribute__((aligned(16))) float4 s_patch[49 * 64];                    // [bin][lane]: 49 KB
    __shared__ __attribute__((aligned(16))) float s_wx[RS_MAXD][8];
    __shared__ float s_wa[4][RS_MAXD], s_wb[4][RS_MAXD];
    __shared__ int s_rows[4][RS_MAXD];
    __shared__ float s_mask[49];
    const int r = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = slice * 256 + lane * 4;
    const size_t C2 = 2 * (size_t)C, MC = (size_t)Rs * C2;
    if (r >= K) {                                                                        // pad rows: zero
        if (c < C)
            for (int q = wave; q < 121; q += 4) {
                float* dst = V + (size_t)q * MC + (size_t)r * C2 + c;
                __builtin_nontemporal_store(w7_u4{0, 0, 0, 0}, reinterpret_cast<w7_u4*>(dst));
                __builtin_nontemporal_store(w7_u4{0, 0, 0, 0}, reinterpret_cast<w7_u4*>(dst + C));
            }
        return;
    }
    const int k = r;
    const RoiRec R = roi_rec(rec_all, feat, k, C, H, W, P);
    // ---- phase A: bin rows ph0, ph0 + 1 of this wave (the row-sum core: rowsum2's bits)
    const int ph0 = wave * 2;
    const bool two = ph0 + 1 < P;
    const int nrows = rs_row_list(R, ph0, two, H, W, lane, s_rows[wave], s_wa[wave], s_wb[wave]);
    rs_fill_wx(s_wx, R, P, W, tid, 256);
    if (tid < 49) s_mask[tid] = masks[(size_t)k * 49 + tid];
    __syncthreads();
    if (c < C) {
        ga_f2 al[7], ah[7], bl[7], bh[7];
        rs_column_walk(s_rows[wave], s_wa[wave], s_wb[wave], nrows, R.ncols, R.xlo, C, R.fb + c, s_wx, al, ah, bl, bh);
#pragma unroll
        for (int pw = 0; pw < 7; ++pw) {
            s_patch[(ph0 * P + pw) * 64 + lane] = make_float4(al[pw].x, al[pw].y, ah[pw].x, ah[pw].y);
            if (two) s_patch[((ph0 + 1) * P + pw) * 64 + lane] = make_float4(bl[pw].x, bl[pw].y, bh[pw].x, bh[pw].y);
        }
    }
    __syncthreads();
    // ---- phase B: tile type `wave` of the patch -> pair image, both halves of the channel concat
    if (c >= C) return;
    const size_t off = (size_t)r * C2 + c;
    const auto plain = [&](int iy, int ix) { return s_patch[(iy * P + ix) * 64 + lane]; };
    const auto masked = [&](int iy, int ix) { return vmul(s_mask[iy * P + ix], s_patch[(iy * P + ix) * 64 + lane]); };
    switch (wave) {
        case 0: w7_input_tile_regs<0, 0>(plain, V, MC, off, scale); w7_input_tile_regs<0, 0>(masked, V, MC, off + C, scale); break;
        case 1: w7_input_tile_regs<0, 1>(plain, V, MC, off, scale); w7_input_tile_regs<0, 1>(masked, V, MC, off + C, scale); break;
        case 2: w7_input_tile_regs<1, 0>(plain, V, MC, off, scale); w7_input_tile_regs<1, 0>(masked, V, MC, off + C, scale); break;
        default: w7_input_tile_regs<1, 1>(plain, V, MC, off, scale); w7_input_tile_regs<1, 1>(masked, V, MC, off + C, scale); break;
    }
}

// ---------------------------------------------------------------------------------------------
// Backward, region form (default).
//
// What bounds the gather kernel is that every gradient vector is re-read by each of the ~3.7 pixel blocks its bin
// touches, from workgroups on different XCDs: 1.5 GB through the fabric for 401 MB of gradients.  Here a workgroup of
// 16 waves owns a REGION of 12 x 16 feature pixels (4 x 4 sub-blocks of 3 x 4, one per wave, 12 float4 accumulators per
// lane) x a 256-channel slice (lanes along C, 16 B per lane) for one group of ROIs.  The gradient slices of the bins that
// touch the region are brought in ONCE per workgroup - all 1024 lanes stream a window of 32 entries (64 KB with the
// mask-cat halves, combined on the way: g_lo + m g_hi) into LDS, double buffered, the next window's loads in flight
// while the waves consume the current one - and every wave reads from LDS the entries whose bin touches its sub-block
// (a ballot over the window's row / column masks picks them).  Re-read factor of a 12 x 16 region at the benchmark's bin
// size (3.6 x 4.1 px): (15.6 / 12)(20.1 / 16) = 1.6 instead of 3.7; registers per lane as in the 3 x 4 gather.
// Entry record in LDS: gradient offset, mask, separable weights wy[4 sub-rows][4] (3 used) and wx[4 sub-columns][4], touch mask.
// Regions are dispatched centre first (they carry the most entries); groups meet in grad_in through atomicAdd.
// ROIs per workgroup (template parameter GS): rg_group_size() below (32: 0.66, 96: 0.26, 160: 0.38, 256: 0.56 ms at 1000 ROIs).
// Entry order inside a group: interleaved over the ROIs (see the entry map below); sub-blocks spread over the SIMDs.
constexpr int RG_SBH = 3, RG_SBW = 4, RG_WR = 4, RG_WC = 4;
constexpr int RG_RH = RG_SBH * RG_WR, RG_RW = RG_SBW * RG_WC;          // 12 x 16 pixels
constexpr int RG_NT = 64 * RG_WR * RG_WC;                               // 1024 threads
constexpr int RG_WIN = 32;                                              // entries per staging window
constexpr int RG_MAXE = 256;                                            // entries per super-window (records in LDS)
// ROIs per workgroup: 64, or 128 when 64 would make more than ~3.5 workgroups per CU (measured, ms at 64 / 128:
// 1000 ROIs on 33 x 43: 0.188 / 0.284, 800 on 27 x 36: 0.159 / 0.253, 1200 on 41 x 54: 0.288 / 0.261, 2000 on 33 x 43: 0.353 / 0.321)
static inline int rg_group_size(int K, int B, int C, int H, int W) {
    const long long wgs = (long long)B * ((K + 63) / 64) * ((H + 11) / 12) * ((W + 15) / 16) * ((C + 255) / 256);
    return wgs > 900 ? 128 : 64;
}
constexpr int RG_REC = 36;                                              // words per entry record: off, m, touch, pad, wy[16], wx[16]
constexpr int RG_MAXREG = 256;
struct RegionOrder { unsigned char o[RG_MAXREG]; };
static inline size_t rg_lds_bytes(int GS, int P) {     // staging windows + entry records + entry map
    return sizeof(float) * (2 * RG_WIN * 256 + RG_MAXE * RG_REC) + sizeof(unsigned short) * ((size_t)GS * P * P + 8);
}

template <bool MASKCAT, int RG_GS>
__global__ __launch_bounds__(RG_NT) void roi_align_bwd_region_kernel(const float* __restrict__ grad_out,
                                                                     const float* __restrict__ masks,
                                                                     float* __restrict__ grad_in, int C, int H, int W, int K,
                                                                     int P, int B, int use_atomic,
                                                                     const float* __restrict__ rec_all,
                                                                     const RegionOrder region_order, int n_regions,
                                                                     int regions_x, int n_slices, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float rg_smem[];
    float (*stage)[RG_WIN][256] = reinterpret_cast<float (*)[RG_WIN][256]>(rg_smem);   // [2][32][256]: 64 KB
    float* erec = rg_smem + 2 * RG_WIN * 256;                                         // [MAXE][REC]: 36 KB
    unsigned short* emap = reinterpret_cast<unsigned short*>(erec + RG_MAXE * RG_REC);   // [GS * P * P]: entry -> ROI | ph << 7 | pw << 11
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // work order: region (centre first) slowest, then ROI group, then channel slice
    int lin = blockIdx.x;
    const int slice = lin % n_slices;
    lin /= n_slices;
    const int groups_total = gridDim.x / (n_slices * n_regions);                      // B * groups
    const int by = lin % groups_total;
    const int region = region_order.o[lin / groups_total];
    const int b = by % B, kgroup = by / B;
    const int y0 = (region / regions_x) * RG_RH, x0 = (region % regions_x) * RG_RW;
    // wave w runs on SIMD w % 4: the sub-blocks of one SIMD are spread out (row t, column (s + 2 t) % 4: every 2 x 2
    // neighbourhood of sub-blocks sits on four different SIMDs) - a bin hits ADJACENT sub-blocks together
    const int wr = wave / RG_WC, wc = (wave + 2 * wr) % RG_WC;
    const int sy0 = y0 + wr * RG_SBH, sx0 = x0 + wc * RG_SBW;
    const int recw = roi_rec_words(P, H, W);
    const int OC = MASKCAT ? 2 * C : C, PP = P * P;

    ga_f2 accl[12], acch[12];
#pragma unroll
    for (int p = 0; p < 12; ++p) accl[p] = acch[p] = ga_f2{0.f, 0.f};

    // ---- inspection: thread t < GS looks at ROI kgroup * GS + t and leaves a descriptor in LDS
    __shared__ int d_base[RG_GS + 1];          // first entry index of the ROI (exclusive prefix sum), [GS] = total
    __shared__ int d_bins[RG_GS];              // phl | pwl << 8 | npw << 16
    __shared__ float d_inv[RG_GS];             // 1 / count
    __shared__ int d_cnt[RG_GS];               // entries of the ROI
    {
        const int k = kgroup * RG_GS + tid;
        int phl = 0, phh = -1, pwl = 0, pwh = -1;
        float inv_count = 0.0f;
        if (tid < RG_GS && k < K) {
            const float* rec = rec_all + (size_t)k * recw;
            const int* yr = reinterpret_cast<const int*>(rec + P * (H + W));
            const int* xr = yr + H;
            if (yr[H + W + 5] == b) {
                int lo = P, hi = -1;
#pragma unroll
                for (int i = 0; i < RG_RH; ++i) {
                    const int r = yr[min(y0 + i, H - 1)];
                    if (y0 + i < H && !(r & 0x10000)) { lo = min(lo, r & 0xff); hi = max(hi, (r >> 8) & 0xff); }
                }
                phl = lo; phh = hi;
                lo = P; hi = -1;
#pragma unroll
                for (int j = 0; j < RG_RW; ++j) {
                    const int r = xr[min(x0 + j, W - 1)];
                    if (x0 + j < W && !(r & 0x10000)) { lo = min(lo, r & 0xff); hi = max(hi, (r >> 8) & 0xff); }
                }
                pwl = lo; pwh = hi;
                inv_count = 1.0f / reinterpret_cast<const float*>(yr)[H + W + 4];
            }
        }
        const int nph = max(phh - phl + 1, 0), npw = max(pwh - pwl + 1, 0);
        const int n_mine = (nph > 0 && npw > 0) ? nph * npw : 0;
        int incl = n_mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int wbase = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w)
            if (w < wave) wbase += s_wave[w];
        if (tid < RG_GS) {
            d_base[tid] = wbase + incl - n_mine;
            d_bins[tid] = phl | (pwl << 8) | (max(npw, 1) << 16);
            d_inv[tid] = inv_count;
            d_cnt[tid] = n_mine;
        }
        if (tid == RG_GS - 1) d_base[RG_GS] = wbase + incl;
        __syncthreads();
        // ---- entry order: INTERLEAVED over the group's ROIs (level l = the l-th touching bin of every ROI that has one):
        // consecutive entries come from different ROIs, i.e. from all over the region, so every window spreads over all
        // waves.  In ROI-major order a window holds the bins of one or two ROIs and costs the time of the 2-4 waves they
        // hit (summed over the windows of cfg2 the busiest wave saw 32 k entries against 9 k on average).
        // Level l starts at sum_r min(n_r, l); wave w writes the levels l = w (mod 16), rank inside a level by ballot.
        {
            constexpr int RPL = RG_GS / 64;                                  // ROIs per lane
            int n[RPL], bins[RPL];
#pragma unroll
            for (int h = 0; h < RPL; ++h) { n[h] = d_cnt[lane + 64 * h]; bins[h] = d_bins[lane + 64 * h]; }
            const unsigned long long below = (1ull << lane) - 1ull;
            for (int l = wave; l < PP; l += 16) {
                int mins = 0, before = 0;
                unsigned long long have[RPL];
                bool any = false;
#pragma unroll
                for (int h = 0; h < RPL; ++h) { have[h] = __ballot(n[h] > l); mins += min(n[h], l); any |= have[h] != 0; }
                if (!any) break;                                             // uniform: levels are nested
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mins += __shfl_xor(mins, o);
#pragma unroll
                for (int h = 0; h < RPL; ++h) {
                    if (n[h] > l) {
                        const int npw = bins[h] >> 16;
                        const int dph = (int)(((float)l + 0.5f) / (float)npw);      // l / npw (exact for these sizes)
                        const int ph = (bins[h] & 0xff) + dph, pw = ((bins[h] >> 8) & 0xff) + l - dph * npw;
                        emap[mins + before + __popcll(have[h] & below)] = (unsigned short)((lane + 64 * h) | (ph << 7) | (pw << 11));
                    }
                    before += __popcll(have[h]);
                }
            }
        }
        __syncthreads();
    }
    const int total = d_base[RG_GS];

    // loader role of this thread inside a staging window: entry le = tid / 32, two float4 of the slice's 64
    const int le = tid >> 5, lq = (tid & 31) * 2;
    const int cbase = slice * 256;
    // consumer role: lane's 4 channels of the slice
    const int my_touch = (7 << (RG_SBH * wr)) | ((15 << (RG_SBW * wc)) << 16);

    for (int w0 = 0; w0 < total; w0 += RG_MAXE) {
        __syncthreads();                                   // previous super-window fully consumed
        // ---- entry records of [w0, w0 + MAXE): 4 threads per entry, each 3 rows of wy and 4 columns of wx
        {
            const int e = tid >> 2, part = tid & 3;
            const int ge = w0 + e;
            int rm = 0, cm = 0;
            if (ge < total) {
                const int code = emap[ge];
                const int lo = code & 127, ph = (code >> 7) & 15, pw = code >> 11;
                const int k = kgroup * RG_GS + lo;
                const float* rec = rec_all + (size_t)k * recw;
                const float* wy = rec + ph * H;
                const float* wx = rec + P * H + pw * W;
                const float inv_count = d_inv[lo];
                float* r = erec + e * RG_REC;
#pragma unroll
                for (int i = 0; i < RG_SBH; ++i) {
                    const int y = y0 + part * RG_SBH + i;
                    const float v = (y < H) ? wy[y] * inv_count : 0.0f;
                    r[4 + part * 4 + i] = v;
                    if (v != 0.0f) rm |= 1 << (part * RG_SBH + i);
                }
#pragma unroll
                for (int j = 0; j < RG_SBW; ++j) {
                    const int x = x0 + part * RG_SBW + j;
                    const float v = (x < W) ? wx[x] : 0.0f;
                    r[20 + part * 4 + j] = v;
                    if (v != 0.0f) cm |= 1 << (part * RG_SBW + j);
                }
                if (part == 0) {
                    reinterpret_cast<int*>(r)[0] = (((k * P) + ph) * P + pw) * OC;      // < 2^31: checked by the launcher
                    r[1] = MASKCAT ? masks[(size_t)k * PP + ph * P + pw] : 0.0f;
                }
            }
            rm |= __shfl_xor(rm, 1); rm |= __shfl_xor(rm, 2);
            cm |= __shfl_xor(cm, 1); cm |= __shfl_xor(cm, 2);
            if (ge < total && part == 0) reinterpret_cast<int*>(erec + e * RG_REC)[2] = rm | (cm << 16);
        }
        __syncthreads();
        const int n = min(RG_MAXE, total - w0);
        const int nwin = (n + RG_WIN - 1) / RG_WIN;
        // ---- software pipeline over the staging windows: the next window's loads are in flight while this one is consumed
        // (two windows in flight - a second register set - measured no faster: 0.213 vs 0.207 ms)
        struct Regs { float4 r0, r1, h0, h1; float m; };
        auto gload = [&](Regs& R, int win) {
            const int e = win * RG_WIN + le;
            R.r0 = R.r1 = R.h0 = R.h1 = make_float4(0.f, 0.f, 0.f, 0.f);
            R.m = 0.0f;
            if (e < n) {
                const float* rr = erec + e * RG_REC;
                const int off = reinterpret_cast<const int*>(rr)[0];
                const int c0 = min(cbase + lq * 4, C - 4), c1 = min(cbase + lq * 4 + 4, C - 4);
                R.r0 = *reinterpret_cast<const float4*>(grad_out + off + c0);
                R.r1 = *reinterpret_cast<const float4*>(grad_out + off + c1);
                if (MASKCAT) {
                    R.h0 = *reinterpret_cast<const float4*>(grad_out + off + C + c0);
                    R.h1 = *reinterpret_cast<const float4*>(grad_out + off + C + c1);
                    R.m = rr[1];
                }
            }
        };
        auto put = [&](const Regs& R, int buf) {
            float4 a = R.r0, c = R.r1;
            if (MASKCAT) {
                a = make_float4(fmaf(R.m, R.h0.x, a.x), fmaf(R.m, R.h0.y, a.y), fmaf(R.m, R.h0.z, a.z), fmaf(R.m, R.h0.w, a.w));
                c = make_float4(fmaf(R.m, R.h1.x, c.x), fmaf(R.m, R.h1.y, c.y), fmaf(R.m, R.h1.z, c.z), fmaf(R.m, R.h1.w, c.w));
            }
            float* sb = &stage[buf][le][lq * 4];
            *reinterpret_cast<float4*>(sb) = a;
            *reinterpret_cast<float4*>(sb + 4) = c;
        };
        auto consume = [&](int buf, int win) {
            // entries of the window whose bin touches this wave's sub-block
            const int e0 = win * RG_WIN;
            int t = 0;
            if (lane < RG_WIN && e0 + lane < n) t = reinterpret_cast<const int*>(erec + (e0 + lane) * RG_REC)[2];
            const bool hit = ((t & my_touch & 0xffff) != 0) && (((t & my_touch) >> 16) != 0);
            unsigned long long todo = __ballot(hit);
            while (todo) {
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const float* rr = erec + (e0 + j) * RG_REC;
                const float4 g = *reinterpret_cast<const float4*>(&stage[buf][j][lane * 4]);
                const float4 wyq = *reinterpret_cast<const float4*>(rr + 4 + wr * 4);
                const float4 wxq = *reinterpret_cast<const float4*>(rr + 20 + wc * 4);
                const ga_f2 gl = ga_lo(g), gh = ga_hi(g);
                const float wys[3] = {wyq.x, wyq.y, wyq.z};
                const float wxs[4] = {wxq.x, wxq.y, wxq.z, wxq.w};
                // (tried: skipping rows with a zero weight by a scalar branch, 0.227 vs 0.213 ms; reading the next entry's
                // LDS operands one iteration ahead, 0.224 vs 0.207 ms - the phase is paced by the busiest wave of a window)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const ga_f2 tl = ga_f2{wys[i], wys[i]} * gl, th = ga_f2{wys[i], wys[i]} * gh;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        accl[i * 4 + jj] = ga_fma(wxs[jj], tl, accl[i * 4 + jj]);
                        acch[i * 4 + jj] = ga_fma(wxs[jj], th, acch[i * 4 + jj]);
                    }
                }
            }
        };
        Regs A;
        gload(A, 0);
        for (int win = 0; win < nwin; ++win) {
            put(A, win & 1);
            __syncthreads();                               // (also: every wave is done with the buffer the NEXT put overwrites)
            if (win + 1 < nwin) gload(A, win + 1);         // in flight while this window is consumed
            consume(win & 1, win);
        }
    }
    // ---- flush this wave's 3 x 4 pixels
    const int cs = slice * 256 + lane * 4;
    if (cs < C && (total > 0 || !use_atomic || partial)) {
#pragma unroll
        for (int i = 0; i < RG_SBH; ++i)
#pragma unroll
            for (int j = 0; j < RG_SBW; ++j)
                if (sy0 + i < H && sx0 + j < W && sy0 + i < y0 + RG_RH) {
                    const size_t o = (((size_t)b * H + sy0 + i) * W + sx0 + j) * C + cs;
                    float* dst = grad_in + o;
                    const float4 v = make_float4(accl[i * 4 + j].x, accl[i * 4 + j].y, acch[i * 4 + j].x, acch[i * 4 + j].y);
                    if (partial) {      // the groups' partial maps are summed by roi_partial_reduce_kernel (no atomics)
                        __builtin_nontemporal_store(v.x, partial + (size_t)kgroup * B * H * W * C + o);
                        __builtin_nontemporal_store(v.y, partial + (size_t)kgroup * B * H * W * C + o + 1);
                        __builtin_nontemporal_store(v.z, partial + (size_t)kgroup * B * H * W * C + o + 2);
                        __builtin_nontemporal_store(v.w, partial + (size_t)kgroup * B * H * W * C + o + 3);
                    } else if (use_atomic) {
                        atomic_add_vec(dst, v);
                    } else {
                        *reinterpret_cast<float4*>(dst) = v;
                    }
                }
    }
}

// Which kernels launch_fwd and launch_bwd take (CIM_ROI_FWD_* / CIM_ROI_BWD_* of include/cim_hip.h), decided here only and
// reported on the host by cim_roi_align_forms.
//   Forward, table-driven: the table workspace, 16-byte channel rows, 32-bit element offsets and bin rows of at most 64 map rows
//   (maps of <= 64 rows, or <= 128 rows with P >= 4: H / P + 2 rows per bin); the row-sum kernel (two bin rows per workgroup) for
//   maps up to 128 columns and P <= 7, the flat entry-list kernel otherwise.  Else the sample-order kernel.
//   Backward, region form: the table workspace, 16-byte channel rows, 8-bit bin indices in the packed ranges (4 in the entry map:
//   P <= 16), 32-bit element offsets, its LDS and region count.  It reuses tables the caller calls ready only when the forward at
//   this geometry is a table form: every other forward leaves the workspace unwritten.
struct RoiForms {
    int fwd, bwd;
    bool bwd_builds_tables;
};

static RoiForms roi_forms(int B, int C, int H, int W, int K, int P, bool maskcat, bool has_ws, bool tables_ready) {
    RoiForms f;
    const bool fwd_tables = has_ws && C % 4 == 0 && P <= FW_MAXP && (long long)H * W * C < (1ll << 30) &&
                            (H <= 64 || (P >= 4 && H <= RS_MAXD));
    if (fwd_tables)
        f.fwd = (P <= 7 && W <= RS_MAXD) ? CIM_ROI_FWD_ROWSUM2 : CIM_ROI_FWD_AGG;
    else
        f.fwd = C % 4 == 0 ? CIM_ROI_FWD_SAMPLE4 : CIM_ROI_FWD_SAMPLE1;
    const bool region = K > 0 && has_ws && C % 4 == 0 && P <= 16 && H < 256 && W < 256 &&
                        (long long)K * P * P * (maskcat ? 2 : 1) * C < (1ll << 31) &&
                        rg_lds_bytes(rg_group_size(K, B, C, H, W), P) <= 158 * 1024 &&
                        ((H + RG_RH - 1) / RG_RH) * ((W + RG_RW - 1) / RG_RW) <= RG_MAXREG &&
                        (long long)B * ((K + 63) / 64) * ((C + 255) / 256) * RG_MAXREG < (1ll << 31);
    f.bwd = region ? CIM_ROI_BWD_REGION : C % 4 == 0 ? CIM_ROI_BWD_GENERIC4 : CIM_ROI_BWD_GENERIC1;
    f.bwd_builds_tables = region && !(tables_ready && fwd_tables);
    return f;
}

template <bool MASKCAT>
int launch_fwd(const float* feat, const float* rois, const float* masks, float* out, int B, int C, int H, int W, int K,
               int P, float scale, int sr, int aligned, hipStream_t st, float* ws) {
    if (K == 0) return 0;
    dim3 grid(K, P), block(256);
    const int form = roi_forms(B, C, H, W, K, P, MASKCAT, ws != nullptr, false).fwd;
    if (form == CIM_ROI_FWD_ROWSUM2 || form == CIM_ROI_FWD_AGG) {
        hipLaunchKernelGGL(roi_tables_kernel, dim3(K), dim3(256), sizeof(float) * roi_rec_words(P, H, W), st, rois, ws, K, P, H, W, scale, sr, aligned);
        if (form == CIM_ROI_FWD_ROWSUM2) {
            const int nth = C >= 1024 ? 256 : ((C / 4 + 63) / 64) * 64;       // narrow maps: no idle waves
            hipLaunchKernelGGL((roi_align_fwd_rowsum2_kernel<MASKCAT>), dim3(K, (P + 1) / 2), dim3(nth), 0, st, feat, masks, out, C, H, W, P, ws);
            return 0;
        }
        hipLaunchKernelGGL((roi_align_fwd_agg_kernel<MASKCAT>), grid, block, 0, st, feat, masks, out, C, H, W, P, ws, rois, scale, sr,
                           aligned);
        return 0;
    }
    // sample-order kernel (the oracle's operation order: bit-identical; any C, P, map size)
    if (form == CIM_ROI_FWD_SAMPLE4)
        hipLaunchKernelGGL((roi_align_fwd_kernel<4, MASKCAT>), grid, block, 0, st, feat, rois, masks, out, C, H, W, P,
                           scale, sr, aligned);
    else
        hipLaunchKernelGGL((roi_align_fwd_kernel<1, MASKCAT>), grid, block, 0, st, feat, rois, masks, out, C, H, W, P,
                           scale, sr, aligned);
    return 0;
}

// Region order, centre first (the centre regions carry the most entries: longest jobs first), computed on the host
// and passed by value.
static RegionOrder region_order(int ry, int rx) {
    RegionOrder ro;
    const int n = ry * rx;
    int idx[RG_MAXREG];
    float d[RG_MAXREG];
    for (int r = 0; r < n; ++r) {
        const float dy = (r / rx) + 0.5f - 0.5f * ry, dx = (r % rx) + 0.5f - 0.5f * rx;
        idx[r] = r;
        d[r] = dy * dy * (float)(RG_RH * RG_RH) + dx * dx * (float)(RG_RW * RG_RW);
    }
    for (int i = 0; i < n; ++i) {
        int best = i;
        for (int j = i + 1; j < n; ++j)
            if (d[idx[j]] < d[idx[best]]) best = j;
        const int t = idx[i]; idx[i] = idx[best]; idx[best] = t;
        ro.o[i] = (unsigned char)idx[i];
    }
    return ro;
}

// grad_in = sum over the ROI groups' partial maps: n4 float4 per map, groups maps `stride4` float4 apart.
__global__ __launch_bounds__(256) void roi_partial_reduce_kernel(const float4* __restrict__ partial, float4* __restrict__ out,
                                                                 size_t n4, int groups) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    typedef float rp_f4 __attribute__((ext_vector_type(4)));
    const rp_f4* p = reinterpret_cast<const rp_f4*>(partial) + i;
    rp_f4 acc = __builtin_nontemporal_load(p);
    for (int g = 1; g < groups; ++g) acc += __builtin_nontemporal_load(p + (size_t)g * n4);
    out[i] = make_float4(acc.x, acc.y, acc.z, acc.w);
}

template <bool MASKCAT>
static int launch_bwd_region(const float* go, const float* rois, const float* masks, float* gin, int B, int C, int H, int W,
                             int K, int P, float scale, int sr, int aligned, float* ws, hipStream_t st, bool build_tables,
                             float* scratch) {
    if (build_tables)
        hipLaunchKernelGGL(roi_tables_kernel, dim3(K), dim3(256), sizeof(float) * roi_rec_words(P, H, W), st, rois, ws, K, P, H, W, scale, sr, aligned);
    const int ry = (H + RG_RH - 1) / RG_RH, rx = (W + RG_RW - 1) / RG_RW, n_regions = ry * rx;
    const RegionOrder order = region_order(ry, rx);
    const int GS = rg_group_size(K, B, C, H, W);
    const int groups = (K + GS - 1) / GS, n_slices = (C + 255) / 256;
    float* partial = (groups > 1) ? scratch : nullptr;      // without scratch the groups meet through atomicAdd (slow)
    if (groups > 1 && !partial) {
        hipError_t e = hipMemsetAsync(gin, 0, sizeof(float) * (size_t)B * H * W * C, st);
        if (e != hipSuccess) return (int)e;
    }
    auto kern = GS == 128 ? roi_align_bwd_region_kernel<MASKCAT, 128> : roi_align_bwd_region_kernel<MASKCAT, 64>;
    const size_t lds = rg_lds_bytes(GS, P);
    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return (int)ea;
    hipLaunchKernelGGL(kern, dim3((unsigned)(n_slices * B * groups * n_regions)), dim3(RG_NT), lds, st, go, masks, gin, C, H, W, K, P, B,
                       groups > 1 ? 1 : 0, ws, order, n_regions, rx, n_slices, partial);
    if (partial) {
        const size_t n4 = (size_t)B * H * W * C / 4;
        hipLaunchKernelGGL(roi_partial_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(partial), reinterpret_cast<float4*>(gin), n4, groups);
    }
    return 0;
}

template <bool MASKCAT>
int launch_bwd(const float* go, const float* rois, const float* masks, float* gin, int B, int C, int H, int W, int K,
               int P, float scale, int sr, int aligned, float* ws, hipStream_t st, int tables_ready, float* scratch) {
    // region form (roi_forms).  With several ROI groups and no partial-map scratch the groups meet through atomicAdd: slow, but
    // every entry point works.
    const RoiForms f = roi_forms(B, C, H, W, K, P, MASKCAT, ws != nullptr, tables_ready != 0);
    if (f.bwd == CIM_ROI_BWD_REGION)
        return launch_bwd_region<MASKCAT>(go, rois, masks, gin, B, C, H, W, K, P, scale, sr, aligned, ws, st, f.bwd_builds_tables, scratch);
    // generic form (odd channel counts, no workspace, maps beyond the region form's limits): one thread per output element,
    // global atomics - the reference's own formulation
    hipError_t e = hipMemsetAsync(gin, 0, sizeof(float) * (size_t)B * H * W * C, st);
    if (e != hipSuccess) return (int)e;
    if (K == 0) return 0;
    dim3 grid(K, P), block(256);
    if (f.bwd == CIM_ROI_BWD_GENERIC4)
        hipLaunchKernelGGL((roi_align_bwd_kernel<4, MASKCAT>), grid, block, 0, st, go, rois, masks, gin, C, H, W, P,
                           scale, sr, aligned);
    else
        hipLaunchKernelGGL((roi_align_bwd_kernel<1, MASKCAT>), grid, block, 0, st, go, rois, masks, gin, C, H, W, P,
                           scale, sr, aligned);
    return 0;
}

}  // namespace

// The body of the forward / backward C entry points: argument check, launch, launch error (`fn`: the entry, for the error text).
#define ROI_CHECK_ARG(cond)                                                   \
    do {                                                                      \
        if (!(cond)) {                                                        \
            cim::set_error("%s: bad argument: %s", fn, #cond);                \
            return -1;                                                        \
        }                                                                     \
    } while (0)

static int roi_finish(const char* fn, int rc) {
    if (rc) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) cim::set_error("%s: %s", fn, hipGetErrorString(e));
    return (int)e;
}

template <bool MASKCAT>
static int run_fwd(const char* fn, const float* feat, const float* rois, const float* masks, float* out, int B, int C, int H, int W,
                   int K, int P, float scale, int sr, int aligned, float* workspace, void* stream) {
    ROI_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && K >= 0 && P > 0 && P <= 65535);
    ROI_CHECK_ARG(rois != nullptr || K == 0);
    ROI_CHECK_ARG(feat && ((out && (masks || !MASKCAT)) || K == 0));
    return roi_finish(fn, launch_fwd<MASKCAT>(feat, rois, masks, out, B, C, H, W, K, P, scale, sr, aligned, cim::as_stream(stream), workspace));
}

template <bool MASKCAT>
static int run_bwd(const char* fn, const float* grad_out, const float* rois, const float* masks, float* grad_in, int B, int C, int H,
                   int W, int K, int P, float scale, int sr, int aligned, float* workspace, int tables_ready, float* scratch,
                   void* stream) {
    ROI_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && K >= 0 && P > 0 && P <= 65535);
    ROI_CHECK_ARG(rois != nullptr || K == 0);
    ROI_CHECK_ARG(grad_in && ((grad_out && (masks || !MASKCAT)) || K == 0) && (workspace || !tables_ready));
    return roi_finish(fn, launch_bwd<MASKCAT>(grad_out, rois, masks, grad_in, B, C, H, W, K, P, scale, sr, aligned, workspace,
                                              cim::as_stream(stream), tables_ready, scratch));
}

extern "C" int cim_roi_align_fwd(const float* feat, const float* rois, float* out, int B, int C, int H, int W, int K,
                                 int P, float spatial_scale, int sampling_ratio, int aligned, void* stream) {
    return run_fwd<false>(__func__, feat, rois, nullptr, out, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, nullptr, stream);
}

extern "C" int cim_roi_align_fwd_ws(const float* feat, const float* rois, float* out, int B, int C, int H, int W, int K,
                                    int P, float spatial_scale, int sampling_ratio, int aligned, float* workspace,
                                    void* stream) {
    return run_fwd<false>(__func__, feat, rois, nullptr, out, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, workspace, stream);
}

extern "C" int cim_roi_align_maskcat_fwd(const float* feat, const float* rois, const float* masks, float* cat, int B,
                                         int C, int H, int W, int K, int P, float spatial_scale, int sampling_ratio,
                                         int aligned, void* stream) {
    return run_fwd<true>(__func__, feat, rois, masks, cat, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, nullptr, stream);
}

extern "C" int cim_roi_align_maskcat_fwd_ws(const float* feat, const float* rois, const float* masks, float* cat, int B,
                                            int C, int H, int W, int K, int P, float spatial_scale, int sampling_ratio,
                                            int aligned, float* workspace, void* stream) {
    return run_fwd<true>(__func__, feat, rois, masks, cat, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, workspace, stream);
}

// (without tables_ready / scratch: the tables are rebuilt, and several ROI groups meet through atomicAdd)
extern "C" int cim_roi_align_bwd(const float* grad_out, const float* rois, float* grad_in, int B, int C, int H, int W,
                                 int K, int P, float spatial_scale, int sampling_ratio, int aligned, float* workspace,
                                 void* stream) {
    return run_bwd<false>(__func__, grad_out, rois, nullptr, grad_in, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, workspace,
                          0, nullptr, stream);
}

extern "C" int cim_roi_align_bwd_ws(const float* grad_out, const float* rois, float* grad_in, int B, int C, int H, int W,
                                    int K, int P, float spatial_scale, int sampling_ratio, int aligned, float* workspace,
                                    int tables_ready, float* scratch, void* stream) {
    return run_bwd<false>(__func__, grad_out, rois, nullptr, grad_in, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, workspace,
                          tables_ready, scratch, stream);
}

extern "C" int cim_roi_align_maskcat_bwd(const float* grad_cat, const float* rois, const float* masks, float* grad_in,
                                         int B, int C, int H, int W, int K, int P, float spatial_scale,
                                         int sampling_ratio, int aligned, float* workspace, void* stream) {
    return run_bwd<true>(__func__, grad_cat, rois, masks, grad_in, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, workspace,
                         0, nullptr, stream);
}

extern "C" int cim_roi_align_maskcat_bwd_ws(const float* grad_cat, const float* rois, const float* masks, float* grad_in,
                                            int B, int C, int H, int W, int K, int P, float spatial_scale,
                                            int sampling_ratio, int aligned, float* workspace, int tables_ready,
                                            float* scratch, void* stream) {
    return run_bwd<true>(__func__, grad_cat, rois, masks, grad_in, B, C, H, W, K, P, spatial_scale, sampling_ratio, aligned, workspace,
                         tables_ready, scratch, stream);
}
#undef ROI_CHECK_ARG

extern "C" int cim_roi_align_wino7_pair_fwd(const float* feat, const float* rois, const float* masks, void* V, const float* scale,
                                           int B, int C, int H, int W, int K, int Rs, int P, float spatial_scale,
                                           int sampling_ratio, int aligned, float* workspace, void* stream) {
    CIM_CHECK_ARG(feat && rois && masks && V && scale && workspace);
    CIM_CHECK_ARG(B > 0 && C > 0 && C % 8 == 0 && H > 0 && W > 0 && K > 0 && Rs >= K && P == 7);
    CIM_CHECK_ARG(H <= RS_MAXD && W <= RS_MAXD && (long long)H * W * C < (1ll << 30));
    hipStream_t st = cim::as_stream(stream);
    hipLaunchKernelGGL(roi_tables_kernel, dim3(K), dim3(256), sizeof(float) * roi_rec_words(P, H, W), st, rois, workspace, K, P, H, W,
                       spatial_scale, sampling_ratio, aligned);
    hipLaunchKernelGGL(roi_align_wino7_pair_kernel, dim3((unsigned)Rs, (unsigned)((C + 255) / 256)), dim3(256), 0, st, feat, masks,
                       (float*)V, C, H, W, K, Rs, workspace, scale);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_roi_align_forms(int B, int C, int H, int W, int K, int P, int maskcat, int has_workspace, int tables_ready,
                                   int* fwd_form, int* bwd_form, int* bwd_builds_tables) {
    CIM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && K >= 0 && P > 0 && P <= 65535);
    CIM_CHECK_ARG(fwd_form && bwd_form && bwd_builds_tables && (has_workspace || !tables_ready));
    const RoiForms f = roi_forms(B, C, H, W, K, P, maskcat != 0, has_workspace != 0, tables_ready != 0);
    *fwd_form = f.fwd;
    *bwd_form = f.bwd;
    *bwd_builds_tables = f.bwd_builds_tables ? 1 : 0;
    return 0;
}

extern "C" long long cim_roi_align_bwd_workspace(int K, int P, int H, int W) {
    return (long long)sizeof(float) * (long long)K * roi_rec_words(P, H, W);
}

extern "C" long long cim_roi_align_bwd_scratch(int K, int B, int C, int H, int W) {
    const int GS = rg_group_size(K, B, C, H, W);
    const long long groups = (K + GS - 1) / GS;
    return groups > 1 ? (long long)sizeof(float) * groups * B * H * W * C : 0;
}
