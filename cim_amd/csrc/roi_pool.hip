// RoIPool forward / backward for gfx950, channels-last, optionally fused with the MaskFuse prologue (mask multiply + channel
// concat): FAST_RCNN.ROI_XFORM_METHOD = RoIPoolF (lib/modeling/model_builder.py:215-233; mmcv.ops.roi_pool).  The contract -
// bin bounds, scan order, ties, NaN, empty bins - is in include/cim_hip.h and DESIGN.md 4.24; tests/golden/roi_pool_np.py
// restates it float for float.
//
// Layout: feat [B,H,W,C], out [K,P,P,C] (or cat [K,P,P,2C]), argmax int32 [K,P,P,C]; lanes run along C.
//   forward   a workgroup owns one (roi, bin row); a lane holds 4 channels (16-byte accesses; 1 where C % 4 != 0 or a base is
//             not 16-byte aligned) and scans its bin's pixels once.
//   backward  every (roi, bin, channel) has ONE destination pixel.  A workgroup owns an 8 x 8 pixel region x 256 channels of one
//             image for one group of ROIs; a lane owns ONE channel's column of the region in LDS ([pixel][lane]: no bank
//             conflict, no other lane ever touches it) and walks ONE list - the group's bins that reach the region, in
//             ascending (k, ph, pw), made by the workgroup from the bins' bounds - adding in that order: no atomics, the same
//             bits every call.  Groups meet through per-group partial maps in the caller's scratch, summed in group order
//             by one streaming pass.
#include <cfloat>
#include "common.h"
#include "../../include/cim_hip.h"

namespace {

struct PoolGeom {
    float rx1, ry1, bw, bh;
    int b;
    bool ok;        // false: malformed (rw <= 0 or rh <= 0) - every output 0, every argmax -1
};

// the geometry and the bounds round every operation separately (the contract): no FMA contraction from here on
#pragma clang fp contract(off)
__device__ __forceinline__ PoolGeom pool_geom(const float* __restrict__ roi, float scale, int P) {
    PoolGeom g;
    g.b = (int)roi[0];
    g.rx1 = roi[1] * scale;
    g.ry1 = roi[2] * scale;
    const float rx2 = (roi[3] + 1.0f) * scale;
    const float ry2 = (roi[4] + 1.0f) * scale;
    const float rw = rx2 - g.rx1, rh = ry2 - g.ry1;
    g.ok = !(rw <= 0.0f || rh <= 0.0f);
    g.bw = rw / (float)P;
    g.bh = rh / (float)P;
    return g;
}

// a rounded bound -> [0, size] (clamped as a float first: the conversion never sees a value outside int; 2147483520 is the
// largest float below 2^31)
__device__ __forceinline__ int pool_clamp(float v, int size) {
    const int i = (int)fminf(fmaxf(v, 0.0f), 2147483520.0f);
    return i < size ? i : size;
}
__device__ __forceinline__ int bin_lo(int p, float bin, float r1, int size) { return pool_clamp(floorf((float)p * bin + r1), size); }
__device__ __forceinline__ int bin_hi(int p, float bin, float r1, int size) { return pool_clamp(ceilf((float)(p + 1) * bin + r1), size); }

template <int VEC> struct PoolVec;
template <> struct PoolVec<1> { using F = float; using I = int; };
template <> struct PoolVec<4> { using F = float4; using I = int4; };

__device__ __forceinline__ void pool_init(float& v, int& i, float fill) { v = fill; i = -1; }
__device__ __forceinline__ void pool_init(float4& v, int4& i, float fill) { v = make_float4(fill, fill, fill, fill); i = make_int4(-1, -1, -1, -1); }
// strict >: the first maximum in scan order wins, NaN is never taken
__device__ __forceinline__ void pool_pick(float& v, int& i, float p, int at) {
    if (p > v) { v = p; i = at; }
}
__device__ __forceinline__ void pool_pick(float4& v, int4& i, float4 p, int at) {
    pool_pick(v.x, i.x, p.x, at);
    pool_pick(v.y, i.y, p.y, at);
    pool_pick(v.z, i.z, p.z, at);
    pool_pick(v.w, i.w, p.w, at);
}
__device__ __forceinline__ float pool_mul(float m, float v) { return m * v; }
__device__ __forceinline__ float4 pool_mul(float m, float4 v) { return make_float4(m * v.x, m * v.y, m * v.z, m * v.w); }

// grid = K * P workgroups: (roi k, bin row ph); block = 256 lanes along C.
template <int VEC, bool MASKCAT>
__global__ __launch_bounds__(256) void roi_pool_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ rois,
                                                           const float* __restrict__ masks, float* __restrict__ out,
                                                           int* __restrict__ argmax, int B, int C, int H, int W, int P, float scale) {
    using F = typename PoolVec<VEC>::F;
    using I = typename PoolVec<VEC>::I;
    const int k = blockIdx.x / P, ph = blockIdx.x - k * P;
    const PoolGeom g = pool_geom(rois + 5 * (size_t)k, scale, P);
    const bool ok = g.ok && g.b >= 0 && g.b < B;        // (an image that is not there is no error: the ROI comes out as a malformed one)
    const float* __restrict__ fb = feat + (size_t)(ok ? g.b : 0) * H * W * C;
    const int OC = MASKCAT ? 2 * C : C;
    const int ylo = ok ? bin_lo(ph, g.bh, g.ry1, H) : 0, yhi = ok ? bin_hi(ph, g.bh, g.ry1, H) : 0;
    for (int c = threadIdx.x * VEC; c < C; c += 256 * VEC) {
        for (int pw = 0; pw < P; ++pw) {
            const int xlo = bin_lo(pw, g.bw, g.rx1, W), xhi = bin_hi(pw, g.bw, g.rx1, W);
            const bool empty = yhi <= ylo || xhi <= xlo;
            F v;
            I idx;
            pool_init(v, idx, empty ? 0.0f : -FLT_MAX);
            if (!empty) {
                for (int y = ylo; y < yhi; ++y) {
                    const float* __restrict__ row = fb + ((size_t)y * W + xlo) * C + c;
#pragma unroll 4
                    for (int x = xlo; x < xhi; ++x, row += C) pool_pick(v, idx, *reinterpret_cast<const F*>(row), y * W + x);
                }
            }
            const size_t bin = ((size_t)k * P + ph) * P + pw;
            *reinterpret_cast<F*>(out + bin * OC + c) = v;
            if (MASKCAT) *reinterpret_cast<F*>(out + bin * OC + C + c) = pool_mul(masks[bin], v);
            if (argmax) *reinterpret_cast<I*>(argmax + bin * C + c) = idx;
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
constexpr int RP_R = 8;                 // a region is RP_R x RP_R pixels
constexpr int RP_NT = 256;              // lanes = channels of a slice; the region's sums take RP_R * RP_R * RP_NT floats = 64 KiB of LDS
constexpr int RP_LIST = 2048;           // bins of a piece of the work list
constexpr int RP_BATCH = 8;             // bins whose loads are in flight together
constexpr int RP_TARGET_WGS = 1024;     // ROI groups are added while the grid stays within this many workgroups (two per CU) ...
constexpr int RP_MAX_GROUPS = 16;       // ... at most this many (each costs one partial map), each of at least RP_MIN_GROUP ROIs
constexpr int RP_MIN_GROUP = 4;
constexpr size_t RP_LDS = sizeof(float) * RP_R * RP_R * RP_NT + sizeof(int) * (RP_LIST + 4 * RP_NT + 4);       // 76 KiB: two workgroups per CU

static inline long long rp_jobs_per_group(int B, int C, int H, int W) {
    return (long long)((H + RP_R - 1) / RP_R) * ((W + RP_R - 1) / RP_R) * ((C + RP_NT - 1) / RP_NT) * B;
}

static inline int rp_groups(int K, int B, int C, int H, int W) {
    long long g = RP_TARGET_WGS / rp_jobs_per_group(B, C, H, W);
    if (g > RP_MAX_GROUPS) g = RP_MAX_GROUPS;
    if (g > K / RP_MIN_GROUP) g = K / RP_MIN_GROUP;
    return g < 1 ? 1 : (int)g;
}

// dst: grad_in (one group) or the groups' partial maps, `map` floats apart.  Every element of a job's region x slice is stored
// once, so every element of every map is written.  jobs_per_xcd: consecutive jobs - the regions of one (group, slice), which
// read the same bins - go to workgroups 8 apart, which share an L2 (an observed placement: speed only).
//
// The group's ROIs are taken RP_NT at a time.  Lane t finds the bins of ROI t that reach the region - bounds are monotone in
// the bin index, so they form one range per axis -, a prefix sum over the lanes orders them, and the workgroup writes them out
// as ONE list of bin numbers in ascending (k, ph, pw), in pieces of RP_LIST.  Then every lane walks the list for its channel:
// the loads of RP_BATCH bins in flight together, the adds in list order.
template <bool MASKCAT>
__global__ __launch_bounds__(RP_NT) void roi_pool_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ rois,
                                                             const float* __restrict__ masks, const int* __restrict__ argmax,
                                                             float* __restrict__ dst, int B, int C, int H, int W, int K, int P,
                                                             float scale, int groups, long long jobs, long long jobs_per_xcd,
                                                             size_t map) {
    extern __shared__ __align__(16) float rp_lds[];
    float* acc = rp_lds;                                                   // [pixel][lane]
    int* list = reinterpret_cast<int*>(rp_lds + RP_R * RP_R * RP_NT);      // [RP_LIST] bin numbers (k * P + ph) * P + pw
    int* r_end = list + RP_LIST;                                           // [lane] bins of ROIs 0 .. lane of the chunk
    int* r_pha = r_end + RP_NT;                                            // [lane] first bin row, first bin column, columns
    int* r_pwa = r_pha + RP_NT;
    int* r_nw = r_pwa + RP_NT;
    int* wsum = r_nw + RP_NT;                                              // [4] bins per wave
    long long job = (long long)(blockIdx.x % 8) * jobs_per_xcd + blockIdx.x / 8;
    if (job >= jobs) return;
    const int nrx = (W + RP_R - 1) / RP_R, nry = (H + RP_R - 1) / RP_R, slices = (C + RP_NT - 1) / RP_NT;
    const int rxi = (int)(job % nrx);
    job /= nrx;
    const int ryi = (int)(job % nry);
    job /= nry;
    const int slice = (int)(job % slices);
    job /= slices;
    const int b = (int)(job % B), grp = (int)(job / B);
    const int tid = threadIdx.x, c = slice * RP_NT + tid;
    const bool live = c < C;            // (a lane without a channel still takes an ROI of every chunk)
    const int y0 = ryi * RP_R, x0 = rxi * RP_R;
    const int y1 = y0 + RP_R < H ? y0 + RP_R : H, x1 = x0 + RP_R < W ? x0 + RP_R : W;
    float* __restrict__ col = acc + tid;        // no other lane ever touches this column
#pragma unroll
    for (int p = 0; p < RP_R * RP_R; ++p) col[p * RP_NT] = 0.0f;

    const int GC = MASKCAT ? 2 * C : C;
    const unsigned origin = (unsigned)(y0 * W + x0);
    const unsigned w2 = W > 0x3fffffff ? 0xffffffffu : 2u * W, w4 = W > 0x1fffffff ? 0xffffffffu : 4u * W;      // (an index is below 2^31)
    const int per = (K + groups - 1) / groups;
    const int k0 = grp * per, k1 = k0 + per < K ? k0 + per : K;
    for (int kc = k0; kc < k1; kc += RP_NT) {
        int pha = P, phb = 0, pwa = P, pwb = 0, nw = 0, n = 0;
        if (kc + tid < k1) {
            const PoolGeom g = pool_geom(rois + 5 * (size_t)(kc + tid), scale, P);
            if (g.b == b && g.ok) {
                for (int p = 0; p < P; ++p) {
                    if (bin_lo(p, g.bh, g.ry1, H) < y1 && bin_hi(p, g.bh, g.ry1, H) > y0) {
                        pha = p < pha ? p : pha;
                        phb = p + 1;
                    }
                    if (bin_lo(p, g.bw, g.rx1, W) < x1 && bin_hi(p, g.bw, g.rx1, W) > x0) {
                        pwa = p < pwa ? p : pwa;
                        pwb = p + 1;
                    }
                }
                if (pha < phb && pwa < pwb) {
                    nw = pwb - pwa;
                    n = (phb - pha) * nw;
                }
            }
        }
        int upto = n;                   // inclusive prefix sum over the wave, then over the waves
        for (int s = 1; s < 64; s <<= 1) {
            const int t = __shfl_up(upto, s);
            if ((tid & 63) >= s) upto += t;
        }
        if ((tid & 63) == 63) wsum[tid >> 6] = upto;
        __syncthreads();
        for (int w = 0; w < (tid >> 6); ++w) upto += wsum[w];
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        r_end[tid] = upto;
        r_pha[tid] = pha;
        r_pwa[tid] = pwa;
        r_nw[tid] = nw;
        __syncthreads();
        for (int base = 0; base < total; base += RP_LIST) {
            const int m = total - base < RP_LIST ? total - base : RP_LIST;
            for (int i = tid; i < m; i += RP_NT) {
                int lo = 0, hi = RP_NT - 1;             // the ROI of bin base + i of the chunk: the first lane whose r_end is above it
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (r_end[mid] > base + i) hi = mid;
                    else lo = mid + 1;
                }
                const int j = base + i - (lo ? r_end[lo - 1] : 0), w = r_nw[lo];
                list[i] = ((kc + lo) * P + r_pha[lo] + j / w) * P + r_pwa[lo] + j % w;
            }
            __syncthreads();
            for (int j0 = 0; j0 < m && live; j0 += RP_BATCH) {
                int idx[RP_BATCH];
                float d[RP_BATCH];
#pragma unroll
                for (int u = 0; u < RP_BATCH; ++u) {        // the loads of a batch are independent: all in flight before the first add
                    idx[u] = -1;
                    d[u] = 0.0f;
                    if (j0 + u < m) {
                        const size_t bin = (size_t)__builtin_amdgcn_readfirstlane(list[j0 + u]);      // (one value for the wave: scalar addresses)
                        idx[u] = argmax[bin * C + c];
                        d[u] = MASKCAT ? grad[bin * GC + c] + masks[bin] * grad[bin * GC + C + c] : grad[bin * GC + c];
                    }
                }
#pragma unroll
                for (int u = 0; u < RP_BATCH; ++u) {        // in order: two bins of a batch may name the same pixel
                    // the pixel's place in the region, if it is in it: idx - origin = row * W + column with column < width <= W
                    // (a pixel left of the region lands a row up with a column at or beyond the width; -1 and any other index
                    // fall out the same way)
                    unsigned t = (unsigned)idx[u] - origin;
                    int r = 0;
                    if (t >= w4) { t -= w4; r = 4; }
                    if (t >= w2) { t -= w2; r += 2; }
                    if (t >= (unsigned)W) { t -= (unsigned)W; r += 1; }
                    const int at = (r < y1 - y0 && t < (unsigned)(x1 - x0)) ? r * RP_R + (int)t : -1;
                    if (at >= 0) col[at * RP_NT] += d[u];
                }
            }
            __syncthreads();
        }
    }
    if (!live) return;
    float* __restrict__ o = dst + (size_t)grp * map + (size_t)b * H * W * C + c;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) o[((size_t)y * W + x) * C] = col[((y - y0) * RP_R + (x - x0)) * RP_NT];
}

// out = the groups' partial maps summed in group order: n elements of VEC floats per map, maps `n` elements apart.
template <int VEC>
__global__ __launch_bounds__(256) void roi_pool_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out, size_t n,
                                                              int groups) {
    using F = typename PoolVec<VEC>::F;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const F* p = reinterpret_cast<const F*>(partial) + i;
    F a = p[0];
    for (int g = 1; g < groups; ++g) {
        const F t = p[(size_t)g * n];
        if constexpr (VEC == 4) a = make_float4(a.x + t.x, a.y + t.y, a.z + t.z, a.w + t.w);
        else a = a + t;
    }
    reinterpret_cast<F*>(out)[i] = a;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

#define POOL_CHECK_ARG(cond)                                                  \
    do {                                                                      \
        if (!(cond)) {                                                        \
            cim::set_error("%s: bad argument: %s", fn, #cond);                \
            return -1;                                                        \
        }                                                                     \
    } while (0)

// what every entry refuses, before any device work
#define POOL_CHECK_DIMS(OC)                                                                  \
    POOL_CHECK_ARG(B >= 1);                                                                  \
    POOL_CHECK_ARG(C >= 1);                                                                  \
    POOL_CHECK_ARG(H >= 1);                                                                  \
    POOL_CHECK_ARG(W >= 1);                                                                  \
    POOL_CHECK_ARG(P >= 1);                                                                  \
    POOL_CHECK_ARG(K >= 0);                                                                  \
    POOL_CHECK_ARG((long long)H * W < (1ll << 31));                                          \
    POOL_CHECK_ARG((double)K * P * P * (OC) < 2147483648.0)

static int pool_finish(const char* fn) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) cim::set_error("%s: %s", fn, hipGetErrorString(e));
    return (int)e;
}

template <bool MASKCAT>
static int pool_fwd(const char* fn, const float* feat, const float* rois, const float* masks, float* out, int* argmax, int B, int C,
                    int H, int W, int K, int P, float scale, void* stream) {
    POOL_CHECK_DIMS(MASKCAT ? 2.0 * C : (double)C);
    POOL_CHECK_ARG(feat != nullptr);
    POOL_CHECK_ARG(rois != nullptr || K == 0);
    POOL_CHECK_ARG(out != nullptr || K == 0);
    POOL_CHECK_ARG(masks != nullptr || K == 0 || !MASKCAT);
    if (K == 0) return 0;
    const dim3 grid((unsigned)(K * P)), block(256);
    hipStream_t st = cim::as_stream(stream);
    if (C % 4 == 0 && aligned16(feat) && aligned16(out) && aligned16(argmax))
        hipLaunchKernelGGL((roi_pool_fwd_kernel<4, MASKCAT>), grid, block, 0, st, feat, rois, masks, out, argmax, B, C, H, W, P, scale);
    else
        hipLaunchKernelGGL((roi_pool_fwd_kernel<1, MASKCAT>), grid, block, 0, st, feat, rois, masks, out, argmax, B, C, H, W, P, scale);
    return pool_finish(fn);
}

template <bool MASKCAT>
static int pool_bwd(const char* fn, const float* grad, const float* rois, const float* masks, const int* argmax, float* grad_in, int B,
                    int C, int H, int W, int K, int P, float scale, float* scratch, void* stream) {
    POOL_CHECK_DIMS(MASKCAT ? 2.0 * C : (double)C);
    POOL_CHECK_ARG(grad_in != nullptr);
    POOL_CHECK_ARG(grad != nullptr || K == 0);
    POOL_CHECK_ARG(rois != nullptr || K == 0);
    POOL_CHECK_ARG(argmax != nullptr || K == 0);
    POOL_CHECK_ARG(masks != nullptr || K == 0 || !MASKCAT);
    const int groups = rp_groups(K, B, C, H, W);
    POOL_CHECK_ARG(scratch != nullptr || groups == 1);
    const long long per_group = rp_jobs_per_group(B, C, H, W), jobs = per_group * groups, jobs_per_xcd = (jobs + 7) / 8;
    POOL_CHECK_ARG(8 * jobs_per_xcd < (1ll << 31));
    const size_t map = (size_t)B * H * W * C;
    hipStream_t st = cim::as_stream(stream);
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(roi_pool_bwd_kernel<MASKCAT>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)RP_LDS);
    if (ea != hipSuccess) {
        cim::set_error("%s: %s", fn, hipGetErrorString(ea));
        return (int)ea;
    }
    hipLaunchKernelGGL((roi_pool_bwd_kernel<MASKCAT>), dim3((unsigned)(8 * jobs_per_xcd)), dim3(RP_NT), RP_LDS, st, grad, rois, masks, argmax,
                       groups > 1 ? scratch : grad_in, B, C, H, W, K, P, scale, groups, jobs, jobs_per_xcd, map);
    if (groups > 1) {
        if (map % 4 == 0 && aligned16(scratch) && aligned16(grad_in))
            hipLaunchKernelGGL((roi_pool_reduce_kernel<4>), dim3((unsigned)((map / 4 + 255) / 256)), dim3(256), 0, st, scratch, grad_in,
                               map / 4, groups);
        else
            hipLaunchKernelGGL((roi_pool_reduce_kernel<1>), dim3((unsigned)((map + 255) / 256)), dim3(256), 0, st, scratch, grad_in, map,
                               groups);
    }
    return pool_finish(fn);
}

extern "C" int cim_roi_pool_fwd(const float* feat, const float* rois, float* out, int* argmax, int B, int C, int H, int W, int K,
                                int P, float spatial_scale, void* stream) {
    return pool_fwd<false>(__func__, feat, rois, nullptr, out, argmax, B, C, H, W, K, P, spatial_scale, stream);
}

extern "C" int cim_roi_pool_maskcat_fwd(const float* feat, const float* rois, const float* masks, float* cat, int* argmax, int B,
                                        int C, int H, int W, int K, int P, float spatial_scale, void* stream) {
    return pool_fwd<true>(__func__, feat, rois, masks, cat, argmax, B, C, H, W, K, P, spatial_scale, stream);
}

extern "C" long long cim_roi_pool_bwd_scratch(int K, int B, int C, int H, int W, int P) {
    if (K < 0 || B < 1 || C < 1 || H < 1 || W < 1 || P < 1) {
        cim::set_error("%s: bad argument: K >= 0 and B, C, H, W, P >= 1", __func__);
        return -1;
    }
    const long long groups = rp_groups(K, B, C, H, W);
    return groups > 1 ? (long long)sizeof(float) * groups * B * H * W * C : 0;
}

extern "C" int cim_roi_pool_bwd(const float* grad_out, const float* rois, const int* argmax, float* grad_in, int B, int C, int H,
                                int W, int K, int P, float spatial_scale, float* scratch, void* stream) {
    return pool_bwd<false>(__func__, grad_out, rois, nullptr, argmax, grad_in, B, C, H, W, K, P, spatial_scale, scratch, stream);
}

extern "C" int cim_roi_pool_maskcat_bwd(const float* grad_cat, const float* rois, const float* masks, const int* argmax,
                                        float* grad_in, int B, int C, int H, int W, int K, int P, float spatial_scale, float* scratch,
                                        void* stream) {
    return pool_bwd<true>(__func__, grad_cat, rois, masks, argmax, grad_in, B, C, H, W, K, P, spatial_scale, scratch, stream);
}
#undef POOL_CHECK_DIMS
#undef POOL_CHECK_ARG
