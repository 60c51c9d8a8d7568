// The PRM classification training head for gfx950: class response maps -> aggregated class scores -> loss, and back.
//
// Replaces the torch composition of lib/prm/prm_model.py for training: F.upsample(scale_factor, 'bilinear', align_corners=True),
// the median filter, PeakStimulation forward / backward (lib/prm/prm_modules.py:9-51) and F.multilabel_soft_margin_loss.  That
// composition writes B C up-sampled maps, pads, pools, sorts and masks them, and scatters a dense gradient of the same size
// back; what moves here is an h x w map in and an h x w gradient out per (image, class).  Exactness contract: DESIGN.md 4.21.
//
// One 256-thread workgroup per (image, class) map, for ALL B C maps.  VALU / LDS work, no MFMA, no scratch, no float atomics:
// every sum runs in a fixed order (lane partials in ascending pixel order, then the halving tree of block_tree_sum).
#include "common.h"
#include "prm_select.h"
#include "../../include/cim_hip.h"

namespace {

using cim::PRM_THREADS;

constexpr unsigned QUIET_NAN = 0x7fc00000u;
constexpr int MAX_MAPS = 1 << 24;

// red[t] += red[t + s] for s = 128, 64 .. 1: the order tests/golden/prm_train_np.py repeats.  Returns red[0] to every thread.
#pragma clang fp contract(off)
__device__ __forceinline__ float block_tree_sum(float* red, float mine) {
    const int tid = threadIdx.x;
    red[tid] = mine;
    __syncthreads();
    for (int s = PRM_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float total = red[0];
    __syncthreads();
    return total;
}

// One axis of the bilinear up-sampling, align_corners = True: the arithmetic of prm_upsample_kernel (prm.hip).
struct Tap {
    int i0, i1;
    float l0, l1;
};
#pragma clang fp contract(off)
__device__ __forceinline__ Tap tap_of(float scale, int o, int n_in) {
    Tap t;
    const float f = scale * (float)o;
    t.i0 = min((int)f, n_in - 1);
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = f - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// ---- forward: up-sample into LDS, median, peak test, bitmap, aggregation ---------------------------------------------------
#pragma clang fp contract(off)
__global__ __launch_bounds__(PRM_THREADS) void prm_stim_fwd_kernel(const float* __restrict__ crm, const float* __restrict__ bias, int C,
                                                                   int h, int w, int H, int W, float sy, float sx,
                                                                   float* __restrict__ agg, int32_t* __restrict__ count,
                                                                   float* __restrict__ median, int32_t* __restrict__ status,
                                                                   uint32_t* __restrict__ bitmap) {
    extern __shared__ __attribute__((aligned(16))) float s_map[];         // [H W]: the up-sampled map
    __shared__ int hist[256];
    __shared__ float s_red[PRM_THREADS];
    __shared__ int s_sel[2], s_nan, s_cnt[PRM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.x, n = H * W, words = (n + 31) >> 5;
    const float* __restrict__ src = crm + (size_t)m * h * w;
    const bool has_bias = bias != nullptr;
    const float bc = has_bias ? bias[m % C] : 0.0f;
    if (tid == 0) s_nan = 0;

    for (int i = tid; i < n; i += PRM_THREADS) {
        const int oy = i / W, ox = i % W;
        const Tap ty = tap_of(sy, oy, h), tx = tap_of(sx, ox, w);
        float v00 = src[ty.i0 * w + tx.i0], v01 = src[ty.i0 * w + tx.i1], v10 = src[ty.i1 * w + tx.i0], v11 = src[ty.i1 * w + tx.i1];
        if (has_bias) {
            v00 = v00 + bc;
            v01 = v01 + bc;
            v10 = v10 + bc;
            v11 = v11 + bc;
        }
        const float top = v00 * tx.l0 + v01 * tx.l1;
        const float bot = v10 * tx.l0 + v11 * tx.l1;
        s_map[i] = top * ty.l0 + bot * ty.l1;
    }
    __syncthreads();

    unsigned med_bits = cim::prm_lower_median_bits(reinterpret_cast<const unsigned*>(s_map), n, hist, s_sel, &s_nan);
    const bool has_nan = s_nan != 0;                                      // (behind the select's last barrier)
    if (has_nan) med_bits = QUIET_NAN;
    const float med = __uint_as_float(med_bits);

    // peaks in row-major order: a wave's ballot is two bitmap words; the lane's partial sum takes its pixels in ascending order
    uint32_t* __restrict__ out = bitmap + (size_t)m * words;
    float part = 0.0f;
    int mine = 0;
    for (int base = 0; base < n; base += PRM_THREADS) {
        const int i = base + tid;
        bool pk = false;
        float v = 0.0f;
        if (i < n && !has_nan) {
            v = s_map[i];
            pk = cim::prm_is_peak(s_map, H, W, i / W, i % W, v, med);
        }
        if (pk) {
            part = part + v;
            ++mine;
        }
        const unsigned long long b = __ballot(pk);
        const int word = (base + wave * 64) >> 5;
        if (lane == 0 && word < words) out[word] = (uint32_t)b;
        if (lane == 32 && word + 1 < words) out[word + 1] = (uint32_t)(b >> 32);
    }
    const float total = block_tree_sum(s_red, part);
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_down(mine, off, 64);      // (integers: any order)
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        int cnt = 0;
        for (int q = 0; q < PRM_THREADS / 64; ++q) cnt += s_cnt[q];
        count[m] = cnt;
        median[m] = med;
        agg[m] = cnt > 0 ? total / (float)cnt : __uint_as_float(QUIET_NAN);
        status[m] = has_nan ? CIM_PRM_STATUS_NAN : (cnt == 0 ? CIM_PRM_STATUS_NO_PEAK : 0);
    }
}

// ---- backward: each low-resolution pixel gathers the peaks of its support, in row-major order --------------------------------
// The up-sampled rows whose taps can land on row p: a superset by one row each side of the real-arithmetic bounds
// (p - 1) / s <= o < (p + 1) / s, s = (n_in - 1) / (n_out - 1); the exact test is the forward's own tap arithmetic.
__device__ __forceinline__ void support_of(int p, int n_in, int n_out, int& lo, int& hi) {
    if (n_in <= 1 || n_out <= 1) {
        lo = 0;
        hi = n_out - 1;
        return;
    }
    const long long d = n_in - 1, e = n_out - 1;
    lo = p >= 1 ? max(0, (int)(((long long)(p - 1) * e) / d) - 1) : 0;
    hi = min(n_out - 1, (int)(((long long)(p + 1) * e + d - 1) / d) + 1);
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(PRM_THREADS) void prm_stim_bwd_kernel(const float* __restrict__ grad_agg, const int32_t* __restrict__ count,
                                                                   const uint32_t* __restrict__ bitmap, int h, int w, int H, int W,
                                                                   float sy, float sx, float* __restrict__ dcrm) {
    __shared__ uint32_t s_bits[CIM_PRM_STIM_MAX_HW / 32];
    const int tid = threadIdx.x, m = blockIdx.x, n = H * W, words = (n + 31) >> 5;
    const int cnt = count[m];
    float* __restrict__ dst = dcrm + (size_t)m * h * w;
    if (cnt <= 0) {                                                       // (uniform) no peak: no gradient
        for (int j = tid; j < h * w; j += PRM_THREADS) dst[j] = 0.0f;
        return;
    }
    for (int q = tid; q < words; q += PRM_THREADS) s_bits[q] = bitmap[(size_t)m * words + q];
    __syncthreads();
    const float gn = grad_agg[m] / (float)cnt;
    for (int j = tid; j < h * w; j += PRM_THREADS) {
        const int py = j / w, px = j % w;
        int ylo, yhi, xlo, xhi;
        support_of(py, h, H, ylo, yhi);
        support_of(px, w, W, xlo, xhi);
        float acc = 0.0f;
        for (int oy = ylo; oy <= yhi; ++oy) {
            const Tap ty = tap_of(sy, oy, h);
            const bool y0 = ty.i0 == py, y1 = ty.i1 == py;
            if (!(y0 || y1)) continue;
            for (int ox = xlo; ox <= xhi; ++ox) {
                const int p = oy * W + ox;
                if (!((s_bits[p >> 5] >> (p & 31)) & 1u)) continue;
                const Tap tx = tap_of(sx, ox, w);
                const bool x0 = tx.i0 == px, x1 = tx.i1 == px;
                if (y0 && x0) acc = acc + (ty.l0 * tx.l0) * gn;
                if (y0 && x1) acc = acc + (ty.l0 * tx.l1) * gn;
                if (y1 && x0) acc = acc + (ty.l1 * tx.l0) * gn;
                if (y1 && x1) acc = acc + (ty.l1 * tx.l1) * gn;
            }
        }
        dst[j] = acc;
    }
}

// dbias[c] = the sum of dcrm[b, c, :, :] over b and the map: lane t takes the elements t, t + 256, .. of the class's
// [B][h w] values in that order, then the tree.
#pragma clang fp contract(off)
__global__ __launch_bounds__(PRM_THREADS) void prm_stim_dbias_kernel(const float* __restrict__ dcrm, int B, int C, int hw,
                                                                     float* __restrict__ dbias) {
    __shared__ float s_red[PRM_THREADS];
    const int c = blockIdx.x;
    const long long total = (long long)B * hw;
    float part = 0.0f;
    for (long long i = threadIdx.x; i < total; i += PRM_THREADS) {
        const long long b = i / hw, j = i % hw;
        part = part + dcrm[((size_t)b * C + c) * hw + j];
    }
    const float sum = block_tree_sum(s_red, part);
    if (threadIdx.x == 0) dbias[c] = sum;
}

// ---- multilabel soft margin loss -------------------------------------------------------------------------------------------
// exp(-a) for a >= 0 and log1p(u) for 0 <= u <= 1 from fp32 multiplies, adds and one divide, so that the NumPy restatement
// repeats them bit for bit (a library expf / log1pf is not reproducible off the device).  Errors: DESIGN.md 4.21.
#pragma clang fp contract(off)
__device__ __forceinline__ float exp_neg(float a) {
    if (a > 80.0f) return 0.0f;                                           // exp(-80) = 1.8e-35: nothing next to 1
    const float k = rintf(a * __uint_as_float(0x3fb8aa3bu));              // a log2(e), round half to even
    float r = a - k * __uint_as_float(0x3f317200u);                       // ln 2, high part (15 significant bits: the product is exact)
    r = r - k * __uint_as_float(0x35bfbe8eu);                             // ln 2, low part
    const float s = -r;                                                   // |s| <= 0.3466
    float p = 1.0f / 5040.0f;
    p = p * s + 1.0f / 720.0f;
    p = p * s + 1.0f / 120.0f;
    p = p * s + 1.0f / 24.0f;
    p = p * s + 1.0f / 6.0f;
    p = p * s + 0.5f;
    p = p * s + 1.0f;
    p = p * s + 1.0f;
    return p * __uint_as_float((unsigned)(127 - (int)k) << 23);           // 2^-k exactly
}

#pragma clang fp contract(off)
__device__ __forceinline__ float log1p_unit(float u) {
    const float z = u / (2.0f + u);                                       // log(1 + u) = 2 atanh(z), z <= 1 / 3
    const float t = z * z;
    float q = 1.0f / 17.0f;
    q = q * t + 1.0f / 15.0f;
    q = q * t + 1.0f / 13.0f;
    q = q * t + 1.0f / 11.0f;
    q = q * t + 1.0f / 9.0f;
    q = q * t + 1.0f / 7.0f;
    q = q * t + 1.0f / 5.0f;
    q = q * t + 1.0f / 3.0f;
    q = q * t + 1.0f;
    return (2.0f * z) * q;
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(PRM_THREADS) void prm_msm_loss_kernel(const float* __restrict__ x, const float* __restrict__ target, int n,
                                                                   float* __restrict__ loss, float* __restrict__ dagg) {
    __shared__ float s_red[PRM_THREADS];
    const float fn = (float)n;
    float part = 0.0f;
    for (int i = threadIdx.x; i < n; i += PRM_THREADS) {
        const float v = x[i], t = target[i];
        const float e = exp_neg(fabsf(v));
        const float l = log1p_unit(e);                                    // softplus(-|x|)
        const float ls_pos = fminf(v, 0.0f) - l;                          // logsigmoid(x)
        const float ls_neg = fminf(-v, 0.0f) - l;                         // logsigmoid(-x)
        part = part + (-(t * ls_pos + (1.0f - t) * ls_neg));
        const float sig = (v >= 0.0f ? 1.0f : e) / (1.0f + e);
        dagg[i] = (sig - t) / fn;
    }
    const float sum = block_tree_sum(s_red, part);
    if (threadIdx.x == 0) loss[0] = sum / fn;
}

bool shape_ok(const char* who, int B, int C, int h, int w, int factor) {
    if (B < 1 || C < 1 || h < 1 || w < 1 || factor < 1) {
        cim::set_error("%s: bad argument: B >= 1 && C >= 1 && h >= 1 && w >= 1 && factor >= 1 (B %d, C %d, h %d, w %d, factor %d)", who, B, C,
                       h, w, factor);
        return false;
    }
    if ((long long)B * C > MAX_MAPS) {
        cim::set_error("%s: %lld maps, at most %d", who, (long long)B * C, MAX_MAPS);
        return false;
    }
    const long long H = (long long)h * factor, W = (long long)w * factor;
    if (H * W > CIM_PRM_STIM_MAX_HW) {
        cim::set_error("%s: an up-sampled map of %lld x %lld pixels, more than CIM_PRM_STIM_MAX_HW = %d (it lives in LDS)", who, H, W,
                       CIM_PRM_STIM_MAX_HW);
        return false;
    }
    return true;
}

// the scales in double on the host, rounded to fp32 (0 when the output side is 1): those of cim_prm_upsample
float scale_of(int n_in, int n_out) { return n_out > 1 ? (float)((double)(n_in - 1) / (double)(n_out - 1)) : 0.0f; }

}  // namespace

extern "C" int cim_prmt_stim_forward(const float* crm, const float* bias, int B, int C, int h, int w, int factor, float* agg,
                                     int32_t* count, float* median, int32_t* status, uint32_t* bitmap, void* stream) {
    if (!shape_ok(__func__, B, C, h, w, factor)) return -1;
    CIM_CHECK_ARG(crm && agg && count && median && status && bitmap);
    const int H = h * factor, W = w * factor;
    const size_t lds = (size_t)H * W * sizeof(float);
    if (lds > 60 * 1024)                                                  // (beside ~2.1 KiB of static LDS)
        CIM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(prm_stim_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
    hipLaunchKernelGGL(prm_stim_fwd_kernel, dim3(B * C), dim3(PRM_THREADS), lds, cim::as_stream(stream), crm, bias, C, h, w, H, W,
                       scale_of(h, H), scale_of(w, W), agg, count, median, status, bitmap);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prmt_stim_backward(const float* grad_agg, const int32_t* count, const uint32_t* bitmap, int B, int C, int h, int w,
                                      int factor, float* dcrm, float* dbias, void* stream) {
    if (!shape_ok(__func__, B, C, h, w, factor)) return -1;
    CIM_CHECK_ARG(grad_agg && count && bitmap && dcrm);
    const int H = h * factor, W = w * factor;
    hipStream_t st = cim::as_stream(stream);
    hipLaunchKernelGGL(prm_stim_bwd_kernel, dim3(B * C), dim3(PRM_THREADS), 0, st, grad_agg, count, bitmap, h, w, H, W, scale_of(h, H),
                       scale_of(w, W), dcrm);
    if (dbias != nullptr) hipLaunchKernelGGL(prm_stim_dbias_kernel, dim3(C), dim3(PRM_THREADS), 0, st, dcrm, B, C, h * w, dbias);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prmt_msm_loss(const float* agg, const float* target, int B, int C, float* loss, float* dagg, void* stream) {
    CIM_CHECK_ARG(B >= 1 && C >= 1 && (long long)B * C <= MAX_MAPS);
    CIM_CHECK_ARG(agg && target && loss && dagg);
    hipLaunchKernelGGL(prm_msm_loss_kernel, dim3(1), dim3(PRM_THREADS), 0, cim::as_stream(stream), agg, target, B * C, loss, dagg);
    CIM_CHECK_LAUNCH();
    return 0;
}
