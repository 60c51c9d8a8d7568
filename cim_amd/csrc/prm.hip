// PRM peaks for gfx950: class response maps -> the points the cluster assignment takes (proposal_prep.hip).
//
// Replaces what tools/pre/AGPL_label_assign.py:136-161 reads from PeakResponseMapping.forward (lib/prm/prm_model_gt.py:216-310):
// F.upsample(scale_factor, 'bilinear', align_corners=True), PeakStimulation.forward (lib/prm/prm_modules.py:9-44: -inf padding,
// max_pool2d(3, 1, return_indices) == own index, value >= torch.median), the selection value > peak_threshold with its arg-max
// fallback, and the ascending argsort of the scores.  Exactness contract: DESIGN.md 4.19.
//
// Work is described by PAIRS (image, class): only the image-level classes of an image are processed (the reference computes
// all C maps and reads those in `lables`).  Three launches for a batch: up-sampling (one lane per output pixel), peaks (one
// workgroup per pair), order (one workgroup per image).  VALU / LDS work, no MFMA, no scratch.
#include "common.h"
#include "prm_select.h"
#include "../../include/cim_hip.h"

namespace {

using cim::PRM_THREADS;
using cim::prm_key;

struct PeakEntry {
    int32_t pix;                                  // y * W + x on the up-sampled grid
    float val;
};

// ---- (a) bilinear up-sampling, align_corners = True --------------------------------------------------------------------------
// Every operation rounded to fp32, no contraction: the NumPy restatement (tests/golden/prm_np.py) repeats exactly these.
#pragma clang fp contract(off)
__global__ __launch_bounds__(PRM_THREADS) void prm_upsample_kernel(const float* __restrict__ crm, const float* __restrict__ bias,
                                                                   const int32_t* __restrict__ desc, int M, int C, int h, int w,
                                                                   int H, int W, float sy, float sx, float* __restrict__ up) {
    const long long idx = (long long)blockIdx.x * PRM_THREADS + threadIdx.x;
    const long long HW = (long long)H * W;
    if (idx >= (long long)M * HW) return;
    const int m = (int)(idx / HW), p = (int)(idx % HW);
    const int oy = p / W, ox = p % W;
    const int b = desc[m], c = desc[M + m];
    const float* __restrict__ src = crm + ((size_t)b * C + c) * h * w;
    const float fy = sy * (float)oy, fx = sx * (float)ox;
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float l1y = fy - (float)y0, l1x = fx - (float)x0;
    const float l0y = 1.0f - l1y, l0x = 1.0f - l1x;
    float v00 = src[y0 * w + x0], v01 = src[y0 * w + x1], v10 = src[y1 * w + x0], v11 = src[y1 * w + x1];
    if (bias != nullptr) {
        const float bc = bias[c];
        v00 = v00 + bc;
        v01 = v01 + bc;
        v10 = v10 + bc;
        v11 = v11 + bc;
    }
    const float top = v00 * l0x + v01 * l1x;
    const float bot = v10 * l0x + v11 * l1x;
    up[idx] = top * l0y + bot * l1y;
}

// ---- (b) median, peak test, ordered compaction, selection: one workgroup per pair ---------------------------------------------
// (keys, the radix select of the median and the 3 x 3 peak test: prm_select.h, shared with prm_train.hip)
__global__ __launch_bounds__(PRM_THREADS) void prm_peaks_kernel(const float* __restrict__ up, int H, int W, float thr,
                                                                float* __restrict__ median, int32_t* __restrict__ pair_counts,
                                                                PeakEntry* __restrict__ plist) {
    __shared__ int hist[256];
    __shared__ int s_sel[2], s_nan;
    __shared__ int s_pk[PRM_THREADS / 64], s_va[PRM_THREADS / 64];
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.x, n = H * W;
    const float* __restrict__ map = up + (size_t)m * n;
    const unsigned* __restrict__ bits = reinterpret_cast<const unsigned*>(map);
    PeakEntry* __restrict__ out = plist + (size_t)m * CIM_PRM_MAX_PEAKS;

    // lower median: the element of rank (n - 1) / 2, most significant byte first; the map is re-read from memory (cache-resident)
    if (tid == 0) {
        s_nan = 0;
        s_best = 0ull;
    }
    const float med = __uint_as_float(cim::prm_lower_median_bits(bits, n, hist, s_sel, &s_nan));

    // peaks in row-major order; the valid ones (value > thr) are compacted in that order (ballot + prefix)
    int nvalid = 0, npeaks = 0;
    unsigned long long best = 0ull;
    for (int base = 0; base < n; base += PRM_THREADS) {
        const int i = base + tid;
        bool pk = false, va = false;
        float v = 0.0f;
        if (i < n) {
            const int y = i / W, x = i % W;
            v = map[i];
            pk = cim::prm_is_peak(map, H, W, y, x, v, med);
            va = pk && v > thr;
            if (pk) {                                                     // arg-max of the peak values: the first of the largest
                unsigned u = __float_as_uint(v);
                if (u == 0x80000000u) u = 0u;                             // -0.0 == +0.0 in the float compare of argmax
                const unsigned long long cand = ((unsigned long long)prm_key(u) << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
                best = cand > best ? cand : best;
            }
        }
        const unsigned long long bp = __ballot(pk), bv = __ballot(va);
        if (lane == 0) {
            s_pk[wave] = __popcll(bp);
            s_va[wave] = __popcll(bv);
        }
        __syncthreads();
        int before = 0, totv = 0, totp = 0;
#pragma unroll
        for (int q = 0; q < PRM_THREADS / 64; ++q) {
            const int c = s_va[q];
            before += q < wave ? c : 0;
            totv += c;
            totp += s_pk[q];
        }
        if (va) {
            const int pos = nvalid + before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bv >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bv, 0u));
            if (pos < CIM_PRM_MAX_PEAKS) {
                out[pos].pix = i;
                out[pos].val = v;
            }
        }
        nvalid += totv;
        npeaks += totp;
        __syncthreads();
    }
    if (best != 0ull) atomicMax(&s_best, best);
    __syncthreads();
    if (tid == 0) {
        int flags = s_nan ? CIM_PRM_STATUS_NAN : 0;
        if (nvalid == 0) {
            if (npeaks > 0) {                                             // prm_model_gt.py:278-298: no peak above the threshold
                const int i = (int)(0xffffffffu - (unsigned)(s_best & 0xffffffffull));
                out[0].pix = i;
                out[0].val = map[i];
                nvalid = 1;
            } else if (!s_nan) {
                flags |= CIM_PRM_STATUS_NO_PEAK;
            }
        }
        median[m] = med;
        pair_counts[3 * m + 0] = npeaks;
        pair_counts[3 * m + 1] = nvalid;
        pair_counts[3 * m + 2] = flags;
    }
}

// ---- (c) per image: concatenate the pairs' lists, order ascending by score (stable), scale to image pixels --------------------
__global__ __launch_bounds__(PRM_THREADS) void prm_order_kernel(const int32_t* __restrict__ desc, int M, int B, int H, int W,
                                                                const int32_t* __restrict__ pair_counts, const PeakEntry* __restrict__ plist,
                                                                int32_t* __restrict__ points, float* __restrict__ scores,
                                                                int32_t* __restrict__ image_out) {
    __shared__ int s_first, s_n;
    __shared__ float s_score[CIM_PRM_MAX_PEAKS];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid == 0) {
        s_first = M;
        s_n = 0;
    }
    __syncthreads();
    for (int m = tid; m < M; m += PRM_THREADS)
        if (desc[m] == b) {
            atomicMin(&s_first, m);
            atomicAdd(&s_n, 1);
        }
    __syncthreads();
    const int p0 = s_first, np = s_n;
    long long total = 0;
    int status = 0;
    for (int q = 0; q < np; ++q) {
        total += pair_counts[3 * (p0 + q) + 1];
        status |= pair_counts[3 * (p0 + q) + 2];
    }
    if (total > CIM_PRM_MAX_PEAKS) status |= CIM_PRM_STATUS_TOO_MANY;
    if (tid == 0) {
        image_out[2 * b + 0] = (int32_t)(total > 0x7fffffffll ? 0x7fffffffll : total);
        image_out[2 * b + 1] = status;
    }
    if (status != 0) return;                                              // (uniform: every thread computed the same words)
    const int T = (int)total;
    PeakEntry e = {0, 0.0f};
    int cls = 0;
    if (tid < T) {
        int off = 0, q = 0;
        for (; q < np; ++q) {
            const int c = pair_counts[3 * (p0 + q) + 1];
            if (tid < off + c) break;
            off += c;
        }
        e = plist[(size_t)(p0 + q) * CIM_PRM_MAX_PEAKS + (tid - off)];
        cls = desc[M + p0 + q];
        s_score[tid] = e.val;
    }
    __syncthreads();
    if (tid < T) {
        int rank = 0;
        for (int j = 0; j < T; ++j) {
            const float s = s_score[j];
            rank += (s < e.val || (s == e.val && j < tid)) ? 1 : 0;
        }
        const int y = e.pix / W, x = e.pix % W;
        const int img_h = desc[2 * M + b], img_w = desc[2 * M + B + b];
        int32_t* pt = points + ((size_t)b * CIM_PRM_MAX_PEAKS + rank) * 5;
        pt[0] = (int32_t)((long long)y * img_h / H);                      // == int(y * img_h / H) in float64 (tests/test_prm_cpu.py)
        pt[1] = (int32_t)((long long)x * img_w / W);
        pt[2] = cls;
        pt[3] = y;
        pt[4] = x;
        scores[(size_t)b * CIM_PRM_MAX_PEAKS + rank] = e.val;
    }
}

size_t plist_bytes(int M) { return (size_t)M * CIM_PRM_MAX_PEAKS * sizeof(PeakEntry); }

// desc_host: pair image [M] | pair class [M] | image height [B] | image width [B]
bool desc_ok(const int32_t* d, int M, int B, int C) {
    for (int m = 0; m < M; ++m) {
        if (d[m] < 0 || d[m] >= B || (m > 0 && d[m] < d[m - 1])) {
            cim::set_error("cim_prm: pair %d names image %d: indices must be ascending and inside 0..%d", m, d[m], B - 1);
            return false;
        }
        if (d[M + m] < 0 || d[M + m] >= C) {
            cim::set_error("cim_prm: pair %d names class %d, outside 0..%d", m, d[M + m], C - 1);
            return false;
        }
    }
    for (int b = 0; b < 2 * B; ++b)
        if (d[2 * M + b] < 1 || d[2 * M + b] > 65535) {
            cim::set_error("cim_prm: image %d has a side of %d pixels, outside 1..65535", b % B, d[2 * M + b]);
            return false;
        }
    return true;
}

#define PRM_CHECK_PAIRS()                                                                                  \
    CIM_CHECK_ARG(M >= 1 && B >= 1 && C >= 1 && desc_host && desc_dev);                                  \
    if (!desc_ok(desc_host, M, B, C)) return -1

int launch_upsample(const float* crm, const float* bias, int C, int h, int w, int factor, int M, const int32_t* desc_dev, float* up,
                    hipStream_t st) {
    const int H = h * factor, W = w * factor;
    // the scales in double on the host, rounded to fp32 (0 when the output side is 1)
    const float sy = H > 1 ? (float)((double)(h - 1) / (double)(H - 1)) : 0.0f;
    const float sx = W > 1 ? (float)((double)(w - 1) / (double)(W - 1)) : 0.0f;
    const long long total = (long long)M * H * W;
    hipLaunchKernelGGL(prm_upsample_kernel, dim3((unsigned)((total + PRM_THREADS - 1) / PRM_THREADS)), dim3(PRM_THREADS), 0, st, crm, bias,
                       desc_dev, M, C, h, w, H, W, sy, sx, up);
    return 0;
}

void launch_peaks(const float* up, int M, int H, int W, int B, const int32_t* desc_dev, float thr, float* median, int32_t* pair_counts,
                  int32_t* points, float* scores, int32_t* image_out, void* ws, hipStream_t st) {
    PeakEntry* plist = static_cast<PeakEntry*>(ws);
    hipLaunchKernelGGL(prm_peaks_kernel, dim3(M), dim3(PRM_THREADS), 0, st, up, H, W, thr, median, pair_counts, plist);
    hipLaunchKernelGGL(prm_order_kernel, dim3(B), dim3(PRM_THREADS), 0, st, desc_dev, M, B, H, W, pair_counts, plist, points, scores,
                       image_out);
}

bool map_ok(int M, long long H, long long W) {
    return H >= 1 && W >= 1 && H * W <= CIM_PRM_MAX_HW && (long long)M * H * W < (1ll << 31) * PRM_THREADS / 2;
}

}  // namespace

extern "C" long long cim_prm_ws_bytes(int M, int HW) {
    CIM_CHECK_ARG(M >= 1 && HW >= 0 && HW <= CIM_PRM_MAX_HW);
    return (long long)(plist_bytes(M) + (size_t)M * HW * sizeof(float));
}

extern "C" int cim_prm_upsample(const float* crm, const float* bias, int B, int C, int h, int w, int factor, int M,
                                const int32_t* desc_host, const int32_t* desc_dev, float* up, void* stream) {
    PRM_CHECK_PAIRS();
    CIM_CHECK_ARG(factor >= 1 && h >= 1 && w >= 1 && map_ok(M, (long long)h * factor, (long long)w * factor));
    CIM_CHECK_ARG(crm && up);
    launch_upsample(crm, bias, C, h, w, factor, M, desc_dev, up, cim::as_stream(stream));
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prm_peaks(const float* up, int M, int H, int W, int B, int C, const int32_t* desc_host, const int32_t* desc_dev,
                             float peak_threshold, float* median, int32_t* pair_counts, int32_t* points, float* scores,
                             int32_t* image_out, void* ws, void* stream) {
    PRM_CHECK_PAIRS();
    CIM_CHECK_ARG(map_ok(M, H, W));
    CIM_CHECK_ARG(up && median && pair_counts && points && scores && image_out && ws);
    launch_peaks(up, M, H, W, B, desc_dev, peak_threshold, median, pair_counts, points, scores, image_out, ws, cim::as_stream(stream));
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prm_points(const float* crm, const float* bias, int B, int C, int h, int w, int factor, int M,
                              const int32_t* desc_host, const int32_t* desc_dev, float peak_threshold, float* median,
                              int32_t* pair_counts, int32_t* points, float* scores, int32_t* image_out, void* ws, void* stream) {
    PRM_CHECK_PAIRS();
    CIM_CHECK_ARG(factor >= 1 && h >= 1 && w >= 1 && map_ok(M, (long long)h * factor, (long long)w * factor));
    CIM_CHECK_ARG(crm && median && pair_counts && points && scores && image_out && ws);
    const int H = h * factor, W = w * factor;
    hipStream_t st = cim::as_stream(stream);
    float* up = reinterpret_cast<float*>(static_cast<char*>(ws) + plist_bytes(M));
    launch_upsample(crm, bias, C, h, w, factor, M, desc_dev, up, st);
    launch_peaks(up, M, H, W, B, desc_dev, peak_threshold, median, pair_counts, points, scores, image_out, ws, st);
    CIM_CHECK_LAUNCH();
    return 0;
}
