// Detection post-processing for gfx950: per-class score threshold + greedy box NMS + the per-image detection limit over
// all classes, and the per-class argmax of CorLoc - the last inference stage, on the scores the forward left on the device.
//
// Replaces box_results_with_nms_and_limit / box_results_for_corloc (lib/core/test.py:320-420),
// mask_results_with_nms_and_limit{,_get_index} (lib/utils/mask_eval_utils.py:6-108) and the compiled greedy NMS they call
// (lib/utils/cython_nms.pyx:36-87).  Results are indices and copies of input scores, bit-identical to the reference
// (exactness contract and tie rule: DESIGN.md 4.11, include/cim_hip.h).
//
// Three launches per image, no host round trip:
//   detect_overlap_kernel   the N x ceil(N/64) u64 overlap matrix, bit (i, j) = ovr(i, j) >= nms_thr with box i in the
//                           pyx's suppressor role; one 64 x 64 tile per wave, the 64 column boxes staged in LDS.  It does
//                           not depend on the class, so every class shares it.
//   detect_nms_kernel       one workgroup per class: candidates s > score_thr (ballot + one LDS atomic per wave), a bitonic
//                           sort of the 64-bit keys (orderable score << 32 | proposal) in LDS, then ONE wave runs the greedy
//                           pass 64 sorted candidates at a time: drop those in the class's `removed` mask (proposal-index
//                           space, two words per lane in registers), resolve the chunk's own conflicts in registers from
//                           the boxes, OR the matrix rows of the chunk's kept boxes into `removed`.
//   detect_limit_kernel     one workgroup: compacts the kept bits in (class, proposal) order, finds the D-th largest kept
//                           score by a radix select on the score bits, writes the records that reach it.
#pragma clang fp contract(off)                      // (x2 - x1 + 1) * ... and iarea + area - w*h: no fused multiply-adds
#include "common.h"
#include "../../include/cim_hip.h"
#include <limits.h>

namespace {

constexpr int kMaxN = CIM_DETECT_MAX_N;

// the greedy pass compares scores as unsigned integers: IEEE order for every non-NaN float, -0 == +0 (NumPy's sort)
__device__ __forceinline__ uint32_t orderable(float f) {
    if (f == 0.0f) f = 0.0f;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ int block_exclusive_scan(int v, int* part, int* total) {      // 1024 lanes; returns the exclusive prefix
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    __syncthreads();                                                     // (part[] of the previous scan has been read)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int p = part[w];
        tot += p;
        woff += (w < wave) ? p : 0;
    }
    *total = tot;
    return woff + incl - v;
}

// cython_nms.pyx:28-32 - the ternaries, not fmaxf / fminf (they differ on NaN)
__device__ __forceinline__ float pyx_max(float a, float b) { return a >= b ? a : b; }
__device__ __forceinline__ float pyx_min(float a, float b) { return a <= b ? a : b; }

// lib/utils/cython_nms.pyx:45 (NumPy fp32, elementwise)
__device__ __forceinline__ float box_area(float4 b) { return (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f); }

// cython_nms.pyx:74-84 operation for operation in fp32: box i is the kept (higher-ranked) one, j the candidate
__device__ __forceinline__ bool overlaps(float4 bi, float ai, float4 bj, float aj, float thr) {
    const float xx1 = pyx_max(bi.x, bj.x);
    const float yy1 = pyx_max(bi.y, bj.y);
    const float xx2 = pyx_min(bi.z, bj.z);
    const float yy2 = pyx_min(bi.w, bj.w);
    const float w = pyx_max(0.0f, xx2 - xx1 + 1.0f);
    const float h = pyx_max(0.0f, yy2 - yy1 + 1.0f);
    const float inter = w * h;
    const float ovr = inter / (ai + aj - inter);                        // correctly rounded fp32 division (no fast-math)
    return ovr >= thr;
}

__global__ __launch_bounds__(64) void detect_overlap_kernel(const float4* __restrict__ boxes, int N, int W, float thr,
                                                            unsigned long long* __restrict__ mat) {
    __shared__ float4 s_box[64];
    __shared__ float s_area[64];
    const int lane = threadIdx.x, jb = blockIdx.x;
    const int j = jb * 64 + lane, i = blockIdx.y * 64 + lane;
    if (j < N) {
        const float4 b = boxes[j];
        s_box[lane] = b;
        s_area[lane] = box_area(b);
    }
    __syncthreads();
    if (i >= N) return;
    const float4 bi = boxes[i];
    const float ai = box_area(bi);
    const int n = min(64, N - jb * 64);
    unsigned long long bits = 0;
    for (int t = 0; t < n; ++t)
        if (overlaps(bi, ai, s_box[t], s_area[t], thr)) bits |= 1ull << t;
    mat[(size_t)i * W + jb] = bits;
}

// keys: (orderable(score) << 32) | proposal, sorted descending = score descending, then HIGHER proposal index first
// (np.argsort(s, kind="stable")[::-1]); 0 pads the sort (no candidate key is 0: candidates are never NaN)
__global__ __launch_bounds__(1024) void detect_nms_kernel(const float* __restrict__ scores, int ld,
                                                          const float4* __restrict__ boxes, int N, int W, float score_thr,
                                                          float nms_thr, const unsigned long long* __restrict__ mat,
                                                          unsigned long long* __restrict__ keepbits) {
    extern __shared__ unsigned long long s_key[];                      // [pow2ceil(N)]
    __shared__ int s_cnt;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    // test.py:370 / mask_eval_utils.py:62: s > float32(SCORE_THRESH); the order of insertion does not matter (keys are unique)
    for (int base = 0; base < N; base += 1024) {
        const int p = base + tid;
        const float s = p < N ? scores[(size_t)p * ld + c] : 0.0f;
        const bool cand = p < N && s > score_thr;
        const unsigned long long b = __ballot(cand);
        int at = 0;
        if (lane == 0 && b) at = atomicAdd(&s_cnt, (int)__popcll(b));
        at = __shfl(at, 0);
        if (cand) s_key[at + __popcll(b & ((1ull << lane) - 1))] = ((unsigned long long)orderable(s) << 32) | (unsigned)p;
    }
    __syncthreads();
    const int cnt = s_cnt;
    int P = 1;
    while (P < cnt) P <<= 1;
    for (int i = cnt + tid; i < P; i += 1024) s_key[i] = 0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {                                 // bitonic sort, descending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 1024) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = s_key[i], b = s_key[ixj];
                    if (((i & k) == 0) ? (a < b) : (a > b)) {
                        s_key[i] = b;
                        s_key[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid >= 64) return;                                             // (no barrier below: one wave finishes the class)

    // greedy pass (cython_nms.pyx:62-85), 64 sorted candidates at a time.  removed / kept: bit p of word q = p >> 6 lives
    // in lane q & 63, register q >> 6
    unsigned long long rem0 = 0, rem1 = 0, kb0 = 0, kb1 = 0;
    for (int b0 = 0; b0 < cnt; b0 += 64) {
        const int q = b0 + lane;
        const bool valid = q < cnt;
        const int p = valid ? (int)(unsigned)s_key[q] : 0;
        const int wq = p >> 6;
        const unsigned long long r0 = __shfl(rem0, wq & 63), r1 = __shfl(rem1, wq & 63);
        bool alive = valid && !((((wq >> 6) ? r1 : r0) >> (p & 63)) & 1ull);
        const float4 bx = boxes[p];
        const float ar = box_area(bx);
        // (b) conflicts inside the chunk: the first alive lane is kept, the later ones it overlaps drop out
        unsigned long long kept = 0, al = __ballot(alive);
        while (al) {
            const int m = __builtin_ctzll(al);
            kept |= 1ull << m;
            const float4 bm = make_float4(__shfl(bx.x, m), __shfl(bx.y, m), __shfl(bx.z, m), __shfl(bx.w, m));
            const float am = __shfl(ar, m);
            if (alive && lane > m && overlaps(bm, am, bx, ar, nms_thr)) alive = false;
            al = __ballot(alive) & ~((2ull << m) - 1);
        }
        // (c) the kept boxes' matrix rows: independent loads, all in flight at once
        const bool more = b0 + 64 < cnt;
        while (kept) {
            const int m = __builtin_ctzll(kept);
            kept &= kept - 1;
            const int pm = __shfl(p, m);
            const int wm = pm >> 6;
            if (lane == (wm & 63)) {
                if (wm >> 6) kb1 |= 1ull << (pm & 63);
                else kb0 |= 1ull << (pm & 63);
            }
            if (more) {
                const unsigned long long* row = mat + (size_t)pm * W;
                if (lane < W) rem0 |= row[lane];
                if (lane + 64 < W) rem1 |= row[lane + 64];
            }
        }
    }
    unsigned long long* kc = keepbits + (size_t)c * W;
    if (lane < W) kc[lane] = kb0;
    if (lane + 64 < W) kc[lane + 64] = kb1;
}

// test.py:395-403: the kept set in (class, proposal) order, thresholded at the max_det-th largest kept score when more
// than max_det are kept.  det records: (proposal, class, score bits)
__global__ __launch_bounds__(1024) void detect_limit_kernel(const float* __restrict__ scores, int ld, int C, int W,
                                                            int max_det, const unsigned long long* __restrict__ keepbits,
                                                            uint32_t* __restrict__ lkey, int* __restrict__ lidx,
                                                            int* __restrict__ lcls, int* __restrict__ det,
                                                            int* __restrict__ count, int* __restrict__ total) {
    __shared__ int s_part[16];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_prefix, s_k;
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 1024) count[c] = 0;
    __threadfence();                                                   // (the zeros reach L2 before any atomic below)
    // compaction of the kept bits: word (c, w) of keepbits is the flat word c * W + w, so flat order = output order
    const int nw = C * W;
    int T = 0;
    for (int base = 0; base < nw; base += 1024) {
        const int qw = base + tid;
        unsigned long long word = qw < nw ? keepbits[qw] : 0ull;
        int tot;
        int o = T + block_exclusive_scan((int)__popcll(word), s_part, &tot);
        const int c = qw / W, p0 = (qw - c * W) * 64;
        while (word) {
            const int p = p0 + __builtin_ctzll(word);
            word &= word - 1;
            lkey[o] = orderable(scores[(size_t)p * ld + c]);
            lidx[o] = p;
            lcls[o] = c;
            ++o;
        }
        T += tot;
    }
    __syncthreads();
    // np.sort(image_scores)[-max_det]: the max_det-th largest, four 8-bit digits from the top
    uint32_t thr_key = 0;                                              // (every candidate key is > 0)
    if (max_det > 0 && T > max_det) {
        uint32_t prefix = 0, mask = 0;
        unsigned k = (unsigned)max_det;
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = tid; i < 256; i += 1024) s_hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < T; i += 1024) {
                const uint32_t key = lkey[i];
                if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned acc = 0;
                int d = 255;
                for (; d > 0; --d) {
                    if (acc + s_hist[d] >= k) break;
                    acc += s_hist[d];
                }
                s_prefix = prefix | ((uint32_t)d << shift);
                s_k = k - acc;
            }
            __syncthreads();
            prefix = s_prefix;
            k = s_k;
            mask |= 0xffu << shift;
            __syncthreads();
        }
        thr_key = prefix;
    }
    // keep score >= image_thresh (ties at the threshold all stay, as in the reference)
    int outn = 0;
    for (int base = 0; base < T; base += 1024) {
        const int i = base + tid;
        const bool on = i < T && lkey[i] >= thr_key;
        int tot;
        const int o = outn + block_exclusive_scan(on ? 1 : 0, s_part, &tot);
        if (on) {
            const int p = lidx[i], c = lcls[i];
            det[3 * (size_t)o] = p;
            det[3 * (size_t)o + 1] = c;
            det[3 * (size_t)o + 2] = __float_as_int(scores[(size_t)p * ld + c]);
            atomicAdd(count + c, 1);
        }
        outn += tot;
    }
    if (tid == 0) *total = outn;
}

// test.py:336-338: np.argmax(scores[:, j]) - the first index of the maximum, the first NaN if there is one
struct ArgMax {
    float v;
    int i;                                                              // -1: nothing seen
};
__device__ __forceinline__ bool beats(ArgMax a, ArgMax b) {             // a before b in argmax order
    if (a.i < 0) return false;
    if (b.i < 0) return true;
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an || bn) return an && bn ? a.i < b.i : an;
    if (a.v != b.v) return a.v > b.v;
    return a.i < b.i;
}

__global__ __launch_bounds__(256) void detect_corloc_kernel(const float* __restrict__ scores, int ld, int N,
                                                            int* __restrict__ out) {
    __shared__ ArgMax s_best[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    ArgMax best = {0.0f, -1};
    for (int p = tid; p < N; p += 256) {
        const ArgMax x = {scores[(size_t)p * ld + c], p};
        if (beats(x, best)) best = x;
    }
    s_best[tid] = best;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h && beats(s_best[tid + h], s_best[tid])) s_best[tid] = s_best[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        out[2 * c] = s_best[0].i;
        out[2 * c + 1] = __float_as_int(s_best[0].v);
    }
}

struct DetectLayout {
    size_t mat, keep, lkey, lidx, lcls, total;
};

DetectLayout layout(int N, int C) {
    const size_t W = (size_t)(N + 63) / 64, cap = (size_t)C * N;
    DetectLayout L;
    L.mat = 0;
    L.keep = L.mat + (size_t)N * W * 8;
    L.lkey = L.keep + (size_t)C * W * 8;
    L.lidx = L.lkey + ((cap * 4 + 255) & ~(size_t)255);
    L.lcls = L.lidx + ((cap * 4 + 255) & ~(size_t)255);
    L.total = L.lcls + ((cap * 4 + 255) & ~(size_t)255);
    return L;
}

bool shape_ok(int N, int C) {
    return N >= 1 && N <= kMaxN && C >= 1 && (long long)C * N <= (long long)(INT_MAX / 3);
}

}  // namespace

extern "C" long long cim_detect_ws_bytes(int N, int C) {
    if (!shape_ok(N, C)) {
        cim::set_error("cim_detect_ws_bytes: need 1 <= N <= %d and C >= 1 with 3 * C * N < 2^31 (N=%d, C=%d)", kMaxN, N, C);
        return -1;
    }
    return (long long)layout(N, C).total;
}

extern "C" int cim_detect_nms_limit(const float* scores, int ld, const float* boxes, int N, int C, float score_thr,
                                    float nms_thr, int max_det, void* ws, int* det, int* count_per_class, int* total,
                                    void* stream) {
    if (!shape_ok(N, C)) {
        cim::set_error("cim_detect_nms_limit: need 1 <= N <= %d and C >= 1 with 3 * C * N < 2^31 (N=%d, C=%d)", kMaxN, N, C);
        return -1;
    }
    CIM_CHECK_ARG(ld >= C);
    CIM_CHECK_ARG(scores && boxes && ws && det && count_per_class && total);
    CIM_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)ws & 7) == 0);
    hipStream_t st = cim::as_stream(stream);
    const int W = (N + 63) / 64;
    const DetectLayout L = layout(N, C);
    char* w = static_cast<char*>(ws);
    auto* mat = reinterpret_cast<unsigned long long*>(w + L.mat);
    auto* keep = reinterpret_cast<unsigned long long*>(w + L.keep);
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    hipLaunchKernelGGL(detect_overlap_kernel, dim3(W, W), dim3(64), 0, st, bx, N, W, nms_thr, mat);
    CIM_CHECK_LAUNCH();
    int P = 1;
    while (P < N) P <<= 1;
    const int lds = P * 8;
    CIM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(detect_nms_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(detect_nms_kernel, dim3(C), dim3(1024), lds, st, scores, ld, bx, N, W, score_thr, nms_thr, mat, keep);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(detect_limit_kernel, dim3(1), dim3(1024), 0, st, scores, ld, C, W, max_det, keep,
                       reinterpret_cast<uint32_t*>(w + L.lkey), reinterpret_cast<int*>(w + L.lidx),
                       reinterpret_cast<int*>(w + L.lcls), det, count_per_class, total);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_detect_corloc(const float* scores, int ld, int N, int C, int* out, void* stream) {
    if (!shape_ok(N, C)) {
        cim::set_error("cim_detect_corloc: need 1 <= N <= %d and C >= 1 (N=%d, C=%d)", kMaxN, N, C);
        return -1;
    }
    CIM_CHECK_ARG(ld >= C);
    CIM_CHECK_ARG(scores && out);
    hipLaunchKernelGGL(detect_corloc_kernel, dim3(C), dim3(256), 0, cim::as_stream(stream), scores, ld, N, out);
    CIM_CHECK_LAUNCH();
    return 0;
}
