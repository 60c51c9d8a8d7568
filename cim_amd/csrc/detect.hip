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
//
// The ragged batch form (cim_batch_detect_nms_limit) runs B images back to back in five launches: a
// one-workgroup prologue (per-image words, tile / matrix / keep offsets from row_off), the overlap tiles of all images in a
// 1-D grid (a binary search finds a tile's image), the NMS on a (C, B) grid, one limit workgroup per image, and the
// compaction of the per-image records into one array.  Each per-image body below (overlap_tile, nms_class, limit_image) is
// ONE __device__ function called by both forms with base pointers, so the exactness contract holds for both.
// Soft-NMS and box voting (TEST.SOFT_NMS / TEST.BBOX_VOTE) are at the end of the file; they share the overlap
// helpers, the block scan and the limit's radix select with the kernels above.
#pragma clang fp contract(off)                      // (x2 - x1 + 1) * ... and iarea + area - w*h: no fused multiply-adds
#include "common.h"
#include "wave_block.h"
#include "../../include/cim_hip.h"
#include <limits.h>
#include <algorithm>

namespace {

constexpr int kMaxN = CIM_DETECT_MAX_N;

// (the greedy pass compares scores as unsigned integers: orderable() of wave_block.h, which also holds the block scan)

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

// TEST.PROPOSAL_FILTER (tools/evaluation.py:108-115): the proposal's scores read as 0 when its area - no + 1, fp32 - is
// > hi or < lo (both strict; bounds = {lo, hi} of the image, null: no filter)
__device__ __forceinline__ bool filtered_out(const float4* box, const float* bounds) {
    if (!bounds) return false;
    const float4 b = *box;
    const float a = (b.z - b.x) * (b.w - b.y);
    return a > bounds[1] || a < bounds[0];
}

// one 64 x 64 tile (row block ib, column block jb) of one image's overlap matrix; one wave
__device__ __forceinline__ void overlap_tile(const float4* __restrict__ boxes, int N, int W, float thr,
                                             unsigned long long* __restrict__ mat, int jb, int ib) {
    __shared__ float4 s_box[64];
    __shared__ float s_area[64];
    const int lane = threadIdx.x;
    const int j = jb * 64 + lane, i = ib * 64 + lane;
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

__global__ __launch_bounds__(64) void detect_overlap_kernel(const float4* __restrict__ boxes, int N, int W, float thr,
                                                            unsigned long long* __restrict__ mat) {
    overlap_tile(boxes, N, W, thr, mat, blockIdx.x, blockIdx.y);
}

// keys: (orderable(score) << 32) | proposal, sorted descending = score descending, then HIGHER proposal index first
// (np.argsort(s, kind="stable")[::-1]); 0 pads the sort (no candidate key is 0: candidates are never NaN)
// one class c of one image: kc = the class's W words of kept bits; s_key = the workgroup's dynamic LDS [pow2ceil(N)]
__device__ __forceinline__ void nms_class(const float* __restrict__ scores, int ld, const float4* __restrict__ boxes, int N,
                                          int W, float score_thr, float nms_thr,
                                          const unsigned long long* __restrict__ mat, unsigned long long* __restrict__ kc,
                                          int c, const float* __restrict__ bounds, unsigned long long* s_key) {
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    // test.py:370 / mask_eval_utils.py:62: s > float32(SCORE_THRESH); the order of insertion does not matter (keys are unique)
    for (int base = 0; base < N; base += 1024) {
        const int p = base + tid;
        const float s = p < N && !filtered_out(boxes + p, bounds) ? scores[(size_t)p * ld + c] : 0.0f;
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
    if (lane < W) kc[lane] = kb0;
    if (lane + 64 < W) kc[lane + 64] = kb1;
}

__global__ __launch_bounds__(1024) void detect_nms_kernel(const float* __restrict__ scores, int ld,
                                                          const float4* __restrict__ boxes, int N, int W, float score_thr,
                                                          float nms_thr, const unsigned long long* __restrict__ mat,
                                                          unsigned long long* __restrict__ keepbits) {
    extern __shared__ unsigned long long s_key[];                      // [pow2ceil(N)]
    const int c = blockIdx.x;
    nms_class(scores, ld, boxes, N, W, score_thr, nms_thr, mat, keepbits + (size_t)c * W, c, nullptr, s_key);
}

// np.sort(image_scores)[-max_det] over the T orderable keys of lkey: the max_det-th largest, four 8-bit digits from the top.
// 0 (below every candidate key) when no limit applies.  The whole 1024-lane workgroup calls it, lkey visible to all lanes.
__device__ __forceinline__ uint32_t limit_threshold(const uint32_t* __restrict__ lkey, int T, int max_det) {
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_prefix, s_k;
    const int tid = threadIdx.x;
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
    return thr_key;
}

// test.py:395-403: the kept set in (class, proposal) order, thresholded at the max_det-th largest kept score when more
// than max_det are kept.  det records: (proposal, class, score bits).  cmask [C] (null: every class): classes whose
// records are written - applied AFTER the limit (generate_mask_for_MaskRCNN.py:124-136 limits over all classes first)
__device__ __forceinline__ void limit_image(const float* __restrict__ scores, int ld, int C, int W, int max_det,
                                            const unsigned long long* __restrict__ keepbits, uint32_t* __restrict__ lkey,
                                            int* __restrict__ lidx, int* __restrict__ lcls, int* __restrict__ det,
                                            int* __restrict__ count, int* __restrict__ total,
                                            const unsigned char* __restrict__ cmask) {
    __shared__ int s_part[16];
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
    const uint32_t thr_key = limit_threshold(lkey, T, max_det);
    // keep score >= image_thresh (ties at the threshold all stay, as in the reference)
    int outn = 0;
    for (int base = 0; base < T; base += 1024) {
        const int i = base + tid;
        const bool on = i < T && lkey[i] >= thr_key && (!cmask || cmask[lcls[i]]);
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

__global__ __launch_bounds__(1024) void detect_limit_kernel(const float* __restrict__ scores, int ld, int C, int W,
                                                            int max_det, const unsigned long long* __restrict__ keepbits,
                                                            uint32_t* __restrict__ lkey, int* __restrict__ lidx,
                                                            int* __restrict__ lcls, int* __restrict__ det,
                                                            int* __restrict__ count, int* __restrict__ total) {
    limit_image(scores, ld, C, W, max_det, keepbits, lkey, lidx, lcls, det, count, total, nullptr);
}

// ---------------------------------------------------------------- ragged batch: B images back to back
// Workspace head (BatchView): what the prologue derives from row_off on the device.  ok = 0 when the device's
// row_off does not give the totals the host sized the grids and the workspace with: every later launch then does nothing
// and total[b] = -1.
struct BatchView {
    int* ok;                    // [1]
    int* start;                 // [B]      first row of image b
    int* n;                     // [B]      N_b
    int* words;                 // [B]      W_b = ceil(N_b / 64)
    int* word_off;              // [B + 1]  prefix of W_b (keep bits: C * word_off[b] words before image b)
    int* tile_off;              // [B + 1]  prefix of W_b^2
    long long* mat_off;         // [B + 1]  prefix of N_b * W_b (u64 words)
};

__host__ __device__ inline size_t batch_meta_bytes(int B) {
    return ((((size_t)2 + 3 * (size_t)B + 2 * ((size_t)B + 1)) * 4 + 7) & ~(size_t)7) + ((size_t)B + 1) * 8;
}

__host__ __device__ inline BatchView batch_view(void* ws, int B) {
    BatchView v;
    int* p = static_cast<int*>(ws);
    v.ok = p;
    v.start = p + 2;
    v.n = v.start + B;
    v.words = v.n + B;
    v.word_off = v.words + B;
    v.tile_off = v.word_off + B + 1;
    v.mat_off = reinterpret_cast<long long*>(static_cast<char*>(ws) + batch_meta_bytes(B) - ((size_t)B + 1) * 8);
    return v;
}

__global__ __launch_bounds__(1024) void detect_batch_prologue_kernel(const int* __restrict__ row_off, int B, int total_n,
                                                                     int tot_words, int tot_tiles, long long tot_mat,
                                                                     void* ws) {
    __shared__ int s_part[16];
    __shared__ long long s_lpart[16];
    __shared__ int s_bad;
    const BatchView v = batch_view(ws, B);
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = (row_off[0] != 0 || row_off[B] != total_n) ? 1 : 0;
    __syncthreads();
    int words = 0, tiles = 0;
    long long mat = 0;
    for (int base = 0; base < B; base += 1024) {
        const int b = base + tid;
        int s = 0, n = 0;
        if (b < B) {
            s = row_off[b];
            n = row_off[b + 1] - s;
            if (s < 0 || n < 1 || n > kMaxN || s > total_n - n) {
                atomicOr(&s_bad, 1);
                s = 0;
                n = 1;
            }
        }
        const int W = (n + 63) / 64;                                   // (0 past the last image)
        int tw, tt;
        long long tm;
        const int ow = words + block_exclusive_scan(W, s_part, &tw);
        const int ot = tiles + block_exclusive_scan(W * W, s_part, &tt);
        const long long om = mat + block_exclusive_scan((long long)n * W, s_lpart, &tm);
        if (b < B) {
            v.start[b] = s;
            v.n[b] = n;
            v.words[b] = W;
            v.word_off[b] = ow;
            v.tile_off[b] = ot;
            v.mat_off[b] = om;
        }
        words += tw;
        tiles += tt;
        mat += tm;
    }
    __syncthreads();
    if (tid == 0) {
        v.word_off[B] = words;
        v.tile_off[B] = tiles;
        v.mat_off[B] = mat;
        *v.ok = (!s_bad && words == tot_words && tiles == tot_tiles && mat == tot_mat) ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void detect_batch_overlap_kernel(const float4* __restrict__ boxes, int B, float thr,
                                                                  void* ws, unsigned long long* __restrict__ mat) {
    const BatchView v = batch_view(ws, B);
    if (!*v.ok) return;
    const int t = blockIdx.x;                                          // < tile_off[B]: the grid is sized by it
    int lo = 0, hi = B - 1;                                            // the last image with tile_off[b] <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (v.tile_off[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    const int W = v.words[lo], local = t - v.tile_off[lo];
    if (local >= W * W) return;
    overlap_tile(boxes + v.start[lo], v.n[lo], W, thr, mat + v.mat_off[lo], local % W, local / W);
}

__global__ __launch_bounds__(1024) void detect_batch_nms_kernel(const float* __restrict__ scores, int ld,
                                                                const float4* __restrict__ boxes, int B, int C,
                                                                float score_thr, float nms_thr,
                                                                const float* __restrict__ area_bounds, void* ws,
                                                                const unsigned long long* __restrict__ mat,
                                                                unsigned long long* __restrict__ keepbits) {
    extern __shared__ unsigned long long s_key[];                      // [pow2ceil(max N_b)]
    const BatchView v = batch_view(ws, B);
    if (!*v.ok) return;
    const int c = blockIdx.x, b = blockIdx.y;
    const int s = v.start[b], W = v.words[b];
    nms_class(scores + (size_t)s * ld, ld, boxes + s, v.n[b], W, score_thr, nms_thr, mat + v.mat_off[b],
              keepbits + (size_t)C * v.word_off[b] + (size_t)c * W, c, area_bounds ? area_bounds + 2 * b : nullptr, s_key);
}

// image b's scratch and records start at element C * start[b] of lkey / lidx / lcls and record C * start[b] of det_img
__global__ __launch_bounds__(1024) void detect_batch_limit_kernel(const float* __restrict__ scores, int ld, int B, int C,
                                                                  int max_det, const unsigned char* __restrict__ class_mask,
                                                                  void* ws, const unsigned long long* __restrict__ keepbits,
                                                                  uint32_t* __restrict__ lkey, int* __restrict__ lidx,
                                                                  int* __restrict__ lcls, int* __restrict__ det_img,
                                                                  int* __restrict__ count, int* __restrict__ total) {
    const BatchView v = batch_view(ws, B);
    const int b = blockIdx.x;
    if (!*v.ok) {
        if (threadIdx.x == 0) total[b] = -1;
        return;
    }
    const int s = v.start[b];
    const size_t e = (size_t)C * s;
    limit_image(scores + (size_t)s * ld, ld, C, v.words[b], max_det, keepbits + (size_t)C * v.word_off[b], lkey + e, lidx + e,
                lcls + e, det_img + 3 * e, count + (size_t)b * C, total + b, class_mask ? class_mask + (size_t)b * C : nullptr);
}

// records of all images into one array, (image, class, proposal) order: image b's go to record sum(total[0 .. b))
__global__ __launch_bounds__(256) void detect_batch_compact_kernel(int B, int C, void* ws, const int* __restrict__ det_img,
                                                                   const int* __restrict__ total, int* __restrict__ det) {
    __shared__ long long s_sum[256];
    const BatchView v = batch_view(ws, B);
    if (!*v.ok) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    long long acc = 0;
    for (int i = tid; i < b; i += 256) acc += total[i];
    s_sum[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s_sum[tid] += s_sum[tid + h];
        __syncthreads();
    }
    const int* src = det_img + 3 * (size_t)C * v.start[b];
    int* dst = det + 3 * (size_t)s_sum[0];
    const int n = 3 * total[b];
    for (int i = tid; i < n; i += 256) dst[i] = src[i];
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

namespace {

struct BatchLayout {
    size_t mat, keep, lkey, lidx, lcls, det_img, total;
    int total_n, tot_words, tot_tiles, max_n;
    long long tot_mat;
};

// false (with the error set) unless 1 <= B <= the image limit, row_off starts at 0, every 1 <= N_b <= CIM_DETECT_MAX_N and
// 3 * C * sum N < 2^31
bool batch_layout(const char* who, const int* row_off, int B, int C, BatchLayout* L) {
    const char* limits = "need 1 <= B <= %d images, row_off[0] = 0 and non-decreasing, each 1 <= N_b <= %d, C >= 1 and "
                         "3 * C * sum N < 2^31";
    char why[256];
    snprintf(why, sizeof why, limits, CIM_BATCH_DETECT_MAX_IMAGES, kMaxN);
    if (!row_off) {
        cim::set_error("%s: row_off (host) is null; %s", who, why);
        return false;
    }
    if (B < 1 || B > CIM_BATCH_DETECT_MAX_IMAGES || C < 1) {
        cim::set_error("%s: %s (B=%d, C=%d)", who, why, B, C);
        return false;
    }
    if (row_off[0] != 0) {
        cim::set_error("%s: %s (row_off[0]=%d)", who, why, row_off[0]);
        return false;
    }
    long long words = 0, tiles = 0, mat = 0;
    int max_n = 0;
    for (int b = 0; b < B; ++b) {
        const long long n = (long long)row_off[b + 1] - row_off[b];
        if (n < 1 || n > kMaxN) {
            cim::set_error("%s: %s (image %d: row_off %d -> %d, N_b=%lld)", who, why, b, row_off[b], row_off[b + 1], n);
            return false;
        }
        const long long W = (n + 63) / 64;
        words += W;
        tiles += W * W;
        mat += n * W;
        if (n > max_n) max_n = (int)n;
    }
    const long long cap = (long long)C * row_off[B];
    if (cap > (long long)(INT_MAX / 3)) {
        cim::set_error("%s: %s (C=%d, sum N=%d)", who, why, C, row_off[B]);
        return false;
    }
    const size_t ints = ((size_t)cap * 4 + 255) & ~(size_t)255;
    L->total_n = row_off[B];
    L->tot_words = (int)words;                                         // <= B * 128
    L->tot_tiles = (int)tiles;                                         // <= B * 128^2 < 2^31 at the image limit
    L->tot_mat = mat;
    L->max_n = max_n;
    L->mat = (batch_meta_bytes(B) + 255) & ~(size_t)255;
    L->keep = L->mat + (size_t)mat * 8;
    L->lkey = L->keep + (size_t)C * (size_t)words * 8;
    L->lidx = L->lkey + ints;
    L->lcls = L->lidx + ints;
    L->det_img = L->lcls + ints;
    L->total = L->det_img + 3 * ints;
    return true;
}

}  // namespace

extern "C" long long cim_batch_detect_ws_bytes(const int* row_off, int B, int C) {
    BatchLayout L;
    if (!batch_layout("cim_batch_detect_ws_bytes", row_off, B, C, &L)) return -1;
    return (long long)L.total;
}

extern "C" int cim_batch_detect_nms_limit(const float* scores, int ld, const float* boxes, const int* row_off_dev,
                                          const int* row_off_host, int B, int C, float score_thr, float nms_thr, int max_det,
                                          const float* area_bounds, const unsigned char* class_mask, void* ws, int* det,
                                          int* count, int* total, void* stream) {
    BatchLayout L;
    if (!batch_layout("cim_batch_detect_nms_limit", row_off_host, B, C, &L)) return -1;
    if (ld < C) {
        cim::set_error("cim_batch_detect_nms_limit: the scores' leading dimension must be >= C (ld=%d, C=%d)", ld, C);
        return -1;
    }
    if (area_bounds && !(score_thr >= 0.0f)) {                         // a filtered score reads 0: it must not be a candidate
        cim::set_error("cim_batch_detect_nms_limit: area_bounds needs score_thr >= 0 (score_thr=%g)", (double)score_thr);
        return -1;
    }
    CIM_CHECK_ARG(scores && boxes && row_off_dev && ws && det && count && total);
    CIM_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)ws & 7) == 0);
    hipStream_t st = cim::as_stream(stream);
    char* w = static_cast<char*>(ws);
    auto* mat = reinterpret_cast<unsigned long long*>(w + L.mat);
    auto* keep = reinterpret_cast<unsigned long long*>(w + L.keep);
    int* det_img = reinterpret_cast<int*>(w + L.det_img);
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    hipLaunchKernelGGL(detect_batch_prologue_kernel, dim3(1), dim3(1024), 0, st, row_off_dev, B, L.total_n, L.tot_words,
                       L.tot_tiles, L.tot_mat, ws);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(detect_batch_overlap_kernel, dim3(L.tot_tiles), dim3(64), 0, st, bx, B, nms_thr, ws, mat);
    CIM_CHECK_LAUNCH();
    int P = 1;
    while (P < L.max_n) P <<= 1;
    const int lds = P * 8;
    CIM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(detect_batch_nms_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(detect_batch_nms_kernel, dim3(C, B), dim3(1024), lds, st, scores, ld, bx, B, C, score_thr, nms_thr,
                       area_bounds, ws, mat, keep);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(detect_batch_limit_kernel, dim3(B), dim3(1024), 0, st, scores, ld, B, C, max_det, class_mask, ws, keep,
                       reinterpret_cast<uint32_t*>(w + L.lkey), reinterpret_cast<int*>(w + L.lidx),
                       reinterpret_cast<int*>(w + L.lcls), det_img, count, total);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(detect_batch_compact_kernel, dim3(B), dim3(256), 0, st, B, C, ws, det_img, total, det);
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

// ---------------------------------------------------------------- soft-NMS, box voting and their limit
// TEST.SOFT_NMS / TEST.BBOX_VOTE of box_results_with_nms_and_limit (lib/core/test.py:378-396): cython_nms.pyx:98-203,
// boxes.py:268-317 over cython_bbox.pyx:32-73.  Per class the records (proposal, class, score bits) go to srec[c][.] in the
// reference's order - selection order under soft-NMS, ascending proposal after the greedy pass -, the voting kernel rewrites
// their scores and fills vbox, and one limit workgroup writes the records that reach the limit, their order preserved.
namespace {

// cython_nms.pyx:166-172 and cython_bbox.pyx:52-72 are the same fp32 expression: t the selected / top box, b the examined
// one.  false (no overlap computed: the pyx skips the row, bbox_overlaps leaves 0) unless iw > 0 and ih > 0.
__device__ __forceinline__ bool guarded_overlap(float4 t, float4 b, float* ov) {
    const float area = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
    const float iw = pyx_min(t.z, b.z) - pyx_max(t.x, b.x) + 1.0f;
    if (!(iw > 0.0f)) return false;
    const float ih = pyx_min(t.w, b.w) - pyx_max(t.y, b.y) + 1.0f;
    if (!(ih > 0.0f)) return false;
    const float ua = (t.z - t.x + 1.0f) * (t.w - t.y + 1.0f) + area - iw * ih;
    *ov = iw * ih / ua;                                                 // correctly rounded fp32 division
    return true;
}

// cython_nms.pyx:174-187: the decayed score weight * s
__device__ __forceinline__ float soft_decay(int kind, float ov, float nt, float sigma, float s) {
    float weight;
    if (kind == CIM_SOFTVOTE_NMS_SOFT_LINEAR) weight = ov > nt ? 1.0f - ov : 1.0f;
    else if (kind == CIM_SOFTVOTE_NMS_SOFT_GAUSSIAN) weight = (float)exp((double)(-(ov * ov) / sigma));   // np.exp: double
    else weight = ov > nt ? 0.0f : 1.0f;
    return weight * s;
}

// the scan of cython_nms.pyx:128-132 keeps the FIRST position of the maximum (strict <)
struct SoftBest {
    float s;
    int q;
};
__device__ __forceinline__ SoftBest soft_better(SoftBest a, SoftBest b) {
    return (b.s > a.s || (b.s == a.s && b.q < a.q)) ? b : a;
}

// One workgroup per class.  LDS: perm [N] i32 (position -> proposal), score [N] f32, hole [N / 2 + 1] u16.
// Per selection step i: argmax over [i, n) and its swap to i; every later position is examined once against the selected
// box (decay + survival flag); then the pyx's swap-with-last removal as a partition: with M survivors the holes (removed
// positions below i + 1 + M, ascending) take the survivors at positions >= i + 1 + M in descending order.
__global__ __launch_bounds__(1024) void softvote_soft_nms_kernel(const float* __restrict__ scores, int ld,
                                                                 const float4* __restrict__ boxes, int N, float score_thr,
                                                                 float nt, float sigma, float min_score, int kind,
                                                                 int* __restrict__ srec, int* __restrict__ scnt) {
    extern __shared__ int s_dyn[];
    __shared__ int s_part[16];
    __shared__ SoftBest s_best[16];
    __shared__ int s_wcnt[128];
    int* s_perm = s_dyn;
    float* s_sc = reinterpret_cast<float*>(s_dyn + N);
    unsigned short* s_hole = reinterpret_cast<unsigned short*>(s_dyn + 2 * (size_t)N);
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    // dets_j: the candidates s > float32(SCORE_THRESH) in ascending proposal order
    int n = 0;
    for (int base = 0; base < N; base += 1024) {
        const int p = base + tid;
        const float s = p < N ? scores[(size_t)p * ld + c] : 0.0f;
        const bool cand = p < N && s > score_thr;
        int tot;
        const int o = n + block_exclusive_scan(cand ? 1 : 0, s_part, &tot);
        if (cand) {
            s_perm[o] = p;
            s_sc[o] = s;
        }
        n += tot;
    }
    __syncthreads();
    int* rec = srec + 3 * (size_t)c * N;
    for (int i = 0; i < n; ++i) {                                       // (n is uniform over the workgroup)
        SoftBest b = {-INFINITY, INT_MAX};
        for (int q = i + tid; q < n; q += 1024) b = soft_better(b, SoftBest{s_sc[q], q});
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b = soft_better(b, SoftBest{__shfl_xor(b.s, o), __shfl_xor(b.q, o)});
        if (lane == 0) s_best[wave] = b;
        __syncthreads();
        b = s_best[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) b = soft_better(b, s_best[w]);
        const int m = b.q;                                              // i <= m < n
        const int pm = s_perm[m], pi = s_perm[i];
        const float sm = s_sc[m], si = s_sc[i];
        __syncthreads();                                                // (rows i and m and s_best have been read)
        // the swap: lane 0 writes row i and the record, the lane that examines position m writes row m below
        if (tid == 0) {
            s_perm[i] = pm;
            s_sc[i] = sm;
            rec[3 * i] = pm;
            rec[3 * i + 1] = c;
            rec[3 * i + 2] = __float_as_int(sm);
        }
        const float4 t = boxes[pm];
        const int lo = i + 1;
        const int tiles = (n - lo + 1023) >> 10;                        // <= 8: N <= 8192
        unsigned long long bal[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bal[j] = 0;
            if (j < tiles) {
                const int q = lo + j * 1024 + tid;
                bool surv = false;
                if (q < n) {
                    const int p = q == m ? pi : s_perm[q];
                    float s = q == m ? si : s_sc[q];
                    float ov;
                    surv = true;
                    if (guarded_overlap(t, boxes[p], &ov)) {
                        s = soft_decay(kind, ov, nt, sigma, s);
                        surv = !(s < min_score);                        // cython_nms.pyx:191, inside the overlap branch
                    }
                    if (q == m) s_perm[q] = p;
                    s_sc[q] = s;
                }
                bal[j] = __ballot(surv);
                if (lane == 0) s_wcnt[j * 16 + wave] = (int)__popcll(bal[j]);
            }
        }
        __syncthreads();
        // survivors before each (tile, wave): every wave scans the <= 128 counts itself
        const int nc = tiles * 16;
        const int v0 = lane < nc ? s_wcnt[lane] : 0, v1 = lane + 64 < nc ? s_wcnt[lane + 64] : 0;
        int i0 = v0, i1 = v1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int x0 = __shfl_up(i0, o), x1 = __shfl_up(i1, o);
            if (lane >= o) {
                i0 += x0;
                i1 += x1;
            }
        }
        i1 += __shfl(i0, 63);
        const int M = __shfl(i1, 63);
        const int e0 = i0 - v0, e1 = i1 - v1;
        int pre[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            pre[j] = 0;
            if (j < tiles) {
                const int at = j * 16 + wave;
                const int a0 = __shfl(e0, at & 63), a1 = __shfl(e1, at & 63);
                pre[j] = (at < 64 ? a0 : a1) + (int)__popcll(bal[j] & below);
                const int q = lo + j * 1024 + tid;
                if (q < n && !((bal[j] >> lane) & 1ull) && q < lo + M) s_hole[(q - lo) - pre[j]] = (unsigned short)q;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < tiles) {
                const int q = lo + j * 1024 + tid;
                if (q < n && ((bal[j] >> lane) & 1ull) && q >= lo + M) {
                    const int dst = s_hole[M - pre[j] - 1];
                    s_perm[dst] = s_perm[q];
                    s_sc[dst] = s_sc[q];
                }
            }
        }
        n = lo + M;
        __syncthreads();
    }
    if (tid == 0) scnt[c] = n;
}

// the greedy pass's kept bits of class c as records in ascending proposal order (dets_j[keep, :])
__global__ __launch_bounds__(1024) void softvote_from_keep_kernel(const float* __restrict__ scores, int ld, int N, int W,
                                                                  const unsigned long long* __restrict__ keepbits,
                                                                  int* __restrict__ srec, int* __restrict__ scnt) {
    __shared__ int s_part[16];
    const int c = blockIdx.x, tid = threadIdx.x;
    unsigned long long word = tid < W ? keepbits[(size_t)c * W + tid] : 0ull;      // W <= 128
    int tot;
    int o = block_exclusive_scan((int)__popcll(word), s_part, &tot);
    int* rec = srec + 3 * (size_t)c * N;
    while (word) {
        const int p = tid * 64 + __builtin_ctzll(word);
        word &= word - 1;
        rec[3 * o] = p;
        rec[3 * o + 1] = c;
        rec[3 * o + 2] = __float_as_int(scores[(size_t)p * ld + c]);
        ++o;
    }
    if (tid == 0) scnt[c] = tot;
}

__device__ __forceinline__ double wave_sum(double v) {                  // a fixed tree: the same bits on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// boxes.py:268-317.  One wave per top detection; class c = blockIdx.y, top t of the class: record srec[c * cap + t], its box
// top_boxes[c * cap + t] or, with top_boxes null, the record's proposal.  The voters are the class's candidates
// (scores[p, c] > score_thr; every row with use_thr == 0) whose fp32 overlap with the top box is >= vote_thr.  Sums are
// taken in double, lane-strided and then over the fixed tree above.  Writes the voted box, and the score by `method`
// (ID: untouched) to out_score[(c * cap + t) * score_stride]; an empty vote set (or weights summing to 0: np.average's
// ZeroDivisionError) writes NaN and counts in *empty.
__global__ __launch_bounds__(256) void softvote_vote_kernel(const float* __restrict__ scores, int ld,
                                                            const float4* __restrict__ boxes, int N, float score_thr,
                                                            int use_thr, float vote_thr, int method, float beta,
                                                            const float4* __restrict__ top_boxes,
                                                            const int* __restrict__ srec, const int* __restrict__ scnt,
                                                            int T, int cap, float4* __restrict__ vbox,
                                                            float* __restrict__ out_score, int score_stride,
                                                            int* __restrict__ empty) {
    const int c = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cnt = scnt ? scnt[c] : T;
    const double dbeta = (double)beta;
    for (int t = blockIdx.x * 4 + wave; t < cnt; t += gridDim.x * 4) {
        const size_t r = (size_t)c * cap + t;
        const float4 tb = top_boxes ? top_boxes[r] : boxes[srec[3 * r]];
        double sx1 = 0, sy1 = 0, sx2 = 0, sy2 = 0, sw = 0, sov = 0, sovw = 0, sp = 0, st = 0, cn = 0;
        for (int p = lane; p < N; p += 64) {
            const float s = scores[(size_t)p * ld + c];
            if (use_thr && !(s > score_thr)) continue;
            const float4 b = boxes[p];
            float ov = 0.0f;
            if (!guarded_overlap(tb, b, &ov)) ov = 0.0f;
            if (!(ov >= vote_thr)) continue;
            const double w = (double)s;
            sx1 += w * (double)b.x;
            sy1 += w * (double)b.y;
            sx2 += w * (double)b.z;
            sy2 += w * (double)b.w;
            sw += w;
            cn += 1.0;
            if (method == CIM_SOFTVOTE_SCORE_IOU_AVG) {
                sov += (double)ov;
                sovw += (double)ov * w;
            } else if (method == CIM_SOFTVOTE_SCORE_GENERALIZED_AVG) {
                sp += pow(w, dbeta);
            } else if (method == CIM_SOFTVOTE_SCORE_TEMP_AVG) {       // boxes.py:292-297 for one voter
                const double a = w, nb = 1.0 - w, mx = a >= nb ? a : nb;
                const double xa = exp(log(a / mx) / dbeta), xb = exp(log(nb / mx) / dbeta);
                st += xa / (xa + xb);
            }
        }
        sx1 = wave_sum(sx1);
        sy1 = wave_sum(sy1);
        sx2 = wave_sum(sx2);
        sy2 = wave_sum(sy2);
        sw = wave_sum(sw);
        cn = wave_sum(cn);
        if (method == CIM_SOFTVOTE_SCORE_IOU_AVG) {
            sov = wave_sum(sov);
            sovw = wave_sum(sovw);
        } else if (method == CIM_SOFTVOTE_SCORE_GENERALIZED_AVG) {
            sp = wave_sum(sp);
        } else if (method == CIM_SOFTVOTE_SCORE_TEMP_AVG) {
            st = wave_sum(st);
        }
        if (lane != 0) continue;
        bool bad = cn == 0.0 || sw == 0.0;
        double score = 0.0;
        if (!bad) {
            if (method == CIM_SOFTVOTE_SCORE_AVG) score = sw / cn;
            else if (method == CIM_SOFTVOTE_SCORE_IOU_AVG) {
                bad = sov == 0.0;
                score = sovw / sov;
            } else if (method == CIM_SOFTVOTE_SCORE_QUASI_SUM) score = sw / pow(cn, dbeta);
            else if (method == CIM_SOFTVOTE_SCORE_GENERALIZED_AVG) score = pow(sp / cn, 1.0 / dbeta);
            else if (method == CIM_SOFTVOTE_SCORE_TEMP_AVG) score = st / cn;
        }
        if (bad) {
            const float nan = __int_as_float(0x7fc00000);
            vbox[r] = make_float4(nan, nan, nan, nan);
            if (method != CIM_SOFTVOTE_SCORE_ID) out_score[r * score_stride] = nan;
            atomicAdd(empty, 1);
        } else {
            vbox[r] = make_float4((float)(sx1 / sw), (float)(sy1 / sw), (float)(sx2 / sw), (float)(sy2 / sw));
            if (method != CIM_SOFTVOTE_SCORE_ID) out_score[r * score_stride] = (float)score;
        }
    }
}

// test.py:399-408 over the per-class records (after voting: the limit sees the re-scored detections): one workgroup.
// Record order is preserved; boxes are the voted ones (vbox) or, with vbox null, the proposals'.
__global__ __launch_bounds__(1024) void softvote_limit_kernel(const float4* __restrict__ boxes, int C, int cap, int max_det,
                                                              const int* __restrict__ srec, const int* __restrict__ scnt,
                                                              const float4* __restrict__ vbox, uint32_t* __restrict__ lkey,
                                                              int* __restrict__ lsrc, int* __restrict__ det,
                                                              float4* __restrict__ det_boxes, int* __restrict__ count,
                                                              int* __restrict__ total) {
    __shared__ int s_part[16];
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 1024) count[c] = 0;
    __threadfence();                                                   // (the zeros reach L2 before any atomic below)
    int T = 0;
    for (int c = 0; c < C; ++c) {
        const int cnt = scnt[c];
        for (int i = tid; i < cnt; i += 1024) {
            const int r = c * cap + i;                                 // < C * N <= INT_MAX / 3
            lkey[T + i] = orderable(__int_as_float(srec[3 * (size_t)r + 2]));
            lsrc[T + i] = r;
        }
        T += cnt;
    }
    __syncthreads();
    const uint32_t thr_key = limit_threshold(lkey, T, max_det);
    int outn = 0;
    for (int base = 0; base < T; base += 1024) {
        const int i = base + tid;
        const bool on = i < T && lkey[i] >= thr_key;
        int tot;
        const int o = outn + block_exclusive_scan(on ? 1 : 0, s_part, &tot);
        if (on) {
            const int r = lsrc[i];
            const int p = srec[3 * (size_t)r], c = srec[3 * (size_t)r + 1];
            det[3 * (size_t)o] = p;
            det[3 * (size_t)o + 1] = c;
            det[3 * (size_t)o + 2] = srec[3 * (size_t)r + 2];
            det_boxes[o] = vbox ? vbox[r] : boxes[p];
            atomicAdd(count + c, 1);
        }
        outn += tot;
    }
    if (tid == 0) *total = outn;
}

struct SoftvoteLayout {
    DetectLayout d;
    size_t srec, scnt, vbox, total;
};

SoftvoteLayout softvote_layout(int N, int C) {
    const size_t cap = (size_t)C * N;
    SoftvoteLayout L;
    L.d = layout(N, C);
    L.srec = (L.d.total + 255) & ~(size_t)255;
    L.scnt = L.srec + ((cap * 12 + 255) & ~(size_t)255);
    L.vbox = L.scnt + (((size_t)C * 4 + 255) & ~(size_t)255);
    L.total = L.vbox + cap * 16;
    return L;
}

bool nms_kind_ok(int k) { return k >= CIM_SOFTVOTE_NMS_GREEDY && k <= CIM_SOFTVOTE_NMS_SOFT_GAUSSIAN; }
bool scoring_ok(int m) { return m >= CIM_SOFTVOTE_SCORE_ID && m <= CIM_SOFTVOTE_SCORE_TEMP_AVG; }

}  // namespace

extern "C" long long cim_softvote_ws_bytes(int N, int C) {
    if (!shape_ok(N, C)) {
        cim::set_error("cim_softvote_ws_bytes: need 1 <= N <= %d and C >= 1 with 3 * C * N < 2^31 (N=%d, C=%d)", kMaxN, N, C);
        return -1;
    }
    return (long long)softvote_layout(N, C).total;
}

extern "C" int cim_softvote_postprocess(const float* scores, int ld, const float* boxes, int N, int C, float score_thr,
                                        float nms_thr, int nms_kind, float sigma, float soft_min_score, int vote,
                                        float vote_thr, int scoring_method, float beta, int max_det, void* ws, int* det,
                                        float* det_boxes, int* count_per_class, int* total, int* empty_votes, void* stream) {
    if (!shape_ok(N, C)) {
        cim::set_error("cim_softvote_postprocess: need 1 <= N <= %d and C >= 1 with 3 * C * N < 2^31 (N=%d, C=%d)", kMaxN, N, C);
        return -1;
    }
    if (!nms_kind_ok(nms_kind) || !scoring_ok(scoring_method)) {
        cim::set_error("cim_softvote_postprocess: unknown nms_kind %d or scoring_method %d", nms_kind, scoring_method);
        return -1;
    }
    if (vote && !(score_thr >= 0.0f)) {                                // the voters' scores are the weights of the mean
        cim::set_error("cim_softvote_postprocess: voting needs score_thr >= 0 (score_thr=%g)", (double)score_thr);
        return -1;
    }
    CIM_CHECK_ARG(ld >= C);
    CIM_CHECK_ARG(scores && boxes && ws && det && det_boxes && count_per_class && total && empty_votes);
    CIM_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)det_boxes & 15) == 0);
    hipStream_t st = cim::as_stream(stream);
    const int W = (N + 63) / 64;
    const SoftvoteLayout L = softvote_layout(N, C);
    char* w = static_cast<char*>(ws);
    const float4* bx = reinterpret_cast<const float4*>(boxes);
    int* srec = reinterpret_cast<int*>(w + L.srec);
    int* scnt = reinterpret_cast<int*>(w + L.scnt);
    float4* vbox = reinterpret_cast<float4*>(w + L.vbox);
    CIM_CHECK_HIP(hipMemsetAsync(empty_votes, 0, sizeof(int), st));
    if (nms_kind == CIM_SOFTVOTE_NMS_GREEDY) {
        auto* mat = reinterpret_cast<unsigned long long*>(w + L.d.mat);
        auto* keep = reinterpret_cast<unsigned long long*>(w + L.d.keep);
        hipLaunchKernelGGL(detect_overlap_kernel, dim3(W, W), dim3(64), 0, st, bx, N, W, nms_thr, mat);
        CIM_CHECK_LAUNCH();
        int P = 1;
        while (P < N) P <<= 1;
        const int lds = P * 8;
        CIM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(detect_nms_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(detect_nms_kernel, dim3(C), dim3(1024), lds, st, scores, ld, bx, N, W, score_thr, nms_thr, mat, keep);
        CIM_CHECK_LAUNCH();
        hipLaunchKernelGGL(softvote_from_keep_kernel, dim3(C), dim3(1024), 0, st, scores, ld, N, W, keep, srec, scnt);
        CIM_CHECK_LAUNCH();
    } else {
        const int lds = 8 * N + 2 * (N / 2 + 1) + 2;
        CIM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(softvote_soft_nms_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(softvote_soft_nms_kernel, dim3(C), dim3(1024), lds, st, scores, ld, bx, N, score_thr, nms_thr, sigma,
                           soft_min_score, nms_kind, srec, scnt);
        CIM_CHECK_LAUNCH();
    }
    if (vote) {
        hipLaunchKernelGGL(softvote_vote_kernel, dim3(std::min(64, (N + 3) / 4), C), dim3(256), 0, st, scores, ld, bx, N, score_thr, 1,
                           vote_thr, scoring_method, beta, (const float4*)nullptr, srec, scnt, 0, N, vbox,
                           reinterpret_cast<float*>(srec) + 2, 3, empty_votes);
        CIM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(softvote_limit_kernel, dim3(1), dim3(1024), 0, st, bx, C, N, max_det, srec, scnt,
                       vote ? vbox : (const float4*)nullptr, reinterpret_cast<uint32_t*>(w + L.d.lkey),
                       reinterpret_cast<int*>(w + L.d.lidx), det, reinterpret_cast<float4*>(det_boxes), count_per_class, total);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_softvote_vote(const float* all_boxes, const float* all_scores, int K, const float* top_boxes, int T,
                                 float vote_thr, int scoring_method, float beta, float* out_boxes, float* out_scores,
                                 int* empty_votes, void* stream) {
    if (K < 1 || T < 1 || !scoring_ok(scoring_method)) {
        cim::set_error("cim_softvote_vote: need K >= 1 voters, T >= 1 top boxes and a known scoring method (K=%d, T=%d, "
                       "scoring_method=%d)", K, T, scoring_method);
        return -1;
    }
    CIM_CHECK_ARG(all_boxes && all_scores && top_boxes && out_boxes && out_scores && empty_votes);
    CIM_CHECK_ARG(((uintptr_t)all_boxes & 15) == 0 && ((uintptr_t)top_boxes & 15) == 0 && ((uintptr_t)out_boxes & 15) == 0);
    hipStream_t st = cim::as_stream(stream);
    CIM_CHECK_HIP(hipMemsetAsync(empty_votes, 0, sizeof(int), st));
    hipLaunchKernelGGL(softvote_vote_kernel, dim3(std::min(1024, (T + 3) / 4), 1), dim3(256), 0, st, all_scores, 1,
                       reinterpret_cast<const float4*>(all_boxes), K, 0.0f, 0, vote_thr, scoring_method, beta,
                       reinterpret_cast<const float4*>(top_boxes), (const int*)nullptr, (const int*)nullptr, T, T,
                       reinterpret_cast<float4*>(out_boxes), out_scores, 1, empty_votes);
    CIM_CHECK_LAUNCH();
    return 0;
}
