// What the two evaluators share (segm_eval.hip: COCOeval 'segm', box_eval.hip: COCOeval 'bbox' and VOC AP): the (image,
// category) group and record layout, the stable score sort, evaluateImg's greedy matcher (one copy, a template over the
// detections' area type), the bottom-up merge round and the block scans.  Included once per translation unit; everything
// has internal linkage.
#pragma once
#include "common.h"
#include "wave_block.h"                             // orderable(): descending score as an ascending unsigned key, ~orderable(s)
#include "../../include/cim_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxGt = CIM_SEGM_MAX_GT;
constexpr int kMaxDt = CIM_DETECT_MAX_N;

// ---- per-image evaluation ---------------------------------------------------------------------------------------------------
// meta (int32): groups [n_groups][8] = (det_start, n_det, gt_start, n_gt, nd_keep, rec_off, pair_off, 0), then det_list [n_dl]
// (image detection indices, input order inside a group), gt_list [n_gl], crowd [G] (by image ground-truth index)
struct Group {
    int det_start, n_det, gt_start, n_gt, nd, rec_off, pair_off;
};
__device__ __forceinline__ Group load_group(const int* __restrict__ meta, int j) {
    const int* g = meta + 8 * j;
    Group r = {g[0], g[1], g[2], g[3], g[4], g[5], g[6]};
    if (r.n_gt > kMaxGt) r.n_gt = kMaxGt;
    if (r.n_det > kMaxDt) r.n_det = kMaxDt;
    if (r.nd > r.n_det) r.nd = r.n_det;
    return r;
}

// record of one (image, category) group, byte offsets from its rec_off (cim_amd/segm_eval.py: _record_layout mirrors this)
struct Rec {
    size_t dtm, score, order, npig, gt_order, dt_ig, gt_ig, bytes;
};
__host__ __device__ __forceinline__ Rec rec_layout(long long nd, long long ng, int A, int T) {
    Rec r;
    r.dtm = 0;                                                           // int64 [A][T][nd]: matched ground-truth id, 0 = none
    r.score = r.dtm + 8 * (size_t)(A * T) * nd;                          // f32 [nd] scores in rank order
    r.order = r.score + 4 * (size_t)nd;                                  // i32 [nd] image detection index of each rank
    r.npig = r.order + 4 * (size_t)nd;                                   // i32 [A] non-ignored ground truths
    r.gt_order = r.npig + 4 * (size_t)A;                                 // i32 [A][ng] image ground-truth index, evaluateImg order
    r.dt_ig = r.gt_order + 4 * (size_t)A * ng;                           // u8 [A][T][nd]
    r.gt_ig = r.dt_ig + (size_t)(A * T) * nd;                            // u8 [A][ng]
    r.bytes = (r.gt_ig + (size_t)A * ng + 7) & ~(size_t)7;
    return r;
}

// COCOeval.computeIoU / evaluateImg: dt sorted by -score, stable over the input order (argsort kind='mergesort'), cut to maxDets[-1]
__global__ __launch_bounds__(256) void segm_dt_sort_kernel(const float* __restrict__ score, const int* __restrict__ meta,
                                                           int n_groups, int T, int A, uint8_t* __restrict__ rec) {
    __shared__ uint32_t s_key[kMaxDt];
    const Group g = load_group(meta, blockIdx.x);
    const int* dl = meta + 8 * n_groups + g.det_start;
    const int n = g.n_det;
    for (int i = threadIdx.x; i < n; i += 256) s_key[i] = orderable(score[dl[i]]);
    __syncthreads();
    const Rec L = rec_layout(g.nd, g.n_gt, A, T);
    uint8_t* r = rec + g.rec_off;
    for (int i = threadIdx.x; i < n; i += 256) {
        const uint32_t ki = s_key[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t kj = s_key[j];
            rank += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
        }
        if (rank < g.nd) {
            reinterpret_cast<float*>(r + L.score)[rank] = score[dl[i]];
            reinterpret_cast<int*>(r + L.order)[rank] = dl[i];
        }
    }
}

// COCOeval.evaluateImg at maxDets[-1] for one (group, area range, threshold)
// AreaT: the detections' area as evaluateImg compares it to the area range - int pixel counts (segm), fp64 w * h (bbox)
template <typename AreaT>
__global__ __launch_bounds__(64) void segm_match_kernel(const AreaT* __restrict__ dt_area, const int* __restrict__ meta,
                                                        int n_groups, int n_dl, int n_gl, const double* __restrict__ gt_area_f,
                                                        const int64_t* __restrict__ gt_id, const double* __restrict__ iou_thrs,
                                                        int T, const double* __restrict__ area_rng, int A,
                                                        const double* __restrict__ iou, uint8_t* __restrict__ rec) {
    __shared__ int s_q[kMaxGt];                                          // evaluateImg position -> group-order index
    const int lane = threadIdx.x;
    const int t = blockIdx.x % T, ai = (blockIdx.x / T) % A, j = blockIdx.x / (T * A);
    const Group g = load_group(meta, j);
    const int ng = g.n_gt, nd = g.nd;
    const int* gl = meta + 8 * n_groups + n_dl + g.gt_start;
    const int* crowd = meta + 8 * n_groups + n_dl + n_gl;
    const double lo = area_rng[2 * ai], hi = area_rng[2 * ai + 1];
    const Rec L = rec_layout(nd, ng, A, T);
    uint8_t* r = rec + g.rec_off;
    // ground truths: _ignore = iscrowd or area outside [lo, hi]; stable argsort of _ignore = non-ignored first
    int nn = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int at = pass ? nn : 0;
        for (int q0 = 0; q0 < ng; q0 += 64) {
            const int q = q0 + lane;
            bool ig = false;
            if (q < ng) {
                const int gg = gl[q];
                const double ar = gt_area_f[gg];
                ig = crowd[gg] != 0 || ar < lo || ar > hi;
            }
            const bool take = q < ng && (pass ? ig : !ig);
            const u64 bal = __ballot(take);
            if (take) s_q[at + __popcll(bal & ((1ull << lane) - 1ull))] = q;
            at += __popcll(bal);
        }
        if (!pass) nn = at;
    }
    __syncthreads();
    if (t == 0) {
        for (int p = lane; p < ng; p += 64) {
            reinterpret_cast<int*>(r + L.gt_order)[(size_t)ai * ng + p] = gl[s_q[p]];
            r[L.gt_ig + (size_t)ai * ng + p] = p >= nn ? 1 : 0;
        }
        if (lane == 0) reinterpret_cast<int*>(r + L.npig)[ai] = nn;
    }
    // greedy matching, detections in rank order; lane holds positions p = lane + 64 c, c < 16
    const double th = iou_thrs[t];
    const double t0 = th < 1.0 - 1e-10 ? th : 1.0 - 1e-10;
    uint32_t matched = 0, crowdbits = 0;
    for (int c = 0; c < 16 && c * 64 + lane < ng; ++c)
        if (crowd[gl[s_q[c * 64 + lane]]]) crowdbits |= 1u << c;
    const double* row0 = iou + g.pair_off;
    const int* order = reinterpret_cast<const int*>(r + L.order);
    int64_t* dtm = reinterpret_cast<int64_t*>(r + L.dtm) + ((size_t)ai * T + t) * nd;
    uint8_t* dtig = r + L.dt_ig + ((size_t)ai * T + t) * nd;
    for (int rk = 0; rk < nd; ++rk) {
        const double* row = row0 + (size_t)rk * ng;
        // best per phase (0: non-ignored positions p < nn, 1: ignored): max IoU >= t0, the later position on ties
        double bv0 = -1.0, bv1 = -1.0;
        int bp0 = -1, bp1 = -1;
        for (int c = 0; c < 16; ++c) {
            const int p = c * 64 + lane;
            if (p >= ng) break;
            if (((matched >> c) & 1u) && !((crowdbits >> c) & 1u)) continue;
            const double v = row[s_q[p]];
            if (v < t0) continue;
            if (p < nn) {
                if (v >= bv0) {
                    bv0 = v;
                    bp0 = p;
                }
            } else if (v >= bv1) {
                bv1 = v;
                bp1 = p;
            }
        }
        int m = -1;
        for (int ph = 0; ph < 2 && m < 0; ++ph) {
            double v = ph ? bv1 : bv0;
            int p = ph ? bp1 : bp0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double v2 = __shfl_xor(v, o);
                const int p2 = __shfl_xor(p, o);
                if (p2 >= 0 && (p < 0 || v2 > v || (v2 == v && p2 > p))) {
                    v = v2;
                    p = p2;
                }
            }
            m = p;
        }
        int64_t id = 0;
        int ig = 0;
        if (m >= 0) {
            if ((m & 63) == lane) matched |= 1u << (m >> 6);
            id = gt_id[gl[s_q[m]]];
            ig = m >= nn ? 1 : 0;
        }
        if (lane == 0) {
            const double da = (double)dt_area[order[rk]];
            if (id == 0 && (da < lo || da > hi)) ig = 1;             // (dtm == 0: also a match to ground-truth id 0)
            dtm[rk] = id;
            dtig[rk] = (uint8_t)ig;
        }
    }
}

// one round: job (startA, lenA, lenB) merges the sorted runs [startA, +lenA) and [startA + lenA, +lenB); keys are unique under
// `less` (KeyLess: the 64-bit keys themselves; box_eval.hip orders element indices by their fp64 confidence).  A job that
// does not lie inside [0, E) moves nothing.
struct KeyLess {
    __device__ __forceinline__ bool operator()(u64 a, u64 b) const { return a < b; }
};
template <typename Less>
__global__ __launch_bounds__(256) void segm_merge_kernel(const u64* __restrict__ src, u64* __restrict__ dst, long long E,
                                                         const int64_t* __restrict__ jobs, const int64_t* __restrict__ round_off,
                                                         int round, Less less) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t* jb = jobs + 3 * round_off[round];
    const int nj = (int)(round_off[round + 1] - round_off[round]);
    if (nj <= 0) return;
    int a = 0, b = nj - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (jb[3 * mid] <= e) a = mid;
        else b = mid - 1;
    }
    const long long sA = jb[3 * a], lA = jb[3 * a + 1], lB = jb[3 * a + 2];
    if (sA < 0 || lA < 0 || lB < 0 || sA > e || lA > E || lB > E || sA + lA + lB > E || e >= sA + lA + lB) return;
    const u64 k = src[e];
    const bool inA = e < sA + lA;
    const u64* o = inA ? src + sA + lA : src + sA;                       // the other run
    long long lo = 0, hi = inA ? lB : lA;                                 // its keys < k
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (less(o[mid], k)) lo = mid + 1;
        else hi = mid;
    }
    const long long i = inA ? e - sA : e - sA - lA;
    dst[sA + i + lo] = k;
}

__device__ __forceinline__ int block_incl_sum(int v, int* part, int* total) {     // 256 lanes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    __syncthreads();
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        tot += part[w];
        off += w < wave ? part[w] : 0;
    }
    *total = tot;
    return off + incl;
}

__device__ __forceinline__ double block_incl_max(double v, double* part, double* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double x = __shfl_up(incl, o);
        if (lane >= o && x > incl) incl = x;
    }
    __syncthreads();
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    double off = -1.0, tot = -1.0;                                       // (precisions are >= 0)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        tot = part[w] > tot ? part[w] : tot;
        if (w < wave && part[w] > off) off = part[w];
    }
    *total = tot;
    return off > incl ? off : incl;
}

}  // namespace
