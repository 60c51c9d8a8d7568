// Instance-segmentation evaluation for gfx950: COCO run-length encoding of masks and COCOeval('segm')'s evaluateImg /
// accumulate on the device - the stage after detection (csrc/detect.hip) that turns kept proposal masks into mask AP.
//
// Replaces pycocotools' mask.encode / decode / iou and COCOeval.evaluateImg / accumulate as the reference calls them
// (tools/evaluation.py:72-145, 236-241; lib/datasets/json_inference.py:24-55; lib/utils/mask_eval_utils.py:113-116).
// Exactness contract (bit-identical fp64 outputs, identical run counts): DESIGN.md 4.12, include/cim_hip.h.
//
// Masks are bit-packed in COCO's COLUMN-MAJOR pixel order (pixel p = x * H + y is bit p & 63 of word p >> 6, one row of
// ceil(H W / 64) words per mask), so a run-length code is a linear scan and an intersection is a popcount of an AND.
//   segm_pack_kernel        [n, H, W] bytes (row-major, optionally gathered by an index list) -> packed; one wave per word
//   segm_area_kernel        pixel count per mask; one wave per mask
//   segm_rle_count_kernel   run counts per mask (transitions + 1); one wave per mask
//   segm_rle_write_kernel   the runs themselves, a wave scan over 64 words at a time; one wave per mask
//   segm_rle_ends_kernel /  decode: inclusive run ends per mask (one wave per mask), then every word from a binary search
//   segm_rle_bits_kernel    over its mask's ends (one lane per word)
//   segm_dt_sort_kernel     per (image, category): stable rank by descending score, truncated to maxDets[-1]
//   segm_iou_kernel         per (image, category): IoU of every (kept detection, ground truth) pair; one wave per pair
//   segm_match_kernel       per (image, category, area range, threshold): evaluateImg's greedy matching; one wave
//   segm_gather_kernel /    accumulate: the records of all images in (category, image, rank) order, 64-bit keys
//   segm_npig_kernel        (orderable score, sequence), non-ignored ground truths per (category, area)
//   segm_merge_kernel       one bottom-up merge round of the per-image sorted runs (a binary search per element)
//   segm_accum_kernel       per (category, area, maxDet, threshold): cumulative TP / FP, precision envelope, searchsorted
// The sort, the matcher, the merge round and the block scans live in eval_match.h, shared with box_eval.hip.
#pragma clang fp contract(off)                      // pr = tp / ((fp + tp) + eps): no fused operations
#include "common.h"
#include "../../include/cim_hip.h"
#include <limits.h>
#include "eval_match.h"

namespace {

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ long long wave_incl_sum64(long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long x = __shfl_up(v, o);
        if (lane >= o) v += x;
    }
    return v;
}

__device__ __forceinline__ long long wave_incl_max64(long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long x = __shfl_up(v, o);
        if (lane >= o && x > v) v = x;
    }
    return v;
}

// bits of word w that lie inside the image, and the run transitions in it: bit j set where pixel j differs from pixel j - 1
// (pixel -1 counts as 0: a mask starting with 1 starts with a zero-length run, as rleEncode's p = 0 start does)
__device__ __forceinline__ u64 transitions(const u64* __restrict__ m, int w, long long HW) {
    const long long rem = HW - (long long)w * 64;
    const u64 valid = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
    const u64 v = m[w];
    const u64 prev = w > 0 ? (m[w - 1] >> 63) : 0ull;
    return (v ^ ((v << 1) | prev)) & valid;
}

__global__ __launch_bounds__(256) void segm_pack_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                        long long n_src, int n, int H, int W, int words,
                                                        u64* __restrict__ packed) {
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gw >= (long long)n * words) return;                          // (wave-uniform)
    const int i = (int)(gw / words), w = (int)(gw - (long long)i * words);
    const long long s = idx ? idx[i] : (long long)i;
    const int HW = H * W;                                                // (<= CIM_SEGM_MAX_HW)
    const int p = w * 64 + lane;
    bool bit = false;
    if (s >= 0 && s < n_src && p < HW) {                               // (an index out of range packs an empty mask)
        const int x = p / H, y = p - x * H;
        bit = src[s * HW + y * W + x] != 0;
    }
    const u64 b = __ballot(bit);
    if (lane == 0) packed[(size_t)i * words + w] = b;
}

__global__ __launch_bounds__(64) void segm_area_kernel(const u64* __restrict__ packed, int words, int* __restrict__ area) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const u64* m = packed + (size_t)i * words;
    int a = 0;
    for (int w = lane; w < words; w += 64) a += __popcll(m[w]);
    a = wave_sum(a);
    if (lane == 0) area[i] = a;
}

__global__ __launch_bounds__(64) void segm_rle_count_kernel(const u64* __restrict__ packed, int words, long long HW,
                                                            int* __restrict__ len) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const u64* m = packed + (size_t)i * words;
    int c = 0;
    for (int w = lane; w < words; w += 64) c += __popcll(transitions(m, w, HW));
    c = wave_sum(c);
    if (lane == 0) len[i] = c + 1;
}

// counts[k] = t_k - t_{k-1} (t_{-1} = 0) for the transition positions t_k, then the last run HW - t_last
__global__ __launch_bounds__(64) void segm_rle_write_kernel(const u64* __restrict__ packed, int words, long long HW,
                                                            const int64_t* __restrict__ off, const int* __restrict__ len,
                                                            uint32_t* __restrict__ counts) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const u64* m = packed + (size_t)i * words;
    uint32_t* out = counts + off[i];
    const long long cap = len[i];
    long long base = 0, last = 0;                                        // runs written, position of the last transition
    for (int w0 = 0; w0 < words; w0 += 64) {
        const int w = w0 + lane;
        u64 t = w < words ? transitions(m, w, HW) : 0ull;
        const long long c = __popcll(t);
        const long long incl = wave_incl_sum64(c);
        const long long lastpos = t ? (long long)w * 64 + 63 - __builtin_clzll(t) : -1;
        const long long imax = wave_incl_max64(lastpos);
        long long prev = __shfl_up(imax, 1);
        if (lane == 0 || prev < last) prev = last;
        long long k = base + incl - c;
        while (t) {
            const long long pos = (long long)w * 64 + __builtin_ctzll(t);
            t &= t - 1;
            if (k < cap) out[k] = (uint32_t)(pos - prev);
            prev = pos;
            ++k;
        }
        base += __shfl(incl, 63);
        const long long tm = __shfl(imax, 63);
        if (tm > last) last = tm;
    }
    if (lane == 0 && base < cap) out[base] = (uint32_t)(HW - last);
}

// ends[k] = min(counts[0] + ... + counts[k], HW) per mask
__global__ __launch_bounds__(64) void segm_rle_ends_kernel(const uint32_t* __restrict__ counts, const int64_t* __restrict__ off,
                                                           const int* __restrict__ len, long long HW, uint32_t* __restrict__ ends) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const long long o = off[i], n = len[i];
    long long carry = 0;
    for (long long k0 = 0; k0 < n; k0 += 64) {
        const long long k = k0 + lane;
        const long long v = k < n ? (long long)counts[o + k] : 0;
        const long long s = carry + wave_incl_sum64(v);
        if (k < n) ends[o + k] = (uint32_t)(s < HW ? s : HW);
        carry = __shfl(s, 63);
        if (carry > HW) carry = HW;
    }
}

// odd runs are ones: word w of mask i from the runs that overlap [64 w, 64 w + 64); pixels past the sum of the counts stay 0
__global__ __launch_bounds__(256) void segm_rle_bits_kernel(const uint32_t* __restrict__ ends, const int64_t* __restrict__ off,
                                                            const int* __restrict__ len, int n, int words, long long HW,
                                                            u64* __restrict__ packed) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)n * words) return;
    const int i = (int)(g / words), w = (int)(g - (long long)i * words);
    const uint32_t* e = ends + off[i];
    const int nr = len[i];
    const long long lo = (long long)w * 64, hi = lo + 64 < HW ? lo + 64 : HW;
    int a = 0, b = nr;                                                   // first run with end > lo
    while (a < b) {
        const int mid = (a + b) >> 1;
        if ((long long)e[mid] > lo) b = mid;
        else a = mid + 1;
    }
    u64 bits = 0;
    for (int k = a; k < nr; ++k) {
        const long long s = k ? (long long)e[k - 1] : 0, t = e[k];
        if (s >= hi) break;
        if (k & 1) {
            const long long x0 = s > lo ? s : lo, x1 = t < hi ? t : hi;
            if (x1 > x0) {
                const int nb = (int)(x1 - x0);
                bits |= (nb == 64 ? ~0ull : ((1ull << nb) - 1ull)) << (x0 - lo);
            }
        }
    }
    packed[(size_t)i * words + w] = bits;
}

// maskUtils.iou (rleIou): inter / (area_d + area_g - inter), inter / area_d for a crowd ground truth, 0 when inter == 0
__global__ __launch_bounds__(256) void segm_iou_kernel(const u64* __restrict__ dt, const u64* __restrict__ gt, int words,
                                                       const int* __restrict__ dt_area, const int* __restrict__ gt_area,
                                                       const int* __restrict__ meta, int n_groups, int n_dl, int n_gl,
                                                       long long pairs, int T, int A, const uint8_t* __restrict__ rec,
                                                       double* __restrict__ iou) {
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= pairs) return;
    int a = 0, b = n_groups - 1;                                         // last group with pair_off <= p
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (meta[8 * mid + 6] <= p) a = mid;
        else b = mid - 1;
    }
    const Group g = load_group(meta, a);
    const long long q = p - g.pair_off;
    if (g.n_gt <= 0 || q >= (long long)g.nd * g.n_gt) return;
    const int rk = (int)(q / g.n_gt), gi = (int)(q - (long long)rk * g.n_gt);
    const Rec L = rec_layout(g.nd, g.n_gt, A, T);
    const int d = reinterpret_cast<const int*>(rec + g.rec_off + L.order)[rk];
    const int* gl = meta + 8 * n_groups + n_dl;
    const int gg = gl[g.gt_start + gi];
    const int crowd = gl[n_gl + gg];
    const u64* md = dt + (size_t)d * words;
    const u64* mg = gt + (size_t)gg * words;
    int inter = 0;
    for (int w = lane; w < words; w += 64) inter += __popcll(md[w] & mg[w]);
    inter = wave_sum(inter);
    if (lane == 0) {
        double v = 0.0;
        if (inter != 0) {
            const long long u = crowd ? (long long)dt_area[d] : (long long)dt_area[d] + gt_area[gg] - inter;
            v = (double)inter / (double)u;
        }
        iou[p] = v;
    }
}

// ---- accumulate ----------------------------------------------------------------------------------------------------------------
// entries [n][6] int64 = (record address, nd, ng, first element, category, 0), sorted by first element (category-major,
// image-minor).  Element e: rank e - first of its entry.
__device__ __forceinline__ int find_entry(const int64_t* __restrict__ ent, int n, long long e) {
    int a = 0, b = n - 1;                                                // last entry with first <= e
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (ent[6 * mid + 3] <= e) a = mid;
        else b = mid - 1;
    }
    return a;
}

__global__ __launch_bounds__(256) void segm_gather_kernel(const int64_t* __restrict__ ent, int n_ent, long long E, int T, int A,
                                                          u64* __restrict__ key, uint8_t* __restrict__ code,
                                                          float* __restrict__ score, int* __restrict__ rank) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int j = find_entry(ent, n_ent, e);
    const int64_t* en = ent + 6 * j;
    const uint8_t* r = reinterpret_cast<const uint8_t*>(en[0]);
    const long long nd = en[1], ng = en[2], rk = e - en[3];
    if (rk < 0 || rk >= nd) return;
    const Rec L = rec_layout(nd, ng, A, T);
    const float s = reinterpret_cast<const float*>(r + L.score)[rk];
    score[e] = s;
    rank[e] = (int)rk;
    key[e] = ((u64)(~orderable(s)) << 32) | (u64)e;
    const int64_t* dtm = reinterpret_cast<const int64_t*>(r + L.dtm);
    for (int q = 0; q < A * T; ++q) {
        const bool ig = r[L.dt_ig + (size_t)q * nd + rk] != 0;
        code[(size_t)q * E + e] = ig ? 0 : (dtm[(size_t)q * nd + rk] != 0 ? 1 : 2);
    }
}

__global__ __launch_bounds__(256) void segm_npig_kernel(const int64_t* __restrict__ ent, int n_ent, int T, int A,
                                                        int* __restrict__ npig) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_ent) return;
    const int64_t* en = ent + 6 * j;
    const uint8_t* r = reinterpret_cast<const uint8_t*>(en[0]);
    const Rec L = rec_layout(en[1], en[2], A, T);
    for (int a = 0; a < A; ++a) atomicAdd(npig + en[4] * A + a, reinterpret_cast<const int*>(r + L.npig)[a]);
}


// COCOeval.accumulate for one (category k, area a, maxDet m, threshold t).  The sorted keys of category k: [c0, c1).
// Pass 1 counts TP / FP / kept (rank < maxDet) detections; pass 2 walks the keys right to left (thread j takes position
// hi - 1 - j, so a prefix over threads is a suffix over positions): tp_i, fp_i, pr_i, the envelope max(pr_j, j >= i), and
// the recall thresholds whose searchsorted(rc, x, 'left') lands on i.
__global__ __launch_bounds__(256) void segm_accum_kernel(const u64* __restrict__ key, const int64_t* __restrict__ cat_off,
                                                         const uint8_t* __restrict__ code, const float* __restrict__ score,
                                                         const int* __restrict__ rank, const int* __restrict__ npig_all,
                                                         long long E, int K, const double* __restrict__ rec_thrs, int R,
                                                         const int* __restrict__ max_dets, int M, int A, int T,
                                                         double* __restrict__ precision, double* __restrict__ recall,
                                                         double* __restrict__ scores) {
    __shared__ double s_q[CIM_SEGM_MAX_R], s_ss[CIM_SEGM_MAX_R], s_rt[CIM_SEGM_MAX_R];
    __shared__ int s_part[4];
    __shared__ double s_dpart[4];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int t = b % T;
    b /= T;
    const int m = b % M;
    b /= M;
    const int a = b % A;
    const int k = b / A;
    const int npig = npig_all[k * A + a];
    const size_t rcl = (((size_t)t * K + k) * A + a) * M + m;
    auto pidx = [&](int r) { return ((((size_t)t * R + r) * K + k) * A + a) * M + m; };
    if (npig == 0) {                                                     // also: no (image, category) record at all
        for (int r = tid; r < R; r += 256) {
            precision[pidx(r)] = -1.0;
            scores[pidx(r)] = -1.0;
        }
        if (tid == 0) recall[rcl] = -1.0;
        return;
    }
    for (int r = tid; r < R; r += 256) {
        s_q[r] = 0.0;
        s_ss[r] = 0.0;
        s_rt[r] = rec_thrs[r];
    }
    const long long c0 = cat_off[k], c1 = cat_off[k + 1];
    const int md = max_dets[m];
    const uint8_t* cd = code + ((size_t)a * T + t) * E;
    int TP = 0, FP = 0, NF = 0;
    for (long long i = c0 + tid; i < c1; i += 256) {
        const long long e = (long long)(key[i] & 0xffffffffull);
        if (rank[e] < md) {
            const int c = cd[e];
            TP += c == 1;
            FP += c == 2;
            ++NF;
        }
    }
    int tot;
    block_incl_sum(TP, s_part, &tot);
    TP = tot;
    block_incl_sum(FP, s_part, &tot);
    FP = tot;
    block_incl_sum(NF, s_part, &tot);
    NF = tot;
    const double dn = (double)npig;
    if (tid == 0) recall[rcl] = NF ? (double)TP / dn : 0.0;
    const double eps = 2.220446049250313e-16;                            // np.spacing(1) = 2^-52
    int ctp = 0, cfp = 0, cf = 0;                                        // carried suffix sums
    double cmax = -1.0;                                                  // carried suffix max of pr
    for (long long hi = c1; hi > c0; hi -= 256) {
        const long long i = hi - 1 - tid;
        bool f = false;
        int tpf = 0, fpf = 0;
        long long e = 0;
        if (i >= c0) {
            e = (long long)(key[i] & 0xffffffffull);
            if (rank[e] < md) {
                f = true;
                const int c = cd[e];
                tpf = c == 1;
                fpf = c == 2;
            }
        }
        int ttp, tfp, tf;
        const int stp = block_incl_sum(tpf, s_part, &ttp);
        const int sfp = block_incl_sum(fpf, s_part, &tfp);
        const int sf = block_incl_sum(f ? 1 : 0, s_part, &tf);
        const int tp = TP - (ctp + stp) + tpf, fp = FP - (cfp + sfp) + fpf, pos = NF - (cf + sf);
        const double dtp = (double)tp, dfp = (double)fp;
        const double pr = f ? dtp / ((dfp + dtp) + eps) : -1.0;
        double tmax;
        double env = block_incl_max(pr, s_dpart, &tmax);
        env = cmax > env ? cmax : env;
        if (f && (tpf || pos == 0)) {
            const double rc = dtp / dn;
            int lo = 0, hi2 = R;                                         // r_end = #{r : rec_thrs[r] <= rc}
            while (lo < hi2) {
                const int mid = (lo + hi2) >> 1;
                if (s_rt[mid] <= rc) lo = mid + 1;
                else hi2 = mid;
            }
            const int r_end = lo;
            int r_beg = 0;
            if (pos > 0) {                                               // first r with rec_thrs[r] > rc of the previous detection
                const double rp = (double)(tp - tpf) / dn;
                lo = 0;
                hi2 = R;
                while (lo < hi2) {
                    const int mid = (lo + hi2) >> 1;
                    if (s_rt[mid] <= rp) lo = mid + 1;
                    else hi2 = mid;
                }
                r_beg = lo;
            }
            const double sc = (double)score[e];
            for (int r = r_beg; r < r_end; ++r) {
                s_q[r] = env;
                s_ss[r] = sc;
            }
        }
        ctp += ttp;
        cfp += tfp;
        cf += tf;
        cmax = cmax > tmax ? cmax : tmax;
    }
    __syncthreads();
    for (int r = tid; r < R; r += 256) {
        precision[pidx(r)] = s_q[r];
        scores[pidx(r)] = s_ss[r];
    }
}

bool mask_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= CIM_SEGM_MAX_HW; }

struct AccLayout {
    size_t key0, key1, code, score, rank, npig, total;
};
AccLayout acc_layout(long long E, int K, int A, int T) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    AccLayout L;
    L.key0 = 0;
    L.key1 = L.key0 + al(8 * (size_t)E);
    L.code = L.key1 + al(8 * (size_t)E);
    L.score = L.code + al((size_t)A * T * E);
    L.rank = L.score + al(4 * (size_t)E);
    L.npig = L.rank + al(4 * (size_t)E);
    L.total = L.npig + al(4 * (size_t)K * A);
    return L;
}

}  // namespace

extern "C" int cim_segm_words(int H, int W) {
    if (!mask_shape_ok(H, W)) {
        cim::set_error("cim_segm_words: need H, W >= 1 and H * W <= %d (H=%d, W=%d)", CIM_SEGM_MAX_HW, H, W);
        return -1;
    }
    return (int)(((long long)H * W + 63) / 64);
}

extern "C" int cim_segm_pack(const uint8_t* masks, const int64_t* idx, long long n_src, int n, int H, int W, uint64_t* packed,
                             void* stream) {
    if (!mask_shape_ok(H, W)) {
        cim::set_error("cim_segm_pack: need H, W >= 1 and H * W <= %d (H=%d, W=%d)", CIM_SEGM_MAX_HW, H, W);
        return -1;
    }
    CIM_CHECK_ARG(n >= 0 && n_src >= 0);
    if (n == 0) return 0;
    CIM_CHECK_ARG(masks && packed);
    const int words = (int)(((long long)H * W + 63) / 64);
    const long long waves = (long long)n * words;
    hipLaunchKernelGGL(segm_pack_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, cim::as_stream(stream), masks, idx,
                       n_src, n, H, W, words, reinterpret_cast<u64*>(packed));
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_segm_area(const uint64_t* packed, int n, int words, int32_t* area, void* stream) {
    CIM_CHECK_ARG(n >= 0 && words >= 1 && words <= CIM_SEGM_MAX_HW / 64);
    if (n == 0) return 0;
    CIM_CHECK_ARG(packed && area);
    hipLaunchKernelGGL(segm_area_kernel, dim3(n), dim3(64), 0, cim::as_stream(stream), reinterpret_cast<const u64*>(packed),
                       words, area);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_segm_rle_count(const uint64_t* packed, int n, int H, int W, int32_t* len, void* stream) {
    if (!mask_shape_ok(H, W)) {
        cim::set_error("cim_segm_rle_count: need H, W >= 1 and H * W <= %d (H=%d, W=%d)", CIM_SEGM_MAX_HW, H, W);
        return -1;
    }
    CIM_CHECK_ARG(n >= 0);
    if (n == 0) return 0;
    CIM_CHECK_ARG(packed && len);
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(segm_rle_count_kernel, dim3(n), dim3(64), 0, cim::as_stream(stream), reinterpret_cast<const u64*>(packed),
                       (int)((HW + 63) / 64), HW, len);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_segm_rle_write(const uint64_t* packed, int n, int H, int W, const int64_t* off, const int32_t* len,
                                  uint32_t* counts, void* stream) {
    if (!mask_shape_ok(H, W)) {
        cim::set_error("cim_segm_rle_write: need H, W >= 1 and H * W <= %d (H=%d, W=%d)", CIM_SEGM_MAX_HW, H, W);
        return -1;
    }
    CIM_CHECK_ARG(n >= 0);
    if (n == 0) return 0;
    CIM_CHECK_ARG(packed && off && len && counts);
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(segm_rle_write_kernel, dim3(n), dim3(64), 0, cim::as_stream(stream), reinterpret_cast<const u64*>(packed),
                       (int)((HW + 63) / 64), HW, off, len, counts);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" long long cim_segm_rle_decode_ws_bytes(long long total_counts) {
    if (total_counts < 0 || total_counts >= (1ll << 31)) {
        cim::set_error("cim_segm_rle_decode_ws_bytes: need 0 <= total counts < 2^31 (got %lld)", total_counts);
        return -1;
    }
    return 4 * total_counts + 8;
}

extern "C" int cim_segm_rle_decode(const uint32_t* counts, const int64_t* off, const int32_t* len, int n, int H, int W, void* ws,
                                   uint64_t* packed, void* stream) {
    if (!mask_shape_ok(H, W)) {
        cim::set_error("cim_segm_rle_decode: need H, W >= 1 and H * W <= %d (H=%d, W=%d)", CIM_SEGM_MAX_HW, H, W);
        return -1;
    }
    CIM_CHECK_ARG(n >= 0);
    if (n == 0) return 0;
    CIM_CHECK_ARG(counts && off && len && ws && packed);
    hipStream_t st = cim::as_stream(stream);
    const long long HW = (long long)H * W;
    const int words = (int)((HW + 63) / 64);
    uint32_t* ends = static_cast<uint32_t*>(ws);
    hipLaunchKernelGGL(segm_rle_ends_kernel, dim3(n), dim3(64), 0, st, counts, off, len, HW, ends);
    CIM_CHECK_LAUNCH();
    const long long th = (long long)n * words;
    hipLaunchKernelGGL(segm_rle_bits_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, st, ends, off, len, n, words, HW,
                       reinterpret_cast<u64*>(packed));
    CIM_CHECK_LAUNCH();
    return 0;
}

static bool image_shape_ok(int D, int G, long long pairs) {
    return D >= 0 && G >= 0 && G <= CIM_SEGM_MAX_GT && pairs >= 0 && pairs <= (long long)D * G && D < (1 << 28);
}

extern "C" long long cim_segm_image_ws_bytes(int D, int G, long long pairs) {
    if (!image_shape_ok(D, G, pairs)) {
        cim::set_error("cim_segm_image_ws_bytes: need D >= 0, 0 <= G <= %d ground truths per image and 0 <= pairs <= D * G "
                       "(D=%d, G=%d, pairs=%lld)", CIM_SEGM_MAX_GT, D, G, pairs);
        return -1;
    }
    auto al = [](long long x) { return (x + 255) & ~255ll; };
    return al(4ll * D) + al(4ll * G) + al(8 * pairs) + 8;
}

extern "C" long long cim_segm_record_bytes(int nd, int ng, int A, int T) {
    if (nd < 0 || nd > CIM_DETECT_MAX_N || ng < 0 || ng > CIM_SEGM_MAX_GT || A < 1 || A > CIM_SEGM_MAX_A || T < 1 ||
        T > CIM_SEGM_MAX_T) {
        cim::set_error("cim_segm_record_bytes: need 0 <= nd <= %d, 0 <= ng <= %d, 1 <= A <= %d, 1 <= T <= %d (nd=%d, ng=%d, A=%d, "
                       "T=%d)", CIM_DETECT_MAX_N, CIM_SEGM_MAX_GT, CIM_SEGM_MAX_A, CIM_SEGM_MAX_T, nd, ng, A, T);
        return -1;
    }
    return (long long)rec_layout(nd, ng, A, T).bytes;
}

extern "C" int cim_segm_eval_image(const uint64_t* dt_packed, int D, const uint64_t* gt_packed, int G, int words,
                                   const float* dt_score, const int32_t* meta, int n_groups, int n_dl, int n_gl,
                                   long long pairs, const double* gt_area, const int64_t* gt_id, const double* iou_thrs, int T,
                                   const double* area_rng, int A, void* ws, void* records, void* stream) {
    if (!image_shape_ok(D, G, pairs)) {
        cim::set_error("cim_segm_eval_image: need D >= 0, 0 <= G <= %d ground truths per image and 0 <= pairs <= D * G "
                       "(D=%d, G=%d, pairs=%lld)", CIM_SEGM_MAX_GT, D, G, pairs);
        return -1;
    }
    CIM_CHECK_ARG(T >= 1 && T <= CIM_SEGM_MAX_T && A >= 1 && A <= CIM_SEGM_MAX_A);
    CIM_CHECK_ARG(words >= 1 && words <= CIM_SEGM_MAX_HW / 64);
    CIM_CHECK_ARG(n_groups >= 0 && n_dl >= 0 && n_dl <= D && n_gl >= 0 && n_gl <= G);
    if (n_groups == 0) return 0;
    CIM_CHECK_ARG(meta && iou_thrs && area_rng && ws && records);
    CIM_CHECK_ARG(D == 0 || (dt_packed && dt_score));
    CIM_CHECK_ARG(G == 0 || (gt_packed && gt_area && gt_id));
    CIM_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)records & 7) == 0);
    hipStream_t st = cim::as_stream(stream);
    auto al = [](long long x) { return (size_t)((x + 255) & ~255ll); };
    char* w = static_cast<char*>(ws);
    int* dt_area = reinterpret_cast<int*>(w);
    int* gt_area_px = reinterpret_cast<int*>(w + al(4ll * D));
    double* iou = reinterpret_cast<double*>(w + al(4ll * D) + al(4ll * G));
    uint8_t* rec = static_cast<uint8_t*>(records);
    const u64* dp = reinterpret_cast<const u64*>(dt_packed);
    const u64* gp = reinterpret_cast<const u64*>(gt_packed);
    if (D > 0) {
        hipLaunchKernelGGL(segm_area_kernel, dim3(D), dim3(64), 0, st, dp, words, dt_area);
        CIM_CHECK_LAUNCH();
        hipLaunchKernelGGL(segm_dt_sort_kernel, dim3(n_groups), dim3(256), 0, st, dt_score, meta, n_groups, T, A, rec);
        CIM_CHECK_LAUNCH();
    }
    if (G > 0) {
        hipLaunchKernelGGL(segm_area_kernel, dim3(G), dim3(64), 0, st, gp, words, gt_area_px);
        CIM_CHECK_LAUNCH();
    }
    if (pairs > 0) {
        hipLaunchKernelGGL(segm_iou_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, st, dp, gp, words, dt_area, gt_area_px,
                           meta, n_groups, n_dl, n_gl, pairs, T, A, rec, iou);
        CIM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(segm_match_kernel<int>, dim3(n_groups * A * T), dim3(64), 0, st, dt_area, meta, n_groups, n_dl, n_gl, gt_area,
                       gt_id, iou_thrs, T, area_rng, A, iou, rec);
    CIM_CHECK_LAUNCH();
    return 0;
}

static bool acc_shape_ok(long long E, int n_ent, int K, int A, int T, int R, int M) {
    return E >= 0 && E < (1ll << 31) && n_ent >= 0 && K >= 1 && A >= 1 && A <= CIM_SEGM_MAX_A && T >= 1 && T <= CIM_SEGM_MAX_T &&
           R >= 1 && R <= CIM_SEGM_MAX_R && M >= 1 && M <= CIM_SEGM_MAX_M && (long long)K * A * M * T < (1ll << 31);
}

extern "C" long long cim_segm_accumulate_ws_bytes(long long E, int K, int A, int T) {
    if (!acc_shape_ok(E, 0, K, A, T, 1, 1)) {
        cim::set_error("cim_segm_accumulate_ws_bytes: need 0 <= E < 2^31 detections, K >= 1, 1 <= A <= %d, 1 <= T <= %d (E=%lld, "
                       "K=%d, A=%d, T=%d)", CIM_SEGM_MAX_A, CIM_SEGM_MAX_T, E, K, A, T);
        return -1;
    }
    return (long long)acc_layout(E, K, A, T).total;
}

extern "C" int cim_segm_accumulate(const int64_t* entries, int n_entries, long long E, int K, const int64_t* cat_off,
                                   const int64_t* jobs, const int64_t* round_off, int rounds, const double* rec_thrs, int R,
                                   const int32_t* max_dets, int M, int A, int T, void* ws, double* precision, double* recall,
                                   double* scores, void* stream) {
    if (!acc_shape_ok(E, n_entries, K, A, T, R, M)) {
        cim::set_error("cim_segm_accumulate: need 0 <= E < 2^31, K >= 1, 1 <= A <= %d, 1 <= T <= %d, 1 <= R <= %d, 1 <= M <= %d "
                       "(E=%lld, K=%d, A=%d, T=%d, R=%d, M=%d)", CIM_SEGM_MAX_A, CIM_SEGM_MAX_T, CIM_SEGM_MAX_R, CIM_SEGM_MAX_M,
                       E, K, A, T, R, M);
        return -1;
    }
    CIM_CHECK_ARG(rounds >= 0 && rounds < 64 && (E == 0 || n_entries > 0));
    CIM_CHECK_ARG(cat_off && rec_thrs && max_dets && ws && precision && recall && scores);
    CIM_CHECK_ARG(n_entries == 0 || entries);
    CIM_CHECK_ARG(rounds == 0 || (jobs && round_off));
    CIM_CHECK_ARG(((uintptr_t)ws & 7) == 0);
    hipStream_t st = cim::as_stream(stream);
    const AccLayout L = acc_layout(E, K, A, T);
    char* w = static_cast<char*>(ws);
    u64* k0 = reinterpret_cast<u64*>(w + L.key0);
    u64* k1 = reinterpret_cast<u64*>(w + L.key1);
    uint8_t* code = reinterpret_cast<uint8_t*>(w + L.code);
    float* sc = reinterpret_cast<float*>(w + L.score);
    int* rank = reinterpret_cast<int*>(w + L.rank);
    int* npig = reinterpret_cast<int*>(w + L.npig);
    CIM_CHECK_HIP(hipMemsetAsync(npig, 0, 4 * (size_t)K * A, st));
    if (n_entries > 0) {
        hipLaunchKernelGGL(segm_npig_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, st, entries, n_entries, T, A, npig);
        CIM_CHECK_LAUNCH();
    }
    const unsigned eb = (unsigned)((E + 255) / 256);
    if (E > 0) {
        hipLaunchKernelGGL(segm_gather_kernel, dim3(eb), dim3(256), 0, st, entries, n_entries, E, T, A, k0, code, sc, rank);
        CIM_CHECK_LAUNCH();
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(segm_merge_kernel<KeyLess>, dim3(eb), dim3(256), 0, st, (r & 1) ? k1 : k0, (r & 1) ? k0 : k1, E,
                               jobs, round_off, r, KeyLess());
            CIM_CHECK_LAUNCH();
        }
    }
    const u64* sorted = (rounds & 1) ? k1 : k0;
    hipLaunchKernelGGL(segm_accum_kernel, dim3((unsigned)((long long)K * A * M * T)), dim3(256), 0, st, sorted, cat_off, code, sc,
                       rank, npig, E, K, rec_thrs, R, max_dets, M, A, T, precision, recall, scores);
    CIM_CHECK_LAUNCH();
    return 0;
}
