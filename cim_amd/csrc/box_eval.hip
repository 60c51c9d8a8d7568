// Box evaluation for gfx950: COCOeval(..., 'bbox')'s evaluateImg per image and the PASCAL VOC devkit's per-class matching,
// precision / recall / AP and CorLoc on the device - the stage after detection (csrc/detect.hip) that scores kept boxes.
//
// Replaces pycocotools' maskApi.c bbIou + COCOeval.evaluateImg as lib/datasets/json_dataset_evaluator.py:105-118 runs them,
// lib/datasets/voc_eval.py:146-228 and lib/datasets/dis_eval.py:88-141.  Exactness contract: DESIGN.md 4.14, include/cim_hip.h.
//
//   box_area_kernel         w * h per detection (what COCO.loadRes stores as a bbox result's area)
//   segm_dt_sort_kernel     eval_match.h: per (image, category) stable rank by descending score, cut to maxDets[-1]
//   box_iou_kernel          bbIou of every (kept detection, ground truth) pair of a group; one lane per pair
//   segm_match_kernel       eval_match.h: evaluateImg's greedy matcher, here on fp64 detection areas
//   voc_match_kernel        per (class, image) group: stable sort by -confidence, then voc_eval's / dis_eval's greedy rule
//   voc_run_sort_kernel     per run (<= 256 detections of one class): stable rank by -confidence in LDS
//   segm_merge_kernel       eval_match.h: one bottom-up merge round, element indices ordered by (-confidence, position)
//   voc_ap_kernel           per class: cumulative tp / fp, rec, prec, the 11-point or the area AP
#pragma clang fp contract(off)                      // every product and sum below is rounded on its own, as NumPy's / C's are
#include "common.h"
#include "../../include/cim_hip.h"
#include <float.h>
#include "eval_match.h"

namespace {

constexpr int kRun = CIM_VOC_MAX_RUN;

// One rounding per operation.  These are plain operators compiled under the pragma above; HIP's __dmul_rn / __dadd_rn are
// header inlines compiled before it, whose results the backend may still fuse into an FMA (seen in the ISA), so they are not used.
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__device__ __forceinline__ double dsub(double a, double b) { return a - b; }

// descending fp64 value as an ascending unsigned key: IEEE order, -0 == +0; total, so a rank is always a permutation
__device__ __forceinline__ u64 orderable64(double f) {
    if (f == 0.0) f = 0.0;
    const u64 u = (u64)__double_as_longlong(f);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void box_area_kernel(const double* __restrict__ box, int D, double* __restrict__ area) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d < D) area[d] = dmul(box[4 * (size_t)d + 2], box[4 * (size_t)d + 3]);
}

// maskApi.c bbIou on (x, y, w, h), operation for operation
__global__ __launch_bounds__(256) void box_iou_kernel(const double* __restrict__ dt, int D, const double* __restrict__ gt, int G,
                                                      const int* __restrict__ meta, int n_groups, int n_dl, int n_gl,
                                                      long long pairs, int T, int A, const uint8_t* __restrict__ rec,
                                                      double* __restrict__ iou) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    int a = 0, b = n_groups - 1;                                         // last group with pair_off <= p
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (meta[8 * mid + 6] <= p) a = mid;
        else b = mid - 1;
    }
    const Group g = load_group(meta, a);
    const long long q = p - g.pair_off;
    if (g.n_gt <= 0 || q < 0 || q >= (long long)g.nd * g.n_gt) return;
    const int rk = (int)(q / g.n_gt), gi = (int)(q - (long long)rk * g.n_gt);
    const Rec L = rec_layout(g.nd, g.n_gt, A, T);
    const int d = reinterpret_cast<const int*>(rec + g.rec_off + L.order)[rk];
    const int* gl = meta + 8 * n_groups + n_dl;
    const int gg = gl[g.gt_start + gi];
    double v = 0.0;
    if (d >= 0 && d < D && gg >= 0 && gg < G) {
        const int crowd = gl[n_gl + gg];
        const double* Dv = dt + 4 * (size_t)d;
        const double* Gv = gt + 4 * (size_t)gg;
        const double da = dmul(Dv[2], Dv[3]), ga = dmul(Gv[2], Gv[3]);
        const double w = dsub(fmin(dadd(Dv[2], Dv[0]), dadd(Gv[2], Gv[0])), fmax(Dv[0], Gv[0]));
        const double h = dsub(fmin(dadd(Dv[3], Dv[1]), dadd(Gv[3], Gv[1])), fmax(Dv[1], Gv[1]));
        if (!(w <= 0.0) && !(h <= 0.0)) {
            const double i = dmul(w, h);
            const double u = crowd ? da : dsub(dadd(da, ga), i);
            v = i / u;
        }
    }
    iou[p] = v;
}

// ---- VOC ---------------------------------------------------------------------------------------------------------------------
// np.max / np.argmax over the overlaps: a NaN beats everything, the first of equals wins
__device__ __forceinline__ bool beats(double v2, int p2, double v, int p) {
    if (p2 < 0) return false;
    if (p < 0) return true;
    const bool n2 = v2 != v2, n = v != v;
    if (n2 || n) return n2 && (!n || p2 < p);
    return v2 > v || (v2 == v && p2 < p);
}

// groups [n_groups][4] = (det_start, n_det, gt_start, n_gt).  256 lanes rank the group's detections; wave 0 then visits them
// in that order, lane l holding ground truths l, l + 64, ... (16 claim bits per lane).
__global__ __launch_bounds__(256) void voc_match_kernel(const double* __restrict__ dt_box, const double* __restrict__ dt_conf, int D,
                                                        const double* __restrict__ gt_box, const uint8_t* __restrict__ gt_diff,
                                                        int G, const int* __restrict__ groups, double ovthresh, int mode,
                                                        uint8_t* __restrict__ tp, uint8_t* __restrict__ fp,
                                                        double* __restrict__ ovmax, int* __restrict__ jmax) {
    __shared__ int s_order[kMaxDt];
    const int* gr = groups + 4 * (size_t)blockIdx.x;
    long long ds = gr[0], n = gr[1], gs = gr[2], ng = gr[3];
    if (ds < 0 || n < 0 || ds + n > D) n = 0;                            // (a group outside the arrays is left alone)
    if (gs < 0 || ng < 0 || gs + ng > G) ng = n = 0;
    if (n > kMaxDt) n = kMaxDt;
    if (ng > kMaxGt) ng = kMaxGt;
    const double* conf = dt_conf + ds;
    for (int i = threadIdx.x; i < n; i += 256) {
        const u64 ki = orderable64(conf[i]);
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const u64 kj = orderable64(conf[j]);
            rank += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
        }
        s_order[rank] = i;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const double* gb = gt_box + 4 * gs;
    uint32_t claimed = 0;
    for (int r = 0; r < n; ++r) {
        const long long d = ds + s_order[r];
        const double b0 = dt_box[4 * d], b1 = dt_box[4 * d + 1], b2 = dt_box[4 * d + 2], b3 = dt_box[4 * d + 3];
        const double barea = dmul(dadd(dsub(b2, b0), 1.0), dadd(dsub(b3, b1), 1.0));
        double bv = 0.0;
        int bp = -1;
        for (int c = 0; c < 16; ++c) {
            const int p = c * 64 + lane;
            if (p >= ng) break;
            const double* q = gb + 4 * (size_t)p;
            const double iw = fmax(dadd(dsub(fmin(q[2], b2), fmax(q[0], b0)), 1.0), 0.0);
            const double ih = fmax(dadd(dsub(fmin(q[3], b3), fmax(q[1], b1)), 1.0), 0.0);
            const double inters = dmul(iw, ih);
            const double garea = dmul(dadd(dsub(q[2], q[0]), 1.0), dadd(dsub(q[3], q[1]), 1.0));
            const double uni = dsub(dadd(barea, garea), inters);
            const double v = inters / uni;
            if (beats(v, p, bv, bp)) {
                bv = v;
                bp = p;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double v2 = __shfl_xor(bv, o);
            const int p2 = __shfl_xor(bp, o);
            if (beats(v2, p2, bv, bp)) {
                bv = v2;
                bp = p2;
            }
        }
        int is_tp = 0, is_fp = 1;
        if (bp >= 0 && bv > ovthresh) {
            if (mode == 1) {
                is_tp = 1;
                is_fp = 0;
            } else {
                const int was = (int)((__shfl(claimed, bp & 63) >> (bp >> 6)) & 1u);
                if (gt_diff[gs + bp]) is_fp = 0;
                else if (!was) {
                    is_tp = 1;
                    is_fp = 0;
                    if (lane == (bp & 63)) claimed |= 1u << (bp >> 6);
                }
            }
        }
        if (lane == 0) {
            tp[d] = (uint8_t)is_tp;
            fp[d] = (uint8_t)is_fp;
            ovmax[d] = bp >= 0 ? bv : -HUGE_VAL;
            jmax[d] = bp;
        }
    }
}

// runs [n_runs][2] int64 = (start, length <= kRun): the run's element indices in (-confidence, position) order
__global__ __launch_bounds__(256) void voc_run_sort_kernel(const double* __restrict__ conf, long long D,
                                                           const int64_t* __restrict__ runs, u64* __restrict__ idx) {
    __shared__ u64 s_key[kRun];
    const long long s = runs[2 * (size_t)blockIdx.x];
    long long n = runs[2 * (size_t)blockIdx.x + 1];
    if (s < 0 || n < 0 || n > kRun || s + n > D) return;
    const int i = threadIdx.x;
    if (i < n) s_key[i] = orderable64(conf[s + i]);
    __syncthreads();
    if (i >= n) return;
    const u64 ki = s_key[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (s_key[j] > ki || (s_key[j] == ki && j < i)) ? 1 : 0;
    idx[s + rank] = (u64)(s + i);
}

struct ConfLess {                                                        // a sorts before b
    const double* conf;
    long long D;
    __device__ __forceinline__ bool operator()(u64 a, u64 b) const {
        const u64 ka = a < (u64)D ? orderable64(conf[a]) : 0ull, kb = b < (u64)D ? orderable64(conf[b]) : 0ull;
        return ka > kb || (ka == kb && a < b);
    }
};

__device__ __forceinline__ double block_sum(double v, double* part) {    // 256 lanes, every lane gets the total
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// voc_eval.py:219-226 and voc_ap for class k, its sorted element indices at idx[c0, c1).  Pass 1 walks left to right:
// cumulative tp / fp, rec, prec, and the maximum precision at rec >= each of the 11 thresholds.  Pass 2 (area form) walks
// right to left as segm_accum_kernel does: the envelope max(prec_j, j >= i) times the recall step at i.
__global__ __launch_bounds__(256) void voc_ap_kernel(const u64* __restrict__ idx, const uint8_t* __restrict__ tp_in,
                                                     const uint8_t* __restrict__ fp_in, long long D,
                                                     const int64_t* __restrict__ class_off, const double* __restrict__ npos,
                                                     const double* __restrict__ thr11, double* __restrict__ rec,
                                                     double* __restrict__ prec, double* __restrict__ ap) {
    __shared__ int s_part[4];
    __shared__ double s_dpart[4];
    __shared__ double s_p11[11];
    const int tid = threadIdx.x, k = blockIdx.x;
    long long c0 = class_off[k], c1 = class_off[k + 1];
    if (c0 < 0 || c1 > D || c0 > c1) c0 = c1 = 0;
    const double dn = npos[k];
    double pmax[11];
#pragma unroll
    for (int t = 0; t < 11; ++t) pmax[t] = -1.0;
    double th[11];
#pragma unroll
    for (int t = 0; t < 11; ++t) th[t] = thr11 ? thr11[t] : 0.0;
    int ctp = 0, cfp = 0;
    for (long long lo = c0; lo < c1; lo += 256) {
        const long long i = lo + tid;
        int t1 = 0, f1 = 0;
        if (i < c1) {
            const u64 e = idx[i];
            if (e < (u64)D) {
                t1 = tp_in[e] != 0;
                f1 = fp_in[e] != 0;
            }
        }
        int ttp, tfp;
        const int stp = block_incl_sum(t1, s_part, &ttp);
        const int sfp = block_incl_sum(f1, s_part, &tfp);
        if (i < c1) {
            const double dtp = (double)(ctp + stp), dfp = (double)(cfp + sfp);
            const double rc = dtp / dn;
            const double pr = dtp / fmax(dadd(dtp, dfp), DBL_EPSILON);
            rec[i] = rc;
            prec[i] = pr;
#pragma unroll
            for (int t = 0; t < 11; ++t)
                if (rc >= th[t] && pr > pmax[t]) pmax[t] = pr;
        }
        ctp += ttp;
        cfp += tfp;
    }
    if (thr11) {
#pragma unroll
        for (int t = 0; t < 11; ++t) {
            double tot;
            block_incl_max(pmax[t], s_dpart, &tot);
            if (tid == 0) s_p11[t] = tot;
        }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0;
            for (int t = 0; t < 11; ++t) a = dadd(a, (s_p11[t] < 0.0 ? 0.0 : s_p11[t]) / 11.0);
            ap[k] = a;
        }
        return;
    }
    __syncthreads();                                                     // (rec / prec of pass 1 are read back below)
    double sum = 0.0, cmax = 0.0;                                        // (mpre's right sentinel is 0)
    for (long long hi = c1; hi > c0; hi -= 256) {
        const long long i = hi - 1 - tid;
        const double pr = i >= c0 ? prec[i] : -1.0;
        double tmax;
        double env = block_incl_max(pr, s_dpart, &tmax);
        env = cmax > env ? cmax : env;
        if (i >= c0) {
            const double r1 = rec[i], r0 = i > c0 ? rec[i - 1] : 0.0;
            if (r1 != r0) sum += dmul(dsub(r1, r0), env);
        }
        cmax = cmax > tmax ? cmax : tmax;
    }
    sum = block_sum(sum, s_dpart);
    if (tid == 0) {
        const double last = c1 > c0 ? rec[c1 - 1] : 0.0;                 // the step up to mrec's right sentinel 1, times mpre = 0
        if (1.0 != last) sum += dmul(dsub(1.0, last), 0.0);
        ap[k] = sum;
    }
}

bool box_image_shape_ok(int D, int G, long long pairs) {
    return D >= 0 && G >= 0 && G <= CIM_SEGM_MAX_GT && pairs >= 0 && pairs <= (long long)D * G && D < (1 << 28);
}

size_t al256(long long x) { return (size_t)((x + 255) & ~255ll); }

}  // namespace

extern "C" long long cim_box_image_ws_bytes(int D, int G, long long pairs) {
    if (!box_image_shape_ok(D, G, pairs)) {
        cim::set_error("cim_box_image_ws_bytes: need D >= 0, 0 <= G <= %d ground truths per image and 0 <= pairs <= D * G "
                       "(D=%d, G=%d, pairs=%lld)", CIM_SEGM_MAX_GT, D, G, pairs);
        return -1;
    }
    return (long long)(al256(8ll * D) + al256(8 * pairs) + 8);
}

extern "C" int cim_box_eval_image(const double* dt_box, int D, const double* gt_box, int G, const float* dt_score,
                                  const int32_t* meta, int n_groups, int n_dl, int n_gl, long long pairs, const double* gt_area,
                                  const int64_t* gt_id, const double* iou_thrs, int T, const double* area_rng, int A, void* ws,
                                  void* records, void* stream) {
    if (!box_image_shape_ok(D, G, pairs)) {
        cim::set_error("cim_box_eval_image: need D >= 0, 0 <= G <= %d ground truths per image and 0 <= pairs <= D * G "
                       "(D=%d, G=%d, pairs=%lld)", CIM_SEGM_MAX_GT, D, G, pairs);
        return -1;
    }
    CIM_CHECK_ARG(T >= 1 && T <= CIM_SEGM_MAX_T && A >= 1 && A <= CIM_SEGM_MAX_A);
    CIM_CHECK_ARG(n_groups >= 0 && n_dl >= 0 && n_dl <= D && n_gl >= 0 && n_gl <= G);
    if (n_groups == 0) return 0;
    CIM_CHECK_ARG(meta && iou_thrs && area_rng && ws && records);
    CIM_CHECK_ARG(D == 0 || (dt_box && dt_score));
    CIM_CHECK_ARG(G == 0 || (gt_box && gt_area && gt_id));
    CIM_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)records & 7) == 0);
    hipStream_t st = cim::as_stream(stream);
    char* w = static_cast<char*>(ws);
    double* dt_area = reinterpret_cast<double*>(w);
    double* iou = reinterpret_cast<double*>(w + al256(8ll * D));
    uint8_t* rec = static_cast<uint8_t*>(records);
    if (D > 0) {
        hipLaunchKernelGGL(box_area_kernel, dim3((D + 255) / 256), dim3(256), 0, st, dt_box, D, dt_area);
        CIM_CHECK_LAUNCH();
        hipLaunchKernelGGL(segm_dt_sort_kernel, dim3(n_groups), dim3(256), 0, st, dt_score, meta, n_groups, T, A, rec);
        CIM_CHECK_LAUNCH();
    }
    if (pairs > 0) {
        hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, dt_box, D, gt_box, G, meta,
                           n_groups, n_dl, n_gl, pairs, T, A, rec, iou);
        CIM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(segm_match_kernel<double>, dim3(n_groups * A * T), dim3(64), 0, st, dt_area, meta, n_groups, n_dl, n_gl,
                       gt_area, gt_id, iou_thrs, T, area_rng, A, iou, rec);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_voc_match(const double* dt_box, const double* dt_conf, int D, const double* gt_box, const uint8_t* gt_difficult,
                             int G, const int32_t* groups, int n_groups, double ovthresh, int mode, uint8_t* tp, uint8_t* fp,
                             double* ovmax, int32_t* jmax, void* stream) {
    if (D < 0 || G < 0 || n_groups < 0 || D >= (1 << 28) || G >= (1 << 28) || (mode != 0 && mode != 1)) {
        cim::set_error("cim_voc_match: need 0 <= D, G < 2^28, n_groups >= 0 and mode 0 (voc_eval) or 1 (dis_eval) (D=%d, G=%d, "
                       "n_groups=%d, mode=%d)", D, G, n_groups, mode);
        return -1;
    }
    if (n_groups == 0 || D == 0) return 0;
    CIM_CHECK_ARG(groups && dt_box && dt_conf && tp && fp && ovmax && jmax);
    CIM_CHECK_ARG(G == 0 || (gt_box && gt_difficult));
    hipLaunchKernelGGL(voc_match_kernel, dim3(n_groups), dim3(256), 0, cim::as_stream(stream), dt_box, dt_conf, D, gt_box,
                       gt_difficult, G, groups, ovthresh, mode, tp, fp, ovmax, jmax);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" long long cim_voc_ap_ws_bytes(long long D) {
    if (D < 0 || D >= (1ll << 31)) {
        cim::set_error("cim_voc_ap_ws_bytes: need 0 <= D < 2^31 detections (D=%lld)", D);
        return -1;
    }
    return (long long)(2 * al256(8 * D) + 8);
}

extern "C" int cim_voc_ap(const double* dt_conf, const uint8_t* tp, const uint8_t* fp, long long D, const int64_t* class_off,
                          const double* npos, int K, const int64_t* runs, int n_runs, const int64_t* jobs,
                          const int64_t* round_off, int rounds, const double* thr11, void* ws, double* rec, double* prec,
                          double* ap, void* stream) {
    if (D < 0 || D >= (1ll << 31) || K < 1 || n_runs < 0 || rounds < 0 || rounds >= 64) {
        cim::set_error("cim_voc_ap: need 0 <= D < 2^31 detections, K >= 1 classes, n_runs >= 0, 0 <= rounds < 64 (D=%lld, K=%d, "
                       "n_runs=%d, rounds=%d)", D, K, n_runs, rounds);
        return -1;
    }
    CIM_CHECK_ARG(class_off && npos && ap && ws);
    CIM_CHECK_ARG(D == 0 || (dt_conf && tp && fp && rec && prec && runs && n_runs > 0));
    CIM_CHECK_ARG(rounds == 0 || (jobs && round_off));
    CIM_CHECK_ARG(((uintptr_t)ws & 7) == 0);
    hipStream_t st = cim::as_stream(stream);
    u64* k0 = reinterpret_cast<u64*>(ws);
    u64* k1 = reinterpret_cast<u64*>(static_cast<char*>(ws) + al256(8 * D));
    if (D > 0) {
        CIM_CHECK_HIP(hipMemsetAsync(ws, 0xff, 2 * al256(8 * D), st));    // (an element no run or job covers reads as "none")
        hipLaunchKernelGGL(voc_run_sort_kernel, dim3(n_runs), dim3(256), 0, st, dt_conf, D, runs, k0);
        CIM_CHECK_LAUNCH();
        const unsigned eb = (unsigned)((D + 255) / 256);
        const ConfLess less = {dt_conf, D};
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(segm_merge_kernel<ConfLess>, dim3(eb), dim3(256), 0, st, (r & 1) ? k1 : k0, (r & 1) ? k0 : k1, D,
                               jobs, round_off, r, less);
            CIM_CHECK_LAUNCH();
        }
    }
    hipLaunchKernelGGL(voc_ap_kernel, dim3(K), dim3(256), 0, st, (rounds & 1) ? k1 : k0, tp, fp, D, class_off, npos, thr11, rec,
                       prec, ap);
    CIM_CHECK_LAUNCH();
    return 0;
}
