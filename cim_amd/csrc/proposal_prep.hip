// Per-proposal training inputs from raw proposal masks, for gfx950: tight boxes, areas, the S x S nearest-resized masks and
// the PRM / point cluster matrix, all derived from the bit-packed words that cim_mask_pack writes.
//
// Replaces tools/pre/generate_7_7_{voc,coco}.py:35-42 (np.nonzero + PIL nearest resize per proposal),
// tools/pre/AGPL_label_assign.py:154-180 and point_level_label_assign.py:66-93 (per point a NumPy mean over the selected
// masks and lib/utils/mask_utils.py:6-18 against every proposal).  Exactness contract: DESIGN.md 4.13.
//
// The byte masks are read once, by the pack.  Box and area are DERIVED from the words (one more pass over 1/8 of the bytes)
// rather than fused into the pack: the pack is a bandwidth kernel of one wave per 1024 pixels, and a fused form would add a
// division per lane and five atomics per wave (a million at 1000 x 375 x 500) to it; from the word-major layout the same five
// numbers cost one coalesced read of 23 MB, the shape of mask_area_kernel.  Integer VALU work throughout, no MFMA.
#include "common.h"
#include "../../include/cim_hip.h"

namespace {

struct Points {                                   // by value in the kernel arguments: no upload, no device pointer to keep alive
    int32_t pix[CIM_PROP_MAX_POINTS];             // row * W + col
    int16_t cls[CIM_PROP_MAX_POINTS];
};

// ---- boxes and areas from the words -----------------------------------------------------------------------------------------
// raw [5][N] int32, zeroed: area | HW - min p | max p + 1 | W - min x | max x + 1 (all met by atomicAdd / atomicMax of
// positive numbers, so 0 = "no bit seen").  grid = (ceil(N/64), chunks), 64 masks x 4 word phases per workgroup: the word index
// is the same in every lane of a wave, so where a word crosses image rows is wave-uniform control flow.
__global__ __launch_bounds__(256) void prop_extent_kernel(const unsigned long long* __restrict__ packed, int N, int words, int wpc,
                                                          int W, int HW, int32_t* __restrict__ raw) {
    __shared__ int part[4][5][64];
    const int m = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + m;
    const int w0 = blockIdx.y * wpc, w1 = min(words, w0 + wpc);
    int a = 0, pmin = HW, pmax = -1, xmin = W, xmax = -1;
    if (n < N)
        for (int w = w0 + ph; w < w1; w += 4) {
            const unsigned long long v = packed[(size_t)w * N + n];
            if (v == 0ull) continue;
            a += __popcll(v);
            const int base = w * 64;
            pmin = min(pmin, base + (int)__builtin_ctzll(v));
            pmax = max(pmax, base + 63 - (int)__builtin_clzll(v));
            // columns: split the word where it crosses image rows (two pieces at most once W >= 64)
            int x = base % W, off = 0;
            while (off < 64) {
                const int len = min(W - x, 64 - off);
                const unsigned long long seg = (v >> off) & (len == 64 ? ~0ull : ((1ull << len) - 1ull));
                if (seg != 0ull) {
                    xmin = min(xmin, x + (int)__builtin_ctzll(seg));
                    xmax = max(xmax, x + 63 - (int)__builtin_clzll(seg));
                }
                off += len;
                x = 0;
            }
        }
    part[ph][0][m] = a;
    part[ph][1][m] = HW - pmin;
    part[ph][2][m] = pmax + 1;
    part[ph][3][m] = W - xmin;
    part[ph][4][m] = xmax + 1;
    __syncthreads();
    if (ph == 0 && n < N) {
        int s = 0, r[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s += part[q][0][m];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = max(r[k], part[q][k + 1][m]);
        }
        if (s != 0) {
            atomicAdd(&raw[n], s);
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicMax(&raw[(size_t)(k + 1) * N + n], r[k]);
        }
    }
}

// ---- boxes, areas and the S x S masks -----------------------------------------------------------------------------------------
// One lane per (proposal, output cell).  Pillow's nearest resize (ImagingScaleAffine): step = (double) extent / S, the first
// coordinate step * 0.5, every further one the previous plus step, truncated; a coordinate outside the crop leaves 0.  The
// closed form floor((c + .5) w / S) differs from it at 26 of the widths below 1400.
#pragma clang fp contract(off)
__device__ __forceinline__ int pil_nearest(int extent, int S, int i) {
    const double step = (double)extent / (double)S;
    double o = step * 0.5;
    for (int k = 0; k < i; ++k) o += step;
    return (int)o;
}

__global__ __launch_bounds__(256) void prop_resize_kernel(const unsigned long long* __restrict__ packed, const int32_t* __restrict__ raw,
                                                          int N, int W, int HW, int S, int32_t* __restrict__ boxes,
                                                          int32_t* __restrict__ area, uint8_t* __restrict__ small, int32_t* __restrict__ empty_flag) {
    const int SS = S * S;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * SS) return;
    const int n = (int)(idx / SS), cell = (int)(idx % SS);
    const int a = raw[n];
    if (a == 0) {                                                         // the reference raises here (min of an empty array)
        if (cell == 0) {
            atomicMax(empty_flag, N - n);
            area[n] = 0;
            boxes[4 * n + 0] = boxes[4 * n + 1] = boxes[4 * n + 2] = boxes[4 * n + 3] = 0;
        }
        small[idx] = 0;
        return;
    }
    const int pmin = HW - raw[(size_t)N + n], pmax = raw[(size_t)2 * N + n] - 1;
    const int xmin = W - raw[(size_t)3 * N + n], xmax1 = raw[(size_t)4 * N + n];
    const int ymin = pmin / W, ymax1 = pmax / W + 1;
    if (cell == 0) {
        area[n] = a;
        boxes[4 * n + 0] = xmin;
        boxes[4 * n + 1] = ymin;
        boxes[4 * n + 2] = xmax1;
        boxes[4 * n + 3] = ymax1;
    }
    const int h = ymax1 - ymin, w = xmax1 - xmin;
    const int sy = pil_nearest(h, S, cell / S), sx = pil_nearest(w, S, cell % S);
    uint8_t bit = 0;
    if (sy < h && sx < w) {
        const int p = (ymin + sy) * W + xmin + sx;
        bit = (uint8_t)((packed[(size_t)(p >> 6) * N + n] >> (p & 63)) & 1ull);
    }
    small[idx] = bit;
}

// ---- cluster assignment -------------------------------------------------------------------------------------------------------
// (a) + (b): one wave per (64-pixel word column w, point j), four points per workgroup so that the column's N words are
// fetched by neighbours.  A lane is a pixel.  Per 64 masks: lane l loads mask n0 + l's word of column w and its word of the
// point's column (both 512 B contiguous rows of the word-major layout), the ballot of the point's bit is the membership of
// those 64 masks, and only the members' words are broadcast (v_readlane) and counted.  |sel_j| is the popcount of the ballots,
// so every wave knows it without a pass of its own.  avg [words][P] word-major like the masks; avg_area by atomicAdd.
__global__ __launch_bounds__(256) void prop_avg_kernel(const unsigned long long* __restrict__ packed, int N, int P, Points pts,
                                                       unsigned long long* __restrict__ avg, int32_t* __restrict__ avg_area) {
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (j >= P) return;
    const int w = blockIdx.x;
    const int pj = pts.pix[j];
    const unsigned long long* __restrict__ col = packed + (size_t)w * N;
    const unsigned long long* __restrict__ sel = packed + (size_t)(pj >> 6) * N;
    const int sb = pj & 63, lb = lane & 31;
    int cnt = 0, nsel = 0;
    for (int n0 = 0; n0 < N; n0 += 64) {
        const int n = n0 + lane;
        unsigned long long v = 0ull, s = 0ull;
        if (n < N) {
            v = col[n];
            s = sel[n];
        }
        unsigned long long members = __ballot((s >> sb) & 1ull);
        nsel += __popcll(members);
        const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
        while (members != 0ull) {
            const int k = (int)__builtin_ctzll(members);
            members &= members - 1ull;
            const unsigned ulo = (unsigned)__builtin_amdgcn_readlane(lo, k), uhi = (unsigned)__builtin_amdgcn_readlane(hi, k);
            cnt += (int)(((lane < 32 ? ulo : uhi) >> lb) & 1u);
        }
    }
    // mean(0) > 0.7 in fp64 == 10 cnt > 7 |sel| in integers (tests/test_proposal_prep_cpu.py walks every cnt <= n <= 2040);
    // |sel| = 0 is NaN > 0.7 in the reference: all false, as here (cnt = 0)
    const unsigned long long word = __ballot(10 * cnt > 7 * nsel);
    if (lane == 0) {
        avg[(size_t)w * P + j] = word;
        if (word != 0ull) atomicAdd(&avg_area[j], __popcll(word));
    }
}

// (c) inter[n][j] = popcount(m_n & avg_j): the and + popcount tile of mask_iou_pair_kernel with a thin second operand.
// grid = (ceil(N/64), word chunks, ceil(P/8)); 64 masks x 4 word phases per workgroup, 8 points per lane in registers, the avg
// words of a 32-word stage in LDS (every lane reads the same address: a broadcast).  Chunks meet by atomicAdd into zeroed inter.
constexpr int PT = 8, AWK = 32;
__global__ __launch_bounds__(256) void prop_inter_kernel(const unsigned long long* __restrict__ packed, int N, int words, int wpc,
                                                         const unsigned long long* __restrict__ avg, int P, int32_t* __restrict__ inter) {
    __shared__ __attribute__((aligned(16))) unsigned long long savg[AWK][PT];
    __shared__ int part[4][PT][64];
    const int tid = threadIdx.x, m = tid & 63, ph = tid >> 6;
    const int n = blockIdx.x * 64 + m;
    const int w0 = blockIdx.y * wpc, w1 = min(words, w0 + wpc);
    const int j0 = blockIdx.z * PT;
    int acc[PT] = {};
    for (int ws = w0; ws < w1; ws += AWK) {
        {
            const int wl = tid / PT, q = tid % PT;
            const int w = ws + wl, j = j0 + q;
            savg[wl][q] = (w < w1 && j < P) ? avg[(size_t)w * P + j] : 0ull;
        }
        __syncthreads();
        if (n < N) {
#pragma unroll
            for (int wl = 0; wl < AWK; wl += 4) {
                const int w = ws + wl + ph;
                if (w < w1) {
                    const unsigned long long v = packed[(size_t)w * N + n];
#pragma unroll
                    for (int q = 0; q < PT; ++q) acc[q] += __popcll(v & savg[wl + ph][q]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < PT; ++q) part[ph][q][m] = acc[q];
    __syncthreads();
    if (ph == 0 && n < N) {
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int s = part[0][q][m] + part[1][q][m] + part[2][q][m] + part[3][q][m];
            if (j0 + q < P && s != 0) atomicAdd(&inter[(size_t)n * P + j0 + q], s);
        }
    }
}

// (d) the sequential rule, one lane per proposal; mat arrives zeroed.  iou = f32(f64(inter) / f64(union)) as
// lib/utils/mask_utils.py:15-17 stores it; rows with iou > 0.5 take the point's cluster number, the last such point wins;
// rows that were 0 < iou <= 0.5 for some point and never assigned go to column 0 with number P + 1.
__global__ __launch_bounds__(256) void prop_assign_kernel(const int32_t* __restrict__ inter, const int32_t* __restrict__ area,
                                                          const int32_t* __restrict__ avg_area, int N, int P, int C, Points pts,
                                                          float* __restrict__ mat) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float* row = mat + (size_t)n * (C + 1);
    if (P == 0) {                                                         // point_level_label_assign.py:60-61
        row[0] = 1.0f;
        return;
    }
    const int an = area[n];
    int col = -1, id = 0;
    bool bg = false;
    for (int j = 0; j < P; ++j) {
        const int it = inter[(size_t)n * P + j];
        const int un = an + avg_area[j] - it;
        const float iou = (float)((double)it / (double)un);               // 0 / 0 (an empty proposal): NaN, neither branch
        if (iou > 0.5f) {
            col = pts.cls[j] + 1;
            id = j + 1;
        }
        bg = bg || (iou <= 0.5f && iou != 0.0f);
    }
    if (col >= 0) row[col] = (float)id;
    else if (bg) row[0] = (float)(P + 1);
}

struct WsLayout {
    size_t avg, avg_area, inter, total;
};
WsLayout ws_layout(int N, int HW, int P) {
    const size_t words = (size_t)(HW + 63) / 64;
    WsLayout l;
    l.avg = 0;
    l.avg_area = words * (size_t)P * 8;
    l.inter = l.avg_area + (((size_t)P * 4 + 7) & ~(size_t)7);
    l.total = l.inter + (size_t)N * P * 4;
    const size_t prep = (size_t)5 * N * 4;
    if (l.total < prep) l.total = prep;
    return l;
}

bool shape_ok(int N, int H, int W) {
    return N >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (long long)H * W <= CIM_SEGM_MAX_HW;
}

}  // namespace

extern "C" long long cim_prop_ws_bytes(int N, int HW, int P) {
    CIM_CHECK_ARG(N >= 1 && HW >= 1 && HW <= CIM_SEGM_MAX_HW && P >= 0 && P <= CIM_PROP_MAX_POINTS);
    return (long long)ws_layout(N, HW, P).total;
}

extern "C" int cim_prop_prepare(const uint8_t* masks_u8, int N, int H, int W, int S, uint64_t* packed, int32_t* boxes, int32_t* area,
                                uint8_t* small, int32_t* empty_flag, void* ws, void* stream) {
    CIM_CHECK_ARG(shape_ok(N, H, W));
    CIM_CHECK_ARG(S >= 1 && S <= CIM_PROP_MAX_S);
    CIM_CHECK_ARG(masks_u8 && packed && boxes && area && small && empty_flag && ws);
    const int HW = H * W, words = (HW + 63) / 64;
    hipStream_t st = cim::as_stream(stream);
    const int rc = cim_mask_pack(masks_u8, packed, N, HW, stream);       // the only launch that reads the byte masks
    if (rc != 0) return rc;
    int32_t* raw = static_cast<int32_t*>(ws);
    CIM_CHECK_HIP(hipMemsetAsync(raw, 0, sizeof(int32_t) * 5 * (size_t)N, st));
    CIM_CHECK_HIP(hipMemsetAsync(empty_flag, 0, sizeof(int32_t), st));
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(packed);
    const int groups = (N + 63) / 64;
    int chunks = (1024 + groups - 1) / groups;                           // ~1024 workgroups, at least 32 words each
    if (chunks > (words + 31) / 32) chunks = (words + 31) / 32;
    const int wpc = (words + chunks - 1) / chunks;
    hipLaunchKernelGGL(prop_extent_kernel, dim3(groups, (words + wpc - 1) / wpc), dim3(256), 0, st, p, N, words, wpc, W, HW, raw);
    const long long cells = (long long)N * S * S;
    hipLaunchKernelGGL(prop_resize_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, p, raw, N, W, HW, S, boxes, area,
                       small, empty_flag);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prop_assign(const uint64_t* packed, const int32_t* area, int N, int H, int W, const int32_t* rows,
                               const int32_t* cols, const int32_t* classes, int P, int C, float* mat, void* ws, void* stream) {
    CIM_CHECK_ARG(shape_ok(N, H, W));
    CIM_CHECK_ARG(P >= 0 && P <= CIM_PROP_MAX_POINTS && C >= 1 && C <= 32767);
    CIM_CHECK_ARG(packed && area && mat && ws);
    CIM_CHECK_ARG(P == 0 || (rows && cols && classes));
    Points pts;
    for (int j = 0; j < P; ++j) {
        CIM_CHECK_ARG(rows[j] >= 0 && rows[j] < H && cols[j] >= 0 && cols[j] < W);      // NumPy would wrap a negative index
        CIM_CHECK_ARG(classes[j] >= 0 && classes[j] < C);
        pts.pix[j] = rows[j] * W + cols[j];
        pts.cls[j] = (int16_t)classes[j];
    }
    for (int j = P; j < CIM_PROP_MAX_POINTS; ++j) {
        pts.pix[j] = 0;
        pts.cls[j] = 0;
    }
    const int HW = H * W, words = (HW + 63) / 64;
    hipStream_t st = cim::as_stream(stream);
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(packed);
    CIM_CHECK_HIP(hipMemsetAsync(mat, 0, sizeof(float) * (size_t)N * (C + 1), st));
    const WsLayout l = ws_layout(N, HW, P);
    char* base = static_cast<char*>(ws);
    unsigned long long* avg = reinterpret_cast<unsigned long long*>(base + l.avg);
    int32_t* avg_area = reinterpret_cast<int32_t*>(base + l.avg_area);
    int32_t* inter = reinterpret_cast<int32_t*>(base + l.inter);
    if (P > 0) {
        CIM_CHECK_HIP(hipMemsetAsync(avg_area, 0, l.total - l.avg_area, st));           // avg_area and inter
        hipLaunchKernelGGL(prop_avg_kernel, dim3(words, (P + 3) / 4), dim3(256), 0, st, p, N, P, pts, avg, avg_area);
        const int groups = (N + 63) / 64, pgroups = (P + PT - 1) / PT;
        int chunks = (1024 + groups * pgroups - 1) / (groups * pgroups);
        if (chunks > (words + AWK - 1) / AWK) chunks = (words + AWK - 1) / AWK;
        const int wpc = (words + chunks - 1) / chunks;
        hipLaunchKernelGGL(prop_inter_kernel, dim3(groups, (words + wpc - 1) / wpc, pgroups), dim3(256), 0, st, p, N, words, wpc, avg, P,
                           inter);
    }
    hipLaunchKernelGGL(prop_assign_kernel, dim3((N + 255) / 256), dim3(256), 0, st, inter, area, avg_area, N, P, C, pts, mat);
    CIM_CHECK_LAUNCH();
    return 0;
}
