// Polygon ground truth for mask AP on gfx950: COCO's polygon fill (rleFrPoly of maskApi.c, then merge as a union) from flat
// fp64 polygon coordinates straight to the packed column-major masks of csrc/segm_eval.hip - the stage pycocotools'
// annToRLE / frPyObjects runs before COCOeval(..., 'segm') on annotation files that store polygons
// (tools/evaluation.py:158,174).  Exactness contract (bit-identical to tests/golden/poly_np.py): DESIGN.md 4.12,
// include/cim_hip.h.
//
// A polygon's edges are walked as "dense points" (one per step of the longer axis on a grid 5 x finer than the pixels); a
// change of column between two neighbouring points is a crossing at a linear pixel position a, and pixel p is set iff an odd
// number of crossings lie at positions <= p.  So the published sort / difference / merge-zero-runs ending is a prefix parity:
//   poly_cross_kernel   one lane per dense point: its edge by a binary search over the edge-length prefix, the point and its
//                       predecessor recomputed from the rounded vertices, one atomicXor of bit a into the polygon's zeroed
//                       scratch words (crossings at one position cancel, which is the merge of zero-length runs)
//   poly_fill_kernel    one workgroup per polygon: prefix-XOR inside each word by shifts, the parity of whole words carried
//                       across lanes by a ballot and across waves through LDS, bits past H W cleared, atomicOr into the
//                       annotation's mask (polygons of one annotation overlap as a union)
// No sort, no host synchronisation, no per-annotation launch.
#pragma clang fp contract(off)                      // ys + s * t + .5 and 5 x + .5: no fused operations
#include "common.h"
#include "../../include/cim_hip.h"

namespace {

typedef unsigned long long u64;

struct Pt {
    int u, v;
};

// (int)(5 c + .5), truncating toward zero
__device__ __forceinline__ int scaled(double c) { return (int)(5.0 * c + .5); }

__device__ __forceinline__ int edge_steps(int xs, int ys, int xe, int ye) {
    const int dx = abs(xe - xs), dy = abs(ye - ys);
    return dx >= dy ? dx : dy;
}

// dense point d (0 .. edge_steps) of the edge (xs, ys) -> (xe, ye): rleFrPoly's first loop nest
__device__ __forceinline__ Pt edge_point(int xs, int ys, int xe, int ye, int d) {
    const int dx = abs(xe - xs), dy = abs(ye - ys);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) {
        int t = xs;
        xs = xe;
        xe = t;
        t = ys;
        ys = ye;
        ye = t;
    }
    Pt p;
    if (dx == 0 && dy == 0) {                                            // (s = 0 / 0 in the published code; v defined as ys)
        p.u = xs;
        p.v = ys;
    } else if (dx >= dy) {
        const double s = (double)(ye - ys) / dx;
        const int t = flip ? dx - d : d;
        p.u = t + xs;
        p.v = (int)(ys + s * t + .5);
    } else {
        const double s = (double)(xe - xs) / dy;
        const int t = flip ? dy - d : d;
        p.v = t + ys;
        p.u = (int)(xs + s * t + .5);
    }
    return p;
}

// last index i in [0, n) with off[i] <= key (off ascending, off[0] <= key)
__device__ __forceinline__ int last_le(const int* __restrict__ off, int n, long long key) {
    int a = 0, b = n - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if ((long long)off[mid] <= key) a = mid;
        else b = mid - 1;
    }
    return a;
}

__global__ __launch_bounds__(256) void poly_cross_kernel(const double* __restrict__ xy, const int* __restrict__ poly_off,
                                                         const int* __restrict__ edge_off, int n_poly, int n_vert,
                                                         long long n_points, int H, int W, int words,
                                                         u64* __restrict__ scratch) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_points) return;
    const int e = last_le(edge_off, n_vert, g);                          // edge e starts at vertex e
    const int p = last_le(poly_off, n_poly, e);
    const int lo = poly_off[p], hi = poly_off[p + 1];
    if (lo < 0 || hi > n_vert || e < lo || e >= hi) return;              // (offsets that do not fit: nothing is read past n_vert)
    const int d = (int)(g - edge_off[e]);
    if (e == lo && d == 0) return;                                       // the polygon's first point has no predecessor
    const int e1 = e + 1 < hi ? e + 1 : lo;                              // the edge's end: the next vertex, or the first again
    const int xs = scaled(xy[2 * (size_t)e]), ys = scaled(xy[2 * (size_t)e + 1]);
    const int xe = scaled(xy[2 * (size_t)e1]), ye = scaled(xy[2 * (size_t)e1 + 1]);
    const Pt cur = edge_point(xs, ys, xe, ye, d);
    Pt prev;
    if (d > 0) {
        prev = edge_point(xs, ys, xe, ye, d - 1);
    } else {                                                             // the last point of the edge before (not assumed equal
        const int x0 = scaled(xy[2 * (size_t)(e - 1)]), y0 = scaled(xy[2 * (size_t)(e - 1) + 1]);    // to this edge's first)
        prev = edge_point(x0, y0, xs, ys, edge_steps(x0, y0, xs, ys));
    }
    if (cur.u == prev.u) return;
    double xd = (double)(cur.u < prev.u ? cur.u : cur.u - 1);
    xd = (xd + .5) / 5.0 - .5;
    if (floor(xd) != xd || xd < 0 || xd > W - 1) return;
    double yd = (double)(cur.v < prev.v ? cur.v : prev.v);
    yd = (yd + .5) / 5.0 - .5;
    if (yd < 0) yd = 0;
    else if (yd > H) yd = H;
    yd = ceil(yd);
    const long long a = (long long)(int)xd * H + (int)yd;                // yd == H: the first pixel of the next column
    if (a >= (long long)H * W) return;                                   // ... or off the end of the image
    atomicXor(&scratch[(size_t)p * words + (size_t)(a >> 6)], 1ull << (a & 63));
}

__global__ __launch_bounds__(256) void poly_fill_kernel(const u64* __restrict__ scratch, const int* __restrict__ poly_ann,
                                                        int n_ann, int words, long long HW, u64* __restrict__ packed) {
    __shared__ int s_par[4];
    const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ann = poly_ann[p];
    if (ann < 0 || ann >= n_ann) return;                                 // (workgroup-uniform)
    const u64* src = scratch + (size_t)p * words;
    u64* dst = packed + (size_t)ann * words;
    int carry = 0;                                                       // parity of the crossings in the words before w0
    for (int w0 = 0; w0 < words; w0 += 256) {
        const int w = w0 + (int)threadIdx.x;
        u64 v = w < words ? src[w] : 0ull;
        v ^= v << 1;                                                     // bit j = parity of bits 0 .. j
        v ^= v << 2;
        v ^= v << 4;
        v ^= v << 8;
        v ^= v << 16;
        v ^= v << 32;
        const u64 odd = __ballot((v >> 63) != 0ull);                     // lanes whose word holds an odd number of crossings
        if (lane == 0) s_par[wave] = __popcll(odd) & 1;
        __syncthreads();
        int before = carry ^ (__popcll(odd & ((1ull << lane) - 1ull)) & 1);
        for (int k = 0; k < wave; ++k) before ^= s_par[k];
        carry ^= s_par[0] ^ s_par[1] ^ s_par[2] ^ s_par[3];
        __syncthreads();                                                 // (s_par is rewritten by the next round)
        if (before) v = ~v;
        if (w < words) {
            const long long rem = HW - (long long)w * 64;
            if (rem < 64) v &= (1ull << rem) - 1ull;                     // bits past H W stay 0
            if (v) atomicOr(&dst[w], v);
        }
    }
}

bool shape_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= CIM_SEGM_MAX_HW; }

}  // namespace

extern "C" long long cim_poly_ws_bytes(int n_poly, int H, int W) {
    if (!shape_ok(H, W) || n_poly < 0) {
        cim::set_error("cim_poly_ws_bytes: need n_poly >= 0, H, W >= 1 and H * W <= %d (n_poly=%d, H=%d, W=%d)", CIM_SEGM_MAX_HW,
                       n_poly, H, W);
        return -1;
    }
    return 8ll * n_poly * (((long long)H * W + 63) / 64) + 8;
}

extern "C" int cim_poly_fill(const double* xy, const int32_t* poly_off, const int32_t* poly_ann, const int32_t* edge_off,
                             int n_poly, int n_vert, long long n_points, int n_ann, int H, int W, void* ws, uint64_t* packed,
                             void* stream) {
    if (!shape_ok(H, W)) {
        cim::set_error("cim_poly_fill: need H, W >= 1 and H * W <= %d (H=%d, W=%d)", CIM_SEGM_MAX_HW, H, W);
        return -1;
    }
    if (n_points < 0 || n_points > CIM_POLY_MAX_POINTS) {
        cim::set_error("cim_poly_fill: %lld dense points in one call, the limit is %d", n_points, CIM_POLY_MAX_POINTS);
        return -1;
    }
    if (n_poly < 0 || n_ann < 0 || n_vert < 3ll * n_poly || n_points < n_vert || (n_poly == 0 && n_vert != 0)) {
        cim::set_error("cim_poly_fill: need n_poly, n_ann >= 0, >= 3 vertices per polygon and >= 1 dense point per vertex "
                       "(n_poly=%d, n_ann=%d, n_vert=%d, n_points=%lld)", n_poly, n_ann, n_vert, n_points);
        return -1;
    }
    if (n_ann == 0) return 0;
    CIM_CHECK_ARG(packed && ((uintptr_t)packed & 7) == 0);
    hipStream_t st = cim::as_stream(stream);
    const long long HW = (long long)H * W;
    const int words = (int)((HW + 63) / 64);
    CIM_CHECK_HIP(hipMemsetAsync(packed, 0, 8 * (size_t)n_ann * words, st));
    if (n_poly == 0) return 0;
    CIM_CHECK_ARG(xy && poly_off && poly_ann && edge_off && ws && ((uintptr_t)ws & 7) == 0);
    u64* scratch = static_cast<u64*>(ws);
    CIM_CHECK_HIP(hipMemsetAsync(scratch, 0, 8 * (size_t)n_poly * words, st));
    hipLaunchKernelGGL(poly_cross_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, st, xy, poly_off, edge_off, n_poly,
                       n_vert, n_points, H, W, words, scratch);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(poly_fill_kernel, dim3(n_poly), dim3(256), 0, st, scratch, poly_ann, n_ann, words, HW,
                       reinterpret_cast<u64*>(packed));
    CIM_CHECK_LAUNCH();
    return 0;
}
