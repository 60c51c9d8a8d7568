// PRM peak back-propagation for gfx950: the element-wise stages and the stem's data gradient of the peak response maps.
//
// Replaces what PeakResponseMapping(...).inference() does after its forward pass (lib/prm/prm_model_gt.py:249-310): P sequential
// backward(retain_graph=True) passes through convolutions patched by lib/prm/prm_modules.py:104-140 (PreHook / PostHook /
// pr_conv2d).  Here ONE backward walk whose batch dimension is the peaks: the tensors of the forward pass (xs = x - min x, the
// post-activation y, the normaliser n = conv(xs, W+)) belong to the image and are shared by every peak; the gradients are
// [P, C, HW].  The heavy products are the existing data gradients (conv1x1.hip) with w = W+; this file holds what they lack:
//
//   min / shift     o = min x into a device scalar (two launches, no host read), xs = x - o
//   gate            g [P,C,HW] -> dconv = ghat of the rule (ReLU gate, BatchNorm scale a, the division by |n| + 1e-10 with its
//                   n < 1e-10 -> 0 mask), optionally multiplied by the consumer's xs on the way in and with the ReLU-gated
//                   gradient of the identity branch (dres) on the way out; the shared tensors are read once per launch
//   scale           dx = xs * dxraw (+ the other branch's gradient)
//   seed            the peaks' one-hot seeds through the adjoint of prm_upsample_kernel's index arithmetic and the classifier's gate
//   stem            the 7 x 7 / stride 2 / pad 3 data gradient with W+, fused with the multiply by xs, the sum over the 3 input
//                   channels and the clamp; per-workgroup partial sums in double, added in a fixed order by the normalising launch
//
// VALU / LDS work, no MFMA, no atomics, every sum in a fixed order: the same bits on every call.  Contract: DESIGN.md 4.25.
#include "common.h"
#include "../../include/cim_hip.h"

namespace {

#pragma clang fp contract(off)

constexpr int THREADS = 256;
constexpr float PR_EPS = 1e-10f;                   // prm_modules.py:126

// ---- min / shift ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_min(float v, float* s_part) {
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(s_part[0], s_part[1]), fminf(s_part[2], s_part[3]));
}

__global__ __launch_bounds__(THREADS) void prmb_min_part_kernel(const float* __restrict__ x, long long n, float* __restrict__ part) {
    __shared__ float s_part[THREADS / 64];
    float v = INFINITY;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) v = fminf(v, x[i]);
    v = block_min(v, s_part);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(THREADS) void prmb_min_finish_kernel(const float* __restrict__ part, int parts, float* __restrict__ out) {
    __shared__ float s_part[THREADS / 64];
    float v = INFINITY;
    for (int i = threadIdx.x; i < parts; i += THREADS) v = fminf(v, part[i]);
    v = block_min(v, s_part);
    if (threadIdx.x == 0) out[0] = v;
}

__global__ __launch_bounds__(THREADS) void prmb_shift_kernel(const float* __restrict__ x, const float* __restrict__ o,
                                                             float* __restrict__ xs, long long n) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) xs[i] = x[i] - o[0];
}

// ---- gate ---------------------------------------------------------------------------------------------------------------------
// ghat of one element: the ReLU gate of the layer's own output, its BatchNorm scale, then PostHook's backward.
__device__ __forceinline__ float gate_one(float g, bool open, bool has_a, float a, float n, float& res) {
    const float t = open ? g : 0.f;
    res = t;
    const float d = has_a ? t * a : t;
    return n < PR_EPS ? 0.f : d / (fabsf(n) + PR_EPS);
}

// One lane owns V consecutive elements of the [C, HW] plane set and walks the P peaks: y, n, mul and a are read once.
template <int V>
__global__ __launch_bounds__(THREADS) void prmb_gate_kernel(const float* __restrict__ g, const float* __restrict__ mul,
                                                            const float* __restrict__ y, const float* __restrict__ a,
                                                            const float* __restrict__ n, float* __restrict__ dconv,
                                                            float* __restrict__ dres, int P, long long CHW, long long HW) {
    const long long e = ((long long)blockIdx.x * THREADS + threadIdx.x) * V;
    if (e >= CHW) return;
    float nv[V], mv[V], av[V];
    bool open[V];
    for (int k = 0; k < V; ++k) {
        nv[k] = n[e + k];
        mv[k] = mul ? mul[e + k] : 1.f;
        open[k] = y ? y[e + k] > 0.f : true;
        av[k] = a ? a[(e + k) / HW] : 1.f;
    }
    for (int p = 0; p < P; ++p) {
        const long long at = (long long)p * CHW + e;
        float gv[V], dv[V], rv[V];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(g + at);
            gv[0] = t.x; gv[1] = t.y; gv[2] = t.z; gv[3] = t.w;
        } else {
            gv[0] = g[at];
        }
        for (int k = 0; k < V; ++k) dv[k] = gate_one(mul ? mv[k] * gv[k] : gv[k], open[k], a != nullptr, av[k], nv[k], rv[k]);
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(dconv + at) = make_float4(dv[0], dv[1], dv[2], dv[3]);
            if (dres) *reinterpret_cast<float4*>(dres + at) = make_float4(rv[0], rv[1], rv[2], rv[3]);
        } else {
            dconv[at] = dv[0];
            if (dres) dres[at] = rv[0];
        }
    }
}

// ---- scale --------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(THREADS) void prmb_scale_kernel(const float* __restrict__ xs, const float* __restrict__ dxraw,
                                                             const float* __restrict__ add, float* __restrict__ dx, int P, long long n) {
    const long long e = ((long long)blockIdx.x * THREADS + threadIdx.x) * V;
    if (e >= n) return;
    float xv[V];
    for (int k = 0; k < V; ++k) xv[k] = xs[e + k];
    for (int p = 0; p < P; ++p) {
        const long long at = (long long)p * n + e;
        if constexpr (V == 4) {
            const float4 r = *reinterpret_cast<const float4*>(dxraw + at);
            float4 o = make_float4(xv[0] * r.x, xv[1] * r.y, xv[2] * r.z, xv[3] * r.w);
            if (add) {
                const float4 q = *reinterpret_cast<const float4*>(add + at);
                o = make_float4(o.x + q.x, o.y + q.y, o.z + q.z, o.w + q.w);
            }
            *reinterpret_cast<float4*>(dx + at) = o;
        } else {
            const float o = xv[0] * dxraw[at];
            dx[at] = add ? o + add[at] : o;
        }
    }
}

// ---- seed ---------------------------------------------------------------------------------------------------------------------
// One axis of prm_upsample_kernel's taps for output index o (prm.hip): (i0, i1, l0, l1).
struct Tap { int i0, i1; float l0, l1; };
__device__ __forceinline__ Tap tap_of(float scale, int o, int n_in) {
    const float f = scale * (float)o;
    Tap t;
    t.i0 = min((int)f, n_in - 1);
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = f - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// dconv [P, C, h, w]: the adjoint of up = (v00 l0x + v01 l1x) l0y + (v10 l0x + v11 l1x) l1y at the peak - the four products
// l?x l?y added to their tap pixels in the order 00, 01, 10, 11 (taps that coincide at a border add up) - then the classifier's
// gate.  A peak outside the grid or the classes seeds nothing (the host entry refuses it first).
__global__ __launch_bounds__(THREADS) void prmb_seed_kernel(const int32_t* __restrict__ peaks, const float* __restrict__ n,
                                                            float* __restrict__ dconv, int P, int C, int h, int w, int H, int W,
                                                            float sy, float sx) {
    const long long chw = (long long)C * h * w;
    const long long idx = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (long long)P * chw) return;
    const int p = (int)(idx / chw);
    const long long e = idx - (long long)p * chw;
    const int c = (int)(e / (h * w)), pix = (int)(e % (h * w)), i = pix / w, j = pix % w;
    const int pc = peaks[3 * p], py = peaks[3 * p + 1], px = peaks[3 * p + 2];
    float acc = 0.f;
    if (c == pc && py >= 0 && py < H && px >= 0 && px < W) {
        const Tap ty = tap_of(sy, py, h), tx = tap_of(sx, px, w);
        if (i == ty.i0 && j == tx.i0) acc = acc + tx.l0 * ty.l0;
        if (i == ty.i0 && j == tx.i1) acc = acc + tx.l1 * ty.l0;
        if (i == ty.i1 && j == tx.i0) acc = acc + tx.l0 * ty.l1;
        if (i == ty.i1 && j == tx.i1) acc = acc + tx.l1 * ty.l1;
    }
    float unused;
    dconv[idx] = gate_one(acc, true, false, 1.f, n[e], unused);
}

// ---- stem ---------------------------------------------------------------------------------------------------------------------
// out[p][y][x] = max(0, sum_ci xs[ci][y][x] * sum_{co,ky,kx} ghat[p][co][(y + 3 - ky) / 2][(x + 3 - kx) / 2] W+[co][ci][ky][kx])
// over the taps whose (y + 3 - ky), (x + 3 - kx) are even and inside the Ho x Wo grid.
// A workgroup owns an 8 x 32 tile of image pixels of one peak.  Its four waves are the four parity classes (y & 1, x & 1) of the
// tile: inside a wave every lane takes the same taps (3 or 4 per axis), so the weights are wave-uniform (scalar loads from the
// [cout][3][7][7] array as it is) and there is no divergence; ghat comes from an LDS patch of 7 x 19 output pixels per channel,
// staged CO channels at a time with zeros outside the grid (no bounds test in the tap loops).
constexpr int ST_TY = 8, ST_TX = 32, ST_PH = 7, ST_PW = 19, ST_CO = 16;

template <int NKY, int NKX>
__device__ __forceinline__ void stem_taps(const float* __restrict__ patch, const float* __restrict__ wc, int ky0, int kx0, int ry, int rx,
                                          float& a0, float& a1, float& a2) {
    // patch: one channel's [ST_PH][ST_PW]; wc: that channel's [3][49] weights; (ry, rx): the patch position of tap (ky0, kx0)
#pragma unroll
    for (int t = 0; t < NKY; ++t) {
#pragma unroll
        for (int u = 0; u < NKX; ++u) {
            const float gv = patch[(ry - t) * ST_PW + (rx - u)];
            const int k = (ky0 + 2 * t) * 7 + kx0 + 2 * u;
            a0 = fmaf(gv, wc[k], a0);
            a1 = fmaf(gv, wc[49 + k], a1);
            a2 = fmaf(gv, wc[98 + k], a2);
        }
    }
}

__global__ __launch_bounds__(THREADS) void prmb_stem_kernel(const float* __restrict__ ghat, const float* __restrict__ wpos,
                                                            const float* __restrict__ xs, float* __restrict__ out,
                                                            double* __restrict__ part, int cout, int H, int W, int Ho, int Wo) {
    __shared__ float s_patch[ST_CO][ST_PH * ST_PW];
    __shared__ double s_sum[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int cls = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform: the parity class
    const int py = cls >> 1, px = cls & 1;
    const int p = blockIdx.z, y0 = blockIdx.y * ST_TY, x0 = blockIdx.x * ST_TX;
    const int y = y0 + 2 * (lane >> 4) + py, x = x0 + 2 * (lane & 15) + px;
    const int oy_base = y0 / 2 - 1, ox_base = x0 / 2 - 1;
    // taps of this class: ky of the parity of y + 3, starting at ky0 = (py + 1) & 1; tap t reads output row (y + 3 - ky0) / 2 - t
    const int ky0 = (py + 1) & 1, kx0 = (px + 1) & 1;
    const int ry = (y + 3 - ky0) / 2 - oy_base, rx = (x + 3 - kx0) / 2 - ox_base;
    const float* __restrict__ gp = ghat + (size_t)p * cout * Ho * Wo;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int c0 = 0; c0 < cout; c0 += ST_CO) {
        const int nc = min(ST_CO, cout - c0);
        __syncthreads();
        for (int i = tid; i < nc * ST_PH * ST_PW; i += THREADS) {
            const int c = i / (ST_PH * ST_PW), r = i % (ST_PH * ST_PW);
            const int oy = oy_base + r / ST_PW, ox = ox_base + r % ST_PW;
            s_patch[c][r] = (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) ? gp[((size_t)(c0 + c) * Ho + oy) * Wo + ox] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const float* __restrict__ wc = wpos + (size_t)(c0 + c) * 147;
            if (ky0 == 0) {
                if (kx0 == 0) stem_taps<4, 4>(s_patch[c], wc, 0, 0, ry, rx, a0, a1, a2);
                else stem_taps<4, 3>(s_patch[c], wc, 0, 1, ry, rx, a0, a1, a2);
            } else {
                if (kx0 == 0) stem_taps<3, 4>(s_patch[c], wc, 1, 0, ry, rx, a0, a1, a2);
                else stem_taps<3, 3>(s_patch[c], wc, 1, 1, ry, rx, a0, a1, a2);
            }
        }
    }
    float s = 0.f;
    if (y < H && x < W) {
        const size_t hw = (size_t)H * W, at = (size_t)y * W + x;
        s = xs[at] * a0;
        s = s + xs[hw + at] * a1;
        s = s + xs[2 * hw + at] * a2;
        s = s < 0.f ? 0.f : s;                                  // clamp(min = 0): a NaN stays
        out[(size_t)p * hw + at] = s;
    }
    double d = (double)s;
    for (int k = 32; k >= 1; k >>= 1) d += __shfl_xor(d, k);
    if (lane == 0) s_sum[tid >> 6] = d;
    __syncthreads();
    if (tid == 0) part[((size_t)p * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
}

// out[p] /= sum of its partials: every workgroup adds the peak's partials in the same fixed order (a strided pass, then a tree).
__global__ __launch_bounds__(THREADS) void prmb_stem_norm_kernel(float* __restrict__ out, const double* __restrict__ part, int parts,
                                                                 long long HW) {
    __shared__ double s_sum[THREADS];
    const int p = blockIdx.y, tid = threadIdx.x;
    double d = 0.0;
    for (int i = tid; i < parts; i += THREADS) d += part[(size_t)p * parts + i];
    s_sum[tid] = d;
    __syncthreads();
    for (int k = THREADS / 2; k >= 1; k >>= 1) {
        if (tid < k) s_sum[tid] += s_sum[tid + k];
        __syncthreads();
    }
    const float total = (float)s_sum[0];
    const long long i = (long long)blockIdx.x * THREADS + tid;
    if (i < HW) out[(size_t)p * HW + i] = out[(size_t)p * HW + i] / total;            // 0 / 0 = NaN, as the reference
}

inline bool aligned16(const void* q) { return q == nullptr || ((size_t)q & 15) == 0; }
inline unsigned blocks_for(long long n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace

extern "C" long long cim_prmb_min_parts(long long n) {
    if (n < 1) return -1;
    const long long b = (n + THREADS - 1) / THREADS;
    return b < CIM_PRMB_MIN_MAX_PARTS ? b : CIM_PRMB_MIN_MAX_PARTS;
}

extern "C" int cim_prmb_min(const float* x, long long n, float* out, float* part, void* stream) {
    CIM_CHECK_ARG(x && out && part && n >= 1);
    const int parts = (int)cim_prmb_min_parts(n);
    hipStream_t st = cim::as_stream(stream);
    hipLaunchKernelGGL(prmb_min_part_kernel, dim3((unsigned)parts), dim3(THREADS), 0, st, x, n, part);
    hipLaunchKernelGGL(prmb_min_finish_kernel, dim3(1), dim3(THREADS), 0, st, part, parts, out);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prmb_shift(const float* x, const float* o, float* xs, long long n, void* stream) {
    CIM_CHECK_ARG(x && o && xs && n >= 1 && n < (1ll << 31));          // (one lane per element: the grid of one launch)
    hipLaunchKernelGGL(prmb_shift_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, cim::as_stream(stream), x, o, xs, n);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prmb_gate(const float* g, const float* mul, const float* y, const float* a, const float* n, float* dconv,
                             float* dres, int P, int C, long long HW, void* stream) {
    CIM_CHECK_ARG(g && n && dconv && P >= 1 && C >= 1 && HW >= 1 && (long long)C * HW < (1ll << 31) && (long long)P * C * HW < (1ll << 40));
    const long long chw = (long long)C * HW;
    hipStream_t st = cim::as_stream(stream);
    const bool vec = HW % 4 == 0 && aligned16(g) && aligned16(mul) && aligned16(y) && aligned16(n) && aligned16(dconv) && aligned16(dres);
    if (vec)
        hipLaunchKernelGGL(prmb_gate_kernel<4>, dim3(blocks_for(chw / 4)), dim3(THREADS), 0, st, g, mul, y, a, n, dconv, dres, P, chw, HW);
    else
        hipLaunchKernelGGL(prmb_gate_kernel<1>, dim3(blocks_for(chw)), dim3(THREADS), 0, st, g, mul, y, a, n, dconv, dres, P, chw, HW);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prmb_scale(const float* xs, const float* dxraw, const float* add, float* dx, int P, long long n, void* stream) {
    CIM_CHECK_ARG(xs && dxraw && dx && P >= 1 && n >= 1 && n < (1ll << 31) && (long long)P * n < (1ll << 40));
    hipStream_t st = cim::as_stream(stream);
    const bool vec = n % 4 == 0 && aligned16(xs) && aligned16(dxraw) && aligned16(add) && aligned16(dx);
    if (vec)
        hipLaunchKernelGGL(prmb_scale_kernel<4>, dim3(blocks_for(n / 4)), dim3(THREADS), 0, st, xs, dxraw, add, dx, P, n);
    else
        hipLaunchKernelGGL(prmb_scale_kernel<1>, dim3(blocks_for(n)), dim3(THREADS), 0, st, xs, dxraw, add, dx, P, n);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_prmb_seed(const int32_t* peaks_dev, const float* n, float* dconv, int P, int C, int h, int w, int factor,
                             void* stream) {
    CIM_CHECK_ARG(peaks_dev && n && dconv && P >= 1 && C >= 1 && h >= 1 && w >= 1 && factor >= 1);
    CIM_CHECK_ARG((long long)h * factor * w * factor <= CIM_PRM_MAX_HW && (long long)P * C * h * w < (1ll << 31));       // (one lane per element)
    const int H = h * factor, W = w * factor;
    // (the scales of cim_prm_upsample: (n_in - 1) / (n_out - 1) in double, rounded to fp32; 0 for a single output pixel)
    const float sy = H > 1 ? (float)((double)(h - 1) / (double)(H - 1)) : 0.f;
    const float sx = W > 1 ? (float)((double)(w - 1) / (double)(W - 1)) : 0.f;
    const long long total = (long long)P * C * h * w;
    hipLaunchKernelGGL(prmb_seed_kernel, dim3(blocks_for(total)), dim3(THREADS), 0, cim::as_stream(stream), peaks_dev, n, dconv, P, C, h, w,
                       H, W, sy, sx);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" long long cim_prmb_stem_workspace(int P, int H, int W) {
    if (P < 1 || H < 1 || W < 1) return -1;
    return (long long)sizeof(double) * P * ((H + ST_TY - 1) / ST_TY) * ((W + ST_TX - 1) / ST_TX);
}

extern "C" int cim_prmb_stem(const float* ghat, const float* wpos, const float* xs, float* out, void* workspace, int P, int cout,
                             int H, int W, int normalise, void* stream) {
    CIM_CHECK_ARG(ghat && wpos && xs && out && workspace && ((size_t)workspace & 7) == 0);
    CIM_CHECK_ARG(P >= 1 && P <= 65535 && cout >= 1 && cout <= 256 && H >= 1 && W >= 1 && W <= 4096 && (long long)H * W < (1ll << 22));
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const dim3 grid((unsigned)((W + ST_TX - 1) / ST_TX), (unsigned)((H + ST_TY - 1) / ST_TY), (unsigned)P);
    CIM_CHECK_ARG(grid.y <= 65535);
    hipStream_t st = cim::as_stream(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(prmb_stem_kernel, grid, dim3(THREADS), 0, st, ghat, wpos, xs, out, part, cout, H, W, Ho, Wo);
    if (normalise)
        hipLaunchKernelGGL(prmb_stem_norm_kernel, dim3(blocks_for((long long)H * W), (unsigned)P), dim3(THREADS), 0, st, out, part,
                           (int)(grid.x * grid.y), (long long)H * W);
    CIM_CHECK_LAUNCH();
    return 0;
}
