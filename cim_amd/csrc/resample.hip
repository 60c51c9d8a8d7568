// Pillow's antialiased resize for gfx950: raw RGB bytes of differing sizes -> the PRM's normalised input.
//
// Replaces the host call Image.resize((448, 448), Image.BILINEAR) of tools/pre/AGPL_label_assign.py (prm_configs.open_transform:
// transforms.Resize([448, 448]) + ToTensor + Normalize) for a BATCH of images.  The arithmetic is Pillow's
// src/libImaging/Resample.c on 8-bit images - precompute_coeffs with the bilinear filter (support 1), normalize_coeffs_8bpc,
// ImagingResampleHorizontal_8bpc, ImagingResampleVertical_8bpc - restated in tests/golden/pil_resample_np.py and bit-identical
// to Pillow for every source with h <= 100 w (beyond that Pillow runs the vertical pass first: refused here).
//
// Three launches for a batch, whatever its size: (a) the coefficient tables, one lane per (image, axis, output index), in fp64
// exactly as Pillow's C computes them; (b) the horizontal pass, one lane per intermediate pixel; (c) the vertical pass with the
// ToTensor + Normalize epilogue of image_prep.hip, one lane per output pixel.  An axis whose size does not change goes through
// its table like any other: at scale 1 the table is one tap of weight 2^22 on the sample itself, i.e. a copy.
// Byte traffic (about 3 MB per image), integer VALU work; no LDS, no MFMA, no scratch.
#include "common.h"
#include "../../include/cim_hip.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_BITS = CIM_RESAMPLE_PRECISION_BITS;

// Workspace: inter_off int64 [B] | bounds_x int32 [B][out_w][2] | bounds_y [B][out_h][2] | coef_x int32 [B][out_w][KX] |
// coef_y [B][out_h][KY] | the uint8 intermediates [h_b][out_w][3], image after image.  KX / KY: the longest table row of the batch.
struct Layout {
    int KX, KY, Hmax;
    size_t bounds_x, bounds_y, coef_x, coef_y, inter, total;
};

int ksize_of(int n_in, int n_out) {
    const double scale = (double)n_in / (double)n_out;
    const double support = 1.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

// desc_host: int64 [B][3] = (byte offset into src, h, w)
bool plan(const int64_t* d, int B, int out_w, int out_h, Layout& L) {
    if (B < 1 || B > 65535 || d == nullptr) {
        cim::set_error("cim_resample: B = %d images, 1..65535 are taken (and a host descriptor)", B);
        return false;
    }
    if (out_w < 1 || out_w > CIM_RESAMPLE_MAX_DST || out_h < 1 || out_h > CIM_RESAMPLE_MAX_DST) {
        cim::set_error("cim_resample: output %d x %d, sides must be 1..%d", out_w, out_h, CIM_RESAMPLE_MAX_DST);
        return false;
    }
    L.KX = L.KY = L.Hmax = 0;
    size_t rows = 0;
    int64_t end = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t off = d[3 * b], h = d[3 * b + 1], w = d[3 * b + 2];
        if (h < 1 || h > CIM_RESAMPLE_MAX_SRC || w < 1 || w > CIM_RESAMPLE_MAX_SRC) {
            cim::set_error("cim_resample: image %d is %lld x %lld, sides must be 1..%d", b, (long long)h, (long long)w, CIM_RESAMPLE_MAX_SRC);
            return false;
        }
        if (h > (int64_t)CIM_RESAMPLE_MAX_ASPECT * w) {
            cim::set_error("cim_resample: image %d is %lld x %lld: h > %d w, where Pillow runs the vertical pass first (refused)", b,
                           (long long)h, (long long)w, CIM_RESAMPLE_MAX_ASPECT);
            return false;
        }
        if (off < end) {
            cim::set_error("cim_resample: image %d starts at byte %lld, before the end of its predecessor (%lld): offsets must ascend", b,
                           (long long)off, (long long)end);
            return false;
        }
        end = off + h * w * 3;
        const int kx = ksize_of((int)w, out_w), ky = ksize_of((int)h, out_h);
        L.KX = kx > L.KX ? kx : L.KX;
        L.KY = ky > L.KY ? ky : L.KY;
        L.Hmax = (int)h > L.Hmax ? (int)h : L.Hmax;
        rows += (size_t)h;
    }
    const size_t nb = (size_t)B;
    L.bounds_x = nb * sizeof(int64_t);
    L.bounds_y = L.bounds_x + nb * out_w * 2 * sizeof(int32_t);
    L.coef_x = L.bounds_y + nb * out_h * 2 * sizeof(int32_t);
    L.coef_y = L.coef_x + nb * out_w * L.KX * sizeof(int32_t);
    L.inter = L.coef_y + nb * out_h * L.KY * sizeof(int32_t);
    L.total = L.inter + rows * out_w * 3;
    return true;
}

// ---- (a) the coefficient tables -----------------------------------------------------------------------------------------------
// IEEE double, every operation rounded on its own (no contraction), the sum of the weights in index order: Pillow's C.
#pragma clang fp contract(off)
__device__ __forceinline__ double rs_weight(int x, int xmin, double center, double ss) {
    double t = ((double)(x + xmin) - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    return t < 1.0 ? 1.0 - t : 0.0;
}

__global__ __launch_bounds__(RS_THREADS) void resample_tables_kernel(const int64_t* __restrict__ desc, int B, int out_w, int out_h,
                                                                     int KX, int KY, int64_t* __restrict__ inter_off,
                                                                     int32_t* __restrict__ bounds_x, int32_t* __restrict__ bounds_y,
                                                                     int32_t* __restrict__ coef_x, int32_t* __restrict__ coef_y) {
    const int xx = blockIdx.x * RS_THREADS + threadIdx.x;
    const int axis = blockIdx.y, b = blockIdx.z;
    if (xx == 0 && axis == 0) {                                  // where image b's intermediate starts: the rows in front of it
        int64_t rows = 0;
        for (int q = 0; q < b; ++q) rows += desc[3 * q + 1];
        inter_off[b] = rows * out_w * 3;
    }
    const int n_out = axis ? out_h : out_w;
    if (xx >= n_out) return;
    const int n_in = (int)desc[3 * b + 1 + (axis ? 0 : 1)];
    const int K = axis ? KY : KX;
    int32_t* __restrict__ bounds = (axis ? bounds_y : bounds_x) + ((size_t)b * n_out + xx) * 2;
    int32_t* __restrict__ k = (axis ? coef_y : coef_x) + ((size_t)b * n_out + xx) * K;

    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const double ss = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    int n = xmax - xmin;
    if (n > K) n = K;                                            // (never: K >= 2 ceil(support) + 1 >= n; keeps the stores inside the row)
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww = ww + rs_weight(x, xmin, center, ss);
    for (int x = 0; x < n; ++x) {
        double w = rs_weight(x, xmin, center, ss);               // (the same value as in the sum: recomputed, not stored)
        if (ww != 0.0) w = w / ww;
        const double scaled = w * (double)(1 << RS_BITS);
        k[x] = w < 0.0 ? (int32_t)(-0.5 + scaled) : (int32_t)(0.5 + scaled);
    }
    for (int x = n; x < K; ++x) k[x] = 0;
    bounds[0] = xmin;
    bounds[1] = n;
}

__device__ __forceinline__ int rs_clip8(int s) {
    s >>= RS_BITS;
    return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// ---- (b) horizontal pass: src [h][w][3] -> intermediate [h][out_w][3] ------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void resample_horizontal_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                         int out_w, int KX, const int64_t* __restrict__ inter_off,
                                                                         const int32_t* __restrict__ bounds_x,
                                                                         const int32_t* __restrict__ coef_x, uint8_t* __restrict__ inter) {
    const int xx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.z;
    const int h = (int)desc[3 * b + 1], w = (int)desc[3 * b + 2];
    if (xx >= out_w || y >= h) return;
    const int32_t* __restrict__ bounds = bounds_x + ((size_t)b * out_w + xx) * 2;
    const int32_t* __restrict__ k = coef_x + ((size_t)b * out_w + xx) * KX;
    const int xmin = bounds[0], n = bounds[1];
    const uint8_t* __restrict__ row = src + desc[3 * b] + ((size_t)y * w + xmin) * 3;
    int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < n; ++x) {
        const int kx = k[x];
        s0 += (int)row[3 * x + 0] * kx;
        s1 += (int)row[3 * x + 1] * kx;
        s2 += (int)row[3 * x + 2] * kx;
    }
    uint8_t* __restrict__ out = inter + inter_off[b] + ((size_t)y * out_w + xx) * 3;
    out[0] = (uint8_t)rs_clip8(s0);
    out[1] = (uint8_t)rs_clip8(s1);
    out[2] = (uint8_t)rs_clip8(s2);
}

// ---- (c) vertical pass + epilogue: intermediate [h][out_w][3] -> uint8 [out_h][out_w][3] and / or fp32 [3][out_h][out_w] --------
// The epilogue is image_prep.hip's: ToTensor (/ 255), Normalize ((x - mean) / std), every operation rounded to fp32.
__global__ __launch_bounds__(RS_THREADS) void resample_vertical_kernel(const uint8_t* __restrict__ inter, const int64_t* __restrict__ inter_off,
                                                                       int out_w, int out_h, int KY, const int32_t* __restrict__ bounds_y,
                                                                       const int32_t* __restrict__ coef_y, uint8_t* __restrict__ dst_u8,
                                                                       float* __restrict__ dst_f32, float m0, float m1, float m2, float d0,
                                                                       float d1, float d2) {
    const int xx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int yy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.z;
    if (xx >= out_w || yy >= out_h) return;
    const int32_t* __restrict__ bounds = bounds_y + ((size_t)b * out_h + yy) * 2;
    const int32_t* __restrict__ k = coef_y + ((size_t)b * out_h + yy) * KY;
    const int ymin = bounds[0], n = bounds[1];
    const size_t pitch = (size_t)out_w * 3;
    const uint8_t* __restrict__ col = inter + inter_off[b] + (size_t)ymin * pitch + (size_t)xx * 3;
    int s[3] = {1 << (RS_BITS - 1), 1 << (RS_BITS - 1), 1 << (RS_BITS - 1)};
    for (int y = 0; y < n; ++y) {
        const int ky = k[y];
        s[0] += (int)col[y * pitch + 0] * ky;
        s[1] += (int)col[y * pitch + 1] * ky;
        s[2] += (int)col[y * pitch + 2] * ky;
    }
    const size_t plane = (size_t)out_h * out_w, pix = (size_t)yy * out_w + xx;
    const float mean[3] = {m0, m1, m2}, stdv[3] = {d0, d1, d2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int byte = rs_clip8(s[c]);
        if (dst_u8 != nullptr) dst_u8[((size_t)b * plane + pix) * 3 + c] = (uint8_t)byte;
        if (dst_f32 != nullptr) {
            const float unit = (float)byte / 255.0f;             // ToTensor
            const float d = unit - mean[c];
            dst_f32[((size_t)b * 3 + c) * plane + pix] = d / stdv[c];      // Normalize
        }
    }
}

struct Views {
    int64_t* inter_off;
    int32_t *bounds_x, *bounds_y, *coef_x, *coef_y;
    uint8_t* inter;
};

Views views(void* ws, const Layout& L) {
    char* p = static_cast<char*>(ws);
    return {reinterpret_cast<int64_t*>(p), reinterpret_cast<int32_t*>(p + L.bounds_x), reinterpret_cast<int32_t*>(p + L.bounds_y),
            reinterpret_cast<int32_t*>(p + L.coef_x), reinterpret_cast<int32_t*>(p + L.coef_y), reinterpret_cast<uint8_t*>(p + L.inter)};
}

void launch_tables(const int64_t* desc_dev, int B, int out_w, int out_h, const Layout& L, const Views& v, hipStream_t st) {
    const int n = out_w > out_h ? out_w : out_h;
    hipLaunchKernelGGL(resample_tables_kernel, dim3((n + RS_THREADS - 1) / RS_THREADS, 2, B), dim3(RS_THREADS), 0, st, desc_dev, B, out_w,
                       out_h, L.KX, L.KY, v.inter_off, v.bounds_x, v.bounds_y, v.coef_x, v.coef_y);
}

}  // namespace

extern "C" long long cim_resample_ws_bytes(int B, const int64_t* desc_host, int out_w, int out_h) {
    Layout L;
    if (!plan(desc_host, B, out_w, out_h, L)) return -1;
    return (long long)L.total;
}

extern "C" int cim_resample_tables(const int64_t* desc_host, const int64_t* desc_dev, int B, int out_w, int out_h, void* ws, void* stream) {
    Layout L;
    if (!plan(desc_host, B, out_w, out_h, L)) return -1;
    CIM_CHECK_ARG(desc_dev && ws);
    launch_tables(desc_dev, B, out_w, out_h, L, views(ws, L), cim::as_stream(stream));
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_resample_rgb(const uint8_t* src, const int64_t* desc_host, const int64_t* desc_dev, int B, int out_w, int out_h,
                                uint8_t* dst_u8, float* dst_f32, const float* mean_std6_host, void* ws, void* stream) {
    Layout L;
    if (!plan(desc_host, B, out_w, out_h, L)) return -1;
    if (dst_u8 == nullptr && dst_f32 == nullptr) {
        cim::set_error("cim_resample_rgb: both destinations are NULL");
        return -1;
    }
    CIM_CHECK_ARG(src && desc_dev && ws && (dst_f32 == nullptr || mean_std6_host != nullptr));
    const float one[6] = {0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f};
    const float* ms = mean_std6_host != nullptr ? mean_std6_host : one;
    hipStream_t st = cim::as_stream(stream);
    const Views v = views(ws, L);
    launch_tables(desc_dev, B, out_w, out_h, L, v, st);
    const dim3 block(RS_THREADS);
    hipLaunchKernelGGL(resample_horizontal_kernel, dim3((out_w + 63) / 64, (L.Hmax + 3) / 4, B), block, 0, st, src, desc_dev, out_w, L.KX,
                       v.inter_off, v.bounds_x, v.coef_x, v.inter);
    hipLaunchKernelGGL(resample_vertical_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4, B), block, 0, st, v.inter, v.inter_off, out_w, out_h,
                       L.KY, v.bounds_y, v.coef_y, dst_u8, dst_f32, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
    CIM_CHECK_LAUNCH();
    return 0;
}
