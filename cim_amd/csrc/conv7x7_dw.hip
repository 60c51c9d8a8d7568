// Weight gradient of the 7 x 7 stem convolution (padding 3, stride 1 / 2, 1..4 input channels) on the fp32 matrix pipe.
//
//   dw[co][ci][ky][kx] = sum over b, oy, ox of dconv[b][co][oy][ox] * x[b][ci][oy s + ky - 3][ox s + kx - 3]
//
// As a GEMM: M = cout, N = cin 49 (147 for RGB), K = B Ho Wo output pixels (802 816 for 16 images of 448 x 448): a short, wide
// result under a very long contraction whose B operand (im2col of x) is 49 / s^2 times larger than x itself.  So the im2col
// matrix is never built: a workgroup stages, per tile of 4 x 32 output pixels of one image,
//   Ds [64 co][128 pixels]            the dconv tile (row stride 129 words), and
//   Xs [cin][rows][row stride RS]     the input strip those pixels reach (3 halo rows / columns each side, zero outside the image)
// in LDS and reads both MFMA operands from there: every staged x element serves up to 49 / s^2 products.
//
// v_mfma_f32_16x16x4_f32 (true fp32 products, no operand splitting): wave w of the four owns the output rows co = 16 w .. 16 w + 15
// of the workgroup's 64 and ALL ceil(N / 16) column tiles (40 accumulator registers for RGB), so nothing is summed across waves.
// Lane (c = lane & 15, q = lane >> 4) supplies A[co = c][k = q] and B[k = q][n = 16 j + c]; a k step is four pixels of one tile
// row.  The column n = (ci, ky, kx) fixes a lane's base address in the strip, ci PL + ky RS + kx, and with RS = 7 and PL = 49
// (mod 32) that base is n (mod 32): the 16 lanes of a quarter read 16 consecutive banks whatever the convolution's stride is -
// the stride only moves the address all 16 share.  The two quarters that a ds_read_b32 serves together (q = 0, 1) take pixels
// 16 / s apart, 16 banks on: conflict-free for both strides.  (The A read has co along its lanes, row stride 129: the quarters'
// bank sets overlap by half at stride 2 - one read in 11 at 2 instead of 1 LDS cycles.)
//
// Summation order: workgroup `split` of a 64-channel group owns the tiles [split tiles_per, (split + 1) tiles_per) - tiles numbered
// (image, tile row, tile column) - and adds their pixels in that order into its accumulators (one fmaf chain per element), then
// writes workspace[split][cout][cin 49].  A second launch sums the splits: eight contiguous runs of splits, each in index order,
// then the eight run sums in index order.  No atomics; the split count depends on the shape alone: the same bits on every call.
#include "common.h"
#include "../../include/cim_hip.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DW_TH = 4, DW_TW = 32;                 // output pixels of a tile (rows x columns)
constexpr int DW_PIX = DW_TH * DW_TW;
constexpr int DW_CO = 64;                            // output channels of a workgroup: 16 per wave
constexpr int DW_DLD = DW_PIX + 1;                   // row stride of the dconv tile (words)
constexpr int DW_MAX_SPLITS = 768;                   // (three workgroups of <= 48.2 KB LDS per CU on 256 CUs; a constant: shape-only splits)

template <int S>
struct Strip {                                       // the input strip of a tile at stride S
    static constexpr int ROWS = (DW_TH - 1) * S + 7, COLS = (DW_TW - 1) * S + 7;
    static constexpr int RS = (COLS + 24) / 32 * 32 + 7;              // >= COLS, = 7 (mod 32)
    static constexpr int PL = (ROWS * RS + 14) / 32 * 32 + 17;        // >= ROWS RS, = 49 (mod 32)
    static_assert(RS >= COLS && RS % 32 == 7 && PL >= ROWS * RS && PL % 32 == 17, "bank layout of the strip");
};

struct DwGeom { int B, cin, cout, H, W, Ho, Wo, tiles_x, tiles_y, ntiles, tiles_per, splits; };

template <int CIN, int S>
__global__ __launch_bounds__(256) void conv7x7_dw_kernel(const float* __restrict__ dconv, const float* __restrict__ x,
                                                         float* __restrict__ ws, const DwGeom g) {
    constexpr int N = CIN * 49, NT = (N + 15) / 16;
    constexpr int ROWS = Strip<S>::ROWS, COLS = Strip<S>::COLS, RS = Strip<S>::RS, PL = Strip<S>::PL;
    __shared__ float Ds[DW_CO * DW_DLD];
    __shared__ float Xs[CIN * PL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, q = lane >> 4;
    const int co0 = blockIdx.y * DW_CO;
    const int split = blockIdx.x;
    const int t_beg = split * g.tiles_per, t_end = min(g.ntiles, t_beg + g.tiles_per);
    const bool active = co0 + 16 * wave < g.cout;            // (wave-uniform: a wave whose 16 channels do not exist only stages)

    // first pixel column of this lane's quarter within a tile row: q = 0, 1 are 16 banks apart in the strip for both strides
    const int pq = S == 2 ? 8 * q : 16 * (q & 1) + 8 * (q >> 1);
    const int ao = (16 * wave + c16) * DW_DLD + pq;
    int bo[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = 16 * j + c16;
        const int ci = n / 49, r = n - ci * 49, ky = r / 7, kx = r - ky * 7;
        // (columns behind N are computed and never stored: they read the bank their lane would have had)
        bo[j] = (n < N ? ci * PL + ky * RS + kx : c16) + pq * S;
    }

    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int tile = t_beg; tile < t_end; ++tile) {
        const int tx = tile % g.tiles_x, rest = tile / g.tiles_x;
        const int ty = rest % g.tiles_y, b = rest / g.tiles_y;
        const int oy0 = ty * DW_TH, ox0 = tx * DW_TW;
        __syncthreads();                                     // (the previous tile's operand reads are done)
        // ---- the dconv tile: lanes along the pixels of a tile row (coalesced loads, conflict-free stores)
#pragma unroll 8
        for (int it = 0; it < DW_CO * DW_PIX / 256; ++it) {
            const int idx = it * 256 + tid;
            const int px = idx & (DW_TW - 1), py = (idx / DW_TW) & (DW_TH - 1), co = idx / DW_PIX;
            const int oy = oy0 + py, ox = ox0 + px, c = co0 + co;
            float v = 0.0f;
            if (c < g.cout && oy < g.Ho && ox < g.Wo) v = dconv[(((size_t)b * g.cout + c) * g.Ho + oy) * g.Wo + ox];
            Ds[co * DW_DLD + py * DW_TW + px] = v;
        }
        // ---- the input strip, halo zero-filled
        const int iy0 = oy0 * S - 3, ix0 = ox0 * S - 3;
        for (int idx = tid; idx < CIN * ROWS * COLS; idx += 256) {
            const int col = idx % COLS, rr = idx / COLS;
            const int row = rr % ROWS, ci = rr / ROWS;
            const int iy = iy0 + row, ix = ix0 + col;
            float v = 0.0f;
            if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = x[(((size_t)b * g.cin + ci) * g.H + iy) * g.W + ix];
            Xs[ci * PL + row * RS + col] = v;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int py = 0; py < DW_TH; ++py) {
#pragma unroll
                for (int t = 0; t < 8; ++t) {                // k step: pixels (py, pq + t) of the four quarters
                    const float a = Ds[ao + py * DW_TW + t];
                    float bv[NT];
#pragma unroll
                    for (int j = 0; j < NT; ++j) bv[j] = Xs[bo[j] + py * S * RS + t * S];
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[j], acc[j], 0, 0, 0);
                }
            }
        }
    }

    // accumulator register r of column tile j: row 4 q + r of the wave's 16, column 16 j + c16
    if (active) {
        float* __restrict__ out = ws + (size_t)split * g.cout * N;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = 16 * j + c16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + 16 * wave + 4 * q + r;
                if (co < g.cout && n < N) out[(size_t)co * N + n] = acc[j][r];
            }
        }
    }
}

// dw[i] = sum over the splits of ws[split][i]: thread (e = element of 32, run of 8) sums a contiguous run of splits in index
// order, eight loads in flight; run 0's thread then adds the eight run sums in index order.
__global__ __launch_bounds__(256) void conv7x7_dw_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int mn, int splits) {
    __shared__ float part[8][32];
    const int e = threadIdx.x & 31, run = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + e;
    const int per = (splits + 7) / 8;
    const int s0 = run * per, s1 = min(splits, s0 + per);
    float v = 0.0f;
    if (i < mn) {
        for (int s = s0; s < s1; s += 8) {
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = s + j < s1 ? ws[(size_t)(s + j) * mn + i] : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (s + j < s1) v += p[j];
        }
    }
    part[run][e] = v;
    __syncthreads();
    if (run == 0 && i < mn) {
        v = part[0][e];
#pragma unroll
        for (int k = 1; k < 8; ++k) v += part[k][e];
        dw[i] = v;
    }
}

DwGeom dw_geom(int B, int cin, int cout, int H, int W, int stride) {
    DwGeom g{};
    g.B = B; g.cin = cin; g.cout = cout; g.H = H; g.W = W;
    g.Ho = (H - 1) / stride + 1; g.Wo = (W - 1) / stride + 1;
    g.tiles_x = (g.Wo + DW_TW - 1) / DW_TW; g.tiles_y = (g.Ho + DW_TH - 1) / DW_TH;
    const long long ntiles = (long long)B * g.tiles_x * g.tiles_y;
    g.ntiles = (int)ntiles;
    g.tiles_per = (int)((ntiles + DW_MAX_SPLITS - 1) / DW_MAX_SPLITS);
    g.splits = (int)((ntiles + g.tiles_per - 1) / g.tiles_per);
    return g;
}

template <int CIN>
void dw_launch(const float* dconv, const float* x, float* ws, const DwGeom& g, int stride, hipStream_t st) {
    const dim3 grid(g.splits, (g.cout + DW_CO - 1) / DW_CO);
    if (stride == 2) hipLaunchKernelGGL((conv7x7_dw_kernel<CIN, 2>), grid, dim3(256), 0, st, dconv, x, ws, g);
    else hipLaunchKernelGGL((conv7x7_dw_kernel<CIN, 1>), grid, dim3(256), 0, st, dconv, x, ws, g);
}

}  // namespace

// (the forward wrapper's limits on H and W; B bounded so that the tile count stays an int)
#define CONV7_DW_SHAPE_OK()                                                                                          \
    CIM_CHECK_ARG(B >= 1 && B <= (1 << 20));                                                                         \
    CIM_CHECK_ARG(cin >= 1 && cin <= 4);                                                                             \
    CIM_CHECK_ARG(cout >= 1 && cout <= 256);                                                                         \
    CIM_CHECK_ARG(stride == 1 || stride == 2);                                                                       \
    CIM_CHECK_ARG(H >= 1 && W >= 1 && W <= 4096);                                                                    \
    CIM_CHECK_ARG((long long)H * W < (1ll << 20));                                                                   \
    CIM_CHECK_ARG((long long)B * (((H - 1) / stride + 4) / 4) * (((W - 1) / stride + 32) / 32) < (1ll << 31) /* B: tiles */)

extern "C" int cim_conv7x7_dw_splits(int B, int cin, int cout, int H, int W, int stride) {
    CONV7_DW_SHAPE_OK();
    return dw_geom(B, cin, cout, H, W, stride).splits;
}

extern "C" long long cim_conv7x7_dw_workspace(int B, int cin, int cout, int H, int W, int stride) {
    CONV7_DW_SHAPE_OK();
    return (long long)dw_geom(B, cin, cout, H, W, stride).splits * cout * cin * 49 * (long long)sizeof(float);
}

extern "C" int cim_conv7x7_dw_f32(const float* dconv, const float* x, float* dw, int B, int cin, int cout, int H, int W,
                                  int stride, float* workspace, void* stream) {
    CIM_CHECK_ARG(dconv != nullptr);
    CIM_CHECK_ARG(x != nullptr);
    CIM_CHECK_ARG(dw != nullptr);
    CIM_CHECK_ARG(workspace != nullptr);
    CONV7_DW_SHAPE_OK();
    const DwGeom g = dw_geom(B, cin, cout, H, W, stride);
    hipStream_t st = cim::as_stream(stream);
    switch (cin) {
        case 1: dw_launch<1>(dconv, x, workspace, g, stride, st); break;
        case 2: dw_launch<2>(dconv, x, workspace, g, stride, st); break;
        case 3: dw_launch<3>(dconv, x, workspace, g, stride, st); break;
        default: dw_launch<4>(dconv, x, workspace, g, stride, st); break;
    }
    CIM_CHECK_LAUNCH();
    const int mn = cout * cin * 49;
    hipLaunchKernelGGL(conv7x7_dw_reduce_kernel, dim3((mn + 31) / 32), dim3(256), 0, st, (const float*)workspace, dw, mn, g.splits);
    CIM_CHECK_LAUNCH();
    return 0;
}
