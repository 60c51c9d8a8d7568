// Batch-statistics BatchNorm (+ residual) (+ ReLU): nn.BatchNorm2d in train() mode, forward and backward.
//
//   forward :  mean[c], var[c] (biased) over the m = N HW values of channel c;  y = relu?(gamma (x - mean) rsqrt(var + eps) + beta (+ res))
//              running_mean = (1 - f) running_mean + f mean;  running_var = (1 - f) running_var + f var m / (m - 1);  batches += 1
//   backward:  dz = dy (y > 0);  S1 = sum dz;  S2 = sum dz (x - mean);  dbeta = S1;  dgamma = rstd S2;
//              dx = gamma rstd (dz - S1 / m - (x - mean) rstd^2 S2 / m);  dres = dz
//
// Layout NCHW fp32.  A channel's values are N planes of HW floats, C HW apart; they are cut into CHUNKS that depend on the shape
// alone (chunk_geom): a plane of more than BT_CHUNK floats into pieces of BT_CHUNK, shorter planes gathered into groups of
// BT_CHUNK / HW whole planes.  One workgroup per (channel, chunk) reduces its chunk and writes a partial to the caller's
// workspace; a finishing launch - one wave per channel - adds each channel's partials in double: lane l the l-th contiguous run
// of chunks in index order, lane 0 then the 64 run results in index order.  No atomics, no workgroup waits for another: the same
// bits on every call and every stream (the pattern of conv7x7_dw.hip).
//
// Statistics, centred at every level: a chunk's partial is (K, s, M2) - its count is a function of the shape - where K is the
// chunk's first value, s = sum (x - K), so that the chunk's sum is count K + s WITHOUT a rounded quotient (small integers and
// constant channels stay exact), and M2 = sum (x - P)^2 - (sum (x - P))^2 / count about the chunk's own mean P = K + s / count,
// from a second read of the chunk (16 KB: it comes from the cache, HBM traffic stays 4 B / element).  The finishing launch
// joins (count, sum, M2) triples with Chan's formula, M2 += M2_b + delta^2 n_a n_b / (n_a + n_b), delta the difference of means.
//
// The forward normalisation is cim_bn_act_fwd (bn_act.hip) on the batch statistics: called, not copied.
// Streaming kernels: 16-byte accesses over the 16-byte aligned part of every run (planes of 49 or 1000 floats start unaligned:
// scalar head and tail); 4 B / element for the statistics, 12 for the backward sums, 16-20 for dx (+ dres).  The statistics
// are fp32 sums, centred; the backward's sums and dx are computed in double (below).
#include <limits.h>

#include "common.h"
#include "../../include/cim_hip.h"

namespace {

constexpr int BT_CHUNK = 4096;                       // floats of a chunk at most: 16 per lane of a 256-lane workgroup
constexpr int BT_WAVE_PLANES = 4;                    // a chunk of at least this many whole planes: one wave per plane

struct ChunkGeom {
    int N, C, HW;
    int pieces;                                      // HW >  BT_CHUNK: pieces of a plane, one per chunk
    int planes;                                      // HW <= BT_CHUNK: whole planes per chunk (1 otherwise)
    int chunks;                                      // per channel
    int vec;                                         // every tensor's base is 16-byte aligned: 16-byte accesses allowed
};

ChunkGeom chunk_geom(int N, int C, int HW) {
    ChunkGeom g{};
    g.N = N; g.C = C; g.HW = HW;
    g.pieces = (int)(((long long)HW + BT_CHUNK - 1) / BT_CHUNK);
    g.planes = HW >= BT_CHUNK ? 1 : BT_CHUNK / HW;
    g.chunks = g.planes == 1 ? N * g.pieces : (N + g.planes - 1) / g.planes;
    g.vec = 0;
    return g;
}

__device__ __forceinline__ int chunk_count(const ChunkGeom& g, int k) {
    if (g.planes == 1) {
        const long long j = k % g.pieces;               // (64-bit: HW may be within BT_CHUNK of INT_MAX)
        return (int)(min((long long)g.HW, (j + 1) * BT_CHUNK) - j * BT_CHUNK);
    }
    return (min(g.N, (k + 1) * g.planes) - k * g.planes) * g.HW;
}

__device__ __forceinline__ size_t chunk_first(const ChunkGeom& g, int c, int k) {       // offset of the chunk's first value
    if (g.planes == 1) return ((size_t)(k / g.pieces) * g.C + c) * g.HW + (size_t)(k % g.pieces) * BT_CHUNK;
    return ((size_t)k * g.planes * g.C + c) * g.HW;
}

// The contiguous run [beg, end) of float offsets among `width` lanes: f4(i) for every 16-byte aligned quad, f1(i) for the up to
// three floats before the first and after the last one (all of them when 16-byte accesses are not allowed).
template <class F1, class F4>
__device__ __forceinline__ void walk_run(size_t beg, size_t end, int vec, int lane, int width, F1 f1, F4 f4) {
    const size_t a = vec ? min(end, (beg + 3) & ~(size_t)3) : end;
    const size_t b = vec ? max(a, end & ~(size_t)3) : end;
    for (size_t i = beg + lane; i < a; i += width) f1(i);
    for (size_t i = a + 4 * (size_t)lane; i < b; i += 4 * (size_t)width) f4(i);
    for (size_t i = b + lane; i < end; i += width) f1(i);
}

// Every value of chunk k of channel c, once, by the 256 lanes of a workgroup.
template <class F1, class F4>
__device__ __forceinline__ void walk_chunk(const ChunkGeom& g, int c, int k, F1 f1, F4 f4) {
    const int tid = threadIdx.x;
    if (g.planes == 1) {
        const int n = k / g.pieces, j = k - n * g.pieces;
        const size_t base = ((size_t)n * g.C + c) * g.HW;
        walk_run(base + (size_t)j * BT_CHUNK, base + min((size_t)g.HW, (size_t)(j + 1) * BT_CHUNK), g.vec, tid, 256, f1, f4);
        return;
    }
    const int n0 = k * g.planes, n1 = min(g.N, n0 + g.planes);
    if (g.planes >= BT_WAVE_PLANES) {
        for (int n = n0 + (tid >> 6); n < n1; n += 4) {
            const size_t base = ((size_t)n * g.C + c) * g.HW;
            walk_run(base, base + g.HW, g.vec, tid & 63, 64, f1, f4);
        }
    } else {
        for (int n = n0; n < n1; ++n) {
            const size_t base = ((size_t)n * g.C + c) * g.HW;
            walk_run(base, base + g.HW, g.vec, tid, 256, f1, f4);
        }
    }
}

__device__ __forceinline__ float4 ld4(const float* p, size_t i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ void st4(float* p, size_t i, const float4& v) { *reinterpret_cast<float4*>(p + i) = v; }

// Sum of (a, b) over the 256 lanes, returned to every lane: xor tree in the wave, then the four wave sums in index order.
template <class T>
__device__ __forceinline__ void block_sum2(T& a, T& b, T (*sh)[4]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    __syncthreads();                                 // (the previous sum's reads are done)
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    a = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
    b = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
}

// grid = C chunks workgroups, (channel, chunk) = (blockIdx.x / chunks, blockIdx.x % chunks); partial [C][chunks][3] = (K, s, M2)
__global__ __launch_bounds__(256) void bn_train_stats_kernel(const float* __restrict__ x, float* __restrict__ part,
                                                             long long* __restrict__ batches, const ChunkGeom g) {
    __shared__ float sh[2][4];
    const int c = blockIdx.x / g.chunks, k = blockIdx.x - c * g.chunks;
    // num_batches_tracked: ONE lane of the launch, an ordinary store.  It is written HERE and not by the finishing launch, whose
    // workgroups all read it (momentum None): a launch boundary orders the store before every one of those reads.
    if (batches != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *batches = *batches + 1;
    const float K = x[chunk_first(g, c, k)];
    const float n = (float)chunk_count(g, k);
    float s = 0.0f, unused = 0.0f;
    walk_chunk(g, c, k, [&](size_t i) { s += x[i] - K; },
               [&](size_t i) { const float4 v = ld4(x, i); s += v.x - K; s += v.y - K; s += v.z - K; s += v.w - K; });
    block_sum2(s, unused, sh);
    const float P = K + s / n;                       // the chunk's mean, rounded: a pivot, its rounding is taken out again below
    float t = 0.0f, q = 0.0f;
    walk_chunk(g, c, k, [&](size_t i) { const float d = x[i] - P; t += d; q = fmaf(d, d, q); },
               [&](size_t i) {
                   const float4 v = ld4(x, i);
                   const float d0 = v.x - P, d1 = v.y - P, d2 = v.z - P, d3 = v.w - P;
                   t += d0; q = fmaf(d0, d0, q);
                   t += d1; q = fmaf(d1, d1, q);
                   t += d2; q = fmaf(d2, d2, q);
                   t += d3; q = fmaf(d3, d3, q);
               });
    block_sum2(t, q, sh);
    if (threadIdx.x == 0) {
        float* __restrict__ out = part + (size_t)blockIdx.x * 3;
        out[0] = K;
        out[1] = s;
        out[2] = fmaxf(q - t * t / n, 0.0f);
    }
}

struct Moments { double n, sum, m2; };

__device__ __forceinline__ void chan_join(Moments& a, const Moments& b) {       // a <- a joined with b (b.n > 0)
    if (a.n == 0.0) { a = b; return; }
    const double delta = b.sum / b.n - a.sum / a.n, n = a.n + b.n;
    a.m2 += b.m2 + delta * delta * (a.n * b.n / n);
    a.sum += b.sum;
    a.n = n;
}

// grid = C, one wave per channel.  mean, var (biased), rstd = rsqrtf(var + eps) as the normalisation computes it; the running
// buffers by torch's rule, f = momentum or, momentum < 0 ("None"), 1 / batches with the count the statistics launch left.
__global__ __launch_bounds__(64) void bn_train_stats_finish_kernel(const float* __restrict__ part, float* __restrict__ mean,
                                                                   float* __restrict__ var, float* __restrict__ rstd,
                                                                   float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                   const long long* __restrict__ batches, float momentum, float eps,
                                                                   const ChunkGeom g) {
    __shared__ Moments runs[64];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int per = (g.chunks + 63) / 64;
    const int k0 = lane * per, k1 = min(g.chunks, k0 + per);
    Moments a{0.0, 0.0, 0.0};
    for (int k = k0; k < k1; ++k) {
        const float* __restrict__ p = part + ((size_t)c * g.chunks + k) * 3;
        const double n = (double)chunk_count(g, k);
        chan_join(a, Moments{n, n * (double)p[0] + (double)p[1], (double)p[2]});
    }
    runs[lane] = a;
    __syncthreads();
    if (lane != 0) return;
    for (int l = 1; l < 64; ++l)
        if (runs[l].n > 0.0) chan_join(a, runs[l]);
    const double m = a.n;                            // = N HW
    const float mu = (float)(a.sum / m), v = (float)(a.m2 / m);
    mean[c] = mu;
    var[c] = v;
    if (rstd != nullptr) rstd[c] = rsqrtf(v + eps);
    if (running_mean != nullptr) {
        // (torch: a momentum of None is the cumulative average, factor 1 / num_batches_tracked after its increment)
        const double f = momentum < 0.0f ? 1.0 / (double)*batches : (double)momentum;
        running_mean[c] = (float)((1.0 - f) * (double)running_mean[c] + f * (a.sum / m));
        running_var[c] = (float)((1.0 - f) * (double)running_var[c] + f * (a.m2 / (m - 1.0)));
    }
}

__device__ __forceinline__ float relu_bwd(float dy, float y) { return y > 0.0f ? dy : 0.0f; }

// The backward's arithmetic is DOUBLE.  dx is what is left of dz after its projections on 1 and on x - mean are taken out, and at
// few values per channel nearly nothing is left (m = 2: the normalised pair is +-1 whatever x is, dx = O(eps / var) dz): fp32 sums
// and an fp32 difference would leave rounding noise of the size of dz there.  The launches stream 12-20 B / element; the
// conversions and the three double operations per element ride under the loads.

// grid = C chunks; partial [C][chunks][2] doubles = (sum dz, sum dz (x - mean)) of the chunk
template <bool RELU>
__global__ __launch_bounds__(256) void bn_train_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                  const float* __restrict__ x, const float* __restrict__ mean,
                                                                  double* __restrict__ part, const ChunkGeom g) {
    __shared__ double sh[2][4];
    const int c = blockIdx.x / g.chunks, k = blockIdx.x - c * g.chunks;
    const double mu = (double)mean[c];
    double s1 = 0.0, s2 = 0.0;
    auto one = [&](float dz, float xv) {
        s1 += (double)dz;
        s2 = fma((double)dz, (double)xv - mu, s2);
    };
    walk_chunk(g, c, k, [&](size_t i) { one(RELU ? relu_bwd(dy[i], y[i]) : dy[i], x[i]); },
               [&](size_t i) {
                   float4 d = ld4(dy, i);
                   const float4 v = ld4(x, i);
                   if (RELU) {
                       const float4 o = ld4(y, i);
                       d.x = relu_bwd(d.x, o.x); d.y = relu_bwd(d.y, o.y); d.z = relu_bwd(d.z, o.z); d.w = relu_bwd(d.w, o.w);
                   }
                   one(d.x, v.x); one(d.y, v.y); one(d.z, v.z); one(d.w, v.w);
               });
    block_sum2(s1, s2, sh);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 2] = s1;
        part[(size_t)blockIdx.x * 2 + 1] = s2;
    }
}

// grid = C, one wave per channel: S1, S2, runs of chunks in index order; dbeta = S1, dgamma = rstd S2, and the two per-channel
// constants of the dx launch, coef [C][2] doubles = (S1 / m, rstd^2 S2 / m).
__global__ __launch_bounds__(64) void bn_train_bwd_finish_kernel(const double* __restrict__ part, const float* __restrict__ rstd,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                 double* __restrict__ coef, const ChunkGeom g) {
    __shared__ double r1[64], r2[64];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int per = (g.chunks + 63) / 64;
    const int k0 = lane * per, k1 = min(g.chunks, k0 + per);
    double s1 = 0.0, s2 = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double* __restrict__ p = part + ((size_t)c * g.chunks + k) * 2;
        s1 += p[0];
        s2 += p[1];
    }
    r1[lane] = s1;
    r2[lane] = s2;
    __syncthreads();
    if (lane != 0) return;
    for (int l = 1; l < 64; ++l) { s1 += r1[l]; s2 += r2[l]; }
    const double m = (double)g.N * (double)g.HW, rs = (double)rstd[c];
    if (dbeta != nullptr) dbeta[c] = (float)s1;
    if (dgamma != nullptr) dgamma[c] = (float)(rs * s2);
    coef[2 * c] = s1 / m;
    coef[2 * c + 1] = rs * rs * s2 / m;
}

// grid = C chunks: dx = gamma rstd (dz - S1 / m - (x - mean) rstd^2 S2 / m), dres = dz
template <bool RELU>
__global__ __launch_bounds__(256) void bn_train_dx_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                          const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const double* __restrict__ coef, float* __restrict__ dx,
                                                          float* __restrict__ dres, const ChunkGeom g) {
    const int c = blockIdx.x / g.chunks, k = blockIdx.x - c * g.chunks;
    const double mu = (double)mean[c], ga = (double)gamma[c] * (double)rstd[c], k1 = coef[2 * c], k2 = coef[2 * c + 1];
    auto one = [&](float dz, float xv) { return (float)(ga * (((double)dz - k1) - ((double)xv - mu) * k2)); };
    walk_chunk(g, c, k,
               [&](size_t i) {
                   const float dz = RELU ? relu_bwd(dy[i], y[i]) : dy[i];
                   if (dx != nullptr) dx[i] = one(dz, x[i]);
                   if (dres != nullptr) dres[i] = dz;
               },
               [&](size_t i) {
                   float4 d = ld4(dy, i);
                   if (RELU) {
                       const float4 o = ld4(y, i);
                       d.x = relu_bwd(d.x, o.x); d.y = relu_bwd(d.y, o.y); d.z = relu_bwd(d.z, o.z); d.w = relu_bwd(d.w, o.w);
                   }
                   if (dx != nullptr) {
                       const float4 v = ld4(x, i);
                       st4(dx, i, float4{one(d.x, v.x), one(d.y, v.y), one(d.z, v.z), one(d.w, v.w)});
                   }
                   if (dres != nullptr) st4(dres, i, d);
               });
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// (the offsets are size_t, the workgroup index C chunks an int: one bound on the element count covers both)
#define BN_TRAIN_SHAPE_OK()                                                                                          \
    CIM_CHECK_ARG(N >= 1);                                                                                           \
    CIM_CHECK_ARG(C >= 1);                                                                                           \
    CIM_CHECK_ARG(HW >= 1);                                                                                          \
    CIM_CHECK_ARG((long long)N * HW >= 2 /* more than 1 value per channel when training */);                         \
    CIM_CHECK_ARG((long long)N * C * HW <= (long long)INT_MAX /* N * C * HW overflows an int */)

extern "C" long long cim_bn_train_chunks(int N, int C, int HW) {
    BN_TRAIN_SHAPE_OK();
    return chunk_geom(N, C, HW).chunks;
}

extern "C" long long cim_bn_train_workspace(int N, int C, int HW) {
    BN_TRAIN_SHAPE_OK();
    // (the statistics' [C][chunks][3] floats; the backward's [C][chunks][2] + [C][2] doubles: four floats each covers both)
    return ((long long)C * chunk_geom(N, C, HW).chunks + C) * 4 * (long long)sizeof(float);
}

extern "C" int cim_bn_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float eps, float momentum,
                                float* running_mean, float* running_var, long long* num_batches_tracked, float* y, float* mean,
                                float* var, float* rstd, int N, int C, int HW, int relu, float* workspace, void* stream) {
    CIM_CHECK_ARG(x != nullptr);
    CIM_CHECK_ARG(gamma != nullptr);
    CIM_CHECK_ARG(beta != nullptr);
    CIM_CHECK_ARG(y != nullptr);
    CIM_CHECK_ARG(mean != nullptr);
    CIM_CHECK_ARG(var != nullptr);
    CIM_CHECK_ARG(workspace != nullptr);
    CIM_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr));
    CIM_CHECK_ARG(momentum >= 0.0f || running_mean == nullptr || num_batches_tracked != nullptr /* momentum None counts batches */);
    BN_TRAIN_SHAPE_OK();
    ChunkGeom g = chunk_geom(N, C, HW);
    g.vec = aligned16(x);
    hipStream_t st = cim::as_stream(stream);
    hipLaunchKernelGGL(bn_train_stats_kernel, dim3(C * g.chunks), dim3(256), 0, st, x, workspace, num_batches_tracked, g);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_train_stats_finish_kernel, dim3(C), dim3(64), 0, st, (const float*)workspace, mean, var, rstd,
                       running_mean, running_var, (const long long*)num_batches_tracked, momentum, eps, g);
    CIM_CHECK_LAUNCH();
    return cim_bn_act_fwd(x, res, gamma, beta, mean, var, eps, y, N, C, HW, relu, stream);
}

extern "C" int cim_bn_train_bwd(const float* dy, const float* y, const float* x, const float* gamma, const float* mean,
                                const float* rstd, float* dx, float* dres, float* dgamma, float* dbeta, int N, int C, int HW,
                                int relu, float* workspace, void* stream) {
    CIM_CHECK_ARG(dy != nullptr);
    CIM_CHECK_ARG(x != nullptr);
    CIM_CHECK_ARG(gamma != nullptr);
    CIM_CHECK_ARG(mean != nullptr);
    CIM_CHECK_ARG(rstd != nullptr);
    CIM_CHECK_ARG(workspace != nullptr);
    CIM_CHECK_ARG(((uintptr_t)workspace & 7) == 0 /* workspace: 8-byte aligned */);
    CIM_CHECK_ARG(y != nullptr || !relu);
    CIM_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr));
    BN_TRAIN_SHAPE_OK();
    ChunkGeom g = chunk_geom(N, C, HW);
    g.vec = aligned16(dy) && aligned16(x) && (!relu || aligned16(y)) && aligned16(dx) && aligned16(dres);
    hipStream_t st = cim::as_stream(stream);
    double* part = reinterpret_cast<double*>(workspace);
    double* coef = part + (size_t)C * g.chunks * 2;
    const dim3 grid(C * g.chunks);
    if (relu) hipLaunchKernelGGL(bn_train_bwd_reduce_kernel<true>, grid, dim3(256), 0, st, dy, y, x, mean, part, g);
    else hipLaunchKernelGGL(bn_train_bwd_reduce_kernel<false>, grid, dim3(256), 0, st, dy, y, x, mean, part, g);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_train_bwd_finish_kernel, dim3(C), dim3(64), 0, st, (const double*)part, rstd, dgamma, dbeta, coef, g);
    CIM_CHECK_LAUNCH();
    if (dx == nullptr && dres == nullptr) return 0;
    if (relu) hipLaunchKernelGGL(bn_train_dx_kernel<true>, grid, dim3(256), 0, st, dy, y, x, gamma, mean, rstd, (const double*)coef, dx, dres, g);
    else hipLaunchKernelGGL(bn_train_dx_kernel<false>, grid, dim3(256), 0, st, dy, y, x, gamma, mean, rstd, (const double*)coef, dx, dres, g);
    CIM_CHECK_LAUNCH();
    return 0;
}
