// Gradient clipping by the global L2 norm, on the device (lib/utils/net.py:15 `clip_gradient`).
//     total = sqrt(sum over all gradients of g^2) ;   coef = max_norm / max(total, max_norm) ;   g = g * coef
// Three launches on one stream, over the chunk table of the fused optimizers (cim_sgd_chunk, flat chunks only):
//   grad_sqsum_kernel        one workgroup per chunk -> partial[chunk], the chunk's sum of squares in fp64
//   grad_norm_finish_kernel  one workgroup: partial[0..n_chunks) -> out[0] = norm, out[1] = coef
//   grad_scale_kernel        one workgroup per chunk: reads out[1]; returns when it is exactly 1, else g *= coef
// The clip coefficient never visits the host.  The result does not depend on the grid, on arrival order or on the run: a
// chunk's sum has one fixed shape (lane: elements in index order into four accumulators; wave: xor butterfly; workgroup: a
// fixed tree over the four waves), every chunk owns one slot of `partial`, and the finish sums the slots in an order that only
// depends on n_chunks.  No atomics.  fp64 throughout: the square of an fp32 value is exact in fp64 and cannot overflow.
#include "common.h"
#include "../../include/cim_hip.h"
#include "optim_stream.h"

namespace {

__device__ __forceinline__ void sq4(double (&a)[4], const float4& v) {
    a[0] = fma((double)v.x, (double)v.x, a[0]);
    a[1] = fma((double)v.y, (double)v.y, a[1]);
    a[2] = fma((double)v.z, (double)v.z, a[2]);
    a[3] = fma((double)v.w, (double)v.w, a[3]);
}

__device__ __forceinline__ float4 scale4(const float4& v, float coef) {
    return make_float4(v.x * coef, v.y * coef, v.z * coef, v.w * coef);
}

// Sum over the workgroup's 256 lanes, valid in thread 0.  Fixed shape: xor butterfly inside a wave, then (w0 + w1) + (w2 + w3).
// `lds` is reused by the caller's next chunk: the trailing barrier keeps wave 0's reads ahead of the next writes.
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
    return s;
}

// the chunk `ch` of its tensor: base pointer, elements (clamped to the tensor's end; 0 for a chunk that names no tensor) and
// whether 16-byte accesses are allowed (chunk offsets are multiples of 4 elements, so the tensor's pointer decides)
__device__ __forceinline__ float* chunk_span(const uint64_t* __restrict__ grads, const int64_t* __restrict__ numel, int n_tensors,
                                             const cim_sgd_chunk& ch, int& n, bool& aligned) {
    n = 0;
    aligned = false;
    if ((unsigned)ch.tensor >= (unsigned)n_tensors) return nullptr;
    const uint64_t base = grads[ch.tensor];
    const int64_t left = numel[ch.tensor] - ch.offset;
    if (ch.offset < 0 || left <= 0 || ch.n <= 0) return nullptr;
    n = left < (int64_t)ch.n ? (int)left : ch.n;
    aligned = (base & 15) == 0;
    return reinterpret_cast<float*>(base) + ch.offset;
}

__global__ __launch_bounds__(256) void grad_sqsum_kernel(const uint64_t* __restrict__ grads, const int64_t* __restrict__ numel,
                                                         int n_tensors, const cim_sgd_chunk* __restrict__ chunks, int n_chunks,
                                                         double* __restrict__ partial) {
  __shared__ double lds[4];
  for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    int n;
    bool aligned;
    const float* __restrict__ g = chunk_span(grads, numel, n_tensors, chunks[ci], n, aligned);
    const int n4 = aligned ? (n & ~3) : 0;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int i = threadIdx.x * 4;
    for (; i + 3 * 1024 < n4; i += 4 * 1024) {           // 4 x 16 B loads in flight per lane
        const float4 v0 = stream_load(g + i), v1 = stream_load(g + i + 1024), v2 = stream_load(g + i + 2048), v3 = stream_load(g + i + 3072);
        sq4(a, v0); sq4(a, v1); sq4(a, v2); sq4(a, v3);
    }
    for (; i < n4; i += 1024) sq4(a, stream_load(g + i));
    for (int j = n4 + threadIdx.x; j < n; j += 256)     // unaligned tensors / tails
        a[0] = fma((double)g[j], (double)g[j], a[0]);
    const double s = block_sum((a[0] + a[1]) + (a[2] + a[3]), lds);
    if (threadIdx.x == 0) partial[ci] = s;
  }
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, int n_chunks, double max_norm,
                                                               float* __restrict__ out) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += 256) acc += partial[i];
    const double total = block_sum(acc, lds);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(total);
    float coef = 1.0f;
    if (norm != norm) coef = __builtin_nanf("");         // Python's max(total, clip_norm) keeps a NaN first argument
    else if (norm > max_norm) coef = (float)(max_norm / norm);      // (norm = +inf: 0)
    out[0] = (float)norm;
    out[1] = coef;
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const uint64_t* __restrict__ grads, const int64_t* __restrict__ numel,
                                                         int n_tensors, const cim_sgd_chunk* __restrict__ chunks, int n_chunks,
                                                         const float* __restrict__ out) {
  const float coef = out[1];
  if (coef == 1.0f) return;                              // nothing to clip: no gradient is touched (a NaN coefficient goes on)
  for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    int n;
    bool aligned;
    float* __restrict__ g = chunk_span(grads, numel, n_tensors, chunks[ci], n, aligned);
    const int n4 = aligned ? (n & ~3) : 0;
    int i = threadIdx.x * 4;
    for (; i + 3 * 1024 < n4; i += 4 * 1024) {           // 4 x 16 B loads in flight per lane, as in the norm launch
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = stream_load(g + i + k * 1024);
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(g + i + k * 1024) = scale4(v[k], coef);
    }
    for (; i < n4; i += 1024) *reinterpret_cast<float4*>(g + i) = scale4(stream_load(g + i), coef);
    for (int j = n4 + threadIdx.x; j < n; j += 256) g[j] *= coef;
  }
}

}  // namespace

extern "C" int cim_grad_norm_multi(const uint64_t* grads, const int64_t* numel, int n_tensors, const cim_sgd_chunk* chunks,
                                   int n_chunks, double* partial, double max_norm, float* out, int max_workgroups, void* stream) {
    CIM_CHECK_ARG(n_chunks >= 0 && n_tensors >= 0 && max_workgroups >= 0);
    CIM_CHECK_ARG(max_norm >= 0.0);
    if (n_chunks == 0) return 0;
    CIM_CHECK_ARG(grads != nullptr && numel != nullptr && chunks != nullptr && partial != nullptr && out != nullptr);
    CIM_CHECK_ARG(n_tensors > 0);
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(optim_grid(n_chunks, max_workgroups)), dim3(256), 0, cim::as_stream(stream), grads, numel,
                       n_tensors, chunks, n_chunks, partial);
    CIM_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, cim::as_stream(stream), partial, n_chunks, max_norm, out);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_grad_scale_multi(const uint64_t* grads, const int64_t* numel, int n_tensors, const cim_sgd_chunk* chunks,
                                    int n_chunks, const float* out, int max_workgroups, void* stream) {
    CIM_CHECK_ARG(n_chunks >= 0 && n_tensors >= 0 && max_workgroups >= 0);
    if (n_chunks == 0) return 0;
    CIM_CHECK_ARG(grads != nullptr && numel != nullptr && chunks != nullptr && out != nullptr);
    CIM_CHECK_ARG(n_tensors > 0);
    hipLaunchKernelGGL(grad_scale_kernel, dim3(optim_grid(n_chunks, max_workgroups)), dim3(256), 0, cim::as_stream(stream), grads, numel,
                       n_tensors, chunks, n_chunks, out);
    CIM_CHECK_LAUNCH();
    return 0;
}
