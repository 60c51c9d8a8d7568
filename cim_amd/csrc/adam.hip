// Fused multi-tensor Adam for the 250-580 M parameters of the CIM models: torch.optim.Adam(params) as constructed at
// tools/train.py:310-311 (SOLVER.TYPE Adam; L2 weight decay, no amsgrad, no maximize), ONE launch for all tensors in the
// two-table form of sgd.hip (same chunk table, same max_workgroups walk, same matrix-mode by-products).
//
// Exact order of operations per element, all fp32 (b1 = (float)beta1, w1 = (float)(1 - beta1) from the DOUBLE beta1, likewise
// b2 / w2; step_size and bc2_sqrt come per tensor from the host, computed in double from that tensor's own step count):
//     g' = fma(wd, p, g)
//     m  = fma(b1, m, w1 * g')
//     v  = fma(b2, v, w2 * (g' * g'))
//     d  = sqrt(v) / bc2_sqrt + eps           sqrt and / correctly rounded, the sum a plain add
//     p  = p - (step_size * m) / d            / correctly rounded, the difference a plain subtract
// Every product and sum above is written out (fmaf where fused), so the compiler's contraction has nothing left to choose.
// A zero g' (zero gradient, no weight decay) on zero moments leaves p untouched: m = v = 0, d = eps, p - 0 / eps = p.
//
// 16 B read + 12 B written per parameter, HBM-bound; the two correctly rounded divisions and the square root are tens of VALU
// instructions per element beside the loads.  Matrix mode keeps 4 rows = 16 x 16 B loads in flight per
// lane (64 VGPRs of load results), nontemporal stores of p / m / v as in the SGD kernel: the updated words are next read one
// step later, after ~7 GB of other traffic, so they need no cache line.
#include "common.h"
#include "../../include/cim_hip.h"
#include "optim_stream.h"

namespace {

struct adam_consts {
    float b1, w1, b2, w2, eps;
};

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const adam_consts& k, float step_size,
                                            float bc2_sqrt, float wd) {
    const float gd = fmaf(wd, p, g);
    m = fmaf(k.b1, m, k.w1 * gd);
    v = fmaf(k.b2, v, k.w2 * (gd * gd));
    const float d = __fadd_rn(__builtin_sqrtf(v) / bc2_sqrt, k.eps);
    p = __fsub_rn(p, __fmul_rn(step_size, m) / d);
}

__device__ __forceinline__ void adam_update4(float4& pv, const float4& gv, float4& mv, float4& vv, const adam_consts& k,
                                             float step_size, float bc2_sqrt, float wd) {
    adam_update(pv.x, gv.x, mv.x, vv.x, k, step_size, bc2_sqrt, wd);
    adam_update(pv.y, gv.y, mv.y, vv.y, k, step_size, bc2_sqrt, wd);
    adam_update(pv.z, gv.z, mv.z, vv.z, k, step_size, bc2_sqrt, wd);
    adam_update(pv.w, gv.w, mv.w, vv.w, k, step_size, bc2_sqrt, wd);
}

// R rows of a matrix-mode tile: all 4 R loads of a lane are issued before the first update.  m[i] = max |p_new| of the lane's
// 4 columns of row i, cm = running column maxima.
template <int R>
__device__ __forceinline__ void adam_rows(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ea,
                                          float* __restrict__ es, size_t ld, const adam_consts& k, float step_size,
                                          float bc2_sqrt, float wd, uint4& cm, unsigned (&m)[R]) {
    float4 pv[R], gv[R], mv[R], vv[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        pv[i] = sgd_load(p + i * ld);
        gv[i] = sgd_load(g + i * ld);
        mv[i] = sgd_load(ea + i * ld);
        vv[i] = sgd_load(es + i * ld);
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        adam_update4(pv[i], gv[i], mv[i], vv[i], k, step_size, bc2_sqrt, wd);
        sgd_store(ea + i * ld, mv[i]);
        sgd_store(es + i * ld, vv[i]);
        sgd_store(p + i * ld, pv[i]);
        const unsigned ax = __float_as_uint(pv[i].x) & 0x7fffffffu, ay = __float_as_uint(pv[i].y) & 0x7fffffffu;
        const unsigned az = __float_as_uint(pv[i].z) & 0x7fffffffu, aw = __float_as_uint(pv[i].w) & 0x7fffffffu;
        cm.x = max(cm.x, ax); cm.y = max(cm.y, ay); cm.z = max(cm.z, az); cm.w = max(cm.w, aw);
        m[i] = max(max(ax, ay), max(az, aw));
    }
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const cim_adam_tensor* __restrict__ tensors,
                                                         const cim_sgd_chunk* __restrict__ chunks, int n_chunks,
                                                         double beta1, double beta2, double eps) {
  const adam_consts k = {(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
  for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    const cim_sgd_chunk ch = chunks[ci];
    const cim_adam_tensor t = tensors[ch.tensor];
    const float step_size = t.step_size, bc2_sqrt = t.bc2_sqrt, wd = t.wd;
    if (t.cols > 0) {
        // matrix mode: a 64-row x 1024-column tile per workgroup, a lane owns 4 consecutive columns (sgd.hip).
        // ch.offset = first row, ch.n = first column.
        const int r0 = (int)ch.offset, r1 = min((int)t.rows, r0 + 64);
        const int c = ch.n + threadIdx.x * 4;
        const bool cin = c < t.cols;
        const size_t ld = (size_t)t.cols;
        const size_t base = (size_t)r0 * ld + (cin ? c : 0);
        float* __restrict__ p = reinterpret_cast<float*>(t.p) + base;
        const float* __restrict__ g = reinterpret_cast<const float*>(t.g) + base;
        float* __restrict__ ea = reinterpret_cast<float*>(t.exp_avg) + base;
        float* __restrict__ es = reinterpret_cast<float*>(t.exp_avg_sq) + base;
        unsigned* row_amax = reinterpret_cast<unsigned*>(t.row_amax);
        unsigned* col_amax = reinterpret_cast<unsigned*>(t.col_amax);
        const bool lead = (threadIdx.x & 63) == 63;
        uint4 cm = make_uint4(0, 0, 0, 0);
        int r = r0;
        for (; r + 4 <= r1; r += 4, p += 4 * ld, g += 4 * ld, ea += 4 * ld, es += 4 * ld) {
            unsigned m[4] = {0, 0, 0, 0};
            if (cin) adam_rows<4>(p, g, ea, es, ld, k, step_size, bc2_sqrt, wd, cm, m);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned mm = sgd_wave_max(m[i]);
                if (lead) atomicMax(row_amax + r + i, mm);
            }
        }
        for (; r < r1; ++r, p += ld, g += ld, ea += ld, es += ld) {
            unsigned m[1] = {0};
            if (cin) adam_rows<1>(p, g, ea, es, ld, k, step_size, bc2_sqrt, wd, cm, m);
            const unsigned mm = sgd_wave_max(m[0]);
            if (lead) atomicMax(row_amax + r, mm);
        }
        if (cin) {
            atomicMax(col_amax + c, cm.x); atomicMax(col_amax + c + 1, cm.y);
            atomicMax(col_amax + c + 2, cm.z); atomicMax(col_amax + c + 3, cm.w);
        }
        continue;
    }
    float* __restrict__ p = reinterpret_cast<float*>(t.p) + ch.offset;
    const float* __restrict__ g = reinterpret_cast<const float*>(t.g) + ch.offset;
    float* __restrict__ ea = reinterpret_cast<float*>(t.exp_avg) + ch.offset;
    float* __restrict__ es = reinterpret_cast<float*>(t.exp_avg_sq) + ch.offset;
    const int n = min(ch.n, (int)(t.n - ch.offset));
    // 16-byte accesses need the four chunk bases aligned (chunk offsets are multiples of 4 elements)
    const bool aligned = ((t.p | t.g | t.exp_avg | t.exp_avg_sq) & 15) == 0;
    const int n4 = aligned ? (n & ~3) : 0;
    for (int i = threadIdx.x * 4; i < n4; i += 256 * 4) {
        float4 pv = *reinterpret_cast<const float4*>(p + i);
        const float4 gv = *reinterpret_cast<const float4*>(g + i);
        float4 mv = *reinterpret_cast<const float4*>(ea + i);
        float4 vv = *reinterpret_cast<const float4*>(es + i);
        adam_update4(pv, gv, mv, vv, k, step_size, bc2_sqrt, wd);
        *reinterpret_cast<float4*>(ea + i) = mv;
        *reinterpret_cast<float4*>(es + i) = vv;
        *reinterpret_cast<float4*>(p + i) = pv;
    }
    for (int i = n4 + threadIdx.x; i < n; i += 256) {      // unaligned tensors / tails
        float pv = p[i], mv = ea[i], vv = es[i];
        adam_update(pv, g[i], mv, vv, k, step_size, bc2_sqrt, wd);
        ea[i] = mv;
        es[i] = vv;
        p[i] = pv;
    }
  }
}

}  // namespace

extern "C" int cim_adam_multi(const cim_adam_tensor* tensors, const cim_sgd_chunk* chunks, int n_chunks, double beta1, double beta2,
                              double eps, int max_workgroups, void* stream) {
    CIM_CHECK_ARG((tensors != nullptr && chunks != nullptr) || n_chunks == 0);
    CIM_CHECK_ARG(n_chunks >= 0 && max_workgroups >= 0);
    CIM_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0);
    if (n_chunks == 0) return 0;
    const int grid = max_workgroups > 0 && max_workgroups < n_chunks ? max_workgroups : n_chunks;
    hipLaunchKernelGGL(adam_multi_kernel, dim3(grid), dim3(256), 0, cim::as_stream(stream), tensors, chunks, n_chunks, beta1, beta2, eps);
    CIM_CHECK_LAUNCH();
    return 0;
}
