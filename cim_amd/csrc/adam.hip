// Fused multi-tensor Adam for the 250-580 M parameters of the CIM models: torch.optim.Adam(params) as constructed at
// tools/train.py:310-311 (SOLVER.TYPE Adam; L2 weight decay, no amsgrad, no maximize), ONE launch for all tensors in the
// two-table form of sgd.hip: chunk table, max_workgroups walk and matrix mode with its by-products are the ONE walk_chunks of
// optim_stream.h; this file is the rule.
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
#include "optim_stream.h"

namespace {

struct AdamRule {
    static constexpr int NS = 2;
    using record = cim_adam_tensor;
    struct consts {
        float b1, w1, b2, w2, eps;
    };
    static __device__ __forceinline__ uint64_t state(const record& t, int k) { return k == 0 ? t.exp_avg : t.exp_avg_sq; }
    consts k;
    float step_size, bc2_sqrt, wd;
    __device__ __forceinline__ AdamRule(const consts& k, const record& t) : k(k), step_size(t.step_size), bc2_sqrt(t.bc2_sqrt), wd(t.wd) {}
    __device__ __forceinline__ void operator()(float& p, float g, float (&s)[NS]) const {
        float &m = s[0], &v = s[1];
        const float gd = fmaf(wd, p, g);
        m = fmaf(k.b1, m, k.w1 * gd);
        v = fmaf(k.b2, v, k.w2 * (gd * gd));
        const float d = __fadd_rn(__builtin_sqrtf(v) / bc2_sqrt, k.eps);
        p = __fsub_rn(p, __fmul_rn(step_size, m) / d);
    }
};

__global__ __launch_bounds__(256) void adam_multi_kernel(const cim_adam_tensor* __restrict__ tensors,
                                                         const cim_sgd_chunk* __restrict__ chunks, int n_chunks,
                                                         double beta1, double beta2, double eps) {
    const AdamRule::consts k = {(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
    walk_chunks<AdamRule>(tensors, chunks, n_chunks, k);
}

}  // namespace

extern "C" int cim_adam_multi(const cim_adam_tensor* tensors, const cim_sgd_chunk* chunks, int n_chunks, double beta1, double beta2,
                              double eps, int max_workgroups, void* stream) {
    CIM_CHECK_ARG((tensors != nullptr && chunks != nullptr) || n_chunks == 0);
    CIM_CHECK_ARG(n_chunks >= 0 && max_workgroups >= 0);
    CIM_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(adam_multi_kernel, dim3(optim_grid(n_chunks, max_workgroups)), dim3(256), 0, cim::as_stream(stream), tensors, chunks, n_chunks, beta1, beta2, eps);
    CIM_CHECK_LAUNCH();
    return 0;
}
