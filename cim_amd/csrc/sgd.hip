// Fused multi-tensor SGD with momentum and weight decay for the 250-580 M parameters of the CIM models
// (SURVEY.md 8 f-4).  Replaces torch.optim.SGD(params, momentum=...) as constructed at
// the reference's tools/train.py:282-311 (two groups: weights, and biases at 2 x lr without weight decay) and stepped
// at :438; the update rule is torch.optim.SGD's (dampening 0, no Nesterov):
//     g' = g + wd * p ;   buf = momentum * buf + g' ;   p = p - lr * buf
// with buf zero-initialised (identical to torch's "first step: buf = g'").  The momentum buffers stay ordinary tensors
// in optimizer.state[p]['momentum_buffer'], so lib/utils/net.py:47-83 (update_learning_rate, _CorrectMomentum) and the
// checkpoint code work unchanged.
//
// One launch for ALL tensors.  Two device tables: `chunks` (tensor index + element offset of every 16384-element chunk;
// built once, it only depends on the tensor sizes) and `tensors` (cim_sgd_tensor: pointers, element count, lr, wd, matrix shape and |max|
// array pointers per tensor: 64 bytes each, refreshed per step - autograd hands out new gradient tensors every step, the chunk layout never changes).
// A workgroup streams one chunk with 16 B accesses: 12 B read + 8 B written per parameter, HBM-bound.  The walk over the two
// tables, the flat chunk and the matrix-mode tile are walk_chunks of optim_stream.h (shared with adam.hip); this file is the rule.
#include "common.h"
#include "optim_stream.h"

namespace {

struct SgdRule {
    static constexpr int NS = 1;
    using record = cim_sgd_tensor;
    using consts = float;                                // momentum
    static __device__ __forceinline__ uint64_t state(const record& t, int) { return t.buf; }
    float momentum, lr, wd;
    __device__ __forceinline__ SgdRule(const consts& k, const record& t) : momentum(k), lr(t.lr), wd(t.wd) {}
    __device__ __forceinline__ void operator()(float& p, float g, float (&s)[NS]) const {
        s[0] = fmaf(momentum, s[0], fmaf(wd, p, g));
        p = fmaf(-lr, s[0], p);
    }
};

__global__ __launch_bounds__(256) void sgd_multi_kernel(const cim_sgd_tensor* __restrict__ tensors,
                                                        const cim_sgd_chunk* __restrict__ chunks, int n_chunks, float momentum) {
    walk_chunks<SgdRule>(tensors, chunks, n_chunks, momentum);
}

}  // namespace

extern "C" int cim_sgd_multi(const cim_sgd_tensor* tensors, const cim_sgd_chunk* chunks, int n_chunks, float momentum,
                             int max_workgroups, void* stream) {
    CIM_CHECK_ARG((tensors != nullptr && chunks != nullptr) || n_chunks == 0);
    CIM_CHECK_ARG(n_chunks >= 0 && max_workgroups >= 0);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(sgd_multi_kernel, dim3(optim_grid(n_chunks, max_workgroups)), dim3(256), 0, cim::as_stream(stream), tensors, chunks, n_chunks, momentum);
    CIM_CHECK_LAUNCH();
    return 0;
}
