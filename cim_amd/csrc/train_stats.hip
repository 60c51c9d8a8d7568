// Training statistics on the device (lib/utils/training_stats.py:65-128, lib/utils/logging.py:60-85).
//   stats_push_kernel      one wave: reads the step's loss scalars through the addresses in its ARGUMENTS (autograd hands out new
//                          tensors every step), forms the total in the reference's order, accumulates over iter_size and commits
//                          to a ring of the last `window` values, an fp64 running sum and a sticky first-non-finite step
//   stats_summary_kernel   one wave: per key the median of the ring (np.median's), the last committed value and the global mean
// The state buffer is the caller's (cim_stats_bytes, zero-filled once); the library keeps nothing.  All loss arithmetic is fp32,
// one rounding per operation (__fadd_rn / __fdiv_rn: no contraction, no reciprocal).  No atomics: lane k owns column k.
#include "common.h"
#include "../../include/cim_hip.h"

namespace {

constexpr int kMaxCols = CIM_STATS_MAX_KEYS + 1;       // the tracked values and the total

struct PushArgs {                                      // a kernel argument: the step's addresses never visit device memory
    const float* value[CIM_STATS_MAX_KEYS];
    int n_values, n_sum, window, iter_size, inner;
};

// state: { uint32 count, first_nonfinite, 0, 0 } ; double sum[cols] ; float acc[cols rounded up to even] ; float ring[window][cols]
struct Layout {
    uint32_t* head;
    double* sum;
    float* acc;
    float* ring;
};
__host__ __device__ inline long long acc_floats(int cols) { return (cols + 1) & ~1; }
__host__ __device__ inline long long state_bytes(int cols, int window) {
    return 16 + 8ll * cols + 4 * acc_floats(cols) + 4ll * window * cols;
}
__device__ __forceinline__ Layout layout_of(void* state, int cols) {
    Layout l;
    char* p = static_cast<char*>(state);
    l.head = reinterpret_cast<uint32_t*>(p);
    l.sum = reinterpret_cast<double*>(p + 16);
    l.acc = reinterpret_cast<float*>(p + 16 + 8 * cols);
    l.ring = l.acc + acc_floats(cols);
    return l;
}

__device__ __forceinline__ bool finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(64) void stats_push_kernel(PushArgs a, void* state) {
    __shared__ float v[CIM_STATS_MAX_KEYS];
    const int k = threadIdx.x, cols = a.n_values + 1;
    const Layout s = layout_of(state, cols);
    const uint32_t count = s.head[0], first_bad = s.head[1];
    if (k < a.n_values) v[k] = *a.value[k];
    __syncthreads();
    bool bad = false;
    if (k < cols) {
        float x;
        if (k < a.n_values) {
            x = v[k];
        } else {                                        // the total: ((0 + v_0) + v_1) + ..., training_stats.py:72-77
            x = 0.0f;
            for (int j = 0; j < a.n_sum; ++j) x = __fadd_rn(x, v[j]);
        }
        bool commit = true;
        if (a.iter_size > 1) {                          // :87-128: sum(list) / iter_size, a true division
            x = __fadd_rn(a.inner == 0 ? 0.0f : s.acc[k], x);
            s.acc[k] = x;
            commit = a.inner == a.iter_size - 1;
            if (commit) x = __fdiv_rn(x, (float)a.iter_size);
        }
        if (commit) {
            s.ring[(count % (uint32_t)a.window) * cols + k] = x;
            s.sum[k] += (double)x;
            bad = !finite(x);
        }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (k == 0 && (a.iter_size == 1 || a.inner == a.iter_size - 1)) {
        s.head[0] = count + 1;
        if (any_bad && first_bad == 0) s.head[1] = count + 1;      // 1-based, written once
    }
}

// out: float [cols][3] = (median, last committed, global mean), then int32 [2] = (first non-finite step or 0, commits so far)
__global__ __launch_bounds__(64) void stats_summary_kernel(void* state, int cols, int window, float* __restrict__ out) {
    __shared__ float ring[CIM_STATS_MAX_WIN];
    __shared__ float mid[2];
    const int i = threadIdx.x;
    const Layout s = layout_of(state, cols);
    const uint32_t count = s.head[0];
    const int n = count < (uint32_t)window ? (int)count : window;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int k = 0; k < cols; ++k) {
        const float x = i < n ? s.ring[i * cols + k] : 0.0f;
        if (i < n) ring[i] = x;
        __syncthreads();
        int rank = 0;                                   // position in the ascending sort, ties in slot order
        for (int j = 0; j < n; ++j) {
            const float y = ring[j];
            rank += (y < x) || (y == x && j < i);
        }
        const bool has_nan = __ballot(i < n && x != x) != 0ull;
        if (i < n && rank == (n - 1) / 2) mid[0] = x;
        if (i < n && rank == n / 2) mid[1] = x;
        __syncthreads();
        if (i == 0) {
            float median = nan;
            if (n > 0 && !has_nan) median = (n & 1) ? mid[0] : __fdiv_rn(__fadd_rn(mid[0], mid[1]), 2.0f);
            out[3 * k + 0] = median;
            out[3 * k + 1] = n > 0 ? ring[(count - 1) % (uint32_t)window] : nan;
            out[3 * k + 2] = n > 0 ? (float)(s.sum[k] / (double)count) : nan;
        }
        __syncthreads();                                // `ring` and `mid` are rewritten for the next key
    }
    if (i == 0) {
        int32_t* tail = reinterpret_cast<int32_t*>(out + 3 * cols);
        tail[0] = (int32_t)s.head[1];
        tail[1] = (int32_t)count;
    }
}

}  // namespace

extern "C" long long cim_stats_bytes(int n_keys, int window) {
    if (n_keys < 1 || n_keys > CIM_STATS_MAX_KEYS || window < 1 || window > CIM_STATS_MAX_WIN) {
        cim::set_error("cim_stats_bytes: n_keys %d outside 1..%d or window %d outside 1..%d", n_keys, CIM_STATS_MAX_KEYS, window,
                       CIM_STATS_MAX_WIN);
        return -1;
    }
    return state_bytes(n_keys + 1, window);
}

extern "C" int cim_stats_push(const uint64_t* values_host, int n_values, int n_sum, int window, int iter_size, int inner, void* state,
                              void* stream) {
    CIM_CHECK_ARG(values_host != nullptr && state != nullptr);
    CIM_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0);
    CIM_CHECK_ARG(n_values >= 1 && n_values <= CIM_STATS_MAX_KEYS);
    CIM_CHECK_ARG(n_sum >= 0 && n_sum <= n_values);
    CIM_CHECK_ARG(window >= 1 && window <= CIM_STATS_MAX_WIN);
    CIM_CHECK_ARG(iter_size >= 1);
    CIM_CHECK_ARG(inner >= 0 && inner < iter_size);
    static_assert(kMaxCols <= 64 && CIM_STATS_MAX_WIN <= 64, "one lane per column / per window slot");
    PushArgs a = {};
    for (int k = 0; k < n_values; ++k) {
        CIM_CHECK_ARG(values_host[k] != 0 && (values_host[k] & 3) == 0);
        a.value[k] = reinterpret_cast<const float*>(values_host[k]);
    }
    a.n_values = n_values, a.n_sum = n_sum, a.window = window, a.iter_size = iter_size, a.inner = inner;
    hipLaunchKernelGGL(stats_push_kernel, dim3(1), dim3(64), 0, cim::as_stream(stream), a, state);
    CIM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cim_stats_summary(void* state, int n_keys, int window, float* out, void* stream) {
    CIM_CHECK_ARG(state != nullptr && out != nullptr);
    CIM_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0);
    CIM_CHECK_ARG(n_keys >= 1 && n_keys <= CIM_STATS_MAX_KEYS);
    CIM_CHECK_ARG(window >= 1 && window <= CIM_STATS_MAX_WIN);
    hipLaunchKernelGGL(stats_summary_kernel, dim3(1), dim3(64), 0, cim::as_stream(stream), state, n_keys + 1, window, out);
    CIM_CHECK_LAUNCH();
    return 0;
}
