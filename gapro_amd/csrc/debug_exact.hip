// Debug: the exact-sum rule, conversion and mean of exact_sum.h evaluated elementwise on the host or on the device, for
// tests/test_exact_sum_cpu.py (host leg against the oracle) and tests/test_exact_sum_gpu.py (device leg against the host).
#include "common.h"
#include "exact_sum.h"

namespace {

struct ExactArgs {
  int n_shift; const double* absmax; const long long* n; int* shift_out;
  int n_fixed; const double* x; const int* xk; long long* fixed_out;
  int n_mean; const long long* sum; const int* mk; const double* count; double* mean_out;
};

__host__ __device__ inline void exact_eval(const ExactArgs& a, int first, int step) {
  for (int i = first; i < a.n_shift; i += step) a.shift_out[i] = fixed_point_shift(a.absmax[i], a.n[i]);
  for (int i = first; i < a.n_fixed; i += step) a.fixed_out[i] = to_fixed(a.x[i], a.xk[i]);
  for (int i = first; i < a.n_mean; i += step) a.mean_out[i] = fixed_mean(a.sum[i], a.mk[i], a.count[i]);
}

__global__ __launch_bounds__(256) void k_exact_sum(ExactArgs a) { exact_eval(a, threadIdx.x, 256); }

}  // namespace

extern "C" int gapro_debug_exact_sum(gapro_ctx* ctx, void* stream_, int32_t n_shift, const double* absmax,
                                     const int64_t* n, int32_t* shift_out, int32_t n_fixed, const double* x,
                                     const int32_t* xk, int64_t* fixed_out, int32_t n_mean, const int64_t* sum,
                                     const int32_t* mk, const double* count, double* mean_out) {
  if (n_shift < 0 || n_fixed < 0 || n_mean < 0 || (n_shift && (!absmax || !n || !shift_out)) ||
      (n_fixed && (!x || !xk || !fixed_out)) || (n_mean && (!sum || !mk || !count || !mean_out)) || (!ctx && stream_))
    return GAPRO_ERR_BAD_ARG;
  const ExactArgs a = {n_shift, absmax, (const long long*)n, shift_out, n_fixed, x, xk, (long long*)fixed_out,
                       n_mean, (const long long*)sum, mk, count, mean_out};
  if (!ctx) {  // host leg: host pointers
    exact_eval(a, 0, 1);
    return GAPRO_OK;
  }
  hipLaunchKernelGGL(k_exact_sum, dim3(1), dim3(256), 0, (hipStream_t)stream_, a);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}
