// Debug entry points of include/gapro_hip_debug.h (libgapro_hip_debug.so, never loaded by the product) on fit_wg.h:
// product-engine bench, MFMA lane-map self test, the fit kernels' special functions, counter calibration streams.
#include "fit_wg.h"
#include "../../include/gapro_hip_debug.h"
#include "mfma64.h"

namespace {
// ---- product engines side by side (debug entry, tools/product_bench.py) --------------------------------
// Every workgroup owns three M_p x M_p matrices (P, Q, C) of a slab and computes C = P^T Q `reps` times with one of the
// staged kernel's product engines, plain-store epilogue: engine 0 = gemm_tn with 32 x 32 wave tiles, 1 = 64 x 64 wave
// tiles, 2 = the workgroup-tiled form (gemm_wg on whole 128 x 128 tiles + per-wave strips at the edge).  shape 0: full contraction range; 1: the
// range [0, i0 + 16) of a lower-triangular P (the A = L^-1 K product's); 2: lower-triangular output, full range.
template <int ENGINE>
__global__ __launch_bounds__(NT, 2) void k_product_bench(int Mp, int reps, int shape, double* __restrict__ slab) {
  extern __shared__ double dyn_lds[];
  ldsd* scratch = (ldsd*)dyn_lds;
  gd* P = (gd*)slab + (size_t)blockIdx.x * 3 * Mp * Mp;
  gd* Q = P + (size_t)Mp * Mp;
  gd* Cm = Q + (size_t)Mp * Mp;
  if (threadIdx.x == 0) {
    g_sh.f.M = Mp;
    g_sh.f.M1 = Mp / 2;
    g_sh.f.Mp = Mp;
  }
  __syncthreads();
  const int shp = shape;
  constexpr int TSZ = ENGINE == 0 ? 32 : ENGINE == 1 ? 64 : 16;  // the engine's own tile: kr is asked per tile
  auto kr = [=](int i0, int j0, int* lo, int* hi) {
    // shapes 3 .. 5 (the caller zeroes the matching triangles of P and Q, so that any superset of a range gives the
    // same bits): 3 = [max(i0, j0), Mp) (T1), 4 = [j0, Mp) (B, G), 5 = [i0, Mp) (G_KX, Pm; with a lower output)
    *lo = shp == 3 ? (i0 > j0 ? i0 : j0) : shp == 4 ? j0 : shp == 5 ? i0 : 0;
    *hi = shp == 1 ? i0 + TSZ : Mp;
  };
  auto epi = [=](int i0, int j0, const d4& v) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) Cm[(size_t)(i0 + lq + 4 * r) * Mp + j0 + lr] = v[r];
  };
  for (int r = 0; r < reps; ++r) {
    if (ENGINE == 0) gemm_tn<2, false, 2, ORD_ROWS_DESC, true>(Mp / 16, Mp / 16, shp == 2 || shp == 5, P, Q, Mp, nullptr, kr, epi);
    else if (ENGINE == 1) gemm_tn<4, false, 2, ORD_ROWS_DESC, true>(Mp / 32, Mp / 32, shp == 2 || shp == 5, P, Q, Mp, nullptr, kr, epi);
    else if (ENGINE == 2) product<4, 1, false, ORD_ROWS_DESC>(Mp / 16, Mp / 16, shp == 2 || shp == 5, P, Q, Mp, nullptr, kr, epi, scratch);
    else return;  // (engine 3 was a two-team form of engine 2: no faster, taken out again -- DESIGN 6.0)
    __syncthreads();
  }
}

// ---- MFMA layout self-test (debug entry, used by tests/test_fit_gpu.py) ------------------------------
__global__ void k_mfma_selftest(const double* __restrict__ P, const double* __restrict__ Q, double* __restrict__ C,
                                int K) {
  // C[16][16] = sum_k P[k][i] Q[k][j], ld = 16
  const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < K; k += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(P[(k + lq) * 16 + lr], Q[(k + lq) * 16 + lr], acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) C[(lq + 4 * r) * 16 + lr] = acc[r];
  if (K < 0) {  // never taken: keeps the four-block form of mfma64.h (an experiment of round 3) compiling (debug TU)
    d4 t = (d4){0.0, 0.0, 0.0, 0.0};
    gapro_mfma::mma16(P[lr], Q[lr], t);
    t = gapro_mfma::unrotate(t);
    C[lane] = t[0];
  }
}

}  // namespace

__global__ void k_stream_calib(long long n, const double* __restrict__ src, double* __restrict__ dst, int mode) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = src[i];
    if (mode == 1) dst[i] = v;
    else acc += v;
  }
  if (mode == 0) {
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&dst[blockIdx.x], acc);
  }
}

extern "C" {

// Debug: the staged kernel's product engines side by side (k_product_bench); d_slab: n_wg * 3 * mp * mp doubles,
// filled by the caller.  Returns the launch's milliseconds (HIP events on `stream`, blocking) in *out_ms.
int gapro_debug_product_bench(gapro_ctx* ctx, void* stream_, int32_t engine, int32_t shape, int32_t mp, int32_t reps,
                              int32_t n_wg, double* d_slab, float* out_ms) {
  if (!ctx || !d_slab || !out_ms || engine < 0 || engine > 2 || shape < 0 || shape > 5 || mp < 128 || mp % 32 ||
      reps <= 0 || n_wg <= 0)
    return GAPRO_ERR_BAD_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const int lds = 8 * kWgRingDoubles + 1024;
  hipEvent_t e0, e1;
  GAPRO_HIP_CHECK(ctx, hipEventCreate(&e0));
  GAPRO_HIP_CHECK(ctx, hipEventCreate(&e1));
  auto launch = [&](int n) -> int {
#define GAPRO_PB(E)                                                                                              \
  do {                                                                                                           \
    GAPRO_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_product_bench<E>,                                    \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds));                 \
    hipLaunchKernelGGL(k_product_bench<E>, dim3(n_wg), dim3(NT), (size_t)lds, stream, (int)mp, n, (int)shape, d_slab); \
  } while (0)
    if (engine == 0) GAPRO_PB(0);
    else if (engine == 1) GAPRO_PB(1);
    else GAPRO_PB(2);
#undef GAPRO_PB
    return GAPRO_OK;
  };
  if (launch(1) != GAPRO_OK) return GAPRO_ERR_HIP;
  GAPRO_HIP_CHECK(ctx, hipEventRecord(e0, stream));
  if (launch(reps) != GAPRO_OK) return GAPRO_ERR_HIP;
  GAPRO_HIP_CHECK(ctx, hipEventRecord(e1, stream));
  GAPRO_HIP_CHECK(ctx, hipEventSynchronize(e1));
  GAPRO_HIP_CHECK(ctx, hipEventElapsedTime(out_ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

// Debug: C = P^T Q for 16-column operands with K rows (K % 4 == 0); checks the MFMA lane maps.
int gapro_debug_mfma_tn(gapro_ctx* ctx, void* stream_, const double* d_P, const double* d_Q, double* d_C, int32_t K) {
  if (!ctx || !d_P || !d_Q || !d_C || K <= 0 || (K & 3)) return GAPRO_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_mfma_selftest, dim3(1), dim3(64), 0, (hipStream_t)stream_, d_P, d_Q, d_C, (int)K);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

// Debug: streaming kernels with a known byte count in this library's own access pattern (one double per
// lane, grid-stride), used to calibrate the FETCH_SIZE / WRITE_SIZE counters.  mode 0: read n doubles and
// write one partial sum per workgroup; mode 1: copy n doubles.
// Debug: the fit kernels' own special functions (fit_math.h) evaluated elementwise, for tests/test_fit_gpu.py
__global__ void k_fit_math(long long n, const double* __restrict__ x, double* __restrict__ out, int which) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double lp, r;
  switch (which) {
    case 0: out[i] = gapro_fit_math::erfcx_tab(x[i]); break;
    case 1: out[i] = gapro_fit_math::exp_neg(x[i]); break;
    case 2: out[i] = gapro_fit_math::ndtr_ratio(x[i]); break;
    default:
      gapro_fit_math::log_ndtr_ratio_erfcx(x[i], &lp, &r);
      out[i] = which == 3 ? lp : r;
  }
}
int gapro_debug_fit_math(gapro_ctx* ctx, void* stream_, int64_t n, const double* d_x, double* d_out, int32_t which) {
  if (!ctx || !d_x || !d_out || n <= 0 || which < 0 || which > 4) return GAPRO_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_fit_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, (long long)n, d_x,
                     d_out, (int)which);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_debug_stream(gapro_ctx* ctx, void* stream_, int64_t n, const double* d_src, double* d_dst, int32_t mode) {
  if (!ctx || !d_src || !d_dst || n <= 0 || mode < 0 || mode > 1) return GAPRO_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_stream_calib, dim3(4096), dim3(256), 0, (hipStream_t)stream_, (long long)n, d_src, d_dst,
                     (int)mode);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
