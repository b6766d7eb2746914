// The single-workgroup fit kernels with 512 threads per fit -- LDS-staged k_svgp_fit<WPS, KMIN> (fit_staged.h) and
// strip-streaming k_svgp_fit_strip<D> (fit_strip.h, which ends in its launch function) -- with the staged kernel's
// launch function and the router's queries (common.h).
// One translation unit on purpose: the backend derives a __noinline__ callee's register budget (diag_factor_invert,
// ...) from every kernel of the module that calls it, and the inliner's decisions depend on which callers share a
// module and in which order they are instantiated (staged first: fit_strip.h comes after the staged launcher).
#include "fit_staged.h"

long long gapro_fit_staged_lds_bytes(int m, int feat_dim) { return staged_lds_bytes(m, feat_dim); }
bool gapro_fit_staged_ok(int m, int feat_dim) { return staged_ok(m, feat_dim); }

int gapro_launch_fit_staged(hipStream_t stream, const FitLaunchStep& s, const FitArgs& a) {
  const int wps = s.variant & ~GAPRO_FIT_STEP_COPY_FREE;
  const bool kmin = (s.variant & GAPRO_FIT_STEP_COPY_FREE) != 0;
  if (wps != 2 && (wps != kWavesPerSimd || !kmin)) return GAPRO_ERR_BAD_ARG;
  auto kern = !kmin ? k_svgp_fit<2, false> : wps == 2 ? k_svgp_fit<2, true> : k_svgp_fit<kWavesPerSimd, true>;
  const size_t lds_bytes = (size_t)s.lds_bytes;
  if (lds_bytes > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return GAPRO_ERR_HIP;
  hipLaunchKernelGGL(kern, dim3(s.grid), dim3(NT), lds_bytes, stream, s.count, a.feat_dim, a.d_feats_spp, a.d_idx,
                     a.d_descs + s.first, a.d_init_mean, *a.opt, a.d_workspace, a.d_probs, a.d_probs_new, a.d_labels,
                     a.d_mu, a.d_var, a.d_fit_status, a.d_fit_loss, gapro_fit_ticket(s, a));
  return hipGetLastError() == hipSuccess ? GAPRO_OK : GAPRO_ERR_HIP;
}

#include "fit_strip.h"

long long gapro_fit_strip_lds_bytes(int m, int feat_dim) { return strip_lds_bytes(m, feat_dim); }
bool gapro_fit_strip_ok(int m, int feat_dim) { return strip_ok(m, feat_dim); }
