// The single-workgroup fit kernels with 512 threads per fit -- LDS-staged k_svgp_fit<WPS, KMIN> (fit_staged.h) and
// strip-streaming k_svgp_fit_strip<D> (fit_strip.h) -- with their launch functions and the router's queries (common.h).
// One translation unit on purpose: the backend derives a __noinline__ callee's register budget (diag_factor_invert,
// ...) from every kernel of the module that calls it, and the inliner's decisions depend on which callers share a
// module and in which order they are instantiated (staged first: fit_strip.h comes after the staged launcher).
#include "fit_staged.h"

long long gapro_fit_staged_lds_bytes(int m, int feat_dim) { return staged_lds_bytes(m, feat_dim); }
bool gapro_fit_staged_ok(int m, int feat_dim) { return staged_ok(m, feat_dim); }

int gapro_launch_fit_staged(hipStream_t stream, int wps, bool kmin, int n_fits, int n_wg, unsigned* d_ticket,
                            int feat_dim, size_t lds_bytes, const float* d_feats_spp, const int* d_idx,
                            const gapro_fit_desc* d_descs, const double* d_init_mean, const gapro_fit_options& opt,
                            double* d_workspace, float* d_probs, float* d_probs_new, unsigned char* d_labels,
                            float* d_mu, float* d_var, int* d_fit_status, double* d_fit_loss) {
  if (wps != 2 && (wps != kWavesPerSimd || !kmin)) return GAPRO_ERR_BAD_ARG;
  auto kern = !kmin ? k_svgp_fit<2, false> : wps == 2 ? k_svgp_fit<2, true> : k_svgp_fit<kWavesPerSimd, true>;
  if (lds_bytes > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return GAPRO_ERR_HIP;
  hipLaunchKernelGGL(kern, dim3(n_wg), dim3(NT), lds_bytes, stream, n_fits, feat_dim, d_feats_spp, d_idx, d_descs,
                     d_init_mean, opt, d_workspace, d_probs, d_probs_new, d_labels, d_mu, d_var, d_fit_status,
                     d_fit_loss, d_ticket);
  return hipGetLastError() == hipSuccess ? GAPRO_OK : GAPRO_ERR_HIP;
}

#include "fit_strip.h"

long long gapro_fit_strip_lds_bytes(int m, int feat_dim) { return strip_lds_bytes(m, feat_dim); }
bool gapro_fit_strip_ok(int m, int feat_dim) { return strip_ok(m, feat_dim); }

int gapro_launch_fit_strip(hipStream_t stream, int n_fits, int n_wg, unsigned* d_ticket, int feat_dim,
                           size_t lds_bytes, const float* d_feats_spp, const int* d_idx, const gapro_fit_desc* d_descs,
                           const double* d_init_mean, const gapro_fit_options& opt, double* d_workspace,
                           float* d_probs, float* d_probs_new, unsigned char* d_labels, float* d_mu, float* d_var,
                           int* d_fit_status, double* d_fit_loss) {
  return launch_fit_strip(stream, n_fits, n_wg, d_ticket, feat_dim, lds_bytes, d_feats_spp, d_idx, d_descs,
                          d_init_mean, opt, d_workspace, d_probs, d_probs_new, d_labels, d_mu, d_var, d_fit_status,
                          d_fit_loss);
}
