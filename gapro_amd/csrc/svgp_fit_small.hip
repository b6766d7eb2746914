// Small-fit translation unit: the strip-streaming fit kernel of fit_strip.h with 256 threads per fit for M_p <= 64.
// M_p <= 64 has at most 8 tiles per strip product: with 8 waves each wave has one tile and the CU idles through every
// memory round trip of the fit it hosts.  Here a fit gets 4 waves (256 VGPRs each, no tighter register budget than
// the 512-thread kernel) and a CU hosts TWO fits.
#define GAPRO_NT 256
#define k_svgp_fit_strip k_svgp_fit_strip256  // distinct kernel name in profiles
#include "fit_strip.h"

// LDS bytes of a small fit in THIS translation unit's layout (NT-dependent reduction scratch)
long long gapro_fit_strip_small_lds_bytes(int m, int feat_dim) { return strip_lds_bytes(m, feat_dim); }

int gapro_launch_fit_strip_small(hipStream_t stream, int n_fits, int n_wg, unsigned* d_ticket, int feat_dim,
                                 size_t lds_bytes, const float* d_feats_spp, const int* d_idx,
                                 const gapro_fit_desc* d_descs, const double* d_init_mean,
                                 const gapro_fit_options& opt, double* d_workspace, float* d_probs, float* d_probs_new,
                                 unsigned char* d_labels, float* d_mu, float* d_var, int* d_fit_status,
                                 double* d_fit_loss) {
  return launch_fit_strip(stream, n_fits, n_wg, d_ticket, feat_dim, lds_bytes, d_feats_spp, d_idx, d_descs,
                          d_init_mean, opt, d_workspace, d_probs, d_probs_new, d_labels, d_mu, d_var, d_fit_status,
                          d_fit_loss);
}
