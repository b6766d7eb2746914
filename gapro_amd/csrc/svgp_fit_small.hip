// Small-fit translation unit: the strip-streaming fit kernel of fit_strip.h with 256 threads per fit for M_p <= 64.
// M_p <= 64 has at most 8 tiles per strip product: with 8 waves each wave has one tile and the CU idles through every
// memory round trip of the fit it hosts.  Here a fit gets 4 waves (256 VGPRs each, no tighter register budget than
// the 512-thread kernel) and a CU hosts TWO fits.
#define GAPRO_NT 256
#define k_svgp_fit_strip k_svgp_fit_strip256  // distinct kernel name in profiles
#define GAPRO_LAUNCH_FIT_STRIP gapro_launch_fit_strip_small
#include "fit_strip.h"

// LDS bytes of a small fit in THIS translation unit's layout (NT-dependent reduction scratch)
long long gapro_fit_strip_small_lds_bytes(int m, int feat_dim) { return strip_lds_bytes(m, feat_dim); }
