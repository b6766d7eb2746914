// Scalar pieces of the SVGP fit shared by every fit kernel of libgapro_hip.so (fit_wg.h and the kernels built on it,
// svgp_fit_cluster.hip, svgp_fit_large.hip, svgp_fit_wave.hip): Gauss-Hermite rule, link functions, likelihood terms,
// wave- and workgroup-level helpers.  Where two kernels compute a piece in a different order or form, both forms are
// here under names that say which one each is, and every kernel keeps the form it was validated with.
#pragma once
#include <math.h>

#include "common.h"
#include "erfcx_table.h"

namespace gapro_fit_math {

// LDS and workspace pointers carry their address space: ds_read/ds_write and global_load/global_store with counted
// vmcnt waits instead of flat_* accesses (unordered completion, vmcnt(0)) and generic->local casts
typedef __attribute__((address_space(3))) double ldsd;
typedef __attribute__((address_space(1))) double gd;

// erfcx(x) = exp(x^2) erfc(x) for x >= 0, the special function of the likelihood phase (two per Gauss-Hermite node pair
// and training point, 50 times per fit).  The math library's erfcx is ~200 instructions over five data-dependent
// branches, and the ten node pairs of a point straddle its ranges, so a wave walks several of them.  Here:
//     erfcx(x) = t Q(t),  t = 2 / (2 + x),  Q = a degree-8 polynomial per sixteenth of t in [0, 1]
// (tools/gen_erfcx_table.py: interpolation error 3e-17, the evaluation within ~2 ulp of the true value): one division,
// five 16-byte loads from a 1.3 KB table, eight FMAs, no branch.  x = inf gives 0, NaN stays NaN.
struct alignas(16) ErfcxRow {
  double c[10];
};
static __constant__ const ErfcxRow kErfcxTab[16] = {GAPRO_ERFCX_TABLE_ROWS};
__device__ inline double erfcx_tab(double x) {
  const double t = 2.0 / (2.0 + x);
  const double tk = 16.0 * t;
  int k = (int)tk;
  k = k > 15 ? 15 : k;
  const double u = fma(2.0, tk - (double)k, -1.0);
  const double* c = kErfcxTab[k].c;
  double p = c[8];
#pragma unroll
  for (int j = 7; j >= 0; --j) p = fma(p, u, c[j]);
  return t * p;
}

// numpy.polynomial.hermite.hermgauss(20): positive nodes (ascending) and their weights; the rule is symmetric.
// Printed with repr() from NumPy 2.2.  (gpytorch settings.num_gauss_hermite_locs = 20)
#define GAPRO_GH_NODES                                                                                             \
  0.24534070830090124, 0.7374737285453944, 1.234076215395323, 1.7385377121165861, 2.2549740020892757,             \
      2.7888060584281305, 3.3478545673832163, 3.944764040115625, 4.603682449550744, 5.387480890011233
#define GAPRO_GH_WEIGHTS                                                                                           \
  0.4622436696006101, 0.28667550536283415, 0.1090172060200233, 0.024810520887463643, 0.0032437733422378567,        \
      0.00022833863601635365, 7.80255647853206e-06, 1.0860693707692782e-07, 4.3993409922731747e-10,                 \
      2.2293936455341447e-13
// compile-time copy (the wave-per-fit kernel stages it into LDS) and constant-memory copy (indexed at run time by the
// workgroup kernels' quadrature loops); one per translation unit
constexpr double kGhT[10] = {GAPRO_GH_NODES};
constexpr double kGhW[10] = {GAPRO_GH_WEIGHTS};
static __constant__ double c_gh_t[10] = {GAPRO_GH_NODES};
static __constant__ double c_gh_w[10] = {GAPRO_GH_WEIGHTS};

// exp(x) for x <= 0: the RBF kernel values (Cholesky input, K_ZX, both kernel-gradient passes: one per pair of points and
// step) and the Gaussian factor of the likelihood.  The math library's exp is 56 instructions (overflow, subnormal and
// directed cases of the full range); here: k = rint(x / ln 2), r = x - k ln 2 (two-part constant, |r| <= 0.347), the Taylor
// polynomial of degree 13 (remainder 4e-18), v_ldexp -- 22 instructions, ~1 ulp.  Arguments below -745 give the same
// subnormal-or-zero as -745; NaN stays NaN.
__device__ inline double exp_neg(double x) {
  x = x < -745.0 ? -745.0 : x;
  const double k = rint(x * 1.4426950408889634074);
  double r = fma(k, -6.93147180369123816490e-01, x);
  r = fma(k, -1.90821492927058770002e-10, r);
  double p = 1.6059043836821613e-10;
  p = fma(p, r, 2.08767569878681e-09);
  p = fma(p, r, 2.505210838544172e-08);
  p = fma(p, r, 2.755731922398589e-07);
  p = fma(p, r, 2.7557319223985893e-06);
  p = fma(p, r, 2.48015873015873e-05);
  p = fma(p, r, 0.0001984126984126984);
  p = fma(p, r, 0.001388888888888889);
  p = fma(p, r, 0.008333333333333333);
  p = fma(p, r, 0.041666666666666664);
  p = fma(p, r, 0.16666666666666666);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)k);
}

// What the fit kernels call.  Default: the math library's functions.  -DGAPRO_FAST_LIK_MATH: the two above -- measured
// +0 .. 3 % per size (the likelihood phase -37 %), +0 .. 1.5 % on the headline, but NOT the default: the one
// ill-conditioned fit of the S3DIS-shaped test scene amplifies any change of rounding by ~1e11 (the oracle's own two
// float64 implementations differ by 3e-6 .. 3e-5 on it), and with these functions the kernel lands 1.1e-4 from the
// autograd oracle there -- beyond north_star's 1e-4 -- where the library functions' bits land at < 8e-5.  Neither is
// "more right"; the pinned one stays.  (LABNOTES R5.5)
#ifdef GAPRO_FAST_LIK_MATH
__device__ inline double lik_erfcx(double x) { return erfcx_tab(x); }
__device__ inline double rbf_exp(double x) { return exp_neg(x); }
#else
__device__ inline double lik_erfcx(double x) { return erfcx(x); }
__device__ inline double rbf_exp(double x) { return exp(x); }
#endif

__device__ inline double softplus(double x) { return log1p(exp(-fabs(x))) + fmax(x, 0.0); }
__device__ inline double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// log Phi(z) and r(z) = phi(z)/Phi(z), both tails stable, in two forms.
//
// log_ndtr_ratio_erfcx (staged, strip and wave-per-fit kernels).  The oracle (oracle/svgp_oracle.py) branches on the
// sign of z -- erfcx for z < 0, erfc for z >= 0 -- and the ten quadrature nodes of a point straddle zero, so a wave ran
// both branches (erfcx, log, erfc, log1p, exp: the likelihood phase was 6 .. 10 % of a step of the strip kernels, 4 .. 7 %
// of the staged kernel's).  Here both signs share t = erfcx(|z| / sqrt 2) and e = exp(-z^2 / 2):
//   z <  0:  Phi = e t / 2          log Phi = log(t / 2) - z^2 / 2     r = sqrt(2 / pi) / t
//   z >= 0:  Phi = 1 - e t / 2      log Phi = log(1 - e t / 2)         r = e / (sqrt(2 pi) Phi)
// -- three library calls and two selects.  erfc(x) = e t to the last bit or two; log(1 - tail) instead of log1p(-tail)
// is absolutely accurate to 1e-16, and log Phi only enters the reported ELBO value.
__device__ inline void log_ndtr_ratio_erfcx(double z, double* lp, double* r) {
  const double rs2 = 0.70710678118654752440;
  const double t = lik_erfcx(fabs(z) * rs2);
  const double hz2 = 0.5 * z * z;
  const double e = rbf_exp(-hz2);
  const bool neg = z < 0.0;
  const double phi_pos = 1.0 - 0.5 * e * t;  // Phi(z) for z >= 0
  *lp = log(neg ? 0.5 * t : phi_pos) - (neg ? hz2 : 0.0);
  *r = (neg ? 0.79788456080286535588 : e * 0.39894228040143267794) / (neg ? t : phi_pos);  // one division
}

// r(z) alone, the same bits as log_ndtr_ratio_erfcx's: log Phi only enters the ELBO VALUE, which is reported after the
// last step and read by nobody before it -- 49 of 50 steps need no log (a quarter of the instructions of an evaluation)
__device__ inline double ndtr_ratio(double z) {
  const double t = lik_erfcx(fabs(z) * 0.70710678118654752440);
  const double e = rbf_exp(-0.5 * z * z);
  const bool neg = z < 0.0;
  return (neg ? 0.79788456080286535588 : e * 0.39894228040143267794) / (neg ? t : 1.0 - 0.5 * e * t);
}

// log_ndtr_ratio_branchy (cluster and generic kernels): the oracle's branches on the sign of z
__device__ inline void log_ndtr_ratio_branchy(double z, double* lp, double* r) {
  const double rs2 = 0.70710678118654752440;
  if (z < 0.0) {
    const double ex = erfcx(-z * rs2);
    *lp = log(0.5 * ex) - 0.5 * z * z;
    *r = 0.79788456080286535588 / ex;  // sqrt(2/pi) / erfcx
  } else {
    const double tail = 0.5 * erfc(z * rs2);
    *lp = log1p(-tail);
    *r = exp(-0.5 * z * z) * 0.39894228040143267794 / (1.0 - tail);
  }
}

// value of `v` in lane `lane` (wave-uniform, compile-time after unrolling): v_readlane, no LDS crossbar
__device__ inline double lane_bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Function arguments of non-kernel functions arrive in VGPRs; these make wave-uniform values scalar again
// so that loop control and address arithmetic run on the scalar unit.
__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T>
__device__ inline T* uni_ptr(T* p) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return (T*)(((unsigned long long)hi << 32) | lo);
}
// a wave-uniform double as a scalar (SGPR pair): loop-invariant values the register allocator would otherwise hold in
// -- or spill from -- vector registers (VALU instructions take one scalar operand for free)
__device__ inline double uni_d(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// Wave sums in two forms that add in a different order.  wave_sum_shfl: the __shfl_xor butterfly (ds_bpermute) of the
// workgroup kernels (staged, strip, cluster, generic); block_sum_shfl sums NW waves' results through `red` (NW doubles
// of LDS) in a fixed order, every thread gets the total.
__device__ inline double wave_sum_shfl(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int NW>
__device__ inline double block_sum_shfl(double v, double* red) {
  v = wave_sum_shfl(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < NW; ++w) t += red[w];
  return t;
}

// wave_sum_dpp (wave-per-fit kernel): cross-lane sums on the VALU (no LDS crossbar: ds_bpermute costs ~100 cycles of
// latency per hop and __shfl_xor compiles to it).
//   v_permlane32_swap exchanges the wave's halves, v_permlane16_swap odd and even rows of 16 (both new on gfx950);
//   within a row the hops are DPP moves (quad_perm, row_half_mirror, row_mirror).
// Fixed tree: every lane ends with the same bits.
template <int CTRL>
__device__ inline double dpp_mov(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ inline double sum_xor32(double v) {  // v[l] + v[l ^ 32]
  const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ inline double sum_xor16(double v) {  // v[l] + v[l ^ 16]
  const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
// sum over the four rows of 16 lanes: every lane gets the total of its column lr
__device__ inline double sum_rows(double v) { return sum_xor32(sum_xor16(v)); }
__device__ inline double wave_sum_dpp(double v) {
  v += dpp_mov<0xB1>(v);   // quad_perm(1, 0, 3, 2)
  v += dpp_mov<0x4E>(v);   // quad_perm(2, 3, 0, 1)
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror
  return sum_rows(v);
}

}  // namespace gapro_fit_math
