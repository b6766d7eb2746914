// Single-workgroup machinery of the batched whitened-SVGP classifier fit for gfx950 (MI355X): one workgroup = one GP fit,
// the whole Adam loop inside one launch.  Shared by the LDS-staged kernel (fit_staged.h: k_svgp_fit<WPS, KMIN>,
// 128 < M_p <= 512) and the strip-streaming kernel (fit_strip.h: k_svgp_fit_strip<D>, M_p <= 128) and parameterised
// by GAPRO_NT, the threads per fit: svgp_fit_wg.hip builds both kernels with 512, svgp_fit_small.hip the strip kernel
// with 256 (M_p <= 64), svgp_fit_debug.hip the debug entry points on these products.  Everything here lives in an
// anonymous namespace, one copy per translation unit.  svgp_fit.hip routes the fits of a launch;
// svgp_fit_cluster.hip spreads one large fit over several workgroups; svgp_fit_large.hip is the generic fallback
// (D > 32) with the same arithmetic.
//
// Replaces reference gapro/gaussian_process_utils.py:382-445 (fit_gp_spp) and the gpytorch objects it builds
// (:11-25): CholeskyVariationalDistribution + whitened VariationalStrategy with learned inducing locations,
// ConstantMean, ScaleKernel(RBFKernel), BernoulliLikelihood (20-point Gauss-Hermite), VariationalELBO,
// Adam(lr=0.1) x training_iter (:416-423), then prediction (:426-438).  There is no autograd on the device: the
// backward pass is the hand-derived one of SURVEY.md Appendix B.5, restated and checked against torch autograd in
// oracle/svgp_oracle.py.
//
// Arithmetic: float64 throughout (DESIGN.md "Precision").  Every M x M x M contraction is an MFMA product on
// v_mfma_f64_16x16x4_f64.  The default form is TN, C[i][j] = sum_k P[k][i] Q[k][j], both operands row-major in k so
// that fragment loads are 128-byte row segments; up to M_p = 256 (KMIN) the products that contract over the COLUMNS of
// A, B, G_A, Pm read those matrices as they are (two consecutive k per 16-byte load), so that no transposed copy is
// ever written.
//
// Per Adam step (round 3's step: 7.67 M^3 executed; G_L is never formed):
//   forward : K_ZZ tiles are evaluated on the fly inside the blocked left-looking Cholesky (16-wide block columns,
//             MFMA updates reading L^T, block column in LDS, 16 x 16 diagonal block factored AND inverted in registers by
//             one wave) -> L^T (the row-major factor L is not written: nothing reads it);  LI = L^-1 (one 16-wide block
//             column per wave, blocks kept in registers) -> LI, LI^T;  KX = k(Z, X);  A = LI KX;  B = LS^T A;
//             mu = A^T m + c;  var = s + eps + colsum(B^2) - colsum(A^2)  (column sums fused into the product epilogues)
//             g_mu, g_v from the 20-point Gauss-Hermite rule of log Phi(y f)
//   backward: G_m, G_c;  G_A = m g_mu^T + LS (2 B g_v) - 2 A diag(g_v);  G_LS = tril(A (2 B g_v)^T) + KL' with the Adam
//             update of LS fused into the epilogue;  G_KX^T = G_A^T LI (only the transposed G_KX is ever read);
//             Pm = Phi(L^T G_L) = Phi(-G_A A^T)   (tril(L^T tril(X)) = tril(L^T X) and L^T LI^T = I);
//             G_Kzz = LI^T (Pm LI): W = Pm LI is lower (M^3 / 3), S = LI^T W (2 M^3 / 3);  one fused pass turns G_Kzz and
//             G_KX into G_s, G_l, G_Z (kernel values recomputed from the LDS copies of Z and X) and applies Adam to Z
//   Adam    : torch.optim.Adam defaults (beta 0.9 / 0.999, eps 1e-8), lr 0.1 on {Z, m, tril(LS), c, rho_s, rho_l}
// Inducing points Z and training points X live transposed in LDS ([d][i]) so that a thread that owns column j reads
// its own point conflict-free and the row point as an LDS broadcast.
#pragma once
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "fit_layout.h"
#include "fit_math.h"
#include "epilogue.h"

namespace {
using namespace gapro_fit;
using namespace gapro_fit_math;

#ifndef GAPRO_NT
#define GAPRO_NT 512
#endif
constexpr int NT = GAPRO_NT;  // threads per fit (the small-fit translation unit builds this file with 256)
constexpr int NW = NT / 64;   // waves per fit
constexpr int kMaxMpLds = 512;          // largest padded M the LDS-staged kernel takes
constexpr int kMaxDynLds = 150 * 1024;  // dynamic LDS budget (160 KiB per CU minus the static part)
constexpr int kRedSlots = 8;            // values reduced across row groups per pass
// 64 x 64 wave tiles from this M_p on (one-per-CU build, D = 6; multiples of 32).  Round 3, 512 fits: M_p = 320 +2.4 %,
// 288 -2.2 % against 32 x 32 tiles; with the copy-free forms, one per CU, M_p = 192 / 224: -15 % (and one per CU with
// 32 x 32 tiles is 7 .. 10 % behind two per CU there).
constexpr int kTu4MinMp = 320;

using gapro_mfma::d4;


// ---- workspace layout (doubles); identical to svgp_fit_large.hip -----------------------------------
// (enums, Layout and make_layout: fit_layout.h, shared by every fit kernel)

// dynamic LDS of the staged kernel: Zt[D][Mp] | Pt[D][Mp] | scratch
constexpr int kTileDoubles = NW * 16 * 17;  // per-wave transpose tiles at the start of the scratch
constexpr int kFuseMaxMp = 128;            // up to this size column sums are fused into GEMM epilogues
// workgroup-tiled products (gemm_wg, beyond kFuseMaxMp): operand chunks in LDS
constexpr int kWgTile = 128;                  // output tile edge of the workgroup
constexpr int kWgKC = 8;                      // k rows per chunk
constexpr int kWgRow = kWgTile + 16;          // LDS row stride of a chunk (doubles): the two k rows a 32-lane group of a
                                              // fragment read touches start 128 bytes apart modulo the 256-byte bank row
constexpr int kWgStage = 2 * kWgKC * kWgRow;  // doubles per LDS stage: P chunk | Q chunk
constexpr int kWgRingDoubles = 2 * kWgStage;  // two stages
inline __host__ __device__ int part_doubles(int Mp) { return Mp <= kFuseMaxMp ? 3 * (Mp / 16) * Mp : 0; }
inline __host__ __device__ int scratch_doubles(int Mp) {
  const int a = kRedSlots * NT;                   // cross-group reductions / quadrature partials
  const int b = Mp * 17 + 64 * 17;                // Cholesky block column (row stride 17) + slack
  // transpose tiles + per-tile-row column sums (M_p <= kFuseMaxMp), or the products' operand ring (beyond it; the
  // transpose tiles then sit inside the ring's second stage, which is idle while a tile's epilogue runs)
  static_assert(kTileDoubles <= kWgStage, "the transpose tiles alias one stage of the operand ring");
  const int c = Mp <= kFuseMaxMp ? kTileDoubles + part_doubles(Mp) : kWgRingDoubles;
  int m = a > b ? a : b;
  return m > c ? m : c;
}
inline __host__ __device__ long long staged_lds_bytes(int m, int d) {
  const int Mp = gapro_pad_m(m, d);
  return 8LL * (2LL * d * Mp + scratch_doubles(Mp));
}
// (gapro_pad_m decides from gapro_staged_lds_bytes_mp, common.h: the two must agree beyond kFuseMaxMp)
inline __host__ __device__ bool staged_ok(int m, int d) {
  return gapro_pad_m(m, d) <= kMaxMpLds && d <= 32 && staged_lds_bytes(m, d) <= kMaxDynLds;
}


struct Fit {
  int M, T, D, Mp;
  int M1;  // train_y = -1 for the first M1 training points, +1 for the others (gaussian_process_utils.py:396-398)
  gd* mat[B_COUNT];
  gd* vec[V_COUNT];
  gd *X, *Z, *mZ, *vZ, *gZ, *Xt, *dinv, *dinvT, *scal;
};

#ifdef GAPRO_PROFILE
constexpr int kProfSlots = 28;
#endif
struct Shared {
  Fit f;
#ifdef GAPRO_PROFILE
  unsigned long long prof[kProfSlots];
  unsigned long long t_last;
  unsigned long long t_start;
#endif
  double red[NW];
  double dblk[16 * 17];
  double dinv[16 * 17];
  double c, rho_s, rho_l, s, ell, inv_l2;
  int status;
  int chol_bad;  // a pivot of the factorisation in progress was not positive (see factorize: the jitter retries)
};
__shared__ Shared g_sh;  // one fit per workgroup

#ifdef GAPRO_PROFILE
__device__ inline void prof_stamp(int id) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = wall_clock64();
    g_sh.prof[id] += t - g_sh.t_last;
    g_sh.t_last = t;
  }
}
#else
__device__ inline void prof_stamp(int) {}
#endif

// one symmetric pair of Gauss-Hermite nodes (t, weight w) of a point: sums for E (want_e only), dE/dmu, dE/dvar
__device__ inline void gh_pair(double y, double mu, double sd, double t, double w, bool want_e, double* E, double* dmu,
                               double* dvar) {
  if (want_e) {  // workgroup-uniform
    double lp, r;
    log_ndtr_ratio_erfcx(y * (mu - sd * t), &lp, &r);
    *E += w * lp; *dmu += w * r; *dvar -= w * t * r;
    log_ndtr_ratio_erfcx(y * (mu + sd * t), &lp, &r);
    *E += w * lp; *dmu += w * r; *dvar += w * t * r;
  } else {
    double r = ndtr_ratio(y * (mu - sd * t));
    *dmu += w * r; *dvar -= w * t * r;
    r = ndtr_ratio(y * (mu + sd * t));
    *dmu += w * r; *dvar += w * t * r;
  }
}

// Which fit of its kernel's list this workgroup runs.  Workgroup b of a launch runs on XCD b % 8 whatever that XCD is
// busy with, so with fit = blockIdx.x an XCD's share of a kernel's fits is fixed before the launch starts, and the XCDs
// ended a launch up to 55 ms apart (tools/fit_timeline.py) even with their shares balanced by cost.  With a ticket
// counter (one per kernel of a launch, zeroed by gapro_svgp_fit_batch) a workgroup takes the next fit of the
// longest-first list when it STARTS; the launcher over-subscribes the grid, the workgroups left without a fit exit at
// once, and an XCD that frees up earlier simply starts more of them.  A fit's result does not depend on who runs it.
__device__ inline int claim_fit(unsigned* ticket) {
  if (!ticket) return blockIdx.x;
  __shared__ int s_claim;
  if (threadIdx.x == 0) s_claim = (int)atomicAdd(ticket, 1u);
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(s_claim);
}

// Deterministic block sum, result broadcast to every thread: block_sum_shfl written out (one more inlining level changed
// the staged kernel's code)
__device__ inline double block_sum(double v) {
  v = wave_sum_shfl(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) g_sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < NW; ++w) t += g_sh.red[w];
  return t;
}

// squared distance between staged points: At[d][i] and Bt[d][j], leading dimension Mp
__device__ inline double sqdist_t(const ldsd* At, int i, const ldsd* Bt, int j, int D, int Mp) {
  double s = 0.0;
  for (int d = 0; d < D; ++d) {
    const double t = At[d * Mp + i] - Bt[d * Mp + j];
    s += t * t;
  }
  return s;
}

// stage n points [n][D] (global, row-major) transposed into LDS dst[D][Mp]; columns >= n are zeroed
__device__ inline void stage_points_t(ldsd* dst, const gd* src, int n, int D, int Mp) {
  for (int e = threadIdx.x; e < D * Mp; e += NT) {
    const int d = e / Mp, i = e - d * Mp;
    dst[e] = i < n ? src[(size_t)i * D + d] : 0.0;
  }
}

// ---- TN-form MFMA product ---------------------------------------------------------------------------
//   C[i][j] = sum_{k in [klo,khi)} P[k][i] * Q[k][j] (* qscale[k] if SCALE),  ld = leading dimension
// Each wave owns (16 TU) x (16 TU) output tiles, round-robin; `lower_only` enumerates tiles ti >= tj.
// kr(i0, j0, &klo, &khi) restricts the contraction (multiples of 16) to where triangular operands are
// non-zero.  epi(i0, j0, tile) consumes one 16x16 result tile in MFMA C layout.  Fragments of the next
// 8-deep block are loaded before the MFMAs of the current one are issued.
// MFMA f64 16x16x4 lane maps (cdna_hip_programming.md section 3): A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15], C/D register r -> row (l >> 4) + 4 r, col l & 15.
// ORD: the order in which the tiles are enumerated, heaviest contraction range first for the product's kr (a wave
// takes the tiles of that order in serpentine rounds: 0..7, 7..0, ...; with triangular operands a round-robin deal in
// row-major order leaves the slowest wave up to 1.8x the mean work, e.g. the same tile column for every tile of a wave
// when a row has 8 tiles).  Which wave computes a tile does not change the tile: results are bit-identical.
enum { ORD_ROWMAJOR = 0,   // equal ranges, or ranges shrinking with the tile row
       ORD_ROWS_DESC = 1,  // ranges growing with the tile row: last row first
       ORD_COLMAJOR = 2,   // ranges shrinking with the tile column
       ORD_SHELLS = 3 };   // ranges shrinking with max(row, column) (square tile grids): shells m = 0, 1, ...
// TRIM: the contraction index runs over inducing / training points; rows >= M of both operands are padding whose
// products with every valid output vanish, so the range stops at M rounded up to the register block (M = 230 padded to
// 256: 9 % fewer loads and MFMAs; valid outputs keep their bits, x + 0 * y = x).
// TU = 4 (the staged kernel's full-register build, M_p >= 352): 64 x 64 wave tiles, i.e. 8 instead of 16 operand columns
// fetched per 16 x 16 output block -- no fragment of these products is ever found in L2 (the hit rate does not move
// with the tile order; 256 concurrent fits stream ~100 MB per Adam step each at M = 384, together the ~6.3 TB/s the
// HBM delivers), so the bytes per block are what a product costs.  The extents are then given in 32 x 32 units and an
// odd count leaves a last row / column of 32 x 32 tiles, dealt after the full ones.
// PK / QK (round 3): the operand is stored with the contraction index along its ROWS' contiguous direction -- P[i][k]
// instead of P[k][i], Q[j][k] instead of Q[k][j] -- so that products of the forms X Y^T and X Y run on the matrices as
// they are and nobody has to write (and read back) a transposed copy: A^T, B^T, G_A^T, Pm^T each cost a full matrix
// of HBM writes per Adam step plus a pass through the waves' LDS transpose tiles.  A lane fetches two consecutive k of
// its row with one 16-byte load (64 contiguous bytes per row and instruction); with any operand in this form the k of
// MFMA step e = 0, 1 of a block of 8 is k0 + 2 (lane >> 4) + e for BOTH operands (a k-major operand then reads rows
// k0 + 2 lq and k0 + 2 lq + 1) -- a fixed permutation of the contraction order inside a block, so these products do not
// have the bits of the k-major form, but every product has ONE form in all kernels' variants that must agree.
typedef double d2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) d2 lds_d2;
typedef __attribute__((address_space(1))) d2 g_d2;

// Round 6 (profiles/r06_spill_traffic.md): every out-of-line product saved and restored the 41 callee-saved VGPRs it
// uses -- ~410 scratch stores and as many loads per wave and Adam step; the stores are 9 % of the bytes the two-per-CU
// staged fits write at M = 160 (the reloads are served by L2), and those fits sit on the memory roof.  Inlining the products into the KERNEL was 3 % slower (the
// register allocator then carries the kernel's long-lived values through every k loop); inlining them into ONE
// out-of-line function per Adam step (step_fn in fit_body, through gemm_tn_in) pays the callee-saved traffic once per
// step: M = 160 -3.3 %, 200 -1.7 %, 256 +0.7 %, 320 / 384 +-0 in time, bit-identical.  The strip kernels' tail products keep
// the out-of-line form (their caller holds 80 accumulator registers across them).
template <int TU, bool SCALE, int KS = 2, int ORD = ORD_ROWMAJOR, bool TRIM = false, int PK = 0, int QK = 0,
          typename KRange, typename Epi>
__device__ __forceinline__ void gemm_tn_body(int mo_tiles, int no_tiles, bool lower_only, const gd* __restrict__ P,
                                          const gd* __restrict__ Q, int ld, const gd* __restrict__ qscale, KRange kr,
                                          Epi epi) {
  mo_tiles = uni(mo_tiles);
  no_tiles = uni(no_tiles);
  lower_only = uni((int)lower_only) != 0;
  ld = uni(ld);
  P = uni_ptr(P);
  Q = uni_ptr(Q);
  qscale = uni_ptr(qscale);
  const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  // One output tile of TV x TV blocks at (i0, j0).  KSV = k-steps (of 4) per register block; two blocks alternate (one
  // in flight): 2 under the 128-VGPR budget of the LDS-staged kernel, 4 in the strip kernels' tail (256 VGPRs: +1.5 %;
  // in the staged kernel -3..-6 %), 1 with the 128 accumulator registers of a 64 x 64 tile.  Everything between the
  // issue of a block's loads and its MFMAs is straight-line code: s_waitcnt counts memory operations in issue order,
  // and behind a join of two paths ("prefetch only if there is a next block") the compiler falls back to waiting for
  // everything, i.e. for the block it has just requested -- no load would ever overlap an MFMA.  So the steady-state
  // loop has no guard in its body (the last one or two blocks are peeled off behind it), and the column scale of the
  // SCALE form is applied when a block is consumed, not when it is loaded (a multiply at load time is a wait at load
  // time).
  auto tile = [&](auto tv_tag, int i0, int j0) {
    constexpr int TV = decltype(tv_tag)::value;
    constexpr bool MINOR = PK || QK;
    constexpr int KSV = MINOR ? 2 : (TV >= 4 ? 1 : KS), KB = 4 * KSV;
    int klo, khi;
    kr(i0, j0, &klo, &khi);
    klo = uni(klo);
    khi = uni(khi);
    if (TRIM) {
      const int kmax = uni((g_sh.f.M + 7) / 8 * 8);  // a multiple of every KB in use but the strip tail's 16 (M_p there)
      khi = khi < kmax ? khi : kmax;
    }
    d4 acc[TV][TV];
#pragma unroll
    for (int u = 0; u < TV; ++u)
#pragma unroll
      for (int v = 0; v < TV; ++v) acc[u][v] = (d4){0.0, 0.0, 0.0, 0.0};
    const gd* pbase = PK ? P + (size_t)(i0 + lr) * ld + 2 * lq : P + (size_t)(MINOR ? 2 * lq : lq) * ld + i0 + lr;
    const gd* qbase = QK ? Q + (size_t)(j0 + lr) * ld + 2 * lq : Q + (size_t)(MINOR ? 2 * lq : lq) * ld + j0 + lr;
    double a0[KSV][TV], b0[KSV][TV], a1[KSV][TV], b1[KSV][TV];
    double s0[KSV], s1[KSV];
    auto load_block = [&](int k, double (&a)[KSV][TV], double (&b)[KSV][TV], double (&sc)[KSV]) {
      if constexpr (MINOR) {
#pragma unroll
        for (int u = 0; u < TV; ++u) {
          if constexpr (PK) {
            const d2 t = *(const g_d2*)(pbase + (size_t)(16 * u) * ld + k);
            a[0][u] = t[0];
            a[1][u] = t[1];
          } else {
            a[0][u] = pbase[(size_t)k * ld + 16 * u];
            a[1][u] = pbase[(size_t)(k + 1) * ld + 16 * u];
          }
        }
#pragma unroll
        for (int v = 0; v < TV; ++v) {
          if constexpr (QK) {
            const d2 t = *(const g_d2*)(qbase + (size_t)(16 * v) * ld + k);
            b[0][v] = t[0];
            b[1][v] = t[1];
          } else {
            b[0][v] = qbase[(size_t)k * ld + 16 * v];
            b[1][v] = qbase[(size_t)(k + 1) * ld + 16 * v];
          }
        }
        if (SCALE) {
          sc[0] = qscale[k + 2 * lq];
          sc[1] = qscale[k + 2 * lq + 1];
        }
      } else {
#pragma unroll
        for (int s = 0; s < KSV; ++s) {
          const gd* pr = pbase + (size_t)(k + 4 * s) * ld;
          const gd* qr = qbase + (size_t)(k + 4 * s) * ld;
#pragma unroll
          for (int u = 0; u < TV; ++u) a[s][u] = pr[16 * u];
#pragma unroll
          for (int v = 0; v < TV; ++v) b[s][v] = qr[16 * v];
          if (SCALE) sc[s] = qscale[k + 4 * s + lq];
        }
      }
    };
    auto mma_block = [&](double (&a)[KSV][TV], double (&b)[KSV][TV], double (&sc)[KSV]) {
#pragma unroll
      for (int s = 0; s < KSV; ++s) {
        double bs[TV];
#pragma unroll
        for (int v = 0; v < TV; ++v) bs[v] = SCALE ? b[s][v] * sc[s] : b[s][v];
#pragma unroll
        for (int u = 0; u < TV; ++u)
#pragma unroll
          for (int v = 0; v < TV; ++v)
            acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][u], bs[v], acc[u][v], 0, 0, 0);
      }
    };
    if (klo < khi) {  // khi - klo is a multiple of KB (tile-aligned ranges, trimmed to a multiple of 8)
      load_block(klo, a0, b0, s0);
      int k = klo;
#pragma nounroll
      for (; k + 2 * KB < khi; k += 2 * KB) {  // steady state: both prefetches are real, no guard in the body
        load_block(k + KB, a1, b1, s1);
        mma_block(a0, b0, s0);
        load_block(k + 2 * KB, a0, b0, s0);
        mma_block(a1, b1, s1);
      }
      if (k + KB < khi) {  // two blocks left
        load_block(k + KB, a1, b1, s1);
        mma_block(a0, b0, s0);
        mma_block(a1, b1, s1);
      } else {  // one block left
        mma_block(a0, b0, s0);
      }
    }
    run_epilogue<TV * TV>(epi, [&](int b, int* i, int* j) { *i = i0 + 16 * (b / TV); *j = j0 + 16 * (b % TV); },
                          [&](int b) -> const d4& { return acc[b / TV][b % TV]; });
  };
  // full tiles: fo x fn of TU x TU blocks.  TU >= 2 takes its extents in HALF tiles (TU = 2: 16 x 16, TU = 4: 32 x 32)
  // and an odd count leaves a last row / column of half-size tiles: M_p need not be a multiple of the tile (round 3:
  // M_p in steps of 16 up to 336, see gapro_pad_m)
  constexpr int TE = TU >= 2 ? TU / 2 : TU;  // blocks per side of an edge tile
  const int fo = TU >= 2 ? mo_tiles / 2 : mo_tiles, fn = TU >= 2 ? no_tiles / 2 : no_tiles;
  const int odd_i = TU >= 2 ? (mo_tiles & 1) : 0, odd_j = (TU >= 2 && !lower_only) ? (no_tiles & 1) : 0;
  const int nfull = lower_only ? fo * (fo + 1) / 2 : fo * fn;
  const int nrow = odd_i ? (lower_only ? mo_tiles : no_tiles) : 0;  // edge row: tiles (mo_tiles - 1, 0 ..) in half tiles
  const int ncol = odd_j ? mo_tiles - odd_i : 0;                    // edge column: tiles (0 .., no_tiles - 1) above it
  const int ntiles = nfull + nrow + ncol;
  const int rounds = (ntiles + NW - 1) / NW;
#pragma nounroll
  for (int q = 0; q < rounds; ++q) {
    const int t = q * NW + ((q & 1) ? NW - 1 - wave : wave);
    if (t >= ntiles) continue;
    if (t >= nfull) {  // half-size edge tiles, a quarter of a full tile's work each
      const int e = t - nfull;
      const int ih = e < nrow ? mo_tiles - 1 : e - nrow, jh = e < nrow ? e : no_tiles - 1;
      tile(std::integral_constant<int, TE>{}, 16 * TE * ih, 16 * TE * jh);
      continue;
    }
    int ti, tj;
    if (lower_only) {
      ti = 0;
      while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
      tj = t - ti * (ti + 1) / 2;
    } else if (ORD == ORD_ROWS_DESC) {
      ti = t / fn;
      tj = t - ti * fn;
      ti = fo - 1 - ti;
    } else if (ORD == ORD_COLMAJOR) {
      tj = t / fo;
      ti = t - tj * fo;
    } else if (ORD == ORD_SHELLS) {
      int m = 0;
      while ((m + 1) * (m + 1) <= t) ++m;
      const int r = t - m * m;
      ti = r <= m ? m : r - m - 1;
      tj = r <= m ? r : m;
    } else {
      ti = t / fn;
      tj = t - ti * fn;
    }
    tile(std::integral_constant<int, TU>{}, 16 * TU * ti, 16 * TU * tj);
  }
}

// the product as a function of its own (the strip kernels' tail products, the debug engines) ...
template <int TU, bool SCALE, int KS = 2, int ORD = ORD_ROWMAJOR, bool TRIM = false, int PK = 0, int QK = 0,
          typename KRange, typename Epi>
__device__ __noinline__ void gemm_tn(int mo_tiles, int no_tiles, bool lower_only, const gd* __restrict__ P,
                                     const gd* __restrict__ Q, int ld, const gd* __restrict__ qscale, KRange kr,
                                     Epi epi) {
  gemm_tn_body<TU, SCALE, KS, ORD, TRIM, PK, QK>(mo_tiles, no_tiles, lower_only, P, Q, ld, qscale, kr, epi);
}
// ... and inlined into its caller (the staged kernel's step function)
template <int TU, bool SCALE, int KS = 2, int ORD = ORD_ROWMAJOR, bool TRIM = false, int PK = 0, int QK = 0,
          typename KRange, typename Epi>
__device__ __forceinline__ void gemm_tn_in(int mo_tiles, int no_tiles, bool lower_only, const gd* __restrict__ P,
                                        const gd* __restrict__ Q, int ld, const gd* __restrict__ qscale, KRange kr,
                                        Epi epi) {
  gemm_tn_body<TU, SCALE, KS, ORD, TRIM, PK, QK>(mo_tiles, no_tiles, lower_only, P, Q, ld, qscale, kr, epi);
}

// ---- TN-form MFMA product, workgroup-tiled through an LDS ring (round 3) ---------------------------------
// The same contract as gemm_tn at TU = 1 -- extents in 16 x 16 blocks, kr(i0, j0) = the contraction range of the block
// at (i0, j0), epi(i0, j0, block) per block, every block accumulated over ascending k in steps of 4 -- and therefore
// the same bits.  What changes is where the operand fragments come from.  With one tile per wave fed from global
// memory every wave fetches its own fragments: 4 FLOP per byte at 32 x 32, and the 256 .. 512 concurrent fits of a
// launch, whose working sets (17 matrices each) hit neither L2 nor the Infinity Cache, move 6.3 TB/s at M = 256 -- the
// staged kernel sat ON the HBM roof (profiles/r03_probes.md).  Here the eight waves of the workgroup share one
// 128 x 128 output tile: an 8-row chunk of both operands (8 KiB each) is fetched ONCE per workgroup, one 16-byte load
// per thread and operand (wave w fetches row w: 1 KiB contiguous), held in registers for two iterations (the
// prefetch distance), written to one of two LDS stages and read from there as MFMA fragments by every wave: 16 FLOP
// per byte of global traffic.  One barrier per chunk.  Wave w owns the 32 x 64 piece at rows 32 r, columns 64 (w >> 2)
// of the tile, r = w & 3 for the first four waves and 3 - (w & 3) for the others: waves w and w + 4 share a SIMD, so
// with triangular operands every SIMD gets a long and a short contraction range.  A piece skips the chunks outside the
// hull of its blocks' ranges (the extra rows inside the hull multiply structural zeros of a triangular operand: x + 0 y
// = x, the bits stay).
// LDS image of a chunk: row k at k * kWgRow doubles with kWgRow = 128 + 16 (padded rows, no swizzle): the two k rows a
// 32-lane group of a fragment read touches start 128 bytes apart modulo the 256-byte bank row, i.e. they land in
// different halves of it (conflict-free ds_read_b64).
template <bool SCALE, bool TRIM, int PF, typename KRange, typename Epi>
__device__ __noinline__ void gemm_wg(int rows16, int cols16, bool lower_only, const gd* __restrict__ P,
                                     const gd* __restrict__ Q, int ld, const gd* __restrict__ qscale, KRange kr,
                                     Epi epi, ldsd* ring) {
  static_assert(NT == 512 || !sizeof(Epi), "gemm_wg: eight waves, one k row of a chunk per wave");
  static_assert(PF == 2 || PF == 4, "gemm_wg: register stages");
  rows16 = uni(rows16);
  cols16 = uni(cols16);
  lower_only = uni((int)lower_only) != 0;
  ld = uni(ld);
  P = uni_ptr(P);
  Q = uni_ptr(Q);
  qscale = uni_ptr(qscale);
  const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  const int rows = 16 * rows16, cols = 16 * cols16;
  const int nti = (rows + kWgTile - 1) / kWgTile, ntj = (cols + kWgTile - 1) / kWgTile;
  const int wi = wave < 4 ? wave : 7 - wave, wj = wave >> 2;
  const int kmax = TRIM ? uni((g_sh.f.M + 7) / 8 * 8) : ld;
  // loader: wave w moves k row w of a chunk, lane l the 16 bytes at columns 2 l, 2 l + 1 of the tile
  const int lcol = 2 * lane;
  const int lds_wr = wave * kWgRow + lcol;
  // fragment reads: element (k = 4 s + lq, column c + lr) of a chunk; block, k-step and stage are immediate offsets
  const int fa = lq * kWgRow + 32 * wi + lr;
  const int fb = kWgKC * kWgRow + lq * kWgRow + 64 * wj + lr;
#pragma nounroll
  for (int ti = 0; ti < nti; ++ti) {
#pragma nounroll
    for (int tj = 0; tj < (lower_only ? ti + 1 : ntj); ++tj) {
      const int I0 = kWgTile * ti, J0 = kWgTile * tj;
      // Contraction range of the workgroup tile and of this wave's piece: the hull of their blocks' ranges.  Every kr
      // of the fit is monotone (lo and hi never decrease with the block row or the block column), so a rectangle's
      // hull is [lo of its first block, hi of its last block]: two calls instead of one per block (64 per tile and
      // wave cost ~3 us of scalar work per tile, a quarter of a tile's time at M_p = 256).  For a lower-triangular
      // output the blocks above the diagonal are not part of it; leaving them in the hull only widens it, and what a
      // wider hull adds are products with structural zeros.
      int klo = 1 << 30, khi = 0, plo = 1 << 30, phi = 0;
      unsigned on_mask = 0;  // bit 4 u + v: block (u, v) of this wave's piece is part of the output
      if (rows - I0 >= kWgTile && cols - J0 >= kWgTile) {  // a full tile: every piece, every block inside the matrix
        int lo, hi, d;
        kr(I0, J0, &lo, &d);
        kr(I0 + kWgTile - 16, J0 + kWgTile - 16, &d, &hi);
        hi = hi < kmax ? hi : kmax;
        if (lo < hi) { klo = lo; khi = hi; }
        const int pi0 = I0 + 32 * wi, pj0 = J0 + 64 * wj;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (!(lower_only && pi0 + 16 * u < pj0 + 16 * v)) on_mask |= 1u << (4 * u + v);
        if (on_mask) {
          kr(pi0, pj0, &lo, &d);
          kr(pi0 + 16, pj0 + 48, &d, &hi);
          hi = hi < kmax ? hi : kmax;
          if (lo < hi) { plo = lo; phi = hi; }
        }
      } else {  // a tile at the matrix edge: block by block
#pragma nounroll
        for (int bi = 0; bi < kWgTile / 16; ++bi) {
          const int ib = I0 + 16 * bi;
          if (ib >= rows) break;
#pragma nounroll
          for (int bj = 0; bj < kWgTile / 16; ++bj) {
            const int jb = J0 + 16 * bj;
            if (jb >= cols) break;
            if (lower_only && ib < jb) continue;
            const bool mine = (bi >> 1) == wi && (bj >> 2) == wj;
            if (mine) on_mask |= 1u << (4 * (bi & 1) + (bj & 3));  // also with an empty range: epi sees a zero block
            int lo, hi;
            kr(ib, jb, &lo, &hi);
            hi = hi < kmax ? hi : kmax;
            if (lo >= hi) continue;
            klo = lo < klo ? lo : klo;
            khi = hi > khi ? hi : khi;
            if (mine) {
              plo = lo < plo ? lo : plo;
              phi = hi > phi ? hi : phi;
            }
          }
        }
      }
      klo = uni(klo) & ~(kWgKC - 1);
      khi = uni(khi);
      plo = uni(plo) & ~(kWgKC - 1);
      phi = uni(phi);
      on_mask = (unsigned)uni((int)on_mask);
      const int nch = klo < khi ? (khi - klo + kWgKC - 1) / kWgKC : 0;  // workgroup-uniform
      d4 acc[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = (d4){0.0, 0.0, 0.0, 0.0};
      if (nch > 0) {
        const bool pin = I0 + lcol < ld, qin = J0 + lcol < ld;  // columns beyond the matrix: blocks that are dropped
        const gd* pg = P + (size_t)wave * ld + (pin ? I0 + lcol : 0);
        const gd* qg = Q + (size_t)wave * ld + (qin ? J0 + lcol : 0);
        // Register stages: chunk n of the tile waits in stage n % PF from its request until it goes to LDS, PF - 1 .. PF
        // iterations later (the chunk index is clamped to the last one, so that every load is unconditional and the
        // waits stay counted).  An iteration cannot be shorter than the memory latency / PF: with one workgroup per CU
        // and two stages the loop ran at the HBM latency, not at the matrix rate.  With SCALE the row's scale rides
        // along (one address per wave) and is applied when the row goes to LDS: b * scale, the same product the
        // per-wave form computes on every fragment.
        d2 rp[PF], rq[PF];
        double rs[PF];
        auto gload = [&](int n, d2& p, d2& q, double& sc) {
          n = n < nch ? n : nch - 1;
          const size_t o = (size_t)(klo + kWgKC * n) * ld;
          p = *(const g_d2*)(pg + o);
          q = *(const g_d2*)(qg + o);
          if (SCALE) sc = qscale[klo + kWgKC * n + wave];
        };
        auto lstore = [&](int stage, const d2& p, const d2& q, double sc) {
          ldsd* base = ring + stage * kWgStage + lds_wr;
          *(lds_d2*)base = p;
          *(lds_d2*)(base + kWgKC * kWgRow) = SCALE ? (d2){q[0] * sc, q[1] * sc} : q;
        };
        // Fragments of one k-step: 2 of A, 4 of B.  Two sets alternate, software-pipelined across the barrier: the
        // second step's set is requested before the first step's MFMAs, the NEXT chunk's first step right behind the
        // barrier, under the second step's MFMAs -- the matrix pipe never waits for an LDS round trip, and a barrier
        // costs what the waves' skew costs (tools/wgloop_peak.py: 47 -> 64 TFLOP/s for this loop with every CU running
        // it).  Every block of a piece that has work is computed, also the ones whose result is dropped (columns
        // beyond the matrix, blocks above the diagonal of a lower-triangular output): a guard per block costs two
        // taken branches per MFMA, and a block's result depends on its own accumulator only.
        double fa0[2], fb0[4], fa1[2], fb1[4];
        auto rd = [&](int stage, int s, double (&a)[2], double (&b)[4]) {
          const ldsd* st = ring + stage * kWgStage + 4 * s * kWgRow;
#pragma unroll
          for (int v = 0; v < 4; ++v) b[v] = st[fb + 16 * v];
#pragma unroll
          for (int u = 0; u < 2; ++u) a[u] = st[fa + 16 * u];
        };
        auto mm = [&](int k0, const double (&a)[2], const double (&b)[4]) {
          if (k0 < plo || k0 >= phi) return;  // wave-uniform: the piece's own contraction range
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
              acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
        };
        // chunk c: CUR = its LDS stage, SLOT = the register stage holding chunk c + 1, refilled with chunk c + 1 + PF
        auto chunk = [&](auto cur_tag, auto slot_tag, int c) {
          constexpr int CUR = decltype(cur_tag)::value, SLOT = decltype(slot_tag)::value;
          const int k0 = klo + kWgKC * c;
          lstore(CUR ^ 1, rp[SLOT], rq[SLOT], rs[SLOT]);
          gload(c + 1 + PF, rp[SLOT], rq[SLOT], rs[SLOT]);
          rd(CUR, 1, fa1, fb1);
          __builtin_amdgcn_sched_barrier(0);
          mm(k0, fa0, fb0);
          __builtin_amdgcn_sched_barrier(0);
          __syncthreads();
          rd(CUR ^ 1, 0, fa0, fb0);
          __builtin_amdgcn_sched_barrier(0);
          mm(k0, fa1, fb1);
          __builtin_amdgcn_sched_barrier(0);
        };
        using I0t = std::integral_constant<int, 0>;
        using I1t = std::integral_constant<int, 1>;
        using I2t = std::integral_constant<int, 2>;
        using I3t = std::integral_constant<int, 3>;
        // prologue: chunks 0 .. PF - 1 requested, chunk 0 on to LDS, chunk PF requested, first fragments read
#pragma unroll
        for (int n = 0; n < PF; ++n) gload(n, rp[n], rq[n], rs[n]);
        lstore(0, rp[0], rq[0], rs[0]);
        gload(PF, rp[0], rq[0], rs[0]);
        __syncthreads();
        rd(0, 0, fa0, fb0);
        int c = 0;
        if constexpr (PF == 2) {
#pragma nounroll
          for (; c + 1 < nch; c += 2) {  // the LDS stages and the register stages alternate by name
            chunk(I0t{}, I1t{}, c);
            chunk(I1t{}, I0t{}, c + 1);
          }
          if (c < nch) chunk(I0t{}, I1t{}, c);
        } else {
#pragma nounroll
          for (; c + 3 < nch; c += 4) {
            chunk(I0t{}, I1t{}, c);
            chunk(I1t{}, I2t{}, c + 1);
            chunk(I0t{}, I3t{}, c + 2);
            chunk(I1t{}, I0t{}, c + 3);
          }
          if (c < nch) chunk(I0t{}, I1t{}, c);
          if (c + 1 < nch) chunk(I1t{}, I2t{}, c + 1);
          if (c + 2 < nch) chunk(I0t{}, I3t{}, c + 2);
        }
      }
      // (no barrier here: what slower waves may still do with the ring is the read-ahead of a chunk that does not
      // exist, and the next tile's prologue has a barrier between its first LDS store and everything else)
      run_epilogue<8>(epi,
                      [&](int b, int* i, int* j) {
                        const bool on = (on_mask >> b) & 1u;
                        *i = on ? I0 + 32 * wi + 16 * (b >> 2) : -1;
                        *j = J0 + 64 * wj + 16 * (b & 3);
                      },
                      [&](int b) -> const d4& { return acc[b >> 2][b & 3]; });
    }
  }
}

// Store a 16x16 accumulator tile (C layout) row-major at Cm[i0.., j0..] and/or transposed at CT[j0.., i0..].
// The transposed copy goes through a per-wave LDS tile so that its global stores are 128-byte rows too.
__device__ inline void store_tile(const d4& v, gd* __restrict__ Cm, gd* __restrict__ CT, int ld, int i0, int j0,
                                  ldsd* tile /* per-wave 16x17 */) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  if (Cm) {
#pragma unroll
    for (int r = 0; r < 4; ++r) Cm[(size_t)(i0 + lq + 4 * r) * ld + j0 + lr] = v[r];
  }
  if (CT) {
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[(lq + 4 * r) * 17 + lr] = v[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) CT[(size_t)(j0 + lq + 4 * r) * ld + i0 + lr] = tile[lr * 17 + lq + 4 * r];
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
  }
}

// Factor the 16x16 diagonal block S (LDS panel rows 0..15, row stride 17) = L_kk L_kk^T and invert L_kk.
// One wave: lane r (mod 16) holds row r in registers; column pivots and multipliers travel by
// v_readlane broadcasts, so the 16 dependent elimination steps never wait on LDS.  The inverse is a
// forward substitution, one column per lane, reading L_kk as LDS broadcasts.  Results: L_kk and
// Dinv = L_kk^-1 in g_sh.dblk / g_sh.dinv, and in global memory (L^T diagonal block, Dinv, Dinv^T).  (Round 3: L itself
// is no longer written by these kernels -- since Pm = Phi(-G_A A^T) nothing reads it; everything works from L^T.)
__device__ __noinline__ void diag_factor_invert(ldsd* panel, int kb) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp;
  kb = uni(kb);
  gd* LT = f.mat[B_LT];
  const int lane = threadIdx.x & 63, r = lane & 15;
#ifdef GAPRO_PROFILE
  const unsigned long long tp0 = wall_clock64();
#endif
  double rdiag[16];  // 1 / L[j][j] (wave-uniform)
  {
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = panel[r * 17 + c];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      double d = lane_bcast(a[j], j);
      if (!(d > 0.0)) {  // not positive definite (or NaN): flag it, keep going with a tiny pivot
        bad = true;
        d = 1e-30;
      }
      const double rs = rsqrt(d);
      rdiag[j] = rs;
      const double lj = (r == j) ? d * rs : a[j] * rs;  // column j of L: rows >= j are meaningful
      a[j] = lj;
#pragma unroll
      for (int c = j + 1; c < 16; ++c) a[c] -= lj * lane_bcast(lj, c);  // only rows r >= c are used later
    }
    if (bad && lane == 0) g_sh.chol_bad = 1;
    if (lane < 16) {
#pragma unroll
      for (int c = 0; c < 16; ++c) g_sh.dblk[r * 17 + c] = (c <= r) ? a[c] : 0.0;  // L_kk
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
#ifdef GAPRO_PROFILE
  const unsigned long long tp1 = wall_clock64();
#endif
  {
    // column r of Dinv by forward substitution, right-looking: x[q] = b[q] / L[q][q], then every later row takes
    // its term, b[rr] -= L[rr][q] x[q] (15 - q independent updates, L_kk read as LDS broadcasts).  The phase is
    // bound by VALU issue (every lane of the wave executes every instruction), so the terms are bare FMAs: x[q] = 0
    // for q < r makes the terms of the rows above the column vanish without a select per term (1.83 -> 0.99 us per
    // block).  Feeding these FMAs from the factor loop's own broadcasts (one fused pass, no LDS reads) was slower:
    // 4.05 us per block against 3.4 for the two loops.
    double x[16], b[16];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) b[rr] = (rr == r) ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      x[q] = (q >= r) ? b[q] * rdiag[q] : 0.0;
#pragma unroll
      for (int rr = q + 1; rr < 16; ++rr) b[rr] = fma(-g_sh.dblk[rr * 17 + q], x[q], b[rr]);
    }
    if (lane < 16) {
#pragma unroll
      for (int c = 0; c < 16; ++c) g_sh.dinv[c * 17 + r] = x[c];  // Dinv[c][r]: lane r holds column r
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
#ifdef GAPRO_PROFILE
  const unsigned long long tp2 = wall_clock64();
#endif
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = lane + 64 * e;
    const int rr = idx >> 4, cc = idx & 15;
    LT[(size_t)(16 * kb + rr) * Mp + 16 * kb + cc] = g_sh.dblk[cc * 17 + rr];
    f.dinv[(size_t)kb * 256 + idx] = g_sh.dinv[rr * 17 + cc];
    f.dinvT[(size_t)kb * 256 + idx] = g_sh.dinv[cc * 17 + rr];
  }
#ifdef GAPRO_PROFILE
  if (lane == 0) {  // wave-0-only sub-phases of the diagonal block (they overlap slot 5, not part of the total)
    const unsigned long long tp3 = wall_clock64();
    g_sh.prof[22] += tp1 - tp0;  // factor
    g_sh.prof[23] += tp2 - tp1;  // inverse
    g_sh.prof[24] += tp3 - tp2;  // stores issued
  }
#endif
}

// acc -= sum_{q < Q} L[i][q] L[j][q] for one 16x16 tile of the Cholesky update (operands from L^T, TN form), Q a
// multiple of 16.  Blocks of four k-steps (eight loads) alternate between two register sets with no guard in the
// steady-state body, so that the loads of a block are in flight during the MFMAs of the previous one (see gemm_tn).
__device__ inline void chol_update_tile(d4& acc, const gd* pa, const gd* pb, int Mp, int Q) {
  const size_t st = (size_t)4 * Mp;
  auto ld = [&](int q, double (&a)[4], double (&b)[4]) {
    const size_t o = (size_t)q * Mp;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = pa[o + e * st];
      b[e] = pb[o + e * st];
    }
  };
  auto mm = [&](double (&a)[4], double (&b)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[e], b[e], acc, 0, 0, 0);
  };
  if (Q <= 0) return;
  double a0[4], b0[4], a1[4], b1[4];
  ld(0, a0, b0);
  int q = 0;
#pragma nounroll
  for (; q + 32 < Q; q += 32) {
    ld(q + 16, a1, b1);
    mm(a0, b0);
    ld(q + 32, a0, b0);
    mm(a1, b1);
  }
  if (q + 16 < Q) {
    ld(q + 16, a1, b1);
    mm(a0, b0);
    mm(a1, b1);
  } else {
    mm(a0, b0);
  }
}

// ---- Cholesky of Kzz + jitter I, fused with the kernel evaluation -----------------------------------
// Left-looking, 16-wide block columns.  Block column kb:
//   (1) S = Kzz[:, kb] - L[:, <kb] L[kb, <kb]^T : the Kzz tile is evaluated from the staged inducing
//       points straight into the MFMA accumulator, the update reads L^T (TN form); S goes to an LDS panel
//   (2) wave 0 factors the 16x16 diagonal block held one row per lane in registers (cross-lane
//       broadcasts, no LDS round trips) and inverts it (column per lane)
//   (3) panel below = S * Dinv^T, computed in LDS, then written once to L^T (rows)
// The padded tail (index >= M) is an identity block.  Strict upper triangle of L stays zero.
template <int DC>
__device__ __noinline__ void cholesky_fused(const ldsd* Zt, ldsd* panel, double s, double inv_l2, double jitter) {
  const Fit& f = g_sh.f;
  Shared& sh = g_sh;
  const int Mp = f.Mp, M = f.M, D = DC ? DC : f.D, nb = Mp / 16;
  gd* LT = f.mat[B_LT];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  for (int kb = 0; kb < nb; ++kb) {
    // (1)
    for (int ib = kb + wave; ib < nb; ib += NW) {
      d4 acc;
      const int col = 16 * kb + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ib + lq + 4 * r;
        double v = 0.0;
        if (row < M && col < M) {
          v = s * gapro_fit_math::rbf_exp(-0.5 * inv_l2 * sqdist_t(Zt, row, Zt, col, D, Mp));
          if (row == col) v += jitter;
        } else if (row == col) {
          v = 1.0;
        }
        acc[r] = v;
      }
      const gd* pa = LT + (size_t)lq * Mp + 16 * ib + lr;
      const gd* pb = LT + (size_t)lq * Mp + 16 * kb + lr;
      chol_update_tile(acc, pa, pb, Mp, 16 * kb);
      ldsd* dst = panel + (16 * (ib - kb)) * 17;
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(lq + 4 * r) * 17 + lr] = acc[r];
    }
    __syncthreads();
    prof_stamp(0);
    // (2)
    if (wave == 0) diag_factor_invert(panel, kb);
    __syncthreads();
    prof_stamp(5);
    // (3) rows below the diagonal block, in LDS: P[i][c] <- sum_{q <= c} S[i][q] Dinv[c][q]
    const int rows_below = Mp - 16 * (kb + 1);
    ldsd* pb = panel + 16 * 17;
    for (int idx = threadIdx.x; idx < rows_below * 16; idx += NT) {
      const int i = idx >> 4, c = idx & 15;
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc += (q <= c) ? pb[i * 17 + q] * sh.dinv[c * 17 + q] : 0.0;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();  // the 16 lanes of a row have all read S before any overwrites it
      pb[i * 17 + c] = acc;
    }
    __syncthreads();
    if (rows_below > 0)
      for (int idx = threadIdx.x; idx < rows_below * 16; idx += NT) {  // L^T rows: contiguous in i
        const int c = idx / rows_below, i = idx - c * rows_below;
        LT[(size_t)(16 * kb + c) * Mp + 16 * (kb + 1) + i] = pb[i * 17 + c];
      }
    __syncthreads();
    prof_stamp(18);
  }
}

// ---- the same factorisation with a one-column look-ahead (strip kernels) ------------------------------
// In cholesky_fused the other waves idle while wave 0 factors the diagonal block (~4.5 us per block column, more
// than the whole MFMA update of a column).  Here two LDS panels alternate: while wave 0 factors the diagonal block
// of column kb, the other waves already build column kb + 1 -- kernel tile minus the contributions of the columns
// < kb, which are final in L^T -- and once column kb's panel has been scaled, its rank-16 contribution is
// subtracted straight from LDS (both operands are rows of the scaled panel) while the panel is written to L / L^T.
// Every accumulator sees the same MFMAs in the same order as in cholesky_fused (the detour of the partial sums
// through LDS is exact), so the factor is bit-identical.
inline __host__ __device__ int chol_panel_doubles(int Mp) { return Mp * 17 + 64 * 17; }
template <int DC>
__device__ __noinline__ void cholesky_fused_lookahead(const ldsd* Zt, ldsd* panels, double s, double inv_l2,
                                                      double jitter) {
  const Fit& f = g_sh.f;
  Shared& sh = g_sh;
  const int Mp = f.Mp, M = f.M, D = DC ? DC : f.D, nb = Mp / 16;
  gd* LT = f.mat[B_LT];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  const int PS = chol_panel_doubles(Mp);
  // block (ib, kb) of Kzz + jitter I minus the contributions of the block columns < qb, into panel dst
  auto build = [&](int ib, int kb, int qb, ldsd* dst_panel) {
    d4 acc;
    const int col = 16 * kb + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ib + lq + 4 * r;
      double v = 0.0;
      if (row < M && col < M) {
        v = s * gapro_fit_math::rbf_exp(-0.5 * inv_l2 * sqdist_t(Zt, row, Zt, col, D, Mp));
        if (row == col) v += jitter;
      } else if (row == col) {
        v = 1.0;
      }
      acc[r] = v;
    }
    const gd* pa = LT + (size_t)lq * Mp + 16 * ib + lr;
    const gd* pb = LT + (size_t)lq * Mp + 16 * kb + lr;
    chol_update_tile(acc, pa, pb, Mp, 16 * qb);
    ldsd* dst = dst_panel + (16 * (ib - kb)) * 17;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(lq + 4 * r) * 17 + lr] = acc[r];
  };
  for (int ib = wave; ib < nb; ib += NW) build(ib, 0, 0, panels);
  __syncthreads();
  for (int kb = 0; kb < nb; ++kb) {
    ldsd* cur = panels + (kb & 1) * PS;
    ldsd* nxt = panels + ((kb + 1) & 1) * PS;
    // (2) diagonal block on wave 0 | column kb + 1 without the contribution of column kb on the other waves
    if (wave == 0) {
      // the serial chain everybody waits for.  In the 256-thread build a SIMD hosts one wave of each of the CU's two
      // fits: the chain goes ahead of the other fit's wave (+2..3 % at M <= 64; with 512 threads it is -0.6 %)
      if (NW <= 4) __builtin_amdgcn_s_setprio(3);
      diag_factor_invert(cur, kb);
      if (NW <= 4) __builtin_amdgcn_s_setprio(0);
    } else {
      for (int ib = kb + wave; ib < nb; ib += NW - 1) build(ib, kb + 1, kb, nxt);
    }
    __syncthreads();
    prof_stamp(5);
    // (3) rows below the diagonal block, in LDS: P[i][c] <- sum_{q <= c} S[i][q] Dinv[c][q]
    const int rows_below = Mp - 16 * (kb + 1);
    ldsd* pb = cur + 16 * 17;
    for (int idx = threadIdx.x; idx < rows_below * 16; idx += NT) {
      const int i = idx >> 4, c = idx & 15;
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc += (q <= c) ? pb[i * 17 + q] * sh.dinv[c * 17 + q] : 0.0;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();  // the 16 lanes of a row have all read S before any overwrites it
      pb[i * 17 + c] = acc;
    }
    __syncthreads();
    // column kb's contribution to column kb + 1, both operands from the scaled panel (block row kb + 1 is its top)
    for (int ib = kb + 1 + wave; ib < nb; ib += NW) {
      ldsd* dst = nxt + (16 * (ib - kb - 1)) * 17;
      const ldsd* la = pb + (16 * (ib - kb - 1) + lr) * 17 + lq;
      const ldsd* lb = pb + lr * 17 + lq;
      d4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = dst[(lq + 4 * r) * 17 + lr];
#pragma unroll
      for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-la[4 * st], lb[4 * st], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(lq + 4 * r) * 17 + lr] = acc[r];
    }
    if (rows_below > 0)
      for (int idx = threadIdx.x; idx < rows_below * 16; idx += NT) {  // L^T rows: contiguous in i
        const int c = idx / rows_below, i = idx - c * rows_below;
        LT[(size_t)(16 * kb + c) * Mp + 16 * (kb + 1) + i] = pb[i * 17 + c];
      }
    __syncthreads();
    prof_stamp(18);
  }
}

// ---- the look-ahead with the next column's partial sums in REGISTERS (staged kernel, round 4) --------------------
// The LDS look-ahead above needs two panels (87 KB at M_p = 256), which the staged kernel does not have beside Z, X
// and its two-workgroups-per-CU budget of 72 KB.  Here the tiles of column kb + 1 that a wave builds while wave 0
// factors the diagonal block of column kb stay in that wave's registers (at most TMAX accumulators of 8 VGPRs: block
// rows kb + w, kb + w + 7, ... for wave w >= 1), take column kb's rank-16 contribution from the scaled panel, and are
// written to the ONE panel once every reader of column kb is done with it.  Same MFMAs in the same order per
// accumulator: bit-identical to cholesky_fused.  Four barriers per block column, as there.
template <int DC, int TMAX>
__device__ __noinline__ void cholesky_fused_lookahead_reg(const ldsd* Zt, ldsd* panel, double s, double inv_l2,
                                                          double jitter) {
  const Fit& f = g_sh.f;
  Shared& sh = g_sh;
  const int Mp = f.Mp, M = f.M, D = DC ? DC : f.D, nb = Mp / 16;
  gd* LT = f.mat[B_LT];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  // block (ib, kb) of Kzz + jitter I minus the contributions of the block columns < qb
  auto build = [&](int ib, int kb, int qb) -> d4 {
    d4 acc;
    const int col = 16 * kb + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ib + lq + 4 * r;
      double v = 0.0;
      if (row < M && col < M) {
        v = s * gapro_fit_math::rbf_exp(-0.5 * inv_l2 * sqdist_t(Zt, row, Zt, col, D, Mp));
        if (row == col) v += jitter;
      } else if (row == col) {
        v = 1.0;
      }
      acc[r] = v;
    }
    const gd* pa = LT + (size_t)lq * Mp + 16 * ib + lr;
    const gd* pb = LT + (size_t)lq * Mp + 16 * kb + lr;
    chol_update_tile(acc, pa, pb, Mp, 16 * qb);
    return acc;
  };
  for (int ib = wave; ib < nb; ib += NW) {
    const d4 acc = build(ib, 0, 0);
    ldsd* dst = panel + (16 * ib) * 17;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(lq + 4 * r) * 17 + lr] = acc[r];
  }
  __syncthreads();
  d4 nx[TMAX];
  for (int kb = 0; kb < nb; ++kb) {
    // (2) diagonal block on wave 0 | column kb + 1 without the contribution of column kb on the other waves
    if (wave == 0) {
      diag_factor_invert(panel, kb);
    } else {
#pragma unroll
      for (int t = 0; t < TMAX; ++t) {
        const int ib = kb + wave + t * (NW - 1);
        if (ib < nb) nx[t] = build(ib, kb + 1, kb);
      }
    }
    __syncthreads();
    prof_stamp(5);
    // (3) rows below the diagonal block, in LDS: P[i][c] <- sum_{q <= c} S[i][q] Dinv[c][q]
    const int rows_below = Mp - 16 * (kb + 1);
    ldsd* pb = panel + 16 * 17;
    for (int idx = threadIdx.x; idx < rows_below * 16; idx += NT) {
      const int i = idx >> 4, c = idx & 15;
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc += (q <= c) ? pb[i * 17 + q] * sh.dinv[c * 17 + q] : 0.0;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();  // the 16 lanes of a row have all read S before any overwrites it
      pb[i * 17 + c] = acc;
    }
    __syncthreads();
    // column kb's contribution to this wave's tiles of column kb + 1, both operands from the scaled panel
    if (wave != 0) {
#pragma unroll
      for (int t = 0; t < TMAX; ++t) {
        const int ib = kb + wave + t * (NW - 1);
        if (ib < nb) {
          const ldsd* la = pb + (16 * (ib - kb - 1) + lr) * 17 + lq;
          const ldsd* lb = pb + lr * 17 + lq;
#pragma unroll
          for (int st = 0; st < 4; ++st)
            nx[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-la[4 * st], lb[4 * st], nx[t], 0, 0, 0);
        }
      }
    }
    if (rows_below > 0)
      for (int idx = threadIdx.x; idx < rows_below * 16; idx += NT) {  // L^T rows: contiguous in i
        const int c = idx / rows_below, i = idx - c * rows_below;
        LT[(size_t)(16 * kb + c) * Mp + 16 * (kb + 1) + i] = pb[i * 17 + c];
      }
    __syncthreads();  // every reader of the scaled column kb is done: the panel takes column kb + 1
    if (wave != 0) {
#pragma unroll
      for (int t = 0; t < TMAX; ++t) {
        const int ib = kb + wave + t * (NW - 1);
        if (ib < nb) {
          ldsd* dst = panel + (16 * (ib - kb - 1)) * 17;
#pragma unroll
          for (int r = 0; r < 4; ++r) dst[(lq + 4 * r) * 17 + lr] = nx[t][r];
        }
      }
    }
    __syncthreads();
    prof_stamp(18);
  }
}

// ---- gpytorch's psd_safe_cholesky around either factorisation -----------------------------------------------
// VariationalStrategy._cholesky_factor calls psd_safe_cholesky(K_ZZ.double() + jitter I): when the factorisation meets
// a non-positive pivot it is repeated on K + j I with j = psd_jitter * 10^i (settings.cholesky_jitter: 1e-8 for
// float64), i = 0 .. psd_retries - 1 (settings.cholesky_max_tries = 3), and only then gives up (NotPSDError -> here
// GAPRO_ERR_CHOLESKY for this fit; the other fits of the launch are unaffected).  The extra jitter lives inside the
// factorisation only: it is not added to the k_xx term of the predictive variance, as in gpytorch.  A function of its
// own so that the retry state is not live across the step loop of the callers.
// LOOKAHEAD: 0 = cholesky_fused, 1 = two LDS panels (strip kernels), 2 / 3 = the next column in registers, at most 3 / 5
// tiles per wave (staged kernel: M_p <= 256 / <= 512)
template <int DC, int LOOKAHEAD>
__device__ __noinline__ void cholesky_psd_safe(const ldsd* Zt, ldsd* scratch, double s, double inv_l2, double jitter,
                                               int retries, double psd_jitter) {
  double extra = 0.0;
  for (int attempt = 0;; ++attempt) {
    if (LOOKAHEAD == 1) cholesky_fused_lookahead<DC>(Zt, scratch, s, inv_l2, jitter + extra);
    else if (LOOKAHEAD == 2) cholesky_fused_lookahead_reg<DC, 3>(Zt, scratch, s, inv_l2, jitter + extra);
    else if (LOOKAHEAD == 3) cholesky_fused_lookahead_reg<DC, 5>(Zt, scratch, s, inv_l2, jitter + extra);
    else cholesky_fused<DC>(Zt, scratch, s, inv_l2, jitter + extra);
    const int bad = g_sh.chol_bad;  // both factorisations end with a workgroup barrier
    if (!bad) return;               // the common case: one LDS read, no extra barrier
    __syncthreads();
    if (threadIdx.x == 0) {
      g_sh.chol_bad = 0;
      if (attempt >= retries) g_sh.status = GAPRO_ERR_CHOLESKY;
    }
    __syncthreads();
    if (attempt >= retries) return;
    extra = psd_jitter * pow(10.0, (double)attempt);
  }
}

// ---- the strip kernels' triangular inverse: one block column per wave as a straight-line chain ---------------
// Same products in the same order as tri_inverse<8> (bit-identical), but instantiated per column length so that
// there is no guard inside the chain: the L operands of block row ii + 1 (and its Dinv^T) are requested before the
// MFMAs of row ii and are in flight while row ii is computed and stored.  In the guarded form every block waits
// for its own loads and, s_waitcnt being what it is behind a join, for the stores of the block before.
template <int CNT>
__device__ inline void inv_column(int k, ldsd* tile) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp;
  const gd* LT = f.mat[B_LT];
  gd* LI = f.mat[B_LI];
  gd* U = f.mat[B_U];
  const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  constexpr int MAXR = CNT > 1 ? CNT - 1 : 1;
  d4 blk[CNT];
  double A0[MAXR * 4], A1[MAXR * 4], D0[4], D1[4];
  // operands of block row ii: L[16(k+ii)+lr][16(k+jj)+4s+lq] for jj < ii, and -Dinv_{k+ii}^T
  auto ldrow = [&](int ii, double (&A)[MAXR * 4], double (&D)[4]) {
    const int i = k + ii;
#pragma unroll
    for (int jj = 0; jj < MAXR; ++jj)
      if (jj < ii) {
        const gd* pa = LT + (size_t)(16 * (k + jj) + lq) * Mp + 16 * i + lr;
#pragma unroll
        for (int st = 0; st < 4; ++st) A[jj * 4 + st] = pa[(size_t)(4 * st) * Mp];
      }
#pragma unroll
    for (int st = 0; st < 4; ++st) D[st] = f.dinvT[(size_t)i * 256 + (4 * st + lq) * 16 + lr];
  };
  d4 dk;
#pragma unroll
  for (int r = 0; r < 4; ++r) dk[r] = f.dinv[(size_t)k * 256 + (lq + 4 * r) * 16 + lr];
  if (CNT > 1) ldrow(1, A1, D1);
  store_tile(dk, LI, U, Mp, 16 * k, 16 * k, tile);
  blk[0] = dk;
#pragma unroll
  for (int ii = 1; ii < CNT; ++ii) {
    if (ii + 1 < CNT) {
      if ((ii + 1) & 1) ldrow(ii + 1, A1, D1);
      else ldrow(ii + 1, A0, D0);
    }
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int jj = 0; jj < MAXR; ++jj)
      if (jj < ii) {
#pragma unroll
        for (int st = 0; st < 4; ++st)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64((ii & 1) ? A1[jj * 4 + st] : A0[jj * 4 + st], blk[jj][st], acc, 0, 0, 0);
      }
    d4 out = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int st = 0; st < 4; ++st)
      out = __builtin_amdgcn_mfma_f64_16x16x4f64(-((ii & 1) ? D1[st] : D0[st]), acc[st], out, 0, 0, 0);
    store_tile(out, LI, U, Mp, 16 * (k + ii), 16 * k, tile);
    blk[ii] = out;
  }
}
__device__ __noinline__ void tri_inverse_strip(ldsd* tiles) {
  const int nb = g_sh.f.Mp / 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  ldsd* tile = tiles + wave * 16 * 17;
  for (int k = wave; k < nb; k += NW) {
    switch (nb - k) {
      case 1: inv_column<1>(k, tile); break;
      case 2: inv_column<2>(k, tile); break;
      case 3: inv_column<3>(k, tile); break;
      case 4: inv_column<4>(k, tile); break;
#if GAPRO_NT >= 320
      case 5: inv_column<5>(k, tile); break;
      case 6: inv_column<6>(k, tile); break;
      case 7: inv_column<7>(k, tile); break;
      default: inv_column<8>(k, tile); break;
#else
      default: break;  // M_p <= 64 on the small-fit route
#endif
    }
  }
}

// ---- LI = L^-1 (lower) and U = LI^T, one 16-wide block column per wave -----------------------------
//   LI_kk = Dinv_k;   LI_ik = -Dinv_i * sum_{j=k}^{i-1} L_ij LI_jk   (i > k)
// Block columns are independent.  For nb <= NBR the blocks of the column stay in registers (an MFMA
// result in C layout is directly the B operand of the next product: register r holds rows 4r + lane/16);
// longer columns re-read their own blocks from memory after a workgroup-scope fence.
template <int NBR>
__device__ __noinline__ void tri_inverse(ldsd* tiles) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp, nb = Mp / 16;
  const gd* LT = f.mat[B_LT];
  gd* LI = f.mat[B_LI];
  gd* U = f.mat[B_U];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  ldsd* tile = tiles + wave * 16 * 17;
  // Which wave takes which block column.  NBR > 0 (M_p <= 128): round-robin, at most one column per wave.  Long
  // columns (NBR == 0, round 4): a column of n blocks is a serial chain of n (n - 1) / 2 block products, and dealt
  // round-robin wave 0 got columns 0, 8, 16, ... -- 1.5x the mean work at M_p = 384, with the whole workgroup waiting
  // for it at the barrier behind this phase.  Longest-processing-time-first instead: columns in ascending k (descending
  // cost) each go to the wave with the least work so far (every wave computes the same table; the result of a column
  // does not depend on who computes it: bit-identical).
  unsigned long long mine = 0;  // bit k: this wave computes block column k (nb <= 32)
  if (NBR == 0) {
    int load[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) load[w] = 0;
    for (int k = 0; k < nb; ++k) {
      int best = 0;
#pragma unroll
      for (int w = 1; w < NW; ++w) best = load[w] < load[best] ? w : best;
      const int n = nb - k;
#pragma unroll
      for (int w = 0; w < NW; ++w) load[w] += (w == best) ? n * (n - 1) / 2 + 1 : 0;
      if (best == wave) mine |= 1ull << k;
    }
  }
  for (int k = NBR > 0 ? wave : 0; k < nb; k += NBR > 0 ? NW : 1) {
    if (NBR == 0 && !((mine >> k) & 1ull)) continue;
    d4 blk[NBR > 0 ? NBR : 1];
    d4 dk;
#pragma unroll
    for (int r = 0; r < 4; ++r) dk[r] = f.dinv[(size_t)k * 256 + (lq + 4 * r) * 16 + lr];
    store_tile(dk, LI, U, Mp, 16 * k, 16 * k, tile);
    if (NBR > 0) blk[0] = dk;
    if (NBR > 0) {
      // relative row index ii = i - k is a compile-time constant: every register index is static
#pragma unroll
      for (int ii = 1; ii < NBR; ++ii) {
        const int i = k + ii;
        if (i < nb) {
          d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int jj = 0; jj < ii; ++jj) {
            const gd* pa = LT + (size_t)(16 * (k + jj) + lq) * Mp + 16 * i + lr;  // L[16i+lr][16(k+jj)+4s+lq]
#pragma unroll
            for (int sstep = 0; sstep < 4; ++sstep)
              acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[(size_t)(4 * sstep) * Mp], blk[jj][sstep], acc, 0, 0, 0);
          }
          d4 out = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int sstep = 0; sstep < 4; ++sstep) {
            const double a = -f.dinvT[(size_t)i * 256 + (4 * sstep + lq) * 16 + lr];  // -Dinv_i[lr][4s + lq]
            out = __builtin_amdgcn_mfma_f64_16x16x4f64(a, acc[sstep], out, 0, 0, 0);
          }
          store_tile(out, LI, U, Mp, 16 * i, 16 * k, tile);
          blk[ii] = out;
        }
      }
    } else {
      for (int i = k + 1; i < nb; ++i) {
        // nacc = -sum_{j = k}^{i - 1} L_ij LI_jk through the Cholesky update's double-buffered block loop (round 4: the
        // loop here issued the eight loads of a block and waited for them before its four MFMAs, one memory round trip
        // per block of a chain of up to nb (nb - 1) / 2 blocks).  -(a) b accumulated is exactly -(a b accumulated), and
        // (-Dinv) x = Dinv (-x): the same bits as before.
        d4 nacc = (d4){0.0, 0.0, 0.0, 0.0};
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        chol_update_tile(nacc, LT + (size_t)(16 * k + lq) * Mp + 16 * i + lr, LI + (size_t)(16 * k + lq) * Mp + 16 * k + lr,
                         Mp, 16 * (i - k));
        d4 out = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int sstep = 0; sstep < 4; ++sstep) {
          const double a = f.dinvT[(size_t)i * 256 + (4 * sstep + lq) * 16 + lr];  // Dinv_i[lr][4s + lq]
          out = __builtin_amdgcn_mfma_f64_16x16x4f64(a, nacc[sstep], out, 0, 0, 0);
        }
        store_tile(out, LI, U, Mp, 16 * i, 16 * k, tile);
      }
    }
  }
}

// ---- elementwise passes, thread-per-column ------------------------------------------------------------
// Threads are laid out as G row groups x Mp columns (Mp <= NT).  A thread owns one column and walks rows
// group, group+G, ...; per-column partial results of the G groups are combined in a fixed order through
// `red` ([kRedSlots][NT] doubles).
struct ColMap {
  int G, col, grp;
  bool active;
};
__device__ inline ColMap col_map(int Mp) {
  ColMap c;
  c.G = NT / Mp;
  c.col = threadIdx.x % Mp;
  c.grp = threadIdx.x / Mp;
  c.active = c.grp < c.G;
  return c;
}

// KX[k][n] = s exp(-|Z_k - P_n|^2 / (2 l^2)) for k < M, n < ncols, zero elsewhere (Pt: staged points)
template <int DC>
__device__ __noinline__ void build_kx(const ldsd* Zt, const ldsd* Pt, int ncols, double s, double inv_l2) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp, M = f.M, D = DC ? DC : f.D;
  gd* KX = f.mat[B_KX];
  const ColMap cm = col_map(Mp);
  if (!cm.active) return;
  const int n = cm.col;
  for (int k = cm.grp; k < Mp; k += cm.G) {
    double v = 0.0;
    if (k < M && n < ncols) v = s * gapro_fit_math::rbf_exp(-0.5 * inv_l2 * sqdist_t(Zt, k, Pt, n, D, Mp));
    KX[(size_t)k * Mp + n] = v;
  }
}

// mu[n] = sum_i m[i] A[i][n],  var[n] = s + jitter + sum_i (BM[i][n]^2 - A[i][n]^2)
__device__ __noinline__ void mean_var(double s, double jitter, ldsd* red) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp;
  const gd* A = f.mat[B_A];
  const gd* BM = f.mat[B_BM];
  const gd* m = f.vec[V_M];
  const ColMap cm = col_map(Mp);
  double pm = 0.0, pv = 0.0;
  if (cm.active) {
    for (int i = cm.grp; i < Mp; i += cm.G) {
      const double a = A[(size_t)i * Mp + cm.col], b = BM[(size_t)i * Mp + cm.col];
      pm += m[i] * a;
      pv += b * b - a * a;
    }
  }
  red[threadIdx.x] = pm;
  red[NT + threadIdx.x] = pv;
  __syncthreads();
  if (threadIdx.x < Mp) {
    double sm = 0.0, sv = 0.0;
    for (int g = 0; g < cm.G; ++g) {
      sm += red[g * Mp + threadIdx.x];
      sv += red[NT + g * Mp + threadIdx.x];
    }
    f.vec[V_MU][threadIdx.x] = sm;
    f.vec[V_VAR][threadIdx.x] = s + jitter + sv;
  }
  __syncthreads();
}

// out[c] = sum_r w[r] Mtx[r][c]
__device__ __noinline__ void weighted_colsum(const gd* Mtx, const gd* w, int Mp, gd* out, ldsd* red) {
  const ColMap cm = col_map(Mp);
  double p = 0.0;
  if (cm.active)
    for (int r = cm.grp; r < Mp; r += cm.G) p += w[r] * Mtx[(size_t)r * Mp + cm.col];
  red[threadIdx.x] = p;
  __syncthreads();
  if (threadIdx.x < Mp) {
    double sacc = 0.0;
    for (int g = 0; g < cm.G; ++g) sacc += red[g * Mp + threadIdx.x];
    out[threadIdx.x] = sacc;
  }
  __syncthreads();
}

// Expected log-likelihood terms: 20-point Gauss-Hermite of log Phi(y f), ten threads per point (one per
// symmetric node pair).  Writes g_mu[n] = -dE/dmu / N and g_v[n] = -dE/dvar / N (0 where the variance
// was clamped), returns sum_n E_n when want_e.
__device__ __noinline__ double quadrature(double c, double min_variance, double Nd, bool want_e, ldsd* red,
                                          double* g_c, double* gv_sum) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp, M = f.M;
  gd* gmu = f.vec[V_GMU];
  gd* gv = f.vec[V_GV];
  double e_tot = 0.0, gc_part = 0.0, gvs_part = 0.0;
  constexpr int PPR = NT / 10;  // points per round
  const int q = threadIdx.x % 10, nl = threadIdx.x / 10;
  for (int n0 = 0; n0 < M; n0 += PPR) {
    const int n = n0 + nl;
    double E = 0.0, dmu = 0.0, dvar = 0.0;
    const bool on = nl < PPR && n < M;
    if (on) {
      const double mu = f.vec[V_MU][n] + c;
      const double vraw = f.vec[V_VAR][n];
      const double var = vraw < min_variance ? min_variance : vraw;
      const double sd = sqrt(2.0 * var);
      const double y = n < f.M1 ? -1.0 : 1.0;  // train_y, not read from memory (global-memory latency in this chain)
      const double t = c_gh_t[q], w = c_gh_w[q];
      gh_pair(y, mu, sd, t, w, want_e, &E, &dmu, &dvar);
    }
    red[threadIdx.x] = E;
    red[NT + threadIdx.x] = dmu;
    red[2 * NT + threadIdx.x] = dvar;
    __syncthreads();
    if (on && q == 0) {
      double se = 0.0, sm = 0.0, sv = 0.0;
      for (int qq = 0; qq < 10; ++qq) {
        se += red[threadIdx.x + qq];
        sm += red[NT + threadIdx.x + qq];
        sv += red[2 * NT + threadIdx.x + qq];
      }
      const double ipi = 0.56418958354775628695;  // 1/sqrt(pi)
      const double vraw = f.vec[V_VAR][n];
      const bool clamped = vraw < min_variance;
      const double var = clamped ? min_variance : vraw;
      const double y = n < f.M1 ? -1.0 : 1.0;  // train_y, not read from memory (global-memory latency in this chain)
      const double g1 = -(ipi * sm * y) / Nd;
      const double g2 = clamped ? 0.0 : -(ipi * sv * y / sqrt(2.0 * var)) / Nd;
      gmu[n] = g1;
      gv[n] = g2;
      e_tot += ipi * se;
      gc_part += g1;
      gvs_part += g2;
    }
    __syncthreads();
  }
  for (int n = M + threadIdx.x; n < Mp; n += NT) {
    gmu[n] = 0.0;
    gv[n] = 0.0;
  }
  *g_c = block_sum(gc_part);
  *gv_sum = block_sum(gvs_part);
  return want_e ? block_sum(e_tot) : 0.0;
}

// Fused kernel-gradient pass + Adam on Z.  The thread owning column j accumulates over rows i:
//   zz: w  = sym(G)[i][j] s E_ij  ->  G_s += sym(G) E,  G_l += w d2,   G_Z[j] += 2 w (Z_j - Z_i)
//   zx: wx = G_KX[j][n=i] KX_jn   ->  G_s += G_KX E,    G_l += wx d2,  G_Z[j] += wx (Z_j - X_i)
// (sym(G) o K is symmetric, so the sum over i of column j equals the row sum of the oracle's formula.)
template <int DMAX, bool ZX, int U, int DC>
__device__ __noinline__ void kernel_grads_adam_z(ldsd* Zt, const ldsd* Xt, const gd* Gm, const gd* GTm,
                                                 const gd* GKXT, double s, double inv_l2, double step_size,
                                                 double bc2s, ldsd* red, double* gs_out, double* gl_out,
                                                 const ldsd* zx_rows = nullptr) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp, M = f.M, D = DC ? DC : f.D;
  const ColMap cm = col_map(Mp);
  const int j = cm.col;
  double acc[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) acc[d] = 0.0;
  double gs = 0.0, gl = 0.0;
  if (DMAX > 8) {
    // Wide features (deep features, D = 32): the difference vectors are never held in registers.  With
    //   sum_i w_i (Z_j - P_i) = Z_j sum_i w_i - sum_i w_i P_i
    // only acc[d] = sum_i w_i P_i[d] and the scalar sum of the weights are accumulated; Z_j, Z_i, X_i are
    // re-read from LDS (conflict-free / broadcast), which keeps the pass inside a 128-VGPR budget.
    double wsum = 0.0;
    if (cm.active && j < M) {
      for (int i = cm.grp; i < M; i += cm.G) {
        const size_t o = (size_t)i * Mp + j;
        const double gsym = 0.5 * (Gm[o] + GTm[o]);
        const double g3 = ZX ? GKXT[o] : 0.0;  // G_KX[j][i]
        double d2 = 0.0, d2x = 0.0;
#pragma unroll 8
        for (int d = 0; d < D; ++d) {
          const double zjd = Zt[d * Mp + j];
          const double a = zjd - Zt[d * Mp + i];
          d2 += a * a;
          if (ZX) {
            const double bx = zjd - Xt[d * Mp + i];
            d2x += bx * bx;
          }
        }
        const double e = gapro_fit_math::rbf_exp(-0.5 * inv_l2 * d2);
        const double w = gsym * s * e;
        gs += gsym * e;
        gl += w * d2;
        double wx = 0.0;
        if (ZX) {
          const double ex = gapro_fit_math::rbf_exp(-0.5 * inv_l2 * d2x);
          wx = g3 * s * ex;
          gs += g3 * ex;
          gl += wx * d2x;
        }
        wsum += 2.0 * w + wx;
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
          if (d < D) acc[d] += 2.0 * w * Zt[d * Mp + i] + (ZX ? wx * Xt[d * Mp + i] : 0.0);
      }
    }
#pragma unroll
    for (int d = 0; d < DMAX; ++d) acc[d] = (d < D) ? wsum * Zt[d * Mp + j] - acc[d] : 0.0;
  } else if (cm.active && j < M) {
    double zj[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) zj[d] = (d < D) ? Zt[d * Mp + j] : 0.0;
    // the (up to) 3 U operand loads of U rows are issued before the first exp: one memory round trip per
    // U rows instead of one per row (U is chosen per calling kernel to fit its register budget; a distinct U
    // also keeps the two kernels from sharing one instantiation compiled for the tighter budget)
    for (int i0 = cm.grp; i0 < M; i0 += cm.G * U) {
      double g1[U], g2[U], g3[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * cm.G;
        const bool act = i < M;
        const size_t o = (size_t)(act ? i : 0) * Mp + j;
        g1[u] = act ? Gm[o] : 0.0;
        g2[u] = act ? GTm[o] : 0.0;
        g3[u] = (ZX && act) ? GKXT[o] : 0.0;  // G_KX[j][i]
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * cm.G;
        if (u * cm.G >= M) break;  // wave-uniform: no row of this or any later u exists (small M)
        if (i < M) {
          double t[DMAX];
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < DMAX; ++d) {
            t[d] = (d < D) ? zj[d] - Zt[d * Mp + i] : 0.0;
            d2 += t[d] * t[d];
          }
          const double e = gapro_fit_math::rbf_exp(-0.5 * inv_l2 * d2);
          const double gsym = 0.5 * (g1[u] + g2[u]);
          const double w = gsym * s * e;
          gs += gsym * e;
          gl += w * d2;
#pragma unroll
          for (int d = 0; d < DMAX; ++d) acc[d] += 2.0 * w * t[d];
          if (ZX) {
            double d2x = 0.0;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
              t[d] = (d < D) ? zj[d] - Xt[d * Mp + i] : 0.0;
              d2x += t[d] * t[d];
            }
            const double ex = gapro_fit_math::rbf_exp(-0.5 * inv_l2 * d2x);
            const double wx = g3[u] * s * ex;
            gs += g3[u] * ex;
            gl += wx * d2x;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) acc[d] += wx * t[d];
          }
        }
      }
    }
  }
  prof_stamp(20);
  *gs_out = block_sum(gs);
  *gl_out = block_sum(gl);
  prof_stamp(21);
  // combine the row groups, kRedSlots feature dimensions at a time, then Adam on Z (and its LDS copy)
  const double b1 = 0.9, b2 = 0.999, aeps = 1e-8;
#pragma unroll
  for (int dc = 0; dc < DMAX; dc += kRedSlots) {
    if (dc < D) {
#pragma unroll
      for (int e = 0; e < kRedSlots; ++e)
        if (dc + e < DMAX) red[e * NT + threadIdx.x] = acc[dc + e];
      __syncthreads();
      if (threadIdx.x < M) {
#pragma unroll
        for (int e = 0; e < kRedSlots; ++e) {
          const int d = dc + e;
          if (d < D && d < DMAX) {
            double sacc = 0.0;
            for (int g = 0; g < cm.G; ++g) sacc += red[e * NT + g * Mp + threadIdx.x];
            const size_t zi = (size_t)threadIdx.x * D + d;
            if (!ZX) sacc += zx_rows ? zx_rows[threadIdx.x * 8 + d] : f.gZ[zi];  // zx part of the strip loop (raw sums)
            const double grad = -inv_l2 * sacc;
            f.gZ[zi] = grad;
            const double m1 = b1 * f.mZ[zi] + (1.0 - b1) * grad;
            const double m2 = b2 * f.vZ[zi] + (1.0 - b2) * grad * grad;
            f.mZ[zi] = m1;
            f.vZ[zi] = m2;
            const double znew = f.Z[zi] - step_size * m1 / (sqrt(m2) / bc2s + aeps);
            f.Z[zi] = znew;
            Zt[d * Mp + threadIdx.x] = znew;
          }
        }
      }
      __syncthreads();
    }
  }
}

// one product of the staged kernel: workgroup-tiled through LDS (WG; extents and ranges per 16 x 16 block) or one
// tile per wave from global memory (gemm_tn)
// (PK / QK: operands with the contraction index along their rows, see gemm_tn; lower-triangular outputs only -- the
// workgroup-tiled form takes k-major operands)
template <int WG, int TU, bool SCALE, int ORD, int PK = 0, int QK = 0, typename KRange, typename Epi>
__device__ inline void product(int mo, int no, bool lower, const gd* __restrict__ P, const gd* __restrict__ Q, int ld,
                               const gd* __restrict__ qs, KRange kr, Epi epi, ldsd* ring) {
  if constexpr (WG == 0) {
    gemm_tn_in<TU, SCALE, 2, ORD, true, PK, QK>(mo, no, lower, P, Q, ld, qs, kr, epi);
  } else {
    // Workgroup-tiled products take the part of the output that whole 128 x 128 tiles cover; what is left at the
    // matrix edge (an L of up to 96 rows / columns, M_p a multiple of 32) goes to the per-wave products as 32 x 32
    // tiles: a workgroup tile with 32 valid rows costs as much as a full one (one wave strip in four has work), which
    // made M_p = 288 25 % slower than the per-wave form.  Same blocks, same k order: the split does not change a bit.
    // (extents rounded up to the strips' 32: the per-wave 32 x 32 form computes a last half-filled tile in full, M_p is
    // a multiple of 32 here)
    const int rows = (16 * mo + 31) / 32 * 32, cols = (16 * no + 31) / 32 * 32;
    const int R = rows / kWgTile * kWgTile, Cc = cols / kWgTile * kWgTile;
    constexpr bool kMajor = !(PK || QK);  // the workgroup-tiled form takes k-major operands only
    if constexpr (kMajor) {
      if (R > 0 && Cc > 0 && !lower) gemm_wg<SCALE, true, WG>(R / 16, Cc / 16, false, P, Q, ld, qs, kr, epi, ring);
    }
    auto strip_t = [&](auto tu_tag, int r0, int c0, int nr, int nc, bool low) {
      constexpr int TUS = decltype(tu_tag)::value;  // 2: 32 x 32 wave tiles, 4: 64 x 64 (extents in half tiles)
      if (nr <= 0 || nc <= 0) return;
      // (row-major tile order: the shell order of some products enumerates SQUARE tile grids only)
      gemm_tn_in<TUS, SCALE, 2, ORD_ROWMAJOR, true, PK, QK>(
          nr / (8 * TUS), nc / (8 * TUS), low, PK ? P + (size_t)r0 * ld : P + r0, QK ? Q + (size_t)c0 * ld : Q + c0, ld, qs,
          [=](int i0, int j0, int* lo, int* hi) {
            int l0, h0, l1, h1;  // a wave tile's range: the hull of its 16 x 16 blocks' (kr is monotone; gemm_tn trims hi)
            kr(r0 + i0, c0 + j0, &l0, &h0);
            kr(r0 + i0 + 16 * TUS - 16, c0 + j0 + 16 * TUS - 16, &l1, &h1);
            *lo = l0;
            *hi = h1;
          },
          shifted_epi(epi, r0, c0));
    };
    auto strip = [&](int r0, int c0, int nr, int nc, bool low) {  // rows [r0, r0 + nr) x columns [c0, c0 + nc)
      strip_t(std::integral_constant<int, 2>{}, r0, c0, nr, nc, low);
    };
    if (lower) {
      // Lower-triangular outputs (G_LS with its Adam epilogue, G_L, Pm) stay per-wave as a whole: a diagonal workgroup
      // tile computes 64 blocks for the 36 it needs, and these are the products with the heaviest epilogues, which the
      // eight waves of a tile then run in lockstep (fit-level, M = 256 two per CU: G_LS 15.6 -> 22.5, Pm 4.0 -> 5.3 ms
      // per fit with the tiled form; G_KX, G, G_A the other way).  64 x 64 wave tiles where round 2 used them.
      if constexpr (WG == 4) {
        if (rows >= 352) {
          strip_t(std::integral_constant<int, 4>{}, 0, 0, rows, cols, true);
          return;
        }
      }
      strip(0, 0, rows, cols, true);
      return;
    }
    if constexpr (kMajor) {
      strip(R, 0, rows - R, cols, false);   // bottom strip, full width
      strip(0, Cc, R, cols - Cc, false);    // right strip above it
    } else {
      strip(0, 0, rows, cols, false);
    }
  }
}

// Common prologue of the fit kernels: workspace pointers, parameter initialisation
// (gaussian_process_utils.py:386-403 and gpytorch's parameter inits), staging of Z and X into LDS.
__device__ inline void fit_setup(const gapro_fit_desc& desc, int D, const float* __restrict__ feats_spp,
                                 const int* __restrict__ idx, const double* __restrict__ init_mean,
                                 double* __restrict__ ws, ldsd* Zt, ldsd* Pt) {
  Shared& sh = g_sh;
  Fit& f = sh.f;
  const Layout lay = make_layout(desc.m1 + desc.m2, desc.t, D);
  gd* base = (gd*)(ws + desc.ws_offset);
  if (threadIdx.x == 0) {
    f.M = desc.m1 + desc.m2;
    f.M1 = desc.m1;
    f.T = desc.t;
    f.D = D;
    f.Mp = lay.Mp;
    for (int b = 0; b < B_COUNT; ++b) f.mat[b] = base + lay.mat + (long long)b * lay.Mp * lay.Mp;
    for (int v = 0; v < V_COUNT; ++v) f.vec[v] = base + lay.vec + (long long)v * lay.Mp;
    f.X = base + lay.xz;
    f.Z = f.X + (long long)lay.Mp * D;
    f.mZ = f.Z + (long long)lay.Mp * D;
    f.vZ = f.mZ + (long long)lay.Mp * D;
    f.gZ = f.vZ + (long long)lay.Mp * D;
    f.Xt = base + lay.xt;
    f.dinv = base + lay.dinv;
    f.dinvT = f.dinv + (long long)lay.Mp * 16;
    f.scal = base + lay.scal;
    sh.c = 0.0;
    sh.rho_s = 0.0;
    sh.rho_l = 0.0;
    sh.status = GAPRO_OK;
    sh.chol_bad = 0;
#ifdef GAPRO_PROFILE
    for (int i = 0; i < kProfSlots; ++i) sh.prof[i] = 0;
    sh.t_last = wall_clock64();
    sh.t_start = sh.t_last;
#endif
  }
  const int M = desc.m1 + desc.m2, Mp = lay.Mp;
  // zero everything the kernel reads before writing: parameters/Adam state, padded operand tails
  for (long long i = threadIdx.x; i < lay.total; i += NT) base[i] = 0.0;
  __syncthreads();
  const int* my_idx = idx + desc.idx_offset;
  for (int e = threadIdx.x; e < M * D; e += NT) {
    const int i = e / D, d = e - i * D;
    const double v = (double)feats_spp[(size_t)my_idx[i] * D + d];  // train_x = cat(b1_feats, b2_feats)  :395
    f.X[e] = v;
    f.Z[e] = v;  // inducing points initialised to train_x  (:14)
  }
  for (int e = threadIdx.x; e < desc.t * D; e += NT) {
    const int i = e / D, d = e - i * D;
    f.Xt[e] = (double)feats_spp[(size_t)my_idx[M + i] * D + d];  // intersect_feats  :386
  }
  for (int i = threadIdx.x; i < M; i += NT) {
    f.vec[V_Y][i] = i < desc.m1 ? -1.0 : 1.0;  // train_y  :396-398
    f.vec[V_M][i] = init_mean ? init_mean[desc.idx_offset + i] : 0.0;
    f.mat[B_LS][(size_t)i * Mp + i] = 1.0;  // chol_variational_covar = I
    f.mat[B_LST][(size_t)i * Mp + i] = 1.0;
  }
  __syncthreads();
  stage_points_t(Zt, f.Z, M, D, Mp);
  stage_points_t(Pt, f.X, M, D, Mp);
  __syncthreads();
}

__device__ inline void fit_epilogue(const gapro_fit_desc& desc, const gapro_fit_options& opt, int* o_status,
                                    double* o_loss) {
  __syncthreads();
  if (threadIdx.x == 0) {
    int st = g_sh.status;
    if (st == GAPRO_OK && !isfinite(o_loss[desc.slot]) && opt.training_iter > 0) st = GAPRO_ERR_NOT_FINITE;
    o_status[desc.slot] = st;
    g_sh.f.scal[S_STATUS] = (double)st;
  }
}

}  // namespace
