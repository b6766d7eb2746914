// The strip-streaming single-workgroup fit kernel k_svgp_fit_strip<DMAX, DC> (M_p <= 128), on the machinery of
// fit_wg.h.  Built with 512 threads per fit by svgp_fit_wg.hip and with 256 by svgp_fit_small.hip (M_p <= 64, there
// named k_svgp_fit_strip256).
#pragma once
#include "fit_wg.h"

namespace {

// =====================================================================================================
// Strip-streaming variant (M_p <= 128): the data-dependent intermediates never touch global memory.
//
// Everything between the triangular factors and the gradients is column-wise in the data index n:
//   KX[:,n] -> A[:,n] = LI KX[:,n] -> B[:,n] = LS^T A[:,n] -> mu_n, var_n -> g_mu_n, g_v_n
//   -> G_A[:,n] = m g_mu_n + LS (2 g_v_n B[:,n]) - 2 g_v_n A[:,n] -> G_KX[:,n] = LI^T G_A[:,n]
// and the only couplings across n are sums:  G_LS += A[:,n] (2 g_v_n B[:,n])^T,  G_L -= G_KX[:,n] A[:,n]^T,
// G_m += A[:,n] g_mu_n, and the kernel-gradient sums.  So the training points are streamed in strips of
// SW = 32 columns held in three LDS buffers (row stride RS = 34: conflict-free for both MFMA operand
// patterns), the two M x M gradient matrices are accumulated as MFMA tiles that stay in registers for
// the whole step (each wave owns up to five 16x16 lower tiles of each), and KX, A, A^T, B, B^T, G_A, G_KX^T
// -- 9 matrix writes and ~13 matrix reads per step in the staged kernel -- disappear from HBM traffic.
// What still streams from L2/HBM per strip are the fixed operands U, LS, LS^T, LI (triangular halves).
// =====================================================================================================
constexpr int SW = 32;  // strip width (data columns)
constexpr int RS = 34;  // LDS row stride of a strip buffer (doubles)
constexpr int kStripMaxMp = 128;
constexpr int kAccTiles = 5;  // lower 16x16 tiles of an 8x8-block matrix: 36 over 8 waves

inline __host__ __device__ int strip_region_doubles(int Mp) {
  const int a = 3 * Mp * RS, b = scratch_doubles(Mp), c = 2 * (Mp * 17 + 64 * 17);  // c: two Cholesky panels
  const int m = a > b ? a : b;
  return m > c ? m : c;
}
inline __host__ __device__ long long strip_lds_bytes(int m, int d) {
  const int Mp = gapro_pad_m(m, d);
  // (+ 8 Mp: the per-row kernel-gradient sums of the fused zx pass, narrow features only)
  return 8LL * (2LL * d * Mp + strip_region_doubles(Mp) + 3 * NT + Mp + 4 * SW + 32 + (d <= 8 ? 8 * Mp : 0));
}
inline __host__ __device__ bool strip_ok(int m, int d) {
  return gapro_pad_m(m, d) <= kStripMaxMp && d <= 32 && strip_lds_bytes(m, d) <= kMaxDynLds;
}

enum { K_LE = 0, K_GE = 1 };
// One strip product: out[16 rb .. ][16 ct ..] = sum_k P[k][16 rb + i] * Sin[k][16 ct + n], k restricted to
// k < 16 (rb+1) (K_LE: P upper-triangular in (k,i)) or k >= 16 rb (K_GE).  Wave rb owns row block rb and both
// 16-column tiles of the strip (at most 8 k-blocks, 16 MFMA groups).  The A operand streams from global memory
// (TN rows); the fixed operand matrices of 256 concurrent fits do not stay in L2, so a fetch costs ~1 us under
// load: ALL of the wave's A fragments (<= 32 loads) are issued up front and the MFMAs consume them in order,
// paying that latency once per product instead of once per k-block.  The B operand comes from the LDS strip buffer.
constexpr int kStripBlocks = kStripMaxMp / 16 + 1;
template <int MODE, typename Epi>
__device__ __noinline__ void strip_gemm(const gd* __restrict__ P, int Mp, const ldsd* Sin, int nbk, Epi epi) {
  // its own function on purpose: the caller keeps 80 accumulator registers alive across it (callee-saved
  // VGPRs), and in here the 36 operand loads must all be in flight at once without a spill between them
  P = uni_ptr(P);
  Mp = uni(Mp);
  nbk = uni(nbk);
  const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  // One row block per wave, BOTH column tiles of the strip: every A fragment is fetched once per workgroup (dealing
  // the 2 nbk tiles out one by one balances the MFMAs better, 9 blocks per wave instead of up to 16, but fetches
  // every fragment twice, and the strip products wait for their operands, not for the matrix cores).
  const int rb = wave;
  if (rb >= nbk) return;
  const int kb0 = MODE == K_LE ? 0 : rb, n = MODE == K_LE ? rb + 1 : nbk - rb;  // first k-block, block count
  const size_t sa = (size_t)4 * Mp;
  double a[kStripBlocks][4];
#pragma unroll
  for (int blk = 0; blk < kStripBlocks; ++blk) {
    if (blk < n) {
      const gd* pa = P + (size_t)(16 * (kb0 + blk) + lq) * Mp + 16 * rb + lr;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a[blk][ks] = pa[ks * sa];
    }
  }
  d4 acc0 = (d4){0.0, 0.0, 0.0, 0.0}, acc1 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int blk = 0; blk < kStripBlocks; ++blk) {
    if (blk < n) {
      const ldsd* pb = Sin + (16 * (kb0 + blk) + lq) * RS + lr;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[blk][ks], pb[4 * ks * RS], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[blk][ks], pb[4 * ks * RS + 16], acc1, 0, 0, 0);
      }
    }
  }
  epi(rb, 0, acc0);
  epi(rb, 1, acc1);
}

__device__ inline void lower_tile(int t, int* ti, int* tj) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  *ti = i;
  *tj = t - i * (i + 1) / 2;
}

// The register-hungry, MFMA-free parts of a strip are separate functions: values that live across a call
// (the gradient tiles) are kept in callee-saved VGPRs instead of being spilled around inlined libm code.
template <int DC>
__device__ __noinline__ void strip_fill_kx(ldsd* Cs, const ldsd* Zt, const ldsd* Xpts, int n0, int nc, double s,
                                           double inv_l2) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp, M = f.M, D = DC ? DC : f.D;
  for (int idx = threadIdx.x; idx < Mp * SW; idx += NT) {
    const int k = idx / SW, n = idx - k * SW;
    double v = 0.0;
    if (k < M && n < nc) v = s * gapro_fit_math::rbf_exp(-0.5 * inv_l2 * sqdist_t(Zt, k, Xpts, n0 + n, D, Mp));
    Cs[k * RS + n] = v;
  }
  __syncthreads();
}

// mu_s[n] = sum_i m[i] As[i][n],  var_s[n] = s + jitter + sum_i (Bs[i][n]^2 - As[i][n]^2) for the SW strip columns
__device__ __noinline__ void strip_mean_var(const ldsd* As, const ldsd* Bs, const ldsd* m_s, ldsd* sred, ldsd* mu_s,
                                            ldsd* var_s, double s, double jitter) {
  const int Mp = g_sh.f.Mp;
  const int n = threadIdx.x % SW, p = threadIdx.x / SW;  // NT / SW row groups
  double pm = 0.0, pv = 0.0;
  for (int i = p; i < Mp; i += NT / SW) {
    const double a = As[i * RS + n], b = Bs[i * RS + n];
    pm += m_s[i] * a;
    pv += b * b - a * a;
  }
  sred[threadIdx.x] = pm;
  sred[NT + threadIdx.x] = pv;
  __syncthreads();
  if (threadIdx.x < SW) {
    double sm = 0.0, sv = 0.0;
    for (int g = 0; g < NT / SW; ++g) {
      sm += sred[g * SW + threadIdx.x];
      sv += sred[NT + g * SW + threadIdx.x];
    }
    mu_s[threadIdx.x] = sm;
    var_s[threadIdx.x] = s + jitter + sv;
  }
  __syncthreads();
}

#if GAPRO_NT >= 10 * 32
// Likelihood gradients of the strip columns (ten threads per column, one per symmetric Gauss-Hermite pair):
// gmu_s / gv_s for the strip, and this thread's contributions to sum E, sum g_mu, sum g_v in out3[0..2].
__device__ __noinline__ void strip_likelihood(const ldsd* mu_s, const ldsd* var_s, ldsd* gmu_s, ldsd* gv_s, ldsd* sred,
                                              int n0, int nc, double c, double min_variance, double Nd,
                                              bool want_e, double* out3) {
  const Fit& f = g_sh.f;
  const int q = threadIdx.x % 10, nl = threadIdx.x / 10;
  double E = 0.0, dmu = 0.0, dvar = 0.0;
  const bool on = nl < nc;
  if (on) {
    const double mu = mu_s[nl] + c;
    const double vraw = var_s[nl];
    const double var = vraw < min_variance ? min_variance : vraw;
    const double sd = sqrt(2.0 * var);
    const double y = n0 + nl < f.M1 ? -1.0 : 1.0;  // train_y (see quadrature)
    const double t = c_gh_t[q], w = c_gh_w[q];
    gh_pair(y, mu, sd, t, w, want_e, &E, &dmu, &dvar);
  }
  sred[threadIdx.x] = E;
  sred[NT + threadIdx.x] = dmu;
  sred[2 * NT + threadIdx.x] = dvar;
  __syncthreads();
  double e_add = 0.0, gc_add = 0.0, gv_add = 0.0;
  if (on && q == 0) {
    double se = 0.0, sm = 0.0, sv = 0.0;
    for (int qq = 0; qq < 10; ++qq) {
      se += sred[threadIdx.x + qq];
      sm += sred[NT + threadIdx.x + qq];
      sv += sred[2 * NT + threadIdx.x + qq];
    }
    const double ipi = 0.56418958354775628695;  // 1/sqrt(pi)
    const double vraw = var_s[nl];
    const bool clamped = vraw < min_variance;
    const double var = clamped ? min_variance : vraw;
    const double y = n0 + nl < f.M1 ? -1.0 : 1.0;  // train_y (see quadrature)
    const double g1 = -(ipi * sm * y) / Nd;
    const double g2 = clamped ? 0.0 : -(ipi * sv * y / sqrt(2.0 * var)) / Nd;
    gmu_s[nl] = g1;
    gv_s[nl] = g2;
    e_add = ipi * se;
    gc_add = g1;
    gv_add = g2;
  }
  if ((int)threadIdx.x >= nc && threadIdx.x < SW) {
    gmu_s[threadIdx.x] = 0.0;
    gv_s[threadIdx.x] = 0.0;
  }
  out3[0] = e_add;
  out3[1] = gc_add;
  out3[2] = gv_add;
  __syncthreads();
}
#else
// 256 threads cover 25 columns per pass: a 32-column strip takes two
__device__ __noinline__ void strip_likelihood(const ldsd* mu_s, const ldsd* var_s, ldsd* gmu_s, ldsd* gv_s, ldsd* sred,
                                              int n0, int nc, double c, double min_variance, double Nd,
                                              bool want_e, double* out3) {
  const Fit& f = g_sh.f;
  constexpr int kCols = NT / 10;  // columns per pass: 51 with 512 threads (one pass per strip), 25 with 256
  const int q = threadIdx.x % 10, nl0 = threadIdx.x / 10;
  double e_add = 0.0, gc_add = 0.0, gv_add = 0.0;
  for (int cbase = 0; cbase < nc; cbase += kCols) {
    const int nl = cbase + nl0;
    double E = 0.0, dmu = 0.0, dvar = 0.0;
    const bool on = nl0 < kCols && nl < nc;
    if (on) {
      const double mu = mu_s[nl] + c;
      const double vraw = var_s[nl];
      const double var = vraw < min_variance ? min_variance : vraw;
      const double sd = sqrt(2.0 * var);
      const double y = n0 + nl < f.M1 ? -1.0 : 1.0;  // train_y (see quadrature)
      const double t = c_gh_t[q], w = c_gh_w[q];
      gh_pair(y, mu, sd, t, w, want_e, &E, &dmu, &dvar);
    }
    sred[threadIdx.x] = E;
    sred[NT + threadIdx.x] = dmu;
    sred[2 * NT + threadIdx.x] = dvar;
    __syncthreads();
    if (on && q == 0) {
      double se = 0.0, sm = 0.0, sv = 0.0;
      for (int qq = 0; qq < 10; ++qq) {
        se += sred[threadIdx.x + qq];
        sm += sred[NT + threadIdx.x + qq];
        sv += sred[2 * NT + threadIdx.x + qq];
      }
      const double ipi = 0.56418958354775628695;  // 1/sqrt(pi)
      const double vraw = var_s[nl];
      const bool clamped = vraw < min_variance;
      const double var = clamped ? min_variance : vraw;
      const double y = n0 + nl < f.M1 ? -1.0 : 1.0;  // train_y (see quadrature)
      const double g1 = -(ipi * sm * y) / Nd;
      const double g2 = clamped ? 0.0 : -(ipi * sv * y / sqrt(2.0 * var)) / Nd;
      gmu_s[nl] = g1;
      gv_s[nl] = g2;
      e_add += ipi * se;
      gc_add += g1;
      gv_add += g2;
    }
    if (kCols < SW) __syncthreads();  // another pass may follow and reuses sred
  }
  if ((int)threadIdx.x >= nc && threadIdx.x < SW) {
    gmu_s[threadIdx.x] = 0.0;
    gv_s[threadIdx.x] = 0.0;
  }
  out3[0] = e_add;
  out3[1] = gc_add;
  out3[2] = gv_add;
  __syncthreads();
}
#endif

#if GAPRO_NT >= 320
// Adam on LS for the wave's lower tiles in straight-line code (see the comment at its twin inside the kernel, used by
// the 256-thread build): a function of its own so that its registers (a tile in flight, a tile being updated, the
// division and square-root sequences) are allocated apart from the strip loop, whose accumulator tiles arrive here
// by value.  R = rounds of the workgroup; a slot past the wave's last tile works on the wave's first tile with
// its stores redirected to the B slot of the workspace, which this kernel never uses (its B lives in LDS).
template <int R>
__device__ __noinline__ void adam_ls_tiles(d4 g0, d4 g1, d4 g2, d4 g3, d4 g4, double Nd, double step_size, double bc2s,
                                           ldsd* tile) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp, M = f.M, nbk = Mp / 16, nt_acc = nbk * (nbk + 1) / 2;
  gd* LS = f.mat[B_LS];
  gd* LST = f.mat[B_LST];
  gd* MLS = f.mat[B_MLS];
  gd* VLS = f.mat[B_VLS];
  gd* Pm = f.mat[B_BM];  // the dead buffer
  const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  const double b1 = 0.9, b2 = 0.999, aeps = 1e-8;
  const d4 gls[5] = {g0, g1, g2, g3, g4};
  double lsv[4], m1v[4], m2v[4], lsn[4], m1n[4], m2n[4];
  auto slot_tile = [&](int q, int* ti, int* tj) {
    const int t = wave + NW * q;
    const bool valid = t < nt_acc;
    lower_tile(valid ? t : wave, ti, tj);
    return valid;
  };
  auto load_tile = [&](int q, double (&l)[4], double (&a1)[4], double (&a2)[4]) {
    int ti, tj;
    slot_tile(q, &ti, &tj);
    const int j = 16 * tj + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t o = (size_t)(16 * ti + lq + 4 * r) * Mp + j;
      l[r] = LS[o];
      a1[r] = MLS[o];
      a2[r] = VLS[o];
    }
  };
  load_tile(0, lsv, m1v, m2v);
#pragma unroll
  for (int q = 0; q < R; ++q) {
    if (q + 1 < R) load_tile(q + 1, lsn, m1n, m2n);
    int ti, tj;
    const bool valid = slot_tile(q, &ti, &tj);
    gd* wLS = uni_ptr(valid ? LS : Pm);
    gd* wMLS = uni_ptr(valid ? MLS : Pm);
    gd* wVLS = uni_ptr(valid ? VLS : Pm);
    gd* wLST = uni_ptr(valid ? LST : Pm);
    const int j = 16 * tj + lr;
    d4 newv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * ti + lq + 4 * r;
      const size_t o = (size_t)i * Mp + j;
      const bool act = j <= i && i < M;
      const double l = act ? lsv[r] : 1.0;
      const double g = gls[q][r] + (l - (i == j ? 1.0 / l : 0.0)) / Nd;
      const double m1 = b1 * m1v[r] + (1.0 - b1) * g;
      const double m2 = b2 * m2v[r] + (1.0 - b2) * g * g;
      const double lnew = l - step_size * m1 / (sqrt(m2) / bc2s + aeps);
      wMLS[o] = act ? m1 : m1v[r];
      wVLS[o] = act ? m2 : m2v[r];
      wLS[o] = act ? lnew : lsv[r];
      newv[r] = act ? lnew : 0.0;
    }
    store_tile(newv, nullptr, wLST, Mp, 16 * ti, 16 * tj, tile);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lsv[r] = lsn[r];
      m1v[r] = m1n[r];
      m2v[r] = m2n[r];
    }
  }
}
#endif

// Kernel gradients through KX, fused into the strip loop (round 5; narrow features): while G_KX[:, n0 .. n0 + 32) is in
// LDS, W_zx = G_KX o KX is formed element by element (kernel value recomputed from the staged points, as the gradient
// pass after the loop did) and summed into per-row accumulators zacc[k][0..5] = sum_n W[k][n] (Z_k - X_n),
// [6] = sum_n G_KX E, [7] = sum_n W d2.  Four adjacent lanes share a row (eight columns each) and are combined by two
// DPP hops.  Before: the strip was stored as G_KX^T rows to the workspace (7 % of a step) and read back by the
// gradient pass, whose zx half was another ~4 % of memory round trips.
template <int DC>
__device__ __noinline__ void strip_kgrad_zx(const ldsd* Gs, const ldsd* Zt, const ldsd* Xpts, ldsd* zacc, int n0, int nc,
                                            double s, double inv_l2) {
  const Fit& f = g_sh.f;
  const int Mp = f.Mp, M = f.M;
  constexpr int D = DC;
  const int row = threadIdx.x >> 2, cg = threadIdx.x & 3;
  double acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.0;
  double gs = 0.0, gl = 0.0;
  if (row < M) {
    double zk[D];
#pragma unroll
    for (int d = 0; d < D; ++d) zk[d] = Zt[d * Mp + row];
#pragma unroll 2
    for (int j = 0; j < SW / 4; ++j) {
      const int n = cg * (SW / 4) + j;
      if (n < nc) {
        double t[D];
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          t[d] = zk[d] - Xpts[d * Mp + n0 + n];
          d2 += t[d] * t[d];
        }
        const double e = gapro_fit_math::rbf_exp(-0.5 * inv_l2 * d2);
        const double g = Gs[row * RS + n];
        const double wx = g * s * e;
        gs += g * e;
        gl += wx * d2;
#pragma unroll
        for (int d = 0; d < D; ++d) acc[d] += wx * t[d];
      }
    }
  }
  using gapro_fit_math::dpp_mov;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    acc[d] += dpp_mov<0xB1>(acc[d]);  // quad_perm(1, 0, 3, 2)
    acc[d] += dpp_mov<0x4E>(acc[d]);  // quad_perm(2, 3, 0, 1)
  }
  gs += dpp_mov<0xB1>(gs);
  gs += dpp_mov<0x4E>(gs);
  gl += dpp_mov<0xB1>(gl);
  gl += dpp_mov<0x4E>(gl);
  if (cg == 0 && row < M) {
    ldsd* z = zacc + row * 8;
#pragma unroll
    for (int d = 0; d < D; ++d) z[d] += acc[d];
    z[6] += gs;
    z[7] += gl;
  }
}

template <int DMAX, int DC>
__device__ void fit_body_strip(const gapro_fit_options& opt, ldsd* Zt, ldsd* Pt, ldsd* region,
                               const gapro_fit_desc& desc, float* __restrict__ o_probs,
                               float* __restrict__ o_probs_new, unsigned char* __restrict__ o_labels,
                               float* __restrict__ o_mu, float* __restrict__ o_var, double* loss_out) {
  const Fit& f = g_sh.f;
  Shared& sh = g_sh;
  const int M = f.M, Mp = f.Mp, D = DC ? DC : f.D, T = f.T;
  const int nbk = Mp / 16, nt_acc = nbk * (nbk + 1) / 2;
  const double Nd = (double)M;
  const double jitter = opt.jitter;
  ldsd* As = region;
  ldsd* Bs = As + Mp * RS;
  ldsd* Cs = Bs + Mp * RS;
  ldsd* scratch = region;  // outside the strip loop the same memory serves Cholesky, tiles and reductions
  ldsd* sred = region + strip_region_doubles(Mp);  // 3 * NT
  ldsd* m_s = sred + 3 * NT;                       // Mp
  ldsd* mu_s = m_s + Mp;                           // SW each
  ldsd* var_s = mu_s + SW;
  ldsd* gmu_s = var_s + SW;
  ldsd* gv_s = gmu_s + SW;
  // narrow features (the reference's xyz + rgb): the zx kernel gradients are summed inside the strip loop
  constexpr bool kFuseKg = DC > 0 && DC <= 6 && !(DMAX > 8);
  ldsd* zacc = gv_s + SW + 32;  // [Mp][8], behind the alignment slack of the vectors
  gd* LS = f.mat[B_LS];
  gd* LST = f.mat[B_LST];
#if GAPRO_NT < 320
  gd* MLS = f.mat[B_MLS];
  gd* VLS = f.mat[B_VLS];
#endif
#if GAPRO_NT < 320
  gd* dead = f.mat[B_BM];   // never read: target of the redirected stores of the straight-line Adam code
#endif
  gd* Pm = f.mat[B_GA];     // Pm^T for the tail products
  gd* T1T = f.mat[B_BMT];
  gd* Gb = f.mat[B_A];
  gd* GTb = f.mat[B_AT];
  gd* GKXT = f.mat[B_GKXT];
  gd* vm = f.vec[V_M];
  const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int lr = lane & 15, lq = lane >> 4;
  ldsd* tile = scratch + wave * 16 * 17;
  double last_loss = 0.0;
  // LDS offsets of this lane's operand rows for the accumulator tiles the wave owns
  int offA[kAccTiles], offB[kAccTiles];
#pragma unroll
  for (int q = 0; q < kAccTiles; ++q) {
    int ti = 0, tj = 0;
    if (wave + NW * q < nt_acc) lower_tile(wave + NW * q, &ti, &tj);
    offA[q] = (16 * ti + lr) * RS + lq;
    offB[q] = (16 * tj + lr) * RS + lq;
  }
#ifdef GAPRO_PROFILE
  auto stamp = [&](int id) { prof_stamp(id); };
#else
  auto stamp = [&](int) {};
#endif
  auto refresh_hypers = [&]() {
    __syncthreads();
    if (threadIdx.x == 0) {
      sh.s = softplus(sh.rho_s);
      sh.ell = softplus(sh.rho_l);
      sh.inv_l2 = 1.0 / (sh.ell * sh.ell);
    }
    __syncthreads();
  };
  auto factorize = [&]() {
    stamp(19);
    cholesky_psd_safe<DC, 1>(Zt, scratch, sh.s, sh.inv_l2, jitter, opt.psd_retries, opt.psd_jitter);
    stamp(1);
    tri_inverse_strip(scratch);
    __syncthreads();
    stamp(2);
  };
  // forward part of one strip: Cs = KX(:, n0..), As = LI Cs, Bs = LS^T As, mu_s / var_s for the strip columns
  auto strip_forward = [&](const ldsd* Xpts, int n0, int nc, double s, double inv_l2) {
    strip_fill_kx<DC>(Cs, Zt, Xpts, n0, nc, s, inv_l2);
    stamp(3);
    strip_gemm<K_LE>(f.mat[B_U], Mp, Cs, nbk, [=](int rb, int ct, const d4& v) {
      const int ln = threadIdx.x & 63, c = ln & 15, g4 = ln >> 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) As[(16 * rb + g4 + 4 * r) * RS + 16 * ct + c] = v[r];
    });
    __syncthreads();
    stamp(4);
    strip_gemm<K_GE>(LS, Mp, As, nbk, [=](int rb, int ct, const d4& v) {
      const int ln = threadIdx.x & 63, c = ln & 15, g4 = ln >> 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) Bs[(16 * rb + g4 + 4 * r) * RS + 16 * ct + c] = v[r];
    });
    __syncthreads();
    stamp(7);
    strip_mean_var(As, Bs, m_s, sred, mu_s, var_s, s, jitter);
    stamp(9);
  };

  for (int step = 1; step <= opt.training_iter; ++step) {
    refresh_hypers();
    const double s = sh.s, ell = sh.ell, inv_l2 = sh.inv_l2, c = sh.c;
    const bool last = step == opt.training_iter;
    factorize();
    for (int i = threadIdx.x; i < Mp; i += NT) m_s[i] = vm[i];
    if (kFuseKg)
      for (int i = threadIdx.x; i < 8 * Mp; i += NT) zacc[i] = 0.0;
    d4 gls[kAccTiles], gl[kAccTiles];
#pragma unroll
    for (int q = 0; q < kAccTiles; ++q) {
      gls[q] = (d4){0.0, 0.0, 0.0, 0.0};
      gl[q] = (d4){0.0, 0.0, 0.0, 0.0};
    }
    double gm_acc = 0.0, e_tot = 0.0, gc_part = 0.0, gvs_part = 0.0;
    __syncthreads();
    stamp(3);

    for (int n0 = 0; n0 < M; n0 += SW) {
      const int nc = (M - n0) < SW ? (M - n0) : SW;
      strip_forward(Pt, n0, nc, s, inv_l2);
      // ---- likelihood gradients of the strip columns
      {
        double part[3];
        strip_likelihood(mu_s, var_s, gmu_s, gv_s, sred, n0, nc, c, opt.min_variance, Nd, last, part);
        e_tot += part[0];
        gc_part += part[1];
        gvs_part += part[2];
      }
      stamp(10);
      // ---- G_LS += A GB^T (register tiles), G_m += A g_mu
      double sc2[SW / 4];
#pragma unroll
      for (int ks = 0; ks < SW / 4; ++ks) sc2[ks] = 2.0 * gv_s[4 * ks + lq];
#pragma unroll
      for (int q = 0; q < kAccTiles; ++q) {
        const int t = wave + NW * q;
        if (t < nt_acc) {
          const ldsd* pa = As + offA[q];
          const ldsd* pb = Bs + offB[q];
          // GB = 2 B diag(g_v) is never materialised: the factor rides on the A operand (k index = n)
#pragma unroll
          for (int ks = 0; ks < SW / 4; ++ks)
            gls[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * ks] * sc2[ks], pb[4 * ks], gls[q], 0, 0, 0);
        }
      }
      if (threadIdx.x < Mp) {
        const ldsd* pa = As + threadIdx.x * RS;
        for (int n = 0; n < SW; ++n) gm_acc += pa[n] * gmu_s[n];
      }
      stamp(11);
      // ---- G_A strip -> Cs:  m g_mu^T + LS GB - 2 A diag(g_v)     (LS[i][j] = LST[j][i], j <= i)
      strip_gemm<K_LE>(LST, Mp, Bs, nbk, [=](int rb, int ct, const d4& v) {
        const int ln = threadIdx.x & 63, c = ln & 15, g4 = ln >> 4;
        const int n = 16 * ct + c;
        const double gvn = gv_s[n], gmn = gmu_s[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * rb + g4 + 4 * r;
          Cs[i * RS + n] = 2.0 * gvn * v[r] + m_s[i] * gmn - 2.0 * As[i * RS + n] * gvn;
        }
      });
      __syncthreads();
      stamp(12);
      // ---- G_KX strip -> Bs:  LI^T G_A   (P = LI[k][i], k >= i)
      strip_gemm<K_GE>(f.mat[B_LI], Mp, Cs, nbk, [=](int rb, int ct, const d4& v) {
        const int ln = threadIdx.x & 63, c = ln & 15, g4 = ln >> 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) Bs[(16 * rb + g4 + 4 * r) * RS + 16 * ct + c] = v[r];
      });
      // ---- L^T G_L -= G_A A^T (register tiles).  The Cholesky backward pass needs Phi(L^T G_L) with
      // G_L = -tril(L^-T G_A A^T); row i of L^T X reads rows k >= i of X only, so the lower triangle of L^T tril(X) is
      // the lower triangle of L^T X = -G_A A^T: no G_L, no product with L^T (the staged kernel has the same identity).
      // Reads the G_A and A strips, not G_KX: no barrier between the G_KX product and this.
#pragma unroll
      for (int q = 0; q < kAccTiles; ++q) {
        const int t = wave + NW * q;
        if (t < nt_acc) {
          const ldsd* pa = Cs + offA[q];
          const ldsd* pb = As + offB[q];
#pragma unroll
          for (int ks = 0; ks < SW / 4; ++ks)
            gl[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[4 * ks], pb[4 * ks], gl[q], 0, 0, 0);
        }
      }
      __syncthreads();
      stamp(15);
      if constexpr (kFuseKg) {
        // ---- kernel gradients through KX while the G_KX strip is on chip (nothing leaves it any more)
        strip_kgrad_zx<DC>(Bs, Zt, Pt, zacc, n0, nc, s, inv_l2);
      } else {
        // ---- G_KX^T rows of the strip -> global (the only intermediate that leaves the chip): the kernel
        // gradient pass after the loop reads G_KX[k][n] as GKXT[n][k], contiguous in k
        for (int idx = threadIdx.x; idx < Mp * nc; idx += NT) {
          const int n = idx / Mp, k = idx - n * Mp;
          GKXT[(size_t)(n0 + n) * Mp + k] = Bs[k * RS + n];
        }
      }
      __syncthreads();
      stamp(18);
    }

    // ---- after the strips: scalars, G_m, ELBO value (last step only)
    const double g_c = block_sum(gc_part);
    const double gv_sum = block_sum(gvs_part);
    if (threadIdx.x < Mp) f.vec[V_GM][threadIdx.x] = gm_acc;
    if (last) {
      const double e_sum = block_sum(e_tot);
      double kl_part = 0.0;
      for (int idx = threadIdx.x; idx < M * M; idx += NT) {
        const int i = idx / M, j = idx - i * M;
        if (j <= i) {
          const double v = LS[(size_t)i * Mp + j];
          kl_part += v * v;
          if (i == j) kl_part -= log(v * v);
        }
      }
      for (int i = threadIdx.x; i < M; i += NT) kl_part += vm[i] * vm[i];
      const double kl = 0.5 * (block_sum(kl_part) - Nd);
      last_loss = -(e_sum / Nd - kl / Nd);
    }
    stamp(6);

    // ---- Adam on LS straight from the register tiles;  G_L tiles -> global for the tail products
    const double b1 = 0.9, b2 = 0.999, aeps = 1e-8;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2s = sqrt(1.0 - pow(b2, (double)step));
    const double step_size = opt.lr / bc1;
#if GAPRO_NT < 320
    // Software-pipelined over the wave's tiles: the loads of tile q+1 are in flight while tile q is updated.  That
    // only works in STRAIGHT-LINE code: s_waitcnt counts memory operations in issue order, and behind any join of
    // two paths (a tile guard, a per-element "if active") the compiler can only wait for vmcnt(0), i.e. for every
    // store of the previous tile to reach memory before the next tile's loads are even consumed.  So: one
    // instantiation per number of rounds (uniform over the workgroup), no guard inside it.  A slot past the wave's
    // last tile runs on the wave's first tile with its stores redirected to a buffer that is dead here (Pm, written
    // in full by the first tail product); inactive elements (upper half of a diagonal tile, padded rows) are loaded
    // and stored back unchanged instead of being skipped.  Bit-identical to the guarded form below.
    auto adam_ls = [&](auto rtag) {
      constexpr int R = decltype(rtag)::value;
      double lsv[4], m1v[4], m2v[4], lsn[4], m1n[4], m2n[4];
      auto slot_tile = [&](int q, int* ti, int* tj) {
        const int t = wave + NW * q;
        const bool valid = t < nt_acc;
        lower_tile(valid ? t : wave, ti, tj);
        return valid;
      };
      auto load_tile = [&](int q, double (&l)[4], double (&a1)[4], double (&a2)[4]) {
        int ti, tj;
        slot_tile(q, &ti, &tj);
        const int j = 16 * tj + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t o = (size_t)(16 * ti + lq + 4 * r) * Mp + j;
          l[r] = LS[o];
          a1[r] = MLS[o];
          a2[r] = VLS[o];
        }
      };
      load_tile(0, lsv, m1v, m2v);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (q + 1 < R) load_tile(q + 1, lsn, m1n, m2n);
        int ti, tj;
        const bool valid = slot_tile(q, &ti, &tj);
        gd* wLS = uni_ptr(valid ? LS : dead);
        gd* wMLS = uni_ptr(valid ? MLS : dead);
        gd* wVLS = uni_ptr(valid ? VLS : dead);
        gd* wPmT = uni_ptr(valid ? Pm : dead);
        gd* wLST = uni_ptr(valid ? LST : dead);
        const int j = 16 * tj + lr;
        d4 newv, pv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * ti + lq + 4 * r;
          const size_t o = (size_t)i * Mp + j;
          const bool act = j <= i && i < M;
          const double l = act ? lsv[r] : 1.0;
          const double g = gls[q][r] + (l - (i == j ? 1.0 / l : 0.0)) / Nd;
          const double m1 = b1 * m1v[r] + (1.0 - b1) * g;
          const double m2 = b2 * m2v[r] + (1.0 - b2) * g * g;
          const double lnew = l - step_size * m1 / (sqrt(m2) / bc2s + aeps);
          wMLS[o] = act ? m1 : m1v[r];
          wVLS[o] = act ? m2 : m2v[r];
          wLS[o] = act ? lnew : lsv[r];
          newv[r] = act ? lnew : 0.0;
          pv[r] = (j < i) ? gl[q][r] : (j == i ? 0.5 * gl[q][r] : 0.0);
        }
        store_tile(newv, nullptr, wLST, Mp, 16 * ti, 16 * tj, tile);
        store_tile(pv, nullptr, wPmT, Mp, 16 * ti, 16 * tj, tile);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          lsv[r] = lsn[r];
          m1v[r] = m1n[r];
          m2v[r] = m2n[r];
        }
      }
    };
    if (wave < nt_acc) {
      switch ((nt_acc + NW - 1) / NW) {  // M_p <= 64 (the small-fit route) with four waves: at most three rounds
        case 1: adam_ls(std::integral_constant<int, 1>()); break;
        case 2: adam_ls(std::integral_constant<int, 2>()); break;
        default: adam_ls(std::integral_constant<int, 3>()); break;
      }
    }
#else
    // 512 threads: the same straight-line code, but as a function of its own (adam_ls_tiles).  Inlined here it makes
    // this phase faster and the strip phases slower (-1..-4 % overall, whatever the instantiation count); as a
    // function it is +3 % fits/s at M = 80, 96 and -0.5..-0.8 % at M = 112, 128 (the stores still in flight delay
    // the first tail product).  Keeping the guarded loop beside it for four and five rounds costs 2..3 % everywhere.
    if (wave < nt_acc) {
      switch ((nt_acc + NW - 1) / NW) {  // 64 < M_p <= 128 with eight waves: two to five rounds
        case 1:
        case 2: adam_ls_tiles<2>(gls[0], gls[1], gls[2], gls[3], gls[4], Nd, step_size, bc2s, tile); break;
        case 3: adam_ls_tiles<3>(gls[0], gls[1], gls[2], gls[3], gls[4], Nd, step_size, bc2s, tile); break;
        case 4: adam_ls_tiles<4>(gls[0], gls[1], gls[2], gls[3], gls[4], Nd, step_size, bc2s, tile); break;
        default: adam_ls_tiles<5>(gls[0], gls[1], gls[2], gls[3], gls[4], Nd, step_size, bc2s, tile); break;
      }
    }
    // Pm^T = Phi(L^T G_L)^T tiles -> global for the tail products
#pragma unroll
    for (int q = 0; q < kAccTiles; ++q) {
      const int t = wave + NW * q;
      if (t < nt_acc) {
        int ti, tj;
        lower_tile(t, &ti, &tj);
        const int j = 16 * tj + lr;
        d4 pv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * ti + lq + 4 * r;
          pv[r] = (j < i) ? gl[q][r] : (j == i ? 0.5 * gl[q][r] : 0.0);
        }
        store_tile(pv, nullptr, Pm, Mp, 16 * ti, 16 * tj, tile);
      }
    }
#endif
    __syncthreads();
    stamp(8);

    // ---- tail: G_Kzz = LI^T Pm LI through global memory, Pm = Phi(L^T G_L) from the register tiles above; two TN
    // products, associated as LI^T (Pm LI): W = Pm LI is lower (M^3 / 3), S = LI^T W costs 2 M^3 / 3
    auto tail = [&](auto tu_tag) {
      constexpr int TU = decltype(tu_tag)::value;
      constexpr int TS = 16 * TU;
      const int mt = Mp / 16;  // gemm_tn's extents: 16 x 16 tiles (TU = 1) or half tiles (TU = 2)
      gd* PmT = Pm;   // Pm^T: the upper and diagonal tiles are written, W reads exactly those
      gd* Wm = T1T;   // W: the lower and diagonal tiles are written, S reads exactly those
      gemm_tn<TU, false, 4>(mt, mt, true, PmT, f.mat[B_LI], Mp, nullptr,
                         [=](int i0, int j0, int* lo, int* hi) { *lo = j0; *hi = i0 + TS < Mp ? i0 + TS : Mp; },
                         [=](int i0, int j0, const d4& v) {
                           const int ln = threadIdx.x & 63, c = ln & 15, g4 = ln >> 4;
#pragma unroll
                           for (int r = 0; r < 4; ++r) {
                             const int i = i0 + g4 + 4 * r, j = j0 + c;
                             Wm[(size_t)i * Mp + j] = (j <= i) ? v[r] : 0.0;
                           }
                         });
      __syncthreads();
      gemm_tn<TU, false, 4, ORD_SHELLS>(mt, mt, false, f.mat[B_LI], Wm, Mp, nullptr,
                         [=](int i0, int j0, int* lo, int* hi) { *lo = i0 > j0 ? i0 : j0; *hi = Mp; },
                         [=](int i, int j, const d4& v) { store_tile(v, Gb, GTb, Mp, i, j, tile); });
      __syncthreads();
    };
    if (Mp >= 64)
      tail(std::integral_constant<int, 2>());
    else
      tail(std::integral_constant<int, 1>());
    stamp(13);
    double g_s, g_l;
    if constexpr (kFuseKg) {
      const double gs_zx = block_sum((int)threadIdx.x < M ? zacc[threadIdx.x * 8 + 6] : 0.0);
      const double gl_zx = block_sum((int)threadIdx.x < M ? zacc[threadIdx.x * 8 + 7] : 0.0);
      kernel_grads_adam_z<DMAX, false, 8, DC>(Zt, Pt, Gb, GTb, GKXT, s, inv_l2, step_size, bc2s, scratch, &g_s, &g_l,
                                              zacc);
      g_s += gs_zx;
      g_l += gl_zx;
    } else {
      kernel_grads_adam_z<DMAX, true, (DMAX <= 8 ? 8 : 2), DC>(Zt, Pt, Gb, GTb, GKXT, s, inv_l2, step_size, bc2s, scratch,
                                                           &g_s, &g_l);
    }
    g_s += gv_sum;
    g_l /= (ell * ell * ell);
    stamp(14);

    auto adam_upd = [&](double p, double& m1, double& m2, double g) {
      m1 = b1 * m1 + (1.0 - b1) * g;
      m2 = b2 * m2 + (1.0 - b2) * g * g;
      return p - step_size * m1 / (sqrt(m2) / bc2s + aeps);
    };
    for (int i = threadIdx.x; i < M; i += NT) {
      const double g = f.vec[V_GM][i] + vm[i] / Nd;
      f.vec[V_GM][i] = g;
      double m1 = f.vec[V_MM][i], m2 = f.vec[V_VM][i];
      vm[i] = adam_upd(vm[i], m1, m2, g);
      f.vec[V_MM][i] = m1;
      f.vec[V_VM][i] = m2;
    }
    if (threadIdx.x == 0) {
      double m1, m2;
      m1 = f.scal[S_MC]; m2 = f.scal[S_VC];
      sh.c = adam_upd(sh.c, m1, m2, g_c);
      f.scal[S_MC] = m1; f.scal[S_VC] = m2;
      m1 = f.scal[S_MRS]; m2 = f.scal[S_VRS];
      sh.rho_s = adam_upd(sh.rho_s, m1, m2, g_s * sigmoid(sh.rho_s));
      f.scal[S_MRS] = m1; f.scal[S_VRS] = m2;
      m1 = f.scal[S_MRL]; m2 = f.scal[S_VRL];
      sh.rho_l = adam_upd(sh.rho_l, m1, m2, g_l * sigmoid(sh.rho_l));
      f.scal[S_MRL] = m1; f.scal[S_VRL] = m2;
    }
    __syncthreads();
    stamp(16);
  }

  // ------------------------------- prediction ------------------------------
  refresh_hypers();
  if (!(opt.eval_stale_chol && opt.training_iter > 0)) factorize();
  const double s = sh.s, inv_l2 = sh.inv_l2, c = sh.c;
  for (int i = threadIdx.x; i < Mp; i += NT) m_s[i] = vm[i];
  for (int t0 = 0; t0 < T; t0 += Mp) {
    const int ncx = (T - t0) < Mp ? (T - t0) : Mp;
    __syncthreads();
    stage_points_t(Pt, f.Xt + (size_t)t0 * D, ncx, D, Mp);
    __syncthreads();
    for (int n0 = 0; n0 < ncx; n0 += SW) {
      const int nc = (ncx - n0) < SW ? (ncx - n0) : SW;
      strip_forward(Pt, n0, nc, s, inv_l2);
      if ((int)threadIdx.x < nc) {
        const int n = threadIdx.x;
        const double mu = mu_s[n] + c;
        const double var = fmax(var_s[n], opt.min_variance);
        const double p = 0.5 * erfc(-(mu / sqrt(1.0 + var)) * 0.70710678118654752440);
        const float pf = (float)p;                       // pred_probs            :432
        const bool lab = pf >= 0.5f;                     // pred_labels           :433
        const long long o = desc.out_offset + t0 + n0 + n;
        o_probs[o] = pf;
        o_probs_new[o] = lab ? pf : 1.0f - pf;           // pred_probs_new        :438
        o_labels[o] = lab ? 1 : 0;
        o_mu[o] = (float)mu;                             // pred_mu               :435
        o_var[o] = (float)var;                           // pred_variance         :436
        if ((!isfinite(mu) || !isfinite(var)) && sh.status == GAPRO_OK) sh.status = GAPRO_ERR_NOT_FINITE;  // first error wins
      }
      __syncthreads();
    }
  }
  stamp(17);
#ifdef GAPRO_PROFILE
  if (threadIdx.x == 0)
{
      for (int i = 0; i < kProfSlots; ++i) f.scal[24 + i] = (double)sh.prof[i];
      unsigned xcc, hwid;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      f.scal[24 + 25] = (double)sh.t_start;  // timeline of the launch: tools/fit_timeline.py
      f.scal[24 + 26] = (double)wall_clock64();
      f.scal[24 + 27] = (double)(((xcc & 15u) << 16) | (hwid & 0xFFFFu));
    }
#endif
  if (threadIdx.x == 0) {
    f.scal[S_C] = sh.c;
    f.scal[S_RS] = sh.rho_s;
    f.scal[S_RL] = sh.rho_l;
    f.scal[S_LOSS] = last_loss;
    *loss_out = last_loss;
  }
}

// one workgroup per CU: the register-resident gradient tiles need the full 256-VGPR budget
template <int DMAX, int DC>
__global__ __launch_bounds__(NT, 2) void k_svgp_fit_strip(int n_fits, int D, const float* __restrict__ feats_spp,
                                                        const int* __restrict__ idx,
                                                        const gapro_fit_desc* __restrict__ descs,
                                                        const double* __restrict__ init_mean, gapro_fit_options opt,
                                                        double* __restrict__ ws, float* __restrict__ o_probs,
                                                        float* __restrict__ o_probs_new,
                                                        unsigned char* __restrict__ o_labels, float* __restrict__ o_mu,
                                                        float* __restrict__ o_var, int* __restrict__ o_status,
                                                        double* __restrict__ o_loss, unsigned* ticket) {
  extern __shared__ double dyn_lds[];
  const int fit = claim_fit(ticket);
  if (fit >= n_fits) return;
  const gapro_fit_desc desc = descs[fit];
  const int Mp = gapro_pad_m(desc.m1 + desc.m2, D);
  ldsd* Zt = (ldsd*)dyn_lds;
  ldsd* Pt = Zt + D * Mp;
  ldsd* region = Pt + D * Mp;
  fit_setup(desc, D, feats_spp, idx, init_mean, ws, Zt, Pt);
  double* loss_slot = &o_loss[desc.slot];
  fit_body_strip<DMAX, DC>(opt, Zt, Pt, region, desc, o_probs, o_probs_new, o_labels, o_mu, o_var, loss_slot);
  fit_epilogue(desc, opt, o_status, o_loss);
}

}  // namespace

// host side: launch of this translation unit's build of the kernel -- gapro_launch_fit_strip (common.h), or the name
// that the including file gives it (svgp_fit_small.hip)
#ifndef GAPRO_LAUNCH_FIT_STRIP
#define GAPRO_LAUNCH_FIT_STRIP gapro_launch_fit_strip
#endif
int GAPRO_LAUNCH_FIT_STRIP(hipStream_t stream, const FitLaunchStep& s, const FitArgs& a) {
  auto kern = a.feat_dim == 6 ? k_svgp_fit_strip<6, 6> : a.feat_dim == 32 ? k_svgp_fit_strip<32, 32> : k_svgp_fit_strip<32, 0>;
  const size_t lds_bytes = (size_t)s.lds_bytes;
  if (lds_bytes > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return GAPRO_ERR_HIP;
  hipLaunchKernelGGL(kern, dim3(s.grid), dim3(NT), lds_bytes, stream, s.count, a.feat_dim, a.d_feats_spp, a.d_idx,
                     a.d_descs + s.first, a.d_init_mean, *a.opt, a.d_workspace, a.d_probs, a.d_probs_new, a.d_labels,
                     a.d_mu, a.d_var, a.d_fit_status, a.d_fit_loss, gapro_fit_ticket(s, a));
  return hipGetLastError() == hipSuccess ? GAPRO_OK : GAPRO_ERR_HIP;
}
