// The LDS-staged single-workgroup fit kernel k_svgp_fit<WPS, KMIN> (128 < M_p <= 512, 512 threads per fit): Z and X
// staged in LDS, every M_p x M_p matrix in the fit's global-memory workspace (the per-step outline: fit_wg.h).  Built
// by svgp_fit_wg.hip, beside the strip kernel.
#pragma once
#include "fit_wg.h"

namespace {

// WG: 0 = one tile per wave (gemm_tn), 2 / 4 = workgroup-tiled products with that many register stages (gemm_wg)
// KMIN: the products that contract over the columns of A, B, G_A and Pm read those matrices as they are (gemm_tn's PK /
// QK forms) and no transposed copy of them is written -- the build for M_p <= 256, where two workgroups share a CU and a
// launch of such fits sits on the HBM roof: 160: +4 .. 8 %, 256: +5 .. 7 % fits/s.  Those loads touch 16 half cache
// lines per instruction where the k-major form touches 4 whole ones, and the lower-triangular products are 25 .. 30 %
// slower with them; with one workgroup per CU (M_p >= 288) that costs what the copies cost (320: -1 %, 384: -3 %,
// 448: +2 %), so the larger fits keep the copies.
template <int TU, int DMAX, int DC, int WG = 0, bool KMIN = false, int EG = 4>
__device__ void fit_body(const gapro_fit_options& opt, ldsd* Zt, ldsd* Pt, ldsd* scratch, const gapro_fit_desc& desc, float* __restrict__ o_probs, float* __restrict__ o_probs_new,
                         unsigned char* __restrict__ o_labels, float* __restrict__ o_mu, float* __restrict__ o_var,
                         double* loss_out) {
  const Fit& f = g_sh.f;
  Shared& sh = g_sh;
  const int M = f.M, Mp = f.Mp, D = DC ? DC : f.D, T = f.T;
  constexpr int TS = 16 * TU;
  constexpr int TSB = TU >= 2 ? 8 * TU : TS;  // unit of gemm_tn's extents (TU >= 2: half tiles, see there)
  const int mt = Mp / TSB;
  const double Nd = (double)M;  // num_data = train_y.numel() (gaussian_process_utils.py:414)
  const double jitter = opt.jitter;
  gd* LS = f.mat[B_LS];
  gd* LST = f.mat[B_LST];
  gd* MLS = f.mat[B_MLS];
  gd* VLS = f.mat[B_VLS];
  gd* A = f.mat[B_A];
  gd* AT = KMIN ? nullptr : f.mat[B_AT];
  gd* BM = f.mat[B_BM];
  gd* BMT = f.mat[B_BMT];  // !KMIN only
  gd* GA = f.mat[B_GA];
  gd* GKXT = f.mat[B_GKXT];
  gd* GAT = KMIN ? nullptr : GKXT;  // !KMIN: G_A^T lives in the G_KX^T slot until G_KX is formed
  gd* vm = f.vec[V_M];
  gd* gmu = f.vec[V_GMU];
  gd* gv = f.vec[V_GV];
  // per-wave transpose tile; with the workgroup-tiled products the operand ring starts the scratch and the tiles alias
  // its second stage (gemm_wg: no stage is live while epilogues run, and a barrier precedes the next use of that stage)
  ldsd* ring = scratch;
  ldsd* tile = scratch + (WG ? kWgStage : 0) + (threadIdx.x >> 6) * 16 * 17;
  static_assert(WG == 0 || TU == 1, "workgroup-tiled products take their extents and ranges per 16 x 16 block");
  double last_loss = 0.0;
#ifdef GAPRO_PROFILE
  // diagnostic build only: per-phase wall-clock shares (100 MHz ticks), see tools/bench_fit.py --profile
  auto stamp = [&](int id) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long t = wall_clock64();
      sh.prof[id] += t - sh.t_last;
      sh.t_last = t;
    }
  };
#else
  auto stamp = [&](int) {};
#endif
  // between the products of the merged backward phase: nothing in the product build; the diagnostic build either keeps
  // the per-product stamps (and with them the barriers: GAPRO_PROFILE_SPLIT) or charges the whole phase to slot 10
#if defined(GAPRO_PROFILE) && defined(GAPRO_PROFILE_SPLIT)
#define STAMP_MERGED(id) do { __syncthreads(); stamp(id); } while (0)
#else
  // merged only in the KMIN instantiations (M_p <= 256).  Beyond, G_A^T lives in the G_KX^T slot until G_KX^T is formed
  // (GAT below), so Pm -- which reads it -- must be complete before G_KX^T starts; and with one workgroup per CU and
  // 64 x 64 tiles the merge measured +-0 there anyway.
#define STAMP_MERGED(id) do { if constexpr (!KMIN) __syncthreads(); } while (0)
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
    // The register look-ahead (next column's tiles built while wave 0 factors the diagonal block) beyond M_p = 256:
    // one workgroup per CU there, nobody else fills the CU while seven waves wait for the diagonal block (512 fits:
    // M = 320 -1.9 %, 384 -1.6 %, 448 -1.0 % in time, bit-identical).  Up to 256 two workgroups share a CU and hide
    // each other's serial stretches: 160 +-0, 200 +1.3 %, 256 +1 % -- not used there.
    cholesky_psd_safe<DC, KMIN ? 0 : 3>(Zt, scratch, sh.s, sh.inv_l2, jitter, opt.psd_retries, opt.psd_jitter);
    stamp(1);
    if (Mp <= 128)
      tri_inverse<8>(scratch);
    else
      tri_inverse<0>(scratch);
    __syncthreads();
    stamp(2);
  };
  // Column sums fused into the GEMM epilogues: every 16x16 result tile leaves the partial sum of its 16 rows per
  // column in part_x[tile_row][column]; summed later in tile order.  The partials live in LDS up to M_p = kFuseMaxMp
  // and beyond it in the G_A slot of the workspace (free until the backward pass; 3/16 of a matrix): a separate pass
  // over A and B (mean_var: two more matrix reads per step, 3 % of a step at M = 257 .. 464) is not needed.
  const bool fuse = Mp <= kFuseMaxMp;
  ldsd* part_m = scratch + kTileDoubles;       // sum_i m[i] A[i][n]   (later reused for G_m partials)
  ldsd* part_a = part_m + (Mp / 16) * Mp;      // sum_i A[i][n]^2
  ldsd* part_b = part_a + (Mp / 16) * Mp;      // sum_j B[j][n]^2
  gd* gpart_m = f.mat[B_GA];
  gd* gpart_a = gpart_m + (size_t)(Mp / 16) * Mp;
  gd* gpart_b = gpart_a + (size_t)(Mp / 16) * Mp;
  // A = LI * KX and B = LS^T A over ncols columns (row-major only: the products that contract over the columns of A
  // and B read them with the contraction index along the rows, gemm_tn's PK / QK forms); then mu (without c) and var
  auto forward_products = [&](int ncols, double s_, double jitter_) {
    const int nt = (ncols + TSB - 1) / TSB;
    // A[i][n] = sum_k U[k][i] KX[k][n],  U[k][i] = LI[i][k] = 0 for k > i
    product<WG, TU, false, ORD_ROWS_DESC>(mt, nt, false, f.mat[B_U], f.mat[B_KX], Mp, nullptr,
                       [=](int i0, int, int* lo, int* hi) { *lo = 0; *hi = i0 + TS; },
                       [=](int i, int n, const d4& v) {
                         if constexpr (KMIN) store_tile(v, A, nullptr, Mp, i, n, tile);
                         else store_tile(v, A, AT, Mp, i, n, tile);
                         {
                           const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
                           double pm = 0.0, pa = 0.0;
#pragma unroll
                           for (int r = 0; r < 4; ++r) {
                             pm += vm[i + lq + 4 * r] * v[r];
                             pa += v[r] * v[r];
                           }
                           pm += __shfl_xor(pm, 16, 64);
                           pa += __shfl_xor(pa, 16, 64);
                           pm += __shfl_xor(pm, 32, 64);
                           pa += __shfl_xor(pa, 32, 64);
                           if (lq == 0) {
                             if (fuse) {
                               part_m[(i >> 4) * Mp + n + lr] = pm;
                               part_a[(i >> 4) * Mp + n + lr] = pa;
                             } else {
                               gpart_m[(size_t)(i >> 4) * Mp + n + lr] = pm;
                               gpart_a[(size_t)(i >> 4) * Mp + n + lr] = pa;
                             }
                           }
                         }
                       }, ring);
    __syncthreads();
    if constexpr (KMIN) {
    // B[j][n] = sum_i LS[i][j] A[i][n],  LS[i][j] = 0 for i < j
    product<WG, TU, false, ORD_ROWMAJOR>(mt, nt, false, LS, A, Mp, nullptr,
                       [=](int j0, int, int* lo, int* hi) { *lo = j0; *hi = Mp; },
                       [=](int j, int n, const d4& v) {
                         store_tile(v, BM, nullptr, Mp, j, n, tile);
                         {
                           const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
                           double pb = 0.0;
#pragma unroll
                           for (int r = 0; r < 4; ++r) pb += v[r] * v[r];
                           pb += __shfl_xor(pb, 16, 64);
                           pb += __shfl_xor(pb, 32, 64);
                           if (lq == 0) {
                             if (fuse) part_b[(j >> 4) * Mp + n + lr] = pb;
                             else gpart_b[(size_t)(j >> 4) * Mp + n + lr] = pb;
                           }
                         }
                       }, ring);
    } else {
    // BMT[n][j] = sum_i A[i][n] LS[i][j],  LS[i][j] = 0 for i < j
    product<WG, TU, false, ORD_COLMAJOR>(nt, mt, false, A, LS, Mp, nullptr,
                       [=](int, int j0, int* lo, int* hi) { *lo = j0; *hi = Mp; },
                       [=](int n, int j, const d4& v) {
                         store_tile(v, BMT, BM, Mp, n, j, tile);
                         {
                           const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
#pragma unroll
                           for (int r = 0; r < 4; ++r) {
                             double pb = v[r] * v[r];
                             pb += __shfl_xor(pb, 1, 64);
                             pb += __shfl_xor(pb, 2, 64);
                             pb += __shfl_xor(pb, 4, 64);
                             pb += __shfl_xor(pb, 8, 64);
                             if (lr == 0) {
                               if (fuse) part_b[(j >> 4) * Mp + n + lq + 4 * r] = pb;
                               else gpart_b[(size_t)(j >> 4) * Mp + n + lq + 4 * r] = pb;
                             }
                           }
                         }
                       }, ring);
    }
    __syncthreads();
    for (int n = threadIdx.x; n < nt * TSB; n += NT) {
      double sm = 0.0, sa = 0.0, sb = 0.0;
      if (fuse) {
        for (int tq = 0; tq < Mp / 16; ++tq) {
          sm += part_m[tq * Mp + n];
          sa += part_a[tq * Mp + n];
          sb += part_b[tq * Mp + n];
        }
      } else {
        for (int tq = 0; tq < Mp / 16; ++tq) {
          sm += gpart_m[(size_t)tq * Mp + n];
          sa += gpart_a[(size_t)tq * Mp + n];
          sb += gpart_b[(size_t)tq * Mp + n];
        }
      }
      f.vec[V_MU][n] = sm;
      f.vec[V_VAR][n] = s_ + jitter_ + (sb - sa);
    }
    __syncthreads();
  };

  // one Adam step as ONE out-of-line function with the products inlined into it: the callee-saved registers are saved
  // once per step instead of once per product call (see gemm_tn_in)
  auto step_fn = [&](int step) __attribute__((noinline)) {
    refresh_hypers();
    const double s = sh.s, ell = sh.ell, inv_l2 = sh.inv_l2, c = sh.c;
    const bool last = step == opt.training_iter;
    // ------------------------------- forward -------------------------------
    factorize();
    build_kx<DC>(Zt, Pt, M, s, inv_l2);
    __syncthreads();
    stamp(3);
    forward_products(M, s, jitter);
    stamp(4);
    double g_c, gv_sum;
    const double e_sum = quadrature(c, opt.min_variance, Nd, last, scratch, &g_c, &gv_sum);
    if (last) {  // the ELBO value is only reported, never used by the optimiser
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

    // ------------------------------- backward ------------------------------
    const double b1 = 0.9, b2 = 0.999, aeps = 1e-8;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2s = sqrt(1.0 - pow(b2, (double)step));
    const double step_size = opt.lr / bc1;
    // G_m = A g_mu (+ m / N, added with the Adam update below): fused into the G_A epilogue; the partials of the
    // 16-column tiles go to LDS, or beyond M_p = kFuseMaxMp to the G_KX slot (written two phases later)
    gd* gpart_g = f.mat[B_GKX];
    // G_A[i][n] = 2 g_v[n] sum_j LS[i][j] BM[j][n] + m[i] g_mu[n] - 2 A[i][n] g_v[n]
    // (two-phase epilogue: the loads of A, m, g_mu, g_v for a group of blocks are issued together, see two_phase_epi)
    struct GaPre { double a[4], m[4], gvn, gmn; };
    product<WG, TU, false, ORD_ROWS_DESC>(mt, mt, false, LST, BM, Mp, nullptr,
                       [=](int i0, int, int* lo, int* hi) { *lo = 0; *hi = i0 + TS; },
                       two_phase_epi<EG>(
                       [=](int i0, int n0) {
                         const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
                         const int n = n0 + lr;
                         GaPre p;
                         p.gvn = gv[n];
                         p.gmn = gmu[n];
#pragma unroll
                         for (int r = 0; r < 4; ++r) {
                           const int i = i0 + lq + 4 * r;
                           p.a[r] = A[(size_t)i * Mp + n];
                           p.m[r] = vm[i];
                         }
                         return p;
                       },
                       [=](int i0, int n0, const d4& v, const GaPre& p) {
                         const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
                         const int n = n0 + lr;
                         const double gvn = p.gvn, gmn = p.gmn;
                         d4 ga;
#pragma unroll
                         for (int r = 0; r < 4; ++r) {
                           const int i = i0 + lq + 4 * r;
                           const double a = p.a[r];
                           ga[r] = 2.0 * gvn * v[r] + p.m[r] * gmn - 2.0 * a * gvn;
                           if constexpr (KMIN) GA[(size_t)i * Mp + n] = ga[r];
                           double pg = a * gmn;
                           pg += __shfl_xor(pg, 1, 64);
                           pg += __shfl_xor(pg, 2, 64);
                           pg += __shfl_xor(pg, 4, 64);
                           pg += __shfl_xor(pg, 8, 64);
                           if (lr == 0) {
                             if (fuse) part_m[(n0 >> 4) * Mp + i] = pg;
                             else gpart_g[(size_t)(n0 >> 4) * Mp + i] = pg;
                           }
                         }
                         if constexpr (!KMIN) store_tile(ga, GA, GAT, Mp, i0, n0, tile);
                       }), ring);
    __syncthreads();
    for (int i = threadIdx.x; i < Mp; i += NT) {
      double sg = 0.0;
      if (fuse) {
        for (int tq = 0; tq < Mp / 16; ++tq) sg += part_m[tq * Mp + i];
      } else {
        for (int tq = 0; tq < Mp / 16; ++tq) sg += gpart_g[(size_t)tq * Mp + i];
      }
      f.vec[V_GM][i] = sg;
    }
    __syncthreads();
    stamp(7);
    // G_LS[i][j] = sum_n A[i][n] 2 g_v[n] BM[j][n] (lower) + KL', Adam on LS fused in the epilogue
    struct LsPre { double l[4], m1[4], m2[4]; };
    auto gls_epi = two_phase_epi<EG>(
                      [=](int i0, int j0) {
                        const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
                        const int j = j0 + lr;
                        LsPre p;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {  // unconditional: every (i, j) of a tile lies inside the M_p x M_p slots
                          const size_t o = (size_t)(i0 + lq + 4 * r) * Mp + j;
                          p.l[r] = LS[o];
                          p.m1[r] = MLS[o];
                          p.m2[r] = VLS[o];
                        }
                        return p;
                      },
                      [=](int i0, int j0, const d4& v, const LsPre& p) {
                        const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
                        const int j = j0 + lr;
                        d4 newv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                          const int i = i0 + lq + 4 * r;
                          const size_t o = (size_t)i * Mp + j;
                          double lnew = 0.0;
                          if (j <= i && i < M) {
                            const double l = p.l[r];
                            const double g = 2.0 * v[r] + (l - (i == j ? 1.0 / l : 0.0)) / Nd;
                            const double m1 = b1 * p.m1[r] + (1.0 - b1) * g;
                            const double m2 = b2 * p.m2[r] + (1.0 - b2) * g * g;
                            MLS[o] = m1;
                            VLS[o] = m2;
                            lnew = l - step_size * m1 / (sqrt(m2) / bc2s + aeps);
                            LS[o] = lnew;
                          }
                          newv[r] = lnew;
                        }
                        store_tile(newv, nullptr, LST, Mp, i0, j0, tile);  // LST[j][i]; zeros above the diagonal
                      });
    auto gls_range = [=](int, int, int* lo, int* hi) { *lo = 0; *hi = Mp; };
    if constexpr (KMIN)  // A and B as they are: both with the contraction index n along their rows
      product<WG, TU, true, ORD_ROWMAJOR, 1, 1>(mt, mt, true, A, BM, Mp, gv, gls_range, gls_epi, ring);
    else
      product<WG, TU, true, ORD_ROWMAJOR>(mt, mt, true, AT, BMT, Mp, gv, gls_range, gls_epi, ring);
    // (round 4) no barrier here, nor after Pm: G_LS, Pm and G_KX^T all read A, B, G_A, LI as the G_A phase left them
    // and write disjoint matrices (Pm now goes to the L slot, which no single-workgroup MFMA kernel writes since
    // round 3, instead of the B buffer G_LS is still reading), so a wave that has finished its G_LS tiles goes straight
    // on to its Pm and G_KX^T tiles.  Three barrier-separated phases whose tiles do not divide evenly among eight waves
    // (36 lower 32 x 32 tiles at M_p = 256: 4.5 rounds, the slowest wave sets the pace of each) become ONE phase of
    // 36 + 36 + 64 tiles, with the heavy Adam epilogue of G_LS under other waves' MFMAs.  Same tiles, same k order:
    // the bits do not change.
    STAMP_MERGED(8);
    // The Cholesky backward pass needs Pm = Phi(L^T G_L) with G_L = -tril(L^-T G_A A^T) = -tril(G_KX A^T).  Row i of
    // L^T X only reads rows k >= i of X, so the lower triangle of L^T tril(X) is the lower triangle of L^T X, and with
    // X = -L^-T G_A A^T:   Pm = Phi(-G_A A^T)   -- no G_L, no product with L^T (rounds 1-2 and the first half of round 3
    // formed G_L and L^T G_L: 1.33 M^3 where this is 1.0 M^3, one phase and one matrix write more).
    // -> B buffer (dead after G_LS).  KMIN: Pm as it is, from G_A and A as they are (contraction index n along their
    // rows); otherwise Pm^T (the k-major P operand of W: Pm^T[k][i] = Pm[i][k], non-zero for k <= i) from G_A^T and A^T
    gd* Pm = f.mat[B_L];
    auto pm_range = [=](int, int, int* lo, int* hi) { *lo = 0; *hi = Mp; };
    if constexpr (KMIN) {
      product<WG, TU, false, ORD_ROWMAJOR, 1, 1>(mt, mt, true, GA, A, Mp, nullptr, pm_range,
                       [=](int i0, int j0, const d4& v) {
                         const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
#pragma unroll
                         for (int r = 0; r < 4; ++r) {
                           const int i = i0 + lq + 4 * r, j = j0 + lr;
                           Pm[(size_t)i * Mp + j] = (j < i) ? -v[r] : (j == i ? -0.5 * v[r] : 0.0);
                         }
                       }, ring);
    } else {
      product<WG, TU, false, ORD_ROWMAJOR>(mt, mt, true, GAT, AT, Mp, nullptr, pm_range,
                       [=](int i0, int j0, const d4& v) {
                         const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
                         d4 pv;
#pragma unroll
                         for (int r = 0; r < 4; ++r) {
                           const int i = i0 + lq + 4 * r, j = j0 + lr;
                           pv[r] = (j < i) ? -v[r] : (j == i ? -0.5 * v[r] : 0.0);
                         }
                         store_tile(pv, nullptr, Pm, Mp, i0, j0, tile);
                       }, ring);
    }
    STAMP_MERGED(9);
    // G_KX^T = G_A^T LI (only the transposed form is used: kernel gradients); formed as the product whose
    // output IS the transposed matrix, so that the epilogue is plain row stores   (Q = LI[k][i], non-zero for k >= i)
    product<WG, TU, false, ORD_COLMAJOR>(mt, mt, false, GA, f.mat[B_LI], Mp, nullptr,
                       [=](int, int i0, int* lo, int* hi) { *lo = i0; *hi = Mp; },
                       [=](int n, int i, const d4& v) { store_tile(v, GKXT, nullptr, Mp, n, i, tile); }, ring);
    __syncthreads();
    stamp(10);
    // G_Kzz (unsymmetrised) = L^-T Pm L^-1, associated as L^-T (Pm L^-1) (round 3): W = Pm L^-1 is a product of two
    // lower-triangular matrices (M^3 / 3, lower-triangular itself), S = L^-T W then costs 2 M^3 / 3 -- 1.0 M^3 where
    // (L^-T Pm) L^-1, rounds 1-2's order, spends 2/3 + 1.  Same value in exact arithmetic; the rounding differs at 1e-16.
    stamp(11);
    // W = Pm L^-1 (lower) -> the G_LS slot, which nothing else writes in this kernel: its upper blocks ARE zero, as the
    // hulls of S's ranges assume   (j0 <= k < i0 + tile: Pm^T[k][i] = 0 for k > i, L^-1[k][j] = 0 for k < j)
    gd* Wm = f.mat[B_GLS];
    auto w_epi = [=](int i0, int j0, const d4& v) {
                         const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
#pragma unroll
                         for (int r = 0; r < 4; ++r) {
                           const int i = i0 + lq + 4 * r, j = j0 + lr;
                           Wm[(size_t)i * Mp + j] = (j <= i) ? v[r] : 0.0;
                         }
                       };
    auto w_range = [=](int i0, int j0, int* lo, int* hi) { *lo = j0; *hi = i0 + TS; };
    if constexpr (KMIN)
      product<WG, TU, false, ORD_ROWMAJOR, 1, 0>(mt, mt, true, Pm, f.mat[B_LI], Mp, nullptr, w_range, w_epi, ring);
    else
      product<WG, TU, false, ORD_ROWMAJOR>(mt, mt, true, Pm, f.mat[B_LI], Mp, nullptr, w_range, w_epi, ring);
    __syncthreads();
    stamp(12);
    // S = L^-T W -> G in the BM buffer, G^T in the A buffer   (k >= max(i0, j0))
    gd* G = BM;
    gd* GT = A;
    product<WG, TU, false, ORD_SHELLS>(mt, mt, false, f.mat[B_LI], Wm, Mp, nullptr,
                       [=](int i0, int j0, int* lo, int* hi) { *lo = i0 > j0 ? i0 : j0; *hi = Mp; },
                       [=](int i, int j, const d4& v) { store_tile(v, G, GT, Mp, i, j, tile); }, ring);
    __syncthreads();
    stamp(13);
    // kernel gradients + Adam on Z
    double g_s, g_l;
    kernel_grads_adam_z<DMAX, true, (DMAX <= 8 ? 2 : 1), DC>(Zt, Pt, G, GT, GKXT, s, inv_l2, step_size, bc2s, scratch, &g_s,
                                                         &g_l);
    g_s += gv_sum;
    g_l /= (ell * ell * ell);
    stamp(14);

    // ------------------------------- Adam (m, scalars) ----------------------
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
  };
#pragma nounroll
  for (int step = 1; step <= opt.training_iter; ++step) step_fn(step);

  // ------------------------------- prediction ------------------------------
  refresh_hypers();
  if (!(opt.eval_stale_chol && opt.training_iter > 0)) factorize();
  const double s = sh.s, inv_l2 = sh.inv_l2, c = sh.c;
  for (int t0 = 0; t0 < T; t0 += Mp) {
    const int nc = (T - t0) < Mp ? (T - t0) : Mp;
    __syncthreads();
    stage_points_t(Pt, f.Xt + (size_t)t0 * D, nc, D, Mp);
    __syncthreads();
    build_kx<DC>(Zt, Pt, nc, s, inv_l2);
    __syncthreads();
    forward_products(nc, s, jitter);
    for (int n = threadIdx.x; n < nc; n += NT) {
      const double mu = f.vec[V_MU][n] + c;
      const double var = fmax(f.vec[V_VAR][n], opt.min_variance);
      const double p = 0.5 * erfc(-(mu / sqrt(1.0 + var)) * 0.70710678118654752440);
      const float pf = (float)p;                       // pred_probs            :432
      const bool lab = pf >= 0.5f;                     // pred_labels           :433
      const long long o = desc.out_offset + t0 + n;
      o_probs[o] = pf;
      o_probs_new[o] = lab ? pf : 1.0f - pf;           // pred_probs_new        :438
      o_labels[o] = lab ? 1 : 0;
      o_mu[o] = (float)mu;                             // pred_mu               :435
      o_var[o] = (float)var;                           // pred_variance         :436
      if ((!isfinite(mu) || !isfinite(var)) && sh.status == GAPRO_OK) sh.status = GAPRO_ERR_NOT_FINITE;  // first error wins
    }
    __syncthreads();
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

// WPS = waves per SIMD the register budget is sized for: kWavesPerSimd (two workgroups per CU) for a full
// launch, 2 (one workgroup per CU, 256 VGPRs, no spills in the body) when the launch has fewer fits than CUs
// KMIN: the copy-free product forms (fit_body), for fits up to M_p = kKminMaxMp -- a function of M_p alone, so that a fit
// has the same bits in every build; the launcher (gapro_svgp_fit_batch) sends a fit to the instantiation of its M_p.
// One form per kernel: with both bodies in one kernel either loses ~2 % (registers, code size).
template <int WPS, bool KMIN>
__global__ __launch_bounds__(NT, WPS) void k_svgp_fit(int n_fits, int D, const float* __restrict__ feats_spp,
                                                 const int* __restrict__ idx, const gapro_fit_desc* __restrict__ descs,
                                                 const double* __restrict__ init_mean, gapro_fit_options opt,
                                                 double* __restrict__ ws, float* __restrict__ o_probs,
                                                 float* __restrict__ o_probs_new, unsigned char* __restrict__ o_labels,
                                                 float* __restrict__ o_mu, float* __restrict__ o_var,
                                                 int* __restrict__ o_status, double* __restrict__ o_loss,
                                                 unsigned* ticket) {
  extern __shared__ double dyn_lds[];
  const int fit = claim_fit(ticket);
  if (fit >= n_fits) return;
  const gapro_fit_desc desc = descs[fit];
  const int Mp = gapro_pad_m(desc.m1 + desc.m2, D);
  ldsd* Zt = (ldsd*)dyn_lds;
  ldsd* Pt = Zt + D * Mp;
  ldsd* scratch = Pt + D * Mp;
  fit_setup(desc, D, feats_spp, idx, init_mean, ws, Zt, Pt);
  double* loss_slot = &o_loss[desc.slot];
  // the reference's two feature widths (xyz+rgb = 6, deep features = 32) get a compile-time D: the distance
  // loops unroll and their LDS reads are issued together; any other D <= 32 runs the generic body
#define GAPRO_FIT_KM(TUV, DM, DCV, WGV)                                                                       \
  fit_body<TUV, DM, DCV, WGV, KMIN, (WPS == 2 ? 4 : 1)>(opt, Zt, Pt, scratch, desc, o_probs, o_probs_new, o_labels, o_mu, \
                                                        o_var, loss_slot)
#define GAPRO_FIT_BODY(DM, DCV)                                                                                   \
  do {                                                                                                            \
    if (Mp > kFuseMaxMp && Mp % 32 == 0 && !(opt.reserved & GAPRO_FIT_DBG_WG_TILED_NONE) &&                       \
        ((opt.reserved & GAPRO_FIT_DBG_WG_TILED_ALL) || Mp % 128 == 0))                                           \
      /* workgroup-tiled products (gemm_wg; bit-identical to the per-wave ones) where whole 128 x 128 tiles       \
         cover the matrix: M_p = 256, 384 (+6 % / +4 % fits/s, a quarter less traffic; neutral to -7 % at         \
         the other sizes: DESIGN 6.0).  The debug bits: every M_p > 128 that is a multiple of 32, or nowhere */   \
      GAPRO_FIT_KM(1, DM, DCV, (WPS == 2 ? 4 : 2));                                                               \
    else if (WPS == 2 && DM == 6 && !KMIN && Mp >= kTu4MinMp && Mp % 32 == 0) {                                   \
      if constexpr (WPS == 2 && DM == 6 && !KMIN)                                                                 \
        fit_body<4, DM, DCV>(opt, Zt, Pt, scratch, desc, o_probs, o_probs_new, o_labels, o_mu, o_var, loss_slot); \
    } else if (Mp >= 128)                                                                                         \
      GAPRO_FIT_KM(2, DM, DCV, 0);                                                                                \
    else                                                                                                          \
      GAPRO_FIT_KM(1, DM, DCV, 0);                                                                                \
  } while (0)
  if (D == 6) GAPRO_FIT_BODY(6, 6);
  else if (D == 32) GAPRO_FIT_BODY(32, 32);
  else GAPRO_FIT_BODY(32, 0);
#undef GAPRO_FIT_BODY
#undef GAPRO_FIT_KM
  fit_epilogue(desc, opt, o_status, o_loss);
}

}  // namespace
