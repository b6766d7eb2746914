// Batched prediction from exported GP states (gapro_svgp_predict_batch): the posterior of many trained whitened-SVGP
// classifiers at test inputs the fits never saw.  Arithmetic: SURVEY Appendix B.4 / oracle svgp_predict, the formulas of
// the fit kernels' own prediction tails; float64 throughout, outputs rounded to float32 once.
//
// Two kernels behind one call.
//   k_svgp_predict_prep   one workgroup per model, largest first: K_ZZ + jitter I from the state, Cholesky with
//                         psd_safe_cholesky's retry rule, L^-1 by forward substitution.  It leaves, per model, in the
//                         caller's workspace: (L^-1)^T and tril(L_S), both M_p x M_p row-major and zero-padded to the
//                         16-wide MFMA tile, and the padded mean.  O(M^3) once per model.
//   k_svgp_predict_apply  one wave per work item (model, tile of 32 test columns).  The tile's k(Z, x) block, M_p x 32,
//                         is evaluated on chip as 16 x 16 tiles in the accumulator layout of v_mfma_f64_16x16x4_f64
//                         (lane l = (lq = l >> 4, lr = l & 15) holds rows lq + 4 r of column lr) -- which is at the same
//                         time the B operand of the next product in the TN form  C[i][j] += sum_k P[k][i] Q[k][j].  So
//                         A = L^-1 KX overwrites KX in place (block rows from the bottom up: row i needs KX rows <= i
//                         only) and B = L_S^T A is transient: only sum (B^2 - A^2) and m^T A leave the products,
//                         summed per lane and then over the four row groups of a column by a fixed shuffle tree.  The
//                         P operands are read straight from the workspace: register r of tile (k, i) is
//                         W[(16 k + lq + 4 r) M_p + 16 i + lr], sixteen consecutive doubles per row group, for (L^-1)^T
//                         and L_S alike; the two matrices of a model are shared by all of its tiles and stay in L2,
//                         every loaded operand feeds the two column blocks of the tile.  The column block lives in LDS
//                         (256 M_p bytes per wave: the launch is split by M_p so that small models keep their
//                         occupancy) or, beyond M_p = 256, in a slice of the workspace that the wave keeps in L2.
// Every column is computed by the same instructions in the same order whatever else is in the tile or the launch: a
// row's result depends on its model and its features only.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "fit_layout.h"
#include "fit_math.h"

namespace {
using namespace gapro_fit;
using gapro_fit_math::ldsd;
using gapro_mfma::d4;

constexpr int kPrepThreads = 1024;
constexpr int kTileCols = 32;      // test columns of one work item (two MFMA column blocks)
constexpr int kCB = kTileCols / 16;
constexpr int kLdsMaxMp = 256;     // largest padded size whose column block lives in LDS (64 KiB)
constexpr int kBigBlocks = 512;    // persistent waves of the launch for the models beyond (each owns a workspace slice)

// One model of the launch as the kernels see it (uploaded to the head of the workspace, largest M_p first)
struct PredModel {
  long long state_off, row_off, out_off;  // doubles / rows / outputs
  long long ws_off;                       // doubles from the workspace's matrix area: LiT [Mp^2] | LS [Mp^2] | mean [Mp]
  long long tile0;                        // first work item of the model inside its launch class
  int t, M, Mp, slot;
};

__device__ inline int pad16(int m) { return (m + 15) / 16 * 16; }

// ------------------------------------------------------------------------------------------------------------------
// prep: Cholesky and inverse of one model on one workgroup, matrices in global memory (they are M_p^2 doubles: up to
// hundreds of megabytes for the largest fits the library takes)
__global__ __launch_bounds__(kPrepThreads) void k_svgp_predict_prep(int n_models, int D,
                                                                     const PredModel* __restrict__ models,
                                                                     const double* __restrict__ state,
                                                                     double* __restrict__ wsm, gapro_fit_options opt,
                                                                     int* __restrict__ go, int* __restrict__ o_status) {
  __shared__ int s_bad;
  __shared__ double s_piv;
  const PredModel pm = models[blockIdx.x];
  const int tid = threadIdx.x, NT = kPrepThreads, lane = tid & 63, wv = tid >> 6, NW = kPrepThreads / 64;
  const double* st = state + pm.state_off;
  const int M = pm.M, Mp = pm.Mp;
  // a state of another shape, or of a failed fit: refuse the model
  int status = GAPRO_OK;
  if ((int)st[SH_M] != M || (int)st[SH_D] != D) status = GAPRO_ERR_BAD_ARG;
  else if (st[SH_STATUS] != 0.0) status = (int)st[SH_STATUS];
  if (status != GAPRO_OK || pm.t == 0) {
    if (tid == 0) {
      o_status[pm.slot] = status;
      go[pm.slot] = 0;  // the apply kernel writes nothing for this model
    }
    return;
  }
  const double jitter = st[SH_JITTER];
  const double s = gapro_fit_math::softplus(st[SH_RS]), ell = gapro_fit_math::softplus(st[SH_RL]);
  const double nh_inv_l2 = -0.5 * (1.0 / (ell * ell));
  const double* Z = st + kStateHeader;
  const double* mean = Z + (long long)M * D;
  const double* LS = mean + M;
  double* LiT = wsm + pm.ws_off;                // (L^-1)^T, row-major [Mp][Mp]
  double* L = LiT + (long long)Mp * Mp;         // the factor while it is needed, then tril(L_S)
  double* mp = L + (long long)Mp * Mp;

  double extra = 0.0;
  for (int attempt = 0;; ++attempt) {
    // lower triangle of K_ZZ + (jitter + extra) I
    for (int i = wv; i < M; i += NW)
      for (int j = lane; j <= i; j += 64) {
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) {
          const double t = Z[(long long)i * D + d] - Z[(long long)j * D + d];
          d2 += t * t;
        }
        const double kv = s * gapro_fit_math::rbf_exp(nh_inv_l2 * d2);
        L[(long long)i * Mp + j] = i == j ? kv + (jitter + extra) : kv;
      }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    // right-looking Cholesky, one column per trip
    for (int j = 0; j < M; ++j) {
      if (tid == 0) {
        const double d = L[(long long)j * Mp + j];
        if (!(d > 0.0)) s_bad = 1;  // not positive definite (or NaN): psd_safe_cholesky's retry condition
        s_piv = sqrt(d);
      }
      __syncthreads();
      if (s_bad) break;
      const double piv = s_piv;
      for (int i = j + tid; i < M; i += NT) L[(long long)i * Mp + j] = i == j ? piv : L[(long long)i * Mp + j] / piv;
      __syncthreads();
      // trailing update of the lower triangle: rows i > j (one wave each), columns j < k <= i
      for (int i = j + 1 + wv; i < M; i += NW) {
        const double lij = L[(long long)i * Mp + j];
        for (int k = j + 1 + lane; k <= i; k += 64) L[(long long)i * Mp + k] -= lij * L[(long long)k * Mp + j];
      }
      __syncthreads();
    }
    __syncthreads();
    if (!s_bad) break;
    if (attempt >= opt.psd_retries) {
      status = GAPRO_ERR_CHOLESKY;
      break;
    }
    extra = opt.psd_jitter;
    for (int e = 0; e < attempt; ++e) extra *= 10.0;  // psd_jitter 10^attempt, replacing the previous amount
    __syncthreads();
  }
  if (tid == 0) {
    o_status[pm.slot] = status;
    go[pm.slot] = status == GAPRO_OK ? 1 : 0;
  }
  if (status != GAPRO_OK) return;

  // (L^-1)^T: thread c solves L x = e_c by forward substitution; row c of LiT is x (zero before c and in the padding)
  for (int c = tid; c < Mp; c += NT) {
    double* x = LiT + (long long)c * Mp;
    for (int r = 0; r < Mp; ++r) x[r] = 0.0;
    if (c < M) {
      x[c] = 1.0 / L[(long long)c * Mp + c];
      for (int r = c + 1; r < M; ++r) {
        const double* lr = L + (long long)r * Mp;
        double acc = 0.0;
        for (int k = c; k < r; ++k) acc = fma(lr[k], x[k], acc);
        x[r] = -acc / lr[r];
      }
    }
  }
  __syncthreads();
  // the factor is no longer needed: its place takes tril(L_S), zero-padded; the padded mean
  for (int i = wv; i < Mp; i += NW)
    for (int j = lane; j < Mp; j += 64) L[(long long)i * Mp + j] = (i < M && j <= i) ? LS[(long long)i * M + j] : 0.0;
  for (int i = tid; i < Mp; i += NT) mp[i] = i < M ? mean[i] : 0.0;
}

// ------------------------------------------------------------------------------------------------------------------
__device__ inline d4 zero4() { return (d4){0.0, 0.0, 0.0, 0.0}; }
// acc += P^T Q for one 16-row block of the contraction index (both operands as accumulator-layout tiles)
__device__ inline d4 tn(d4 acc, const d4& P, const d4& Q) {
#pragma unroll
  for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(P[r], Q[r], acc, 0, 0, 0);
  return acc;
}

// One work item: `buf` holds the tile's column block, tile k of column block cb at ((cb NB + k) 4 + r) 64 + lane.
// DC: feature width known at compile time (the test point's coordinates stay in registers), 0 = any width.
template <int DC, typename BufPtr>
__device__ inline void predict_tile(const PredModel& pm, long long tile, int D, const double* __restrict__ state,
                                    const double* __restrict__ wsm, const float* __restrict__ feats,
                                    long long n_feat_rows, const int* __restrict__ rows, double min_variance,
                                    BufPtr buf, float* __restrict__ o_probs, float* __restrict__ o_probs_new,
                                    unsigned char* __restrict__ o_labels, float* __restrict__ o_mu,
                                    float* __restrict__ o_var, int* __restrict__ o_status) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  const int M = pm.M, Mp = pm.Mp, NB = Mp >> 4;
  const double* st = state + pm.state_off;
  const double jitter = st[SH_JITTER], c = st[SH_C];
  const double s = gapro_fit_math::softplus(st[SH_RS]), ell = gapro_fit_math::softplus(st[SH_RL]);
  const double nh_inv_l2 = -0.5 * (1.0 / (ell * ell));
  const double* Z = st + kStateHeader;
  const double* LiT = wsm + pm.ws_off;
  const double* LS = LiT + (long long)Mp * Mp;
  const double* mp = LS + (long long)Mp * Mp;
  const int Dr = DC ? DC : D;

  // ---- KX tiles: rows = inducing points, column lr of block cb = test row tile * 32 + 16 cb + lr
  bool bad_row = false, bad_x = false;
#pragma unroll
  for (int cb = 0; cb < kCB; ++cb) {
    const long long tr = tile * kTileCols + 16 * cb + lr;
    const bool on = tr < pm.t;
    long long row = on ? (long long)rows[pm.row_off + tr] : 0;
    if (row < 0 || row >= n_feat_rows) {
      bad_row = true;
      row = 0;
    }
    const float* x = feats + row * Dr;
    double xr[DC ? DC : 1];
    if (DC) {
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        xr[d] = (double)x[d];
        bad_x = bad_x || (on && !isfinite(xr[d]));
      }
    }
    for (int k = 0; k < NB; ++k) {
      double s2[4] = {0.0, 0.0, 0.0, 0.0};
      int zr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * k + lq + 4 * r;
        zr[r] = i < M ? i : 0;
      }
      if (DC) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int d = 0; d < DC; ++d) {
            const double t = Z[(long long)zr[r] * DC + d] - xr[d];
            s2[r] += t * t;
          }
      } else {
        for (int d = 0; d < D; ++d) {
          const double xd = (double)x[d];
          bad_x = bad_x || (on && !isfinite(xd));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double t = Z[(long long)zr[r] * D + d] - xd;
            s2[r] += t * t;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool in = 16 * k + lq + 4 * r < M && on;
        buf[((cb * NB + k) * 4 + r) * 64 + lane] = in ? s * gapro_fit_math::rbf_exp(nh_inv_l2 * s2[r]) : 0.0;
      }
    }
  }
  // (every lane reads back only what it wrote itself: the block needs no hand-over between lanes)

  // ---- A = L^-1 KX in place, block rows from the bottom up; m^T A on the way
  double pmu[kCB], pv[kCB];
#pragma unroll
  for (int cb = 0; cb < kCB; ++cb) pmu[cb] = pv[cb] = 0.0;
  for (int i = NB - 1; i >= 0; --i) {
    d4 acc[kCB];
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb) acc[cb] = zero4();
    const double* pcol = LiT + 16 * i + lr;
    for (int k = 0; k <= i; ++k) {
      d4 P;
#pragma unroll
      for (int r = 0; r < 4; ++r) P[r] = pcol[(long long)(16 * k + lq + 4 * r) * Mp];
#pragma unroll
      for (int cb = 0; cb < kCB; ++cb) {
        d4 Q;
#pragma unroll
        for (int r = 0; r < 4; ++r) Q[r] = buf[((cb * NB + k) * 4 + r) * 64 + lane];
        acc[cb] = tn(acc[cb], P, Q);
      }
    }
    double mv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mv[r] = mp[16 * i + lq + 4 * r];
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double a = acc[cb][r];
        buf[((cb * NB + i) * 4 + r) * 64 + lane] = a;
        pmu[cb] = fma(mv[r], a, pmu[cb]);
      }
  }
  // ---- B = L_S^T A, block row i from the A rows k >= i; only sum (B^2 - A^2) is kept, element by element as in the
  // fit kernels' prediction tails (with L_S = I, the untrained model, the sum is exactly zero)
  for (int i = 0; i < NB; ++i) {
    d4 acc[kCB];
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb) acc[cb] = zero4();
    const double* pcol = LS + 16 * i + lr;
    for (int k = i; k < NB; ++k) {
      d4 P;
#pragma unroll
      for (int r = 0; r < 4; ++r) P[r] = pcol[(long long)(16 * k + lq + 4 * r) * Mp];
#pragma unroll
      for (int cb = 0; cb < kCB; ++cb) {
        d4 Q;
#pragma unroll
        for (int r = 0; r < 4; ++r) Q[r] = buf[((cb * NB + k) * 4 + r) * 64 + lane];
        acc[cb] = tn(acc[cb], P, Q);
      }
    }
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double a = buf[((cb * NB + i) * 4 + r) * 64 + lane], b = acc[cb][r];
        pv[cb] += b * b - a * a;
      }
  }
  // ---- the four row groups of a column, fixed tree; five stores per row
  int st_out = GAPRO_OK;
#pragma unroll
  for (int cb = 0; cb < kCB; ++cb) {
    const double dv = gapro_fit_math::sum_rows(pv[cb]);
    const double mu = gapro_fit_math::sum_rows(pmu[cb]) + c;
    const long long tr = tile * kTileCols + 16 * cb + lr;
    if (lq == 0 && tr < pm.t) {
      const double var = fmax(s + jitter + dv, min_variance);
      const double p = 0.5 * erfc(-(mu / sqrt(1.0 + var)) * 0.70710678118654752440);
      const float pf = (float)p;
      const bool lab = pf >= 0.5f;
      const long long o = pm.out_off + tr;
      o_probs[o] = pf;
      o_probs_new[o] = lab ? pf : 1.0f - pf;
      o_labels[o] = lab ? 1 : 0;
      o_mu[o] = (float)mu;
      o_var[o] = (float)var;
      if (!isfinite(mu) || !isfinite(var)) st_out = GAPRO_ERR_NOT_FINITE;
    }
  }
  if (bad_x) st_out = GAPRO_ERR_NOT_FINITE;  // (an infinite coordinate gives k = 0, a finite result: flagged all the same)
  if (bad_row) st_out = GAPRO_ERR_BAD_ARG;
  if (st_out != GAPRO_OK) atomicMin(&o_status[pm.slot], st_out);  // (rare; the minimum is the same in any order)
}

// the model of work item `item`: the last one whose first item is <= item
__device__ inline int find_model(const PredModel* __restrict__ models, int n, long long item) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (models[mid].tile0 <= item) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// LDSBUF: the column block in dynamic LDS, one work item per workgroup; otherwise a persistent wave with a slice of
// the workspace (scratch + blockIdx.x * scratch_stride), taking items grid-stride
template <int DC, bool LDSBUF>
__global__ __launch_bounds__(64) void k_svgp_predict_apply(int n_models, long long n_items, int D,
                                                           const PredModel* __restrict__ models,
                                                           const double* __restrict__ state,
                                                           const double* __restrict__ wsm, double* __restrict__ scratch,
                                                           long long scratch_stride, const float* __restrict__ feats,
                                                           long long n_feat_rows, const int* __restrict__ rows,
                                                           double min_variance, const int* __restrict__ go,
                                                           float* __restrict__ o_probs,
                                                           float* __restrict__ o_probs_new,
                                                           unsigned char* __restrict__ o_labels, float* __restrict__ o_mu,
                                                           float* __restrict__ o_var, int* __restrict__ o_status) {
  extern __shared__ double dyn_lds[];
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int mi = find_model(models, n_models, item);
    const PredModel pm = models[mi];
    // a model the prep kernel refused (state of a failed fit, wrong shape, Cholesky failure) is not predicted: nothing
    // is written for it
    if (!go[pm.slot]) continue;
    if constexpr (LDSBUF) {
      predict_tile<DC>(pm, item - pm.tile0, D, state, wsm, feats, n_feat_rows, rows, min_variance, (ldsd*)dyn_lds,
                       o_probs, o_probs_new, o_labels, o_mu, o_var, o_status);
    } else {
      predict_tile<DC>(pm, item - pm.tile0, D, state, wsm, feats, n_feat_rows, rows, min_variance,
                       scratch + (long long)blockIdx.x * scratch_stride, o_probs, o_probs_new, o_labels, o_mu, o_var,
                       o_status);
    }
  }
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
// head of the workspace: the model table, then one go / no-go flag per model (prep -> apply)
inline size_t table_bytes(int n) { return align256((size_t)n * sizeof(PredModel)); }
inline size_t head_bytes(int n) { return table_bytes(n) + align256((size_t)n * sizeof(int)); }
inline int host_pad16(int m) { return (std::max(m, 1) + 15) / 16 * 16; }
inline long long model_ws_doubles(int Mp) { return 2LL * Mp * Mp + Mp; }

}  // namespace

extern "C" {

size_t gapro_svgp_predict_workspace_bytes(int32_t n_models, int32_t feat_dim, const int32_t* h_m) {
  if (n_models <= 0 || feat_dim <= 0 || !h_m) return 0;
  size_t bytes = head_bytes(n_models);
  int big = 0;
  for (int i = 0; i < n_models; ++i) {
    const int Mp = host_pad16(h_m[i]);
    bytes += (size_t)model_ws_doubles(Mp) * 8;
    if (Mp > kLdsMaxMp) big = std::max(big, Mp);
  }
  bytes = align256(bytes);
  if (big) bytes += (size_t)kBigBlocks * kCB * big * 16 * 8;
  return bytes;
}

int gapro_svgp_predict_batch(gapro_ctx* ctx, void* stream_, int32_t n_models, int32_t feat_dim, const double* d_state,
                             const int32_t* h_m, const gapro_predict_desc* h_descs, const float* d_feats,
                             int64_t n_feat_rows, const int32_t* d_rows, const gapro_fit_options* opt,
                             void* d_workspace, size_t workspace_bytes, float* d_probs, float* d_probs_new,
                             uint8_t* d_labels, float* d_mu, float* d_var, int32_t* d_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_models == 0) return GAPRO_OK;
  if (n_models < 0 || feat_dim <= 0 || !d_state || !h_m || !h_descs || !d_feats || n_feat_rows <= 0 || !d_rows || !opt ||
      !d_workspace || !d_probs || !d_probs_new || !d_labels || !d_mu || !d_var || !d_status)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_predict_batch: bad argument");
  if (opt->psd_retries < 0 || opt->psd_retries > 8 || !(opt->psd_jitter >= 0.0))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_predict_batch: bad options");
  if (!(opt->min_variance >= 0.0 && opt->min_variance < INFINITY))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_predict_batch: min_variance %g is negative or not finite",
                      opt->min_variance);
  const size_t need = gapro_svgp_predict_workspace_bytes(n_models, feat_dim, h_m);
  if (need > workspace_bytes)
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_svgp_predict_batch: workspace too small (%zu > %zu)", need,
                      workspace_bytes);
  hipStream_t stream = (hipStream_t)stream_;
  // the models, largest first (the prep kernel's long workgroups start first); the apply launches take contiguous
  // ranges of that order: beyond kLdsMaxMp | <= 256 | <= 128 | <= 64
  std::vector<PredModel> pm((size_t)n_models);
  long long ws_off = 0;
  for (int i = 0; i < n_models; ++i) {
    if (h_m[i] <= 0 || h_descs[i].t < 0)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_predict_batch: model %d has no inducing points or t < 0", i);
    PredModel& p = pm[(size_t)i];
    p.state_off = h_descs[i].state_offset;
    p.row_off = h_descs[i].row_offset;
    p.out_off = h_descs[i].out_offset;
    p.t = h_descs[i].t;
    p.M = h_m[i];
    p.Mp = host_pad16(h_m[i]);
    p.slot = i;
    p.ws_off = ws_off;
    p.tile0 = 0;
    ws_off += model_ws_doubles(p.Mp);
  }
  std::stable_sort(pm.begin(), pm.end(), [](const PredModel& a, const PredModel& b) { return a.Mp > b.Mp; });
  const int caps[4] = {1 << 30, kLdsMaxMp, 128, 64};
  int cls_lo[5] = {0, 0, 0, 0, n_models};
  long long cls_items[4] = {0, 0, 0, 0};
  int cls_mp[4] = {0, 0, 0, 0};
  {
    int i = 0;
    for (int c = 0; c < 4; ++c) {
      cls_lo[c] = i;
      const int floor_mp = c < 3 ? caps[c + 1] : 0;
      while (i < n_models && pm[(size_t)i].Mp > floor_mp) {
        PredModel& p = pm[(size_t)i];
        p.tile0 = cls_items[c];
        cls_items[c] += ((long long)p.t + kTileCols - 1) / kTileCols;
        cls_mp[c] = std::max(cls_mp[c], p.Mp);
        ++i;
      }
    }
  }
  char* wsb = (char*)d_workspace;
  PredModel* d_models = (PredModel*)wsb;
  int* d_go = (int*)(wsb + table_bytes(n_models));
  const size_t head = head_bytes(n_models);
  double* wsm = (double*)(wsb + head);
  double* scratch = (double*)(wsb + align256(head + (size_t)ws_off * 8));
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_models, pm.data(), pm.size() * sizeof(PredModel), hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipStreamSynchronize(stream));  // `pm` is pageable host memory that dies with this call
  hipLaunchKernelGGL(k_svgp_predict_prep, dim3(n_models), dim3(kPrepThreads), 0, stream, (int)n_models, (int)feat_dim,
                     d_models, d_state, wsm, *opt, d_go, d_status);
  GAPRO_LAUNCH_CHECK(ctx);
  for (int c = 0; c < 4; ++c) {
    if (cls_items[c] == 0) continue;
    const int nm = cls_lo[c + 1] - cls_lo[c];
    const PredModel* dm = d_models + cls_lo[c];
    const bool lds = c > 0;
    const size_t lds_bytes = lds ? (size_t)kCB * cls_mp[c] * 16 * 8 : 0;
    const long long stride = lds ? 0 : (long long)kCB * cls_mp[c] * 16;
    const long long grid = lds ? cls_items[c] : std::min<long long>(cls_items[c], kBigBlocks);
    if (grid > 0x7fffffffLL)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_predict_batch: more than 2^31 column tiles in one launch");
#define GAPRO_PREDICT_LAUNCH(DCV, LDSV)                                                                             \
  do {                                                                                                              \
    auto kern = k_svgp_predict_apply<DCV, LDSV>;                                                                    \
    if (lds_bytes > 48 * 1024)                                                                                      \
      GAPRO_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,      \
                                               (int)lds_bytes));                                                    \
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64), lds_bytes, stream, nm, cls_items[c], (int)feat_dim, dm, \
                       d_state, (const double*)wsm, scratch, stride, d_feats, (long long)n_feat_rows, d_rows,       \
                       opt->min_variance, (const int*)d_go, d_probs, d_probs_new, d_labels, d_mu, d_var, d_status); \
  } while (0)
    if (feat_dim == 6) {
      if (lds) GAPRO_PREDICT_LAUNCH(6, true);
      else GAPRO_PREDICT_LAUNCH(6, false);
    } else {
      if (lds) GAPRO_PREDICT_LAUNCH(0, true);
      else GAPRO_PREDICT_LAUNCH(0, false);
    }
#undef GAPRO_PREDICT_LAUNCH
    GAPRO_LAUNCH_CHECK(ctx);
  }
  return GAPRO_OK;
}

}  // extern "C"
