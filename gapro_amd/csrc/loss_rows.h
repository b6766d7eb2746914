// A matched row of a criterion, walked and differentiated: what ISBNet's matched losses (match_loss.hip) and SPFormer's
// (spf_loss.hip) compute per (query, instance) pair, once.  A workgroup of four waves takes one row, thread t the
// columns t, t + 256, ..:
//   walk_row        the first walk over the logit row: the dice, BCE, IoU and level-set sums and the clamped means
//   walk_members    the second walk: the level-set spread around those means
//   mask_grad_row   the gradient by the row's logits of the dice, BCE and level-set terms, from the caller's coefficients
//   wave_lse, class_grad_row   the class term of a query's logit row and its gradient
// A criterion hands over its row as a RowCols and what it weighs the terms by as values; the records, the normalisers,
// the conditions and the refusals stay with it.  Every sum is a per-thread float64 partial, reduced by wave_reduce.h's
// butterfly and then across the waves through LDS in wave order; the counts are integers.  The walks own their LDS
// slots and are called by every thread of the workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include "match_math.h"
#include "wave_reduce.h"

constexpr int kLossThreads = 256, kLossWaves = 4;
constexpr int kLossMaxF = GAPRO_MATCH_LOSS_MAX_FEATS;

// every thread's partial -> the workgroup's sum in every thread: the butterfly, then the waves in their order
__device__ inline double block_sum(double v, double* slot /* [kLossWaves] in LDS, this quantity's own */) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = slot[0];
#pragma unroll
  for (int k = 1; k < kLossWaves; ++k) s += slot[k];
  return s;
}
__device__ inline int block_sum(int v, int* slot) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return slot[0] + slot[1] + slot[2] + slot[3];
}

struct BoxTest {  // criterion.py:196-198 (SPFormer's loss.py:354-356) in float32: the padded faces of one label box
  float lo[3], hi[3];
};
__device__ inline BoxTest box_test(const float* __restrict__ g) {
  BoxTest bt;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    bt.lo[k] = g[k] - 0.005f;
    bt.hi[k] = g[k + 3] + 0.005f;
  }
  return bt;
}
__device__ inline bool inside(const BoxTest& bt, const float* __restrict__ c) {  // a NaN coordinate is outside
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) in = in && c[k] >= bt.lo[k] && c[k] <= bt.hi[k];
  return in;
}

struct RowCols {   // one matched row over its sample's S columns
  const float* x;  // [S] the query's mask logits
  const float* t;  // [S] the instance's targets
  const float* w;  // [S] the columns' weights
  const float* c;  // [S, 3] their coordinates
  const float* f;  // [S, F] their features
  int S, F;
  BoxTest bt;      // the instance's label box: its members are the level-set term's columns
};

struct RowSums {
  double ssig, st, sst;  // sum sig, sum t, sum sig t
  double swb, sw;        // sum w' (softplus(x) - x t) with w' the BCE weight, sum w
  double a, inter;       // sum of sig over the members, sum [x >= 0] t
  int cnt, nr;           // sum [x >= 0], the members
  double mu[kLossMaxF];  // the members' sig-weighted feature means, over max(a, 1e-5); 0 from F on
  bool odd_target;       // this thread met a target that is neither 0 nor 1 (the one field that is not a sum)
};

// the first walk; the BCE weight of a column is its w, or 1 for an unweighted BCE
__device__ inline RowSums walk_row(const RowCols& rc, bool weighted) {
  __shared__ double s_d[7 + kLossMaxF][kLossWaves];
  __shared__ int s_i[2][kLossWaves];
  RowSums r;
  r.ssig = r.st = r.sst = r.swb = r.sw = r.a = r.inter = 0.0;
  r.cnt = r.nr = 0;
  r.odd_target = false;
  double bf[kLossMaxF];
#pragma unroll
  for (int f = 0; f < kLossMaxF; ++f) bf[f] = 0.0;
  for (int s = threadIdx.x; s < rc.S; s += kLossThreads) {
    const double x = (double)rc.x[s], tv = (double)rc.t[s], wv = (double)rc.w[s];
    r.odd_target = r.odd_target || (tv != 0.0 && tv != 1.0);
    const Sig sg = sigmoid_of(x);
    const double sp = softplus_of(x, sg);
    r.ssig += sg.sig;
    r.st += tv;
    r.sst += sg.sig * tv;
    r.swb += (weighted ? wv : 1.0) * (sp - x * tv);
    r.sw += wv;
    if (x >= 0.0) {
      ++r.cnt;
      r.inter += tv;
    }
    if (inside(rc.bt, rc.c + (size_t)s * 3)) {
      ++r.nr;
      r.a += sg.sig;
#pragma unroll
      for (int f = 0; f < kLossMaxF; ++f)
        if (f < rc.F) bf[f] += sg.sig * (double)rc.f[(size_t)s * rc.F + f];
    }
  }
  r.ssig = block_sum(r.ssig, s_d[0]);
  r.st = block_sum(r.st, s_d[1]);
  r.sst = block_sum(r.sst, s_d[2]);
  r.swb = block_sum(r.swb, s_d[3]);
  r.sw = block_sum(r.sw, s_d[4]);
  r.a = block_sum(r.a, s_d[5]);
  r.inter = block_sum(r.inter, s_d[6]);
  r.cnt = block_sum(r.cnt, s_i[0]);
  r.nr = block_sum(r.nr, s_i[1]);
  const double a_cl = r.a < 1e-5 ? 1e-5 : r.a;  // clamp(min=1e-5); a NaN stays
#pragma unroll
  for (int f = 0; f < kLossMaxF; ++f) r.mu[f] = f < rc.F ? block_sum(bf[f], s_d[7 + f]) / a_cl : 0.0;
  return r;
}

// the second walk, over the members only: sum sig |f - mu|^2 / nr.  For nr > 0; whether a row takes the walk is the
// caller's condition, uniform over the workgroup.
__device__ inline double walk_members(const RowCols& rc, const double* mu, int nr) {
  __shared__ double s_ls[kLossWaves];
  double ls = 0.0;
  for (int s = threadIdx.x; s < rc.S; s += kLossThreads) {
    if (!inside(rc.bt, rc.c + (size_t)s * 3)) continue;
    const Sig sg = sigmoid_of((double)rc.x[s]);
    double dev = 0.0;
#pragma unroll
    for (int f = 0; f < kLossMaxF; ++f)
      if (f < rc.F) {
        const double df = (double)rc.f[(size_t)s * rc.F + f] - mu[f];
        dev += df * df;
      }
    ls += sg.sig * dev;
  }
  return block_sum(ls, s_ls) / (double)nr;
}

// out[s] = d / d x[s] of the caller's weighted sum of the row's terms, for the row's own columns s = t, t + 256, ..:
//   dice       sig' (kd_num - t kd_den): kd_num = k (2 sst + 1), kd_den = 2 k (ssig + st + 1), k the upstream weight
//              over the normaliser and the squared denominator
//   BCE        k_bce w' (sig - t), w' as in walk_row
//   level set  for a member, sig' k_ls sum_f ((f - mu_f)^2 - rfk mu_f f).  rfk is 0 for a free mean, whose own
//              derivative cancels (sum v (f - mu) = 0); below the clamp mu = (sum v f) / 1e-5 and rfk = 2 (1e-5 - a) / 1e-5.
//              k_ls = 0: the row has no level-set term.
__device__ inline void mask_grad_row(const RowCols& rc, double kd_num, double kd_den, double k_bce, bool weighted,
                                     double k_ls, double rfk, const double* mu, float* __restrict__ out) {
  for (int s = threadIdx.x; s < rc.S; s += kLossThreads) {
    const double x = (double)rc.x[s], tv = (double)rc.t[s];
    const double wv = weighted ? (double)rc.w[s] : 1.0;
    const Sig sg = sigmoid_of(x);
    const double sm = sg.e / (1.0 + sg.e);                      // min(sig, 1 - sig)
    const double dsig = sm / (1.0 + sg.e);                      // sig (1 - sig)
    const double sig_t = x >= 0.0 ? (1.0 - tv) - sm : sm - tv;  // sig - t, cancellation-free (consumer.hip k_wbce_grad)
    double dv = kd_num - tv * kd_den;
    if (k_ls != 0.0 && inside(rc.bt, rc.c + (size_t)s * 3)) {
      double dev = 0.0;
#pragma unroll
      for (int f = 0; f < kLossMaxF; ++f)
        if (f < rc.F) {
          const double fv = (double)rc.f[(size_t)s * rc.F + f], df = fv - mu[f];
          dev += df * df - rfk * mu[f] * fv;
        }
      dv += k_ls * dev;
    }
    out[s] = (float)(dsig * dv + k_bce * wv * sig_t);
  }
}

// log sum_c exp z[c] of a query's C class logits, by one wave, in every lane; a NaN logit makes it NaN
__device__ inline double wave_lse(const float* __restrict__ z, int C) {
  const int lane = threadIdx.x & 63;
  double m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmax(m, (double)z[c]);
  m = wave_max(m);
  double sum = 0.0;
  for (int c = lane; c < C; c += 64) sum += exp((double)z[c] - m);
  sum = wave_sum(sum);
  return m + log(sum);
}

// out[c] = k (softmax(z)[c] - [c == tgt]) for c = first, first + step, .., without the cancellation at p -> 1
__device__ inline void class_grad_row(const float* __restrict__ z, int C, double lse, long long tgt, double k,
                                      int first, int step, float* __restrict__ out) {
  for (int c = first; c < C; c += step) {
    const double dz = (double)z[c] - lse;
    out[c] = (float)(k * (c == tgt ? expm1(dz) : exp(dz)));
  }
}
