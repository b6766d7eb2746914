// ISBNet's dynamic-convolution mask head (include/gapro_hip.h, "Dynamic-convolution mask head"): the
// loop of ISBNet.forward_head (isbnet/model/isbnet.py:783-828) with mask_heads_forward (:855-885), forward and backward,
// without the [Q, C + 6, N_b] input the reference materialises.
//   forward          a workgroup of four waves per (sample, query): the query's weights go to LDS once (float32, as they
//                    are given), wave w takes the sample's 16-point tiles w, w + 4, ..  A tile is x[KP x 16] in LDS
//                    (float64); both layers are FP64 MFMA products with the points as COLUMNS, so the first layer's
//                    accumulator block (rows = channels g + 4 r, columns = points) is the second layer's B operand as it
//                    stands: its k-step r contracts the channels g + 4 r, and the A operand W2^T is read in that order.
//                    Nothing moves between the layers.  The last layer is 4 FMAs a lane and two shuffles.
//   backward_queries the same grid: recomputes h1, h2 of a tile, forms dh2 and dh1 the same way (accumulator -> B operand),
//                    and adds the tile to dW1 = dh1 x^T and dW2 = h1 dh2^T -- products over the POINTS, whose A operands
//                    (dh1, dh2) and B operands (x^T, h1^T) are read transposed from LDS tiles of row stride 17.  The
//                    bias, W3 and query-box sums are per-lane partials, reduced by shuffles at the end.  The waves are
//                    added in wave order through LDS; every element of the controller row is then stored once.
//   backward_points  a workgroup per 64 points of a sample (a wave per 16), the queries in ascending order: the feature
//                    rows of dx = W1 dh1 accumulate in the MFMA accumulators across the queries, the box rows are taken
//                    times sign(d) per query.
// Arithmetic: float64 from the float32 inputs, one rounding on the store; no floating-point atomics; the order of every
// sum is fixed by this layout.  relu'(0) = 0 and sign(0) = 0.  The channels are contracted features first, geometry
// last (a permutation of the sum, not of the definition).
#include "common.h"
#include "launch_util.h"
#include "mfma64.h"

#include <cstdint>

namespace {

using gapro_mfma::d4;
using gapro_mfma::mma16;
using gapro_mfma::unrotate;

constexpr int kThreads = 256, kWaves = 4, kTile = 16, kLd = 17;
constexpr int kPointTile = kWaves * kTile;  // points of a backward_points workgroup
constexpr int kMaxBatch = GAPRO_DYCO_MAX_BATCH;

template <int C>
struct Dy {
  static constexpr int H = C / 2, K = C + 6;
  static constexpr int KP = (K + 3) / 4 * 4;            // contraction length of the first layer
  static constexpr int KR = (KP + 3 + 15) / 16 * 16;    // rows of an x tile: KP, three rows of sign(d), padding
  static constexpr int JB = C / 16, AB = KR / 16;       // 16-row blocks of h1 and of x
  static constexpr int LD1 = C + 1, LD2 = 17;           // row strides of W1 and W2 in LDS (floats)
  // the controller row
  static constexpr int oW2 = K * C, oW3 = oW2 + C * H, ob1 = oW3 + H, ob2 = ob1 + C, ob3 = ob2 + H, P = ob3 + 1;
  // the weights in LDS (floats): W1[KR][LD1] (internal channel order, rows >= K zero), W2[C][LD2] (columns >= H zero),
  // b1[C], b2[16], W3[16]
  static constexpr int lW2 = KR * LD1, lb1 = lW2 + C * LD2, lb2 = lb1 + C, lW3 = lb2 + 16, NW = lW3 + 16;
  static constexpr int XT = KR * kLd;                   // doubles of an x tile
  static_assert(C % 16 == 0 && H <= 16 && KP - K == 2, "built for C = 16 and 32");
};

struct DyArgs {
  const float *theta, *feat, *locs, *box, *qloc, *qbox;
  long long ld_feat;
  int B, Q;
  long long off[kMaxBatch + 1];
  int tile_first[kMaxBatch + 1];  // backward_points: the first workgroup of every sample
  float* y;
  const float* gy;
  float *d_theta, *d_qbox, *d_feat, *d_box;
};

// internal channel (features first) -> the definition's channel (geometry first)
template <int C>
__device__ inline int channel_of(int ap) { return ap < C ? ap + 6 : ap - C; }

// where slot l of the weights in LDS comes from in the controller row; -1: a zero (padding)
template <int C>
__device__ inline int weight_source(int l) {
  using D = Dy<C>;
  if (l < D::lW2) {
    const int ap = l / D::LD1, j = l % D::LD1;
    return ap < D::K && j < C ? channel_of<C>(ap) * C + j : -1;
  }
  if (l < D::lb1) {
    const int j = (l - D::lW2) / D::LD2, k = (l - D::lW2) % D::LD2;
    return k < D::H ? D::oW2 + j * D::H + k : -1;
  }
  if (l < D::lb2) return D::ob1 + (l - D::lb1);
  if (l < D::lW3) return l - D::lb2 < D::H ? D::ob2 + (l - D::lb2) : -1;
  return l - D::lW3 < D::H ? D::oW3 + (l - D::lW3) : -1;
}

// A query's weights on their way to LDS: thread t holds the slots t, t + 256, ..  Fetch and store are apart so that
// the by-point kernel can have the next query's row in flight while it works on this one.
template <int C>
struct WeightRegs {
  static constexpr int kPer = (Dy<C>::NW + kThreads - 1) / kThreads;
  float v[kPer];
  __device__ inline void fetch(const float* __restrict__ theta) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int l = threadIdx.x + u * kThreads;
      const int s = l < Dy<C>::NW ? weight_source<C>(l) : -1;
      const float t = theta[s >= 0 ? s : 0];  // always an address inside the row
      v[u] = s >= 0 ? t : 0.f;
    }
  }
  __device__ inline void store(float* w) const {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int l = threadIdx.x + u * kThreads;
      if (l < Dy<C>::NW) w[l] = v[u];
    }
  }
};

template <int C>
__device__ inline void load_weights(const float* __restrict__ theta, float* w) {
  WeightRegs<C> r;
  r.fetch(theta);
  r.store(w);
}

// rows [0, C) of a wave's x tile: the features of the points n0 .. n0 + 15 (zeros beyond n_end)
template <int C>
__device__ inline void build_features(double* xt, const float* __restrict__ feat, long long ld, long long n0,
                                      long long n_end, int lane) {
  for (int e = lane; e < kTile * C; e += 64) {
    const int n = e / C, c = e % C;
    const long long p = n0 + n;
    xt[c * kLd + n] = p < n_end ? (double)feat[p * ld + c] : 0.0;
  }
}

// rows [C, KR): the six geometry channels of the tile for one query, zeros, and sign(d) of the box channels
template <int C>
__device__ inline void build_geometry(double* xt, const float* __restrict__ locs, const float* __restrict__ box,
                                      const double (&ql)[3], const double (&qd)[3], long long n0, long long n_end,
                                      int lane) {
  using D = Dy<C>;
  if (lane < 16) {
    const long long p = n0 + lane;
    const bool in = p < n_end;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double rel = 0.0, d = 0.0;
      if (in) {
        rel = ql[c] - (double)locs[p * 3 + c];
        d = qd[c] - ((double)box[p * 6 + 3 + c] - (double)box[p * 6 + c]);
      }
      xt[(C + c) * kLd + lane] = rel;
      xt[(C + 3 + c) * kLd + lane] = fabs(d);
      xt[(D::KP + c) * kLd + lane] = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    }
  } else if (lane < 32) {
    const int n = lane - 16;
    for (int r = D::K; r < D::KP; ++r) xt[r * kLd + n] = 0.0;
    for (int r = D::KP + 3; r < D::KR; ++r) xt[r * kLd + n] = 0.0;
  }
}

__device__ inline double relu(double v) { return v <= 0.0 ? 0.0 : v; }  // a NaN stays

// h1 = relu(b1 + W1^T x), h2 = relu(b2 + W2^T h1) of one tile: accumulator layout, register r = channel g + 4 r (+ 16 jb),
// column = point i
template <int C>
__device__ inline void layers(const float* w, const double* xt, int g, int i, d4 (&h1)[Dy<C>::JB], d4& h2) {
  using D = Dy<C>;
#pragma unroll
  for (int jb = 0; jb < D::JB; ++jb) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < D::KP / 4; ++s)
      mma16((double)w[(4 * s + g) * D::LD1 + jb * 16 + i], xt[(4 * s + g) * kLd + i], acc);
    acc = unrotate(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) h1[jb][r] = relu(acc[r] + (double)w[D::lb1 + jb * 16 + g + 4 * r]);
  }
  d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int jb = 0; jb < D::JB; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r)  // this step contracts the channels jb 16 + 4 r + (0 .. 3)
      mma16((double)w[D::lW2 + (jb * 16 + g + 4 * r) * D::LD2 + i], h1[jb][r], acc);
  acc = unrotate(acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) h2[r] = relu(acc[r] + (double)w[D::lb2 + g + 4 * r]);
}

// dh2 = gy W3 [h2 > 0], dh1 = (W2 dh2) [h1 > 0]: the same layout
template <int C>
__device__ inline void hidden_grads(const float* w, double gy, int g, int i, const d4 (&h1)[Dy<C>::JB], const d4& h2,
                                    d4& dh2, d4 (&dh1)[Dy<C>::JB]) {
  using D = Dy<C>;
#pragma unroll
  for (int r = 0; r < 4; ++r) dh2[r] = h2[r] > 0.0 ? gy * (double)w[D::lW3 + g + 4 * r] : 0.0;
#pragma unroll
  for (int jb = 0; jb < D::JB; ++jb) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) mma16((double)w[D::lW2 + (jb * 16 + i) * D::LD2 + g + 4 * r], dh2[r], acc);
    acc = unrotate(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) dh1[jb][r] = h1[jb][r] > 0.0 ? acc[r] : 0.0;
  }
}

// acc (rotated layout) += rows [16 ab, 16 ab + 16) of dx = W1 dh1
template <int C>
__device__ inline void input_grad_block(const float* w, int ab, int g, int i, const d4 (&dh1)[Dy<C>::JB], d4& acc) {
  using D = Dy<C>;
#pragma unroll
  for (int jb = 0; jb < D::JB; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) mma16((double)w[(ab * 16 + i) * D::LD1 + jb * 16 + g + 4 * r], dh1[jb][r], acc);
}

// The box rows of dx times sign(d): rows 3 .. 5 of the geometry block are (g, r) = (3, 0), (0, 1), (1, 1).  Returns the
// lane's box channel (-1: none) and adds its term.
__device__ inline int box_channel(int g) { return g == 3 ? 0 : (g == 0 ? 1 : (g == 1 ? 2 : -1)); }
template <int C>
__device__ inline double box_term(const double* xt, int g, int i, const d4& dxg) {
  const int c = box_channel(g);
  const double v = g == 3 ? dxg[0] : dxg[1];
  return c >= 0 ? xt[(Dy<C>::KP + c) * kLd + i] * v : 0.0;
}

__device__ inline double shfl_xor(double v, int m) { return __shfl_xor(v, m, 64); }
__device__ inline double sum16(double v) {  // over the 16 lanes of a row: every lane gets the sum
  v += shfl_xor(v, 1);
  v += shfl_xor(v, 2);
  v += shfl_xor(v, 4);
  v += shfl_xor(v, 8);
  return v;
}

struct QueryGeom {
  double ql[3], qd[3];
};
__device__ inline QueryGeom query_geom(const DyArgs& a, long long bq) {
  QueryGeom q;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q.ql[c] = (double)a.qloc[bq * 3 + c];
    q.qd[c] = (double)a.qbox[bq * 6 + 3 + c] - (double)a.qbox[bq * 6 + c];
  }
  return q;
}

template <int C>
__global__ __launch_bounds__(kThreads) void k_dyco_forward(DyArgs a) {
  using D = Dy<C>;
  __shared__ float w[D::NW];
  __shared__ double tiles[kWaves][D::XT];
  const int b = blockIdx.x / a.Q, q = blockIdx.x % a.Q;
  const long long n_first = a.off[b], n_end = a.off[b + 1], nb = n_end - n_first;
  if (nb <= 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
  const long long bq = (long long)b * a.Q + q;
  load_weights<C>(a.theta + bq * D::P, w);
  const QueryGeom qg = query_geom(a, bq);
  float* __restrict__ y = a.y + (n_first - a.off[0]) * a.Q + (long long)q * nb;
  double* xt = tiles[wave];
  const long long n_tiles = (nb + kTile - 1) / kTile;
  for (long long t0 = 0; t0 < n_tiles; t0 += kWaves) {  // the same trip count in every wave: the barriers are uniform
    const long long tile = t0 + wave, n0 = n_first + tile * kTile;
    __syncthreads();
    if (tile < n_tiles) {
      build_features<C>(xt, a.feat, a.ld_feat, n0, n_end, lane);
      build_geometry<C>(xt, a.locs, a.box, qg.ql, qg.qd, n0, n_end, lane);
    }
    __syncthreads();
    if (tile < n_tiles) {
      d4 h1[D::JB], h2;
      layers<C>(w, xt, g, i, h1, h2);
      double part = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) part += (double)w[D::lW3 + g + 4 * r] * h2[r];
      part += shfl_xor(part, 16);
      part += shfl_xor(part, 32);
      if (g == 0 && n0 + i < n_end) y[tile * kTile + i] = (float)part;
    }
  }
}

template <int C>
__global__ __launch_bounds__(kThreads) void k_dyco_backward_queries(DyArgs a) {
  using D = Dy<C>;
  constexpr int kT0 = D::XT, kT2 = kT0 + C * kLd, kWaveLds = kT2 + 16 * kLd;  // x | h1, then dh1 | dh2
  static_assert(kWaves * kWaveLds >= D::P + 3, "the wave sums overlay the tiles");
  __shared__ float w[D::NW];
  __shared__ double lds[kWaves * kWaveLds];
  const int b = blockIdx.x / a.Q, q = blockIdx.x % a.Q;
  const long long n_first = a.off[b], n_end = a.off[b + 1], nb = n_end - n_first > 0 ? n_end - n_first : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
  const long long bq = (long long)b * a.Q + q;
  load_weights<C>(a.theta + bq * D::P, w);
  const QueryGeom qg = query_geom(a, bq);
  const float* __restrict__ gy = a.gy + (n_first - a.off[0]) * a.Q + (long long)q * nb;
  double *xt = lds + wave * kWaveLds, *t0 = xt + kT0, *t2 = xt + kT2;

  d4 dW1[D::JB][D::AB], dW2[D::JB];  // rotated layout until the end
#pragma unroll
  for (int jb = 0; jb < D::JB; ++jb) {
    dW2[jb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ab = 0; ab < D::AB; ++ab) dW1[jb][ab] = d4{0.0, 0.0, 0.0, 0.0};
  }
  d4 db1[D::JB], db2 = {0.0, 0.0, 0.0, 0.0}, dw3 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int jb = 0; jb < D::JB; ++jb) db1[jb] = d4{0.0, 0.0, 0.0, 0.0};
  double dq = 0.0;

  const long long n_tiles = (nb + kTile - 1) / kTile;
  for (long long tt = 0; tt < n_tiles; tt += kWaves) {
    const long long tile = tt + wave, n0 = n_first + tile * kTile;
    const bool live = tile < n_tiles;
    __syncthreads();
    if (live) {
      build_features<C>(xt, a.feat, a.ld_feat, n0, n_end, lane);
      build_geometry<C>(xt, a.locs, a.box, qg.ql, qg.qd, n0, n_end, lane);
    }
    __syncthreads();
    d4 h1[D::JB], h2, dh2, dh1[D::JB];
    if (live) {
      layers<C>(w, xt, g, i, h1, h2);
      const double gyn = n0 + i < n_end ? (double)gy[tile * kTile + i] : 0.0;
      hidden_grads<C>(w, gyn, g, i, h1, h2, dh2, dh1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dw3[r] += gyn * h2[r];
        db2[r] += dh2[r];
        t2[(g + 4 * r) * kLd + i] = dh2[r];
#pragma unroll
        for (int jb = 0; jb < D::JB; ++jb) {
          db1[jb][r] += dh1[jb][r];
          t0[(jb * 16 + g + 4 * r) * kLd + i] = h1[jb][r];
        }
      }
      if (a.d_qbox) {
        d4 dxg = {0.0, 0.0, 0.0, 0.0};
        input_grad_block<C>(w, D::JB, g, i, dh1, dxg);
        dq += box_term<C>(xt, g, i, unrotate(dxg));
      }
    }
    __syncthreads();
    if (live) {  // dW2[k][j] += sum_n dh2[k][n] h1[j][n]
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double av = t2[i * kLd + 4 * s + g];
#pragma unroll
        for (int jb = 0; jb < D::JB; ++jb) mma16(av, t0[(jb * 16 + i) * kLd + 4 * s + g], dW2[jb]);
      }
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int jb = 0; jb < D::JB; ++jb) t0[(jb * 16 + g + 4 * r) * kLd + i] = dh1[jb][r];
    }
    __syncthreads();
    if (live) {  // dW1[a][j] += sum_n dh1[j][n] x[a][n]
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int jb = 0; jb < D::JB; ++jb) {
          const double av = t0[(jb * 16 + i) * kLd + 4 * s + g];
#pragma unroll
          for (int ab = 0; ab < D::AB; ++ab) mma16(av, xt[(ab * 16 + i) * kLd + 4 * s + g], dW1[jb][ab]);
        }
    }
  }

  // the sums over a tile's 16 points that the lanes hold apart
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dw3[r] = sum16(dw3[r]);
    db2[r] = sum16(db2[r]);
#pragma unroll
    for (int jb = 0; jb < D::JB; ++jb) db1[jb][r] = sum16(db1[jb][r]);
  }
  dq = sum16(dq);
  // the four waves, in wave order, into the controller row's own order: R[P] and the three box-dimension sums
  double* R = lds;
  const int cb = box_channel(g);
  for (int wv = 0; wv < kWaves; ++wv) {
    __syncthreads();
    if (wave != wv) continue;
    const bool first = wv == 0;
#pragma unroll
    for (int jb = 0; jb < D::JB; ++jb) {
#pragma unroll
      for (int ab = 0; ab < D::AB; ++ab) {
        const d4 v = unrotate(dW1[jb][ab]);
        const int ap = ab * 16 + i;
        if (ap < D::K) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int at = channel_of<C>(ap) * C + jb * 16 + g + 4 * r;
            R[at] = (first ? 0.0 : R[at]) + v[r];
          }
        }
      }
      const d4 v2 = unrotate(dW2[jb]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = g + 4 * r;
        if (k < D::H) {
          const int at = D::oW2 + (jb * 16 + i) * D::H + k;
          R[at] = (first ? 0.0 : R[at]) + v2[r];
        }
      }
    }
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = g + 4 * r;
#pragma unroll
        for (int jb = 0; jb < D::JB; ++jb) {
          const int at = D::ob1 + jb * 16 + k;
          R[at] = (first ? 0.0 : R[at]) + db1[jb][r];
        }
        if (k < D::H) {
          R[D::oW3 + k] = (first ? 0.0 : R[D::oW3 + k]) + dw3[r];
          R[D::ob2 + k] = (first ? 0.0 : R[D::ob2 + k]) + db2[r];
        }
      }
      if (cb >= 0) R[D::P + cb] = (first ? 0.0 : R[D::P + cb]) + dq;
    }
  }
  __syncthreads();
  if (a.d_theta) {
    float* __restrict__ out = a.d_theta + bq * D::P;
    for (int p = threadIdx.x; p < D::P; p += kThreads) out[p] = p == D::ob3 ? 0.f : (float)R[p];
  }
  if (a.d_qbox && threadIdx.x < 6) {  // d(max) = +sum, d(min) = -sum
    const double v = R[D::P + threadIdx.x % 3];
    a.d_qbox[bq * 6 + threadIdx.x] = (float)(threadIdx.x < 3 ? 0.0 - v : v);
  }
}

template <int C>
__global__ __launch_bounds__(kThreads) void k_dyco_backward_points(DyArgs a) {
  using D = Dy<C>;
  __shared__ float w[D::NW];
  __shared__ double tiles[kWaves][D::XT];
  int b = 0;
  while (b + 1 < a.B && (int)blockIdx.x >= a.tile_first[b + 1]) ++b;
  const long long n_first = a.off[b], n_end = a.off[b + 1], nb = n_end - n_first;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
  const long long n0 = n_first + ((long long)blockIdx.x - a.tile_first[b]) * kPointTile + wave * kTile;
  const bool live = n0 < n_end;  // a wave beyond the sample's end keeps the barriers company
  const float* __restrict__ gy = a.gy + (n_first - a.off[0]) * a.Q + (n0 - n_first);
  double* xt = tiles[wave];
  if (live) build_features<C>(xt, a.feat, a.ld_feat, n0, n_end, lane);
  d4 dxf[D::JB];
#pragma unroll
  for (int jb = 0; jb < D::JB; ++jb) dxf[jb] = d4{0.0, 0.0, 0.0, 0.0};
  double dp = 0.0;
  WeightRegs<C> next;
  next.fetch(a.theta + (long long)b * a.Q * D::P);
  for (int q = 0; q < a.Q; ++q) {
    const long long bq = (long long)b * a.Q + q;
    __syncthreads();  // every wave has left query q - 1
    next.store(w);
    if (live) {
      const QueryGeom qg = query_geom(a, bq);
      build_geometry<C>(xt, a.locs, a.box, qg.ql, qg.qd, n0, n_end, lane);
    }
    __syncthreads();
    const double gyn = live && n0 + i < n_end ? (double)gy[(long long)q * nb + i] : 0.0;
    if (q + 1 < a.Q) next.fetch(a.theta + (bq + 1) * D::P);  // in flight under this query's products
    if (live) {
      d4 h1[D::JB], h2, dh2, dh1[D::JB];
      layers<C>(w, xt, g, i, h1, h2);
      hidden_grads<C>(w, gyn, g, i, h1, h2, dh2, dh1);
      if (a.d_feat) {
#pragma unroll
        for (int ab = 0; ab < D::JB; ++ab) input_grad_block<C>(w, ab, g, i, dh1, dxf[ab]);
      }
      if (a.d_box) {
        d4 dxg = {0.0, 0.0, 0.0, 0.0};
        input_grad_block<C>(w, D::JB, g, i, dh1, dxg);
        dp += box_term<C>(xt, g, i, unrotate(dxg));
      }
    }
  }
  const long long p = n0 + i;
  if (!live || p >= n_end) return;
  if (a.d_feat) {
#pragma unroll
    for (int ab = 0; ab < D::JB; ++ab) {
      const d4 v = unrotate(dxf[ab]);
#pragma unroll
      for (int r = 0; r < 4; ++r) a.d_feat[p * C + ab * 16 + g + 4 * r] = (float)v[r];
    }
  }
  const int cb = box_channel(g);
  if (a.d_box && cb >= 0) {  // d = q_dim - (max - min): d(min) = +sum, d(max) = -sum
    a.d_box[p * 6 + cb] = (float)dp;
    a.d_box[p * 6 + 3 + cb] = (float)(0.0 - dp);
  }
}

bool fill_args(DyArgs* a, int B, int Q, int C, const int64_t* h_off, long long n_points) {
  if (B < 1 || B > kMaxBatch || Q < 1 || (C != 16 && C != 32) || !h_off || n_points < 0) return false;
  if ((long long)B * Q > 0x7fffffffLL) return false;
  if (h_off[0] < 0 || h_off[B] > n_points) return false;
  long long tiles = 0;
  for (int b = 0; b < B; ++b) {
    if (h_off[b + 1] < h_off[b]) return false;
    a->off[b] = h_off[b];
    a->tile_first[b] = (int)tiles;
    tiles += (h_off[b + 1] - h_off[b] + kPointTile - 1) / kPointTile;
    if (tiles > 0x7fffffffLL) return false;
  }
  a->off[B] = h_off[B];
  a->tile_first[B] = (int)tiles;
  a->B = B;
  a->Q = Q;
  return true;
}

}  // namespace

extern "C" {

int64_t gapro_dyco_param_count(int32_t mask_dim_out) {
  if (mask_dim_out == 32) return Dy<32>::P;
  if (mask_dim_out == 16) return Dy<16>::P;
  return 0;
}

size_t gapro_dyco_workspace_bytes(int32_t, int32_t, int64_t, int32_t) { return 0; }

int gapro_dyco_forward(gapro_ctx* ctx, void* stream_, int32_t n_batches, int32_t n_queries, int32_t mask_dim_out,
                       const int64_t* h_batch_offsets, int64_t n_points, const float* d_controllers,
                       const float* d_mask_features, int64_t ld_features, const float* d_locs_float,
                       const float* d_box_preds, const float* d_queries_locs, const float* d_queries_box_preds,
                       void* d_workspace, size_t workspace_bytes, float* d_mask_logits) {
  (void)d_workspace;
  (void)workspace_bytes;
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  DyArgs a{};
  if (!fill_args(&a, n_batches, n_queries, mask_dim_out, h_batch_offsets, n_points) || !d_controllers ||
      !d_queries_locs || !d_queries_box_preds || ld_features < mask_dim_out)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_dyco_forward: bad argument");
  if (a.off[n_batches] == a.off[0]) return GAPRO_OK;  // no point: no output
  if (!d_mask_features || !d_locs_float || !d_box_preds || !d_mask_logits)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_dyco_forward: bad argument");
  a.theta = d_controllers;
  a.feat = d_mask_features;
  a.ld_feat = ld_features;
  a.locs = d_locs_float;
  a.box = d_box_preds;
  a.qloc = d_queries_locs;
  a.qbox = d_queries_box_preds;
  a.y = d_mask_logits;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)(n_batches * n_queries));
  if (mask_dim_out == 32) hipLaunchKernelGGL(k_dyco_forward<32>, grid, dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(k_dyco_forward<16>, grid, dim3(kThreads), 0, stream, a);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_dyco_backward(gapro_ctx* ctx, void* stream_, int32_t n_batches, int32_t n_queries, int32_t mask_dim_out,
                        const int64_t* h_batch_offsets, int64_t n_points, const float* d_controllers,
                        const float* d_mask_features, int64_t ld_features, const float* d_locs_float,
                        const float* d_box_preds, const float* d_queries_locs, const float* d_queries_box_preds,
                        const float* d_grad_logits, void* d_workspace, size_t workspace_bytes,
                        float* d_grad_controllers, float* d_grad_queries_box_preds, float* d_grad_mask_features,
                        float* d_grad_box_preds) {
  (void)d_workspace;
  (void)workspace_bytes;
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  DyArgs a{};
  if (!fill_args(&a, n_batches, n_queries, mask_dim_out, h_batch_offsets, n_points) || !d_controllers ||
      !d_queries_locs || !d_queries_box_preds || ld_features < mask_dim_out)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_dyco_backward: bad argument");
  const bool any = a.off[n_batches] > a.off[0];
  if (any && (!d_mask_features || !d_locs_float || !d_box_preds || !d_grad_logits))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_dyco_backward: bad argument");
  a.theta = d_controllers;
  a.feat = d_mask_features;
  a.ld_feat = ld_features;
  a.locs = d_locs_float;
  a.box = d_box_preds;
  a.qloc = d_queries_locs;
  a.qbox = d_queries_box_preds;
  a.gy = d_grad_logits;
  a.d_theta = d_grad_controllers;
  a.d_qbox = d_grad_queries_box_preds;
  a.d_feat = d_grad_mask_features;
  a.d_box = d_grad_box_preds;
  hipStream_t stream = (hipStream_t)stream_;
  if (d_grad_controllers || d_grad_queries_box_preds) {  // a sample without points writes its zeros here too
    const dim3 grid((unsigned)(n_batches * n_queries));
    if (mask_dim_out == 32) hipLaunchKernelGGL(k_dyco_backward_queries<32>, grid, dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(k_dyco_backward_queries<16>, grid, dim3(kThreads), 0, stream, a);
  }
  if (d_grad_mask_features || d_grad_box_preds) {
    // the points no sample owns: rows [0, off[0]) and [off[B], n_points)
    const long long lo = a.off[0], hi = a.off[n_batches];
    if (d_grad_mask_features) {
      const size_t row = (size_t)mask_dim_out * sizeof(float);
      if (lo > 0) GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_grad_mask_features, 0, (size_t)lo * row, stream));
      if (hi < n_points)
        GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_grad_mask_features + hi * mask_dim_out, 0, (size_t)(n_points - hi) * row,
                                            stream));
    }
    if (d_grad_box_preds) {
      const size_t row = 6 * sizeof(float);
      if (lo > 0) GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_grad_box_preds, 0, (size_t)lo * row, stream));
      if (hi < n_points)
        GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_grad_box_preds + hi * 6, 0, (size_t)(n_points - hi) * row, stream));
    }
    if (any) {
      const dim3 grid((unsigned)a.tile_first[n_batches]);
      if (mask_dim_out == 32) hipLaunchKernelGGL(k_dyco_backward_points<32>, grid, dim3(kThreads), 0, stream, a);
      else hipLaunchKernelGGL(k_dyco_backward_points<16>, grid, dim3(kThreads), 0, stream, a);
    }
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
