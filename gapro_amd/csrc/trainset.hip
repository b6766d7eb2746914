// Training-set assembly of point-level GP fits (gapro_trainset_count / gapro_trainset_fill): every problem of a
// batch through one launch per kernel, the rows written straight into the table the fit launch reads.
//
// Replaces reference gapro/gaussian_process_utils.py:36-76 (fit_gp): the pooling of each side's points to superpoint
// means (:64-69, torch.unique + torch_scatter mean) and the npoint_nearest points of each side nearest to the
// intersection's centroid (:39, :49-62, torch.topk).  Both deviate from the reference where the reference is not
// reproducible: the sums are exact int64 sums of fixed-point terms (integer atomics, any order gives
// the same bits; no float atomic anywhere in this file), and the selection orders by (distance, position in the
// side's list) where torch.topk leaves ties open.
//
// A batch is ragged (sides of 1 .. 1e5 points): grid.y = (problem, side), grid.x strides over the side's list, and a
// workgroup whose share of a short list is empty leaves at once.
#include "common.h"
#include "exact_sum.h"
#include "launch_util.h"
#include "scan.h"
#include "wave_reduce.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kSelThreads = 1024;  // one workgroup per (problem, side) in the selection kernel
constexpr int kMaxNearest = GAPRO_TRAINSET_MAX_NEAREST;  // survivors are ordered in LDS
static_assert(kSelThreads == kMaxNearest, "k_ts_nearest orders one survivor per thread");
static_assert(kThreads == kScanThreads, "k_ts_rank calls block_exclusive");

static_assert(sizeof(gapro_trainset_desc) == 40, "gapro_trainset_desc layout is part of the ABI (ctypes mirror)");

struct SideRef {
  const int* list;  // the side's point indices
  int n;            // their number
  int m;            // rows of the side in the table
  long long row0;   // its first row
  int prob;
};

__device__ inline SideRef side_of(const gapro_trainset_desc* __restrict__ descs, const int* __restrict__ idx, int side) {
  const gapro_trainset_desc& d = descs[side >> 1];
  SideRef s;
  s.prob = side >> 1;
  if (side & 1) {
    s.list = idx + d.idx_offset + d.n1; s.n = d.n2; s.m = d.m2; s.row0 = d.row_offset + d.m1;
  } else {
    s.list = idx + d.idx_offset; s.n = d.n1; s.m = d.m1; s.row0 = d.row_offset;
  }
  return s;
}

// a point index outside [0, n_points) is reported (BAD_ARG) and read as point 0, so that nothing leaves the arrays
__device__ inline int checked_point(int p, long long n_points, int* status) {
  if ((unsigned long long)(long long)p >= (unsigned long long)n_points) {
    *status = GAPRO_ERR_BAD_ARG;
    return 0;
  }
  return p;
}

// ---- pool, pass 1: which superpoints does a side touch, and their ascending ranks ---------------------------------
__global__ __launch_bounds__(kThreads) void k_ts_mark(const gapro_trainset_desc* __restrict__ descs,
                                                      const int* __restrict__ idx, const int* __restrict__ spp_inv,
                                                      long long n_points, int n_spps, int* __restrict__ marks,
                                                      int* __restrict__ status) {
  const SideRef s = side_of(descs, idx, blockIdx.y);
  int* __restrict__ mk = marks + (long long)blockIdx.y * n_spps;
  const int stride = gridDim.x * kThreads;
  for (int j = blockIdx.x * kThreads + threadIdx.x; j < s.n; j += stride) {
    const int p = checked_point(s.list[j], n_points, &status[s.prob]);
    const int r = spp_inv[p];
    if ((unsigned)r < (unsigned)n_spps) mk[r] = 1;
    else status[s.prob] = GAPRO_ERR_BAD_ARG;
  }
}

// marks -> 1 + rank among the side's superpoints (0 = not in the side); counts[side] = their number
__global__ __launch_bounds__(kThreads) void k_ts_rank(int n_spps, int* __restrict__ marks, int* __restrict__ counts) {
  int* __restrict__ mk = marks + (long long)blockIdx.x * n_spps;
  __shared__ int wave_tot[kScanWaves];
  int carry = 0;
  for (int b0 = 0; b0 < n_spps; b0 += kThreads) {  // uniform
    const int i = b0 + threadIdx.x;
    const int v = i < n_spps ? mk[i] : 0;
    int tot;
    const int before = block_exclusive(v, wave_tot, &tot);
    if (i < n_spps) mk[i] = v ? carry + before + v : 0;
    carry += tot;
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// ---- pool, pass 2: exact sums per (side, superpoint) --------------------------------------------------------------
// Eight lanes per point, as k_pool (partition.hip): lane k adds features k, k + 8, ..., lane D % 8 the count.  The
// eight points of a wave usually share a superpoint: their terms are then summed by shuffles first.
__global__ __launch_bounds__(kThreads) void k_ts_accum(const gapro_trainset_desc* __restrict__ descs,
                                                       const int* __restrict__ idx, const int* __restrict__ spp_inv,
                                                       const long long* __restrict__ spp, const float* __restrict__ feats,
                                                       long long n_points, int n_spps, int d, int shift,
                                                       const int* __restrict__ marks,
                                                       unsigned long long* __restrict__ sums, int* __restrict__ cnt,
                                                       long long* __restrict__ sel, long long n_rows,
                                                       int* __restrict__ status) {
  const SideRef s = side_of(descs, idx, blockIdx.y);
  const int* __restrict__ mk = marks + (long long)blockIdx.y * n_spps;
  const int k = threadIdx.x & (kLanesPerPoint - 1);
  const int ppb = kThreads / kLanesPerPoint;
  const int stride = gridDim.x * ppb;
  for (int j = blockIdx.x * ppb + threadIdx.x / kLanesPerPoint; j < s.n; j += stride) {
    const int p = checked_point(s.list[j], n_points, &status[s.prob]);
    const int r = spp_inv[p];
    const int rank = (unsigned)r < (unsigned)n_spps ? mk[r] - 1 : -1;
    long long row = -1;
    if (rank >= 0 && rank < s.m && s.row0 + rank < n_rows) row = s.row0 + rank;
    else status[s.prob] = GAPRO_ERR_BAD_ARG;  // row counts that are not this side's (gapro_trainset_count)
    const float* f = feats + (long long)p * d;
    const int j_first = __shfl(j, 0, 64);
    const bool full_wave = j_first + 64 / kLanesPerPoint - 1 < s.n;
    const bool one_row = full_wave && __all(row >= 0 && row == __shfl(row, 0, 64));
    if (one_row) {
      const bool head = (threadIdx.x & 63) < kLanesPerPoint;
      if (head && k == (d & (kLanesPerPoint - 1))) {
        atomicAdd(&cnt[row], 64 / kLanesPerPoint);
        sel[row] = spp[p];
      }
      accumulate_features_wave8(sums + row * d, f, d, k, shift, head);
    } else if (row >= 0) {
      if (k == (d & (kLanesPerPoint - 1))) {
        atomicAdd(&cnt[row], 1);
        sel[row] = spp[p];  // every writer of a row holds the same id
      }
      accumulate_features(sums + row * d, f, d, k, shift);
    }
  }
}

// mean = fixed_mean (exact_sum.h), rounded once to float32; an empty row's count is clamped at 1 as in k_pool_finalize
__global__ __launch_bounds__(kThreads) void k_ts_pool_finalize(long long n_rows, int d, int shift,
                                                               const long long* __restrict__ sums,
                                                               const int* __restrict__ cnt, float* __restrict__ train) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_rows * d) return;
  const int c = cnt[i / d];
  train[i] = (float)fixed_mean(sums[i], shift, (double)(c > 0 ? c : 1));
}

// ---- nearest: the intersection's centroid as exact fixed-point sums -----------------------------------------------
// Largest |coordinate| among the FINITE coordinates of the input, as the bit pattern of a non-negative double (orders as
// an integer): the scale of the centroid's fixed-point sums must not depend on a non-finite coordinate somewhere in the
// input (the scene header's range does: an infinite coordinate would round every problem's terms to integers).
__global__ __launch_bounds__(kThreads) void k_ts_coord_absmax(const double* __restrict__ coords, long long n3,
                                                              unsigned long long* __restrict__ amax_bits) {
  double m = 0.0;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n3; i += stride) {
    const double v = fabs(coords[i]);
    if (isfinite(v)) m = fmax(m, v);
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.0) atomicMax(amax_bits, (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(kThreads) void k_ts_centroid(const gapro_trainset_desc* __restrict__ descs,
                                                          const int* __restrict__ idx, const double* __restrict__ coords,
                                                          long long n_points,
                                                          const unsigned long long* __restrict__ amax_bits,
                                                          unsigned long long* __restrict__ csum, int* __restrict__ status) {
  const gapro_trainset_desc& ds = descs[blockIdx.y];
  const int coord_shift = fixed_point_shift(__longlong_as_double((long long)*amax_bits), n_points);
  const int* __restrict__ list = idx + ds.idx_offset + ds.n1 + ds.n2;
  const int t = ds.t;
  if (blockIdx.x * kThreads >= t) return;
  long long a[3] = {0, 0, 0};
  const int stride = gridDim.x * kThreads;
  for (int j = blockIdx.x * kThreads + threadIdx.x; j < t; j += stride) {
    const int p = checked_point(list[j], n_points, &status[blockIdx.y]);
    const double x = coords[3LL * p], y = coords[3LL * p + 1], z = coords[3LL * p + 2];
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      a[0] += to_fixed(x, coord_shift);
      a[1] += to_fixed(y, coord_shift);
      a[2] += to_fixed(z, coord_shift);
    } else {
      status[blockIdx.y] = GAPRO_ERR_NOT_FINITE;
    }
  }
  __shared__ long long sh[kThreads / 64][3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int c = 0; c < 3; ++c) a[c] = wave_sum(a[c]);
  if (lane == 0) for (int c = 0; c < 3; ++c) sh[w][c] = a[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    long long v = 0;
    for (int j = 0; j < kThreads / 64; ++j) v += sh[j][threadIdx.x];
    atomicAdd(&csum[3LL * blockIdx.y + threadIdx.x], (unsigned long long)v);
  }
}

// ---- nearest: the k points of a side nearest to the centroid, ordered by (distance, position) ---------------------
// The distance is recomputed from the coordinates in every pass (no array per side): (dx dx + dy dy) + dz dz with every
// operation rounded on its own: contraction into FMAs is switched off for the function (the __dmul_rn / __dadd_rn forms
// are inlined with the translation unit's contraction setting and do get fused).  A non-negative double orders as its
// 64-bit pattern.
__device__ inline unsigned long long dist_key(const double* __restrict__ coords, int p, double cx, double cy, double cz) {
#pragma clang fp contract(off)
  const double dx = coords[3LL * p] - cx, dy = coords[3LL * p + 1] - cy, dz = coords[3LL * p + 2] - cz;
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double dd = (xx + yy) + zz;
  return (unsigned long long)__double_as_longlong(dd);
}

__global__ __launch_bounds__(kSelThreads) void k_ts_nearest(const gapro_trainset_desc* __restrict__ descs,
                                                            const int* __restrict__ idx, const double* __restrict__ coords,
                                                            const float* __restrict__ feats, long long n_points, int d,
                                                            int k_near, const unsigned long long* __restrict__ amax_bits,
                                                            const long long* __restrict__ csum, float* __restrict__ train,
                                                            long long* __restrict__ sel, long long n_rows,
                                                            int* __restrict__ status) {
  const SideRef s = side_of(descs, idx, blockIdx.x);
  const int t = descs[s.prob].t;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kk = s.n < k_near ? s.n : k_near;  // rows this side fills
  __shared__ unsigned long long s_key[kMaxNearest];
  __shared__ unsigned s_pos[kMaxNearest];
  __shared__ int s_pt[kMaxNearest];
  __shared__ unsigned hist[256];
  __shared__ unsigned wcnt[kSelThreads / 64];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_remaining, s_nlt;
  if (kk != s.m || kk > kMaxNearest || s.row0 < 0 || s.row0 + kk > n_rows) {  // rows that are not this side's
    if (tid == 0) status[s.prob] = GAPRO_ERR_BAD_ARG;
    return;
  }
  s_pt[tid] = 0;  // kSelThreads == kMaxNearest: every slot holds a valid point whatever follows
  __syncthreads();
  if (s.n <= k_near) {  // the side as it is given
    for (int j = tid; j < s.n; j += kSelThreads) {
      const int p = checked_point(s.list[j], n_points, &status[s.prob]);
      if (!(isfinite(coords[3LL * p]) && isfinite(coords[3LL * p + 1]) && isfinite(coords[3LL * p + 2])))
        status[s.prob] = GAPRO_ERR_NOT_FINITE;
      s_pt[j] = p;
    }
  } else {
    double cx = 0.0, cy = 0.0, cz = 0.0;
    const int coord_shift = fixed_point_shift(__longlong_as_double((long long)*amax_bits), n_points);
    if (t > 0) {
      cx = fixed_mean(csum[3LL * s.prob], coord_shift, (double)t);
      cy = fixed_mean(csum[3LL * s.prob + 1], coord_shift, (double)t);
      cz = fixed_mean(csum[3LL * s.prob + 2], coord_shift, (double)t);
    } else if (tid == 0) {
      status[s.prob] = GAPRO_ERR_BAD_ARG;  // no centroid
    }
    // radix select, eight bits a pass from the top: the pattern V of the k-th smallest distance, and how many of the
    // distances equal to V belong to the k
    unsigned long long prefix = 0;
    unsigned remaining = (unsigned)k_near;
    for (int pass = 7; pass >= 0; --pass) {
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      const int sh_hi = 8 * (pass + 1);
      for (int j = tid; j < s.n; j += kSelThreads) {
        const int p = checked_point(s.list[j], n_points, &status[s.prob]);
        if (pass == 7 && !(isfinite(coords[3LL * p]) && isfinite(coords[3LL * p + 1]) && isfinite(coords[3LL * p + 2])))
          status[s.prob] = GAPRO_ERR_NOT_FINITE;
        const unsigned long long key = dist_key(coords, p, cx, cy, cz);
        if (pass == 7 || (key >> sh_hi) == (prefix >> sh_hi)) atomicAdd(&hist[(unsigned)(key >> (8 * pass)) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned acc = 0, b = 0;
        for (; b < 255u; ++b) {
          if (acc + hist[b] >= remaining) break;
          acc += hist[b];
        }
        s_prefix = prefix | ((unsigned long long)b << (8 * pass));
        s_remaining = remaining - acc;
        s_nlt = 0u;
      }
      __syncthreads();
      prefix = s_prefix;
      remaining = s_remaining;
    }
    const unsigned long long V = prefix;
    const unsigned r_eq = remaining, n_less = (unsigned)k_near - r_eq;
    // collect: every distance below V (any order), and of those equal to V the first r_eq by position
    unsigned eq_carry = 0;
    for (int base = 0; base < s.n; base += kSelThreads) {
      const int j = base + tid;
      unsigned long long key = ~0ull;
      if (j < s.n) key = dist_key(coords, checked_point(s.list[j], n_points, &status[s.prob]), cx, cy, cz);
      const bool lt = j < s.n && key < V, eq = j < s.n && key == V;
      if (lt) {
        const unsigned slot = atomicAdd(&s_nlt, 1u);
        if (slot < n_less) { s_key[slot] = key; s_pos[slot] = (unsigned)j; }
      }
      const unsigned long long bal = __ballot(eq);
      if (lane == 0) wcnt[w] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned before = eq_carry, tot = 0;
      for (int q = 0; q < kSelThreads / 64; ++q) {
        if (q < w) before += wcnt[q];
        tot += wcnt[q];
      }
      const unsigned off = before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
      if (eq && off < r_eq) { s_key[n_less + off] = key; s_pos[n_less + off] = (unsigned)j; }
      eq_carry += tot;
      __syncthreads();
    }
    // order the k survivors by (distance, position): each counts those ahead of it
    if (tid < k_near) {
      const unsigned long long key = s_key[tid];
      const unsigned pos = s_pos[tid] < (unsigned)s.n ? s_pos[tid] : 0u;
      int rank = 0;
      for (int q = 0; q < k_near; ++q) {
        const unsigned long long kq = s_key[q];
        rank += (kq < key) | ((kq == key) & (s_pos[q] < pos));
      }
      s_pt[rank] = checked_point(s.list[pos], n_points, &status[s.prob]);
    }
  }
  __syncthreads();
  for (int r = tid; r < kk; r += kSelThreads) sel[s.row0 + r] = s_pt[r];
  for (int e = tid; e < kk * d; e += kSelThreads) {
    const int r = e / d, c = e - r * d;
    const float v = feats[(long long)s_pt[r] * d + c];
    if (!isfinite(v)) status[s.prob] = GAPRO_ERR_NOT_FINITE;
    train[(s.row0 + r) * d + c] = v;
  }
}

struct Plan {
  size_t marks = 0, sums = 0, cnt = 0, csum = 0, total = 0;  // byte offsets of the regions, and the size
  long long rows_cap = 0;
  int n_max = 1, t_max = 1;
};

// pool: marks i32[2 P S] | sums i64[R D] | counts i32[R], R = sum over the sides of min(n, S) >= the rows of any
// outcome of the count; nearest: centroid sums i64[3 P] | max |finite coordinate| u64
bool plan(int mode, const gapro_trainset_desc* h, int n_problems, int n_spps, int d, Plan* out) {
  if (!h || n_problems <= 0 || n_problems > GAPRO_TRAINSET_MAX_PROBLEMS || d <= 0 || (mode == GAPRO_TRAINSET_POOL && n_spps <= 0)) return false;
  Plan p;
  for (int i = 0; i < n_problems; ++i) {
    if (h[i].n1 <= 0 || h[i].n2 <= 0 || h[i].t < 0 || h[i].idx_offset < 0) return false;
    p.rows_cap += std::min(h[i].n1, n_spps) + std::min(h[i].n2, n_spps);
    p.n_max = std::max(p.n_max, std::max(h[i].n1, h[i].n2));
    p.t_max = std::max(p.t_max, h[i].t);
  }
  if (mode == GAPRO_TRAINSET_POOL) {
    p.marks = 0;
    p.sums = align_up((size_t)2 * n_problems * n_spps * sizeof(int), 256);
    p.cnt = p.sums + align_up((size_t)p.rows_cap * d * sizeof(long long), 256);
    p.total = p.cnt + align_up((size_t)p.rows_cap * sizeof(int), 256);
  } else {
    p.total = align_up((size_t)(3 * n_problems + 1) * sizeof(long long), 256);
  }
  *out = p;
  return true;
}

}  // namespace

extern "C" {

size_t gapro_trainset_workspace_bytes(int32_t mode, const gapro_trainset_desc* h_descs, int32_t n_problems,
                                      int32_t n_spps, int32_t feat_dim) {
  Plan p;
  if ((mode != GAPRO_TRAINSET_POOL && mode != GAPRO_TRAINSET_NEAREST) ||
      !plan(mode, h_descs, n_problems, n_spps, feat_dim, &p))
    return 0;
  return p.total;
}

int gapro_trainset_count(gapro_ctx* ctx, void* stream_, int32_t n_problems, int32_t feat_dim,
                         const gapro_trainset_desc* h_descs, gapro_trainset_desc* d_descs, int64_t n_points,
                         int32_t n_spps, const int32_t* d_spp_inv, const int32_t* d_idx, void* d_workspace,
                         size_t workspace_bytes, int32_t* d_counts, int32_t* d_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  Plan p;
  if (!plan(GAPRO_TRAINSET_POOL, h_descs, n_problems, n_spps, feat_dim, &p) || !d_descs || n_points <= 0 ||
      !d_spp_inv || !d_idx || !d_workspace || !d_counts || !d_status)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_trainset_count: bad argument");
  if (workspace_bytes < p.total)
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_trainset_count: workspace too small (%zu > %zu)", p.total,
                      workspace_bytes);
  hipStream_t stream = (hipStream_t)stream_;
  int* marks = (int*)((char*)d_workspace + p.marks);
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_descs, h_descs, (size_t)n_problems * sizeof(gapro_trainset_desc),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(marks, 0, (size_t)2 * n_problems * n_spps * sizeof(int), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, (size_t)n_problems * sizeof(int), stream));
  const unsigned ny = 2u * (unsigned)n_problems;
  hipLaunchKernelGGL(k_ts_mark, dim3(grid_for(p.n_max, 4, 128), ny), dim3(kThreads), 0, stream, d_descs, d_idx,
                     d_spp_inv, (long long)n_points, (int)n_spps, marks, d_status);
  hipLaunchKernelGGL(k_ts_rank, dim3(ny), dim3(kThreads), 0, stream, (int)n_spps, marks, d_counts);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_trainset_fill(gapro_ctx* ctx, void* stream_, int32_t mode, int32_t n_problems, int32_t feat_dim,
                        const gapro_trainset_desc* h_descs, gapro_trainset_desc* d_descs, int64_t n_points,
                        int32_t n_spps, const double* d_coords, const float* d_feats, const int64_t* d_spp,
                        const int32_t* d_spp_inv, int32_t fixed_shift, int32_t npoint_nearest, const int32_t* d_idx,
                        void* d_workspace, size_t workspace_bytes, int64_t n_rows, float* d_train, int64_t* d_sel,
                        int32_t* d_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  Plan p;
  const bool pool = mode == GAPRO_TRAINSET_POOL;
  if ((!pool && mode != GAPRO_TRAINSET_NEAREST) || !plan(mode, h_descs, n_problems, n_spps, feat_dim, &p) || !d_descs ||
      n_points <= 0 || !d_feats || !d_idx || !d_workspace || !d_train || !d_sel || !d_status || n_rows <= 0 ||
      (pool ? (!d_spp || !d_spp_inv) : (!d_coords || npoint_nearest < 1 || npoint_nearest > kMaxNearest)))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_trainset_fill: bad argument");
  if (workspace_bytes < p.total)
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_trainset_fill: workspace too small (%zu > %zu)", p.total,
                      workspace_bytes);
  for (int i = 0; i < n_problems; ++i) {  // every problem's rows inside the table (the kernels check each side again)
    const gapro_trainset_desc& d = h_descs[i];
    const bool rows_ok = pool ? (d.m1 >= 1 && d.m2 >= 1 && d.m1 <= std::min(d.n1, n_spps) && d.m2 <= std::min(d.n2, n_spps))
                              : (d.m1 == std::min(d.n1, npoint_nearest) && d.m2 == std::min(d.n2, npoint_nearest));
    if (!rows_ok || d.row_offset < 0 || d.row_offset + d.m1 + d.m2 > n_rows)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_trainset_fill: problem %d: rows [%lld, +%d +%d) of %lld", i,
                        (long long)d.row_offset, d.m1, d.m2, (long long)n_rows);
    // the fixed-point scales leave room for 4 N terms per sum: a list (an index may be listed more than once) is held
    // to GAPRO_TRAINSET_MAX_LIST_FACTOR N entries
    if (std::max(std::max(d.n1, d.n2), d.t) > GAPRO_TRAINSET_MAX_LIST_FACTOR * n_points)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_trainset_fill: problem %d: a list of more than %d N entries", i,
                        GAPRO_TRAINSET_MAX_LIST_FACTOR);
    if (!pool && d.t == 0 && std::max(d.n1, d.n2) > npoint_nearest)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_trainset_fill: problem %d: no intersection point, no centroid", i);
  }
  if (pool && n_rows > p.rows_cap) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_trainset_fill: more rows than sides hold");
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_descs, h_descs, (size_t)n_problems * sizeof(gapro_trainset_desc),
                                      hipMemcpyHostToDevice, stream));
  const unsigned ny = 2u * (unsigned)n_problems;
  if (pool) {  // d_status carries on from gapro_trainset_count
    unsigned long long* sums = (unsigned long long*)((char*)d_workspace + p.sums);
    int* cnt = (int*)((char*)d_workspace + p.cnt);
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, (size_t)n_rows * feat_dim * sizeof(long long), stream));
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(cnt, 0, (size_t)n_rows * sizeof(int), stream));
    hipLaunchKernelGGL(k_ts_accum, dim3(grid_for((long long)p.n_max * kLanesPerPoint, 4, 256), ny), dim3(kThreads), 0,
                       stream, d_descs, d_idx, d_spp_inv, (const long long*)d_spp, d_feats, (long long)n_points,
                       (int)n_spps, (int)feat_dim, (int)fixed_shift, (const int*)((char*)d_workspace + p.marks), sums,
                       cnt, (long long*)d_sel, (long long)n_rows, d_status);
    hipLaunchKernelGGL(k_ts_pool_finalize, dim3((unsigned)((n_rows * feat_dim + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, (long long)n_rows, (int)feat_dim, (int)fixed_shift,
                       (const long long*)sums, (const int*)cnt, d_train);
  } else {
    unsigned long long* csum = (unsigned long long*)d_workspace;
    unsigned long long* amax = csum + 3 * (size_t)n_problems;
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(csum, 0, (size_t)(3 * n_problems + 1) * sizeof(long long), stream));
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, (size_t)n_problems * sizeof(int), stream));
    hipLaunchKernelGGL(k_ts_coord_absmax, dim3(grid_for(3 * (long long)n_points, 8, 512)), dim3(kThreads), 0,
                       stream, d_coords, 3 * (long long)n_points, amax);
    hipLaunchKernelGGL(k_ts_centroid, dim3(grid_for(p.t_max, 4, 64), (unsigned)n_problems), dim3(kThreads), 0,
                       stream, d_descs, d_idx, d_coords, (long long)n_points, (const unsigned long long*)amax, csum,
                       d_status);
    hipLaunchKernelGGL(k_ts_nearest, dim3(ny), dim3(kSelThreads), 0, stream, d_descs, d_idx, d_coords, d_feats,
                       (long long)n_points, (int)feat_dim, (int)npoint_nearest, (const unsigned long long*)amax,
                       (const long long*)csum, d_train, (long long*)d_sel, (long long)n_rows, d_status);
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
