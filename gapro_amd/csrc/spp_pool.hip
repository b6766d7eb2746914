// Superpoint pooling (include/gapro_hip.h, "Superpoint pooling"): torch_scatter's scatter_mean /
// scatter_max of per-point or per-voxel features to superpoints, with their gradients, in float32 in a defined order.
// The plan (gapro_spp_plan_build), once a step: a CSR of the points by superpoint and, with a point map, one of the
// points by source row, both by the same routine, csr_by_key:
// k_spp_keys      a thread a point: its key (the superpoint id, or the source row), the sentinel key n_keys for a point
//                 whose id or map value is out of range (it sorts behind every segment and is raised in the status).
// a stable LSD radix sort of (key, point) by 8-bit digits, ceil(bits(n_keys) / 8) passes, a pass being
//   k_spp_hist      a workgroup a tile of kTile points: the tile's 256 digit counts (integer LDS atomics), stored
//                   bin-major so that ONE exclusive scan of the whole array is the place of every (bin, tile) run;
//   scan_enqueue    that scan, in place (scan.h, three launches);
//   k_spp_scatter   the tile again, 256 points at a time in point order: a point's rank among the equal digits of its
//                   wave by eight ballots, the waves' bin counts in LDS, the running place of each bin.
// k_spp_offsets   a thread a key: the lower bound of the key in the sorted keys, by bisection.
// The cost of every kernel is linear in the points whatever the segments' lengths; no workgroup waits for another; the
// only atomics are integer counts, whose sums do not depend on the schedule.
// The pooling (gapro_spp_pool_forward / _backward): a thread per output element, see k_spp_forward.
#include "common.h"
#include "launch_util.h"
#include "scan.h"
#include "wave_reduce.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kBins = 256;                          // an 8-bit digit
constexpr int kTileChunks = 16;                     // chunks of kThreads points in a tile
constexpr int kTile = kThreads * kTileChunks;       // GAPRO_SPP_SORT_TILE
constexpr int kGridCap = 1 << 16;
constexpr int kAhead = 8;                          // gathered loads in flight per thread of the pooling kernels
constexpr long long kMaxIndex = 0x7fffffffLL;
constexpr long long kMaxKeys = GAPRO_SPP_MAX_SEGMENTS;
static_assert(kTile == GAPRO_SPP_SORT_TILE, "the header states the tile");
static_assert(kBins == kThreads, "a thread a bin in the sort kernels");
static_assert(kThreads == kScanThreads, "k_spp_batch_scan calls block_exclusive");

typedef unsigned long long u64;

__device__ inline long long load_index(const void* p, int is64, long long i) {
  return is64 ? ((const long long*)p)[i] : (long long)((const int*)p)[i];
}

struct KeyArgs {
  const void* index;
  const void* map;  // or null
  int index_i64, map_i64, by_row;
  long long n, S, R;
  unsigned* keys;
  int* vals;
  int* status;
};

__global__ __launch_bounds__(kThreads) void k_spp_keys(KeyArgs a) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i0 = (long long)blockIdx.x * kThreads; i0 < a.n; i0 += stride) {  // uniform over the workgroup
    const long long i = i0 + threadIdx.x;
    int flag = 0;
    if (i < a.n) {
      const long long s = load_index(a.index, a.index_i64, i);
      long long r = 0;
      if (s < 0 || s >= a.S) flag |= GAPRO_SPP_FLAG_INDEX;
      if (a.map) {
        r = load_index(a.map, a.map_i64, i);
        if (r < 0 || r >= a.R) flag |= GAPRO_SPP_FLAG_MAP;
      }
      a.keys[i] = a.by_row ? (unsigned)(flag ? a.R : r) : (unsigned)(flag ? a.S : s);
      a.vals[i] = (int)i;
    }
    flag = wave_or(flag);
    if ((threadIdx.x & 63) == 0 && flag) raise_bad_arg(a.status, flag);
  }
}

__global__ __launch_bounds__(kThreads) void k_spp_hist(const unsigned* __restrict__ keys, long long n, int shift,
                                                       long long n_tiles, int* __restrict__ hist) {
  __shared__ int bins[kBins];
  bins[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kTile;
#pragma unroll 4
  for (int j = 0; j < kTileChunks; ++j) {
    const long long i = base + j * kThreads + threadIdx.x;
    if (i < n) atomicAdd(&bins[(keys[i] >> shift) & (kBins - 1)], 1);
  }
  __syncthreads();
  hist[(long long)threadIdx.x * n_tiles + blockIdx.x] = bins[threadIdx.x];
}

// The places of a tile's points: `place[bin]` starts at the scanned count of (bin, tile) and runs through the tile in
// point order, 256 points at a time; inside the 256 the waves are in point order and so are the lanes of a wave.
__global__ __launch_bounds__(kThreads) void k_spp_scatter(const unsigned* __restrict__ keys,
                                                          const int* __restrict__ vals, long long n, int shift,
                                                          long long n_tiles, const int* __restrict__ offsets,
                                                          unsigned* __restrict__ keys_out, int* __restrict__ vals_out) {
  __shared__ int place[kBins];
  __shared__ int wave_bins[kWaves][kBins];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  place[threadIdx.x] = offsets[(long long)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < kWaves; ++w) wave_bins[w][threadIdx.x] = 0;
  const long long base = (long long)blockIdx.x * kTile;
  for (int j = 0; j < kTileChunks && base + (long long)j * kThreads < n; ++j) {  // uniform
    __syncthreads();  // place and the cleared counts are written
    const long long i = base + j * kThreads + threadIdx.x;
    const bool have = i < n;
    const unsigned key = have ? keys[i] : 0u;
    const int val = have ? vals[i] : 0;
    const int d = (int)((key >> shift) & (kBins - 1));
    u64 same = __ballot(have);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const u64 set = __ballot(have && ((d >> b) & 1));
      same &= ((d >> b) & 1) ? set : ~set;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    if (have && rank == 0) wave_bins[wave][d] = __popcll(same);
    __syncthreads();
    if (have) {
      long long pos = (long long)place[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wave_bins[w][d];
      if (pos >= 0 && pos < n) {  // always, for the counts this tile gave k_spp_hist
        keys_out[pos] = key;
        vals_out[pos] = val;
      }
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {  // the thread of a bin: nobody else touches these words here
      add += wave_bins[w][threadIdx.x];
      wave_bins[w][threadIdx.x] = 0;
    }
    place[threadIdx.x] += add;
  }
}

// off[k] for k in [0, n_keys]: the entries of the sorted keys below k (the sentinels, equal to n_keys, are below none)
__global__ __launch_bounds__(kThreads) void k_spp_offsets(const unsigned* __restrict__ keys, long long n,
                                                          long long n_keys, int* __restrict__ off,
                                                          int* __restrict__ counts /* or null */) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k <= n_keys; k += stride) {
    long long lo[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const long long want = k + t;
      long long a = 0, b = n;  // at most 32 halvings
      while (a < b) {
        const long long m = a + (b - a) / 2;
        if ((long long)keys[m] < want) a = m + 1;
        else b = m;
      }
      lo[t] = a;
      if (!counts || k == n_keys) break;
    }
    off[k] = (int)lo[0];
    if (counts && k < n_keys) counts[k] = (int)(lo[1] - lo[0]);
  }
}

// the source row of every listed point, in the CSR's order; -1 behind the last segment
__global__ __launch_bounds__(kThreads) void k_spp_rows(const int* __restrict__ seg_off, const int* __restrict__ seg_pts,
                                                       const void* map, int map_i64, long long n, long long S,
                                                       int* __restrict__ seg_rows) {
  const long long stride = (long long)gridDim.x * kThreads, listed = seg_off[S];
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < n; k += stride) {
    const long long p = seg_pts[k];
    seg_rows[k] = (k < listed && p >= 0 && p < n) ? (int)load_index(map, map_i64, p) : -1;
  }
}

// a non-empty segment counts for the sample that holds its first point
__global__ __launch_bounds__(kThreads) void k_spp_batch_count(const int* __restrict__ seg_off,
                                                              const int* __restrict__ seg_pts, long long n, long long S,
                                                              const void* offsets, int offsets_i64, int B,
                                                              int* batch_count) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long s = (long long)blockIdx.x * kThreads + threadIdx.x; s < S; s += stride) {
    const long long lo = seg_off[s], hi = seg_off[s + 1];
    if (lo < 0 || lo >= hi || lo >= n) continue;
    const long long first = seg_pts[lo];
    int a = 0, b = B + 1;  // the offsets beyond `first` start at a
    while (a < b) {
      const int m = a + (b - a) / 2;
      if (load_index(offsets, offsets_i64, m) <= first) a = m + 1;
      else b = m;
    }
    if (a >= 1 && a <= B) atomicAdd(batch_count + (a - 1), 1);
  }
}

__global__ __launch_bounds__(kThreads) void k_spp_batch_scan(const int* __restrict__ batch_count, int B,
                                                             long long* __restrict__ out /* [B + 1] */) {
  __shared__ int wave_tot[kWaves];
  long long running = 0;
  for (int b0 = 0; b0 < B; b0 += kThreads) {  // uniform
    const int b = b0 + threadIdx.x;
    const int v = b < B ? batch_count[b] : 0;
    int all;
    const int before = block_exclusive(v, wave_tot, &all);
    if (b < B) out[b + 1] = running + before + v;
    running += all;
  }
  if (threadIdx.x == 0) out[0] = 0;
}

// ---- pooling ---------------------------------------------------------------------------------------------------------
// A thread per output element (s, c), consecutive threads consecutive c and then s: the C threads of a segment read the
// same CSR entries (one fetch, broadcast) and C consecutive floats of each listed row, and the stores of a wave are one
// contiguous run.  kAhead entries and their values are fetched together, then combined in the segment's order: the sum
// (or the comparison chain) of one output is serial, its length the segment's.
struct PoolArgs {
  const float* src;      // [R or N][ld]
  long long ld;
  const int* seg_off;    // [S + 1]
  const int* seg_pts;    // [N]
  const int* seg_rows;   // [N] the rows the values are read from; null: the points themselves
  float* out;            // [S][C]
  long long* arg;        // [S][C], max
  long long S, N, rows;  // rows: the rows of src
  int C;
};

__device__ inline void split(long long e, int C, bool small, long long* v, int* c) {
  *v = small ? (long long)((unsigned)e / (unsigned)C) : e / C;
  *c = (int)(e - *v * C);
}

template <bool kMax>
__global__ __launch_bounds__(kThreads) void k_spp_forward(PoolArgs a) {
#pragma clang fp contract(off)
  const long long total = a.S * a.C, stride = (long long)gridDim.x * kThreads;
  const bool small = total <= kMaxIndex;
  const int* __restrict__ rows = a.seg_rows ? a.seg_rows : a.seg_pts;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    long long s;
    int c;
    split(e, a.C, small, &s, &c);
    long long lo = a.seg_off[s], hi = a.seg_off[s + 1];
    if (lo < 0 || hi > a.N || hi < lo) hi = lo = 0;  // never, for a plan the build wrote
    const float* __restrict__ x = a.src + c;
    float acc = 0.f;
    long long best = a.N;
    bool have = false;
    int n = 0;
    for (long long k0 = lo; k0 < hi; k0 += kAhead) {
      float f[kAhead];
      long long p[kAhead];
      bool ok[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const long long k = k0 + u < hi ? k0 + u : hi - 1;
        const long long r = rows[k];
        p[u] = kMax ? (long long)a.seg_pts[k] : 0;
        ok[u] = r >= 0 && r < a.rows;
        f[u] = x[(ok[u] ? r : 0) * a.ld];
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {  // selects, no branches: a branch here would pull every load behind its test
        const bool use = ok[u] && k0 + u < hi;
        n += use ? 1 : 0;
        if (kMax) {
          const bool take = use && (!have || f[u] > acc);
          acc = take ? f[u] : acc;
          best = take ? p[u] : best;
          have = have || use;
        } else {
          acc = use ? acc + f[u] : acc;
        }
      }
    }
    if (kMax) {
      a.out[e] = have ? acc : 0.f;
      a.arg[e] = best;
    } else {
      a.out[e] = n > 0 ? acc / (float)n : 0.f;
    }
  }
}

struct BackArgs {
  const float* g;          // [S][C]
  const long long* arg;    // [S][C], max
  const void* index;       // [N]
  const void* map;         // [N] or null
  const int* counts;       // [S]
  const int* row_off;      // [R + 1], mapped
  const int* row_pts;      // [N], mapped
  float* d_src;            // [R or N][C], written whole
  long long S, N, R;
  int C, index_i64, map_i64;
};

// the gradient of point p (in [0, N)) in channel c: fl(g / fl(n)) or the winner's g; 0 for a point that is in no segment
// (`listed` false: its map value is out of range).  Selects, no branches: the callers fetch several points together.
template <bool kMax>
__device__ inline float point_grad(const BackArgs& a, long long p, int c, bool listed) {
#pragma clang fp contract(off)
  const long long s = load_index(a.index, a.index_i64, p);
  const bool ok = listed && s >= 0 && s < a.S;
  const long long at = (ok ? s : 0) * a.C + c;
  const float g = a.g[at];
  if (kMax) return (ok && a.arg[at] == p) ? g : 0.f;
  const int n = a.counts[ok ? s : 0];
  return (ok && n > 0) ? g / (float)(n > 0 ? n : 1) : 0.f;
}

template <bool kMax>
__global__ __launch_bounds__(kThreads) void k_spp_backward_points(BackArgs a) {
  const long long total = a.N * a.C, stride = (long long)gridDim.x * kThreads;
  const bool small = total <= kMaxIndex;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    long long p;
    int c;
    split(e, a.C, small, &p, &c);
    bool listed = true;
    if (a.map) {  // uniform
      const long long r = load_index(a.map, a.map_i64, p);
      listed = r >= 0 && r < a.R;
    }
    a.d_src[e] = point_grad<kMax>(a, p, c, listed);
  }
}

// a thread per (row, c): the gradients of the row's points, added in ascending point order from +0
template <bool kMax>
__global__ __launch_bounds__(kThreads) void k_spp_backward_rows(BackArgs a) {
#pragma clang fp contract(off)
  const long long total = a.R * a.C, stride = (long long)gridDim.x * kThreads;
  const bool small = total <= kMaxIndex;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    long long r;
    int c;
    split(e, a.C, small, &r, &c);
    long long lo = a.row_off[r], hi = a.row_off[r + 1];
    if (lo < 0 || hi > a.N || hi < lo) hi = lo = 0;
    float acc = 0.f;
    for (long long k0 = lo; k0 < hi; k0 += 4) {
      float d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long k = k0 + u < hi ? k0 + u : hi - 1;
        const long long p = a.row_pts[k];
        const bool in = p >= 0 && p < a.N;  // always, and its map value is r: the build listed it here
        d[u] = point_grad<kMax>(a, in ? p : 0, c, in);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = k0 + u < hi ? acc + d[u] : acc;
    }
    a.d_src[e] = acc;
  }
}

int key_passes(long long n_keys) {  // the largest key is the sentinel n_keys
  int bits = 0;
  while ((n_keys >> bits) != 0) ++bits;
  return (bits + 7) / 8;
}

struct SortWs {
  unsigned *keys_a, *keys_b;  // [n]
  int* vals;                  // [n]
  int* hist;                  // [256 tiles]
  int* block_sums;            // [scan_blocks(256 tiles)]
  int* batch_count;           // [n_batches]
  size_t bytes;
};

SortWs ws_layout(void* base, long long n, long long n_batches) {
  SortWs w{};
  Carver c(base);
  const long long n_tiles = (n + kTile - 1) / kTile, cells = n_tiles * kBins;
  w.keys_a = c.take<unsigned>((size_t)n);
  w.keys_b = c.take<unsigned>((size_t)n);
  w.vals = c.take<int>((size_t)n);
  w.hist = c.take<int>((size_t)cells);
  w.block_sums = c.take<int>((size_t)scan_blocks(cells));
  w.batch_count = c.take<int>((size_t)(n_batches > 0 ? n_batches : 1));
  w.bytes = c.bytes();
  return w;
}

// off[n_keys + 1] and pts[n] of the points by key, every run in ascending point order; counts[n_keys] when given
int csr_by_key(gapro_ctx* ctx, hipStream_t stream, const SortWs& w, KeyArgs ka, long long n_keys, int* off, int* pts,
               int* counts) {
  const long long n = ka.n, n_tiles = (n + kTile - 1) / kTile, cells = n_tiles * kBins;
  const int passes = key_passes(n_keys);
  // the values alternate between the workspace and pts and end in pts
  unsigned *k_in = w.keys_a, *k_out = w.keys_b;
  int *v_in = (passes & 1) ? w.vals : pts, *v_out = (passes & 1) ? pts : w.vals;
  ka.keys = k_in;
  ka.vals = v_in;
  hipLaunchKernelGGL(k_spp_keys, dim3(grid_for(n, 1, kGridCap)), dim3(kThreads), 0, stream, ka);
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(k_spp_hist, dim3((unsigned)n_tiles), dim3(kThreads), 0, stream, k_in, n, shift, n_tiles, w.hist);
    scan_enqueue(stream, ScanFrom{w.hist}, ScanInto{w.hist}, cells, w.block_sums, nullptr);
    hipLaunchKernelGGL(k_spp_scatter, dim3((unsigned)n_tiles), dim3(kThreads), 0, stream, k_in, v_in, n, shift,
                       n_tiles, w.hist, k_out, v_out);
    unsigned* tk = k_in;
    k_in = k_out;
    k_out = tk;
    int* tv = v_in;
    v_in = v_out;
    v_out = tv;
  }
  hipLaunchKernelGGL(k_spp_offsets, dim3(grid_for(n_keys + 1, 1, kGridCap)), dim3(kThreads), 0, stream, k_in, n, n_keys,
                     off, counts);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

bool plan_sizes_ok(const gapro_spp_plan* p) {
  return p && p->n_points >= 1 && p->n_points <= kMaxIndex && p->n_spps >= 1 && p->n_spps <= kMaxKeys &&
         p->n_rows >= 0 && p->n_rows <= kMaxKeys && (p->index_i64 == 0 || p->index_i64 == 1) &&
         (p->map_i64 == 0 || p->map_i64 == 1) && p->d_index && p->d_seg_off && p->d_seg_pts && p->d_counts &&
         ((p->n_rows == 0 && !p->d_point_map) ||
          (p->n_rows >= 1 && p->d_point_map && p->d_row_off && p->d_row_pts && p->d_seg_rows));
}

}  // namespace

extern "C" {

size_t gapro_spp_plan_workspace_bytes(int64_t n_points, int64_t n_batches) {
  if (n_points < 1 || n_points > kMaxIndex || n_batches < 0 || n_batches > GAPRO_SPP_MAX_BATCHES) return 0;
  return ws_layout(nullptr, n_points, n_batches).bytes;
}

int gapro_spp_plan_build(gapro_ctx* ctx, void* stream_, const gapro_spp_plan* plan, int64_t n_batches,
                         const void* d_batch_offsets, int32_t offsets_i64, int64_t* d_spp_batch_offsets,
                         void* d_workspace, size_t workspace_bytes, int32_t* d_status, int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!plan_sizes_ok(plan) || !d_status || n_batches < 0 || n_batches > GAPRO_SPP_MAX_BATCHES ||
      (n_batches > 0 && (!d_batch_offsets || !d_spp_batch_offsets)) || (offsets_i64 != 0 && offsets_i64 != 1))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spp_plan_build: bad argument");
  const size_t need = gapro_spp_plan_workspace_bytes(plan->n_points, n_batches);
  if (!d_workspace || need == 0 || workspace_bytes < need)
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_spp_plan_build: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const long long n = plan->n_points, S = plan->n_spps, R = plan->n_rows;
  const SortWs w = ws_layout(d_workspace, n, n_batches);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_SPP_STATUS_WORDS * sizeof(int32_t), stream));
  KeyArgs ka{};
  ka.index = plan->d_index;
  ka.map = plan->d_point_map;
  ka.index_i64 = plan->index_i64;
  ka.map_i64 = plan->map_i64;
  ka.n = n;
  ka.S = S;
  ka.R = R;
  ka.status = (int*)d_status;
  ka.by_row = 0;
  int rc = csr_by_key(ctx, stream, w, ka, S, plan->d_seg_off, plan->d_seg_pts, plan->d_counts);
  if (rc != GAPRO_OK) return rc;
  if (R > 0) {
    ka.by_row = 1;
    rc = csr_by_key(ctx, stream, w, ka, R, plan->d_row_off, plan->d_row_pts, nullptr);
    if (rc != GAPRO_OK) return rc;
    hipLaunchKernelGGL(k_spp_rows, dim3(grid_for(n, 1, kGridCap)), dim3(kThreads), 0, stream, plan->d_seg_off,
                       plan->d_seg_pts, plan->d_point_map, plan->map_i64, n, S, plan->d_seg_rows);
  }
  if (n_batches > 0) {
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.batch_count, 0, (size_t)n_batches * sizeof(int), stream));
    hipLaunchKernelGGL(k_spp_batch_count, dim3(grid_for(S, 1, kGridCap)), dim3(kThreads), 0, stream, plan->d_seg_off,
                       plan->d_seg_pts, n, S, d_batch_offsets, offsets_i64, (int)n_batches, w.batch_count);
    hipLaunchKernelGGL(k_spp_batch_scan, dim3(1), dim3(kThreads), 0, stream, w.batch_count, (int)n_batches,
                       (long long*)d_spp_batch_offsets);
  }
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_SPP_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_spp_pool_forward(gapro_ctx* ctx, void* stream_, const gapro_spp_plan* plan, const float* d_src,
                           int64_t src_rows, int64_t src_ld, int32_t n_channels, int32_t reduce, int32_t through_map,
                           float* d_out, int64_t* d_arg) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!plan_sizes_ok(plan) || !d_src || !d_out || n_channels < 1 || src_ld < n_channels ||
      (reduce != GAPRO_SPP_MEAN && reduce != GAPRO_SPP_MAX) || (reduce == GAPRO_SPP_MAX && !d_arg) ||
      (through_map != 0 && through_map != 1) || (through_map && plan->n_rows == 0) ||
      src_rows != (through_map ? plan->n_rows : plan->n_points))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spp_pool_forward: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  PoolArgs a{d_src, src_ld, plan->d_seg_off, plan->d_seg_pts, through_map ? plan->d_seg_rows : nullptr, d_out,
             (long long*)d_arg, plan->n_spps, plan->n_points, src_rows, n_channels};
  const int grid = grid_for(a.S * a.C, 1, kGridCap);
  if (reduce == GAPRO_SPP_MAX) hipLaunchKernelGGL(k_spp_forward<true>, dim3(grid), dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(k_spp_forward<false>, dim3(grid), dim3(kThreads), 0, stream, a);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_spp_pool_backward(gapro_ctx* ctx, void* stream_, const gapro_spp_plan* plan, const float* d_grad_out,
                            int32_t n_channels, int32_t reduce, int32_t through_map, const int64_t* d_arg,
                            float* d_grad_src) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!plan_sizes_ok(plan) || !d_grad_out || !d_grad_src || n_channels < 1 ||
      (reduce != GAPRO_SPP_MEAN && reduce != GAPRO_SPP_MAX) || (reduce == GAPRO_SPP_MAX && !d_arg) ||
      (through_map != 0 && through_map != 1) || (through_map && plan->n_rows == 0))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spp_pool_backward: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  BackArgs a{d_grad_out, (const long long*)d_arg, plan->d_index, plan->d_point_map, plan->d_counts, plan->d_row_off,
             plan->d_row_pts, d_grad_src, plan->n_spps, plan->n_points, plan->n_rows, n_channels, plan->index_i64,
             plan->map_i64};
  const bool max = reduce == GAPRO_SPP_MAX;
  if (through_map) {
    const int grid = grid_for(a.R * a.C, 1, kGridCap);
    if (max) hipLaunchKernelGGL(k_spp_backward_rows<true>, dim3(grid), dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(k_spp_backward_rows<false>, dim3(grid), dim3(kThreads), 0, stream, a);
  } else {
    const int grid = grid_for(a.N * a.C, 1, kGridCap);
    if (max) hipLaunchKernelGGL(k_spp_backward_points<true>, dim3(grid), dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(k_spp_backward_points<false>, dim3(grid), dim3(kThreads), 0, stream, a);
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
