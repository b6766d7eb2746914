// The consumers' voxelisation (include/gapro_hip.h, "Voxelisation"): voxelization_idx and voxelization
// of isbnet.ops / pointgroup_ops (src/voxelize/voxelize.cpp, voxelize.cu) on the device.
// The count call (gapro_voxelize_count):
// k_vox_insert   a thread a point: an open-addressing table of int32 slots, a power of two.  A slot holds a point index:
//                claimed by compare-and-swap from empty, an occupant compared by reading its coordinate row, an equal
//                key lowers the slot with an atomic minimum -- so a slot ends as its voxel's first point whatever the
//                schedule.  The probe loop is bounded by the table.
// scan_enqueue   a point is "first" iff its slot holds it; the exclusive scan of those flags (scan.h, three launches) is
//                the voxel number, stored as rank[i] and, for a first, as first_of[rank]; the total is header[2].
// k_vox_assign   input_map, and per voxel an integer atomic count whose return value is the point's place in its row
//                (any order: the fill sorts), the last point by an atomic maximum (mode 2), max_active by one atomic
//                maximum a wave.
// The fill call (gapro_voxelize_fill): k_vox_coords, then k_vox_single (modes 0..2) or k_vox_scatter and the ranking of
// every row, the rank of an entry being the number of smaller entries in its row: k_vox_rank<8> (rows of 2..8 entries,
// 8 lanes a row), k_vox_rank<64> (9..64, a wave a row), k_vox_rank_wg (longer rows: a workgroup a row through LDS, at
// most GAPRO_VOXELIZE_MAX_ACTIVE / 256 entries a thread, each against the row in LDS).
// The pooling (gapro_voxel_pool_forward / _backward): a thread per output element (v, c), see k_pool_forward.
#include "common.h"
#include "launch_util.h"
#include "scan.h"
#include "voxel_hash.h"
#include "wave_reduce.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kGridCap = 1 << 16;
constexpr int kEmpty = -1;
constexpr long long kMaxIndex = 0x7fffffffLL;
constexpr int kMaxActive = GAPRO_VOXELIZE_MAX_ACTIVE;
static_assert(kMaxActive % kThreads == 0, "k_vox_rank_wg gives every thread the same number of entries");

typedef unsigned long long u64;

// the workspace of n points; every part is aligned to 256 bytes
struct VoxWs {
  int* table;       // [slots]
  int* slot;        // [n] the slot of a point's voxel; -1: the point joined none
  int* rank;        // [n] firsts before the point
  int* first_of;    // [n] by voxel: its first point
  int* count;       // [n] by voxel
  int* pos;         // [n] the place the point claimed in its row
  int* last;        // [n] by voxel: its last point (mode 2)
  int* block_sums;  // [scan_blocks(n)]
  size_t bytes;
};

VoxWs ws_layout(void* base, long long n) {
  VoxWs w{};
  Carver c(base);
  w.table = c.take<int>((size_t)gapro_vox_slots(n));
  w.slot = c.take<int>((size_t)n);
  w.rank = c.take<int>((size_t)n);
  w.first_of = c.take<int>((size_t)n);
  w.count = c.take<int>((size_t)n);
  w.pos = c.take<int>((size_t)n);
  w.last = c.take<int>((size_t)n);
  w.block_sums = c.take<int>((size_t)scan_blocks(n));
  w.bytes = c.bytes();
  return w;
}

template <int kCols>
__device__ inline bool same_row(const long long* a, const long long* b) {
  bool eq = true;
#pragma unroll
  for (int c = 0; c < kCols; ++c) eq = eq && a[c] == b[c];
  return eq;
}

template <int kCols>
__global__ __launch_bounds__(kThreads) void k_vox_insert(const long long* __restrict__ coords, long long n, int* table,
                                                         u64 mask, int* __restrict__ slot, int* status) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    long long key[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) key[c] = coords[kCols * i + c];
    int mine = -1;
    if (kCols == 4 && key[0] < 0) {
      raise_bad_arg(status, GAPRO_VOXELIZE_FLAG_BATCH);
    } else {
      u64 s = gapro_vox_hash((const int64_t*)key, kCols) & mask;
      for (u64 probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {  // bounded by the table
        const int held = atomicCAS(table + s, kEmpty, (int)i);
        if (held == kEmpty) {
          mine = (int)s;
          break;
        }
        // an occupant is a point index below n whose key never changes: only points of the same key replace it
        if (same_row<kCols>(coords + kCols * (long long)held, key)) {
          atomicMin(table + s, (int)i);
          mine = (int)s;
          break;
        }
      }
      if (mine < 0) raise_bad_arg(status, GAPRO_VOXELIZE_FLAG_TABLE);  // a table with more points than slots: not built
    }
    slot[i] = mine;
  }
}

// the scan's value: is point i (< n) the first of its voxel
struct IsFirst {
  const int* __restrict__ table;
  const int* __restrict__ slot;
  __device__ int operator()(long long i) const {
    const int s = slot[i];
    return (s >= 0 && table[s] == (int)i) ? 1 : 0;
  }
};

// the scan's result: the firsts before point i are its rank, and a first's rank is its voxel
struct EmitRank {
  int* __restrict__ rank;
  int* __restrict__ first_of;
  __device__ void operator()(long long i, int r, int first) const {
    rank[i] = r;
    if (first) first_of[r] = (int)i;  // r < the number of voxels <= n
  }
};

__global__ __launch_bounds__(kThreads) void k_vox_assign(const int* __restrict__ table, const int* __restrict__ slot,
                                                         const int* __restrict__ rank, long long n, int mode,
                                                         int* __restrict__ input_map, int* count, int* __restrict__ pos,
                                                         int* last, int* header) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i0 = (long long)blockIdx.x * kThreads; i0 < n; i0 += stride) {  // uniform over the workgroup
    const long long i = i0 + threadIdx.x;
    int held = 0;
    if (i < n) {
      const int s = slot[i];
      int v = -1, p = -1;
      if (s >= 0) {
        v = rank[table[s]];  // the slot holds the voxel's first point, whose rank is the voxel's number
        p = atomicAdd(count + v, 1);
        if (mode == 2) atomicMax(last + v, (int)i);
        if (mode == 0 && p > 0) raise_bad_arg(header, GAPRO_VOXELIZE_FLAG_DUPLICATE);
        held = p + 1;
      }
      input_map[i] = v;
      pos[i] = p;
    }
    held = wave_max(held);
    if ((threadIdx.x & 63) == 0 && held > 0) atomicMax(header + 3, held);
  }
}

struct FillArgs {
  const long long* coords;
  const int* input_map;
  const int *first_of, *count, *pos, *last;
  long long* out_coords;
  int* out_map;
  int* status;
  long long n, M;
  int cols, A, mode;
};

__global__ __launch_bounds__(kThreads) void k_vox_coords(FillArgs a) {
  const long long total = a.M * a.cols, stride = (long long)gridDim.x * kThreads;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const long long v = e / a.cols;
    const int c = (int)(e - v * a.cols);
    const long long f = a.first_of[v];
    if (f < 0 || f >= a.n) {
      raise_bad_arg(a.status, GAPRO_VOXELIZE_FLAG_TABLE);
      a.out_coords[e] = 0;
    } else {
      a.out_coords[e] = a.coords[f * a.cols + c];
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_vox_single(FillArgs a) {
  const long long stride = (long long)gridDim.x * kThreads;
  const int* __restrict__ src = a.mode == 2 ? a.last : a.first_of;
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < a.M; v += stride) {
    a.out_map[2 * v] = 1;
    a.out_map[2 * v + 1] = src[v];
  }
}

// the table is zeros; every point writes itself to the place it claimed, the claimer of place 0 the count
__global__ __launch_bounds__(kThreads) void k_vox_scatter(FillArgs a) {
  const long long stride = (long long)gridDim.x * kThreads;
  const long long width = a.A + 1;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
    const long long v = a.input_map[i];
    const int p = a.pos[i];
    if (v < 0 || v >= a.M || p < 0 || p >= a.A) {
      raise_bad_arg(a.status, GAPRO_VOXELIZE_FLAG_TABLE);
      continue;
    }
    int* __restrict__ row = a.out_map + v * width;
    row[1 + p] = (int)i;
    if (p == 0) {
      const int c = a.count[v];
      if (c < 1 || c > a.A) raise_bad_arg(a.status, GAPRO_VOXELIZE_FLAG_TABLE);
      row[0] = c < 1 ? 1 : c > a.A ? a.A : c;
    }
  }
}

// G lanes a row, for the rows of more than `lo` and at most G entries.  The lanes of a row load its entries, count the
// smaller ones by G cross-lane reads, and store in place: the loads of a wave are complete before its stores issue.
template <int G>
__global__ __launch_bounds__(kThreads) void k_vox_rank(int* out_map, long long M, int A, int lo) {
  const long long width = (long long)A + 1, stride = (long long)gridDim.x * (kThreads / G);
  const int l = threadIdx.x % G;
  for (long long r0 = (long long)blockIdx.x * (kThreads / G); r0 < M; r0 += stride) {  // uniform over the workgroup
    const long long v = r0 + threadIdx.x / G;
    int* row = out_map + (v < M ? v : 0) * width;
    int n = v < M ? row[0] : 0;
    n = n > A ? A : n;
    const bool rows_mine = n > lo && n <= G;
    const bool have = rows_mine && l < n;
    const int e = have ? row[1 + l] : 0x7fffffff;
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < G; ++j) rank += __shfl(e, j, G) < e ? 1 : 0;
    if (have && rank < n) row[1 + rank] = e;
  }
}

// a workgroup a row, for the rows of more than 64 entries: the row in LDS, every thread ranks its entries against it
__global__ __launch_bounds__(kThreads) void k_vox_rank_wg(int* out_map, long long M, int A) {
  __shared__ int buf[kMaxActive];
  const long long width = (long long)A + 1;
  for (long long v = blockIdx.x; v < M; v += gridDim.x) {
    int* row = out_map + v * width;
    int n = row[0];  // uniform
    n = n > A ? A : n;
    n = n > kMaxActive ? kMaxActive : n;
    if (n <= 64) continue;
    for (int j = threadIdx.x; j < n; j += kThreads) buf[j] = row[1 + j];
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += kThreads) {
      const int e = buf[j];
      int rank = 0;
      for (int k = 0; k < n; ++k) rank += buf[k] < e ? 1 : 0;  // the same address in every lane: a broadcast
      row[1 + rank] = e;
    }
    __syncthreads();
  }
}

// ---- pooling ---------------------------------------------------------------------------------------------------------
// A thread per output element (v, c), consecutive threads consecutive c and then v: the stores of a wave are one
// contiguous run, the C threads of a row read the same table entries (one fetch, broadcast) and C consecutive floats of
// each listed point.  Four table entries and their features are fetched together, then added in the row's order.
struct PoolArgs {
  const float* in;   // forward: feats [N][C]; backward: d_out [M][C]
  const int* rule;   // [M][A + 1]
  float* out;        // forward: [M][C]; backward: d_feats [N][C], cleared
  int* marks;        // check: [N], cleared
  int* status;
  long long N, M;
  int C, A, average;
};

__device__ inline float pool_mult(int n, int average) { return (average && n > 0) ? 1.0f / (float)n : 1.0f; }

__device__ inline void split(long long e, int C, bool small, long long* v, int* c) {
  *v = small ? (long long)((unsigned)e / (unsigned)C) : e / C;
  *c = (int)(e - *v * C);
}

__global__ __launch_bounds__(kThreads) void k_pool_forward(PoolArgs a) {
#pragma clang fp contract(off)
  const long long total = a.M * a.C, stride = (long long)gridDim.x * kThreads;
  const bool small = total <= kMaxIndex;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    long long v;
    int c;
    split(e, a.C, small, &v, &c);
    const int* __restrict__ r = a.rule + v * ((long long)a.A + 1);
    const int n = r[0];
    float acc = 0.f;
    if (n < 0 || n > a.A) {
      if (c == 0) raise_bad_arg(a.status, GAPRO_VOXEL_POOL_FLAG_COUNT);
    } else {
      const float mult = pool_mult(n, a.average);
      const float* __restrict__ x = a.in + c;
      for (int k0 = 1; k0 <= n; k0 += 4) {
        float f[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + u <= n ? k0 + u : n;
          const long long p = r[k];
          ok[u] = p >= 0 && p < a.N;
          f[u] = x[(ok[u] ? p : 0) * a.C];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (k0 + u > n) break;
          if (!ok[u]) {
            if (c == 0) raise_bad_arg(a.status, GAPRO_VOXEL_POOL_FLAG_INDEX);
            continue;
          }
          const float prod = mult * f[u];
          acc = acc + prod;
        }
      }
    }
    a.out[e] = acc;
  }
}

__global__ __launch_bounds__(kThreads) void k_pool_backward(PoolArgs a) {
#pragma clang fp contract(off)
  const long long total = a.M * a.C, stride = (long long)gridDim.x * kThreads;
  const bool small = total <= kMaxIndex;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    long long v;
    int c;
    split(e, a.C, small, &v, &c);
    const int* __restrict__ r = a.rule + v * ((long long)a.A + 1);
    const int n = r[0];
    if (n < 0 || n > a.A) {
      if (c == 0) raise_bad_arg(a.status, GAPRO_VOXEL_POOL_FLAG_COUNT);
      continue;
    }
    const float g = pool_mult(n, a.average) * a.in[e];
    float* __restrict__ out = a.out + c;
    for (int k = 1; k <= n; ++k) {
      const long long p = r[k];
      if (p < 0 || p >= a.N) {
        if (c == 0) raise_bad_arg(a.status, GAPRO_VOXEL_POOL_FLAG_INDEX);
        continue;
      }
      out[p * a.C] = g;
    }
  }
}

// a thread per table cell (v, k), k in 1..A: the counts, the indices, and with the marks the points listed twice
__global__ __launch_bounds__(kThreads) void k_pool_check(PoolArgs a) {
  const long long total = a.M * a.A, stride = (long long)gridDim.x * kThreads;
  const bool small = total <= kMaxIndex;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    long long v;
    int k;
    split(e, a.A, small, &v, &k);
    const int* __restrict__ r = a.rule + v * ((long long)a.A + 1);
    const int n = r[0];
    if (n < 0 || n > a.A) {
      if (k == 0) raise_bad_arg(a.status, GAPRO_VOXEL_POOL_FLAG_COUNT);
      continue;
    }
    if (k >= n) continue;
    const long long p = r[1 + k];
    if (p < 0 || p >= a.N) raise_bad_arg(a.status, GAPRO_VOXEL_POOL_FLAG_INDEX);
    else if (atomicAdd(a.marks + p, 1) > 0) raise_bad_arg(a.status, GAPRO_VOXEL_POOL_FLAG_TWICE);
  }
}

bool pool_sizes_ok(int64_t n_points, int32_t n_channels, int64_t n_voxels, int64_t max_active) {
  return n_points >= 1 && n_points <= kMaxIndex && n_channels >= 1 && n_voxels >= 1 && n_voxels <= kMaxIndex &&
         max_active >= 1 && max_active <= kMaxIndex && n_voxels * (max_active + 1) <= kMaxIndex;
}

int copy_status(gapro_ctx* ctx, hipStream_t stream, const int32_t* d_status, int32_t* h_status_pinned) {
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_VOXELIZE_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

}  // namespace

extern "C" {

size_t gapro_voxelize_workspace_bytes(int64_t n_points) {
  if (n_points < 1 || n_points > kMaxIndex) return 0;
  return ws_layout(nullptr, n_points).bytes;
}

int gapro_voxelize_count(gapro_ctx* ctx, void* stream_, int64_t n_points, int32_t cols, const int64_t* d_coords,
                         int32_t mode, void* d_workspace, size_t workspace_bytes, int32_t* d_input_map,
                         gapro_voxelize_header* d_header, gapro_voxelize_header* h_header_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_points < 1 || n_points > kMaxIndex || (cols != 3 && cols != 4) || mode < 0 || mode > 4 || !d_coords ||
      !d_input_map || !d_header)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_voxelize_count: bad argument");
  if (!d_workspace || workspace_bytes < gapro_voxelize_workspace_bytes(n_points))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_voxelize_count: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const VoxWs w = ws_layout(d_workspace, n_points);
  const long long n = n_points, slots = gapro_vox_slots(n);
  int* header = (int*)d_header;
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(header, 0, sizeof(gapro_voxelize_header), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.table, 0xff, (size_t)slots * sizeof(int), stream));  // kEmpty
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.count, 0, (size_t)n * sizeof(int), stream));
  if (mode == 2) GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.last, 0xff, (size_t)n * sizeof(int), stream));  // -1
  const int grid = grid_for(n, 1, kGridCap);
  const long long* coords = (const long long*)d_coords;
  if (cols == 4)
    hipLaunchKernelGGL(k_vox_insert<4>, dim3(grid), dim3(kThreads), 0, stream, coords, n, w.table, (u64)(slots - 1),
                       w.slot, header);
  else
    hipLaunchKernelGGL(k_vox_insert<3>, dim3(grid), dim3(kThreads), 0, stream, coords, n, w.table, (u64)(slots - 1),
                       w.slot, header);
  scan_enqueue(stream, IsFirst{w.table, w.slot}, EmitRank{w.rank, w.first_of}, n, w.block_sums, header + 2);
  hipLaunchKernelGGL(k_vox_assign, dim3(grid), dim3(kThreads), 0, stream, w.table, w.slot, w.rank, n, mode,
                     (int*)d_input_map, w.count, w.pos, w.last, header);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_header_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_header_pinned, d_header, sizeof(gapro_voxelize_header), hipMemcpyDeviceToHost,
                                        stream));
  return GAPRO_OK;
}

int gapro_voxelize_fill(gapro_ctx* ctx, void* stream_, int64_t n_points, int32_t cols, const int64_t* d_coords,
                        int32_t mode, int64_t n_voxels, int64_t max_active, const void* d_workspace,
                        size_t workspace_bytes, const int32_t* d_input_map, int64_t* d_output_coords,
                        int32_t* d_output_map, int32_t* d_status, int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  int64_t width = 0;
  if (n_points < 1 || n_points > kMaxIndex || (cols != 3 && cols != 4) || !d_coords || !d_input_map ||
      !d_output_coords || !d_output_map || !d_status || n_voxels > n_points ||
      gapro_voxelize_table_shape(mode, n_voxels, max_active, &width) != GAPRO_OK)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_voxelize_fill: bad argument");
  if (!d_workspace || workspace_bytes < gapro_voxelize_workspace_bytes(n_points))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_voxelize_fill: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const VoxWs w = ws_layout((void*)d_workspace, n_points);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_VOXELIZE_STATUS_WORDS * sizeof(int32_t), stream));
  FillArgs a{};
  a.coords = (const long long*)d_coords;
  a.input_map = (const int*)d_input_map;
  a.first_of = w.first_of;
  a.count = w.count;
  a.pos = w.pos;
  a.last = w.last;
  a.out_coords = (long long*)d_output_coords;
  a.out_map = (int*)d_output_map;
  a.status = (int*)d_status;
  a.n = n_points;
  a.M = n_voxels;
  a.cols = cols;
  a.A = (int)(width - 1);
  a.mode = mode;
  hipLaunchKernelGGL(k_vox_coords, dim3(grid_for(a.M * cols, 1, kGridCap)), dim3(kThreads), 0, stream, a);
  if (mode <= 2) {
    hipLaunchKernelGGL(k_vox_single, dim3(grid_for(a.M, 1, kGridCap)), dim3(kThreads), 0, stream, a);
  } else {
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_output_map, 0, (size_t)(n_voxels * width) * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_vox_scatter, dim3(grid_for(a.n, 1, kGridCap)), dim3(kThreads), 0, stream, a);
    if (a.A > 1)
      hipLaunchKernelGGL(k_vox_rank<8>, dim3(grid_for(a.M * 8, 1, kGridCap)), dim3(kThreads), 0, stream, a.out_map, a.M,
                         a.A, 1);
    if (a.A > 8)
      hipLaunchKernelGGL(k_vox_rank<64>, dim3(grid_for(a.M * 64, 1, kGridCap)), dim3(kThreads), 0, stream, a.out_map,
                         a.M, a.A, 8);
    if (a.A > 64)
      hipLaunchKernelGGL(k_vox_rank_wg, dim3((unsigned)(a.M < 4096 ? a.M : 4096)), dim3(kThreads), 0, stream,
                         a.out_map, a.M, a.A);
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return copy_status(ctx, stream, d_status, h_status_pinned);
}

size_t gapro_voxel_pool_workspace_bytes(int64_t n_points) {
  if (n_points < 1 || n_points > kMaxIndex) return 0;
  return align_up((size_t)n_points * sizeof(int), 256);
}

int gapro_voxel_pool_forward(gapro_ctx* ctx, void* stream_, int64_t n_points, int32_t n_channels, const float* d_feats,
                             int64_t n_voxels, int64_t max_active, const int32_t* d_map_rule, int32_t mode,
                             int32_t check, void* d_workspace, size_t workspace_bytes, float* d_out, int32_t* d_status,
                             int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!pool_sizes_ok(n_points, n_channels, n_voxels, max_active) || !d_feats || !d_map_rule || !d_out || !d_status ||
      (check != 0 && check != 1))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_voxel_pool_forward: bad argument");
  if (check && (!d_workspace || workspace_bytes < gapro_voxel_pool_workspace_bytes(n_points)))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_voxel_pool_forward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_VOXELIZE_STATUS_WORDS * sizeof(int32_t), stream));
  PoolArgs a{d_feats, (const int*)d_map_rule, d_out, (int*)d_workspace, (int*)d_status, n_points, n_voxels,
             n_channels, (int)max_active, mode == 4};
  if (check) {
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_workspace, 0, (size_t)n_points * sizeof(int), stream));
    hipLaunchKernelGGL(k_pool_check, dim3(grid_for(a.M * a.A, 1, kGridCap)), dim3(kThreads), 0, stream, a);
  }
  hipLaunchKernelGGL(k_pool_forward, dim3(grid_for(a.M * a.C, 1, kGridCap)), dim3(kThreads), 0, stream, a);
  GAPRO_LAUNCH_CHECK(ctx);
  return copy_status(ctx, stream, d_status, h_status_pinned);
}

int gapro_voxel_pool_backward(gapro_ctx* ctx, void* stream_, int64_t n_points, int32_t n_channels,
                              const float* d_grad_out, int64_t n_voxels, int64_t max_active, const int32_t* d_map_rule,
                              int32_t mode, float* d_grad_feats, int32_t* d_status, int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!pool_sizes_ok(n_points, n_channels, n_voxels, max_active) || !d_grad_out || !d_map_rule || !d_grad_feats ||
      !d_status)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_voxel_pool_backward: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_VOXELIZE_STATUS_WORDS * sizeof(int32_t), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_grad_feats, 0, (size_t)n_points * n_channels * sizeof(float), stream));
  PoolArgs a{d_grad_out, (const int*)d_map_rule, d_grad_feats, nullptr, (int*)d_status, n_points, n_voxels,
             n_channels, (int)max_active, mode == 4};
  hipLaunchKernelGGL(k_pool_backward, dim3(grid_for(a.M * a.C, 1, kGridCap)), dim3(kThreads), 0, stream, a);
  GAPRO_LAUNCH_CHECK(ctx);
  return copy_status(ctx, stream, d_status, h_status_pinned);
}

}  // extern "C"
