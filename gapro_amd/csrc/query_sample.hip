// The consumer's query sampling (include/gapro_hip.h, "Query sampling"): the furthest point sampling and
// the ball queries of ISBNet's Point Aggregator (isbnet/model/aggregator.py:63-115, 154-205), batch-flat and batched,
// as two kernels.
// k_fps         one workgroup of 1024 threads per sample, every output of the sample in one launch (a launch per path
//               that n_points admits: a workgroup serves its sample in the launch of the sample's path).  Thread t owns the
//               points t, t + 1024, ..; their running minima stay in registers (and their coordinates too, up to
//               kResidentCap points; up to kStreamedCap the coordinates stream from L2; beyond it the minima live in the
//               workspace).  An iteration is: update and scan the own points, a wave maximum of the 64-bit key
//               (distance bits + 1) << 32 | ~index by cross-lane shuffles, one LDS slot per wave (key and coordinates of
//               the wave's winner), ONE barrier, and the maximum of the sixteen slots in every wave.  The slots are
//               double-buffered: the barrier of iteration s + 1 is what frees the slots of iteration s.  The key is an
//               integer, so the winner does not depend on the order of the reduction: the largest distance, and among
//               equal ones the lowest index.  No workgroup waits for another.
// k_ball_query  one wave per query: the query's sample is scanned 64 points at a time in index order (four such chunks
//               in flight), the ballot of `d2 < r2` and a prefix population count place the hits, the scan stops at
//               nsample hits.
// Every squared distance is ((dx*dx + dy*dy) + dz*dz) with each operation rounded on its own: sqdist() switches
// contraction off for itself, and the file does for the rest.
#include "common.h"
#include "label_types.h"
#include "launch_util.h"
#include "wave_reduce.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kFpsThreads = GAPRO_FPS_THREADS, kFpsWaves = kFpsThreads / 64;
constexpr int kResidentK = 16, kStreamedK = 64;  // points of a thread whose state is in registers
constexpr int kFpsGroup = 8;  // points of a thread whose loads are in flight together
constexpr long long kResidentCap = (long long)kFpsThreads * kResidentK;
constexpr long long kStreamedCap = (long long)kFpsThreads * kStreamedK;
constexpr int kBqThreads = 256, kBqUnroll = 4;
constexpr long long kMaxIndex = 0x7fffffffLL;
constexpr float kFarAway = 1e10f;     // the running minimum before the first update
constexpr float kOriginBall = 1e-3f;  // skip_origin: x*x + y*y + z*z at or below this is no candidate
static_assert(kFpsWaves == 16, "the slot reduction folds sixteen lanes");
static_assert(kStreamedK <= 64, "the candidate bits of a thread are one 64-bit word");

typedef unsigned long long u64;

// hipcc contracts by default, and the __fmul_rn / __fadd_rn of its headers are plain operators compiled with that
// default: they fuse after inlining.  The pragma inside the function is the guard.
__device__ inline float sqdist(float dx, float dy, float dz) {
#pragma clang fp contract(off)
  return (dx * dx + dy * dy) + dz * dz;
}

// status[0] the code, status[1] the flags: a bad argument wins over a non-finite coordinate whatever the order
__device__ inline void raise(int* status, int flag) {
  if (flag & GAPRO_QS_FLAG_NOT_FINITE) {
    atomicOr(status + 1, flag);
    atomicCAS(status, (int)GAPRO_OK, (int)GAPRO_ERR_NOT_FINITE);
  } else {
    raise_bad_arg(status, flag);  // launch_util.h
  }
}

struct Offsets {
  const void* off;      // i32 / i64 [B]: sample b owns the points [off[b - 1], off[b]), off[-1] = 0
  const void* new_off;  // the same for the outputs / queries
  int off_i64, new_off_i64, B;
  long long N, M;
};

// the range of sample b in a table of `total` entries; false: it decreases or leaves [0, total]
__device__ inline bool range_of(const void* table, int i64, int b, long long total, long long* lo, long long* hi) {
  *lo = b > 0 ? idx_at(table, i64, b - 1) : 0;
  *hi = idx_at(table, i64, b);
  return *lo >= 0 && *lo <= *hi && *hi <= total;
}

struct FpsArgs {
  Offsets o;
  const float* xyz;  // [N][3]
  float* ws;         // [N] the running minima of a sample beyond kStreamedCap points
  int* idx;          // [M]
  float* dist;       // [N] or null: the running minima as the last iteration left them
  int* status;
  int skip_origin, local_index;
};

struct Pick {
  unsigned i;
  float x, y, z;
};

struct FpsShared {
  u64 key[2][kFpsWaves];
  float4 pt[2][kFpsWaves];
};

// a thread's best (distance `bd` < 0: none) as the key the maxima are taken of
__device__ inline u64 fps_key(float bd, unsigned bi) {
  return bd >= 0.f ? ((u64)(__float_as_uint(bd) + 1u) << 32) | (u64)(~bi) : 0ull;
}

struct Best {  // a thread's best so far: distance (< 0: none), point, index
  float d, x, y, z;
  unsigned i;
};

// Point i with the running minimum dj against the last output: the new minimum; the thread's best follows.  The thread
// visits its points in ascending index and the test is strict, so of equal distances the lowest index stays.
__device__ inline float fps_visit(Best& b, const Pick& old, float px, float py, float pz, float dj, unsigned i) {
  const float d2 = sqdist(px - old.x, py - old.y, pz - old.z);
  if (d2 < dj) dj = d2;  // a NaN leaves the minimum, as fminf
  if (dj > b.d) b = Best{dj, px, py, pz, i};
  return dj;
}

// The workgroup's winner from every thread's key and point.  Non-zero keys are distinct (they hold the index), so one
// lane of a wave holds the wave's maximum; a wave without a candidate reports 0, and when all do point 0 is the answer.
__device__ inline Pick fps_pick(FpsShared& sh, int buf, u64 key, float bx, float by, float bz,
                                const float* __restrict__ xyz) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 wmax = wave_max(key);
  if (wmax != 0ull ? key == wmax : lane == 0) {
    sh.key[buf][wave] = wmax;
    sh.pt[buf][wave] = make_float4(bx, by, bz, 0.f);
  }
  __syncthreads();
  const u64 mine = sh.key[buf][lane & (kFpsWaves - 1)];
  u64 k = mine;
  for (int o = kFpsWaves / 2; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(k, o, 64);
    k = t > k ? t : k;
  }
  if (k == 0ull) return Pick{0u, xyz[0], xyz[1], xyz[2]};  // uniform, and rare: not worth three registers
  const int w = __ffsll((long long)__ballot(mine == k)) - 1;  // one of the first sixteen lanes holds it
  const float4 p = sh.pt[buf][w];
  return Pick{~(unsigned)(k & 0xffffffffull), p.x, p.y, p.z};
}

// kMode 0: K points a thread with coordinates and minima in registers; 1: the minima in registers, the coordinates read
// every iteration; 2: both read every iteration, the minima in `ws`.  n0: first point, n: points, m0: first output, m:
// outputs (n, m >= 1).  Uniform over the workgroup.
template <int kMode, int K>
__device__ inline void fps_sample(const FpsArgs& a, FpsShared& sh, long long n0, unsigned n, long long m0, long long m) {
  const unsigned t = threadIdx.x;
  const float* __restrict__ xyz = a.xyz + 3 * n0;
  float* __restrict__ ws = kMode == 2 ? a.ws + n0 : nullptr;
  const int base = a.local_index ? 0 : (int)n0;
  float x[kMode == 0 ? K : 1], y[kMode == 0 ? K : 1], z[kMode == 0 ? K : 1], d[kMode == 2 ? 1 : K];
  u64 live = 0ull;  // modes 0 and 1: bit j: the point t + 1024 j exists and is a candidate
  bool bad = false;
  if constexpr (kMode != 2) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const unsigned i = t + (unsigned)j * kFpsThreads;
      d[j] = kFarAway;
      if (i < n) {
        const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
        if constexpr (kMode == 0) {
          x[j] = px;
          y[j] = py;
          z[j] = pz;
        }
        bad = bad || !(isfinite(px) && isfinite(py) && isfinite(pz));
        if (!(a.skip_origin && sqdist(px, py, pz) <= kOriginBall)) live |= 1ull << j;
      } else if constexpr (kMode == 0) {
        x[j] = y[j] = z[j] = 0.f;
      }
    }
  } else {
    for (unsigned i = t; i < n; i += kFpsThreads) {
      const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
      bad = bad || !(isfinite(px) && isfinite(py) && isfinite(pz));
      ws[i] = kFarAway;
    }
  }
  if (__ballot(bad) != 0ull && (t & 63) == 0) raise(a.status, GAPRO_QS_FLAG_NOT_FINITE);
  Pick old{0u, xyz[0], xyz[1], xyz[2]};
  if (t == 0) a.idx[m0] = base;
  for (long long s = 1; s < m; ++s) {
    Best best{-1.f, 0.f, 0.f, 0.f, 0u};
    if constexpr (kMode != 2) {
      // the candidate bits and the thread's first index are made opaque here: otherwise K loop-invariant tests and K
      // addresses are kept in registers across the iterations, and the minima no longer fit beside them
      unsigned t0 = t;
      u64 lv = live;
      asm volatile("" : "+v"(t0), "+v"(lv));
#pragma unroll
      for (int j0 = 0; j0 < K; j0 += kFpsGroup) {
        if ((unsigned)j0 * kFpsThreads >= n) break;  // uniform
        if constexpr (kMode == 0) {
#pragma unroll
          for (int g = 0; g < kFpsGroup; ++g) {
            const int j = j0 + g;
            if ((lv >> j) & 1ull) d[j] = fps_visit(best, old, x[j], y[j], z[j], d[j], t0 + (unsigned)j * kFpsThreads);
          }
        } else {  // the loads of a group are issued together: a load's latency is paid once a group, not once a point
          float px[kFpsGroup], py[kFpsGroup], pz[kFpsGroup];
#pragma unroll
          for (int g = 0; g < kFpsGroup; ++g) {  // a point beyond n reads point n - 1 and is not visited
            const unsigned i = min(t0 + (unsigned)(j0 + g) * kFpsThreads, n - 1u);
            px[g] = xyz[3 * (size_t)i];
            py[g] = xyz[3 * (size_t)i + 1];
            pz[g] = xyz[3 * (size_t)i + 2];
          }
#pragma unroll
          for (int g = 0; g < kFpsGroup; ++g) {
            const int j = j0 + g;
            if ((lv >> j) & 1ull) d[j] = fps_visit(best, old, px[g], py[g], pz[g], d[j], t0 + (unsigned)j * kFpsThreads);
          }
        }
      }
    } else {
      for (unsigned i0 = t; i0 < n; i0 += kFpsGroup * kFpsThreads) {
        float px[kFpsGroup], py[kFpsGroup], pz[kFpsGroup], dj[kFpsGroup];
#pragma unroll
        for (int g = 0; g < kFpsGroup; ++g) {
          const unsigned i = min(i0 + (unsigned)g * kFpsThreads, n - 1u);
          px[g] = xyz[3 * (size_t)i];
          py[g] = xyz[3 * (size_t)i + 1];
          pz[g] = xyz[3 * (size_t)i + 2];
          dj[g] = ws[i];
        }
#pragma unroll
        for (int g = 0; g < kFpsGroup; ++g) {
          const unsigned i = i0 + (unsigned)g * kFpsThreads;
          if (i >= n || (a.skip_origin && sqdist(px[g], py[g], pz[g]) <= kOriginBall)) continue;
          const float dn = fps_visit(best, old, px[g], py[g], pz[g], dj[g], i);
          if (dn < dj[g]) ws[i] = dn;
        }
      }
    }
    old = fps_pick(sh, (int)(s & 1), fps_key(best.d, best.i), best.x, best.y, best.z, xyz);
    if (t == 0) a.idx[m0 + s] = base + (int)old.i;
  }
  if (a.dist) {
    float* __restrict__ out = a.dist + n0;
    if constexpr (kMode != 2) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const unsigned i = t + (unsigned)j * kFpsThreads;
        if (i < n) out[i] = d[j];
      }
    } else {
      for (unsigned i = t; i < n; i += kFpsThreads) out[i] = ws[i];  // the thread's own entries
    }
  }
}

// One instantiation per path, so that each has the registers of its own path only: a workgroup whose sample belongs to
// another path returns at once, and the host launches only the paths n_points admits.
template <int kMode>
__global__ __launch_bounds__(kFpsThreads) void k_fps(FpsArgs a) {
  __shared__ FpsShared sh;
  const int b = blockIdx.x;
  long long n0, n1, m0, m1;
  const bool points_ok = range_of(a.o.off, a.o.off_i64, b, a.o.N, &n0, &n1);
  const bool outputs_ok = range_of(a.o.new_off, a.o.new_off_i64, b, a.o.M, &m0, &m1);
  const long long n = n1 - n0, m = m1 - m0;
  // everything below is uniform over the workgroup
  if (points_ok && outputs_ok && (n <= kResidentCap ? 0 : n <= kStreamedCap ? 1 : 2) != kMode) return;
  if (!points_ok || !outputs_ok) {  // its n may be anything: the first path reports it
    if (kMode == 0 && threadIdx.x == 0) raise(a.status, GAPRO_QS_FLAG_OFFSETS);
    return;
  }
  if (m == 0) return;
  if (n == 0) {
    for (long long j = threadIdx.x; j < m; j += kFpsThreads) a.idx[m0 + j] = -1;
    if (threadIdx.x == 0) raise(a.status, GAPRO_QS_FLAG_EMPTY);
    return;
  }
  fps_sample<kMode, kMode == 0 ? kResidentK : kMode == 1 ? kStreamedK : 1>(a, sh, n0, (unsigned)n, m0, m);
}

struct BqArgs {
  Offsets o;
  const float* xyz;      // [N][3]
  const float* new_xyz;  // [M][3]
  int* idx;              // [M][nsample]
  int* counts;           // [M] or null
  int* status;
  float r2;
  int nsample, local_index;
};

__global__ __launch_bounds__(kBqThreads) void k_ball_query(BqArgs a) {
  const int lane = threadIdx.x & 63, ns = a.nsample;
  if (blockIdx.x == 0) {  // both tables, whole: a decrease or an entry outside its range
    bool bad = false;
    for (int b = threadIdx.x; b < a.o.B; b += kBqThreads) {
      long long lo, hi;
      bad = bad || !range_of(a.o.off, a.o.off_i64, b, a.o.N, &lo, &hi);
      bad = bad || !range_of(a.o.new_off, a.o.new_off_i64, b, a.o.M, &lo, &hi);
    }
    if (bad) raise(a.status, GAPRO_QS_FLAG_OFFSETS);
  }
  const long long n_waves = (long long)gridDim.x * (kBqThreads / 64);
  for (long long q = (long long)blockIdx.x * (kBqThreads / 64) + (threadIdx.x >> 6); q < a.o.M; q += n_waves) {
    int* __restrict__ row = a.idx + q * ns;
    int b = 0;  // the first sample whose queries end beyond q (uniform over the wave, as everything here)
    while (b < a.o.B && q >= idx_at(a.o.new_off, a.o.new_off_i64, b)) ++b;
    long long n0 = 0, n1 = 0;
    if (b == a.o.B || !range_of(a.o.off, a.o.off_i64, b, a.o.N, &n0, &n1)) {
      if (lane == 0) raise(a.status, GAPRO_QS_FLAG_OFFSETS);  // a query of no sample, or a sample of no valid range
      n0 = n1 = 0;
    }
    const long long sub = a.local_index ? n0 : 0;
    const float qx = a.new_xyz[3 * q], qy = a.new_xyz[3 * q + 1], qz = a.new_xyz[3 * q + 2];
    int cnt = 0, first = 0;
    for (long long c0 = n0; c0 < n1 && cnt < ns; c0 += 64 * kBqUnroll) {
      bool hit[kBqUnroll];
#pragma unroll
      for (int u = 0; u < kBqUnroll; ++u) {
        const long long k = c0 + 64 * u + lane;
        hit[u] = false;
        if (k < n1) {
          const float px = a.xyz[3 * k], py = a.xyz[3 * k + 1], pz = a.xyz[3 * k + 2];
          hit[u] = sqdist(qx - px, qy - py, qz - pz) < a.r2;
        }
      }
#pragma unroll
      for (int u = 0; u < kBqUnroll; ++u) {
        const u64 mask = __ballot(hit[u]);
        if (cnt < ns && mask != 0ull) {  // uniform
          const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
          if (hit[u] && pos < ns) row[pos] = (int)(c0 + 64 * u + lane - sub);
          if (cnt == 0) first = (int)(c0 + 64 * u + (__ffsll((long long)mask) - 1) - sub);
          cnt += __popcll(mask);
        }
      }
    }
    cnt = cnt < ns ? cnt : ns;
    for (int p = cnt + lane; p < ns; p += 64) row[p] = cnt > 0 ? first : 0;
    if (a.counts && lane == 0) a.counts[q] = cnt;
  }
}

bool is_flag(int32_t v) { return v == 0 || v == 1; }

bool sizes_ok(int64_t n_points, int64_t m_total, int32_t n_samples) {
  return n_points >= 0 && n_points <= kMaxIndex && m_total >= 0 && m_total <= kMaxIndex && n_samples >= 1 &&
         n_samples <= GAPRO_QS_MAX_SAMPLES;
}

}  // namespace

extern "C" {

int gapro_fps_plan(int64_t n_max, int64_t* xyz_capacity, int64_t* capacity) {
  if (xyz_capacity) *xyz_capacity = kResidentCap;
  if (capacity) *capacity = kStreamedCap;
  if (n_max < 0 || n_max > kMaxIndex) return GAPRO_ERR_BAD_ARG;
  return n_max <= kResidentCap ? GAPRO_FPS_RESIDENT : n_max <= kStreamedCap ? GAPRO_FPS_STREAMED : GAPRO_FPS_GLOBAL;
}

size_t gapro_fps_workspace_bytes(int64_t n_points) {
  if (n_points < 0 || n_points > kMaxIndex) return 0;
  return align_up(n_points > kStreamedCap ? (size_t)n_points * sizeof(float) : 1, 256);
}

int gapro_fps_batch(gapro_ctx* ctx, void* stream_, int64_t n_points, const float* d_xyz, int32_t n_samples,
                    const void* d_offset, int32_t offset_i64, const void* d_new_offset, int32_t new_offset_i64,
                    int64_t m_total, int32_t flags, void* d_workspace, size_t workspace_bytes, int32_t* d_idx,
                    float* d_dist, int32_t* d_status, int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!sizes_ok(n_points, m_total, n_samples) || !d_offset || !d_new_offset || !d_status || !is_flag(offset_i64) ||
      !is_flag(new_offset_i64) || (flags & ~(GAPRO_FPS_SKIP_ORIGIN | GAPRO_QS_LOCAL_INDEX)) ||
      (n_points > 0 && !d_xyz) || (m_total > 0 && !d_idx))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_fps_batch: bad argument");
  if (n_points > kStreamedCap && (!d_workspace || workspace_bytes < gapro_fps_workspace_bytes(n_points)))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_fps_batch: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_QS_STATUS_WORDS * sizeof(int32_t), stream));
  if (m_total > 0) {
    FpsArgs a{};
    a.o = Offsets{d_offset, d_new_offset, offset_i64, new_offset_i64, n_samples, n_points, m_total};
    a.xyz = d_xyz;
    a.ws = n_points > kStreamedCap ? (float*)d_workspace : nullptr;
    a.idx = (int*)d_idx;
    a.dist = d_dist;
    a.status = (int*)d_status;
    a.skip_origin = (flags & GAPRO_FPS_SKIP_ORIGIN) != 0;
    a.local_index = (flags & GAPRO_QS_LOCAL_INDEX) != 0;
    hipLaunchKernelGGL(k_fps<0>, dim3(n_samples), dim3(kFpsThreads), 0, stream, a);
    if (n_points > kResidentCap) hipLaunchKernelGGL(k_fps<1>, dim3(n_samples), dim3(kFpsThreads), 0, stream, a);
    if (n_points > kStreamedCap) hipLaunchKernelGGL(k_fps<2>, dim3(n_samples), dim3(kFpsThreads), 0, stream, a);
    GAPRO_LAUNCH_CHECK(ctx);
  }
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_QS_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_ball_query_batch(gapro_ctx* ctx, void* stream_, int64_t n_points, const float* d_xyz, int64_t m_total,
                           const float* d_new_xyz, int32_t n_samples, const void* d_offset, int32_t offset_i64,
                           const void* d_new_offset, int32_t new_offset_i64, double radius, int32_t nsample,
                           int32_t flags, int32_t* d_idx, int32_t* d_counts, int32_t* d_status,
                           int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!sizes_ok(n_points, m_total, n_samples) || !d_offset || !d_new_offset || !d_status || !is_flag(offset_i64) ||
      !is_flag(new_offset_i64) || (flags & ~GAPRO_QS_LOCAL_INDEX) || (n_points > 0 && !d_xyz) ||
      (m_total > 0 && (!d_idx || !d_new_xyz)) || nsample < 1 || nsample > GAPRO_BALL_QUERY_MAX_NSAMPLE ||
      m_total * (int64_t)nsample > kMaxIndex || !std::isfinite(radius))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_ball_query_batch: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_QS_STATUS_WORDS * sizeof(int32_t), stream));
  if (m_total > 0) {
    const float r = (float)radius;
    BqArgs a{};
    a.o = Offsets{d_offset, d_new_offset, offset_i64, new_offset_i64, n_samples, n_points, m_total};
    a.xyz = d_xyz;
    a.new_xyz = d_new_xyz;
    a.idx = (int*)d_idx;
    a.counts = (int*)d_counts;
    a.status = (int*)d_status;
    a.r2 = r * r;
    a.nsample = nsample;
    a.local_index = (flags & GAPRO_QS_LOCAL_INDEX) != 0;
    hipLaunchKernelGGL(k_ball_query, dim3(grid_for(m_total * 64, 1, 1 << 16)), dim3(kBqThreads), 0, stream, a);
    GAPRO_LAUNCH_CHECK(ctx);
  }
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_QS_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

}  // extern "C"
