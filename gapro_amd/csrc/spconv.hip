// The consumers' sparse 3D convolutions (include/gapro_hip.h, "Sparse convolutions"): spconv's
// SubMConv3d(k = 3, padding = 1), SparseConv3d(k = 2, stride = 2) and SparseInverseConv3d(k = 2), the three layers the
// U-Nets of ISBNet (isbnet/model/blocks.py:158-255) and SPFormer (spformer/model/backbone.py:38-208) are built from.
// The plans:
//   k_sp_insert        a thread a row: the packed key of (batch, z, y, x) into an open-addressing table of 64-bit keys by
//                      compare-and-swap; the value of a slot is the row.  A key packs every axis with one cell of margin
//                      on both sides, so that the key of a probe at -1 or at D is the key of no voxel.
//   k_sp_neighbours    a thread per (offset, row), rows fastest: nbr[27][V], the row at p + d or -1.
//   k_sp_down_insert   the coarse key (b, z >> 1, y >> 1, x >> 1) into the table; per slot the first child by an integer
//                      atomic minimum and the mask of child slots by an atomic or (a bit set twice is a duplicate row).
//   scan_enqueue       a row is "first" iff its slot's minimum is the row; the exclusive scan of those flags (scan.h,
//                      three launches) numbers the coarse rows by their first child in ascending input row.
//   k_sp_down_fill     coarse_coords, children[8][V_c], parent[V], child_slot[V].
// The convolutions, all three layers and their input gradients through ONE kernel:
//   k_spconv<NB>       a workgroup of four waves takes 64 output rows, a wave 16 of them, and 16 NB output channels,
//                      NB = 1, 2, 4 or 8 (grid.y takes the rest).  For every table offset k that any of the workgroup's
//                      rows has a pair at, and every chunk of 32 input channels: the weight slice W_k[chunk][channels] goes to LDS once for
//                      the four waves (float32, as given); a lane fetches two float4 of its row's neighbour; FP64 MFMA
//                      products y[16 rows x 16 channels] += X[16 x 4] W^T[4 x 16] with the rows as the A operand, whose
//                      block rotations (mfma64.h) are then made once per step and shared by the NB channel blocks.  A
//                      wave skips an offset none of its rows has a pair at.  The input gradient is this kernel on the
//                      transposed table with the weights read through other strides.
//   k_spconv_wgrad     dW[k] = sum_rows g[r] (x) x[tab[k][r]]: MFMA products with the ROWS as the contraction, a wave per
//                      16 x 64 tile of (C_out, C_in), a workgroup per (row chunk, k, four tiles); float64 partials per
//                      chunk, added in ascending chunk order and rounded once by k_spconv_wfinish.  k_spconv_bias_part:
//                      the column sums of g by the same two stages.
// Arithmetic: float64 from the float32 inputs, one rounding on the store; no floating-point atomics; the order of every
// sum is fixed by this layout and does not depend on the other rows of a tile (a missing pair adds exact zeros).
#include "common.h"
#include "launch_util.h"
#include "mfma64.h"
#include "scan.h"
#include "voxel_hash.h"

#include <cstdint>

namespace {

using gapro_mfma::AFrag;
using gapro_mfma::d4;
using gapro_mfma::make_afrag;
using gapro_mfma::mma16;
using gapro_mfma::unrotate;

constexpr int kThreads = 256, kWaves = 4, kTile = 16;
constexpr int kRowsWg = kWaves * kTile;            // output rows of a k_spconv workgroup
constexpr int kChunkC = GAPRO_SPCONV_CIN_CHUNK;    // input channels of one weight slice in LDS
constexpr int kGridCap = 1 << 16;
constexpr long long kMaxRows = GAPRO_SPCONV_MAX_ROWS;
constexpr int kMaxC = GAPRO_SPCONV_MAX_CHANNELS;
constexpr int kMinChunkRows = GAPRO_SPCONV_MIN_CHUNK_ROWS;
constexpr size_t kPartBudget = (size_t)GAPRO_SPCONV_PARTIAL_BYTES;
static_assert(kChunkC == 32, "a lane fetches two float4 of a chunk");

typedef unsigned long long u64;
constexpr u64 kEmptyKey = ~0ULL;

// ---- plans ---------------------------------------------------------------------------------------------------------------
struct Geo {
  const void* coords;  // [n][4]: batch, z, y, x
  long long n;
  int i64, B;
  int D[3], Do[3];     // the extents and the strided layer's output extents
};

__device__ inline long long coord_at(const Geo& g, long long i, int c) {
  return g.i64 ? ((const long long*)g.coords)[4 * i + c] : (long long)((const int*)g.coords)[4 * i + c];
}

// a row's coordinates; false (and the flag raised) for a batch index or a coordinate outside the grid
__device__ inline bool read_row(const Geo& g, long long i, long long (&p)[4], int* status) {
#pragma unroll
  for (int c = 0; c < 4; ++c) p[c] = coord_at(g, i, c);
  if (p[0] < 0 || p[0] >= g.B) {
    raise_bad_arg(status, GAPRO_SPCONV_FLAG_BATCH);
    return false;
  }
  if (p[1] < 0 || p[1] >= g.D[0] || p[2] < 0 || p[2] >= g.D[1] || p[3] < 0 || p[3] >= g.D[2]) {
    raise_bad_arg(status, GAPRO_SPCONV_FLAG_RANGE);
    return false;
  }
  return true;
}

// every axis with a cell of margin on both sides: for z in [-1, D] the key is that of no other (b, z, y, x)
__device__ inline u64 fine_key(const Geo& g, long long b, long long z, long long y, long long x) {
  return (((u64)b * (u64)(g.D[0] + 2) + (u64)(z + 1)) * (u64)(g.D[1] + 2) + (u64)(y + 1)) * (u64)(g.D[2] + 2) +
         (u64)(x + 1);
}
__device__ inline u64 coarse_key(const Geo& g, long long b, long long z, long long y, long long x) {
  return (((u64)b * (u64)g.Do[0] + (u64)z) * (u64)g.Do[1] + (u64)y) * (u64)g.Do[2] + (u64)x;
}

// the slot of `key`, claimed if no row had it; -1: the table is full (more rows than slots: not built).  *fresh: claimed.
__device__ inline long long claim(u64* keys, u64 mask, u64 key, bool* fresh) {
  u64 s = gapro_vox_mix(key) & mask;
  for (u64 probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {  // bounded by the table
    const u64 held = atomicCAS(keys + s, kEmptyKey, key);
    if (held == kEmptyKey || held == key) {
      *fresh = held == kEmptyKey;
      return (long long)s;
    }
  }
  return -1;
}

__device__ inline int find(const u64* __restrict__ keys, const int* __restrict__ vals, u64 mask, u64 key) {
  u64 s = gapro_vox_mix(key) & mask;
  for (u64 probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
    const u64 held = keys[s];
    if (held == key) return vals[s];
    if (held == kEmptyKey) return -1;
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void k_sp_insert(Geo g, u64* keys, int* __restrict__ vals, u64 mask,
                                                        int* status) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < g.n; i += stride) {
    long long p[4];
    if (!read_row(g, i, p, status)) continue;
    bool fresh = false;
    const long long s = claim(keys, mask, fine_key(g, p[0], p[1], p[2], p[3]), &fresh);
    if (s < 0) raise_bad_arg(status, GAPRO_SPCONV_FLAG_TABLE);
    else if (!fresh) raise_bad_arg(status, GAPRO_SPCONV_FLAG_DUPLICATE);
    else vals[s] = (int)i;  // read by the next kernel only
  }
}

__global__ __launch_bounds__(kThreads) void k_sp_neighbours(Geo g, const u64* __restrict__ keys,
                                                            const int* __restrict__ vals, u64 mask,
                                                            int* __restrict__ nbr) {
  const long long total = 27 * g.n, stride = (long long)gridDim.x * kThreads;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int k = (int)(e / g.n);
    const long long r = e - (long long)k * g.n;
    const long long b = coord_at(g, r, 0);
    const long long z = coord_at(g, r, 1) + (k / 9 - 1), y = coord_at(g, r, 2) + (k / 3 % 3 - 1),
                    x = coord_at(g, r, 3) + (k % 3 - 1);
    int t = -1;
    // a row outside the grid (flagged by the insert) has no pairs; a probe outside [0, D) would miss by the packing
    if (b >= 0 && b < g.B && z >= 0 && z < g.D[0] && y >= 0 && y < g.D[1] && x >= 0 && x < g.D[2] &&
        coord_at(g, r, 1) < g.D[0] && coord_at(g, r, 2) < g.D[1] && coord_at(g, r, 3) < g.D[2] &&
        coord_at(g, r, 1) >= 0 && coord_at(g, r, 2) >= 0 && coord_at(g, r, 3) >= 0)
      t = find(keys, vals, mask, fine_key(g, b, z, y, x));
    nbr[e] = t;
  }
}

__device__ inline int child_of(const long long (&p)[4]) { return (int)(((p[1] & 1) << 2) | ((p[2] & 1) << 1) | (p[3] & 1)); }

__global__ __launch_bounds__(kThreads) void k_sp_down_insert(Geo g, u64* keys, int* first, int* child_mask, u64 mask,
                                                             int* __restrict__ slot, int* status) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < g.n; i += stride) {
    long long p[4];
    int mine = -1;
    if (read_row(g, i, p, status)) {
      const long long z = p[1] >> 1, y = p[2] >> 1, x = p[3] >> 1;
      if (z < g.Do[0] && y < g.Do[1] && x < g.Do[2]) {  // else the last slice of an odd extent: in no coarse voxel
        bool fresh = false;
        const long long s = claim(keys, mask, coarse_key(g, p[0], z, y, x), &fresh);
        if (s < 0) {
          raise_bad_arg(status, GAPRO_SPCONV_FLAG_TABLE);
        } else {
          atomicMin(first + s, (int)i);
          const int bit = 1 << child_of(p);
          if (atomicOr(child_mask + s, bit) & bit) raise_bad_arg(status, GAPRO_SPCONV_FLAG_DUPLICATE);
          mine = (int)s;
        }
      }
    }
    slot[i] = mine;
  }
}

// the scan's value: is row i (< n) the first child of its coarse voxel
struct IsFirst {
  const int* __restrict__ first;
  const int* __restrict__ slot;
  __device__ int operator()(long long i) const {
    const int s = slot[i];
    return (s >= 0 && first[s] == (int)i) ? 1 : 0;
  }
};

// the scan's result: the firsts before row i
struct EmitRank {
  int* __restrict__ rank;
  __device__ void operator()(long long i, int r, int) const { rank[i] = r; }
};

__global__ __launch_bounds__(kThreads) void k_sp_down_fill(Geo g, const int* __restrict__ first,
                                                           const int* __restrict__ slot, const int* __restrict__ rank,
                                                           long long n_out, int* __restrict__ coarse,
                                                           int* __restrict__ children, int* __restrict__ parent,
                                                           int* __restrict__ child_slot, int* status) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < g.n; i += stride) {
    long long p[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) p[c] = coord_at(g, i, c);
    const int s = slot[i], child = child_of(p);
    int q = -1;
    if (s >= 0) {
      const int f = first[s];
      q = (f >= 0 && f < g.n) ? rank[f] : -1;
      if (q < 0 || q >= n_out) {  // not the count's workspace, or not its n_out
        raise_bad_arg(status, GAPRO_SPCONV_FLAG_TABLE);
        q = -1;
      }
    }
    parent[i] = q;
    child_slot[i] = child;
    if (q >= 0) {
      children[(long long)child * n_out + q] = (int)i;
      if (first[s] == (int)i) {
        coarse[4 * (long long)q + 0] = (int)p[0];
        coarse[4 * (long long)q + 1] = (int)(p[1] >> 1);
        coarse[4 * (long long)q + 2] = (int)(p[2] >> 1);
        coarse[4 * (long long)q + 3] = (int)(p[3] >> 1);
      }
    }
  }
}

// the workspace of a plan over n rows; every part is aligned to 256 bytes
struct PlanWs {
  u64* keys;        // [slots]
  int* vals;        // [slots] subm: the row of a key; down: the first child of a coarse key
  int* child_mask;  // [slots] down
  int* slot;        // [n] down: the slot of a row's coarse voxel; -1: in none
  int* rank;        // [n] down: firsts before the row
  int* block_sums;  // [scan_blocks(n)]
  size_t bytes;
};

PlanWs plan_layout(void* base, long long n, bool down) {
  PlanWs w{};
  Carver c(base);
  const size_t slots = (size_t)gapro_vox_slots(n);
  w.keys = c.take<u64>(slots);
  w.vals = c.take<int>(slots);
  if (down) {
    w.child_mask = c.take<int>(slots);
    w.slot = c.take<int>((size_t)n);
    w.rank = c.take<int>((size_t)n);
    w.block_sums = c.take<int>((size_t)scan_blocks(n));
  }
  w.bytes = c.bytes();
  return w;
}

// the geometry of a call; false for extents the key packing cannot hold
bool fill_geo(Geo* g, int64_t n_rows, const void* d_coords, int32_t coords_i64, const int32_t* h_shape, int32_t B) {
  if (n_rows < 1 || n_rows > kMaxRows || !d_coords || (coords_i64 != 0 && coords_i64 != 1) || !h_shape || B < 1)
    return false;
  unsigned __int128 cells = (unsigned __int128)B;
  for (int c = 0; c < 3; ++c) {
    if (h_shape[c] < 1 || h_shape[c] > 0x7ffffffd) return false;
    cells *= (unsigned __int128)(h_shape[c] + 2);
    g->D[c] = h_shape[c];
    g->Do[c] = h_shape[c] >= 2 ? (h_shape[c] - 2) / 2 + 1 : 0;
  }
  if (cells >= ((unsigned __int128)1 << 63)) return false;  // kEmptyKey stays no voxel's key
  g->coords = d_coords;
  g->n = n_rows;
  g->i64 = coords_i64;
  g->B = B;
  return true;
}

// ---- the gather-GEMM --------------------------------------------------------------------------------------------------------
// A table in one of two forms: tab[K][R_out] (k_of == NULL), or "one of K": tab[R_out] and k_of[R_out], the pair of row
// r being (k_of[r], tab[r]).  An entry outside [0, R_in) is no pair.
struct Table {
  const int* tab;
  const int* k_of;
  long long R_out, R_in;
  int K;
};
__device__ inline int pair_at(const Table& t, int k, long long r) {
  int v;
  if (t.k_of) v = t.k_of[r] == k ? t.tab[r] : -1;
  else v = t.tab[(long long)k * t.R_out + r];
  return (v >= 0 && v < t.R_in) ? v : -1;
}

struct ConvArgs {
  Table t;
  int Ci, Co, reverse_k;        // contracted and produced channels of THIS launch; weights of offset K - 1 - k
  long long ws_o, ws_k, ws_i;   // the weight of (produced o, offset k, contracted i) is w[o ws_o + k ws_k + i ws_i]
  const float *x, *w, *bias;
  float* y;
};

template <int NB>
__global__ __launch_bounds__(kThreads) void k_spconv(ConvArgs a) {
  constexpr int CO = NB * 16, LDW = CO + 16;  // LDW = 16 (mod 32): the two lane groups of a 32-lane LDS read differ
  __shared__ float wl[kChunkC * LDW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
  const long long r0 = (long long)blockIdx.x * kRowsWg + wave * kTile;
  const int co0 = blockIdx.y * CO;
  const bool vec = (a.Ci & 3) == 0, ci_fast = a.ws_i == 1;
  const int nb_live = (a.Co - co0 + 15) / 16;  // the last group of channel blocks may be short: no product on padding
  d4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = d4{0.0, 0.0, 0.0, 0.0};

  for (int k = 0; k < a.t.K; ++k) {  // uniform over the workgroup
    const long long r = r0 + i;
    const int t = r < a.t.R_out ? pair_at(a.t, k, r) : -1;
    const bool wave_has = __ballot(t >= 0) != 0ULL;
    if (!__syncthreads_or(wave_has ? 1 : 0)) continue;  // no row of the workgroup has a pair at k
    const long long wk = (long long)(a.reverse_k ? a.t.K - 1 - k : k) * a.ws_k;
    const float* __restrict__ xr = a.x + (long long)(t >= 0 ? t : 0) * a.Ci;
    for (int c0 = 0; c0 < a.Ci; c0 += kChunkC) {
      // the lane's eight channels of the chunk: c0 + 16 u + 4 g + (0 .. 3); in flight under the weight slice
      float xv[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = c0 + 16 * u + 4 * g;
        if (t >= 0 && vec && c < a.Ci) {
          const float4 v = *(const float4*)(xr + c);
          xv[u][0] = v.x, xv[u][1] = v.y, xv[u][2] = v.z, xv[u][3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) xv[u][j] = (t >= 0 && c + j < a.Ci) ? xr[c + j] : 0.f;
        }
      }
      __syncthreads();  // every wave has left the slice before
      for (int e = threadIdx.x; e < kChunkC * CO; e += kThreads) {
        int cl, ol;
        if (ci_fast) {  // 8 consecutive contracted channels of 8 produced ones a quarter wave
          cl = (e & 7) + 8 * ((e >> 6) & 3);
          ol = ((e >> 3) & 7) + 8 * (e >> 8);
        } else {
          ol = e % CO;
          cl = e / CO;
        }
        const int o = co0 + ol, c = c0 + cl;
        wl[cl * LDW + ol] = (o < a.Co && c < a.Ci) ? a.w[o * a.ws_o + wk + c * a.ws_i] : 0.f;
      }
      __syncthreads();
      if (!wave_has) continue;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (c0 + 16 * u >= a.Ci) break;  // uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const AFrag af = make_afrag((double)xv[u][j]);
          const float* __restrict__ wrow = wl + (16 * u + 4 * g + j) * LDW + i;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            if (nb < nb_live) mma16(af, (double)wrow[nb * 16], acc[nb]);  // uniform
        }
      }
    }
  }
  // register r of a block: row g + 4 r of the wave's 16, produced channel i of the block's 16
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const d4 v = unrotate(acc[nb]);
    const int o = co0 + nb * 16 + i;
    if (o >= a.Co) continue;
    const double b = a.bias ? (double)a.bias[o] : 0.0;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const long long row = r0 + g + 4 * rr;
      if (row < a.t.R_out) a.y[row * a.Co + o] = (float)(v[rr] + b);
    }
  }
}

int launch_conv(gapro_ctx* ctx, hipStream_t stream, const ConvArgs& a) {
  const int blocks16 = (a.Co + 15) / 16;
  const long long gx = (a.t.R_out + kRowsWg - 1) / kRowsWg;
  if (gx > 0x7fffffffLL) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spconv: too many rows");
#define GAPRO_SPCONV_LAUNCH(NB)                                                                                \
  hipLaunchKernelGGL(k_spconv<NB>, dim3((unsigned)gx, (unsigned)((blocks16 + NB - 1) / NB)), dim3(kThreads), 0, \
                     stream, a)
  if (blocks16 <= 1) GAPRO_SPCONV_LAUNCH(1);
  else if (blocks16 <= 2) GAPRO_SPCONV_LAUNCH(2);
  else if (blocks16 <= 4) GAPRO_SPCONV_LAUNCH(4);
  else GAPRO_SPCONV_LAUNCH(8);  // beyond 128 channels grid.y takes groups of 8 blocks
#undef GAPRO_SPCONV_LAUNCH
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

// ---- the weight gradient ----------------------------------------------------------------------------------------------------
constexpr int kWgNI = 4;  // 16-channel blocks of C_in in a wave's tile

struct WgradArgs {
  Table t;
  int Ci, Co;
  const float *x, *gy;
  double *part, *bias_part;  // [n_chunks][K][Co][Ci], [n_chunks][Co]
  long long chunk_rows;
  int n_chunks;
};

__global__ __launch_bounds__(kThreads) void k_spconv_wgrad(WgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
  const int n_ig = (a.Ci + 16 * kWgNI - 1) / (16 * kWgNI), n_cb = (a.Co + 15) / 16;
  const int tile = blockIdx.z * kWaves + wave;
  if (tile >= n_cb * n_ig) return;  // no barrier in this kernel
  const int cb = tile / n_ig, ig = tile - cb * n_ig, k = blockIdx.y;
  const long long ra = (long long)blockIdx.x * a.chunk_rows;
  const long long rb = ra + a.chunk_rows < a.t.R_out ? ra + a.chunk_rows : a.t.R_out;
  const int co = cb * 16 + i, ci0 = ig * 16 * kWgNI + i;
  d4 acc[kWgNI];
#pragma unroll
  for (int n = 0; n < kWgNI; ++n) acc[n] = d4{0.0, 0.0, 0.0, 0.0};
  for (long long r16 = ra; r16 < rb; r16 += 16) {
    float av[4], bv[4][kWgNI];
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // step s contracts the rows r16 + 4 s + (0 .. 3)
      const long long row = r16 + 4 * s + g;
      const int t = row < rb ? pair_at(a.t, k, row) : -1;
      any = any || t >= 0;
      av[s] = (t >= 0 && co < a.Co) ? a.gy[row * a.Co + co] : 0.f;
#pragma unroll
      for (int n = 0; n < kWgNI; ++n)
        bv[s][n] = (t >= 0 && ci0 + 16 * n < a.Ci) ? a.x[(long long)t * a.Ci + ci0 + 16 * n] : 0.f;
    }
    if (__ballot(any) == 0ULL) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const AFrag af = make_afrag((double)av[s]);
#pragma unroll
      for (int n = 0; n < kWgNI; ++n) mma16(af, (double)bv[s][n], acc[n]);
    }
  }
  double* __restrict__ out = a.part + ((long long)blockIdx.x * a.t.K + k) * a.Co * a.Ci;
#pragma unroll
  for (int n = 0; n < kWgNI; ++n) {
    const d4 v = unrotate(acc[n]);
    const int ci = ci0 + 16 * n;
    if (ci >= a.Ci) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int o = cb * 16 + g + 4 * rr;
      if (o < a.Co) out[(long long)o * a.Ci + ci] = v[rr];
    }
  }
}

// the column sums of g over a chunk's rows, ascending
__global__ __launch_bounds__(kThreads) void k_spconv_bias_part(WgradArgs a) {
  const long long ra = (long long)blockIdx.x * a.chunk_rows;
  const long long rb = ra + a.chunk_rows < a.t.R_out ? ra + a.chunk_rows : a.t.R_out;
  for (int o = threadIdx.x; o < a.Co; o += kThreads) {
    double s = 0.0;
    for (long long r = ra; r < rb; ++r) s += (double)a.gy[r * a.Co + o];
    a.bias_part[(long long)blockIdx.x * a.Co + o] = s;
  }
}

// the chunks in ascending order, one rounding: dW[C_out][K][C_in] and dbias[C_out]
__global__ __launch_bounds__(kThreads) void k_spconv_wfinish(WgradArgs a, float* __restrict__ dw,
                                                             float* __restrict__ dbias) {
  const long long per_k = (long long)a.Co * a.Ci, nw = dw ? per_k * a.t.K : 0, total = nw + (dbias ? a.Co : 0);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    double s = 0.0;
    if (e < nw) {
      const long long o = e / ((long long)a.t.K * a.Ci), rem = e - o * a.t.K * a.Ci;
      const long long k = rem / a.Ci, c = rem - k * a.Ci;
      const double* __restrict__ p = a.part + (k * a.Co + o) * a.Ci + c;
      for (int ch = 0; ch < a.n_chunks; ++ch) s += p[(long long)ch * a.t.K * per_k];
      dw[e] = (float)s;
    } else {
      const long long o = e - nw;
      for (int ch = 0; ch < a.n_chunks; ++ch) s += a.bias_part[(long long)ch * a.Co + o];
      dbias[o] = (float)s;
    }
  }
}

bool conv_sizes_ok(int64_t rows_out, int64_t rows_in, int32_t K, int32_t c_in, int32_t c_out) {
  return rows_out >= 1 && rows_out <= kMaxRows && rows_in >= 1 && rows_in <= kMaxRows && K >= 1 && K <= 27 &&
         c_in >= 1 && c_in <= kMaxC && c_out >= 1 && c_out <= kMaxC;
}

long long chunk_rows_of(int64_t rows, int32_t K, int32_t c_in, int32_t c_out) {
  const size_t per_chunk = ((size_t)K * c_in * c_out + c_out) * sizeof(double);
  long long max_chunks = (long long)(kPartBudget / per_chunk);
  if (max_chunks < 1) max_chunks = 1;
  long long rows_per = (rows + max_chunks - 1) / max_chunks;
  rows_per = (rows_per + 63) / 64 * 64;
  return rows_per < kMinChunkRows ? kMinChunkRows : rows_per;
}

Table table_of(int64_t rows_out, int64_t rows_in, int32_t K, const int32_t* d_table, const int32_t* d_k_of) {
  return Table{(const int*)d_table, (const int*)d_k_of, rows_out, rows_in, K};
}

}  // namespace

extern "C" {

size_t gapro_spconv_subm_plan_workspace_bytes(int64_t n_rows) {
  if (n_rows < 1 || n_rows > kMaxRows) return 0;
  return plan_layout(nullptr, n_rows, false).bytes;
}

int gapro_spconv_subm_plan(gapro_ctx* ctx, void* stream_, int64_t n_rows, const void* d_coords, int32_t coords_i64,
                           const int32_t* h_spatial_shape, int32_t batch_size, void* d_workspace,
                           size_t workspace_bytes, int32_t* d_neighbours, int32_t* d_status,
                           int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  Geo g{};
  if (!fill_geo(&g, n_rows, d_coords, coords_i64, h_spatial_shape, batch_size) || !d_neighbours || !d_status)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG,
                      "gapro_spconv_subm_plan: bad argument, or batch_size and spatial_shape beyond the 63-bit key");
  if (!d_workspace || workspace_bytes < gapro_spconv_subm_plan_workspace_bytes(n_rows))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_spconv_subm_plan: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const PlanWs w = plan_layout(d_workspace, n_rows, false);
  const u64 slots = (u64)gapro_vox_slots(n_rows);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_SPCONV_STATUS_WORDS * sizeof(int32_t), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.keys, 0xff, (size_t)slots * sizeof(u64), stream));  // kEmptyKey
  hipLaunchKernelGGL(k_sp_insert, dim3(grid_for(n_rows, 1, kGridCap)), dim3(kThreads), 0, stream, g, w.keys, w.vals,
                     slots - 1, (int*)d_status);
  hipLaunchKernelGGL(k_sp_neighbours, dim3(grid_for(27 * n_rows, 1, kGridCap)), dim3(kThreads), 0, stream, g, w.keys,
                     w.vals, slots - 1, (int*)d_neighbours);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_SPCONV_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

size_t gapro_spconv_down_plan_workspace_bytes(int64_t n_rows) {
  if (n_rows < 1 || n_rows > kMaxRows) return 0;
  return plan_layout(nullptr, n_rows, true).bytes;
}

int gapro_spconv_down_count(gapro_ctx* ctx, void* stream_, int64_t n_rows, const void* d_coords, int32_t coords_i64,
                            const int32_t* h_spatial_shape, int32_t batch_size, void* d_workspace,
                            size_t workspace_bytes, int32_t* d_header, int32_t* h_header_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  Geo g{};
  if (!fill_geo(&g, n_rows, d_coords, coords_i64, h_spatial_shape, batch_size) || !d_header)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG,
                      "gapro_spconv_down_count: bad argument, or batch_size and spatial_shape beyond the 63-bit key");
  if (!d_workspace || workspace_bytes < gapro_spconv_down_plan_workspace_bytes(n_rows))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_spconv_down_count: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const PlanWs w = plan_layout(d_workspace, n_rows, true);
  const u64 slots = (u64)gapro_vox_slots(n_rows);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_header, 0, GAPRO_SPCONV_STATUS_WORDS * sizeof(int32_t), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.keys, 0xff, (size_t)slots * sizeof(u64), stream));   // kEmptyKey
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.vals, 0x7f, (size_t)slots * sizeof(int), stream));   // above every row
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.child_mask, 0, (size_t)slots * sizeof(int), stream));
  hipLaunchKernelGGL(k_sp_down_insert, dim3(grid_for(n_rows, 1, kGridCap)), dim3(kThreads), 0, stream, g, w.keys,
                     w.vals, w.child_mask, slots - 1, w.slot, (int*)d_header);
  scan_enqueue(stream, IsFirst{w.vals, w.slot}, EmitRank{w.rank}, (long long)n_rows, w.block_sums,
               (int*)d_header + 2);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_header_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_header_pinned, d_header, GAPRO_SPCONV_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_spconv_down_fill(gapro_ctx* ctx, void* stream_, int64_t n_rows, const void* d_coords, int32_t coords_i64,
                           const int32_t* h_spatial_shape, int32_t batch_size, int64_t n_out,
                           const void* d_workspace, size_t workspace_bytes, int32_t* d_coarse_coords,
                           int32_t* d_children, int32_t* d_parent, int32_t* d_child_slot, int32_t* d_status,
                           int32_t* h_status_pinned) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  Geo g{};
  if (!fill_geo(&g, n_rows, d_coords, coords_i64, h_spatial_shape, batch_size) || n_out < 0 || n_out > n_rows ||
      !d_parent || !d_child_slot || !d_status || (n_out > 0 && (!d_coarse_coords || !d_children)))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spconv_down_fill: bad argument");
  if (!d_workspace || workspace_bytes < gapro_spconv_down_plan_workspace_bytes(n_rows))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_spconv_down_fill: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const PlanWs w = plan_layout((void*)d_workspace, n_rows, true);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, GAPRO_SPCONV_STATUS_WORDS * sizeof(int32_t), stream));
  if (n_out > 0)
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_children, 0xff, (size_t)(8 * n_out) * sizeof(int32_t), stream));  // -1
  hipLaunchKernelGGL(k_sp_down_fill, dim3(grid_for(n_rows, 1, kGridCap)), dim3(kThreads), 0, stream, g, w.vals, w.slot,
                     w.rank, (long long)n_out, (int*)d_coarse_coords, (int*)d_children, (int*)d_parent,
                     (int*)d_child_slot, (int*)d_status);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_SPCONV_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int64_t gapro_spconv_chunk_rows(int64_t rows_out, int32_t K, int32_t c_in, int32_t c_out) {
  if (!conv_sizes_ok(rows_out, 1, K, c_in, c_out)) return 0;
  return chunk_rows_of(rows_out, K, c_in, c_out);
}

size_t gapro_spconv_workspace_bytes(int64_t rows_out, int32_t K, int32_t c_in, int32_t c_out) {
  if (!conv_sizes_ok(rows_out, 1, K, c_in, c_out)) return 0;
  const long long cr = chunk_rows_of(rows_out, K, c_in, c_out), n_chunks = (rows_out + cr - 1) / cr;
  return align_up((size_t)n_chunks * K * c_in * c_out * sizeof(double), 256) +
         align_up((size_t)n_chunks * c_out * sizeof(double), 256);
}

int gapro_spconv_forward(gapro_ctx* ctx, void* stream_, int64_t rows_out, int64_t rows_in, int32_t K,
                         const int32_t* d_table, const int32_t* d_k_of, int32_t c_in, int32_t c_out, const float* d_x,
                         const float* d_weight, const float* d_bias, float* d_y) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!conv_sizes_ok(rows_out, rows_in, K, c_in, c_out) || !d_table || !d_x || !d_weight || !d_y)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spconv_forward: bad argument");
  ConvArgs a{};
  a.t = table_of(rows_out, rows_in, K, d_table, d_k_of);
  a.Ci = c_in, a.Co = c_out, a.reverse_k = 0;
  a.ws_o = (long long)K * c_in, a.ws_k = c_in, a.ws_i = 1;
  a.x = d_x, a.w = d_weight, a.bias = d_bias, a.y = d_y;
  return launch_conv(ctx, (hipStream_t)stream_, a);
}

int gapro_spconv_backward_input(gapro_ctx* ctx, void* stream_, int64_t rows_out, int64_t rows_in, int32_t K,
                                const int32_t* d_table_t, const int32_t* d_k_of, int32_t reverse_k, int32_t c_in,
                                int32_t c_out, const float* d_grad_y, const float* d_weight, float* d_grad_x) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!d_grad_x) return GAPRO_OK;  // not asked for: not launched
  if (!conv_sizes_ok(rows_out, rows_in, K, c_in, c_out) || !d_table_t || !d_grad_y || !d_weight ||
      (reverse_k != 0 && reverse_k != 1))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spconv_backward_input: bad argument");
  ConvArgs a{};
  a.t = table_of(rows_out, rows_in, K, d_table_t, d_k_of);
  a.Ci = c_out, a.Co = c_in, a.reverse_k = reverse_k;  // produces the layer's C_in from its C_out
  a.ws_o = 1, a.ws_k = c_in, a.ws_i = (long long)K * c_in;
  a.x = d_grad_y, a.w = d_weight, a.bias = nullptr, a.y = d_grad_x;
  return launch_conv(ctx, (hipStream_t)stream_, a);
}

int gapro_spconv_backward_weight(gapro_ctx* ctx, void* stream_, int64_t rows_out, int64_t rows_in, int32_t K,
                                 const int32_t* d_table, const int32_t* d_k_of, int32_t c_in, int32_t c_out,
                                 const float* d_x, const float* d_grad_y, void* d_workspace, size_t workspace_bytes,
                                 float* d_grad_weight, float* d_grad_bias) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!d_grad_weight && !d_grad_bias) return GAPRO_OK;  // not asked for: not launched
  if (!conv_sizes_ok(rows_out, rows_in, K, c_in, c_out) || !d_table || !d_x || !d_grad_y)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spconv_backward_weight: bad argument");
  if (!d_workspace || workspace_bytes < gapro_spconv_workspace_bytes(rows_out, K, c_in, c_out))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_spconv_backward_weight: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  WgradArgs a{};
  a.t = table_of(rows_out, rows_in, K, d_table, d_k_of);
  a.Ci = c_in, a.Co = c_out;
  a.x = d_x, a.gy = d_grad_y;
  a.chunk_rows = chunk_rows_of(rows_out, K, c_in, c_out);
  a.n_chunks = (int)((rows_out + a.chunk_rows - 1) / a.chunk_rows);
  a.part = (double*)d_workspace;
  a.bias_part = (double*)((char*)d_workspace + align_up((size_t)a.n_chunks * K * c_in * c_out * sizeof(double), 256));
  if (d_grad_weight) {
    const int tiles = ((c_out + 15) / 16) * ((c_in + 16 * kWgNI - 1) / (16 * kWgNI));
    hipLaunchKernelGGL(k_spconv_wgrad, dim3((unsigned)a.n_chunks, (unsigned)K, (unsigned)((tiles + kWaves - 1) / kWaves)),
                       dim3(kThreads), 0, stream, a);
  }
  if (d_grad_bias) hipLaunchKernelGGL(k_spconv_bias_part, dim3((unsigned)a.n_chunks), dim3(kThreads), 0, stream, a);
  const long long total = (d_grad_weight ? (long long)K * c_in * c_out : 0) + (d_grad_bias ? c_out : 0);
  hipLaunchKernelGGL(k_spconv_wfinish, dim3(grid_for(total, 1, kGridCap)), dim3(kThreads), 0, stream, a, d_grad_weight,
                     d_grad_bias);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
