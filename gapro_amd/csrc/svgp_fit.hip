// Host entry of the batched whitened-SVGP classifier fit: gapro_svgp_fit_batch[_ex, _state] routes every fit of a launch
// to one of the fit kernels (fit_route), plans the launches on the host as data (plan_fit_launch) and issues them side
// by side from one loop through their launch functions (common.h); workspace planning, the fit timing API and
// k_fit_cond, the conditioning figure of every fit.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "fit_layout.h"

using namespace gapro_fit;

// Conditioning figure of every fit of a launch (round 6): every kernel leaves the inverses of the 16 x 16 diagonal blocks of
// its LAST Cholesky factor in the fit's workspace (f.dinv: the triangular solves read them; the wave-per-fit kernel, which
// keeps L^-1 on chip, stores the diagonal on its way out), and the diagonal of L^-1 is 1 / L_jj.  One wave per fit:
// cond[slot] = (max_j L_jj / min_j L_jj)^2 over the M real rows -- a lower bound of cond_2(K_ZZ + jitter I) that costs a
// few hundred loads per fit.  Fits whose sigma^2 no float64 implementation reproduces to 1e-4 are exactly
// the ones where this figure is large; the caller gets it next to the status instead of finding out from an oracle.
__global__ __launch_bounds__(256) void k_fit_cond(int n_fits, int D, const gapro_fit_desc* __restrict__ descs,
                                                  const double* __restrict__ ws, double* __restrict__ out) {
  const int fit = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (fit >= n_fits) return;
  const gapro_fit_desc d = descs[fit];
  const int M = d.m1 + d.m2;
  const Layout lay = make_layout(M, d.t, D);
  const double* dinv = ws + d.ws_offset + lay.dinv;
  double rmin = 1e300, rmax = 0.0;
  for (int j = lane; j < M; j += 64) {
    const double r = fabs(dinv[(size_t)(j >> 4) * 256 + 17 * (j & 15)]);
    rmin = fmin(rmin, r);
    rmax = fmax(rmax, r);
  }
  for (int o = 32; o > 0; o >>= 1) {
    rmin = fmin(rmin, __shfl_xor(rmin, o, 64));
    rmax = fmax(rmax, __shfl_xor(rmax, o, 64));
  }
  if (lane == 0) {
    const double q = rmax / rmin;  // = max L_jj / min L_jj
    out[d.slot] = q * q;
  }
}

// Trained model of every fit of a launch (gapro_svgp_fit_batch_state), gathered behind the fit kernels like the figures
// above.  Every route leaves its final parameters at the same places of the fit's slab: Z [M_p][D] behind X (the strip
// and staged kernels update it together with their LDS copy, fit_wg.h), the mean in V_M, tril(L_S) row-major in B_LS
// (float32 in the first half of the slot where the cluster kernel ran the fit in GAPRO_PRECISION_MIXED), c, rho_s,
// rho_l and the status in the scalar tail; the wave-per-fit kernel writes them there on its way out when asked.  One
// workgroup per fit copies the M real rows into the route-independent state layout of include/gapro_hip.h.
// [f32_lo, f32_hi): the launch's cluster fits when their L_S is float32.
__global__ __launch_bounds__(256) void k_gp_state_export(int D, const gapro_fit_desc* __restrict__ descs,
                                                         const double* __restrict__ ws, double* __restrict__ state,
                                                         const long long* __restrict__ state_off, double jitter,
                                                         int f32_lo, int f32_hi) {
  const gapro_fit_desc d = descs[blockIdx.x];
  const int M = d.m1 + d.m2;
  const Layout lay = make_layout(M, d.t, D);
  const double* base = ws + d.ws_offset;
  double* out = state + state_off[d.slot];
  const int tid = threadIdx.x;
  if (tid == 0) {
    const double* scal = base + lay.scal;
    out[SH_M] = (double)M;
    out[SH_D] = (double)D;
    out[SH_STATUS] = scal[S_STATUS];
    out[SH_JITTER] = jitter;
    out[SH_C] = scal[S_C];
    out[SH_RS] = scal[S_RS];
    out[SH_RL] = scal[S_RL];
    out[SH_RESERVED] = 0.0;
  }
  const double* Z = base + lay.xz + (long long)lay.Mp * D;
  double* oz = out + kStateHeader;
  for (int e = tid; e < M * D; e += 256) oz[e] = Z[e];
  const double* vm = base + lay.vec + (long long)V_M * lay.Mp;
  double* om = oz + (long long)M * D;
  for (int e = tid; e < M; e += 256) om[e] = vm[e];
  const double* LS = base + lay.mat + (long long)B_LS * lay.Mp * lay.Mp;
  const bool f32 = (int)blockIdx.x >= f32_lo && (int)blockIdx.x < f32_hi;
  double* ol = om + M;
  for (long long e = tid; e < (long long)M * M; e += 256) {
    const int i = (int)(e / M), j = (int)(e - (long long)i * M);
    const long long src = (long long)i * lay.Mp + j;
    ol[e] = j <= i ? (f32 ? (double)((const float*)LS)[src] : LS[src]) : 0.0;
  }
}

// 0 = strip-streaming kernel, 1 = LDS-staged kernel, 2 = generic kernel, 3 = strip-streaming kernel of the small-fit
// translation unit (M_p <= 64: 256 threads per fit, two fits per CU), 4 = cluster kernel (one fit over several
// workgroups), 5 = the wave-per-fit kernel (svgp_fit_wave.hip: M_p <= 48 at feat_dim 6).  flags:
// gapro_fit_options.reserved (GAPRO_FIT_DBG_*).
constexpr int kSmallFitMp = 64;
static int fit_route(int m, int feat_dim, int flags) {
  const int Mp = gapro_pad_m(m, feat_dim);
  if (!(flags & GAPRO_FIT_DBG_NO_WAVE) && Mp <= gapro_fit_wave_max_mp(feat_dim)) return 5;
  // large fits: spread over several CUs (svgp_fit_cluster.hip)
  const bool clus = !(flags & GAPRO_FIT_DBG_NO_CLUSTER) && feat_dim <= 32;
  if (clus && gapro_cluster_size(Mp, (flags & GAPRO_FIT_DBG_CLUSTER_ALL) != 0) > 0) return 4;
  if (!(flags & GAPRO_FIT_DBG_NO_STRIP) && gapro_fit_strip_ok(m, feat_dim)) {
    const bool small = Mp <= kSmallFitMp && 2 * gapro_fit_strip_small_lds_bytes(m, feat_dim) + 16384 <= 160 * 1024;
    return (small && !(flags & GAPRO_FIT_DBG_NO_SMALL)) ? 3 : 0;
  }
  if (gapro_fit_staged_ok(m, feat_dim)) return 1;
  // neither LDS-resident kernel takes it (deep features: Z and X of M_p > 192 points at D = 32 do not fit beside the
  // Cholesky block column): the cluster kernel keeps the points in global memory and runs such a fit on one workgroup
  if (clus && gapro_cluster_size(Mp, true) > 0) return 4;
  return 2;
}

// The launch groups of gapro_svgp_fit_batch, in the order of the descriptor array it uploads.  Kernels are launched
// in another order: cluster, large, staged, strip, small, wave 3 / 2 / 1 (LABNOTES R4.4).
enum FitGroupId { G_LARGE, G_STAGED, G_STRIP, G_SMALL, G_CLUSTER, G_WAVE3, G_WAVE2, G_WAVE1, kFitGroups };
static int fit_group(int route, int m, int feat_dim) {  // (a wave fit's by its block count: M_p = 16 nb)
  static const int of_route[6] = {G_STRIP, G_STAGED, G_LARGE, G_SMALL, G_CLUSTER, G_WAVE1};
  return route == GAPRO_FIT_KERNEL_WAVE ? G_WAVE1 + 1 - gapro_pad_m(m, feat_dim) / 16 : of_route[route];
}
// kernel (GAPRO_FIT_KERNEL_*), fit stream (gapro_ctx::fit_stream), first counter of the launch's ticket set and timing
// class (gapro_fit_timing) of every group
static const struct { int kernel, stream, ticket, timing; } kFitGroupLaunch[kFitGroups] = {
    {2, 0, -1, 0},  // large: the generic kernel, ahead of the staged fits on their stream
    {1, 0, 0, 0},   // staged: tickets 0 .. 2 for its three launches; the third may go to fit stream 4 (below)
    {0, 1, 3, 1},   // strip
    {3, 2, 4, 2},   // small
    {4, 3, 5, 3},   // cluster: tickets 5 .. 7 are its diagnostics (gapro_fit_timing_cluster_info)
    {5, 5, 10, 4},  // wave, M_p = 48
    {5, 6, 9, 4},   // wave, M_p = 32
    {5, 7, 8, 4},   // wave, M_p = 16
};
constexpr int kStaged2 = 4;  // fit stream and join event of the two-per-CU staged launch beside the others

// Everything gapro_svgp_fit_batch decides from the sizes of its fits and its debug flags, before it touches the device:
// plan_fit_launch is a pure function (gapro_fit_launch_plan hands it out; tests/test_fit_plan_cpu.py holds it to the
// decisions of rounds 4 to 6 that the comments below record).
struct FitLaunchPlan {
  std::vector<gapro_fit_desc> descs;        // in upload order: the groups of FitGroupId, each longest first
  long long ws_bytes = 0;                   // workspace the fits' ws_offset need
  std::vector<int> cl_index, cl_mp, cl_g;   // cluster fits: place in descs, padded size, workgroups per cluster
  FitLaunchStep steps[GAPRO_FIT_MAX_STEPS]; // in the order of issue
  int n_steps = 0;
  int bad_fit = -1;                         // first fit with an empty side (nothing else is valid then)
  int slow_m = 0;                           // M of the first fit beyond the cluster kernel's cap, on the generic kernel
};

static FitLaunchPlan plan_fit_launch(const gapro_fit_desc* h_descs, int n_fits, int feat_dim, int flags, int n_cu) {
  FitLaunchPlan p;
  // Routing (gapro_fit_route).  Every group is sorted longest processing time first (cost ~ M^3): workgroups are
  // dispatched in block order, so the expensive fits start first and the tail of a launch stays short.  One sort by
  // (group, M descending, input index) does it.
  struct Key { int group, m, i; };
  std::vector<Key> keys(n_fits);
  size_t count[kFitGroups] = {}, base[kFitGroups];
  for (int i = 0; i < n_fits; ++i) {
    const gapro_fit_desc& d = h_descs[i];
    const int m = d.m1 + d.m2;
    if (d.m1 <= 0 || d.m2 <= 0 || d.t < 0) {
      p.bad_fit = i;
      return p;
    }
    p.ws_bytes = std::max<long long>(p.ws_bytes, (d.ws_offset + gapro_fit_workspace_doubles(m, d.t, feat_dim)) * 8LL);
    const int g = fit_group(fit_route(m, feat_dim, flags), m, feat_dim);
    keys[i] = {g, m, i};
    ++count[g];
    // beyond the cluster kernel's cap (kClusterMaxMp: its merge inverse keeps one LDS record per pair of panels) a
    // fit runs on ONE workgroup of the generic kernel: correct, but minutes per fit -- never silently
    if (g == G_LARGE && feat_dim <= 32 && gapro_pad_m(m, feat_dim) > kClusterMaxMp && !p.slow_m) p.slow_m = m;
  }
  std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
    return a.group != b.group ? a.group < b.group : a.m != b.m ? a.m > b.m : a.i < b.i;
  });
  p.descs.resize(n_fits);
  for (int k = 0; k < n_fits; ++k) {
    p.descs[k] = h_descs[keys[k].i];
    p.descs[k].slot = keys[k].i;
  }
  for (int g = 0; g < kFitGroups; ++g) base[g] = g ? base[g - 1] + count[g - 1] : 0;
  const gapro_fit_desc* staged = p.descs.data() + base[G_STAGED];
  // the staged fits whose LDS fits a CU twice and the larger ones are two launches (see below)
  const long long kTwice = 72 * 1024;
  size_t nbig = 0, nkmaj = 0;  // sorted by M, the LDS need grows with M: [0, nkmaj) M_p > kKminMaxMp, [0, nbig) "big"
  long long lds_big = 0, lds_rest = 0, lds_kmaj = 0;
  for (size_t k = 0; k < count[G_STAGED]; ++k) {
    const int m = staged[k].m1 + staged[k].m2;
    const long long b = gapro_fit_staged_lds_bytes(m, feat_dim);
    // (the product forms of a fit are a function of its M_p, k_svgp_fit's KMIN: fits beyond kKminMaxMp are a launch of
    // their own -- with D = 6 exactly the fits that need more than kTwice)
    const bool kmaj = gapro_pad_m(m, feat_dim) > kKminMaxMp;
    if (kmaj) {
      ++nkmaj;
      lds_kmaj = std::max(lds_kmaj, b);
    }
    if (kmaj || b > kTwice) {
      ++nbig;
      if (!kmaj) lds_big = std::max(lds_big, b);
    } else {
      lds_rest = std::max(lds_rest, b);
    }
  }
  // Default since round 4: ticket counters (claim_fit) -- the fits stay in plain longest-first order and are taken by
  // the workgroups in the order in which they start; GAPRO_FIT_DBG_STATIC_MAP restores the mapping fit = blockIdx.x
  const bool tickets = !(flags & GAPRO_FIT_DBG_STATIC_MAP);
  if (!tickets) {
    // Workgroup b of a launch runs on XCD b % 8 (one slice of 32 CUs; the cluster kernel's same-XCD barrier relies on
    // the same fact and checks it), so in longest-first order XCD 0 would get the largest fit of every group of eight
    // and XCD 7 the smallest, in every kernel: at the end of a launch four XCDs sat idle for ~50 ms while the others
    // still had their share of strip fits (tools/fit_timeline.py).  Every second group of eight is reversed.
    auto serpentine = [&](size_t lo, size_t hi) {
      for (size_t g0 = lo + 8; g0 + 8 <= hi; g0 += 16) std::reverse(p.descs.begin() + g0, p.descs.begin() + g0 + 8);
    };
    serpentine(base[G_STRIP], base[G_STRIP] + count[G_STRIP]);
    serpentine(base[G_SMALL], base[G_SMALL] + count[G_SMALL]);
    serpentine(base[G_STAGED], base[G_STAGED] + nbig);
    serpentine(base[G_STAGED] + nbig, base[G_STAGED] + count[G_STAGED]);
  }
  p.cl_index.resize(count[G_CLUSTER]);
  p.cl_mp.resize(count[G_CLUSTER]);
  p.cl_g.resize(count[G_CLUSTER]);
  for (size_t k = 0; k < count[G_CLUSTER]; ++k) {
    const gapro_fit_desc& d = p.descs[base[G_CLUSTER] + k];
    p.cl_index[k] = (int)(base[G_CLUSTER] + k);
    p.cl_mp[k] = gapro_pad_m(d.m1 + d.m2, feat_dim);
    p.cl_g[k] = gapro_cluster_size(p.cl_mp[k], true);
  }
  // The kernels go to the context's fit streams so that the staged kernel (a few large fits, which leave most CUs
  // idle), the strip kernels and the others run side by side; GAPRO_FIT_DBG_CALLER_STREAM keeps them on the caller's
  const bool own = !(flags & GAPRO_FIT_DBG_CALLER_STREAM);
  // a step of group g: fits [first, first + n) of the group, counter `part` of the group's
  auto step = [&](int g, size_t first, size_t n, int variant, size_t grid, long long lds,
                  int part = 0) -> FitLaunchStep& {
    const auto& L = kFitGroupLaunch[g];
    FitLaunchStep& s = p.steps[p.n_steps++];
    s = FitLaunchStep{L.kernel, variant, (int)(base[g] + first), (int)n, (int)grid, own ? L.stream : -1,
                      tickets && L.ticket >= 0 ? L.ticket + part : -1, L.timing, 0, 0, lds};
    return s;
  };
  // grid of a ticketed kernel: twice its fits, so that an XCD (a fixed eighth of the grid) can run up to twice its share
  auto grid_of = [&](size_t n) { return tickets ? 2 * n : n; };
  auto max_lds = [&](int g, long long (*bytes)(int, int)) {  // largest dynamic LDS need of a fit of the group
    long long b = 0;
    for (size_t k = 0; k < count[g]; ++k)
      b = std::max(b, bytes(p.descs[base[g] + k].m1 + p.descs[base[g] + k].m2, feat_dim));
    return b;
  };
  // First the largest fits of the launch, each over several CUs.
  // (Round 4, tried: holding the other kernels back until the cluster's members are resident.  They are within 1 .. 15
  // us anyway, and every cluster sits on one XCD (gapro_fit_timing_cluster_info); what makes the same cluster kernel
  // take 240 ms in one run of a step and 500 ms in the next is what runs beside it -- LABNOTES R4.4.)
  if (count[G_CLUSTER]) step(G_CLUSTER, 0, count[G_CLUSTER], 0, 0, 0);
  // gate of the two-per-CU staged launch and of the small fits (below): behind the cluster kernel
  const bool gate = count[G_CLUSTER] && own;
  if (count[G_LARGE]) step(G_LARGE, 0, count[G_LARGE], 0, count[G_LARGE], 0);
  // The dynamic LDS of a launch is its largest fit's, and beyond ~72 KiB (M_p > 256 at D = 6) a CU holds ONE
  // workgroup whatever the registers allow: a launch with one such fit ran every staged fit one per CU.  So the
  // staged fits go out as two launches side by side: those whose LDS fits a CU twice in the `<4>` build (128 VGPRs,
  // two workgroups per CU: 17 % more fits/s at M <= 256 than one per CU), the larger ones in the `<2>` build (the
  // whole register file, no spills).  Either part with fewer fits than CUs takes `<2>` as well.
  auto staged_step = [&](size_t first, size_t n, long long lds, bool kmaj, int part) -> FitLaunchStep& {
    const bool one_per_cu = (int)n <= n_cu || lds > kTwice;
    return step(G_STAGED, first, n, kmaj ? 2 : (one_per_cu ? 2 : kWavesPerSimd) | GAPRO_FIT_STEP_COPY_FREE, grid_of(n),
                lds, part);
  };
  if (nkmaj > 0) staged_step(0, nkmaj, lds_kmaj, true, 0);
  // M_p <= kKminMaxMp with an LDS need beyond kTwice (wide features): behind the former
  if (nbig > nkmaj) staged_step(nkmaj, nbig - nkmaj, lds_big, false, 1);
  if (nbig < count[G_STAGED]) {
    FitLaunchStep& s = staged_step(nbig, count[G_STAGED] - nbig, lds_rest, false, 2);
    if (nbig > 0 && own) s.stream = kStaged2;  // beside the larger ones
    // The two-per-CU staged fits are the launch's memory-bound class (3.8 FLOP/B: with the chip to themselves they
    // sit on the HBM roof), the cluster fits its latency-bound one (a chain of cluster barriers and small products
    // per Adam step).  Side by side from the start, the same cluster kernel took 230 .. 270 ms or 500 .. 800 ms
    // depending on which kernels the runtime happened to put on one hardware queue (LABNOTES R4.4); so the order is
    // explicit: this launch starts when the cluster kernel has ended -- small and strip fits, light on memory, take
    // the CUs beside the clusters meanwhile.  Same box, 2 x 8 steps: 361 .. 372 scenes/s with 4 or 8 hardware queues
    // (GPU_MAX_HW_QUEUES), the cluster kernel at its undisturbed time in every step; without the gate 368 / 372 with
    // the default 4 queues (the lucky mapping) and 351 .. 362 with 8.
    s.wait_gate = gate;
  }
  if (count[G_STRIP])
    step(G_STRIP, 0, count[G_STRIP], 0, grid_of(count[G_STRIP]), max_lds(G_STRIP, gapro_fit_strip_lds_bytes));
  // the small fits start behind the cluster kernel as well: beside the clusters run the whole-CU strip fits and the
  // one-per-CU staged fits, and every CU half the two-per-CU staged fits leave later goes to a small fit, light on
  // memory, instead of a second memory-bound one -- 367.8 / 367.4 / 362.6 scenes/s against 364.0 / 363.2 / 356.1
  // without this gate, alternating on one box
  if (count[G_SMALL])
    step(G_SMALL, 0, count[G_SMALL], 0, grid_of(count[G_SMALL]), max_lds(G_SMALL, gapro_fit_strip_small_lds_bytes))
        .wait_gate = gate;
  // One wave per fit (svgp_fit_wave.hip), one kernel per block count, side by side on their own streams; the waves of a
  // kernel take its fits by ticket until none is left.  They touch no memory between their first and last step, so
  // nothing holds them back: they take whatever wave slots and LDS the other kernels leave.
  for (int g = G_WAVE3; g <= G_WAVE1; ++g) {
    if (!count[g]) continue;
    const int nb = G_WAVE1 + 1 - g;
    const int slots = n_cu * gapro_fit_wave_per_cu(nb, feat_dim);
    step(g, 0, count[g], nb, std::min<size_t>(count[g], (size_t)std::max(slots, 1)), 0);
  }
  return p;
}

// Grows the context's buffers to the launch: the state offsets by fit slot (n_state fits: 0 without a state export) and
// the cluster kernel's staging (n_clus fits): block table and one barrier counter line per fit, two halves of each.
static int grow_fit_buffers(gapro_ctx* ctx, size_t n_state, size_t n_clus) {
  if (n_state > ctx->state_off_cap) {
    if (ctx->d_state_off) (void)hipFree(ctx->d_state_off);
    ctx->d_state_off = nullptr;
    ctx->state_off_cap = 0;
    const size_t cap = std::max<size_t>(1024, 2 * n_state);
    GAPRO_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_state_off, cap * sizeof(long long)));
    ctx->state_off_cap = cap;
  }
  const size_t need_stage = n_clus ? gapro_cluster_stage_bytes((int)n_clus) : 0;
  if (2 * need_stage > ctx->cl_stage_bytes) {  // cl_stage_bytes counts BOTH halves; a launch uses one of them
    if (ctx->h_cl_stage) (void)hipHostFree(ctx->h_cl_stage);
    if (ctx->d_cl_stage) (void)hipFree(ctx->d_cl_stage);
    ctx->h_cl_stage = ctx->d_cl_stage = nullptr;
    ctx->cl_stage_bytes = 0;
    GAPRO_HIP_CHECK(ctx, hipHostMalloc(&ctx->h_cl_stage, 2 * need_stage, hipHostMallocDefault));
    GAPRO_HIP_CHECK(ctx, hipMalloc(&ctx->d_cl_stage, 2 * need_stage));
    ctx->cl_stage_bytes = 2 * need_stage;
  }
  if (n_clus > ctx->cl_ctl_fits) {
    if (ctx->d_cl_ctl) (void)hipFree(ctx->d_cl_ctl);
    ctx->d_cl_ctl = nullptr;
    ctx->cl_ctl_fits = 0;
    GAPRO_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_cl_ctl, 2 * 2 * n_clus * 128));  // two halves
    ctx->cl_ctl_fits = 2 * n_clus;
  }
  return GAPRO_OK;
}

// launch function and name of a step's kernel, by GAPRO_FIT_KERNEL_* (the cluster kernel's takes its staging as well)
static const struct { int (*launch)(hipStream_t, const FitLaunchStep&, const FitArgs&); const char* name; } kFitKernel[6] = {
    {gapro_launch_fit_strip, "strip"}, {gapro_launch_fit_staged, "staged"},   {gapro_launch_fit_large, "generic"},
    {gapro_launch_fit_strip_small, "small-fit"}, {nullptr, "cluster"}, {gapro_launch_fit_wave, "wave"}};

extern "C" {

int64_t gapro_fit_workspace_doubles(int32_t m, int32_t t, int32_t feat_dim) {
  if (m <= 0 || t < 0 || feat_dim <= 0) return 0;
  return make_layout(m, t, feat_dim).total;
}

int64_t gapro_fit_plan_workspace(gapro_fit_desc* h_descs, int32_t n_fits, int32_t feat_dim) {
  if (!h_descs || n_fits < 0) return 0;
  int64_t off = 0;
  for (int i = 0; i < n_fits; ++i) {
    h_descs[i].ws_offset = off;
    off += gapro_fit_workspace_doubles(h_descs[i].m1 + h_descs[i].m2, h_descs[i].t, feat_dim);
  }
  return off * (int64_t)sizeof(double);
}

int gapro_fit_workspace_layout(int32_t m, int32_t t, int32_t feat_dim, int64_t* out8) {
  if (!out8 || m <= 0 || feat_dim <= 0) return GAPRO_ERR_BAD_ARG;
  const Layout L = make_layout(m, t, feat_dim);
  out8[0] = L.Mp; out8[1] = L.mat; out8[2] = L.vec; out8[3] = L.xz; out8[4] = L.xt; out8[5] = L.dinv;
  out8[6] = L.scal; out8[7] = L.total;
  return GAPRO_OK;
}

int gapro_svgp_fit_batch(gapro_ctx* ctx, void* stream_, int32_t n_fits, int32_t feat_dim, const float* d_feats_spp,
                         const int32_t* d_idx, const gapro_fit_desc* h_descs, gapro_fit_desc* d_descs,
                         const double* d_init_mean, const gapro_fit_options* opt, double* d_workspace,
                         size_t workspace_bytes, float* d_probs, float* d_probs_new, uint8_t* d_labels, float* d_mu,
                         float* d_var, int32_t* d_fit_status, double* d_fit_loss) {
  return gapro_svgp_fit_batch_ex(ctx, stream_, n_fits, feat_dim, d_feats_spp, d_idx, h_descs, d_descs, d_init_mean, opt,
                                 d_workspace, workspace_bytes, d_probs, d_probs_new, d_labels, d_mu, d_var, d_fit_status,
                                 d_fit_loss, nullptr);
}

int64_t gapro_gp_state_doubles(int32_t m, int32_t feat_dim) {
  if (m <= 0 || feat_dim <= 0) return 0;
  return state_doubles(m, feat_dim);
}

int64_t gapro_gp_state_plan(const gapro_fit_desc* h_descs, int32_t n_fits, int32_t feat_dim, int64_t* h_state_offsets) {
  if (!h_descs || !h_state_offsets || n_fits < 0) return 0;
  int64_t off = 0;
  for (int i = 0; i < n_fits; ++i) {
    h_state_offsets[i] = off;
    off += gapro_gp_state_doubles(h_descs[i].m1 + h_descs[i].m2, feat_dim);
  }
  return off * (int64_t)sizeof(double);
}

int gapro_svgp_fit_batch_ex(gapro_ctx* ctx, void* stream_, int32_t n_fits, int32_t feat_dim, const float* d_feats_spp,
                            const int32_t* d_idx, const gapro_fit_desc* h_descs, gapro_fit_desc* d_descs,
                            const double* d_init_mean, const gapro_fit_options* opt, double* d_workspace,
                            size_t workspace_bytes, float* d_probs, float* d_probs_new, uint8_t* d_labels, float* d_mu,
                            float* d_var, int32_t* d_fit_status, double* d_fit_loss, double* d_fit_cond) {
  return gapro_svgp_fit_batch_state(ctx, stream_, n_fits, feat_dim, d_feats_spp, d_idx, h_descs, d_descs, d_init_mean,
                                    opt, d_workspace, workspace_bytes, d_probs, d_probs_new, d_labels, d_mu, d_var,
                                    d_fit_status, d_fit_loss, d_fit_cond, nullptr, nullptr, 0);
}

int gapro_svgp_fit_batch_state(gapro_ctx* ctx, void* stream_, int32_t n_fits, int32_t feat_dim,
                               const float* d_feats_spp, const int32_t* d_idx, const gapro_fit_desc* h_descs,
                               gapro_fit_desc* d_descs, const double* d_init_mean, const gapro_fit_options* opt,
                               double* d_workspace, size_t workspace_bytes, float* d_probs, float* d_probs_new,
                               uint8_t* d_labels, float* d_mu, float* d_var, int32_t* d_fit_status, double* d_fit_loss,
                               double* d_fit_cond, double* d_state, const int64_t* h_state_offsets, size_t state_bytes) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_fits == 0) return GAPRO_OK;
  if (n_fits < 0 || feat_dim <= 0 || !d_feats_spp || !d_idx || !h_descs || !d_descs || !opt || !d_workspace ||
      !d_probs || !d_probs_new || !d_labels || !d_mu || !d_var || !d_fit_status || !d_fit_loss || workspace_bytes == 0)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_fit_batch: bad argument");
  if (opt->training_iter < 0 || !(opt->lr > 0.0) || !(opt->jitter >= 0.0) || opt->psd_retries < 0 ||
      opt->psd_retries > 8 || !(opt->psd_jitter >= 0.0))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_fit_batch: bad options");
  // (a NaN would switch the clamp off without a word: `vraw < NaN` is false in every kernel)
  if (!(opt->min_variance >= 0.0 && opt->min_variance < INFINITY))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_fit_batch: min_variance %g is negative or not finite",
                      opt->min_variance);
  const int route_flags = opt->reserved;
  if (route_flags & ~GAPRO_FIT_DBG_ALL)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_fit_batch: unknown or retired debug bits 0x%x in reserved",
                      (unsigned)(route_flags & ~GAPRO_FIT_DBG_ALL));
  hipStream_t stream = (hipStream_t)stream_;
  const FitLaunchPlan plan = plan_fit_launch(h_descs, n_fits, feat_dim, route_flags, ctx->n_cu);
  if (plan.bad_fit >= 0)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_fit_batch: fit %d has an empty side", plan.bad_fit);
  if (plan.slow_m) {
    static bool warned = false;
    if (!warned) {
      warned = true;
      fprintf(stderr, "libgapro_hip: a GP fit with M = %d inducing points exceeds the multi-workgroup kernel's cap "
                      "(M_p <= %d): it runs on one workgroup of the generic kernel (minutes per fit)\n", plan.slow_m,
              gapro_fit::kClusterMaxMp);
    }
  }
  if ((size_t)plan.ws_bytes > workspace_bytes)
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_svgp_fit_batch: workspace too small (%lld > %zu)", plan.ws_bytes,
                      workspace_bytes);
  if (d_state) {  // every fit's state inside the caller's buffer; the offsets go up with the descriptors (below)
    if (!h_state_offsets) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_svgp_fit_batch_state: no state offsets");
    for (int i = 0; i < n_fits; ++i) {
      const long long end = h_state_offsets[i] + state_doubles(h_descs[i].m1 + h_descs[i].m2, feat_dim);
      if (h_state_offsets[i] < 0 || (unsigned long long)end * 8ULL > state_bytes)
        return gapro_fail(ctx, GAPRO_ERR_WORKSPACE,
                          "gapro_svgp_fit_batch_state: state of fit %d ends at %lld bytes of %zu", i, end * 8LL, state_bytes);
    }
  }
  const size_t n_clus = plan.cl_index.size();
  if (const int rc = grow_fit_buffers(ctx, d_state ? (size_t)n_fits : 0, n_clus)) return rc;
  // ticket counters of this launch (FitLaunchStep::ticket; kTicketsPerSet of them).  The sets rotate, so that a set is
  // zeroed again only kTicketSets launches later
  unsigned* tk = nullptr;
  if (!(route_flags & GAPRO_FIT_DBG_STATIC_MAP)) {
    tk = ctx->d_tickets + (size_t)(ctx->ticket_seq++ % gapro_ctx::kTicketSets) * gapro_ctx::kTicketsPerSet;
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(tk, 0, gapro_ctx::kTicketsPerSet * sizeof(unsigned), stream));
  }
  // cluster kernel: block table and barrier counters go up on `stream` too, so that after the synchronisation below the
  // kernel is the first thing its stream has to do
  int cl_blocks = 0, cl_members = 0, cl_par = 0;
  char* cl_d_half = nullptr;
  unsigned* cl_ctl_half = nullptr;
  if (n_clus) {
    // the block table is built in one half of the context's pinned buffer, the halves alternating per launch: the
    // copy of launch i - 2 has long been consumed (callers collect a launch before they issue the one after next),
    // so the host never waits for the previous cluster kernel here
    // (the device copies alternate the same way, so that two launches issued from different streams --
    // GAPRO_FIT_DBG_CALLER_STREAM puts the kernels on the caller's stream -- never share a block table or a barrier
    // counter)
    const size_t par = ctx->cl_parity & 1;
    cl_par = (int)par;
    // this half's previous user may still be running on another stream (overlapping launches, several caller streams):
    // the upload and the counter reset below wait for it
    if (ctx->clus_half_used[par]) GAPRO_HIP_CHECK(ctx, hipStreamWaitEvent(stream, ctx->ev_clus_half[par], 0));
    char* h_half = (char*)ctx->h_cl_stage + par * (ctx->cl_stage_bytes / 2);
    cl_d_half = (char*)ctx->d_cl_stage + par * (ctx->cl_stage_bytes / 2);
    cl_ctl_half = ctx->d_cl_ctl + par * ctx->cl_ctl_fits * 32;
    ctx->cl_parity++;
    const int rc = gapro_prepare_fit_cluster(stream, (int)n_clus, plan.cl_index.data(), plan.cl_mp.data(),
                                             plan.cl_g.data(), h_half, cl_d_half, cl_ctl_half, &cl_blocks, &cl_members);
    if (rc != GAPRO_OK) return gapro_fail(ctx, rc, "gapro_svgp_fit_batch: cluster block table upload failed");
  }
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_descs, plan.descs.data(), plan.descs.size() * sizeof(gapro_fit_desc),
                                      hipMemcpyHostToDevice, stream));
  if (d_state)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_state_off, h_state_offsets, (size_t)n_fits * sizeof(long long),
                                        hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipStreamSynchronize(stream));  // plan.descs is pageable host memory that dies with this call
  // No fork event is needed for the fit streams: `stream` has just been synchronised, so everything the kernels read is
  // complete (and an event recorded here completes together with the NEXT dispatch of `stream` under this runtime,
  // which would serialise the kernels again).  All are joined back into `stream` with events.
  // A timing class (FitLaunchStep::timing) is the steps that share a pair of timing marks: its stream is its first
  // step's, [first, last] are its steps in the order of issue.
  constexpr int NK = gapro_fit_timing::kKernels;
  int first[NK], last[NK];
  for (int c = 0; c < NK; ++c) first[c] = last[c] = -1;
  for (int k = 0; k < plan.n_steps; ++k) {
    const int c = plan.steps[k].timing;
    if (first[c] < 0) first[c] = k;
    last[c] = k;
  }
  gapro_fit_timing* tm = ctx->armed_timing;
  ctx->armed_timing = nullptr;
  if (tm) {
    tm->tickets = tk;
    for (int c = 0; c < NK; ++c) tm->used[c] = first[c] >= 0;
  }
  auto on = [&](const FitLaunchStep& s) { return s.stream >= 0 ? ctx->fit_stream[s.stream] : stream; };
  auto mark = [&](const FitLaunchStep& s, int end) {  // timing event of the step's class on its stream: start, end
    return tm ? hipEventRecord(tm->ev[2 * s.timing + end], on(s)) : hipSuccess;
  };
  // the event that joins a step's stream into another: ev_join[stream]; a wave stream's is ev_join[4 + nb]
  auto join = [&](const FitLaunchStep& s, hipStream_t into) {
    hipEvent_t ev = ctx->ev_join[s.kernel == GAPRO_FIT_KERNEL_WAVE ? 4 + s.variant : s.stream];
    const hipError_t e = hipEventRecord(ev, on(s));
    return e != hipSuccess ? e : hipStreamWaitEvent(into, ev, 0);
  };
  gapro_fit_options wave_opt = *opt;  // the wave kernel keeps its model on chip: it writes it out only when asked
  if (d_state) wave_opt.reserved |= kFitOptKeepState;
  const FitArgs args = {feat_dim, d_feats_spp, d_idx, d_descs, d_init_mean, opt, d_workspace, d_probs, d_probs_new,
                        d_labels, d_mu, d_var, d_fit_status, d_fit_loss, tk};
  FitArgs wave_args = args;
  wave_args.opt = &wave_opt;
  for (int k = 0; k < plan.n_steps; ++k) {
    FitLaunchStep s = plan.steps[k];
    const FitLaunchStep& cls = plan.steps[first[s.timing]];
    // the small fits' span starts behind the gate; the staged class's mark is in front of its gated launch
    const bool opens = first[s.timing] == k, mark_behind_gate = s.kernel == GAPRO_FIT_KERNEL_SMALL;
    if (opens && !mark_behind_gate) GAPRO_HIP_CHECK(ctx, mark(cls, 0));
    if (s.wait_gate) GAPRO_HIP_CHECK(ctx, hipStreamWaitEvent(on(s), ctx->ev_gate, 0));
    if (opens && mark_behind_gate) GAPRO_HIP_CHECK(ctx, mark(cls, 0));
    const bool cluster = s.kernel == GAPRO_FIT_KERNEL_CLUSTER;
    if (cluster) s.grid = cl_blocks;
    const int rc = cluster ? gapro_launch_fit_cluster(on(s), s, args, cl_d_half, cl_ctl_half)
                           : kFitKernel[s.kernel].launch(on(s), s, s.kernel == GAPRO_FIT_KERNEL_WAVE ? wave_args : args);
    if (rc != GAPRO_OK)
      return gapro_fail(ctx, rc, "gapro_svgp_fit_batch: %s kernel launch failed", kFitKernel[s.kernel].name);
    // a step beside its class's stream (the two-per-CU staged launch on stream 4, the later wave kernels): the class
    // is finished once its stream has passed this point
    if (s.stream != cls.stream) GAPRO_HIP_CHECK(ctx, join(s, on(cls)));
    if (last[s.timing] == k) GAPRO_HIP_CHECK(ctx, mark(cls, 1));
    if (cluster) {
      GAPRO_HIP_CHECK(ctx, hipEventRecord(ctx->ev_clus_half[cl_par], on(s)));
      ctx->clus_half_used[cl_par] = true;
      // gate of the two-per-CU staged launch and of the small fits: behind the cluster kernel
      if (s.stream >= 0) GAPRO_HIP_CHECK(ctx, hipEventRecord(ctx->ev_gate, on(s)));
    }
  }
  // every class's stream joins the caller's once: the wave kernels' first (their stream has collected the others)
  for (int c : {4, 0, 1, 2, 3})
    if (first[c] >= 0 && plan.steps[first[c]].stream >= 0) GAPRO_HIP_CHECK(ctx, join(plan.steps[first[c]], stream));
  // conditioning figures, behind every kernel of the launch (they have been joined into `stream` above)
  if (d_fit_cond)
    hipLaunchKernelGGL(k_fit_cond, dim3((n_fits + 3) / 4), dim3(256), 0, stream, (int)n_fits, (int)feat_dim, d_descs,
                       d_workspace, d_fit_cond);
  if (d_state) {
    const bool f32 = opt->precision == GAPRO_PRECISION_MIXED && n_clus;
    const int lo = f32 ? plan.cl_index[0] : 0, hi = f32 ? lo + (int)n_clus : 0;
    hipLaunchKernelGGL(k_gp_state_export, dim3(n_fits), dim3(256), 0, stream, (int)feat_dim, d_descs, d_workspace,
                       d_state, ctx->d_state_off, opt->jitter, lo, hi);
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_fit_route(int32_t m, int32_t feat_dim) { return fit_route(m, feat_dim, 0); }

int gapro_fit_route_flags(int32_t m, int32_t feat_dim, int32_t flags) {
  return (flags & ~GAPRO_FIT_DBG_ALL) ? (int)GAPRO_ERR_BAD_ARG : fit_route(m, feat_dim, flags);
}

int gapro_fit_launch_plan(const gapro_fit_desc* h_descs, int32_t n_fits, int32_t feat_dim, int32_t flags, int32_t n_cu,
                          gapro_fit_launch_step* steps_out, int32_t max_steps, int32_t* n_steps_out,
                          int32_t* order_out) {
  if (!h_descs || !steps_out || !n_steps_out || !order_out || n_fits <= 0 || feat_dim <= 0 || n_cu <= 0 ||
      (flags & ~GAPRO_FIT_DBG_ALL))
    return GAPRO_ERR_BAD_ARG;
  const FitLaunchPlan plan = plan_fit_launch(h_descs, n_fits, feat_dim, flags, n_cu);
  if (plan.bad_fit >= 0 || plan.n_steps > max_steps) return GAPRO_ERR_BAD_ARG;
  std::copy(plan.steps, plan.steps + plan.n_steps, steps_out);
  *n_steps_out = plan.n_steps;
  for (int k = 0; k < n_fits; ++k) order_out[k] = plan.descs[k].slot;
  return GAPRO_OK;
}

int gapro_fit_padded_m(int32_t m, int32_t feat_dim) { return gapro_pad_m(m, feat_dim); }

int gapro_fit_timing_create(gapro_ctx* ctx, gapro_fit_timing** out) {
  if (!ctx || !out) return GAPRO_ERR_BAD_ARG;
  gapro_fit_timing* t = new (std::nothrow) gapro_fit_timing();
  if (!t) return GAPRO_ERR_OOM;
  for (int i = 0; i < 2 * gapro_fit_timing::kKernels; ++i)
    if (hipEventCreate(&t->ev[i]) != hipSuccess) {
      gapro_fit_timing_destroy(t);
      return gapro_fail(ctx, GAPRO_ERR_HIP, "gapro_fit_timing_create: hipEventCreate failed");
    }
  *out = t;
  return GAPRO_OK;
}

void gapro_fit_timing_destroy(gapro_fit_timing* t) {
  if (!t) return;
  for (int i = 0; i < 2 * gapro_fit_timing::kKernels; ++i)
    if (t->ev[i]) (void)hipEventDestroy(t->ev[i]);
  delete t;
}

int gapro_fit_timing_arm(gapro_ctx* ctx, gapro_fit_timing* t) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  ctx->armed_timing = t;
  if (t) t->used[0] = t->used[1] = t->used[2] = t->used[3] = t->used[4] = false;
  return GAPRO_OK;
}

static int fit_timing_read(gapro_ctx* ctx, gapro_fit_timing* t, float* out_ms5, float* out_wave_ms) {
  constexpr int NK = gapro_fit_timing::kKernels;
  for (int i = 0; i < 5; ++i) out_ms5[i] = 0.f;
  if (out_wave_ms) *out_wave_ms = 0.f;
  const int slot[NK] = {0, 1, 3, 4, -1};  // staged, strip, small-fit strip, cluster, wave-per-fit
  float start[NK] = {0.f, 0.f, 0.f, 0.f, 0.f}, end[NK] = {0.f, 0.f, 0.f, 0.f, 0.f};
  int ref = -1;
  for (int k = 0; k < NK; ++k) {
    if (!t->used[k]) continue;
    float ms = 0.f;
    GAPRO_HIP_CHECK(ctx, hipEventSynchronize(t->ev[2 * k + 1]));
    GAPRO_HIP_CHECK(ctx, hipEventElapsedTime(&ms, t->ev[2 * k], t->ev[2 * k + 1]));
    if (slot[k] >= 0) out_ms5[slot[k]] = ms;
    else if (out_wave_ms) *out_wave_ms = ms;
    if (ref < 0) ref = k;
    float off = 0.f;  // start of kernel k relative to the first used kernel's start
    if (k != ref) GAPRO_HIP_CHECK(ctx, hipEventElapsedTime(&off, t->ev[2 * ref], t->ev[2 * k]));
    start[k] = off;
    end[k] = off + ms;
  }
  if (ref >= 0) {
    float lo = 0.f, hi = 0.f;
    for (int k = 0; k < NK; ++k)
      if (t->used[k]) {
        lo = start[k] < lo ? start[k] : lo;
        hi = end[k] > hi ? end[k] : hi;
      }
    out_ms5[2] = hi - lo;
  }
  return GAPRO_OK;
}

int gapro_fit_timing_read(gapro_ctx* ctx, gapro_fit_timing* t, float* out_ms5) {
  if (!ctx || !t || !out_ms5) return GAPRO_ERR_BAD_ARG;
  return fit_timing_read(ctx, t, out_ms5, nullptr);
}

int gapro_fit_timing_read_wave(gapro_ctx* ctx, gapro_fit_timing* t, float* out_ms) {
  if (!ctx || !t || !out_ms) return GAPRO_ERR_BAD_ARG;
  float ms5[5];
  return fit_timing_read(ctx, t, ms5, out_ms);
}

int gapro_fit_timing_cluster_info(gapro_ctx* ctx, gapro_fit_timing* t, int32_t* out3) {
  if (!ctx || !t || !out3) return GAPRO_ERR_BAD_ARG;
  out3[0] = out3[1] = out3[2] = 0;
  if (!t->tickets || !t->used[3]) return GAPRO_OK;
  GAPRO_HIP_CHECK(ctx, hipEventSynchronize(t->ev[7]));
  unsigned v[3] = {0, 0, 0};
  GAPRO_HIP_CHECK(ctx, hipMemcpy(v, t->tickets + 5, sizeof(v), hipMemcpyDeviceToHost));
  out3[0] = (int32_t)v[2];
  out3[1] = (int32_t)v[1];
  out3[2] = (int32_t)v[0];
  return GAPRO_OK;
}

int gapro_fit_timing_offsets(gapro_ctx* ctx, gapro_fit_timing* ref, gapro_fit_timing* t, float* out_ms2) {
  if (!ctx || !ref || !t || !out_ms2) return GAPRO_ERR_BAD_ARG;
  out_ms2[0] = out_ms2[1] = 0.f;
  int rk = -1;
  for (int k = 0; k < gapro_fit_timing::kKernels && rk < 0; ++k)
    if (ref->used[k]) rk = k;
  if (rk < 0) return GAPRO_OK;
  GAPRO_HIP_CHECK(ctx, hipEventSynchronize(ref->ev[2 * rk]));
  bool any = false;
  float lo = 0.f, hi = 0.f;
  for (int k = 0; k < gapro_fit_timing::kKernels; ++k) {
    if (!t->used[k]) continue;
    float a = 0.f, b = 0.f;
    GAPRO_HIP_CHECK(ctx, hipEventSynchronize(t->ev[2 * k + 1]));
    GAPRO_HIP_CHECK(ctx, hipEventElapsedTime(&a, ref->ev[2 * rk], t->ev[2 * k]));
    GAPRO_HIP_CHECK(ctx, hipEventElapsedTime(&b, ref->ev[2 * rk], t->ev[2 * k + 1]));
    lo = (!any || a < lo) ? a : lo;
    hi = (!any || b > hi) ? b : hi;
    any = true;
  }
  out_ms2[0] = lo;
  out_ms2[1] = hi;
  return GAPRO_OK;
}

}  // extern "C"
