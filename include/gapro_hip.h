/*
 * gapro_hip.h -- C ABI of libgapro_hip.so: the MI355X (gfx950) implementation of GaPro's
 * Gaussian-Process pseudo-label generator.
 *
 * The reference has no FFI for this path: it is plain Python on torch + gpytorch +
 * torch_scatter (paths relative to the reference checkout):
 *   gapro/gen_ps_utils.py:293-482            gen_pseudo_label_gaussian_process
 *   gapro/gaussian_process_utils.py:382-445  fit_gp_spp
 * Each entry point below names the reference lines it replaces.  A maintainer binds them
 * with ctypes (gapro_amd/_lib.py is that binding).
 *
 * Conventions
 *   - every function returns a gapro_status (0 = ok); nothing throws across the ABI;
 *     gapro_last_error(ctx) gives the message of the last failure on that context;
 *   - pointers named d_* are DEVICE pointers (hipMalloc'd or torch CUDA tensors), h_* are host
 *     pointers; the caller allocates every buffer, the library owns only gapro_ctx and
 *     gapro_schedule handles;
 *   - `stream` is a hipStream_t passed as void* (0 = null stream); device entry points only
 *     enqueue work unless documented "blocking";
 *   - one ctx per (process, device); a ctx is not thread-safe, distinct ctxs are.
 */
#ifndef GAPRO_HIP_H
#define GAPRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAPRO_VERSION 200 /* 0.2.0 */

typedef enum {
  GAPRO_OK = 0,
  GAPRO_ERR_BAD_ARG = -1,
  GAPRO_ERR_OOM = -2,
  GAPRO_ERR_HIP = -3,
  GAPRO_ERR_NOT_FINITE = -4,   /* a fit produced NaN/Inf */
  GAPRO_ERR_CHOLESKY = -5,     /* K_ZZ + jitter*I not positive definite */
  GAPRO_ERR_SPP_RANGE = -6,    /* superpoint id range exceeds the rank-table capacity */
  GAPRO_ERR_WORKSPACE = -7,    /* workspace too small */
  GAPRO_ERR_TIMEOUT = -8,      /* a fit spread over several workgroups gave up at a cluster barrier: a member was
                                * not resident within GAPRO_CLUSTER_BARRIER_TIMEOUT_MS (default 5000); per-fit
                                * status like GAPRO_ERR_CHOLESKY, the launch's other fits are unaffected.  The outputs
                                * (and the workspace) of a fit with this status are UNDEFINED: its members computed on
                                * unsynchronised data after the barrier gave up.  Transient by nature: callers retry the
                                * fit with the cluster kernel switched off (gapro_fit_options.reserved | 8), as
                                * gapro_amd.pipeline.Pipeline does */
  GAPRO_ERR_IO = -9,           /* gapro_pth_*: open / read / write failed, or a damaged file */
  GAPRO_ERR_UNSUPPORTED = -10  /* gapro_pth_*: a well-formed file this reader does not handle (compressed member,
                                * tensor storages, object / big-endian / Fortran arrays, ...): fall back to torch.load */
} gapro_status;

typedef struct gapro_ctx gapro_ctx;
typedef struct gapro_schedule gapro_schedule;

int gapro_version(void);
int gapro_ctx_create(int device, gapro_ctx** out);
void gapro_ctx_destroy(gapro_ctx* ctx);
const char* gapro_last_error(const gapro_ctx* ctx);

/* ------------------------------------------------------------------------------------------
 * Scene partition (device).  Replaces gen_ps_utils.py:312-326 and :347-363.
 * ---------------------------------------------------------------------------------------- */

/* Scene statistics, produced on the device by gapro_partition_prepare and copied to the host. */
typedef struct {
  double coord_min[3];   /* torch.min(coords_float, dim=0)        gen_ps_utils.py:317 */
  double coord_max[3];   /* torch.max(coords_float, dim=0)        gen_ps_utils.py:318 */
  int64_t spp_min;       /* smallest / largest superpoint id                          */
  int64_t spp_max;
  float feat_absmax;     /* max |mask_feats| (sets the fixed-point scale of the pooled sums) */
  int32_t fixed_shift;   /* pooled feature sums are exact int64 sums of rint(x * 2^fixed_shift) */
  int32_t n_spps;        /* len(torch.unique(spp))                gen_ps_utils.py:312-313 */
  int32_t status;        /* gapro_status raised on the device (e.g. GAPRO_ERR_SPP_RANGE) */
} gapro_scene_header;

/* Bytes of device workspace gapro_partition_prepare needs for `spp_range_cap` distinct id slots. */
size_t gapro_partition_prepare_workspace_bytes(int64_t n_points, int64_t spp_range_cap);

/* BLOCKING.  coords min/max, |feats| max, and the dense rank of every point's superpoint id
 * (the `return_inverse` output of torch.unique, gen_ps_utils.py:312).
 *   d_coords f64[N,3], d_feats f32[N,D], d_spp i64[N]  ->  d_spp_inv i32[N], *h_header        */
int gapro_partition_prepare(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t feat_dim,
                            const double* d_coords, const float* d_feats, const int64_t* d_spp,
                            int64_t spp_range_cap, void* d_workspace, size_t workspace_bytes,
                            int32_t* d_spp_inv, gapro_scene_header* h_header);

/* Same, enqueue only: the header lands in `h_header_pinned` (page-locked host memory) once the stream
 * reaches that point; the caller synchronises and checks header->status itself.  Lets a batch of
 * scenes share one synchronisation. */
int gapro_partition_prepare_async(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t feat_dim,
                                  const double* d_coords, const float* d_feats, const int64_t* d_spp,
                                  int64_t spp_range_cap, void* d_workspace, size_t workspace_bytes,
                                  int32_t* d_spp_inv, gapro_scene_header* h_header_pinned);

/* Fused point-in-box membership + superpoint pooling (gen_ps_utils.py:349-363) in one pass over
 * the points.  Box corners are the float64 `boxes` of gen_ps_utils.py:329-341 (float32-rounded
 * instance/wall corners held in float64, then the float64 floor box); the +-0.005 margin is
 * applied inside, in float64.
 *   in : d_coords f64[N,3], d_feats f32[N,D], d_spp_inv i32[N], d_boxes f64[B,6]
 *   tmp: d_feat_sum i64[S,D]  (zeroed by the call)
 *   out: d_occ_count i32[S,B], d_point_count i32[S], d_feats_spp f32[S,D],
 *        d_occ_bits u64[S, ceil(B/64)]  (bit b of row s = bb_occupancy_spp[s,b]),
 *        d_n_bbs i32[S]                 (n_bbs_per_spp, gen_ps_utils.py:363)
 * `thresh_spp_occu` is compared as float32, as torch does.             */
int gapro_partition_pool(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t feat_dim,
                         int32_t n_boxes, int32_t n_spps, int32_t fixed_shift, float thresh_spp_occu,
                         const double* d_coords, const float* d_feats, const int32_t* d_spp_inv,
                         const double* d_boxes, int64_t* d_feat_sum, int32_t* d_occ_count,
                         int32_t* d_point_count, float* d_feats_spp, uint64_t* d_occ_bits,
                         int32_t* d_n_bbs);

/* Superpoint -> point broadcast of the three point-length outputs (gen_ps_utils.py:478-480). */
int gapro_broadcast_labels(gapro_ctx* ctx, void* stream, int64_t n_points, const int32_t* d_spp_inv,
                           const int32_t* d_sem_spp, const int32_t* d_inst_spp, const float* d_prob_spp,
                           int32_t* d_sem, int32_t* d_inst, float* d_prob);

/* ---- Batched forms: every scene of a batch in ONE launch per kernel (grid.y = scene). ----------
 * A 64-scene batch through the per-scene calls above is ~1200 launches of 3-5 us kernels; the batched
 * calls are ~15.  One gapro_scene_task per scene holds the device pointers of that scene; the three
 * calls read the fields of their stage (the caller fills n_spps / fixed_shift from the headers between
 * prepare and pool).  `h_tasks` is copied to `d_tasks` (device, n_scenes tasks) on the stream and must
 * stay valid until the stream has executed that copy. */
typedef struct {
  /* every stage */
  int64_t n_points;
  const double* coords;       /* f64[N,3] */
  const float* feats;         /* f32[N,D] */
  const int64_t* spp;         /* i64[N]   */
  int32_t* spp_inv;           /* i32[N]   out of prepare, in of pool / broadcast */
  /* prepare */
  void* prepare_ws;           /* >= gapro_partition_prepare_workspace_bytes(N, spp_range_cap) */
  int64_t spp_range_cap;
  /* pool */
  const double* boxes;        /* f64[B,6] */
  int32_t n_boxes, n_spps, fixed_shift;
  float thresh_spp_occu;
  int64_t* feat_sum;          /* i64[S,D] tmp */
  int32_t* occ_count;         /* i32[S,B] */
  int32_t* point_count;       /* i32[S]   */
  float* feats_spp;           /* f32[S,D] */
  uint64_t* occ_bits;         /* u64[S,ceil(B/64)] */
  int32_t* n_bbs;             /* i32[S]   */
  /* broadcast */
  const int32_t* sem_spp;     /* i32[S] */
  const int32_t* inst_spp;    /* i32[S] */
  const float* prob_spp;      /* f32[S] */
  int32_t* sem;               /* i32[N] */
  int32_t* inst;              /* i32[N] */
  float* prob;                /* f32[N] */
} gapro_scene_task;

/* gapro_partition_prepare_async for n_scenes scenes; the headers land in h_headers_pinned[n_scenes]
 * (page-locked) through d_headers[n_scenes] (device) once the stream reaches that point. */
int gapro_partition_prepare_batch(gapro_ctx* ctx, void* stream, int32_t n_scenes, int32_t feat_dim,
                                  const gapro_scene_task* h_tasks, gapro_scene_task* d_tasks,
                                  gapro_scene_header* d_headers, gapro_scene_header* h_headers_pinned);
/* gapro_partition_pool for n_scenes scenes (zeroes the tallies itself). */
int gapro_partition_pool_batch(gapro_ctx* ctx, void* stream, int32_t n_scenes, int32_t feat_dim,
                               const gapro_scene_task* h_tasks, gapro_scene_task* d_tasks);
/* Which pooling kernel gapro_partition_pool_batch runs for (feat_dim, the largest n_boxes of the batch): 6, 5 or 4 =
 * the LDS-table kernel with 2^that slots, 0 = the global-atomics kernel (also whenever GAPRO_POOL_GLOBAL_ATOMICS is set),
 * GAPRO_ERR_BAD_ARG = more boxes than the LDS holds corners of (1365), or a non-positive argument. */
int gapro_partition_pool_plan(int32_t feat_dim, int32_t n_boxes_max);
/* gapro_broadcast_labels for n_scenes scenes. */
int gapro_broadcast_labels_batch(gapro_ctx* ctx, void* stream, int32_t n_scenes,
                                 const gapro_scene_task* h_tasks, gapro_scene_task* d_tasks);

/* ------------------------------------------------------------------------------------------
 * Label-side kernels on either end of the path (not needed by a caller of
 * gen_pseudo_label_gaussian_process itself).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t instance_num;  /* int(instance_label.max()) + 1            gen_ps_utils.py:200 */
  int32_t n_boxes;       /* non-empty instance ids = rows of the outputs              */
  int32_t status;        /* GAPRO_ERR_BAD_ARG: an id >= max_instances was met         */
  int32_t reserved;
} gapro_instance_header;

size_t gapro_instance_info_workspace_bytes(int32_t max_instances);
/* getInstanceInfo (gen_ps_utils.py:195-239) in one pass over the points: per non-empty GT instance id, in
 * ascending id order, the axis-aligned box [min xyz | max xyz] (f64), the class = semantic label of the
 * instance's first point (minus 2 unless -100 when scannet_class_shift != 0, :236-237) and the volume
 * prod(clip(max - min, 0)) (f64).  Labels come as the float64 arrays the ScanNet .pth files hold.
 *   in : d_coords f64[N,3], d_instance_label f64[N], d_semantic_label f64[N]
 *   out: d_box f64[<=max_instances,6], d_cls f64[..], d_volume f64[..], d_corners f32[N,6] or NULL
 *        (corners_label, :203,219-220), header (device + page-locked host copy, enqueue only)     */
int gapro_instance_info(gapro_ctx* ctx, void* stream, int64_t n_points, const double* d_coords,
                        const double* d_instance_label, const double* d_semantic_label, int32_t max_instances,
                        int32_t scannet_class_shift, void* d_workspace, size_t workspace_bytes, double* d_box,
                        double* d_cls, double* d_volume, float* d_corners, gapro_instance_header* d_header,
                        gapro_instance_header* h_header_pinned);

/* Pseudo-label evaluation (the reference's eval_ps_labels.py, :35-42,100-257): get_miou_scene and
 * get_scene_sem_conf for a batch of scenes laid out back to back in the label arrays, unfiltered (row 0) and
 * for K probability thresholds (row t = the points with prob >= thresholds[t-1], the reference's commented-out
 * certain_cond filter :214-220, applied to all four arrays), in one pass over the points; one scene without
 * thresholds is the per-scene evaluation.  Integer atomics only: every row is bit-identical to the reference's
 * get_miou_scene / get_scene_sem_conf on the filtered scene alone, whatever the batch composition. */
enum {
  GAPRO_LABEL_F64 = 1,  /* ScanNet *_inst_nostuff.pth labels */
  GAPRO_LABEL_I32 = 2,  /* gen_ps label files */
  GAPRO_LABEL_I64 = 3
};
#define GAPRO_EVAL_MAX_THRESHOLDS 32

typedef struct {
  int64_t point_offset;  /* in : first point of the scene in the label arrays                              */
  int64_t n_points;      /* in : may be 0                                                                  */
  int32_t max_gt;        /* in : GT instance ids are < max_gt (>= 1); a larger id sets status[scene]       */
  int32_t max_ps;        /* in : pseudo instance ids are < max_ps (>= 1)                                   */
  int64_t ws_offset;     /* set by gapro_eval_batch_workspace_bytes: the scene's bytes in the workspace    */
  int64_t row_offset;    /* set by gapro_eval_batch_workspace_bytes: the scene's first entry in d_max_iou  */
} gapro_eval_scene;

/* Fills ws_offset / row_offset of h_scenes[n_scenes] and returns the workspace size in bytes; the IoU outputs
 * hold row_offset[last] + (n_thresholds + 1) * max_gt[last] entries (0 on a bad argument). */
size_t gapro_eval_batch_workspace_bytes(gapro_eval_scene* h_scenes, int32_t n_scenes, int32_t n_thresholds);
/*   in : labels of n_total_points points, each array in its own dtype code (GT: F64 / I32 / I64, pseudo: I32 /
 *        I64); d_prob f32[n_total_points] (NULL when n_thresholds = 0); h_thresholds f32[n_thresholds],
 *        ascending (host); scannet_remap != 0 applies sem[sem != -100] -= 2, then -1 / -2 -> 18 to the GT
 *        semantic labels (:196-197); h_scenes as filled above, d_scenes device space for n_scenes of them.
 *   out: d_max_iou / d_gt_cls f32 at row_offset + t * max_gt + g: scene, threshold row t, GT id g: the largest
 *        IoU = inter / (|gt| + |ps| - inter + 1e-4) (float32, the reference's operation order) over the pseudo
 *        instances whose class (label of their first point) equals the GT instance's, and that class (-1 for an
 *        empty id; the caller keeps the entries with class >= 0, :139);
 *        d_conf i64[n_thresholds + 1, C, C] summed over the batch (rows = GT class, columns = pseudo class,
 *        over the points with GT != -100; a pseudo label of -100 counts as a wrong class);
 *        d_kept i64[n_scenes, n_thresholds + 1] points per scene and row; d_status i32[n_scenes]
 *        (GAPRO_ERR_BAD_ARG: an id beyond max_gt / max_ps: that scene's IoUs are not valid).  Enqueue only.
 * Confusion only: with d_inst_gt and d_inst_ps both NULL, no instance tables are tallied.  d_conf and d_kept
 * are produced as above; d_max_iou / d_gt_cls may be NULL (if given, every id reads as empty), the instance
 * dtype codes are ignored, and max_gt = max_ps = 1 keeps the workspace at its minimum. */
int gapro_eval_batch(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_eval_scene* h_scenes,
                     gapro_eval_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype, const void* d_sem_gt,
                     int32_t inst_gt_dtype, const void* d_inst_gt, int32_t sem_ps_dtype, const void* d_sem_ps,
                     int32_t inst_ps_dtype, const void* d_inst_ps, const float* d_prob, int32_t n_thresholds,
                     const float* h_thresholds, int32_t scannet_remap, int32_t num_classes, void* d_workspace,
                     size_t workspace_bytes, float* d_max_iou, float* d_gt_cls, int64_t* d_conf, int64_t* d_kept,
                     int32_t* d_status);

/* ScanNet instance AP of pseudo-labels (the reference's eval_ap_ps_labels.py with ISBNet's
 * ScanNetEval.assign_instances_for_scan): the integer tables of a batch of scenes laid out back to back, in two
 * calls with one host read of the key counts in between.  A GT point's key is the code
 * (sem + 1) * 1000 + (inst + 1) after the optional remap; it is a GT instance when sem + 1 is in 1..18 and
 * inst + 1 in [0, 1000), i.e. inst in -1..998, else the point is void.  The matching and the AP run on the host.
 * Integer atomics only: every table is bit-identical to a plain tally of the scene alone, whatever the batch
 * composition. */
typedef struct {
  int64_t point_offset;  /* in : first point of the scene in the label arrays                                 */
  int64_t n_points;      /* in : may be 0                                                                     */
  int32_t max_ps;        /* in : pseudo instance ids are -100 (none) or in [0, max_ps) (>= 1)                 */
  int32_t n_keys;        /* in for gapro_eval_ap_tables: the scene's d_n_keys from gapro_eval_ap_keys         */
  int64_t ws_offset;     /* set by gapro_eval_ap_workspace_bytes: the scene's bytes in the workspace          */
  int64_t id_offset;     /* set by gapro_eval_ap_workspace_bytes: the scene's first entry in the per-id outputs */
  int64_t key_offset;    /* set by gapro_eval_ap_pair_cells: the scene's first entry in the per-key outputs   */
  int64_t pair_offset;   /* set by gapro_eval_ap_pair_cells: the scene's first cell in d_pair                 */
} gapro_eval_ap_scene;

/* Fills ws_offset / id_offset of h_scenes[n_scenes] and returns the workspace size in bytes (0 on a bad
 * argument); the per-id outputs hold id_offset[last] + max_ps[last] entries. */
size_t gapro_eval_ap_workspace_bytes(gapro_eval_ap_scene* h_scenes, int32_t n_scenes);
/* Pass 1.  in : GT labels of n_total_points points in their dtype codes (F64 / I32 / I64); scannet_remap != 0
 *        applies sem[sem != -100] -= 2, then -1 / -2 -> 18 (eval_ap_ps_labels.py:59-60).
 *   out: d_n_keys i32[n_scenes] distinct GT instance keys per scene; d_status i32[n_scenes] (GAPRO_ERR_BAD_ARG:
 *        an instance id >= 999); the key ranks in the workspace.  Enqueue only. */
int gapro_eval_ap_keys(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_eval_ap_scene* h_scenes,
                       gapro_eval_ap_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype, const void* d_sem_gt,
                       int32_t inst_gt_dtype, const void* d_inst_gt, int32_t scannet_remap, void* d_workspace,
                       size_t workspace_bytes, int32_t* d_n_keys, int32_t* d_status);
/* With n_keys set: fills key_offset / pair_offset and returns the pair cells, the sum over the scenes of
 * (n_keys + 1) * (max_ps + 1) (0 on a bad argument); the per-key outputs hold key_offset[last] + n_keys[last]. */
int64_t gapro_eval_ap_pair_cells(gapro_eval_ap_scene* h_scenes, int32_t n_scenes);
/* Pass 2, on the workspace of pass 1.  in : the labels as for gapro_eval_ap_keys plus the pseudo labels (I32 /
 *        I64) and d_prob f32[n_total_points] or NULL.
 *   out: per key k of a scene, ascending: d_key_code i32 (class * 1000 + inst + 1), d_key_n i32 points;
 *        per pseudo id p: d_ps_n i32 points, d_ps_label i32 = pseudo semantic label + 1 of its first point when
 *        that is in 1..18, else 0, d_ps_void i32 points of no GT instance, d_ps_sum i64 = sum over its points of
 *        rint(double(prob) * 2^32) (0 without d_prob);
 *        d_pair i32 [n_keys + 1][max_ps + 1] at pair_offset: points per (key + 1, id + 1), row 0 = void, column
 *        0 = pseudo id -100;
 *        d_status i32[n_scenes] (GAPRO_ERR_BAD_ARG: a GT instance id >= 999, a pseudo id < 0 other than -100 or
 *        >= max_ps, n_keys below pass 1's count, or a probability that is NaN or outside [0, 1]: that scene's
 *        tables are not valid).  Enqueue only. */
int gapro_eval_ap_tables(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_eval_ap_scene* h_scenes,
                         gapro_eval_ap_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype,
                         const void* d_sem_gt, int32_t inst_gt_dtype, const void* d_inst_gt, int32_t sem_ps_dtype,
                         const void* d_sem_ps, int32_t inst_ps_dtype, const void* d_inst_ps, const float* d_prob,
                         int32_t scannet_remap, void* d_workspace, size_t workspace_bytes, int32_t* d_key_code,
                         int32_t* d_key_n, int32_t* d_ps_n, int32_t* d_ps_label, int32_t* d_ps_void,
                         int64_t* d_ps_sum, int32_t* d_pair, int32_t* d_status);
/* The AP tables with probability-threshold rows, as gapro_eval_batch has them: row 0 is the scene as it is, row t
 * (1..n_thresholds) the scene restricted, in all four label arrays, to the points with prob >= thresholds[t-1]
 * (float32 compare).  A row's tables are the tables of that filtered scene: an id's label is that of its first kept
 * point, the counts and d_ps_sum are over the kept points.  Pass 1 is unchanged and ranks the keys of the whole
 * scene, so a key without a kept point stays in its place with d_key_n = 0 (the caller drops it), as a pseudo id
 * without a kept point has d_ps_n = 0 and d_ps_label = 0.  One pass over the points, one atomic of each kind per
 * point, into the tables of the point's bin #{j : prob >= thresholds[j]}; a suffix sum / min over the bins makes
 * the rows.
 * gapro_eval_ap_workspace_bytes_rows: gapro_eval_ap_workspace_bytes (same ws_offset / id_offset, so the workspace
 * serves gapro_eval_ap_keys as it is) plus n_thresholds first-point rows behind the scenes' blocks; 0 on a bad
 * argument or n_thresholds outside [0, GAPRO_EVAL_MAX_THRESHOLDS]. */
size_t gapro_eval_ap_workspace_bytes_rows(gapro_eval_ap_scene* h_scenes, int32_t n_scenes, int32_t n_thresholds);
/* Pass 2 with rows.  in : as gapro_eval_ap_tables, plus h_thresholds f32[n_thresholds] (host), ascending; d_prob
 *        is needed when n_thresholds > 0; the workspace of pass 1, sized by gapro_eval_ap_workspace_bytes_rows.
 *   out: every per-key, per-id and pair output of gapro_eval_ap_tables with a leading row dimension of
 *        n_thresholds + 1 whose stride is the output's size for the whole batch: d_key_code / d_key_n
 *        i32[rows][key_offset[last] + n_keys[last]] (d_key_code is the same in every row), d_ps_n / d_ps_label /
 *        d_ps_void i32 and d_ps_sum i64 [rows][id_offset[last] + max_ps[last]], d_pair i32[rows][pair cells].  Row
 *        0's block is gapro_eval_ap_tables' output, bit for bit; gapro_eval_ap_tables is this call without
 *        thresholds.  The points of a scene's row are the sum of its pair cells.  d_status i32[n_scenes] as for
 *        gapro_eval_ap_tables: a probability that is NaN or outside [0, 1] is GAPRO_ERR_BAD_ARG for the scene.
 * Refused with GAPRO_ERR_BAD_ARG: n_thresholds outside [0, GAPRO_EVAL_MAX_THRESHOLDS], thresholds that are NaN
 * or not ascending (equal ones are allowed), thresholds without d_prob; GAPRO_ERR_WORKSPACE: a workspace
 * without the first-point rows.  Enqueue only. */
int gapro_eval_ap_tables_rows(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_eval_ap_scene* h_scenes,
                              gapro_eval_ap_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype,
                              const void* d_sem_gt, int32_t inst_gt_dtype, const void* d_inst_gt, int32_t sem_ps_dtype,
                              const void* d_sem_ps, int32_t inst_ps_dtype, const void* d_inst_ps, const float* d_prob,
                              int32_t n_thresholds, const float* h_thresholds, int32_t scannet_remap, void* d_workspace,
                              size_t workspace_bytes, int32_t* d_key_code, int32_t* d_key_n, int32_t* d_ps_n,
                              int32_t* d_ps_label, int32_t* d_ps_void, int64_t* d_ps_sum, int32_t* d_pair,
                              int32_t* d_status);

/* Heuristic labelers: gen_pseudo_label (gen_ps_utils.py:485-569; rule 0 = "volume",
 * 1 = "dist", 2 = "none") and gen_pseudo_label_box2mask (:242-290; rule 3).  Membership in the INSTANCE boxes
 * (float32 box, 0.005 margin applied in float32, compared in float64), the rule for points inside several boxes,
 * then (align != 0, the scannetv2 branch) the superpoint vote spp_align_label (:99-123) with the >= 0.7
 * occupancy mask (not for box2mask).  "dist" reproduces the reference's indexing of the coordinate array by the
 * rank among the multi-box points (:525).  d_spp_inv = dense superpoint ranks from gapro_partition_prepare.
 *   out: d_sem i32[N] (class, instance_classes for background, -100), d_inst i32[N] (box index or -100) */
size_t gapro_label_heuristic_workspace_bytes(int64_t n_points, int32_t n_spps, int32_t n_boxes);
int gapro_label_heuristic(gapro_ctx* ctx, void* stream, int64_t n_points, const double* d_coords,
                          const int32_t* d_spp_inv, int32_t n_spps, int32_t n_boxes, const float* d_box,
                          const float* d_volume, const int64_t* d_cls, int32_t rule, int32_t align,
                          int32_t instance_classes, void* d_workspace, size_t workspace_bytes, int32_t* d_sem,
                          int32_t* d_inst);

/* ------------------------------------------------------------------------------------------
 * Consumer-side label ops: what the training code does with the generated labels.
 * Forward values and the gradients w.r.t. the network outputs come out of the same call; reductions are
 * float64 sums of float32 terms.  `grad_out` scales the gradients (pass 1 and multiply later to stay async).
 * ---------------------------------------------------------------------------------------- */
/* custom_scatter_mean (ISBNet/isbnet/model/model_utils.py:600-613) of the three label channels at once
 * (isbnet.py:387-389): out[s] = mean of the points with index s (count clamped at 1, as torch_scatter does).
 *   d_index i64[N] in [0, n_out) (a point whose index is outside is skipped), d_sums_ws f64[3 n_out] and
 *   d_counts_ws i32[n_out] are scratch. */
int gapro_label_pool_mean(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t n_out, const int64_t* d_index,
                          const float* d_prob, const float* d_mu, const float* d_var, double* d_sums_ws,
                          int32_t* d_counts_ws, float* d_out_prob, float* d_out_mu, float* d_out_var);
/* Probability-weighted BCE with logits (ISBNet/isbnet/model/criterion.py:287-288):
 *   loss = sum_{g,p} bce(x[g][p], y[g][p]) w[p] / sum_p w[p] / (G + 1e-6),  x, y f32[G,P] row-major, w f32[P];
 *   d_grad_logits f32[G,P] or NULL; d_acc2 f64[2] scratch. */
int gapro_weighted_bce_with_logits(gapro_ctx* ctx, void* stream, int32_t n_rows, int64_t n_cols, const float* d_logits,
                                   const float* d_targets, const float* d_weights, float grad_out, double* d_acc2,
                                   float* d_loss, float* d_grad_logits);
/* KL-to-GP auxiliary loss (ISBNet/isbnet/model/criterion.py:435-463): labels of -100 are ignored; GP variances
 * <= epsilon use the (exp(logvar) - 1)^2 + (mu - mu_l)^2 branch, the others the Gaussian KL expression; each
 * branch is averaged over its own count (+1e-4) and scaled by `weight`.  Gradients w.r.t. mu_pred / logvar_pred
 * (f32[n], or both NULL); d_acc4 f64[4] scratch. */
int gapro_kl_gp_loss(gapro_ctx* ctx, void* stream, int64_t n, const float* d_mu_labels, const float* d_var_labels,
                     const float* d_mu_pred, const float* d_logvar_pred, float epsilon, float weight, float grad_out,
                     double* d_acc4, float* d_loss, float* d_grad_mu, float* d_grad_logvar);

/* ------------------------------------------------------------------------------------------
 * Static pair schedule and merge (host).  Replaces the control flow of gen_ps_utils.py:365-476.
 * Which pairs are fitted and on which superpoints depends only on (boxes, bb_occupancy_spp),
 * never on GP outputs, so the whole schedule is enumerated before any fit runs.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_events;       /* containment verdicts + GP fits, in reference order */
  int32_t n_fits;
  int64_t n_event_idx;    /* total length of all intersect index lists */
  int64_t n_fit_idx;      /* total length of all [b1_inds | b2_inds | intersect_inds] lists */
  int64_t n_fit_out;      /* total number of test superpoints over all fits */
  int32_t max_m;          /* largest m1+m2 of any fit */
  int32_t max_t;          /* largest |intersect_inds| of any fit */
} gapro_schedule_counts;

/* One GP fit of the batch.  Index lists live in one int32 array laid out
 * [b1_inds (m1) | b2_inds (m2) | intersect_inds (t)] at idx_offset; values are ROWS of the
 * feats_spp array handed to gapro_svgp_fit_batch (superpoint index + feats_row_base). */
typedef struct {
  int32_t m1, m2, t;
  int32_t b1, b2;        /* the two boxes (informational) */
  int32_t scene;         /* caller tag (informational) */
  int32_t slot;          /* row of d_fit_status / d_fit_loss this fit reports to (set by the library) */
  int32_t reserved;
  int64_t idx_offset;    /* into the index array */
  int64_t out_offset;    /* into the per-test-superpoint outputs */
  int64_t ws_offset;     /* into the workspace, in doubles (filled by gapro_fit_plan_workspace) */
} gapro_fit_desc;

/* h_boxes f64[B,6], h_occ_bits u64[S,ceil(B/64)], h_n_bbs i32[S] (outputs of gapro_partition_pool). */
int gapro_schedule_build(int32_t n_spps, int32_t n_boxes, const double* h_boxes,
                         const uint64_t* h_occ_bits, const int32_t* h_n_bbs, gapro_schedule** out);
void gapro_schedule_free(gapro_schedule* s);
int gapro_schedule_get_counts(const gapro_schedule* s, gapro_schedule_counts* out);
/* Export the fits: h_descs[n_fits], h_idx i32[n_fit_idx].  `feats_row_base` is added to every
 * index, `idx_base`/`out_base` to the offsets, `scene` is copied into the descs (for batching
 * several scenes into one gapro_svgp_fit_batch call). */
int gapro_schedule_export_fits(const gapro_schedule* s, int32_t feats_row_base, int64_t idx_base,
                               int64_t out_base, int32_t scene, gapro_fit_desc* h_descs, int32_t* h_idx);
/* Export the events for inspection/tests: kind (0 contain, 1 fit), b1, b2, winner (contain) or
 * fit id (fit), offsets[n_events+1] into h_event_idx (superpoint indices of the intersection). */
int gapro_schedule_export_events(const gapro_schedule* s, uint8_t* h_kind, int32_t* h_b1, int32_t* h_b2,
                                 int32_t* h_aux, int64_t* h_offsets, int32_t* h_event_idx);
/* The fit events that tested each superpoint, as a CSR over the superpoints: entries [h_offsets[sp], h_offsets[sp + 1])
 * of h_fit / h_pos, in event order (the order in which the merge meets them).  h_fit is the fit's index in
 * gapro_schedule_export_fits order, h_pos the superpoint's position inside that fit's intersection, i.e. its row in the
 * fit's output slice.  h_offsets i64[n_spps + 1]; h_fit, h_pos i32[gapro_schedule_counts.n_fit_out] (may be NULL when
 * that is 0).  Containment events are not listed. */
int gapro_schedule_export_testers(const gapro_schedule* s, int64_t* h_offsets, int32_t* h_fit, int32_t* h_pos);

/* Merge + fallback + label tables (gen_ps_utils.py:365-383, :411-423, :438-476).
 * Fit outputs are this schedule's slices (out_offset relative to 0): probs_new f32, labels u8,
 * mu f32, var f32, each [n_fit_out].
 *   in : h_boxes_cls i64[B], h_boxes_volume f64[B], n_fg_instances, instance_classes
 *   out: h_sem_spp i32[S], h_inst_spp i32[S], h_prob_spp f32[S], h_mu_spp f32[S], h_var_spp f32[S] */
int gapro_schedule_merge(const gapro_schedule* s, const float* h_probs_new, const uint8_t* h_labels,
                         const float* h_mu, const float* h_var, const int64_t* h_boxes_cls,
                         const double* h_boxes_volume, int32_t n_fg_instances, int32_t instance_classes,
                         int32_t* h_sem_spp, int32_t* h_inst_spp, float* h_prob_spp, float* h_mu_spp,
                         float* h_var_spp);
/* gapro_schedule_merge plus one more output: h_winner_fit i32[S] (NULL = not wanted, which is gapro_schedule_merge; the
 * other outputs are the same bits either way).  winner[sp] is the index, in gapro_schedule_export_fits order, of the fit
 * whose outputs superpoint sp ends up with, -1 where no fit labels it:
 *   - it starts at -1;
 *   - a fit event that overwrites sp (the strict float32 `<` on probs_new) sets it to that fit;
 *   - a containment event that writes sp sets it back to -1 (probability 1; the superpoint keeps the stale mu / var
 *     of the fit it had, as gapro_schedule_merge always did);
 *   - the smallest-volume fallback only touches superpoints no event determined, which have no winner. */
int gapro_schedule_merge_ex(const gapro_schedule* s, const float* h_probs_new, const uint8_t* h_labels,
                            const float* h_mu, const float* h_var, const int64_t* h_boxes_cls,
                            const double* h_boxes_volume, int32_t n_fg_instances, int32_t instance_classes,
                            int32_t* h_sem_spp, int32_t* h_inst_spp, float* h_prob_spp, float* h_mu_spp,
                            float* h_var_spp, int32_t* h_winner_fit);

/* ------------------------------------------------------------------------------------------
 * Batched variational-GP fit (device). Replaces gaussian_process_utils.py:382-445 and the
 * gpytorch objects it builds (GPClassificationModel :11-25, BernoulliLikelihood, VariationalELBO,
 * Adam lr 0.1, 50 steps).  One workgroup trains one fit for all `training_iter` steps inside a
 * single launch; every fit of every scene in the batch runs concurrently.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t training_iter;     /* 50   gaussian_process_utils.py:382,416 */
  double lr;                 /* 0.1  gaussian_process_utils.py:410 */
  double jitter;             /* 1e-4 gpytorch variational_cholesky_jitter (float32 default) */
  double min_variance;       /* 1e-6 gpytorch settings.min_variance; negative or not finite is refused (BAD_ARG) */
  int32_t eval_stale_chol;   /* 0 = refactor K_ZZ with the trained parameters for prediction (default);
                                1 = reuse the factor of the last training step */
  int32_t reserved;          /* 0; debug bits GAPRO_FIT_DBG_* (below); any other bit is refused */
  int32_t psd_retries;       /* 3    gpytorch settings.cholesky_max_tries: a factorisation that meets a non-positive
                              *      pivot is repeated on K + psd_jitter 10^i I, i < psd_retries (psd_safe_cholesky,
                              *      reached from gaussian_process_utils.py:417); 0 = fail at once */
  int32_t precision;         /* GAPRO_PRECISION_*: arithmetic of the fit (0 = float64 throughout, the default) */
  double psd_jitter;         /* 1e-8 gpytorch settings.cholesky_jitter for float64 (K_ZZ is factored in double) */
} gapro_fit_options;

/* gapro_fit_options.reserved: debug bits, 0 in the product.  gapro_svgp_fit_batch refuses any bit not named here
 * (GAPRO_ERR_BAD_ARG). */
enum {
  GAPRO_FIT_DBG_NO_STRIP = 1,             /* never route a fit to the strip-streaming kernels */
  GAPRO_FIT_DBG_CALLER_STREAM = 2,        /* launch the fit kernels on the caller's stream (not the fit streams) */
  GAPRO_FIT_DBG_NO_SMALL = 4,             /* no small-fit kernel (M_p <= 64 runs the 512-thread strip kernel) */
  GAPRO_FIT_DBG_NO_CLUSTER = 8,           /* no cluster kernel (large fits stay on one workgroup) */
  GAPRO_FIT_DBG_CLUSTER_ALL = 16,         /* the cluster kernel for every fit it can take (M_p >= 64, M_p % 32 == 0) */
  GAPRO_FIT_DBG_WG_TILED_ALL = 8192,      /* workgroup-tiled products through LDS in the staged kernel at every
                                           * M_p > 128 (default: M_p = 256, 384 only; bit-identical either way) */
  GAPRO_FIT_DBG_CLUSTER_STALL = 32768,    /* TEST: the last member of every cluster never arrives (barrier timeout) */
  GAPRO_FIT_DBG_WG_TILED_NONE = 131072,   /* no workgroup-tiled products (round 2's products) */
  GAPRO_FIT_DBG_STATIC_MAP = 262144,      /* workgroup b of a fit kernel runs fit b of its list (default: the
                                           * workgroups take the fits in the order in which they start, claim_fit in
                                           * csrc/fit_wg.h) */
  GAPRO_FIT_DBG_NO_WAVE = 1048576,        /* no wave-per-fit kernel (M_p <= 48 runs the small-fit strip kernel) */
  GAPRO_FIT_DBG_ALL = 1 | 2 | 4 | 8 | 16 | 8192 | 32768 | 131072 | 262144 | 1048576
};

/* gapro_fit_options.precision */
enum {
  GAPRO_PRECISION_F64 = 0,   /* everything in float64 (a superset of the reference's split) */
  GAPRO_PRECISION_MIXED = 1  /* the reference's own split: parameters, kernel matrices, A, B, variances and their
                              * gradients in float32 (v_mfma_f32), float64 for the Cholesky factor, the L^-1
                              * products and their backward (gpytorch _cholesky_factor / torch autograd).
                              * Implemented by the cluster kernel (route 4); fits routed to the other kernels run
                              * in float64, a superset of the split */
};

void gapro_fit_options_default(gapro_fit_options* opt);

/* Workspace doubles one fit with m = m1+m2 inducing points, t test points, feat_dim d needs. */
int64_t gapro_fit_workspace_doubles(int32_t m, int32_t t, int32_t feat_dim);
/* Fill ws_offset of every desc; returns the total workspace size in BYTES. */
int64_t gapro_fit_plan_workspace(gapro_fit_desc* h_descs, int32_t n_fits, int32_t feat_dim);

/* d_feats_spp f32[rows,D]; d_idx i32; h_descs gapro_fit_desc[n_fits] on the HOST (the library orders
 * the launch longest-fit-first and picks the kernel variant per fit) and d_descs, a device buffer of
 * n_fits descriptors the library fills (the call synchronises the stream once for that copy, then
 * only enqueues);
 * d_init_mean f64 (optional, may be NULL = zeros): initial variational mean of fit i at
 *   d_init_mean[idx_offset ... + m] (gpytorch adds 1e-3*randn here; zeros make runs reproducible);
 * outputs per test superpoint at out_offset: d_probs f32, d_probs_new f32, d_labels u8,
 *   d_mu f32, d_var f32  (pred_probs, pred_probs_new, pred_labels, pred_mu, pred_variance);
 * d_fit_status i32[n_fits] (gapro_status per fit, in h_descs order), d_fit_loss f64[n_fits] (last
 *   ELBO loss, in h_descs order). */
int gapro_svgp_fit_batch(gapro_ctx* ctx, void* stream, int32_t n_fits, int32_t feat_dim,
                         const float* d_feats_spp, const int32_t* d_idx, const gapro_fit_desc* h_descs,
                         gapro_fit_desc* d_descs, const double* d_init_mean, const gapro_fit_options* opt,
                         double* d_workspace,
                         size_t workspace_bytes, float* d_probs, float* d_probs_new, uint8_t* d_labels,
                         float* d_mu, float* d_var, int32_t* d_fit_status, double* d_fit_loss);
/* The same launch with one more optional per-fit output (round 6): d_fit_cond[n_fits] (double, device; NULL = not wanted)
 * receives a conditioning figure of each fit's LAST Cholesky factorisation, (max_j L_jj / min_j L_jj)^2 over the fit's M
 * rows -- a lower bound of cond_2(K_ZZ + jitter I), read from the diagonal-block inverses the kernels keep anyway.  A
 * diagnostic, NOT a predictor of which fits are numerically soft: on the S3DIS-shaped test scene the two fits whose
 * sigma^2 no float64 implementation reproduces to 1e-4 rank 38th and 55th of 66 by this figure (and 35th / 61st by the
 * true cond_2 at the initial hyper-parameters); what identifies them is a perturbation probe -- the fits once more with
 * the jitter on K_ZZ's diagonal scaled by (1 + 1e-11) (Pipeline.reproducibility_probe).  Status, outputs and arithmetic
 * are those of gapro_svgp_fit_batch. */
int gapro_svgp_fit_batch_ex(gapro_ctx* ctx, void* stream, int32_t n_fits, int32_t feat_dim,
                            const float* d_feats_spp, const int32_t* d_idx, const gapro_fit_desc* h_descs,
                            gapro_fit_desc* d_descs, const double* d_init_mean, const gapro_fit_options* opt,
                            double* d_workspace,
                            size_t workspace_bytes, float* d_probs, float* d_probs_new, uint8_t* d_labels,
                            float* d_mu, float* d_var, int32_t* d_fit_status, double* d_fit_loss, double* d_fit_cond);

/* ------------------------------------------------------------------------------------------
 * The trained models of a fit launch, and predictions from them at other inputs.
 *
 * State of one fit with M = m1 + m2 inducing points at feature width D: gapro_gp_state_doubles(M, D) =
 * 8 + M D + M + M M doubles, the same layout whatever kernel trained the fit and whatever `precision` it ran in:
 *   [0] M   [1] D   [2] the fit's gapro_status (0 = ok; a failed fit leaves a state that says so)
 *   [3] variational jitter the fit was trained with (gapro_fit_options.jitter)
 *   [4] c (constant mean)   [5] rho_s (raw output scale)   [6] rho_l (raw length scale)   [7] 0 (reserved)
 *   Z f64[M, D] row-major | variational mean f64[M] | tril(L_S) f64[M, M] row-major, upper part zero
 * Output scale and length scale are softplus(rho_s), softplus(rho_l).  Unpadded: M = 50 exports 50 rows.
 * ---------------------------------------------------------------------------------------- */
int64_t gapro_gp_state_doubles(int32_t m, int32_t feat_dim);
/* h_state_offsets[i] (in doubles) for fit i of h_descs, packed in order; returns the total size in BYTES. */
int64_t gapro_gp_state_plan(const gapro_fit_desc* h_descs, int32_t n_fits, int32_t feat_dim, int64_t* h_state_offsets);
/* gapro_svgp_fit_batch_ex with the trained models kept: when the launch has finished, d_state + h_state_offsets[i]
 * holds the state of fit i (h_descs order).  d_state == NULL is exactly gapro_svgp_fit_batch_ex; with a state buffer
 * the launch's outputs, statuses and losses are the same bits.  state_bytes = size of d_state (GAPRO_ERR_WORKSPACE if a
 * state would end beyond it).  Launches that keep states must be issued on one stream per context. */
int gapro_svgp_fit_batch_state(gapro_ctx* ctx, void* stream, int32_t n_fits, int32_t feat_dim,
                               const float* d_feats_spp, const int32_t* d_idx, const gapro_fit_desc* h_descs,
                               gapro_fit_desc* d_descs, const double* d_init_mean, const gapro_fit_options* opt,
                               double* d_workspace, size_t workspace_bytes, float* d_probs, float* d_probs_new,
                               uint8_t* d_labels, float* d_mu, float* d_var, int32_t* d_fit_status, double* d_fit_loss,
                               double* d_fit_cond, double* d_state, const int64_t* h_state_offsets, size_t state_bytes);

/* One model of a predict launch: its state at d_state + state_offset (doubles); test row r of the model is the feature
 * row d_rows[row_offset + r], r < t; its five outputs go to [out_offset, out_offset + t). */
typedef struct {
  int64_t state_offset;
  int64_t row_offset;
  int64_t out_offset;
  int32_t t;
  int32_t reserved;      /* 0 */
} gapro_predict_desc;

/* Bytes of device workspace a predict launch of n_models models needs; h_m[i] = M of model i. */
size_t gapro_svgp_predict_workspace_bytes(int32_t n_models, int32_t feat_dim, const int32_t* h_m);
/* Posterior of every model at its test rows (gaussian_process_utils.py:426-438 with the model's own parameters):
 *   K_ZZ + jitter I is factored FRESH from the state (psd_safe_cholesky's retry rule: opt->psd_retries, opt->psd_jitter;
 *   a state exported from an eval_stale_chol = 1 launch therefore predicts with the fresh factor, not the stale one),
 *   A = L^-1 k(Z, x), mu = A^T m + c, var = max(s + jitter + |L_S^T A|^2 - |A|^2, opt->min_variance),
 *   p = Phi(mu / sqrt(1 + var)), label = (float)p >= 0.5f, probs_new = label ? p : 1 - p; float64, rounded to float32 once.
 * The variational jitter is the MODEL's (state header [3]); min_variance and the retry settings come from `opt`.
 * h_m[i] / h_descs[i]: M and descriptor of model i (host).  d_feats f32[n_feat_rows, feat_dim]; d_rows i32 (rows may
 * repeat, any order).  d_status i32[n_models]: GAPRO_OK, the state's own status if its fit had failed (nothing is
 * written for that model), GAPRO_ERR_BAD_ARG (state of another M / D, or a row outside [0, n_feat_rows)),
 * GAPRO_ERR_CHOLESKY (nothing written), GAPRO_ERR_NOT_FINITE (a non-finite result).  A model never affects another, and
 * a row's result does not depend on which models or rows share the launch.  t = 0 is a no-op for that model.  The call
 * synchronises the stream once (descriptor upload), then only enqueues. */
int gapro_svgp_predict_batch(gapro_ctx* ctx, void* stream, int32_t n_models, int32_t feat_dim, const double* d_state,
                             const int32_t* h_m, const gapro_predict_desc* h_descs, const float* d_feats,
                             int64_t n_feat_rows, const int32_t* d_rows, const gapro_fit_options* opt,
                             void* d_workspace, size_t workspace_bytes, float* d_probs, float* d_probs_new,
                             uint8_t* d_labels, float* d_mu, float* d_var, int32_t* d_status);

/* ------------------------------------------------------------------------------------------
 * Point-level labels inside GP-labelled superpoints (csrc/point_refine.hip; no reference counterpart: the reference
 * labels whole superpoints, gen_ps_utils.py:438-480).  After the ordered merge a superpoint is REFINED iff a fit won it
 * (gapro_schedule_merge_ex: winner >= 0).  Every point of a refined superpoint is predicted from its own feature row by
 * the model that won the superpoint, and its own five values replace the broadcast ones:
 *   (p, p_new, label, mu, var) = gapro_svgp_predict_batch's result for that model at feats[i]   (float32 row, width D)
 *   box = label ? b2 : b1;  sem[i] = boxes_cls[box];  inst[i] = box, or -100 when box >= n_fg_instances;
 *   prob[i] = p_new;  mu[i] = mu;  var[i] = var.
 * Every other point keeps the broadcast values, mu[i] = mu_spp[spp_inv[i]], var[i] = var_spp[spp_inv[i]]: all five
 * outputs are point-length.  In this mode ("winner") the competition between several fits that tested one superpoint is
 * not re-run per point: the superpoint-level merge picks the model, and that model alone labels the points, between its
 * own two boxes.
 *
 * The "compete" mode re-runs it.  The refined set is the same (a superpoint with winner >= 0 is listed by no containment
 * event: a containment write sets probability 1, which no p_new <= 1 passes under the strict `<`, and a later one resets
 * the winner; so its history is fit events only and its probability starts at 0).  Every fit that TESTED the superpoint
 * (gapro_schedule_export_testers, event order) is evaluated at every point of it, and the merge is replayed for the
 * point alone: best = 0.0f; for k in order: if (best < p_new_k) take k   (strict, float32: the first maximum; a NaN never
 * wins).  The point's five values come from the fit that took it, by the rule above.  Containment- and fallback-labelled
 * superpoints are not refined in either mode, and the schedule stays static.
 *
 * The chain of a batch, on one stream: gapro_broadcast_labels_batch -> gapro_point_refine_gather -> ONE
 * gapro_svgp_predict_batch over the gathered rows (identity d_rows, out_offset == row_offset) -> gapro_point_refine_apply.
 * The launch's ROW TABLE holds the points of every refined superpoint of every scene: a superpoint's points form one
 * block of point_count[sp] rows, the blocks of one model's superpoints are contiguous, and the host plans the block
 * starts (sp_row) from the point counts gapro_partition_pool left.  Row indices are int32 (the predict ABI).
 * The chain of "compete": gapro_broadcast_labels_batch -> gapro_point_refine_gather (blocks in (scene, superpoint)
 * order) -> gapro_point_refine_expand -> ONE gapro_svgp_predict_batch over the gathered rows with the expanded d_rows
 * (a row is listed once per tester of its superpoint: R rows become R2 >= R) -> gapro_point_refine_apply with
 * n_models = 0 (the mu / var broadcast) -> gapro_point_refine_compete.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t n_points;
  int32_t n_spps;
  int32_t reserved;          /* 0 */
  const int32_t* spp_inv;    /* i32[N] */
  const float* feats;        /* f32[N,D]                                                   gather */
  const int64_t* sp_row;     /* i64[S] first row of the superpoint's block, -1 = not refined gather */
  int32_t* cursor;           /* i32[S] tmp: next free position of each block (zeroed by the call) gather */
  const float* mu_spp;       /* f32[S]                                                     apply */
  const float* var_spp;      /* f32[S]                                                     apply */
  int32_t* sem;              /* i32[N] in/out: the broadcast labels, refined in place       apply */
  int32_t* inst;             /* i32[N] in/out                                              apply */
  float* prob;               /* f32[N] in/out                                              apply */
  float* mu;                 /* f32[N] out                                                 apply */
  float* var;                /* f32[N] out                                                 apply */
} gapro_point_refine_scene;

/* One predict model of the launch as gapro_point_refine_apply needs it: its rows are [row_offset, row_offset + t) of the
 * row table and of the five predict outputs; (sem, inst) of a point labelled 0 (box b1) and 1 (box b2), prepared on the
 * host with the rule above. */
typedef struct {
  int64_t row_offset;
  int32_t t;
  int32_t scene;             /* index into the scenes of the call */
  int32_t sem1, inst1;
  int32_t sem2, inst2;
} gapro_point_refine_model;

/* One pass over the points of every scene (grid.y = scene): a point of a refined superpoint takes the next free position
 * of its superpoint's block, copies its feat_dim floats to d_row_feats f32[n_rows, feat_dim] and writes its scene-local
 * index to d_row_point i32[n_rows].  The ORDER of the points inside a block is not part of the contract (it follows the
 * order in which the atomics land); a predict row's result is its own, so the per-point outputs do not depend on it.
 * sp_row must give every refined superpoint a block of exactly its number of points inside [0, n_rows), blocks disjoint;
 * a position that would fall outside the table is dropped, never written.  h_scenes is copied to d_scenes (device,
 * n_scenes entries) on the stream and must stay valid until the stream has executed that copy.  n_scenes == 0 or
 * n_rows == 0: nothing is launched.  GAPRO_ERR_BAD_ARG: a null or negative argument, n_rows beyond 2^31 - 1 (refused
 * before anything is launched).  Enqueue only. */
int gapro_point_refine_gather(gapro_ctx* ctx, void* stream, int32_t n_scenes, int32_t feat_dim,
                              const gapro_point_refine_scene* h_scenes, gapro_point_refine_scene* d_scenes,
                              int64_t n_rows, float* d_row_feats, int32_t* d_row_point);
/* mu[i] = mu_spp[spp_inv[i]], var[i] = var_spp[spp_inv[i]] for every point of every scene; then, for every row r of every
 * model whose d_model_status is 0 (NULL = all), the five values of point d_row_point[r] of the model's scene from the
 * predict outputs at r.  sem / inst / prob must already hold the broadcast labels (same stream).  h_models is copied to
 * d_models on the stream like the scenes.  n_models == 0 (then the model and row arguments may be NULL) leaves the
 * broadcast; n_scenes == 0 is a no-op.  A row whose point index lies outside its scene is skipped.  Enqueue only. */
int gapro_point_refine_apply(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_point_refine_scene* h_scenes,
                             gapro_point_refine_scene* d_scenes, int32_t n_models,
                             const gapro_point_refine_model* h_models, gapro_point_refine_model* d_models,
                             int64_t n_rows, const int32_t* d_row_point, const float* d_probs_new,
                             const uint8_t* d_labels, const float* d_mu, const float* d_var,
                             const int32_t* d_model_status);

/* "compete": one refined superpoint = one BLOCK of gathered rows, tested by n_seg fits; one (tester, block) pair = one
 * SEGMENT of block.n_rows consecutive entries of the predict launch's d_rows and of its outputs. */
typedef struct {
  int64_t row_start;         /*  0  first gathered row of the block (sp_row of its superpoint) */
  int32_t n_rows;            /*  8  its number of points, > 0 */
  int32_t scene;             /* 12  index into the scenes of the call */
  int32_t seg_start;         /* 16  its segments are [seg_start, seg_start + n_seg), in tester (event) order */
  int32_t n_seg;             /* 20  >= 0 */
} gapro_point_refine_block;  /* 24 bytes */

typedef struct {
  int64_t out_start;         /*  0  entry j of the segment is d_rows[out_start + j] and output row out_start + j */
  int32_t model;             /*  8  index into the predict models of the launch */
  int32_t reserved;          /* 12  0 */
} gapro_point_refine_segment; /* 16 bytes */

/* d_rows[seg.out_start + j] = block.row_start + j for every segment of every block and j < block.n_rows: the row list of
 * the predict launch (d_rows i32[n_rows2]).  The segments of one model must be contiguous there for the model's
 * row_offset / out_offset / t to describe them; that is the planner's business, the call only checks bounds.  h_blocks
 * must be ascending in row_start and disjoint inside [0, n_rows); every segment must lie inside [0, n_rows2).  The host
 * arrays are copied to d_blocks / d_segs on the stream and must stay valid until the stream has executed the copies.
 * n_blocks == 0 or n_segs == 0: nothing is launched.  GAPRO_ERR_BAD_ARG: a null or negative argument, a block or
 * segment out of bounds, n_rows or n_rows2 beyond 2^31 - 1 (refused before anything is launched).  Enqueue only. */
int gapro_point_refine_expand(gapro_ctx* ctx, void* stream, int32_t n_blocks, const gapro_point_refine_block* h_blocks,
                              gapro_point_refine_block* d_blocks, int32_t n_segs,
                              const gapro_point_refine_segment* h_segs, gapro_point_refine_segment* d_segs,
                              int64_t n_rows, int64_t n_rows2, int32_t* d_rows);
/* The per-point merge.  For gathered row r = block.row_start + j of every block: best = 0.0f; the block's segments in
 * order, those of a model with non-zero d_model_status (NULL = all 0) skipped: p = d_probs_new[seg.out_start + j];
 * if (best < p) the segment takes the row.  The five values of point d_row_point[r] of the block's scene are then
 * written from the taking segment's output row and its model's (sem, inst) pair, as gapro_point_refine_apply does; a row
 * that no segment took, or whose point index lies outside its scene, is skipped (its point keeps what it holds: run
 * gapro_point_refine_apply with n_models = 0 before, on the same stream).  d_row_model i32[n_rows] (NULL = not wanted)
 * receives the model that took row r, -1 for a skipped row.  Of a gapro_point_refine_model only scene and the two pairs
 * are read.  Block and segment rules, copies and refusals as for gapro_point_refine_expand; every row is written by
 * exactly one lane (no atomics).  n_blocks == 0 or n_scenes == 0 is a no-op.  Enqueue only. */
int gapro_point_refine_compete(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_point_refine_scene* h_scenes,
                               gapro_point_refine_scene* d_scenes, int32_t n_models,
                               const gapro_point_refine_model* h_models, gapro_point_refine_model* d_models,
                               int32_t n_blocks, const gapro_point_refine_block* h_blocks,
                               gapro_point_refine_block* d_blocks, int32_t n_segs,
                               const gapro_point_refine_segment* h_segs, gapro_point_refine_segment* d_segs,
                               int64_t n_rows, int64_t n_rows2, const int32_t* d_row_point, const float* d_probs_new,
                               const uint8_t* d_labels, const float* d_mu, const float* d_var,
                               const int32_t* d_model_status, int32_t* d_row_model);

/* "vote": the chain of "compete" up to and including the predict launch, then a majority vote inside every block; the
 * result is written to the block's SUPERPOINT, and the ordinary gapro_broadcast_labels_batch runs behind it, so the
 * outputs keep the default path's lengths.  One workgroup per block:
 *   1. take   every gathered row of the block is taken by a segment exactly as in gapro_point_refine_compete (one device
 *             function).  A taken row VOTES for the box `label ? b2 : b1` of the taking model (h_model_boxes i32[2 *
 *             n_models] = b1, b2 of every model, >= 0); a row that no segment took votes for nobody.
 *   2. box    X = the box with the most votes, the lowest box index among equals (spp_align_label's first maximum over
 *             class = box + 1).  spp_major_voting's occupancy gate is vacuous here: a box whose fit tests a superpoint
 *             occupies it, so every candidate's gate is open.
 *   3. fit    f* = the segment that took the most voters for X, the earliest in tester order among equals.  Its voters
 *             for X carry one label, hence one sign convention for mu.
 *   4. values (sem, inst) = f*'s pair for that label (of a gapro_point_refine_model only scene and the pairs are read);
 *             prob = (sum of p_new over ALL voters for X) / block.n_rows (the winning class's term of spp_major_voting's
 *             sum: mean confidence x vote share); mu, var = the means over the voters for X that f* took.  Each of the
 *             three is an exact sum: k = fixed_point_shift(largest finite |value| of that quantity among the block's
 *             voting rows, each read at the output row that took it; block.n_rows), sum of rint(x 2^k) in int64,
 *             ldexp(sum, -k) / count in float64, rounded once to float32.  k is per block: a scene's result does not
 *             depend on what shares its batch, nor on the gather order.  A non-finite summand makes that one value the
 *             quiet NaN 0x7fc00000.
 *   5. none   a block in which nobody voted keeps what the five tables hold (the merge's values).
 * h_block_spp i32[n_blocks]: the scene-local superpoint of every block, inside [0, scene.n_spps); no two blocks may
 * share one.  d_block_out i32[3 * n_blocks] (NULL = not wanted): the model of f*, X and the votes for X; -1, -1, 0 for
 * rule 5.  Block and segment rules, copies and refusals as for gapro_point_refine_expand; also refused: a negative box,
 * a model whose two boxes are equal (both labels of its segments would argue for one box, two candidates where rule 3
 * counts the voters of one label, and the means of rule 4 would be taken over more rows than they are divided by),
 * a block of more than 2048 segments (the candidates' counters live in LDS).  Only thread 0 of a workgroup writes, to
 * its own block's entries.  n_blocks == 0 or n_scenes == 0 is a no-op.  Enqueue only. */
typedef struct {
  int32_t* sem_spp;          /* i32[S] in/out: the merge's tables, voted in place */
  int32_t* inst_spp;         /* i32[S] */
  float* prob_spp;           /* f32[S] */
  float* mu_spp;             /* f32[S] */
  float* var_spp;            /* f32[S] */
  int32_t n_spps;            /* S */
  int32_t reserved;          /* 0 */
} gapro_point_refine_vote_scene; /* 48 bytes */

int gapro_point_refine_vote(gapro_ctx* ctx, void* stream, int32_t n_scenes,
                            const gapro_point_refine_vote_scene* h_scenes, gapro_point_refine_vote_scene* d_scenes,
                            int32_t n_models, const gapro_point_refine_model* h_models,
                            gapro_point_refine_model* d_models, const int32_t* h_model_boxes, int32_t* d_model_boxes,
                            int32_t n_blocks, const gapro_point_refine_block* h_blocks,
                            gapro_point_refine_block* d_blocks, const int32_t* h_block_spp, int32_t* d_block_spp,
                            int32_t n_segs, const gapro_point_refine_segment* h_segs,
                            gapro_point_refine_segment* d_segs, int64_t n_rows, int64_t n_rows2,
                            const float* d_probs_new, const uint8_t* d_labels, const float* d_mu, const float* d_var,
                            const int32_t* d_model_status, int32_t* d_block_out);

/* ------------------------------------------------------------------------------------------
 * Superpoint vote of per-point labels (csrc/spp_vote.hip).  Replaces gen_ps_utils.py:99-129 spp_align_label
 * (GAPRO_VOTE_ALIGN) and :132-166 spp_major_voting (GAPRO_VOTE_MAJOR).
 *   d_ids i32[N] dense rank of each point's superpoint (gapro_partition_prepare's spp_inv, or the inverse of a sorted
 *   unique), S = the exact number of ranks: every s in [0, S) must own a point (a superpoint without one gets label 0
 *   and probability 0, which nothing gathers);
 *   d_label i32[N] or i64[N] (label_is_i64) in [0, C): 0 = background, c >= 1 = box c - 1;  d_prob f32[N].
 * cnt[s, c] = points of s labelled c (int32 atomics), n[s] = sum_c cnt[s, c].  Masked count m[s, 0] = cnt[s, 0] and, for
 * c >= 1, m[s, c] = cnt[s, c] where the gate of (s, c - 1) is open, else 0.  The gate:
 *   ALIGN  d_gate u8[C - 1, S] (the reference's bb_occupancy_spp, non-zero = open); NULL = every gate open;
 *   MAJOR  d_gate u8[N, C - 1] (bb_occupancy): open when every point of s lies in box c - 1, i.e. the integer count of
 *          non-zero entries over s equals n[s] (the reference's scatter(mean) == 1 for 0 / 1 inputs).
 * label_spp[s] = the first maximum of m[s, .] over ascending c (torch.argmax; an all-masked row gives 0);
 * d_label_out i64[N] = label_spp[ids].  With d_prob (ALIGN: optional, d_prob_out NULL with it; MAJOR: required),
 * P[s, c] = the exact sum of prob over the points of s labelled c: rint(x 2^k) in int64, k = fixed_point_shift(max
 * |prob|, N).  d_prob_out f32[N] = prob_spp[ids] with
 *   ALIGN  prob_spp[s] = ldexp(sum_c P[s, c], -k) / n[s] in float64, rounded once to float32;
 *   MAJOR  prob_spp[s] = sum_c (P[s, c] / (cnt[s, c] + 1e-4)) * (m[s, c] / n[s]), float64, c ascending, every operation
 *          rounded on its own (no contraction), the result rounded once to float32.
 * The reference sums probabilities in float32 in scatter order, and its :141-143 indexes the occupancy scatter with the
 * raw superpoint ids (it only runs on dense ids); the exact sums and the ranks replace both.  The entry point takes
 * ranks; the Python functions rank ids of ANY range (sorted unique on the device), not only those the partition's
 * flag table holds.
 * d_status i32[1]: GAPRO_OK; GAPRO_ERR_BAD_ARG (an id outside [0, S), a label outside [0, C), MAJOR: a probability
 * outside [0, 1], which the reference asserts against at :154); GAPRO_ERR_NOT_FINITE (a non-finite probability; it wins
 * over BAD_ARG).  With a non-zero status nothing is written to the outputs.  Refused before anything is launched
 * (GAPRO_ERR_BAD_ARG): a null or non-positive argument, S > N, S * C > 2^31 - 1; GAPRO_ERR_WORKSPACE: d_ws smaller
 * than gapro_spp_vote_workspace_bytes (0 for sizes the call would refuse).  Enqueue only.
 * ---------------------------------------------------------------------------------------- */
enum { GAPRO_VOTE_ALIGN = 0, GAPRO_VOTE_MAJOR = 1 };
size_t gapro_spp_vote_workspace_bytes(int64_t n_points, int32_t n_spps, int32_t n_classes);
int gapro_spp_vote(gapro_ctx* ctx, void* stream, int32_t mode, int64_t n_points, int32_t n_spps, int32_t n_classes,
                   const int32_t* d_ids, const void* d_label, int32_t label_is_i64, const float* d_prob,
                   const uint8_t* d_gate, void* d_ws, size_t ws_bytes, int64_t* d_label_out, float* d_prob_out,
                   int32_t* d_status);

/* ------------------------------------------------------------------------------------------
 * Instance-label preparation of the consumer's training step (csrc/inst_prep.hip).  Replaces ISBNet's
 * get_cropped_instance_label (isbnet/model/model_utils.py:589-597; gapro/gen_ps_utils.py:64-72 is the same function)
 * and get_instance_info (model_utils.py:519-555), which loop over the instance ids on the host.
 *   d_instance_label, d_semantic_label: GAPRO_LABEL_F64 / _I32 / _I64 arrays of n_points entries; a label < 0 (or NaN)
 *   names no instance.  d_coords f32[N,3].
 * Crop: P = the distinct ids >= 0, K = |P|.  Ids of P below K stay; the holes h_0 < h_1 < .. of [0, K) take the ids of P
 * that are >= K in descending order (the largest goes to h_0).  Negative labels are untouched; without an id >= 0 nothing
 * changes.  This closed form equals the reference's loop.
 * Info, per instance id r in [0, I), I = max id + 1:
 *   d_instance_cls i64[r]      semantic label of the instance's first point (lowest index), minus label_shift unless -100
 *   d_instance_box f32[r,6]    [min xyz | max xyz] (-0.0 orders below +0.0)
 *   d_instance_pointnum i32[r] its points
 *   d_centroid_offset f32[N,3] centroid - p with one float32 subtraction; centroid = the exact mean: int64 sums of
 *                              rint(x 2^k), k = fixed_point_shift(largest |coordinate| of the labelled points, N), then
 *                              ldexp(sum, -k) / count in float64, rounded once to float32 (the reference's float32 mean
 *                              has no stated order: DESIGN.md 4.7)
 *   d_corners_offset f32[N,6]  (min - p | max - p), one float32 subtraction per component
 *   rows of points without an instance are -100.  The per-instance outputs hold max_ids rows.
 * gapro_inst_prepare = the crop (in place) followed by the info on the cropped labels, in one chain: I = K.
 * The header (device + page-locked host copy when h_header_pinned is given) carries the result of the call:
 *   GAPRO_ERR_BAD_ARG     an id >= GAPRO_INST_PREP_MAX_IDS or a float64 label that is no integer; info / prepare:
 *                         no id >= 0 (the reference fails on torch.stack([])); info: an empty id below the largest (the
 *                         reference fails on min of an empty tensor)
 *   GAPRO_ERR_WORKSPACE   an id >= max_ids: run again with max_ids > header.max_id
 *   GAPRO_ERR_NOT_FINITE  info / prepare: a non-finite coordinate on a point with an id >= 0 (one without is ignored)
 * BAD_ARG wins over WORKSPACE, which wins over NOT_FINITE.  With a non-zero status neither the labels nor the outputs
 * are written.  Refused before anything is launched (GAPRO_ERR_BAD_ARG): a null or non-positive argument, an unknown
 * label type, max_ids outside [1, GAPRO_INST_PREP_MAX_IDS]; GAPRO_ERR_WORKSPACE: a workspace smaller than
 * gapro_inst_prep_workspace_bytes (0 for a max_ids the calls refuse).  Enqueue only; the results are the same bits for
 * every run.  The passes over the points run at most GAPRO_INST_PREP_GRID_CAP workgroups of 256 threads; new ids below
 * GAPRO_INST_PREP_LDS_IDS are tallied in LDS.
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_INST_PREP_MAX_IDS 1048576 /* 2^20 */
#define GAPRO_INST_PREP_GRID_CAP 512
#define GAPRO_INST_PREP_LDS_IDS 512
typedef struct {
  int32_t instance_num; /* I: crop / prepare: K; info: max id + 1 */
  int32_t n_ids;        /* K distinct ids >= 0 */
  int32_t max_id;       /* largest id met, clamped to GAPRO_INST_PREP_MAX_IDS; -1 without one */
  int32_t status;
  int32_t fixed_shift;  /* k of the centroid sums */
  int32_t flags;        /* 1: non-finite coordinate, 2: id beyond the bound or not an integer, 4: id >= max_ids */
} gapro_inst_prep_header; /* 24 bytes */

size_t gapro_inst_prep_workspace_bytes(int32_t max_ids);
int gapro_inst_crop(gapro_ctx* ctx, void* stream, int64_t n_points, void* d_instance_label, int32_t label_type,
                    int32_t max_ids, void* d_workspace, size_t workspace_bytes, gapro_inst_prep_header* d_header,
                    gapro_inst_prep_header* h_header_pinned);
int gapro_inst_info(gapro_ctx* ctx, void* stream, int64_t n_points, const float* d_coords,
                    const void* d_instance_label, int32_t label_type, const void* d_semantic_label, int32_t semantic_type,
                    int64_t label_shift, int32_t max_ids, void* d_workspace, size_t workspace_bytes,
                    int64_t* d_instance_cls, float* d_instance_box, int32_t* d_instance_pointnum,
                    float* d_centroid_offset, float* d_corners_offset, gapro_inst_prep_header* d_header,
                    gapro_inst_prep_header* h_header_pinned);
int gapro_inst_prepare(gapro_ctx* ctx, void* stream, int64_t n_points, const float* d_coords, void* d_instance_label,
                       int32_t label_type, const void* d_semantic_label, int32_t semantic_type, int64_t label_shift,
                       int32_t max_ids, void* d_workspace, size_t workspace_bytes, int64_t* d_instance_cls,
                       float* d_instance_box, int32_t* d_instance_pointnum, float* d_centroid_offset,
                       float* d_corners_offset, gapro_inst_prep_header* d_header,
                       gapro_inst_prep_header* h_header_pinned);

/* ------------------------------------------------------------------------------------------
 * Ground-truth instance masks per batch sample of the consumer's training step (csrc/spp_gt.hip).  Replaces ISBNet's
 * get_spp_gt (isbnet/model/model_utils.py:692-738) and get_subsample_gt (:647-689), which loop over the samples and,
 * on the host, over a device tensor of instance ids.  Two calls with one host read between them: gapro_spp_gt_count
 * reports how many rows and columns every sample has, the caller allocates, gapro_spp_gt_fill writes.
 *   d_labels        GAPRO_LABEL_F64 / _I32 / _I64 [n_labels]: the instance id of a point, or ignore_label
 *   d_gather        i64[n_points] or NULL.  Point p of the call reads its label (and superpoint) at d_gather[p]; NULL:
 *                   at p, and n_labels == n_points
 *   d_spps          i32 (spp_is_i64 == 0) or i64 [n_labels] superpoint ids in [0, n_spps), or NULL with n_spps == 0:
 *                   every point is its own column
 *   d_instance_cls  GAPRO_LABEL_F64 / _I32 / _I64 [n_cls]: the class of every instance id
 *   d_offsets       i64[batch_size + 1]: sample b holds the points [d_offsets[b], d_offsets[b + 1]); points before the
 *                   first and after the last offset belong to no sample and are not read at all
 * Per sample b:
 *   rows     the distinct labels of its points, ascending, that differ from ignore_label and whose class is >= 0
 *   columns  the distinct superpoint ids of its points, ascending (the same id may occur in two samples); without
 *            d_spps its points in their order
 *   mask     f32[rows, columns], row-major.  c(i, s) = points of column s labelled i, n(s) = all points of column s,
 *            ignored ones included:  mask = 1.0f where 2 c >= n (GAPRO_SPP_GT_HALF) or 2 c > n (GAPRO_SPP_GT_STRICT),
 *            else 0.0f.  For n(s) < 2^24 the first is the reference's float32 scatter_mean(label == i) >= 0.5 to the
 *            bit (two integers below 2^24 are exact in float32 and their correctly rounded quotient cannot reach or
 *            cross 0.5 from the other side); beyond, the integer rule is the definition.  Without d_spps n = 1 and
 *            the mask is (label == i).
 * gapro_spp_gt_count writes d_header (and its page-locked host copy when h_header_pinned is given): the struct below
 * followed by batch_size pairs {int32 n_inst_gt, int32 n_spp}, GAPRO_SPP_GT_HEADER_BYTES(batch_size) in all.  It leaves
 * the presence bit-words, their prefix popcounts (rank of an id = prefix of its word + set bits below it) and the packed
 * offsets in the workspace, which gapro_spp_gt_fill reads: same inputs, same workspace, nothing in between.
 * gapro_spp_gt_fill writes, packed sample after sample,
 *   d_mask f32[total_cells]   the masks; during the call the buffer holds the counts c as uint32
 *   d_cls  [total_rows]       d_instance_cls[id] of every row, in cls_type (NULL = not wanted)
 *   d_box  f32[total_rows, 6] d_instance_box[id] (f32[n_cls, 6]), bit copies (both NULL = not wanted)
 *   d_ids  i64[total_rows]    the id of every row (NULL = not wanted)
 * mask_cells / n_rows are the lengths the caller allocated; smaller ones than the header's totals: GAPRO_ERR_WORKSPACE
 * in d_header->status (when given), nothing written.
 * Refusals of the data, header.status of gapro_spp_gt_count; flags names every cause met, bad_sample the lowest sample
 * of the winning one.  In this order of precedence:
 *   GAPRO_ERR_BAD_ARG    flags & 1: offsets that decrease or leave [0, n_points] (bad_sample = the first such b; the
 *                        points are not looked at)
 *   GAPRO_ERR_BAD_ARG    flags & 2: a d_gather entry outside [0, n_labels)
 *   GAPRO_ERR_BAD_ARG    flags & 4: a label that is not ignore_label and is negative, >= n_cls, or (float64) no integer
 *   GAPRO_ERR_SPP_RANGE  flags & 8: a superpoint id outside [0, n_spps)
 * With a non-zero status gapro_spp_gt_fill writes nothing.  Refused before anything is launched (GAPRO_ERR_BAD_ARG): a
 * null or non-positive argument, an unknown type code or rule, d_spps without n_spps or the reverse, d_gather == NULL
 * with n_labels != n_points, n_points or n_labels > 2^31 - 1, batch_size > GAPRO_SPP_GT_MAX_SAMPLES, n_cls >
 * GAPRO_INST_PREP_MAX_IDS, batch_size * n_spps > GAPRO_SPP_GT_MAX_BATCH_SPPS, d_box without d_instance_box;
 * GAPRO_ERR_WORKSPACE: a workspace smaller than gapro_spp_gt_workspace_bytes (0 for sizes the calls refuse).  Both calls
 * only enqueue; integer atomics only, so the results are the same bits for every run.  The passes over the points run at
 * most GAPRO_SPP_GT_GRID_CAP workgroups of 256 threads.
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_SPP_GT_MAX_SAMPLES 1024
#define GAPRO_SPP_GT_MAX_BATCH_SPPS 2147483647 /* 2^31 - 1 */
#define GAPRO_SPP_GT_GRID_CAP 512
enum { GAPRO_SPP_GT_HALF = 0, GAPRO_SPP_GT_STRICT = 1 };
typedef struct {
  int32_t status;
  int32_t bad_sample;   /* lowest sample of the winning refusal; -1 without one */
  int32_t flags;        /* 1: offsets, 2: gather index, 4: label, 8: superpoint id */
  int32_t batch_size;
  int64_t total_rows;   /* sum of n_inst_gt */
  int64_t total_cols;   /* sum of n_spp */
  int64_t total_cells;  /* sum of n_inst_gt * n_spp */
} gapro_spp_gt_header; /* 40 bytes; batch_size x {int32_t n_inst_gt, n_spp} follow */
#define GAPRO_SPP_GT_HEADER_BYTES(batch_size) (40 + 8 * (size_t)(batch_size))

size_t gapro_spp_gt_workspace_bytes(int64_t n_points, int32_t batch_size, int32_t n_cls, int32_t n_spps);
int gapro_spp_gt_count(gapro_ctx* ctx, void* stream, int64_t n_points, int64_t n_labels, const void* d_labels,
                       int32_t label_type, const int64_t* d_gather, const void* d_spps, int32_t spp_is_i64,
                       int32_t n_spps, const void* d_instance_cls, int32_t cls_type, int32_t n_cls,
                       const int64_t* d_offsets, int32_t batch_size, int64_t ignore_label, void* d_workspace,
                       size_t workspace_bytes, gapro_spp_gt_header* d_header, gapro_spp_gt_header* h_header_pinned);
int gapro_spp_gt_fill(gapro_ctx* ctx, void* stream, int64_t n_points, int64_t n_labels, const void* d_labels,
                      int32_t label_type, const int64_t* d_gather, const void* d_spps, int32_t spp_is_i64,
                      int32_t n_spps, const void* d_instance_cls, int32_t cls_type, int32_t n_cls,
                      const float* d_instance_box, const int64_t* d_offsets, int32_t batch_size, int64_t ignore_label,
                      int32_t rule, void* d_workspace, size_t workspace_bytes, float* d_mask, int64_t mask_cells,
                      void* d_cls, float* d_box, int64_t* d_ids, int64_t n_rows, gapro_spp_gt_header* d_header);

/* ------------------------------------------------------------------------------------------
 * Predicted instances: the consumer's inference post-processing (csrc/proposals.hip).  Replaces ISBNet.get_instance
 * (isbnet/model/isbnet.py:887-1005) with the nms it calls (model_utils.py:77-169), custom_scatter_mean (:600-613),
 * superpoint_align (:447-470) and rle_encode_gpu_batch (isbnet/util/rle.py:47-69): float products of bit masks, a host
 * loop per surviving proposal and a blocking copy per instance.  Two calls with one host read between them, as
 * gapro_spp_gt_*: gapro_proposals_count runs stages 1-6 and counts the runs, the caller allocates, gapro_proposals_fill
 * writes.  One scene a call.
 * gapro_proposals_inputs (GAPRO_PROPOSALS_FULL; Q = n_queries, C = instance_classes, V = n_voxels, N = n_points):
 *   cls_logits f32[Q, C + 1], conf_logits f32[Q], box_preds f32[Q, 6] (NULL: the boxes are zeros)
 *   mask_logits     f32[Q, V] with n_mask_cols == 0, or f32[Q, n_mask_cols] with voxel_spps i32 / i64 [V] in
 *                   [0, n_mask_cols): bit (q, v) reads column voxel_spps[v] (what the reference expands at isbnet.py:610)
 *   v2p_map         i32 / i64 [N] in [0, V);  spps i32 / i64 [N] in [0, n_spps)
 *   semantic_preds  i32 / i64 [V], with n_sem2ins > 0 only
 *   the *_i64 members say which of the two integer types a pointer has
 * Stages.  Every floating-point term is evaluated in float64 from the float32 inputs and rounded to float32 once, where
 * the stage says so; everything else is integer.
 *   1 scores      score[q, c] = float32(sqrt(softmax(cls_logits[q, :])[c] * clamp(conf[q], 0, 1))), c < C; the softmax is
 *                 exp(x - max) over the sum of these terms in ascending c.  The candidates are the min(pre_topk, Q C)
 *                 largest by float32 value, descending; equal values by ascending flat index q C + c (this tie rule is
 *                 the library's own: the reference's torch.topk has none).
 *   2 mask bits   bit (q, v) = mask_logits >= logit_thresh, a float32 comparison; 64-bit words along v (the ballot of a
 *                 wavefront that loaded 64 consecutive values), the bits beyond V zero; npoints[q] = the row's popcount.
 *                 A candidate stays if npoints >= npoint_thresh; the order is kept.
 *   3 inter       inter[a, b] = sum_w popcount(A_w & B_w), exact, no atomics; iou = float32(inter) / float32(n_a + n_b -
 *                 inter), one float32 division.  For V < 2^24 this is the reference's float32 einsum and division to the
 *                 bit; beyond, the integer form is the definition.
 *   4 nms         MATRIX: d_ij = iou_ij for i < j of one class, else 0; c_i = max_k d_ki; coef_j = min_i exp(-2 d_ij^2) /
 *                 exp(-2 c_i^2); new_j = float32(score_j coef_j), float64 inside.  Kept: the min(topk, n) largest new
 *                 (ties: the earlier sorted position), or with topk == -1 those with new >= final_score_thresh (float32);
 *                 written in descending new, ties by position.  STANDARD: the reference's greedy loop: a kept pivot
 *                 removes every later candidate of its class with iou > nms_threshold (float32, the stage-3 value);
 *                 scores and order unchanged.  One workgroup, a suppressed bitmap in LDS, no host.
 *   5 refine      c(k, s) = points p with spps[p] == s whose voxel v2p_map[p] has bit k; n(s) = points of s;
 *                 m(k, p) = [2 c(k, spps[p]) >= n(spps[p])] -- the GAPRO_SPP_GT_HALF rule, equal to the reference's
 *                 float32 scatter_mean >= 0.5 by the proof given there.  A row stays if sum_p m(k, p) >= npoint_thresh.
 *   6 sem2ins     for each i of sem2ins_classes a row whose voxel bits are semantic_preds[v] == i, through stage 5's rule,
 *                 with no NMS and no point count.  These rows come first: conf 1.0, label_id i + 1, query -1, a zero box.
 *                 The reference's case "every spps entry is ignore_label" is not built: such ids are refused.
 *   7 runs        per row the transitions of m(k, .) with a zero before and after: 1-based starts, each followed by its
 *                 length, int64: the `counts` of rle_encode_gpu_batch, byte for byte.
 * label_id of an ordinary row = class + label_shift (1 for scannetv2, 3 for s3dis).
 * GAPRO_PROPOSALS_NMS: stages 3-4 alone for a caller that holds masks (the reference's `nms`): mask_logits is u8[Q, V]
 * (GAPRO_PROPOSALS_MASK_U8, bit = non-zero) or f32[Q, V], Q <= GAPRO_PROPOSALS_MAX_PRE_TOPK; cand_scores f32[Q] and
 * cand_classes i32[Q] replace stage 1: every row is a candidate, sorted by (score descending, row ascending); no
 * npoints filter; an empty union has iou 0.  The rows out name their masks by `query`; no runs.
 * GAPRO_PROPOSALS_RLE: stage 7 alone: mask_logits is u8[Q, N], Q <= GAPRO_PROPOSALS_MAX_PRE_TOPK +
 * GAPRO_PROPOSALS_MAX_SEM2INS; every row is kept.
 * gapro_proposals_count writes d_header (and its page-locked host copy when h_header_pinned is given): the struct below
 * followed by int32 n_runs of every row out; gapro_proposals_header_bytes(...) in all, sized for the most rows the call
 * can give (pre_topk, or topk where matrix NMS cuts to it, plus n_sem2ins).  gapro_proposals_fill reads what the count left in the workspace -- same inputs, nothing in between -- and
 * writes (NULL = not wanted)
 *   d_conf f32[n_rows], d_label_id i32[n_rows], d_box f32[n_rows, 6] (bit copies of box_preds), d_query i32[n_rows]
 *   d_run_offsets i64[n_rows + 1] in runs; d_runs i64[2 total_runs]: row r owns d_runs[2 off[r], 2 off[r + 1])
 *   d_masks u8[n_rows, N]: m(k, .), on request
 * cap_rows / cap_runs are the lengths the caller allocated; smaller ones than the header's: GAPRO_ERR_WORKSPACE in
 * d_header->status (when given), nothing written.
 * Refusals of the data, header.status of gapro_proposals_count; flags names every cause met.  In this order of
 * precedence:
 *   GAPRO_ERR_NOT_FINITE  flags & 1: a non-finite cls_logits or conf_logits entry (every score takes part in stage 1), or
 *                         cand_scores entry
 *   GAPRO_ERR_NOT_FINITE  flags & 2: a non-finite mask_logits entry read for the row of a stage-1 candidate
 *   GAPRO_ERR_BAD_ARG     flags & 4: a v2p_map entry outside [0, V)
 *   GAPRO_ERR_BAD_ARG     flags & 8: a voxel_spps entry outside [0, n_mask_cols)
 *   GAPRO_ERR_SPP_RANGE   flags & 16: a spps id outside [0, n_spps)
 * With a non-zero status n_rows is 0 and gapro_proposals_fill writes nothing.  Refused before anything is launched
 * (GAPRO_ERR_BAD_ARG): a null or non-positive argument, npoint_thresh < 1, pre_topk outside [1,
 * GAPRO_PROPOSALS_MAX_PRE_TOPK], Q C > 2^20, V or N > 2^31 - 1, an unknown mode, NMS type or mask type, topk < -1,
 * n_sem2ins outside [0, GAPRO_PROPOSALS_MAX_SEM2INS], a threshold that is not finite, (pre_topk + n_sem2ins) n_spps >
 * 2^31 - 1; GAPRO_ERR_WORKSPACE: a workspace smaller than gapro_proposals_workspace_bytes (0 for sizes the calls
 * refuse).  The two structs are host memory, read while the call enqueues.  Both calls only enqueue: a scene costs one
 * host read.  Integer atomics only, so the results are the same bits for every run.  The passes over the scores, voxels,
 * points and pairs run at most GAPRO_PROPOSALS_GRID_CAP workgroups of 256 threads; the passes per row (stages 5 and 7)
 * at most 1024 workgroups a row, one per chunk of at least 1024 points.
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_PROPOSALS_MAX_PRE_TOPK 1024
#define GAPRO_PROPOSALS_MAX_SEM2INS 8
#define GAPRO_PROPOSALS_GRID_CAP 2048
enum { GAPRO_PROPOSALS_FULL = 0, GAPRO_PROPOSALS_NMS = 1, GAPRO_PROPOSALS_RLE = 2 };
enum { GAPRO_PROPOSALS_NMS_MATRIX = 0, GAPRO_PROPOSALS_NMS_STANDARD = 1 };
enum { GAPRO_PROPOSALS_MASK_F32 = 0, GAPRO_PROPOSALS_MASK_U8 = 1 };
typedef struct {
  int64_t n_queries, n_voxels, n_points;
  int32_t n_spps;
  int32_t n_mask_cols;      /* 0: mask_logits has a column per voxel */
  const float* cls_logits;
  const float* conf_logits;
  const float* box_preds;
  const void* mask_logits;
  const void* voxel_spps;
  const void* v2p_map;
  const void* spps;
  const void* semantic_preds;
  const float* cand_scores;     /* GAPRO_PROPOSALS_NMS */
  const int32_t* cand_classes;  /* GAPRO_PROPOSALS_NMS */
  int32_t mask_type;
  int32_t voxel_spps_i64, v2p_i64, spps_i64, semantic_i64;
  int32_t reserved;
} gapro_proposals_inputs; /* 136 bytes */
typedef struct {
  int32_t mode;
  int32_t instance_classes;
  int32_t pre_topk;         /* 300 in the reference */
  int32_t type_nms;
  int32_t topk;             /* -1: none */
  int32_t npoint_thresh;
  int32_t label_shift;
  int32_t n_sem2ins;
  float logit_thresh;
  float final_score_thresh; /* 0.1 in the reference */
  float nms_threshold;
  int32_t reserved;
  int32_t sem2ins_classes[GAPRO_PROPOSALS_MAX_SEM2INS];
} gapro_proposals_params; /* 80 bytes */
typedef struct {
  int32_t status;
  int32_t flags;            /* 1: score input, 2: mask value, 4: v2p_map, 8: voxel_spps, 16: spps */
  int32_t n_rows;
  int32_t n_sem2ins;        /* the first rows */
  int64_t total_runs;
  int32_t n_candidates;     /* after stage 1 */
  int32_t n_after_npoints;  /* after stage 2 */
  int32_t n_after_nms;      /* after stage 4 */
  int32_t n_after_refine;   /* after stage 5 */
} gapro_proposals_header; /* 40 bytes; n_rows x int32_t n_runs follow */
#define GAPRO_PROPOSALS_HEADER_BYTES(max_rows) (40 + 4 * (size_t)(max_rows))

size_t gapro_proposals_workspace_bytes(const gapro_proposals_inputs* in, const gapro_proposals_params* params);
size_t gapro_proposals_header_bytes(const gapro_proposals_inputs* in, const gapro_proposals_params* params);
int gapro_proposals_count(gapro_ctx* ctx, void* stream, const gapro_proposals_inputs* in,
                          const gapro_proposals_params* params, void* d_workspace, size_t workspace_bytes,
                          gapro_proposals_header* d_header, gapro_proposals_header* h_header_pinned);
int gapro_proposals_fill(gapro_ctx* ctx, void* stream, const gapro_proposals_inputs* in,
                         const gapro_proposals_params* params, void* d_workspace, size_t workspace_bytes, float* d_conf,
                         int32_t* d_label_id, float* d_box, int32_t* d_query, int64_t cap_rows, int64_t* d_run_offsets,
                         int64_t* d_runs, int64_t cap_runs, uint8_t* d_masks, gapro_proposals_header* d_header);

/* ------------------------------------------------------------------------------------------
 * SPFormer's predicted instances: the second consumer's inference post-processing (csrc/spf_predict.hip).  Replaces
 * SPFormer.predict_by_feat (SPFormer/spformer/model/spformer.py:180-242) with the rle_encode_gpu_batch it calls: a
 * [K, N] int32 expansion of the superpoint masks, three boolean compactions of it, and per instance a nonzero, a boolean
 * gather of the coordinates and two blocking copies.  Two calls with one host read between them, as gapro_proposals_*.
 * One scene a call.  Q = n_queries, C = num_class, S = n_spps (the columns of the mask logits), N = n_points,
 * K = min(topk_insts, Q C).
 * gapro_spf_predict_inputs:
 *   labels f32[Q, C + 1], pred_scores f32[Q] (the raw linear output: it may be negative), masks f32[Q, S]
 *   superpoints i32 / i64 [N] in [0, S) (superpoints_i64 says which), coords_float f32[N, 3]
 * Steps.  Every floating-point term is evaluated in float64 from the float32 inputs and rounded to float32 once;
 * everything else is integer or a bit copy (the rule of "Predicted instances" above).
 *   1 scores   s[q, c] = float32(softmax(labels[q, :])[c] * pred_scores[q]), c < C; the softmax runs over all C + 1
 *              columns as exp(x - max) over the sum of these terms in ascending c; the last column is dropped and the
 *              rest are not renormalised.  A -0.0 is stored as +0.0.  The candidates are the K largest s by float32
 *              value, descending; equal values by ascending flat index q C + c (the tie rule, radix select and sort of
 *              "Predicted instances" stage 1; the reference's torch.topk(sorted=False) has no rule).
 *   2 bits     bit (q, j) = masks[q, j] > 0, a strict float32 comparison: a logit of +0.0 or -0.0 is not set.  64 bits
 *              to a word by the ballot of a wavefront that loaded 64 consecutive values; the tail of the last word is
 *              zero.  For a candidate's row: cnt = the set bits, sum = the float64 sum of 1 / (1 + exp(-x)) over the set
 *              entries, in an order the kernel fixes (a lane adds its words in ascending order, the 64 lanes fold by the
 *              xor butterfly 32 .. 1, the four waves add in ascending order), so two runs give the same bytes.
 *              conf = float32(softmax64 * pred_scores * sum / (cnt + 1e-6)), one float64 expression rounded once (the
 *              softmax term as in step 1, before its rounding); cnt = 0 gives conf = 0; a -0.0 is stored as +0.0.
 *   3 tables   per superpoint j, once a call: n(j) = its points; lo(j), hi(j) = the component-wise min and max of
 *              coords_float over them.  Integer atomics only: the float min / max go through the order-preserving
 *              integer image of the float32 bits (sign set: all bits flipped; else the sign bit set), so -0.0 < +0.0.
 *   4 rows     for candidate k with query q_k: npoints[k] = sum_j bit(q_k, j) n(j), int64; box[k] = the min of lo(j) and
 *              the max of hi(j) over the set j with n(j) > 0.  A row is kept if conf > score_thr (float32, strict) and
 *              then npoints > npoint_thr (strict).  No [K, N] array exists.
 *   5 order    the kept rows in descending conf; equal values in candidate order.  (The reference's own order is whatever
 *              torch.topk(sorted=False) returned.)
 *   6 runs     per kept row the transitions of m(k, p) = bit(q_k, superpoints[p]) along p with a zero before and after:
 *              1-based starts, each followed by its length, int64: the `counts` of rle_encode_gpu_batch, byte for byte.
 * gapro_spf_predict_count runs all of it up to the run counts and writes d_header (and its page-locked host copy when
 * h_header_pinned is given): the struct below followed by int32 n_runs of every row out,
 * gapro_spf_predict_header_bytes(...) in all, sized for K rows.  gapro_spf_predict_fill reads what the count left in the
 * workspace -- same inputs, nothing in between -- and writes (NULL = not wanted, but for d_run_offsets)
 *   d_conf f32[n_rows], d_label_id i32[n_rows] = c + 1, d_box f32[n_rows, 6] (min xyz, max xyz), d_query i32[n_rows]
 *   d_run_offsets i64[n_rows + 1] in runs; d_runs i64[2 total_runs]: row r owns d_runs[2 off[r], 2 off[r + 1])
 *   d_masks u8[n_rows, N]: m(k, .), on request
 * cap_rows / cap_runs are the lengths the caller allocated; smaller ones than the header's: GAPRO_ERR_WORKSPACE in
 * d_header->status (when given), nothing written.
 * Refusals of the data, header.status of gapro_spf_predict_count; flags names every cause met.  In this order of
 * precedence:
 *   GAPRO_ERR_NOT_FINITE  flags & 1: a non-finite labels or pred_scores entry (every score takes part in step 1)
 *   GAPRO_ERR_NOT_FINITE  flags & 2: a non-finite masks entry in the row of a candidate
 *   GAPRO_ERR_NOT_FINITE  flags & 4: a non-finite coords_float entry
 *   GAPRO_ERR_SPP_RANGE   flags & 8: a superpoints id outside [0, S)
 * With a non-zero status the stage counts and n_rows are 0 and gapro_spf_predict_fill writes nothing.  Refused before
 * anything is launched (GAPRO_ERR_BAD_ARG): a null or non-positive argument, topk_insts outside [1,
 * GAPRO_PROPOSALS_MAX_PRE_TOPK], Q C > 2^20, S or N > 2^31 - 1, npoint_thr < 0 (so that a kept row always has a point
 * and a box), a score_thr that is not finite; GAPRO_ERR_WORKSPACE: a workspace smaller than
 * gapro_spf_predict_workspace_bytes (0 for sizes the calls refuse).  The two structs are host memory, read while the
 * call enqueues.  Both calls only enqueue: a scene costs one host read.  The passes over the queries and points run at
 * most GAPRO_PROPOSALS_GRID_CAP workgroups of 256 threads, step 2 and 4 a workgroup per candidate, step 6 at most 1024
 * workgroups a row, one per chunk of at least 1024 points.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t n_queries, n_spps, n_points;
  const float* labels;
  const float* pred_scores;
  const float* masks;
  const void* superpoints;
  const float* coords_float;
  int32_t superpoints_i64;
  int32_t reserved;
} gapro_spf_predict_inputs; /* 72 bytes */
typedef struct {
  int32_t num_class;
  int32_t topk_insts;       /* 100 in the released configuration */
  int32_t npoint_thr;       /* 100 */
  float score_thr;          /* 0.0 */
} gapro_spf_predict_params; /* 16 bytes */
typedef struct {
  int32_t status;
  int32_t flags;            /* 1: labels / pred_scores, 2: mask value, 4: coords_float, 8: superpoints */
  int32_t n_candidates;     /* after step 1 */
  int32_t n_after_score;    /* rows with conf > score_thr */
  int32_t n_rows;           /* of them, rows with npoints > npoint_thr */
  int32_t reserved;
  int64_t total_runs;
} gapro_spf_predict_header; /* 32 bytes; n_rows x int32_t n_runs follow */
#define GAPRO_SPF_PREDICT_HEADER_BYTES(max_rows) (32 + 4 * (size_t)(max_rows))

size_t gapro_spf_predict_workspace_bytes(const gapro_spf_predict_inputs* in, const gapro_spf_predict_params* params);
size_t gapro_spf_predict_header_bytes(const gapro_spf_predict_inputs* in, const gapro_spf_predict_params* params);
int gapro_spf_predict_count(gapro_ctx* ctx, void* stream, const gapro_spf_predict_inputs* in,
                            const gapro_spf_predict_params* params, void* d_workspace, size_t workspace_bytes,
                            gapro_spf_predict_header* d_header, gapro_spf_predict_header* h_header_pinned);
int gapro_spf_predict_fill(gapro_ctx* ctx, void* stream, const gapro_spf_predict_inputs* in,
                           const gapro_spf_predict_params* params, void* d_workspace, size_t workspace_bytes,
                           float* d_conf, int32_t* d_label_id, float* d_box, int32_t* d_query, int64_t cap_rows,
                           int64_t* d_run_offsets, int64_t* d_runs, int64_t cap_runs, uint8_t* d_masks,
                           gapro_spf_predict_header* d_header);

/* ------------------------------------------------------------------------------------------
 * Cost matrices of the consumer's Hungarian matcher (csrc/match_cost.hip).  Replaces the per-sample expression chain of
 * ISBNet's HungarianMatcher.get_match (isbnet/model/matcher.py:144-199): one call enqueues the cost matrices of every
 * sample of a batch.  Sample b has n_queries queries, n_inst kept instances, n_cols columns (superpoints or subsampled
 * points) and n_classes classes.  With x = d_mask_logits (f32[n_queries, n_cols]) and t = d_mask (f32[n_inst, n_cols]
 * holding 0 / 1, as gapro_spp_gt_fill writes it), sig = sigmoid(x), sp = softplus(x) = log(1 + exp(x)):
 *   dice[q,i]  = 1 - (2 sum_s sig[q,s] t[i,s] + 1) / (sum_s sig[q,s] + sum_s t[i,s] + 1)             (matcher.py:43-47)
 *   bce[q,i]   = (sum_s sp[q,s] - sum_s x[q,s] t[i,s]) / n_cols                                      (:74-81)
 *   class[q,i] = -softmax(d_cls_logits[b,q,:])[cls[i]]                                               (:173-175)
 *   conf[q,i]  = -d_conf_logits[b,q]                                                                 (:177)
 *   giou[q,i]  = -GIoU(d_box_preds[b,q], box[i]), with the clamps at 0 and the two + 1e-6 of model_utils.py:385-413
 *   cost       = w_class class + w_dice dice + w_bce bce + w_conf conf + w_giou giou                 (:192)
 * The bce line is the reference's BCE(x,1) . t + BCE(x,0) . (1 - t): BCE(x,0) = sp, BCE(x,1) = sp - x, so their
 * difference is -x, and since t is 0 or 1 the identity is exact.  Every term is evaluated in float64 from the float32
 * inputs, every sum over s is a float64 sum in a fixed order, the cost is combined in float64 and rounded to float32 once;
 * an entry that is then NaN or +-inf becomes 100000.0f (:196-197).  No floating-point atomics: two calls on the same
 * input give the same bytes.  A NaN propagates as in the reference: through the min / max / clamp of the boxes too.
 *
 * h_tasks is read during the call only.  A task with n_inst == 0 is a sample without a kept instance: its pointers are
 * not looked at and nothing is written for it.  The call uploads one table, launches two kernels and, when given, copies
 * d_cost to h_cost_pinned and d_status to h_status_pinned behind them; it only enqueues.
 * d_status i32[GAPRO_MATCH_STATUS_WORDS] = {status, the lowest sample of the refusal or -1, flags, 0}.  Refusals of the
 * data, with nothing written to d_cost:
 *   GAPRO_ERR_BAD_ARG  flags & 1: a class label outside [0, n_classes);  flags & 2: a mask value that is neither 0 nor 1
 * Refused before anything is launched (GAPRO_ERR_BAD_ARG): a null or non-positive argument, ld_logits < n_cols, an
 * unknown cls_type (GAPRO_LABEL_I32 / _I64 only), no task with an instance, cost_offsets whose [n_queries, n_inst]
 * blocks overlap or leave [0, cost_floats), a weight that is negative or not finite, batch_size >
 * GAPRO_SPP_GT_MAX_SAMPLES; GAPRO_ERR_WORKSPACE: a workspace smaller than gapro_match_cost_workspace_bytes (0 for sizes
 * the call refuses; total_inst / total_cols = the sums of n_inst / n_cols over the tasks with n_inst > 0).
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_MATCH_STATUS_WORDS 4
typedef struct {            /* one per sample; n_inst == 0: the sample has no kept instance, nothing is written */
  const float* d_mask_logits;   /* f32[n_queries, n_cols], row stride ld_logits */
  int64_t      ld_logits;
  const float* d_mask;          /* f32[n_inst, n_cols], packed, 0 / 1 */
  const void*  d_cls;           /* GAPRO_LABEL_I32 / _I64 [n_inst] */
  const float* d_box;           /* f32[n_inst, 6] */
  int32_t      n_inst, n_cols;
  int64_t      cost_offset;     /* floats from d_cost to this sample's f32[n_queries, n_inst] */
} gapro_match_task;
typedef struct { double w_class, w_dice, w_bce, w_conf, w_giou; } gapro_match_weights; /* defaults 0.5, 1, 1, 0.2, 0.2 */
size_t gapro_match_cost_workspace_bytes(int32_t batch_size, int32_t n_queries, int64_t total_inst, int64_t total_cols);
int gapro_match_cost(gapro_ctx* ctx, void* stream, const gapro_match_task* h_tasks, int32_t batch_size,
                     int32_t n_queries, int32_t n_classes, int32_t cls_type,
                     const float* d_cls_logits /* [B,Q,C] */, const float* d_conf_logits /* [B,Q] */,
                     const float* d_box_preds /* [B,Q,6] */, const gapro_match_weights* w /* NULL: defaults */,
                     void* d_workspace, size_t workspace_bytes, float* d_cost, int64_t cost_floats,
                     float* h_cost_pinned /* NULL or cost_floats: async copy behind the kernels */,
                     int32_t* d_status, int32_t* h_status_pinned);

/* ------------------------------------------------------------------------------------------
 * Matched losses (csrc/match_loss.hip).  Replaces the loop of ISBNet's Criterion.single_layer_loss
 * (isbnet/model/criterion.py:235-331): the seven main losses of a whole batch in two launches, their gradients in one.
 * Sample b has n_queries queries, n_gt matched rows (h_rows[row_offset + r] = the query of row r, distinct, in
 * [0, n_queries)), n_cols columns which are [col_offset, col_offset + n_cols) of d_prob_labels (f32[n_points]),
 * d_levelset_feats (f32[n_points, n_feats], 1 <= n_feats <= GAPRO_MATCH_LOSS_MAX_FEATS) and d_levelset_coords
 * (f32[n_points, 3]).  A task with n_gt == 0 is a skipped sample: it adds nothing, not even a class term, but counts in
 * the division by batch_size.  The rule continues the matcher's: float64 from the float32 inputs, every sum a float64
 * sum in a fixed order, one rounding.  With x the matched rows of the logits, t = d_inst_labels, w the sample's slice of
 * d_prob_labels, n = n_gt, e = exp(-|x|), sig = (x >= 0 ? 1 : e) / (1 + e), sp = max(x, 0) + log1p(e), per sample:
 *   dice     = sum_r [1 - (2 sum_s sig t + 1) / (sum_s sig + sum_s t + 1)] / (n + 1e-6)                  (:23-43)
 *   bce      = (sum_{r,s} w_s (sp - x t)) / (sum_s w_s) / (n + 1e-6); a zero weight sum gives NaN         (:287-288)
 *   iou      = sum_r (conf_r - inter_r / (union_r + 1e-6))^2 / n, inter = sum_s [x >= 0] t,
 *              union = sum_s [x >= 0] + sum_s t - inter; no gradient through the IoU                      (:10-20, 293-297)
 *   cls      = sum_q W[tgt_q] (lse_q - z[q, tgt_q]) / sum_q W[tgt_q] over ALL queries, tgt_q the matched row's class
 *              or n_classes - 1, W = d_empty_weight (f32[n_classes])                                     (:299-310)
 *   box      = (voxel_scale / 50) sum |box_pred - box_label| / n                                          (:312-315)
 *   giou     = sum_r (1 - GIoU_r) / n, the clamps at 0 and the two + 1e-6 of model_utils.py:277-306; min / max / clamp
 *              hand a NaN on
 *   levelset = sum_r L_r / (n + 1e-4): column s belongs to box r iff coords >= (float)(lo - 0.005f) and
 *              coords <= (float)(hi + 0.005f) on all three axes, a FLOAT32 comparison (a NaN is outside); with n_r the
 *              member count, v = sig(x[r, s]), A = sum v, mu_f = (sum v f_sf) / max(A, 1e-5):
 *              L_r = (1 / n_r) sum_s v sum_f (f_sf - mu_f)^2, a box with n_r = 0 left out                 (:193-233)
 * d_losses f32[GAPRO_MATCH_LOSS_N] = the samples' values added in sample order and divided by batch_size, in the order
 * dice, bce, cls, iou, box, giou, levelset.  The IoU predicate is the exact x >= 0 (the reference's float32
 * sigmoid(x) >= 0.5 also admits negative x of magnitude below about 6e-8).
 * gapro_match_loss_backward: the exact derivatives of these expressions, weighted by d_grad_losses (f32[7], read on the
 * device), in float64, rounded once: L1 with sign(0) = 0, the clamps and min / max with torch's subgradients (a clamp
 * passes at equality, min / max share a tie), the max(A, 1e-5) branch with its own d mu / d v, sig - t in the
 * cancellation-free form; nothing overflows at |x| = 100.  A NULL gradient pointer is not written.  d_grad_mask_logits
 * holds the kept samples' packed f32[n_queries, n_cols] blocks one after the other in sample order; every row of a kept
 * sample is written (zeros for an unmatched query), and every row of d_grad_cls_logits / _conf_logits / _box_preds
 * (zeros for a skipped sample).  It reads the workspace and the inputs as the forward call left them.
 * No floating-point atomics: two calls give equal bytes.  The forward call uploads one table (tasks, row indices, the
 * per-query table query -> row or -1, the zeroed status), launches two kernels and, when given, copies d_status to
 * h_status_pinned behind them; both calls only enqueue.
 * d_status i32[GAPRO_MATCH_STATUS_WORDS] = {status, the lowest sample of the refusal or -1, flags, 0}.  Refused by the
 * device: flags & 1, a class label outside [0, n_classes): GAPRO_ERR_BAD_ARG, all seven losses NaN, and the backward
 * call writes zeros.  Refused before anything is launched (GAPRO_ERR_BAD_ARG): a null or non-positive argument,
 * n_feats outside its range, ld_logits < n_cols, columns that leave [0, n_points), a row_offset that is not the sum of
 * the earlier n_gt, a row index outside [0, n_queries) or listed twice, every sample skipped, a voxel_scale that is not
 * finite, batch_size > GAPRO_SPP_GT_MAX_SAMPLES; GAPRO_ERR_WORKSPACE: a workspace smaller than
 * gapro_match_loss_workspace_bytes (0 for sizes the call refuses; total_gt = the sum of n_gt).
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_MATCH_LOSS_N 7
#define GAPRO_MATCH_LOSS_MAX_FEATS 8
typedef struct {            /* one per sample; n_gt == 0: skipped */
  const float* d_mask_logits;   /* f32[n_queries, n_cols], row stride ld_logits */
  int64_t      ld_logits;
  const float* d_inst_labels;   /* f32[n_gt, n_cols], packed */
  const void*  d_cls_labels;    /* GAPRO_LABEL_I32 / _I64 [n_gt] */
  const float* d_box_labels;    /* f32[n_gt, 6] */
  int32_t      n_gt, n_cols;
  int64_t      col_offset;      /* the sample's first column in d_prob_labels, d_levelset_feats, d_levelset_coords */
  int64_t      row_offset;      /* the sum of n_gt over the samples before this one */
} gapro_match_loss_task;
size_t gapro_match_loss_workspace_bytes(int32_t batch_size, int32_t n_queries, int64_t total_gt);
int gapro_match_loss_forward(gapro_ctx* ctx, void* stream, const gapro_match_loss_task* h_tasks,
                             const int32_t* h_rows /* [total_gt] */, int32_t batch_size, int32_t n_queries,
                             int32_t n_classes, int32_t cls_type, int32_t n_feats,
                             const float* d_cls_logits /* [B,Q,C] */, const float* d_conf_logits /* [B,Q] */,
                             const float* d_box_preds /* [B,Q,6] */, const float* d_prob_labels,
                             const float* d_levelset_feats, const float* d_levelset_coords, int64_t n_points,
                             const float* d_empty_weight /* [C] */, double voxel_scale, void* d_workspace,
                             size_t workspace_bytes, float* d_losses /* [7] */, int32_t* d_status,
                             int32_t* h_status_pinned /* NULL: no copy */);
int gapro_match_loss_backward(gapro_ctx* ctx, void* stream, int32_t batch_size, int32_t n_queries, int32_t n_classes,
                              int32_t cls_type, int32_t n_feats, int64_t total_gt, const float* d_cls_logits,
                              const float* d_conf_logits, const float* d_box_preds, const float* d_prob_labels,
                              const float* d_levelset_feats, const float* d_levelset_coords,
                              const float* d_empty_weight, double voxel_scale, const void* d_workspace,
                              size_t workspace_bytes, const float* d_grad_losses /* [7] */,
                              float* d_grad_cls_logits /* [B,Q,C] or NULL */, float* d_grad_mask_logits,
                              float* d_grad_conf_logits /* [B,Q] or NULL */, float* d_grad_box_preds /* [B,Q,6] or NULL */);

/* ------------------------------------------------------------------------------------------
 * SPFormer's criterion (csrc/spf_loss.hip).  Replaces the per-sample loops of SPFormer's Criterion.forward and
 * get_layer_loss (SPFormer/spformer/model/loss.py:415-499, 263-349) for ALL prediction heads at once: the five losses
 * of every head in two launches, their gradients in one.  There are n_heads heads (the main head LAST, aux head i at
 * index i), batch_size samples, n_queries queries and n_classes = num_class + 1 classes, the last one "no object".
 * Task h * batch_size + b is head h of sample b: its class logits f32[n_queries, n_classes] and scores f32[n_queries],
 * its mask logits, and the sample's GT (n_inst instances: masks f32[n_inst, n_cols] of 0 / 1, labels, boxes).  Its
 * n_gt matched pairs are h_rows / h_cols[row_offset + r]: the query and the GT instance of row r (queries distinct and
 * in [0, n_queries), instances in [0, n_inst)).  n_gt == 0 is a skipped sample: only its class terms count.  The
 * sample's columns are [col_offset, col_offset + n_cols) of d_sp_prob (f32[n_points]), d_sp_feats
 * (f32[n_points, n_feats]) and d_sp_coords (f32[n_points, 3]).
 * The rule is the matched losses': float64 from the float32 inputs, every sum a float64 sum in a fixed order, one
 * rounding.  With x the matched rows of the logits, t the matched GT masks, w the sample's slice of d_sp_prob, n = n_gt,
 * S = n_cols, B = batch_size, e = exp(-|x|), sig = (x >= 0 ? 1 : e) / (1 + e), sp = max(x, 0) + log1p(e), per head:
 *   cls      = sum_{b,q} W[tgt] (lse - z[tgt]) / sum_{b,q} W[tgt] over all B Q queries, tgt the matched instance's label
 *              or num_class, W = 1 but non_object_weight for num_class; not divided by B                  (:419-428)
 *   bce      = sum_b bce_b / B.  As released (:464-466; `reduce="none"` is the legacy boolean and selects the mean):
 *              bce_b = [sum_{r,s} (sp - x t) / (n S)] * (sum_s w / sum_s w), the factor being 1, or NaN for a weight sum
 *              that is 0, infinite or NaN.  GAPRO_SPF_WEIGHTED_BCE: bce_b = sum_{r,s} w_s (sp - x t) / (sum_s w) / n
 *   dice     = sum_b [sum_r (1 - (2 sum_s sig t + 1) / (sum_s sig + sum_s t + 1)) / n]; divided by B for the aux heads
 *              (:331) and, as released, NOT for the main head (:469-488) unless GAPRO_SPF_DICE_DIV_MAIN
 *   score    = sum_b [sum_{kept r} (score_r - iou_r)^2 / n_kept] / B with inter = sum_s [x >= 0] t,
 *              union = sum_s [x >= 0] + sum_s t - inter, iou = inter / (union + 1e-6); a row is kept iff iou > 0.5,
 *              decided as the integer predicate 2 inter > union; a sample without a kept row adds nothing; no gradient
 *              through the IoU                                                                            (:455-462)
 *   levelset = sum_b [sum_r L_r / (n + 1e-4)] / B with the matched losses' L_r (float32 membership test, n_r members,
 *              mu_f = (sum v f) / max(A, 1e-5)); a box takes part iff n_r >= min_points (>= 1)              (:351-391)
 * d_losses f32[n_heads, GAPRO_SPF_LOSS_N] in the order cls, bce, dice, score, levelset.  A batch whose samples are all
 * skipped is legitimate: its class loss, and zeros.  gapro_spf_loss_backward: the exact float64 derivatives, weighted by
 * d_grad_losses (f32[n_heads, 5], read on the device), rounded once, with the kink conventions of the matched losses.
 * It writes EVERY element of d_grad_labels (f32[n_heads, B, Q, n_classes]), d_grad_scores (f32[n_heads, B, Q]) and
 * d_grad_masks (the packed f32[n_queries, n_cols] blocks of the tasks with n_gt > 0, in task order), zeros included; a
 * NULL pointer is not written.  No floating-point atomics: two calls give equal bytes, and a head's values do not
 * depend on the other heads of the call.  The forward call uploads one table (tasks, rows, columns, query -> row or -1,
 * the zeroed status), launches two kernels and, when given, copies d_status to h_status_pinned; both calls only enqueue.
 * d_status i32[GAPRO_MATCH_STATUS_WORDS] = {status, the lowest task of the refusal or -1, flags, 0}.  Refused by the
 * device (GAPRO_ERR_BAD_ARG, every loss NaN, the backward writes zeros): flags & 1, a matched label outside
 * [0, num_class); flags & 2, a matched mask value that is neither 0 nor 1.  Refused before anything is launched
 * (GAPRO_ERR_BAD_ARG): a null or non-positive argument, n_feats outside [1, GAPRO_MATCH_LOSS_MAX_FEATS], n_classes < 2,
 * a non_object_weight that is not finite, ld_logits < n_cols, columns that leave [0, n_points), a row_offset that is
 * not the sum of the earlier n_gt, a row or column index out of range or a row listed twice, n_heads * batch_size >
 * GAPRO_SPP_GT_MAX_SAMPLES; GAPRO_ERR_WORKSPACE: a workspace smaller than gapro_spf_loss_workspace_bytes (0 for sizes
 * the call refuses; total_gt = the sum of n_gt over all tasks, which may be 0).
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_SPF_LOSS_N 5
#define GAPRO_SPF_WEIGHTED_BCE 1
#define GAPRO_SPF_DICE_DIV_MAIN 2
typedef struct {            /* one per (head, sample); n_gt == 0: skipped */
  const float* d_labels;        /* f32[n_queries, n_classes] */
  const float* d_scores;        /* f32[n_queries] */
  const float* d_mask_logits;   /* f32[n_queries, n_cols], row stride ld_logits */
  int64_t      ld_logits;
  const float* d_gt_masks;      /* f32[n_inst, n_cols], packed */
  const void*  d_gt_labels;     /* GAPRO_LABEL_I32 / _I64 [n_inst] */
  const float* d_gt_boxes;      /* f32[n_inst, 6] */
  int32_t      n_gt, n_inst, n_cols, reserved;
  int64_t      col_offset;      /* the sample's first column in d_sp_prob, d_sp_feats, d_sp_coords */
  int64_t      row_offset;      /* the sum of n_gt over the tasks before this one */
} gapro_spf_loss_task;
typedef struct {
  int32_t n_heads, batch_size, n_queries, n_classes, cls_type, n_feats, min_points, flags;
  double  non_object_weight;
} gapro_spf_loss_dims;
size_t gapro_spf_loss_workspace_bytes(int32_t n_heads, int32_t batch_size, int32_t n_queries, int64_t total_gt);
int gapro_spf_loss_forward(gapro_ctx* ctx, void* stream, const gapro_spf_loss_dims* dims,
                           const gapro_spf_loss_task* h_tasks /* [n_heads * batch_size] */,
                           const int32_t* h_rows /* [total_gt] */, const int32_t* h_cols /* [total_gt] */,
                           const float* d_sp_prob, const float* d_sp_feats, const float* d_sp_coords, int64_t n_points,
                           void* d_workspace, size_t workspace_bytes, float* d_losses /* [n_heads, 5] */,
                           int32_t* d_status, int32_t* h_status_pinned /* NULL: no copy */);
int gapro_spf_loss_backward(gapro_ctx* ctx, void* stream, const gapro_spf_loss_dims* dims, int64_t total_gt,
                            const float* d_sp_prob, const float* d_sp_feats, const float* d_sp_coords,
                            const void* d_workspace, size_t workspace_bytes,
                            const float* d_grad_losses /* [n_heads, 5] */, float* d_grad_labels, float* d_grad_scores,
                            float* d_grad_masks);

/* ------------------------------------------------------------------------------------------
 * Point-wise losses (csrc/point_loss.hip).  Replaces ISBNet's Criterion.cal_point_wise_loss
 * (isbnet/model/criterion.py:136-191, called at :357): the four losses over all n_points voxels of a batch in two
 * launches, their gradients in one, with no host read.  The rule continues the matched losses': float64 from the float32
 * inputs, every sum a float64 sum in a fixed order, one rounding, no floating-point atomics.  With z = d_semantic_scores
 * (f32[n_points, n_classes], row stride ld_scores), y = d_semantic_labels, W = d_semantic_weight (f32[n_classes]; NULL:
 * ones), c = d_corners_offset and l = d_corners_offset_labels (f32[n_points, 6]), x = d_coords_float (f32[n_points, 3]),
 * P = {i : d_instance_labels[i] != ignore_label}, n = |P|:
 *   sem     = sum_{y_i != ignore} W[y_i] (lse_i - z[i, y_i]) / sum_{y_i != ignore} W[y_i], lse the max-shifted
 *             log-sum-exp; NaN when every label is ignored, as F.cross_entropy                            (:154-156)
 *   corners = (voxel_scale / 50) sum_P sum_k |c_ik - l_ik| / n                                            (:173-175, 187)
 *   giou    = sum_P (1 - GIoU(a_i, b_i)) / n, a_i = c_i + [x_i, x_i], b_i = l_i + [x_i, x_i] (the reference forms a and b
 *             in float32; here the add is float64 as everything else), the three clamps at 0 and the two + 1e-6 of
 *             model_utils.py:416-444; min / max / clamp hand a NaN on                                     (:177-181)
 *   conf    = sum_P (box_conf_i - IoU(a_i, b_i))^2 / n, no gradient through the IoU                       (:183-184)
 * d_losses f32[GAPRO_POINT_LOSS_N] in this order.  With n == 0 the last three are exactly 0 and their gradients exactly
 * zero; THE ONE DEVIATION: the reference's 0 * corners_offset.sum() is NaN for non-finite inputs, this call's 0 is not.
 * An instance label is only compared with ignore_label.
 * gapro_point_loss_backward: the exact derivatives of these expressions, weighted by d_grad_losses (f32[4], read on the
 * device), in float64, rounded once, with the conventions of gapro_match_loss_backward: L1 with sign(0) = 0, a clamp
 * passes at equality, min / max share a tie, softmax minus one-hot is expm1(z - lse) at the target; nothing overflows at
 * |z| = 100.  A NULL gradient pointer is not written; the others are written whole by the kernel (no memset):
 * d_grad_semantic_scores f32[n_points, n_classes] packed, a row zero where the label is ignored (so all zeros when every
 * label is ignored, as torch's backward); d_grad_corners_offset f32[n_points, 6], the L1 plus the GIoU term, and
 * d_grad_box_conf f32[n_points], both zero outside P.  It reads the workspace and the inputs as the forward call left
 * them.
 * Kernels: `partial`, ceil(n_points / GAPRO_POINT_LOSS_RUN) workgroups of 256 threads, one record each; `finish`, one
 * workgroup, thread t folding the records t, t + GAPRO_POINT_LOSS_FOLD, ..; `backward` on `partial`'s grid.  Both calls
 * only enqueue; the forward call copies d_status to h_status_pinned behind its kernels when given.
 * d_status i32[GAPRO_MATCH_STATUS_WORDS] = {status, the lowest point of the refusal or -1, flags, 0}.  Refused by the
 * device: flags & 1, a semantic label that is neither ignore_label nor in [0, n_classes): GAPRO_ERR_BAD_ARG, all four
 * losses NaN, and the backward call writes zeros.  Refused before anything is launched (GAPRO_ERR_BAD_ARG): a null
 * argument, n_points outside [1, 2^31 - 1], n_classes outside [GAPRO_POINT_LOSS_MIN_CLASSES,
 * GAPRO_POINT_LOSS_MAX_CLASSES], ld_scores < n_classes, an unknown label type, a voxel_scale that is not finite;
 * GAPRO_ERR_WORKSPACE: a workspace smaller than gapro_point_loss_workspace_bytes (0 for sizes the call refuses).
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_POINT_LOSS_N 4
#define GAPRO_POINT_LOSS_MIN_CLASSES 2
#define GAPRO_POINT_LOSS_MAX_CLASSES 64
#define GAPRO_POINT_LOSS_RUN 1024   /* points of one workgroup of `partial` and `backward` */
#define GAPRO_POINT_LOSS_FOLD 256   /* records `finish` folds in one pass */
size_t gapro_point_loss_workspace_bytes(int64_t n_points, int32_t n_classes);
int gapro_point_loss_forward(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t n_classes,
                             const float* d_semantic_scores, int64_t ld_scores, const void* d_semantic_labels,
                             int32_t semantic_type, const void* d_instance_labels, int32_t instance_type,
                             const float* d_corners_offset, const float* d_box_conf,
                             const float* d_corners_offset_labels, const float* d_coords_float,
                             const float* d_semantic_weight /* [C] or NULL */, int64_t ignore_label, double voxel_scale,
                             void* d_workspace, size_t workspace_bytes, float* d_losses /* [4] */, int32_t* d_status,
                             int32_t* h_status_pinned /* NULL: no copy */);
int gapro_point_loss_backward(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t n_classes,
                              const float* d_semantic_scores, int64_t ld_scores, const void* d_semantic_labels,
                              int32_t semantic_type, const void* d_instance_labels, int32_t instance_type,
                              const float* d_corners_offset, const float* d_box_conf,
                              const float* d_corners_offset_labels, const float* d_coords_float,
                              const float* d_semantic_weight, int64_t ignore_label, double voxel_scale,
                              const void* d_workspace, size_t workspace_bytes, const float* d_grad_losses /* [4] */,
                              float* d_grad_semantic_scores /* [N,C] or NULL */,
                              float* d_grad_corners_offset /* [N,6] or NULL */, float* d_grad_box_conf /* [N] or NULL */);

/* Rectangular linear sum assignment on the host (csrc/lsap.cc; no device, no ctx): the scipy.optimize call of
 * matcher.py:201-204.  cost is f32[n_rows, n_cols] with row stride ld; dup >= 1 solves the problem whose column j, j in
 * [0, dup n_cols), is cost[:, j % n_cols] -- the reference's final_cost.repeat(1, dup_gt) without the repeated matrix.
 * Shortest augmenting paths with float64 duals (Jonker and Volgenant 1987 in the rectangular form of Crouse 2016); the
 * side with fewer entries is the one whose every entry is assigned.  *n_out = min(n_rows, dup n_cols) pairs: rows
 * ascending, cols the ORIGINAL column j % n_cols.  The assignment is optimal; among equal-cost optima it is the one this
 * search finds, the same for every run: a search step that can close several columns at the same distance closes an
 * unassigned one before an assigned one and, among those, the one with the lowest index j.
 * GAPRO_ERR_BAD_ARG: a null or non-positive argument, ld < n_cols, dup n_cols beyond 2^31 - 1; GAPRO_ERR_NOT_FINITE: a
 * NaN or infinite entry (gapro_match_cost has replaced them). */
int gapro_lsap_solve(int32_t n_rows, int32_t n_cols, const float* cost, int64_t ld, int32_t dup,
                     int32_t* n_out, int32_t* rows /* [min(n_rows, dup*n_cols)] */, int32_t* cols);

/* ------------------------------------------------------------------------------------------
 * Query sampling (csrc/query_sample.hip).  Replaces the CUDA-only extensions behind ISBNet's Point
 * Aggregator (isbnet/model/aggregator.py:63-115, 154-205): isbnet.ops.furthestsampling_batchflat and
 * ballquery_batchflat, pointnet2's furthest_point_sample and ball_query.  The batched forms are the batch-flat kernels
 * with uniform offsets and GAPRO_QS_LOCAL_INDEX.
 * Samples: d_offset and d_new_offset are int32 / int64 device arrays of n_samples entries (*_i64 = 1: int64).  Sample b
 * owns the points [offset[b - 1], offset[b]) of d_xyz f32[n_points, 3] and the outputs / queries [new_offset[b - 1],
 * new_offset[b]), with offset[-1] = new_offset[-1] = 0; a leading 0 is an empty first sample.  Outputs beyond the last
 * entry of d_new_offset are not written.
 * Every squared distance is ((dx*dx + dy*dy) + dz*dz) in float32, each operation rounded on its own (no contraction).
 * gapro_fps_batch: one workgroup of GAPRO_FPS_THREADS threads serves a sample, for all of its outputs, and never waits
 *   for another workgroup; one launch per path below that n_points admits (a workgroup whose sample is of another path
 *   returns at once), each over all samples.  d_idx i32[m_total]: the first
 *   output of a sample is its first point; each later one the point with the largest running minimum of the squared
 *   distances to the outputs before it (the minimum starts at 1e10f; a NaN distance leaves it), AMONG EQUAL MAXIMA THE
 *   LOWEST INDEX.  More outputs than points repeat indices: once every minimum is 0 the first point wins.  Indices count
 *   from the start of d_xyz, with GAPRO_QS_LOCAL_INDEX from the sample's first point.  GAPRO_FPS_SKIP_ORIGIN (pointnet2's
 *   flavour): a point with x*x + y*y + z*z <= 1e-3f, evaluated as the distances are, is never a candidate and its
 *   minimum is never updated; without a candidate the sample's first point is the answer.  d_dist f32[n_points] or NULL:
 *   every point's running minimum as the last iteration left it, i.e. over all outputs of its sample but the last.
 *   The minima of a sample stay in registers up to *capacity points (gapro_fps_plan), its coordinates too up to
 *   *xyz_capacity; a larger sample keeps the minima in the workspace, gapro_fps_workspace_bytes(n_points) bytes.  The
 *   results do not depend on the path.  gapro_fps_plan returns the path of a sample of n_max points.
 * gapro_ball_query_batch: one wave a query.  d_idx i32[m_total, nsample]: the first nsample points of the query's own
 *   sample, in ascending index, with d2 < r2, r2 = (float)radius * (float)radius -- strictly: a point at exactly the
 *   radius is no hit; the remaining slots repeat the first hit; A QUERY WITHOUT A HIT HAS A ROW OF ZEROS (index 0 of the
 *   whole table, as the reference's zero-initialised output).  A NaN distance is no hit.  d_counts i32[m_total] or
 *   NULL: the hits, at most nsample.  Every row is written whole.
 * d_status i32[GAPRO_QS_STATUS_WORDS] = {status, flags, 0, 0}, cleared by the call, copied to h_status_pinned behind the
 * kernel when given.  Both calls only enqueue.  Raised by the device:
 *   GAPRO_ERR_BAD_ARG     GAPRO_QS_FLAG_OFFSETS: offsets that decrease or leave [0, n_points] / [0, m_total], or a query
 *                         beyond the last new_offset.  Such a sample writes no index (its queries: rows of zeros)
 *   GAPRO_ERR_BAD_ARG     GAPRO_QS_FLAG_EMPTY: fps, a sample with outputs and no points: its outputs are -1
 *   GAPRO_ERR_NOT_FINITE  GAPRO_QS_FLAG_NOT_FINITE: fps, a coordinate that is not finite; the indices stay inside the
 *                         sample's range.  A bad argument wins over it
 * Nothing is read or written out of range in any of these cases.  Refused before anything is launched
 * (GAPRO_ERR_BAD_ARG): a null argument, n_points or m_total outside [0, 2^31 - 1], n_samples outside [1,
 * GAPRO_QS_MAX_SAMPLES], an unknown flag, nsample outside [1, GAPRO_BALL_QUERY_MAX_NSAMPLE], m_total * nsample beyond
 * 2^31 - 1, a radius that is not finite; GAPRO_ERR_WORKSPACE: a workspace smaller than gapro_fps_workspace_bytes.
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_FPS_THREADS 1024
#define GAPRO_FPS_RESIDENT 0   /* gapro_fps_plan: coordinates and minima in registers */
#define GAPRO_FPS_STREAMED 1   /* the minima in registers, the coordinates read from L2 every iteration */
#define GAPRO_FPS_GLOBAL 2     /* the minima in the workspace */
#define GAPRO_FPS_SKIP_ORIGIN 1
#define GAPRO_QS_LOCAL_INDEX 2
#define GAPRO_QS_MAX_SAMPLES 4096
#define GAPRO_QS_STATUS_WORDS 4
#define GAPRO_QS_FLAG_OFFSETS 1
#define GAPRO_QS_FLAG_EMPTY 2
#define GAPRO_QS_FLAG_NOT_FINITE 4
#define GAPRO_BALL_QUERY_MAX_NSAMPLE 4096
int gapro_fps_plan(int64_t n_max, int64_t* xyz_capacity /* or NULL */, int64_t* capacity /* or NULL */);
size_t gapro_fps_workspace_bytes(int64_t n_points);
int gapro_fps_batch(gapro_ctx* ctx, void* stream, int64_t n_points, const float* d_xyz, int32_t n_samples,
                    const void* d_offset, int32_t offset_i64, const void* d_new_offset, int32_t new_offset_i64,
                    int64_t m_total, int32_t flags, void* d_workspace, size_t workspace_bytes,
                    int32_t* d_idx /* [m_total] */, float* d_dist /* [n_points] or NULL */, int32_t* d_status,
                    int32_t* h_status_pinned /* NULL: no copy */);
int gapro_ball_query_batch(gapro_ctx* ctx, void* stream, int64_t n_points, const float* d_xyz, int64_t m_total,
                           const float* d_new_xyz, int32_t n_samples, const void* d_offset, int32_t offset_i64,
                           const void* d_new_offset, int32_t new_offset_i64, double radius, int32_t nsample,
                           int32_t flags, int32_t* d_idx /* [m_total, nsample] */,
                           int32_t* d_counts /* [m_total] or NULL */, int32_t* d_status,
                           int32_t* h_status_pinned /* NULL: no copy */);

/* ------------------------------------------------------------------------------------------
 * Voxelisation (csrc/voxelize.hip, csrc/voxelize_host.cc).  Replaces the CUDA-only extension behind
 * isbnet.ops / pointgroup_ops voxelization_idx and voxelization (src/voxelize/voxelize.cpp, voxelize.cu).
 * The definition.  coords is int64[n_points, cols], cols 3 or 4 (4: the batch index in column 0).  A voxel is a
 * distinct row, over all columns and all 64 bits of each value.  VOXELS ARE NUMBERED BY THE INDEX OF THEIR FIRST POINT
 * IN ASCENDING ORDER
 * (the insertion order of the reference's hash map, not a sorted order).
 *   input_map     i32[n_points]            the voxel of each point
 *   output_coords i64[n_voxels, cols]      the row of each voxel's first point
 *   output_map    i32[n_voxels, width]     modes 3, 4: width = max_active + 1, a row is {count, its point indices in
 *                                          ascending order, zeros}; mode 1: {1, first point}; mode 2: {1, last point};
 *                                          mode 0: as mode 1, refused when a voxel holds two points (width 2 for 0..2)
 * max_active is the largest number of points in a voxel (every mode reports it; modes 3 and 4 refuse one beyond
 * GAPRO_VOXELIZE_MAX_ACTIVE).  gapro_voxelize_table_shape is the header arithmetic both paths share: *width for the
 * mode, GAPRO_ERR_BAD_ARG for a mode outside 0..4, n_voxels or max_active < 1, max_active > 1 in mode 0, max_active
 * beyond the cap in modes 3 and 4, or n_voxels * width beyond 2^31 - 1.
 * Device path, count / one header read / fill.  gapro_voxelize_count writes d_input_map and d_header
 * (gapro_voxelize_header, cleared by the call, copied to h_header_pinned behind the kernels when given);
 * gapro_voxelize_fill takes n_voxels and max_active as the caller read them, the SAME workspace
 * (gapro_voxelize_workspace_bytes(n_points) bytes; 0 for sizes the calls refuse) and writes d_output_coords and
 * d_output_map whole.  Both only enqueue.  The count: an open-addressing table of gapro_voxelize_plan slots (a power of
 * two, at least 2 n_points up to 2^31), a slot claimed by compare-and-swap and lowered to its voxel's first point by an
 * integer atomic minimum, an exclusive scan of the "first" flags, integer atomic counts.  The fill: points claim row
 * slots by the count's atomics, then every row is put in ascending order by rank counting (rows up to 8 entries by 8
 * lanes, up to 64 by a wave, longer ones by a workgroup through LDS).  Integer atomics only; every probe loop is
 * bounded by the table; no workgroup waits for another; the results do not depend on the schedule.
 * Raised by the device (header.status / header.flags; fill: d_status i32[GAPRO_VOXELIZE_STATUS_WORDS]):
 *   GAPRO_ERR_BAD_ARG  GAPRO_VOXELIZE_FLAG_BATCH: a negative batch index (4 columns); the point joins no voxel
 *   GAPRO_ERR_BAD_ARG  GAPRO_VOXELIZE_FLAG_DUPLICATE: mode 0 and a voxel of two points
 *   GAPRO_ERR_BAD_ARG  GAPRO_VOXELIZE_FLAG_TABLE: fill, n_voxels / max_active that are not the count's
 * Nothing is read or written out of range in any of these cases.  Refused before anything is launched
 * (GAPRO_ERR_BAD_ARG): a null argument, n_points outside [1, 2^31 - 1], cols other than 3 or 4, a mode outside 0..4,
 * what gapro_voxelize_table_shape refuses; GAPRO_ERR_WORKSPACE: a workspace smaller than
 * gapro_voxelize_workspace_bytes.  gapro_voxelize_hash is the table's hash of a row (the slot is hash & (slots - 1)).
 * Host path (no device in the process: a DataLoader worker): gapro_voxelize_host_count fills input_map and the header
 * and returns a handle, gapro_voxelize_host_fill writes the two tables from it, gapro_voxelize_host_free releases it.
 * An ordinary hash map in insertion order: an independent second implementation of the definition above.
 * Pooling.  feats f32[n_points, n_channels], map_rule i32[n_voxels, max_active + 1] (any table of that shape).
 * gapro_voxel_pool_forward: for row v with n = map_rule[v, 0], mult = 1.0f / (float)n when mode == 4 and n > 0, else
 *   1.0f; out[v, c] = (((+0 + fl(mult * x_1)) + fl(mult * x_2)) + ...) in the row's order, in float32, the product and
 *   the sum each rounded on their own (no contraction): the order of the reference's atomic adds from a zeroed buffer.
 *   A row with n = 0 is zeros; every mode runs this kernel.
 * gapro_voxel_pool_backward: d_feats[p, c] = fl(mult * d_out[v, c]) for every point p listed in row v, 0 for every
 *   unlisted point: the array is cleared, then plain stores by row -- no floating-point atomics.  This equals the
 *   reference for every table that lists a point at most once (every table gapro_voxelize_fill writes).
 * d_status i32[GAPRO_VOXELIZE_STATUS_WORDS] = {status, flags, 0, 0}, cleared by the call, copied to h_status_pinned
 * when given.  GAPRO_ERR_BAD_ARG with GAPRO_VOXEL_POOL_FLAG_COUNT (a count outside [0, max_active]: the row pools to zeros
 * and receives no gradient), _INDEX (a point index outside [0, n_points): the entry is skipped), _TWICE (forward with
 * check != 0 only: a point listed twice, found with an int32 mark per point in the workspace,
 * gapro_voxel_pool_workspace_bytes(n_points) bytes, and integer atomics).  Refused before anything is launched: a null
 * argument, n_points, n_voxels or n_channels outside [1, 2^31 - 1], max_active < 1, n_voxels * (max_active + 1) beyond
 * 2^31 - 1 (the products with n_channels are 64-bit); GAPRO_ERR_WORKSPACE: check and a workspace that is too small.
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_VOXELIZE_MAX_ACTIVE 4096
#define GAPRO_VOXELIZE_STATUS_WORDS 4
#define GAPRO_VOXELIZE_FLAG_BATCH 1
#define GAPRO_VOXELIZE_FLAG_DUPLICATE 2
#define GAPRO_VOXELIZE_FLAG_TABLE 4
#define GAPRO_VOXEL_POOL_FLAG_COUNT 1
#define GAPRO_VOXEL_POOL_FLAG_INDEX 2
#define GAPRO_VOXEL_POOL_FLAG_TWICE 4
typedef struct gapro_voxelize_header {
  int32_t status;      /* gapro_status raised on the device */
  int32_t flags;       /* GAPRO_VOXELIZE_FLAG_* */
  int32_t n_voxels;    /* M */
  int32_t max_active;  /* the largest number of points in a voxel, whatever the mode */
} gapro_voxelize_header;
int gapro_voxelize_table_shape(int32_t mode, int64_t n_voxels, int64_t max_active, int64_t* width /* or NULL */);
int64_t gapro_voxelize_plan(int64_t n_points);  /* slots of the device table; 0: n_points outside [1, 2^31 - 1] */
uint64_t gapro_voxelize_hash(const int64_t* row, int32_t cols);
size_t gapro_voxelize_workspace_bytes(int64_t n_points);
int gapro_voxelize_count(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t cols, const int64_t* d_coords,
                         int32_t mode, void* d_workspace, size_t workspace_bytes, int32_t* d_input_map /* [n_points] */,
                         gapro_voxelize_header* d_header, gapro_voxelize_header* h_header_pinned /* NULL: no copy */);
int gapro_voxelize_fill(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t cols, const int64_t* d_coords,
                        int32_t mode, int64_t n_voxels, int64_t max_active, const void* d_workspace,
                        size_t workspace_bytes, const int32_t* d_input_map, int64_t* d_output_coords /* [M, cols] */,
                        int32_t* d_output_map /* [M, width] */, int32_t* d_status,
                        int32_t* h_status_pinned /* NULL: no copy */);
int gapro_voxelize_host_count(const int64_t* coords, int64_t n_points, int32_t cols, int32_t mode,
                              int32_t* input_map /* [n_points] */, gapro_voxelize_header* header, void** handle);
int gapro_voxelize_host_fill(const void* handle, const int64_t* coords, const int32_t* input_map,
                             int64_t* output_coords /* [M, cols] */, int32_t* output_map /* [M, width] */);
void gapro_voxelize_host_free(void* handle);
size_t gapro_voxel_pool_workspace_bytes(int64_t n_points);
int gapro_voxel_pool_forward(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t n_channels, const float* d_feats,
                             int64_t n_voxels, int64_t max_active, const int32_t* d_map_rule, int32_t mode,
                             int32_t check, void* d_workspace /* check: the marks */, size_t workspace_bytes,
                             float* d_out /* [M, C] */, int32_t* d_status,
                             int32_t* h_status_pinned /* NULL: no copy */);
int gapro_voxel_pool_backward(gapro_ctx* ctx, void* stream, int64_t n_points, int32_t n_channels,
                              const float* d_grad_out /* [M, C] */, int64_t n_voxels, int64_t max_active,
                              const int32_t* d_map_rule, int32_t mode, float* d_grad_feats /* [N, C] */,
                              int32_t* d_status, int32_t* h_status_pinned /* NULL: no copy */);

/* ------------------------------------------------------------------------------------------
 * Superpoint pooling (csrc/spp_pool.hip).  Replaces torch_scatter's scatter_mean / scatter_max where
 * the consumers pool backbone features to superpoints (SPFormer spformer.py:251-280, ISBNet isbnet.py:735-748 and
 * model_utils.py:600-613), with their gradients.
 * The definition.  src is f32[R, C] (rows of any stride >= C), index is i32/i64[N] with values in [0, S), point_map is
 * an optional i32/i64[N] with values in [0, R): point p reads row point_map[p] of src; without it R == N and point p
 * reads row p.  Segment s is the set of points with index[p] == s IN ASCENDING p, n_s its length.
 *   mean      out[s, c] = fl(sum / fl(n_s)), sum = ((+0 + x_1) + x_2) + ... over the segment in ascending p, every
 *             operation rounded to float32 on its own (no contraction), a true division and not a multiplication by a
 *             reciprocal.  n_s = 0 gives +0.0; a lone -0.0 gives +0.0.  This is scatter_mean (scatter_add_, the count
 *             clamped to 1, true_divide_) with its atomics arriving in point order.
 *   max       best starts as the segment's first value and arg as that point; a later value replaces it only if
 *             v > best in float32: the lowest point index wins ties (+0.0 against -0.0 included), a NaN never replaces
 *             anything and a leading NaN is never replaced.  n_s = 0 gives +0.0 and arg = N.  arg is i64[S, C] and
 *             holds POINT indices.
 *   backward  mean: d_point[p, c] = fl(g[index[p], c] / fl(n)); max: d_point[p, c] = g[s, c] if arg[s, c] == p, else 0.
 *             Without point_map d_src = d_point; with it d_src[r, c] is the sum of d_point[p, c] over the points with
 *             point_map[p] == r in ascending p, in float32 from +0, and a row that no point reads gets 0.  The
 *             gradient array is written whole by plain stores.  No floating-point atomics anywhere.
 * The plan (gapro_spp_plan: sizes and device pointers, a host struct read when a call enqueues; the caller owns every
 * array and keeps index and point_map unchanged while the plan is in use).  gapro_spp_plan_build writes
 *   seg_off i32[S + 1], seg_pts i32[N]   the CSR by superpoint, each segment in ascending point order; the points left
 *                                        out (below) follow the last segment in ascending order
 *   counts  i32[S]
 *   row_off i32[R + 1], row_pts i32[N]   with point_map: the CSR by source row, by the same routine
 *   seg_rows i32[N]                      with point_map: point_map[seg_pts[k]]; -1 behind the last segment
 * by a stable LSD radix sort of the point indices by key: 8-bit digits, ceil(bits(S) / 8) passes (the key S is the
 * sentinel of a point left out), per pass a histogram per tile of GAPRO_SPP_SORT_TILE points, an exclusive scan of the
 * bin-major histogram in three launches (no look-back, no spin-wait) and a stable scatter (ballot ranks within a wave,
 * a per-wave bin scan in LDS); the offsets by bisection.  Integer atomics only, the output does not depend on the
 * schedule, and the cost is linear in N whatever the segments' lengths.
 * With n_batches > 0, d_batch_offsets (i32/i64[n_batches + 1], the point offsets of the samples) gives
 * d_spp_batch_offsets i64[n_batches + 1]: entry b + 1 minus entry b is the number of non-empty segments whose first
 * point lies in sample b -- the reference's loop of torch.unique when no id is shared between samples.
 * d_status i32[GAPRO_SPP_STATUS_WORDS] = {status, flags, 0, 0}, cleared by the call, copied to h_status_pinned when
 * given: GAPRO_ERR_BAD_ARG with GAPRO_SPP_FLAG_INDEX (an index outside [0, S)) or GAPRO_SPP_FLAG_MAP (a map value
 * outside [0, R)).  A flagged point is left out of every segment and row and receives no gradient; nothing is read or
 * written out of range.  Refused before anything is launched (GAPRO_ERR_BAD_ARG): a null argument, N outside
 * [1, 2^31 - 1], S outside [1, GAPRO_SPP_MAX_SEGMENTS], R beyond it, n_batches beyond GAPRO_SPP_MAX_BATCHES;
 * GAPRO_ERR_WORKSPACE: fewer than gapro_spp_plan_workspace_bytes(N, n_batches) bytes (0 for sizes the build refuses).
 * gapro_spp_pool_forward: a thread per (segment, channel), consecutive lanes on consecutive channels; reduce is
 * GAPRO_SPP_MEAN or GAPRO_SPP_MAX (d_arg needed); through_map != 0 reads src [n_rows, C] through the plan's map,
 * through_map == 0 reads src [N, C] by point (a plan with a map serves both).  gapro_spp_pool_backward writes
 * d_grad_src [n_rows or N, C] whole.  Both only enqueue; C is any positive int.
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_SPP_SORT_TILE 4096
#define GAPRO_SPP_MAX_SEGMENTS (1 << 24)
#define GAPRO_SPP_MAX_BATCHES 65536
#define GAPRO_SPP_STATUS_WORDS 4
#define GAPRO_SPP_FLAG_INDEX 1
#define GAPRO_SPP_FLAG_MAP 2
#define GAPRO_SPP_MEAN 0
#define GAPRO_SPP_MAX 1
typedef struct gapro_spp_plan {
  int64_t n_points;          /* N */
  int64_t n_spps;            /* S */
  int64_t n_rows;            /* R; 0: no point_map */
  const void* d_index;       /* [N] */
  const void* d_point_map;   /* [N] or NULL */
  int32_t index_i64;         /* 1: d_index is int64 */
  int32_t map_i64;
  int32_t* d_seg_off;        /* [S + 1] */
  int32_t* d_seg_pts;        /* [N] */
  int32_t* d_counts;         /* [S] */
  int32_t* d_row_off;        /* [R + 1] or NULL */
  int32_t* d_row_pts;        /* [N] or NULL */
  int32_t* d_seg_rows;       /* [N] or NULL */
} gapro_spp_plan;
size_t gapro_spp_plan_workspace_bytes(int64_t n_points, int64_t n_batches);
int gapro_spp_plan_build(gapro_ctx* ctx, void* stream, const gapro_spp_plan* plan, int64_t n_batches,
                         const void* d_batch_offsets /* or NULL */, int32_t offsets_i64,
                         int64_t* d_spp_batch_offsets /* [n_batches + 1] or NULL */, void* d_workspace,
                         size_t workspace_bytes, int32_t* d_status, int32_t* h_status_pinned /* NULL: no copy */);
int gapro_spp_pool_forward(gapro_ctx* ctx, void* stream, const gapro_spp_plan* plan, const float* d_src,
                           int64_t src_rows, int64_t src_ld, int32_t n_channels, int32_t reduce, int32_t through_map,
                           float* d_out /* [S, C] */, int64_t* d_arg /* [S, C]; NULL for the mean */);
int gapro_spp_pool_backward(gapro_ctx* ctx, void* stream, const gapro_spp_plan* plan,
                            const float* d_grad_out /* [S, C] */, int32_t n_channels, int32_t reduce,
                            int32_t through_map, const int64_t* d_arg /* max */,
                            float* d_grad_src /* [n_rows or N, C] */);

/* ------------------------------------------------------------------------------------------
 * Dynamic-convolution mask head (csrc/dyco_head.hip).  Replaces the per-sample loop of
 * ISBNet.forward_head (isbnet/model/isbnet.py:783-828) with parse_dynamic_params (:834-853) and mask_heads_forward
 * (:855-885), and its autograd, without the [Q, C + 6, N_b] input the reference materialises.
 * The definition.  For sample b, point n in [off[b], off[b + 1]) and query q, with C = mask_dim_out:
 *     x[0:3]   = queries_locs[b, q, :] - locs_float[n, :]
 *     x[3:6]   = | (qbox[b, q, 3:6] - qbox[b, q, 0:3]) - (box_preds[n, 3:6] - box_preds[n, 0:3]) |
 *     x[6:6+C] = mask_features[n, :]
 *     theta    = controllers[b, q, :]
 * theta holds P floats: W1[(C + 6) x C] (row-major, input channel major), W2[C x C/2], W3[C/2], b1[C], b2[C/2], b3[1];
 *     h1[j]   = max(0, b1[j] + sum_a W1[a, j] x[a])
 *     h2[k]   = max(0, b2[k] + sum_j W2[j, k] h1[j])
 *     y[q, n] = sum_k W3[k] h2[k]
 * b3 is not read.  P = (C + 6) C + C C/2 + C/2 + C + C/2 + 1: 1793 at C = 32, 513 at C = 16; any other C is refused.
 * The logits are packed by sample: sample b's f32[Q, N_b] starts Q (off[b] - off[0]) floats into d_mask_logits, and
 * d_grad_logits has the same layout.
 * Arithmetic: float64 from the float32 inputs (FP64 MFMA), rounded once to float32 on the store; no floating-point
 * atomics, every sum in a fixed order, so two calls give equal bytes.
 * Gradients: controllers (the b3 column exact zeros), queries_box_preds, mask_features and box_preds; relu' at a
 * pre-activation of exactly 0 is 0 and the derivative of |d| at d = 0 is 0.  h1 and h2 are recomputed; nothing of size
 * Q x N x C is stored.  One kernel is organised by query (controllers, queries_box_preds: the points in ascending
 * tiles of 16, the four waves of a workgroup added in wave order) and one by point (mask_features, box_preds: the
 * queries in ascending order); a kernel whose two outputs are both NULL is not launched.  Every gradient array that is
 * given is written whole by plain stores, the rows of points outside [off[0], off[B]) and of samples without points
 * included.  mask_features has rows of stride ld_features >= C; its gradient is dense [N, C].
 * h_batch_offsets: B + 1 host integers, not decreasing, inside [0, n_points]; B <= GAPRO_DYCO_MAX_BATCH.  Both calls
 * only enqueue.  The workspace is not used (gapro_dyco_workspace_bytes is 0; NULL is accepted).
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_DYCO_MAX_BATCH 64
int64_t gapro_dyco_param_count(int32_t mask_dim_out);   /* P; 0 for a C that is not built */
size_t gapro_dyco_workspace_bytes(int32_t n_batches, int32_t n_queries, int64_t n_points, int32_t mask_dim_out);
int gapro_dyco_forward(gapro_ctx* ctx, void* stream, int32_t n_batches, int32_t n_queries, int32_t mask_dim_out,
                       const int64_t* h_batch_offsets, int64_t n_points, const float* d_controllers /* [B, Q, P] */,
                       const float* d_mask_features /* [N, C], row stride ld_features */, int64_t ld_features,
                       const float* d_locs_float /* [N, 3] */, const float* d_box_preds /* [N, 6] */,
                       const float* d_queries_locs /* [B, Q, 3] */, const float* d_queries_box_preds /* [B, Q, 6] */,
                       void* d_workspace, size_t workspace_bytes, float* d_mask_logits /* packed */);
int gapro_dyco_backward(gapro_ctx* ctx, void* stream, int32_t n_batches, int32_t n_queries, int32_t mask_dim_out,
                        const int64_t* h_batch_offsets, int64_t n_points, const float* d_controllers,
                        const float* d_mask_features, int64_t ld_features, const float* d_locs_float,
                        const float* d_box_preds, const float* d_queries_locs, const float* d_queries_box_preds,
                        const float* d_grad_logits /* packed */, void* d_workspace, size_t workspace_bytes,
                        float* d_grad_controllers /* [B, Q, P] or NULL */,
                        float* d_grad_queries_box_preds /* [B, Q, 6] or NULL */,
                        float* d_grad_mask_features /* [N, C] or NULL */, float* d_grad_box_preds /* [N, 6] or NULL */);

/* ------------------------------------------------------------------------------------------
 * Sparse convolutions (csrc/spconv.hip).  The three spconv layers the U-Nets of both consumers are
 * built from (ISBNet/isbnet/model/blocks.py:158-255, SPFormer/spformer/model/backbone.py:38-208), as functions of
 * (features, weight, plan), and the plans ("rulebooks") they share.  spconv has no build for this GPU; that the kernel
 * index and weight conventions below are spconv 2.x's rests on its documentation and on the reference's use of it, not
 * on a run.
 * The definitions.  coords is int32 or int64 [V, 4] with columns (batch, z, y, x), the rows unique, batch in [0, B) and
 * (z, y, x) inside spatial_shape = (Dz, Dy, Dx).  A weight is f32[C_out, kz, ky, kx, C_in] (K = kz ky kx offsets,
 * k = (kz, ky, kx) flattened), bias f32[C_out] or NULL.  row(b, p) is the row whose coordinates are (b, p), if any.
 *   Submanifold, k = 3:   y[r] = bias + sum over d in {-1, 0, 1}^3 of W[:, d + 1, :] x[row(b_r, p_r + d)], over the
 *       offsets whose voxel is active, in the same sample and inside [0, D).  The output rows are the input rows.
 *       This is the dense cross-correlation conv3d(padding = 1) of the scattered grid, read at the active sites.
 *   Strided, k = 2, stride 2, no padding:  the coarse voxel of a row is (b, z >> 1, y >> 1, x >> 1); a row whose coarse
 *       coordinate reaches D_out = (D - 2) / 2 + 1 in any axis (the last slice of an odd extent; D_out = 0 for D = 1)
 *       contributes to nothing.  y[q] = bias + sum over the children of q of W[:, p_child & 1, :] x[child].  COARSE ROWS
 *       ARE NUMBERED BY THEIR FIRST CHILD IN ASCENDING INPUT ROW.
 *   Inverse, k = 2, on a strided plan:  the output rows are the strided layer's INPUT rows;
 *       y[i] = bias + W[:, p_i & 1, :] x[parent(i)]; a row without a parent gets bias alone.  This is the dense
 *       conv_transpose3d(stride = 2) read at the fine active sites.
 * Arithmetic: float64 from the float32 operands (FP64 MFMA), bias added last, one rounding on the store; no
 * floating-point atomics; the order of every sum is fixed by the layout and, for the outputs and the input gradients,
 * does not depend on the other rows of the call: two calls give equal bytes and a batch equals each of its samples
 * alone.  Finite inputs are expected (an absent pair enters a tile's product as a zero).
 * The plans.  gapro_spconv_subm_plan: neighbours int32[27][V], offset-major, -1 for "none"; no host read.
 * gapro_spconv_down_count, ONE host read of the header {status, flags, n_out, 0}, gapro_spconv_down_fill with that
 * n_out: coarse_coords int32[n_out, 4], children int32[8][n_out] (the child slot is (z & 1) 4 + (y & 1) 2 + (x & 1),
 * -1 for "none"), parent int32[V] (-1 for a dropped row) and child_slot int32[V].  Status words {status, flags, ..}:
 * a duplicate row, a coordinate outside spatial_shape and a batch index outside [0, B) set GAPRO_ERR_BAD_ARG and a
 * flag; they are copied to h_*_pinned only when it is given.  A flagged row has no pairs.  A key packs (b, z + 1, y + 1,
 * x + 1) over extents D + 2, so that a probe at -1 or at D is the key of no voxel of any sample; B (Dz + 2) (Dy + 2)
 * (Dx + 2) >= 2^63 is refused.
 * The convolutions take ONE table form: K offsets and, per output row and offset, an input row or -1 -- either
 * d_table int32[K][rows_out] with d_k_of NULL, or "one of K": d_table int32[rows_out] and d_k_of int32[rows_out], the
 * only pair of row r being (d_k_of[r], d_table[r]).  An entry outside [0, rows_in) is no pair.
 *   layer      forward                      backward_input (rows_out = the layer's input rows)      backward_weight
 *   subm       neighbours, K = 27           neighbours, reverse_k = 1 (nbrT[k] = nbr[26 - k])       neighbours
 *   strided    children, K = 8              parent with child_slot, one of 8                        children
 *   inverse    parent/child_slot, one of 8  children, K = 8                                         parent/child_slot
 * backward_input is the forward kernel on the transposed table with the weights read transposed; c_in and c_out are
 * the LAYER's in every call.  backward_weight: dW[k] = sum over rows of g[r] (x) x[table[k][r]] by FP64 MFMA with the
 * rows as the contraction; chunks of gapro_spconv_chunk_rows rows go to float64 partials in the workspace
 * (gapro_spconv_workspace_bytes, at most about GAPRO_SPCONV_PARTIAL_BYTES, a chunk never below
 * GAPRO_SPCONV_MIN_CHUNK_ROWS rows) and a second kernel adds the chunks in ascending order and rounds once; d_grad_bias
 * is the column sum of g by the same two stages.  A backward call whose outputs are all NULL launches nothing.  Every
 * gradient given is written whole by plain stores.  1 <= C_in, C_out <= GAPRO_SPCONV_MAX_CHANNELS, any value.
 * ---------------------------------------------------------------------------------------- */
#define GAPRO_SPCONV_STATUS_WORDS 4
#define GAPRO_SPCONV_FLAG_DUPLICATE 1
#define GAPRO_SPCONV_FLAG_RANGE 2
#define GAPRO_SPCONV_FLAG_BATCH 4
#define GAPRO_SPCONV_FLAG_TABLE 8          /* a workspace that is not the count's, or more rows than table slots */
#define GAPRO_SPCONV_MAX_ROWS (1LL << 30)
#define GAPRO_SPCONV_MAX_CHANNELS 512
#define GAPRO_SPCONV_CIN_CHUNK 32          /* contracted channels of one weight slice in LDS */
#define GAPRO_SPCONV_MIN_CHUNK_ROWS 256
#define GAPRO_SPCONV_PARTIAL_BYTES (64LL << 20)
size_t gapro_spconv_subm_plan_workspace_bytes(int64_t n_rows);   /* 0: n_rows beyond the bounds */
int gapro_spconv_subm_plan(gapro_ctx* ctx, void* stream, int64_t n_rows, const void* d_coords /* [V, 4] */,
                           int32_t coords_i64, const int32_t* h_spatial_shape /* 3, host */, int32_t batch_size,
                           void* d_workspace, size_t workspace_bytes, int32_t* d_neighbours /* [27][V] */,
                           int32_t* d_status /* GAPRO_SPCONV_STATUS_WORDS */, int32_t* h_status_pinned /* or NULL */);
size_t gapro_spconv_down_plan_workspace_bytes(int64_t n_rows);
int gapro_spconv_down_count(gapro_ctx* ctx, void* stream, int64_t n_rows, const void* d_coords, int32_t coords_i64,
                            const int32_t* h_spatial_shape, int32_t batch_size, void* d_workspace,
                            size_t workspace_bytes, int32_t* d_header /* GAPRO_SPCONV_STATUS_WORDS */,
                            int32_t* h_header_pinned /* or NULL */);
int gapro_spconv_down_fill(gapro_ctx* ctx, void* stream, int64_t n_rows, const void* d_coords, int32_t coords_i64,
                           const int32_t* h_spatial_shape, int32_t batch_size, int64_t n_out,
                           const void* d_workspace /* the count's */, size_t workspace_bytes,
                           int32_t* d_coarse_coords /* [n_out, 4] */, int32_t* d_children /* [8][n_out] */,
                           int32_t* d_parent /* [V] */, int32_t* d_child_slot /* [V] */, int32_t* d_status,
                           int32_t* h_status_pinned /* or NULL */);
int64_t gapro_spconv_chunk_rows(int64_t rows_out, int32_t K, int32_t c_in, int32_t c_out);   /* 0: beyond the bounds */
size_t gapro_spconv_workspace_bytes(int64_t rows_out, int32_t K, int32_t c_in, int32_t c_out);
int gapro_spconv_forward(gapro_ctx* ctx, void* stream, int64_t rows_out, int64_t rows_in, int32_t K,
                         const int32_t* d_table, const int32_t* d_k_of /* or NULL */, int32_t c_in, int32_t c_out,
                         const float* d_x /* [rows_in, C_in] */, const float* d_weight /* [C_out, K, C_in] */,
                         const float* d_bias /* [C_out] or NULL */, float* d_y /* [rows_out, C_out] */);
int gapro_spconv_backward_input(gapro_ctx* ctx, void* stream, int64_t rows_out, int64_t rows_in, int32_t K,
                                const int32_t* d_table_t, const int32_t* d_k_of /* or NULL */, int32_t reverse_k,
                                int32_t c_in, int32_t c_out, const float* d_grad_y /* [rows_in, C_out] */,
                                const float* d_weight, float* d_grad_x /* [rows_out, C_in] or NULL */);
int gapro_spconv_backward_weight(gapro_ctx* ctx, void* stream, int64_t rows_out, int64_t rows_in, int32_t K,
                                 const int32_t* d_table, const int32_t* d_k_of /* or NULL */, int32_t c_in,
                                 int32_t c_out, const float* d_x /* [rows_in, C_in] */,
                                 const float* d_grad_y /* [rows_out, C_out] */, void* d_workspace,
                                 size_t workspace_bytes, float* d_grad_weight /* [C_out, K, C_in] or NULL */,
                                 float* d_grad_bias /* [C_out] or NULL */);

/* ------------------------------------------------------------------------------------------
 * Training sets of point-level fits (csrc/trainset.hip).  Replaces gaussian_process_utils.py:36-76 (fit_gp): a problem
 * is three lists of POINT indices, and its training set is built on the device, either by pooling each side's points
 * to superpoint means (:64-69) or by keeping the npoint_nearest points of each side nearest to the centroid of the
 * intersection's points (:39, :49-62).  The rows go straight into a table a fit launch reads with identity indices
 * (side 1's rows, then side 2's).  Exact and order-independent where the reference is not:
 *   pool     side rows = its distinct superpoints in ascending id order; a row is the mean of the side's points of that
 *            superpoint (an index listed twice counts twice): sum of rint(x 2^fixed_shift) in int64, then
 *            ldexp(sum, -fixed_shift) / count in float64, rounded once to float32 -- gapro_partition_pool's expression;
 *   nearest  centroid c = ldexp(sum of rint(x 2^coord_shift), -coord_shift) / t in float64 per axis; a side of
 *            n <= npoint_nearest points is kept in its order; a longer one keeps its npoint_nearest smallest
 *            (dx dx + dy dy) + dz dz (every operation rounded to float64 on its own), ordered by (distance, position in
 *            the side's list); rows are those points' own features.
 * d_spp_inv, n_spps and fixed_shift come from gapro_partition_prepare on the whole input; coord_shift is the same rule
 * applied to the largest |coordinate| among the FINITE coordinates of the input and n_points, computed by the call on
 * the device (a non-finite coordinate somewhere must not change the other problems' centroids).  Both scales leave room
 * for 4 N terms per sum: a list may hold at most GAPRO_TRAINSET_MAX_LIST_FACTOR N entries.
 * ---------------------------------------------------------------------------------------- */
enum {
  GAPRO_TRAINSET_POOL = 0,
  GAPRO_TRAINSET_NEAREST = 1
};
#define GAPRO_TRAINSET_MAX_NEAREST 1024
#define GAPRO_TRAINSET_MAX_LIST_FACTOR 2
#define GAPRO_TRAINSET_MAX_PROBLEMS 32767 /* of one call: grid.y = (problem, side) stays below 65 536 */

/* One problem: its lists lie back to back, [b1 (n1) | b2 (n2) | intersect (t)], at idx_offset of one int32 index array. */
typedef struct {
  int64_t idx_offset;
  int32_t n1, n2, t;     /* n1, n2 >= 1; t >= 0 */
  int32_t m1, m2;        /* in for gapro_trainset_fill: rows of the two sides -- pool: the counts gapro_trainset_count
                          * wrote; nearest: min(n, npoint_nearest) */
  int32_t reserved;      /* 0 */
  int64_t row_offset;    /* in for gapro_trainset_fill: the problem's first row in d_train / d_sel */
} gapro_trainset_desc;

/* Bytes of the workspace both calls below use for these problems (the lists' lengths bound the rows of every outcome of
 * the count; 0 on a bad argument).  n_spps is ignored in nearest mode. */
size_t gapro_trainset_workspace_bytes(int32_t mode, const gapro_trainset_desc* h_descs, int32_t n_problems,
                                      int32_t n_spps, int32_t feat_dim);
/* Pool mode, pass 1: d_counts i32[2 n_problems] = distinct superpoints of side 1 and side 2 of every problem; their
 * ranks stay in the workspace for the fill.  d_status i32[n_problems] is cleared, then GAPRO_ERR_BAD_ARG for a problem
 * with a point index outside [0, n_points).  h_descs is copied to d_descs on the stream.  Enqueue only: the caller copies
 * the counts to the host, plans m1 / m2 / row_offset from them and calls gapro_trainset_fill with the same workspace. */
int gapro_trainset_count(gapro_ctx* ctx, void* stream, int32_t n_problems, int32_t feat_dim,
                         const gapro_trainset_desc* h_descs, gapro_trainset_desc* d_descs, int64_t n_points,
                         int32_t n_spps, const int32_t* d_spp_inv, const int32_t* d_idx, void* d_workspace,
                         size_t workspace_bytes, int32_t* d_counts, int32_t* d_status);
/* The rows.  in : d_coords f64[N,3] (nearest), d_feats f32[N,D], d_spp i64[N] and d_spp_inv i32[N] (pool), d_idx.
 *   out: d_train f32[n_rows, D]; d_sel i64[n_rows]: the row's superpoint id (pool) or point index (nearest);
 *        d_status i32[n_problems] (pool: carried on from the count; nearest: cleared first): GAPRO_ERR_BAD_ARG (an index
 *        outside the points, row counts that are not the problem's), GAPRO_ERR_NOT_FINITE (nearest: a non-finite
 *        coordinate among the problem's points or a non-finite feature in one of its rows; in pool mode
 *        gapro_partition_prepare has refused such an input as a whole).  A problem never affects another.
 * npoint_nearest in [1, GAPRO_TRAINSET_MAX_NEAREST]; a problem with t = 0 and a side longer than npoint_nearest has no
 * centroid and is refused, and so is a list beyond the length bound (GAPRO_ERR_BAD_ARG, nothing is launched).
 * Enqueue only. */
int gapro_trainset_fill(gapro_ctx* ctx, void* stream, int32_t mode, int32_t n_problems, int32_t feat_dim,
                        const gapro_trainset_desc* h_descs, gapro_trainset_desc* d_descs, int64_t n_points,
                        int32_t n_spps, const double* d_coords, const float* d_feats, const int64_t* d_spp,
                        const int32_t* d_spp_inv, int32_t fixed_shift, int32_t npoint_nearest, const int32_t* d_idx,
                        void* d_workspace, size_t workspace_bytes, int64_t n_rows, float* d_train, int64_t* d_sel,
                        int32_t* d_status);

/* Which kernel gapro_svgp_fit_batch routes a fit of m = m1 + m2 inducing points to: 0 = strip-streaming
 * kernel (64 < M_p <= 128), 1 = LDS-staged kernel (128 < M_p < 512 while Z and X fit the LDS: M_p <= 192 at
 * feat_dim 32), 2 = generic kernel (feat_dim > 32), 3 = the small-fit strip kernel (M_p <= 64: 256 threads per fit,
 * two fits per CU), 4 = the cluster kernel (M_p >= 512: one fit spread over 4..32 workgroups with cluster barriers;
 * also, on one workgroup, every fit that fits neither LDS kernel), 5 = the wave-per-fit kernel (M_p <= 48 at
 * feat_dim 6: one wavefront trains one fit, eight / four fits per CU, nothing leaves the CU between the first and the
 * last Adam step).  M_p = m padded to the MFMA tile. */
int gapro_fit_route(int32_t m, int32_t feat_dim);
/* The same for a launch whose gapro_fit_options.reserved holds `flags` (GAPRO_FIT_DBG_* bits; gapro_fit_route is
 * flags = 0).  A bit outside GAPRO_FIT_DBG_ALL returns GAPRO_ERR_BAD_ARG, as the launch refuses it. */
int gapro_fit_route_flags(int32_t m, int32_t feat_dim, int32_t flags);

/* One kernel launch of a gapro_svgp_fit_batch call, as the library plans it on the host before it issues anything. */
enum {
  GAPRO_FIT_KERNEL_STRIP = 0, GAPRO_FIT_KERNEL_STAGED = 1, GAPRO_FIT_KERNEL_GENERIC = 2, GAPRO_FIT_KERNEL_SMALL = 3,
  GAPRO_FIT_KERNEL_CLUSTER = 4, GAPRO_FIT_KERNEL_WAVE = 5, /* the codes of gapro_fit_route */
  GAPRO_FIT_STEP_COPY_FREE = 8, GAPRO_FIT_MAX_STEPS = 10
};
typedef struct {
  int32_t kernel;     /* GAPRO_FIT_KERNEL_* */
  int32_t variant;    /* staged: waves per SIMD of the build (2 or 4: one or two workgroups per CU), plus
                       * GAPRO_FIT_STEP_COPY_FREE where it uses the copy-free product forms (M_p <= 256);
                       * wave: M_p / 16; else 0 */
  int32_t first;      /* the step's fits: [first, first + count) of the uploaded descriptor array */
  int32_t count;
  int32_t grid;       /* workgroups; 0 for the cluster kernel, whose block table is built when it is issued */
  int32_t stream;     /* index of the library's fit stream, or -1: the caller's stream */
  int32_t ticket;     /* counter of the launch's ticket set from which the workgroups take their fits, or -1: workgroup
                       * b runs fit b (for the cluster kernel the first of its three diagnostic counters) */
  int32_t timing;     /* timing class of gapro_fit_timing: 0 staged and generic, 1 strip, 2 small, 3 cluster, 4 wave */
  int32_t wait_gate;  /* 1: the step starts when the launch's cluster kernel has ended */
  int32_t reserved;
  int64_t lds_bytes;  /* dynamic LDS of the launch (its largest fit's); 0 where the kernel's launcher computes it */
} gapro_fit_launch_step;
/* The launches that gapro_svgp_fit_batch makes of the n_fits fits h_descs (only m1, m2 and t are read) at feature
 * width feat_dim with gapro_fit_options.reserved = flags on a device of n_cu compute units: the launch calls the same
 * planner, so this IS its launch structure.  Needs no context and no device.  steps_out receives *n_steps_out <=
 * GAPRO_FIT_MAX_STEPS records in the order of issue (cluster, generic, staged M_p > 256, staged beyond 72 KiB of LDS,
 * staged two per CU, strip, small, wave M_p = 48 / 32 / 16; a kernel without fits has no step); order_out[k]
 * (n_fits entries) is the index in h_descs of the k-th uploaded descriptor -- the groups in the order generic, staged,
 * strip, small, cluster, wave 48 / 32 / 16, each longest first and equal sizes in input order.  A bit of flags
 * outside GAPRO_FIT_DBG_ALL, a fit with an empty side, n_fits, feat_dim or n_cu <= 0, a null pointer or max_steps
 * below the number of steps return GAPRO_ERR_BAD_ARG. */
int gapro_fit_launch_plan(const gapro_fit_desc* h_descs, int32_t n_fits, int32_t feat_dim, int32_t flags, int32_t n_cu,
                          gapro_fit_launch_step* steps_out, int32_t max_steps, int32_t* n_steps_out,
                          int32_t* order_out);
/* Padded size M_p of a fit's M x M matrices (a multiple of 16; of 32 where the kernel that takes the fit needs it):
 * a function of (M, D) only, never of the routing options.  The workspace layout is built on it. */
int gapro_fit_padded_m(int32_t m, int32_t feat_dim);

/* Optional device-side timing of one fit launch (bench.py's roofline figure).  gapro_svgp_fit_batch runs
 * its kernels on streams the context owns (cluster, staged, strip and small-fit strip kernel side by side), so
 * events on the caller's stream do not bracket them.  An armed timing object makes the NEXT gapro_svgp_fit_batch
 * record HIP events around each kernel on the stream it is launched on.  gapro_fit_timing_read blocks until
 * that launch has finished: out_ms5 = {staged (+ generic) kernel ms, strip kernel ms, first start -> last end
 * ms, small-fit strip kernel ms, cluster kernel ms}; a kernel that was not launched reads 0. */
typedef struct gapro_fit_timing gapro_fit_timing;
int gapro_fit_timing_create(gapro_ctx* ctx, gapro_fit_timing** out);
void gapro_fit_timing_destroy(gapro_fit_timing* t);
int gapro_fit_timing_arm(gapro_ctx* ctx, gapro_fit_timing* t);
int gapro_fit_timing_read(gapro_ctx* ctx, gapro_fit_timing* t, float* out_ms5);
/* Milliseconds of the wave-per-fit kernels of the timed launch (route 5; first start -> last end of its up to three
 * kernels; 0 when the launch had none).  They are part of gapro_fit_timing_read's span.  Blocks like it. */
int gapro_fit_timing_read_wave(gapro_ctx* ctx, gapro_fit_timing* t, float* out_ms);
/* Diagnostics of the cluster kernel of the timed launch (blocks until it has finished; read it before 64 further
 * launches of this context): out3 = {clusters of more than one workgroup, those whose members did NOT all run on one
 * XCD (their barriers carry the L2 write-back), member workgroups}. */
int gapro_fit_timing_cluster_info(gapro_ctx* ctx, gapro_fit_timing* t, int32_t* out3);
/* Where launch t lies on the time axis of launch ref: out_ms2 = {first kernel start, last kernel end} of t in ms after
 * the start event of ref's first kernel.  Consecutive launches of a pipeline overlap (the next one is enqueued while
 * the tail of the previous one runs, and a start event fires when its stream reaches it, not when the kernel gets
 * CUs): bench.py counts the overlapped time once when it averages launch durations.  Blocks until t has finished. */
int gapro_fit_timing_offsets(gapro_ctx* ctx, gapro_fit_timing* ref, gapro_fit_timing* t, float* out_ms2);

/* ------------------------------------------------------------------------------------------
 * Scene / label files (host; no device, no ctx, no Python objects -- callable from any thread without the GIL).
 * Replaces the `torch.load` of gen_ps.py:45-46 (scene tuple written by ISBNet/dataset/scannetv2/prepare_data_inst.py:104,
 * superpoint ids written by prepare_superpoint.py:27) and the `torch.save` of gen_ps.py:132.
 *
 * A torch.save()d NumPy array / tuple of NumPy arrays is a stored zip whose data.pkl (pickle protocol 2) holds every
 * array buffer as latin-1 text re-encoded as UTF-8; unpickling it costs ~25 ms of a core per ScanNet scene under the GIL.
 * gapro_pth_open maps the file and walks the pickle; gapro_pth_read transcodes one array's payload back to bytes
 * straight into the caller's buffer (e.g. pinned staging memory).  GAPRO_ERR_UNSUPPORTED = well-formed but not handled
 * here: the caller falls back to torch.load.  Errors: gapro_pth_last_error() (thread-local text).
 * ---------------------------------------------------------------------------------------- */
typedef struct gapro_pth_file gapro_pth_file;
typedef struct gapro_pth_array {
  int32_t kind;      /* NumPy dtype kind character: 'f', 'i', 'u' or 'b' (bool) */
  int32_t itemsize;  /* bytes per element: 1, 2, 4 or 8 (little-endian) */
  int32_t ndim;      /* 0..4 */
  int32_t encoded;   /* read: 1 = stored as UTF-8 text (protocol 2), 0 = raw bytes (protocol >= 3); ignored on write */
  int64_t shape[4];  /* C order; entries beyond ndim are 1 */
  int64_t nbytes;    /* prod(shape) * itemsize */
} gapro_pth_array;
int gapro_pth_open(const char* path, gapro_pth_file** out);
/* number of arrays (1 for a bare array), and whether the top-level object is a tuple / list */
int gapro_pth_count(const gapro_pth_file* f);
int gapro_pth_is_sequence(const gapro_pth_file* f);
int gapro_pth_info(const gapro_pth_file* f, int32_t index, gapro_pth_array* out);
/* decode array `index` into h_dst; dst_bytes must equal its nbytes */
int gapro_pth_read(const gapro_pth_file* f, int32_t index, void* h_dst, int64_t dst_bytes);
void gapro_pth_close(gapro_pth_file* f);
/* Write n_arrays host arrays as one torch.load()-able file (tuple when as_tuple, else the single bare array):
 * stored zip, protocol-2 pickle naming numpy.core.multiarray (importable by NumPy 1.x and 2.x); written to a
 * temporary name in the same directory and renamed (atomic). */
int gapro_pth_write(const char* path, int32_t n_arrays, const gapro_pth_array* descs, const void* const* h_data,
                    int32_t as_tuple);
const char* gapro_pth_last_error(void);
/* which UTF-8 -> byte transcoder this process uses: "avx512" (VBMI2), "bmi2" or "scalar" (GAPRO_PTH_DECODER pins one;
 * a tier the CPU lacks falls back to the next) */
const char* gapro_pth_decoder(void);
/* the writer's tiers: byte -> UTF-8 transcoder "avx512" / "bmi2" / "scalar" (GAPRO_PTH_ENCODER pins one) and zip CRC-32
 * "clmul" (PCLMULQDQ folding) / "table" (slice-by-8; GAPRO_PTH_CRC pins one) */
const char* gapro_pth_encoder(void);
const char* gapro_pth_crc(void);
/* the two writer primitives on their own (tests hold every tier to the scalar one): CRC-32 of n bytes; latin-1 -> UTF-8
 * of n bytes into dst (dst_cap >= 2 n + 64), returns the encoded length or a negative gapro_status */
uint32_t gapro_pth_crc32(const void* data, int64_t n);
int64_t gapro_pth_encode_latin1(const void* src, int64_t n, void* dst, int64_t dst_cap);
/* The reference's default features (gen_ps.py:55: np.concatenate([xyz, rgb], -1) of the UN-aligned coordinates, uploaded
 * as float32 at :84): h_feats[n][6] = float32 of [xyz | rgb], one pass on the host. */
int gapro_scene_default_feats(const double* h_xyz, const double* h_rgb, int64_t n_points, float* h_feats);
/* getInstanceInfo (gen_ps_utils.py:195-239) on the HOST in one pass, without the corner labels: boxes
 * h_box[n_boxes][6] = (min xyz, max xyz), class h_cls (ScanNet: -2 unless -100), volume h_vol, indexed by the rank among
 * the non-empty instance ids; *instance_num = max id + 1.  cap = rows the output arrays hold; GAPRO_ERR_BAD_ARG with
 * *instance_num set when it is too small.  For loader threads: the device form (gapro_instance_info) is a kernel and
 * would wait for a running fit launch to drain. */
int gapro_scene_instance_boxes(const double* h_xyz, const double* h_inst, const double* h_sem, int64_t n_points,
                               int32_t scannet, int32_t cap, double* h_box, double* h_cls, double* h_vol,
                               int32_t* n_boxes, int32_t* instance_num);

/* ------------------------------------------------------------------------------------------
 * Batch feeder of the gen_ps driver (host threads of the library's own; no Python objects, no GIL; csrc/feeder.hip).
 * Replaces the per-scene host half of gen_ps.py:36-132: torch.load of the scene tuple and the superpoint ids (:45-46),
 * the default features from the UN-aligned points (:55), the axis alignment (:58-69), getInstanceInfo (:71-77), the
 * upload (:83-87), and on the way out the device -> host copies and torch.save of the 5-tuple (:126-132).
 *
 *   submit    scene / superpoint / alignment (/ feature) file paths, in the order the scenes are wanted
 *   poll      wait until the next scenes of that order are loaded into pinned memory; how many, and the device bytes
 *   upload    one asynchronous copy per scene into the caller's device slab on the feed's own stream; records out
 *   batch_wait  make a stream wait for a batch's copies
 *   export    label files: device -> host behind the caller's event, gapro_pth_write; export_wait collects them
 *
 * device < 0: host-only mode (gen_ps --dry_run): pageable memory, no copies; `upload` hands out host images and
 * `export` takes host pointers.  Scenes the native reader does not handle come back with status GAPRO_ERR_UNSUPPORTED
 * (the caller reads them its own way); a scene without instances has n_instances == 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct gapro_feed gapro_feed;
typedef struct gapro_feed_scene {
  int32_t status;        /* gapro_status of the load */
  int32_t n_points;      /* N */
  int32_t n_instances;   /* instance boxes found (getInstanceInfo's non-empty ids) */
  int32_t feat_dim;      /* D: 6 (xyz + rgb) or the width of the feature file */
  /* byte offsets of the scene's arrays in the device slab of its upload (256-byte aligned):
   * coords f64[N,3] (aligned), feats f32[N,D], spp i64[N], sem f64[N], inst f64[N] (the file's label arrays) */
  int64_t off_coords, off_feats, off_spp, off_sem, off_inst;
  const double* inst_box;  /* f64[n_instances,6] (min xyz, max xyz), inst_cls f64[n_instances], inst_vol f64[n_instances]: */
  const double* inst_cls;  /* host memory of the feed, valid until the next gapro_feed_upload                            */
  const double* inst_vol;
  void* host_image;      /* host-only mode: base address the offsets are relative to (valid until release_batch) */
} gapro_feed_scene;
typedef struct gapro_feed_out {
  const void* d_sem;     /* i32[n_points] */
  const void* d_inst;    /* i32[n_points] */
  const void* d_prob;    /* f32[n_points] */
  const void* d_mu;      /* f32[n_mu] */
  const void* d_var;     /* f32[n_mu] */
  int64_t n_points, n_mu;
  const char* path;      /* label file to write (atomically) */
} gapro_feed_out;
/* n_threads loader / writer threads; budget_bytes caps the pinned memory of scenes loaded but not yet uploaded (plus
 * label files being written); default_feat_dim = 6 */
int gapro_feed_create(int32_t device, int32_t n_threads, int64_t budget_bytes, int32_t default_feat_dim,
                      gapro_feed** out);
void gapro_feed_destroy(gapro_feed* f);
/* Stop the threads and leave everything else to the end of the process: unpinning the staging pool of a worker takes
 * ~0.6 s (8 GB), which a process that is about to exit need not spend.  The handle must not be used afterwards. */
void gapro_feed_detach(gapro_feed* f);
const char* gapro_feed_last_error(const gapro_feed* f);
/* feat_paths may be NULL (default features), and so may its entries */
int gapro_feed_submit(gapro_feed* f, int32_t n, const char* const* scene_paths, const char* const* spp_paths,
                      const char* const* align_paths, const char* const* feat_paths);
/* no further submit: polls stop waiting for scenes that will never come */
int gapro_feed_close(gapro_feed* f);
/* Block until min_ready scenes at the head of the order are loaded (fewer when the feed is closed and runs out, or
 * when the byte budget holds fewer: the call then returns what IS loaded as soon as no loader can make progress
 * without the caller taking it -- it never waits for a count the budget cannot hold), or timeout_ms passed (< 0: no
 * limit); *n_ready = loaded scenes in a row from the head (<= max_scenes), *slab_bytes the device bytes their images
 * need. */
int gapro_feed_poll(gapro_feed* f, int32_t min_ready, int32_t max_scenes, int32_t timeout_ms, int32_t* n_ready,
                    int64_t* slab_bytes);
/* The next n loaded scenes: copies into d_slab (slab_bytes >= what poll reported for them), out[n], *batch_id.  The
 * copies run on the feed's own stream behind everything queued so far on slab_stream (hipStream_t; NULL = the default
 * stream): the stream the slab was allocated on when it comes from a stream-ordered / caching allocator.  Sizes and
 * states are validated before anything changes; after a HIP failure (GAPRO_ERR_HIP) the feed refuses further calls. */
int gapro_feed_upload(gapro_feed* f, int32_t n, void* d_slab, int64_t slab_bytes, void* slab_stream, gapro_feed_scene* out,
                      int64_t* batch_id);
int gapro_feed_batch_wait(gapro_feed* f, int64_t batch_id, void* stream);
/* host-only mode: the images of a batch are no longer needed (device mode: recycles completed batches) */
int gapro_feed_release_batch(gapro_feed* f, int64_t batch_id);
/* Queue n label files.  ready_event (hipEvent_t or NULL): recorded by the caller behind the kernels that produce the
 * arrays; they must stay valid until gapro_feed_export_wait has counted the scene. */
int gapro_feed_export(gapro_feed* f, int32_t n, const gapro_feed_out* items, void* ready_event);
/* wait until the first `until_done` label files in submission order (< 0: all queued so far) are written or failed;
 * *n_done = files finished as a CONTIGUOUS PREFIX of the submission order: the arrays of export k may be released
 * when n_done > k, whatever later exports have finished already */
int gapro_feed_export_wait(gapro_feed* f, int64_t until_done, int32_t timeout_ms, int64_t* n_done, int64_t* n_failed);
int gapro_feed_export_error(gapro_feed* f, int32_t index, char* buf, int32_t cap);
/* where the feeder threads' time went, summed over threads: out8 = {s inside the staging allocations, blocks, bytes,
 * s inside scene loads, scenes, s inside label writes, files, s from create to the first loaded scene} */
int gapro_feed_stats(gapro_feed* f, double* out8);

/* ------------------------------------------------------------------------------------------
 * Device memory, streams, events owned by the library (round 6; csrc/devmem.hip).  SURVEY.md 8b: "library owns an
 * opaque ctx: device, stream, workspace arena".  A caller without torch (the gen_ps workers: gapro_amd/devmem.py) gets
 * everything the path needs from here; the torch-tensor API shims keep using torch's allocator and streams.
 * The reference has no counterpart: its tensors come from torch (gen_ps.py:79-89).
 * ---------------------------------------------------------------------------------------- */
/* Caching arena with stream-ordered reuse: a block is allocated FOR a stream (hipStream_t; NULL = the default stream)
 * and, once freed, is only handed out again for that stream, so gapro_dev_free never waits for the device.  A block
 * used on a second stream must be ordered by events before it is freed. */
int gapro_dev_alloc(gapro_ctx* ctx, size_t bytes, void* stream, void** out);
int gapro_dev_free(gapro_ctx* ctx, void* p);
int gapro_dev_trim(gapro_ctx* ctx);   /* give every cached block back to the driver (synchronises the device) */
int gapro_dev_stats(gapro_ctx* ctx, int64_t* reserved_bytes, int64_t* in_use_bytes, int64_t* device_free_bytes,
                    int64_t* device_total_bytes);   /* any pointer may be NULL */
int gapro_host_alloc(gapro_ctx* ctx, size_t bytes, void** out);   /* page-locked host memory */
int gapro_host_free(gapro_ctx* ctx, void* p);
int gapro_stream_create(gapro_ctx* ctx, void** out);              /* non-blocking stream on the context's device */
int gapro_stream_destroy(gapro_ctx* ctx, void* stream);
int gapro_stream_sync(gapro_ctx* ctx, void* stream);
int gapro_device_sync(gapro_ctx* ctx);
int gapro_event_create(gapro_ctx* ctx, int32_t timing, void** out);
int gapro_event_destroy(gapro_ctx* ctx, void* ev);
int gapro_event_record(gapro_ctx* ctx, void* ev, void* stream);
int gapro_stream_wait_event(gapro_ctx* ctx, void* stream, void* ev);
int gapro_event_sync(gapro_ctx* ctx, void* ev);
int gapro_event_query(gapro_ctx* ctx, void* ev);                  /* 1 complete, 0 not yet, < 0 gapro_status */
int gapro_event_elapsed_ms(gapro_ctx* ctx, void* ev_start, void* ev_end, float* out_ms);
/* kind: 0 host -> device, 1 device -> host, 2 device -> device */
int gapro_memcpy_async(gapro_ctx* ctx, void* dst, const void* src, size_t bytes, int32_t kind, void* stream);
int gapro_memset_async(gapro_ctx* ctx, void* dst, int32_t value, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Inspection (tests): where a fit's trained parameters live in its workspace.  The measurement / self-test entry points
 * (gapro_debug_*) are NOT part of this library: include/gapro_hip_debug.h, libgapro_hip_debug.so.
 * ---------------------------------------------------------------------------------------- */
/* Offsets (doubles, relative to a fit's ws_offset) of the fit's workspace regions, so tests can
 * inspect trained parameters: out8 = {Mp, matrices, vectors, X/Z block, test points, Dinv blocks,
 * scalars, total}.  Matrices are Mp x Mp row-major in the order LS, LS^T, Adam m/v of LS, G_LS, L,
 * L^T, L^-1, L^-T, KX, A, A^T, B, B^T, G_A, G_KX, G_KX^T; scalars: c, rho_s, rho_l, ... , loss.
 * Which of the intermediate slots a fit fills depends on its kernel (the single-workgroup MFMA kernels keep L^T but
 * not L, and up to M_p = 256 no A^T / B^T): trained parameters -- L_S, m (vector 1), Z, the scalars -- always. */
int gapro_fit_workspace_layout(int32_t m, int32_t t, int32_t feat_dim, int64_t* out8);

#ifdef __cplusplus
}
#endif
#endif /* GAPRO_HIP_H */
