"""Host orchestration of the pseudo-label path on one GPU: enumerate -> batch-fit -> ordered merge.

Mirrors what reference gapro/gen_ps_utils.py:293-482 does for one scene, but staged so that any
number of scenes share each device launch:

  stage A  gapro_partition_prepare   scene stats + dense superpoint ranks        (device)
  stage B  gapro_partition_pool      membership + pooling in one pass            (device)
  stage C  gapro_schedule_build      static pair schedule                         (host, C++)
  stage D  gapro_svgp_fit_batch      every GP fit of every scene in ONE launch    (device)
  stage E  gapro_schedule_merge      ordered merge, fallback, label tables        (host, C++)
  stage F  gapro_broadcast_labels    superpoint -> point                          (device)
  stage G  gapro_point_refine_*      opt-in (point_level), in point_level.py: every point of a GP-labelled superpoint
                                     predicted from its own features by the model that won the superpoint (device;
                                     planned on the host: refine_plan, then refine_chain for every mode)
                                     ("compete": by every fit that tested the superpoint, the merge replayed per point;
                                      "vote": that, then the superpoint takes the box most of its points chose -- in
                                      front of stage F, which broadcasts the voted tables)

All arithmetic happens in libgapro_hip.so.  Device memory, streams and events come from a backend (devmem.py): torch's
(default: the Python API shims take and return torch tensors) or the library's own arena ("native": the gen_ps workers,
which then never import torch -- round 6).
"""
from __future__ import annotations

import os
import ctypes as C
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import FitDesc, SceneHeader, SceneTask, ScheduleCounts
from .fit_runner import FitRunner, PendingFit, _host, _ptr, _to_np
from .gp_model import SceneFit, state_doubles
from .point_level import (BLOCK_DTYPE, SEGMENT_DTYPE, plan_point_compete, plan_point_winner,  # noqa: F401 (re-exported)
                          point_level_kw, point_mode, refine_chain, refine_plan)


class LazyViews(dict):
    """Per-scene views into the batch-wide buffers, created on first access: a batch of 256 scenes would otherwise
    pay thousands of tensor-view constructions on the host between two fit launches; the kernels only need the
    addresses, which are plain integer arithmetic."""

    def __init__(self):
        super().__init__()
        self._specs = {}

    def spec(self, name, buf, off, nbytes, dtype, shape):
        self._specs[name] = (buf, off, nbytes, dtype, shape)
        self.pop(name, None)
        return buf.data_ptr() + off

    def __missing__(self, name):
        buf, off, nbytes, dtype, shape = self._specs[name]
        v = buf[off:off + nbytes].view(dtype).view(*shape)
        self[name] = v
        return v

    def __contains__(self, name):
        return dict.__contains__(self, name) or name in self._specs


@dataclass
class SceneJob:
    """Inputs of one gen_pseudo_label_gaussian_process call (reference gen_ps_utils.py:293-307)."""
    coords: object  # f64[N,3] device (torch.Tensor or devmem.DevBuf)
    feats: object  # f32[N,D] device
    spp: object  # i64[N] device
    instance_cls: np.ndarray  # i64[Bi]
    instance_box: np.ndarray  # f32[Bi,6]
    instance_box_volume: np.ndarray  # f32[Bi]
    wall_box: np.ndarray  # f32[Bw,6] (may be empty)
    wall_box_volume: np.ndarray  # f32[Bw]
    instance_classes: int = 18
    ground_h: float = 0.1
    thresh_spp_occu: float = 0.8
    # --- filled by the stages ---
    header: Optional[SceneHeader] = None
    n_spps: int = 0
    boxes: Optional[np.ndarray] = None
    boxes_cls: Optional[np.ndarray] = None
    boxes_volume: Optional[np.ndarray] = None
    feats_row_base: int = 0
    dev: dict = field(default_factory=LazyViews)
    host: dict = field(default_factory=LazyViews)
    schedule: Optional[C.c_void_p] = None
    counts: Optional[ScheduleCounts] = None
    fit_base: int = 0
    out_base: int = 0
    outputs: Optional[tuple] = None
    error: Optional[Exception] = None  # why the scene could not be processed (Pipeline.strict = False)
    # Pipeline.run(..., keep_models=True): pooled features f32[S, D] (NumPy) and the scene's fits in schedule order as
    # (b1, b2, train superpoint ranks [b1_inds | b2_inds], test superpoint ranks, GPModel)
    feats_spp: Optional[np.ndarray] = None
    fits: Optional[list] = None
    winner: Optional[np.ndarray] = None  # keep_models: i32[S] index into fits of the fit that labelled the superpoint, or -1
    point_fit: Optional[np.ndarray] = None  # keep_models + point_level="compete": i32[N] fit that labelled the point, or -1
    vote_box: Optional[np.ndarray] = None  # keep_models + point_level="vote": i32[S] the box the points chose, or -1
    vote_count: Optional[np.ndarray] = None  # ... and its votes, 0 where the superpoint was not voted on
    scene_key: int = 0  # stable id of the scene (e.g. crc32 of the scan name): seeds the optional initial-mean noise

    @property
    def spp_inv(self):
        """i32[N] dense superpoint rank of every point (view into the batch-wide buffer, created on demand)."""
        return self.dev["spp_inv"] if "spp_inv" in self.dev else None

    @property
    def n_points(self):
        return int(self.coords.shape[0])

    @property
    def n_boxes(self):
        return int(self.boxes.shape[0])


def make_job(coords_float, mask_feats, spp, instance_cls, instance_box, instance_box_volume, wall_box,
             wall_box_volume, instance_classes=18, ground_h=0.1, thresh_spp_occu=0.8, device=None,
             scene_key: int = 0, backend=None) -> SceneJob:
    """backend: a devmem.NativeBackend (arrays are its device buffers or host arrays; no torch), else torch."""
    if backend is not None and backend.name == "native":
        def dev(x, dtype):
            if backend.is_device_array(x):
                if x.dtype != np.dtype(dtype):
                    raise ValueError("device buffer of dtype %s where %s is expected" % (x.dtype, np.dtype(dtype)))
                return x
            return backend.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=dtype))

        f64, f32, i64 = np.float64, np.float32, np.int64
    else:
        import torch

        device = torch.device(device if device is not None else "cuda:0")

        def dev(x, dtype):
            t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
            return t.to(device=device, dtype=dtype, non_blocking=True).contiguous()

        f64, f32, i64 = torch.float64, torch.float32, torch.int64
    coords = dev(coords_float, f64)
    feats = dev(mask_feats, f32)  # mask_feats.float()  gen_ps_utils.py:315
    if feats.dim() != 2 or coords.dim() != 2 or coords.shape[1] != 3 or feats.shape[0] != coords.shape[0]:
        raise ValueError("coords_float must be [N,3] and mask_feats [N,D]")
    sp = dev(spp, i64).reshape(-1)
    if sp.shape[0] != coords.shape[0]:
        raise ValueError("spp must have one id per point")
    ibox = _to_np(instance_box, np.float32).reshape(-1, 6)
    has_wall = wall_box is not None and len(wall_box) > 0
    return SceneJob(coords, feats, sp, _to_np(instance_cls, np.int64).reshape(-1), ibox,
                    _to_np(instance_box_volume, np.float32).reshape(-1),
                    _to_np(wall_box, np.float32).reshape(-1, 6) if has_wall else np.zeros((0, 6), np.float32),
                    _to_np(wall_box_volume, np.float32).reshape(-1) if has_wall else np.zeros((0,), np.float32),
                    int(instance_classes), float(ground_h), float(thresh_spp_occu), scene_key=int(scene_key))


@dataclass
class BatchState:
    """A batch on its way through the stages: _partition creates it, _schedule_all and _launch fill it, _finish ends it."""
    jobs: list  # the scenes that passed stage A
    all_jobs: list  # every scene of the batch, rejected ones included
    stream: object
    slot: str  # name of the stream's buffers (pinned staging, workspace)
    mark: Callable  # _marker of the batch
    tasks: object  # gapro_scene_task array (host) and its device mirror
    d_tasks: object
    keep_debug: bool = False
    keep_models: bool = False
    feats_spp_all: object = None  # stage B: pooled features f32[sum S, D] of every scene
    n_fits: int = 0  # stage C: the fit descriptors of the whole batch and their index array
    n_out: int = 0
    descs: object = None
    h_idx: Optional[np.ndarray] = None
    pending: Optional[PendingFit] = None  # stage D: the launch in flight


class Pipeline(FitRunner):
    def __init__(self, device=0, training_iter=50, init_mean_std=0.0, seed=0, eval_stale_chol=False,
                 spp_range_cap=None, force_staged=False, precision="f64", cluster_all=False, backend="torch",
                 point_level=False):
        mode = point_mode(point_level)  # refused before a context is made
        super().__init__(device, training_iter, init_mean_std, seed, eval_stale_chol, force_staged, precision,
                         cluster_all, backend)
        self.spp_range_cap = spp_range_cap
        # point_level: after the ordered merge every point of a superpoint that a GP fit labelled is predicted from its
        # own feature row by the model that won the superpoint (point_level.py: refine_plan / refine_chain, one chain
        # for every mode); all five outputs are then point-length.  Off (the default): nothing of it runs.  True /
        # "winner": that model alone (plan_point_winner).  "compete": every fit that TESTED the superpoint is evaluated at
        # every point of it and the merge's rule is replayed per point (plan_point_compete).
        # "vote": the chain of "compete" up to its predict launch, then every refined superpoint takes the box most of its
        # points chose (the chain runs in FRONT of the label broadcast): the outputs keep the default path's lengths.
        self.point_level = mode is not None
        self.point_mode = mode
        self.point_outputs = mode in ("winner", "compete")  # all five outputs at point length
        if self.point_level and not self.serialize_fits:
            # the fit launches keep their states on the device, which the library allows on one stream per context at
            # a time: the pipeline's three streams qualify only while launch i + 1 waits for launch i
            raise ValueError("point_level needs serialised fit launches (GAPRO_OVERLAP_FITS is set)")
        self.last_refine = {}  # point_level: refined superpoints, rows, models and host seconds of the last batch's plan
        self._ident_rows = None
        # strict: a scene that cannot be processed (non-finite input, id range beyond the rank table, a GP fit that
        # fails after the jitter retries) raises, as the reference would.  The gen_ps driver clears it: the scene's
        # outputs come back as None with job.error set, and the other scenes of the batch are unaffected.
        self.strict = True
        self.last_stats = {}
        # with profile_fit: torch events (current stream = the stream the kernels are launched on) around the batched
        # partition calls: dicts with 'prepare', 'pool', 'broadcast' -> (start, end) and the points they cover
        self.part_events = []
        self.profile_stages = False  # bench.py --stage-times: synchronising per-stage wall clock
        self.stage_times = {}
        self._pin_events = {}
        self._keep = {}


    # ------------------------------------------------------------------ batched partition plumbing
    def _task_array(self, jobs: Sequence[SceneJob]):
        """One gapro_scene_task per scene (host ctypes array + its device mirror), created once per batch and
        refilled stage by stage."""
        tasks = (SceneTask * len(jobs))()
        for t, job in zip(tasks, jobs):
            t.n_points = job.n_points
            t.coords, t.feats, t.spp = job.coords.data_ptr(), job.feats.data_ptr(), job.spp.data_ptr()
        d_tasks = self.be.empty(len(jobs) * C.sizeof(SceneTask))
        return tasks, d_tasks

    @staticmethod
    def _carve(sizes, align=256):
        """Offsets of consecutive `align`-aligned regions of the given byte sizes, and the total."""
        offs, tot = [], 0
        for sz in sizes:
            offs.append(tot)
            tot += (int(sz) + align - 1) // align * align
        return offs, max(tot, align)

    def _part_event(self, jobs, name):
        if not self.profile_fit:
            return None
        e0 = self.be.event(enable_timing=True)
        e0.record(self.be.current_stream())
        return dict(name=name, start=e0, points=sum(j.n_points for j in jobs), feat_dim=int(jobs[0].feats.shape[1]))

    def _part_event_end(self, ev):
        if ev is not None:
            ev["end"] = self.be.event(enable_timing=True)
            ev["end"].record(self.be.current_stream())
            self.part_events.append(ev)

    # ------------------------------------------------------------------ stage A
    def _prepare_finish(self, job: SceneJob, hdr: SceneHeader):
        if hdr.status != 0:
            msg = "scene has a non-finite coordinate or feature" if hdr.status == _lib.GAPRO_ERR_NOT_FINITE else \
                "superpoint id range [%d, %d] exceeds the rank table (%d slots)" % (hdr.spp_min, hdr.spp_max,
                                                                                    job.host["range_cap"])
            job.error = _lib.GaproError(int(hdr.status), msg)
            if self.strict:
                raise job.error
            return
        job.header = hdr
        job.n_spps = int(hdr.n_spps)
        job.dev.pop("prep_ws", None)
        # boxes = cat(instance, wall, floor) with torch's dtype promotion (gen_ps_utils.py:317-345); the instance
        # and wall rows do not depend on the scene statistics and are assembled once per job
        st = job.host.get("_static")
        if st is None:
            nw = len(job.wall_box)
            st = (np.concatenate([job.instance_box.astype(np.float64), job.wall_box.astype(np.float64),
                                  np.zeros((1, 6))], 0),
                  np.ascontiguousarray(np.concatenate([job.instance_cls,
                                                       np.full(nw + 1, job.instance_classes, dtype=np.int64)])),
                  np.concatenate([job.instance_box_volume.astype(np.float64), job.wall_box_volume.astype(np.float64),
                                  np.zeros(1)]))
            dict.__setitem__(job.host, "_static", st)
        mn, mx = hdr.coord_min, hdr.coord_max
        boxes, vol = st[0].copy(), st[2].copy()
        boxes[-1] = (mn[0], mn[1], mn[2], mx[0], mx[1], mn[2] + job.ground_h)
        floor = boxes[-1]
        vol[-1] = max(floor[3] - floor[0], 0.001) * max(floor[4] - floor[1], 0.001) * max(floor[5] - floor[2], 0.001)
        job.boxes, job.boxes_cls, job.boxes_volume = boxes, st[1], vol

    def _prepare(self, job: SceneJob):
        """Single-scene, blocking form (tests)."""
        self._prepare_all([job])

    def _prepare_all(self, jobs: Sequence[SceneJob]):
        """Scene statistics + dense superpoint ranks of every scene: one launch per kernel, one sync."""
        lib, be = self.lib, self.be
        tasks, d_tasks = self._task_array(jobs)
        D = int(jobs[0].feats.shape[1])
        caps = [int(self.spp_range_cap) if self.spp_range_cap else max(4 * j.n_points, 1 << 20) for j in jobs]
        ws_off, ws_tot = self._carve([lib.gapro_partition_prepare_workspace_bytes(j.n_points, c)
                                      for j, c in zip(jobs, caps)])
        prep_ws = be.empty(ws_tot)
        inv_off, inv_tot = self._carve([4 * j.n_points for j in jobs])
        spp_inv_all = be.empty(inv_tot)
        hsz = C.sizeof(SceneHeader)
        d_headers = be.empty(len(jobs) * hsz)
        pinned = self._pinned("headers%x" % int(be.current_stream().cuda_stream), len(jobs) * hsz)
        for t, job, cap, wo, io in zip(tasks, jobs, caps, ws_off, inv_off):
            t.spp_inv = job.dev.spec("spp_inv", spp_inv_all, io, 4 * job.n_points, be.i32, (job.n_points,))
            dict.__setitem__(job.host, "range_cap", cap)
            t.prepare_ws, t.spp_range_cap = prep_ws.data_ptr() + wo, cap
        ev = self._part_event(jobs, "prepare")
        self.ctx.check(lib.gapro_partition_prepare_batch(
            self.ctx.handle, self._sh(), len(jobs), D, C.cast(tasks, C.c_void_p), _ptr(d_tasks),
            _ptr(d_headers), _ptr(pinned)))
        self._part_event_end(ev)
        be.current_stream().synchronize()  # one sync for the whole batch
        raw = pinned.numpy()
        for i, job in enumerate(jobs):
            self._prepare_finish(job, SceneHeader.from_buffer_copy(raw[i * hsz:(i + 1) * hsz].tobytes()))
        good = [i for i, job in enumerate(jobs) if job.error is None]
        if len(good) != len(jobs):  # non-strict: the rejected scenes leave the batch here
            tasks2 = (SceneTask * max(len(good), 1))()
            for k, i in enumerate(good):
                tasks2[k] = tasks[i]
            tasks = tasks2
            d_tasks = be.empty(max(len(good), 1) * C.sizeof(SceneTask))
        return tasks, d_tasks

    # ------------------------------------------------------------------ stage B
    def _pool(self, job: SceneJob, feats_spp_all, stage=None, off: int = 0):
        """Single-scene form (tests)."""
        tasks, d_tasks = self._task_array([job])
        tasks[0].spp_inv = job.spp_inv.data_ptr()
        self._pool_all([job], tasks, d_tasks, feats_spp_all, stage)

    def _pool_all(self, jobs: Sequence[SceneJob], tasks, d_tasks, feats_spp_all, stage=None):
        """Fused membership + pooling of every scene: one launch per kernel; the two small tables the host
        scheduler needs (occ_bits, n_bbs) of all scenes come back in ONE device-to-host copy (no sync here)."""
        lib, be = self.lib, self.be
        D = int(jobs[0].feats.shape[1])
        # boxes of every scene: one pinned staging buffer, one upload
        box_off, box_tot = self._carve([j.boxes.nbytes for j in jobs], 64)
        slot = "%x" % int(be.current_stream().cuda_stream)
        h_boxes = self._pinned("boxes" + slot, box_tot)
        hb = h_boxes.numpy()
        for job, bo in zip(jobs, box_off):
            hb[bo:bo + job.boxes.nbytes] = job.boxes.view(np.uint8).reshape(-1)
        d_boxes = be.empty(box_tot)
        d_boxes.copy_(h_boxes[:box_tot], non_blocking=True)
        # host-visible tables [occ_bits | n_bbs] per scene, laid out exactly like the pinned staging area
        # (point_level: point_count rides along -- the host plans the row table of the predict launch from it)
        pl = 4 if self.point_level else 0
        tab_sizes = [j.n_spps * (((j.n_boxes + 63) // 64) * 8 + 4 + pl) for j in jobs]
        tab_off, tab_tot = self._carve(tab_sizes, 16)
        d_tables = be.empty(tab_tot)
        # integer tallies [feat_sum i64 | occ_count i32 | point_count i32] per scene
        tal_sizes = [j.n_spps * (8 * D + 4 * j.n_boxes + 4 - pl) for j in jobs]
        tal_off, tal_tot = self._carve(tal_sizes, 16)
        d_tallies = be.empty(tal_tot)
        if stage is None:
            stage = be.pinned(tab_tot)
        fbase, fstride = feats_spp_all.data_ptr(), 4 * D
        for t, job, bo, to, ao in zip(tasks, jobs, box_off, tab_off, tal_off):
            S, B = job.n_spps, job.n_boxes
            W = (B + 63) // 64
            d = job.dev
            t.boxes = d.spec("boxes", d_boxes, bo, job.boxes.nbytes, be.f64, (B, 6))
            t.feat_sum = d.spec("feat_sum", d_tallies, ao, 8 * S * D, be.i64, (S, D))
            t.occ_count = d.spec("occ_count", d_tallies, ao + 8 * S * D, 4 * S * B, be.i32, (S, B))
            if pl:
                t.point_count = d.spec("point_count", d_tables, to + 8 * S * W + 4 * S, 4 * S, be.i32, (S,))
            else:
                t.point_count = d.spec("point_count", d_tallies, ao + 8 * S * D + 4 * S * B, 4 * S, be.i32, (S,))
            t.occ_bits = d.spec("occ_bits", d_tables, to, 8 * S * W, be.i64, (S, W))
            t.n_bbs = d.spec("n_bbs", d_tables, to + 8 * S * W, 4 * S, be.i32, (S,))
            t.feats_spp = fbase + job.feats_row_base * fstride
            dict.__setitem__(d, "feats_spp", None)
            d._specs["feats_spp"] = (feats_spp_all.view(be.u8).view(-1), job.feats_row_base * fstride, S * fstride,
                                     be.f32, (S, D))
            dict.pop(d, "feats_spp", None)
            t.n_boxes, t.n_spps = B, S
            t.fixed_shift, t.thresh_spp_occu = int(job.header.fixed_shift), float(job.thresh_spp_occu)
            h = job.host
            h.spec("occ_bits_pin", stage, to, 8 * S * W, be.i64, (S, W))
            h.spec("n_bbs_pin", stage, to + 8 * S * W, 4 * S, be.i32, (S,))
            if pl:
                h.spec("point_count_pin", stage, to + 8 * S * W + 4 * S, 4 * S, be.i32, (S,))
        ev = self._part_event(jobs, "pool")
        self.ctx.check(lib.gapro_partition_pool_batch(self.ctx.handle, self._sh(), len(jobs), D,
                                                      C.cast(tasks, C.c_void_p), _ptr(d_tasks)))
        self._part_event_end(ev)
        stage[:tab_tot].copy_(d_tables, non_blocking=True)

    # ------------------------------------------------------------------ stage C
    def _host_threads(self):
        if getattr(self, "_host_pool", None) is None:
            import concurrent.futures as cf

            self._host_pool = cf.ThreadPoolExecutor(max_workers=max(2, min(16, (os.cpu_count() or 4) // 8)))
        return self._host_pool

    def _schedule(self, job: SceneJob):
        h = job.host
        h["occ_bits"] = np.ascontiguousarray(h["occ_bits_pin"].numpy().view(np.uint64))
        h["n_bbs"] = np.ascontiguousarray(h["n_bbs_pin"].numpy())
        if "point_count_pin" in h:
            h["point_count"] = h["point_count_pin"].numpy().copy()  # read at the END of the batch: not a view of the stage
        sched = C.c_void_p()
        rc = self.lib.gapro_schedule_build(job.n_spps, job.n_boxes, _ptr(job.boxes), _ptr(h["occ_bits"]),
                                           _ptr(h["n_bbs"]), C.byref(sched))
        if rc != 0:
            raise _lib.GaproError(rc, "gapro_schedule_build")
        job.schedule = sched
        cnt = ScheduleCounts()
        self.lib.gapro_schedule_get_counts(sched, C.byref(cnt))
        job.counts = cnt

    # ------------------------------------------------------------------ run
    def run(self, jobs: Sequence[SceneJob], keep_debug: bool = False, keep_models: bool = False):
        """Process a batch of scenes; fills job.outputs = (sem i32[N], inst i32[N], prob f32[N], mu f32[S],
        var f32[S]) as device tensors (same lengths as the reference returns).  With ``keep_models`` every
        job also gets ``feats_spp``, ``fits`` and ``winner`` (see SceneJob): the trained GP of every box pair, for
        predictions at other inputs (predict_models), and which of them labelled each superpoint.  The outputs are the
        same bits either way.  A ``point_level`` pipeline returns mu and var at point length, f32[N] (see __init__)."""
        return self._finish(self._start(jobs, keep_debug, keep_models))

    kSlots = 3  # pipeline streams = slots of per-batch buffers (see _stream_batches)

    def _ensure_streams(self):
        if not hasattr(self, "_streams"):
            self._streams = [self.be.new_stream() for _ in range(self.kSlots)]
            for st in self._streams:
                self._ws.setdefault("s%x" % int(st.cuda_stream), None)

    def run_pipelined(self, batches: Sequence[Sequence[SceneJob]]):
        """Several batches back to back, software-pipelined.  The fit workgroups fill every CU for the whole
        launch and the short partition / broadcast kernels cannot be dispatched beside them (measured: they
        wait until CUs drain, whatever the stream priorities), so the order is built around that (_stream_batches):

            partition(i+1) in the tail of fit(i-1) -> launch fit(i) -> while it runs, on the host: schedule(i+1),
            merge(i-1); broadcast(i-1) is enqueued without waiting for it

        Same results as run() batch by batch."""
        self._ensure_streams()
        # inputs produced on the caller's stream are ordered before both pipeline streams ONCE: an event on
        # the (legacy default) stream recorded per batch would also wait for every blocking stream
        ready = self.be.current_stream().record_event()
        for st in self._streams:
            st.wait_event(ready)
        outs = list(self._stream_batches(iter(batches)))
        for st in self._streams:
            self.be.current_stream().wait_stream(st)
        return outs

    def run_stream(self, batches):
        """run_pipelined for an ITERATOR of batches (e.g. a dataset being read from disk): yields the outputs of
        every batch, in order, one batch behind the one being launched.  The consumer may use the yielded
        tensors on the current stream right away (they are ordered after the pipeline's streams)."""
        self._ensure_streams()
        ready = self.be.current_stream().record_event()
        for st in self._streams:
            st.wait_event(ready)
        for i, out in enumerate(self._stream_batches(iter(batches))):
            self.be.current_stream().wait_stream(self._streams[i % self.kSlots])
            yield out

    def _stream_batches(self, it):
        """The software pipeline of run_pipelined / run_stream over an iterator (lookahead of one batch).

        Batch k lives on stream / buffer slot k % kSlots.  Iteration i, entered while fit(i-1) runs:
            partition(i+1)   the host blocks on its two round trips; the kernels cannot be dispatched beside a fit that
                             holds every CU: by the host-side trace (bench.py --trace) they complete when the last
                             workgroups of fit(i-1) end, also on a stream that is not ordered behind that fit (three
                             slots; with two, batch i+1 shared the stream of batch i-1, which gapro_svgp_fit_batch
                             joins its kernels back into) and with more hardware queues (GPU_MAX_HW_QUEUES = 8 / 16:
                             slower); ~10 ms of partition kernels and round trips stay between two fits
            launch fit(i)
            pull batch i+2, schedule(i+1), finish(i-1): host work while fit(i) runs
        Queueing fit(i+1) behind fit(i) instead (two fits in flight, five slots) starves the partition kernels until
        BOTH have drained: measured, 64 ms of idle GPU every second step, 287 vs 300 scenes/s."""
        S = self.kSlots

        def on(k, fn, *a):
            with self.be.stream(self._streams[k % S]):
                return fn(*a)

        # a batch is pulled from the iterator under the pipeline stream that will process it: whatever device work
        # building its jobs enqueues (a dtype cast, .contiguous() of a strided input in make_job) is then ordered
        # before its partition kernels, for every batch and not only the first
        cur = on(0, next, it, None)
        if cur is None:
            return
        i = 0
        cur_state = on(0, self._partition, cur, False)
        on(0, self._schedule_all, cur_state)
        # The first fit launch goes out before the second batch is even asked for (round 5): with the native feeder the
        # iterator hands the first batch over ~0.3 s into a run and blocks ~0.2 s for the second -- time the GPU would
        # sit idle in the plain order below, which partitions batch i + 1 before it launches batch i.  (Round 4 tried the
        # same and measured nothing: the Python loaders, not the order, were what the first launch waited for.)
        on(0, self._launch, cur_state)
        nxt = on(1, next, it, None)
        prev_state = None
        while cur_state is not None:
            nxt_state = on(i + 1, self._partition, nxt, False) if nxt is not None else None
            # point_level: finish(i-1) waits for its predict kernels (the predict entry synchronises its stream and the
            # per-model status is read back), and those cannot be dispatched beside a fit that holds every CU: it runs
            # BEFORE fit(i) is launched.  The merge of batch i-1 is then not hidden behind a fit; the pull and the
            # schedule of the batches behind it still are.
            early = None
            if self.point_level and prev_state is not None:
                early = on(i - 1, self._finish, prev_state, False)
            if i > 0:
                on(i, self._launch, cur_state)
            # everything below is host work that runs while the fit just launched occupies the GPU: the merge of the
            # previous batch, fetching the batch after next from the iterator (building jobs, reading / uploading
            # scenes), the schedule of the next batch.  The merge comes FIRST (round 6): fit(i-1) has ended -- the
            # partition kernels above only ran once it had drained -- and the pull can block for a whole batch of
            # reads, which in a worker's first second kept finished labels waiting for 0.3 .. 0.5 s
            if prev_state is not None:
                yield early if early is not None else on(i - 1, self._finish, prev_state, False)
            nxt = on(i + 2, next, it, None) if nxt is not None else None
            if nxt_state is not None:
                on(i + 1, self._schedule_all, nxt_state)
            prev_state, cur_state = cur_state, nxt_state
            i += 1
        yield on(i - 1, self._finish, prev_state, True)

    def _start(self, jobs: Sequence[SceneJob], keep_debug: bool = False, keep_models: bool = False):
        """Stages A-D: everything up to and including the (asynchronous) fit launch."""
        state = self._partition(jobs, keep_debug)
        state.keep_models = keep_models
        self._schedule_all(state)
        self._launch(state)
        return state

    def _marker(self, jobs):
        import time as _time
        t = [_time.perf_counter()]

        def _mark(name):
            if self.trace is not None:  # host-side timeline, no synchronisation added
                self.trace.append((_time.perf_counter(), id(jobs) & 0xFFFF, name))
            if self.profile_stages:
                self.be.synchronize()
                now = _time.perf_counter()
                self.stage_times[name] = self.stage_times.get(name, 0.0) + (now - t[0])
                t[0] = now

        return _mark

    def _partition(self, jobs: Sequence[SceneJob], keep_debug: bool = False):
        """Stages A-B on the current stream: superpoint ids, pooled features, occupancy tables on the host."""
        _mark = self._marker(jobs)
        stream = self.be.current_stream()
        slot = "s%x" % int(stream.cuda_stream)
        _mark("start")
        all_jobs = list(jobs)
        tasks, d_tasks = self._prepare_all(jobs)
        jobs = [j for j in all_jobs if j.error is None]
        _mark("A prepare")
        if not jobs:
            return BatchState([], all_jobs, stream, slot, _mark, tasks, d_tasks, keep_debug)
        D = int(jobs[0].feats.shape[1])
        base = 0
        for job in jobs:
            if int(job.feats.shape[1]) != D:
                raise ValueError("all scenes of a batch must share the feature dimension")
            job.feats_row_base = base
            base += job.n_spps
        feats_spp_all = self.be.empty_typed((base, D), self.be.f32)
        # one pinned staging area for the tables the host scheduler needs from every scene
        need = sum(job.n_spps * (((job.n_boxes + 63) // 64) * 8 + 4 + (4 if self.point_level else 0)) + 16
                   for job in jobs)
        stage = self._pinned(slot + "tables", need)
        self._pool_all(jobs, tasks, d_tasks, feats_spp_all, stage)
        stream.synchronize()  # one sync: pooled tables of every scene are on the host
        _mark("B pool")
        return BatchState(jobs, all_jobs, stream, slot, _mark, tasks, d_tasks, keep_debug, feats_spp_all=feats_spp_all)

    def _schedule_all(self, state: BatchState):
        """Stage C (host only): static pair schedule of every scene, fit descriptors of the whole batch."""
        lib = self.lib
        jobs, _mark = state.jobs, state.mark
        if not jobs:
            return
        # one host thread per scene (gapro_schedule_build is host C++ behind ctypes: no GIL): 256 scenes took 0.45 s on
        # the main thread, more than half of what a fit launch of that batch lasts -- the product path's steady state
        # was bound by this thread, not by the GPU
        if len(jobs) >= 8:
            list(self._host_threads().map(self._schedule, jobs))
        else:
            for job in jobs:
                self._schedule(job)
        _mark("C schedule")
        n_fits = sum(j.counts.n_fits for j in jobs)
        n_idx = sum(j.counts.n_fit_idx for j in jobs)
        n_out = sum(j.counts.n_fit_out for j in jobs)
        descs = (FitDesc * max(n_fits, 1))()
        h_idx = np.zeros(max(n_idx, 1), dtype=np.int32)
        fo = io = oo = 0
        for si, job in enumerate(jobs):
            job.fit_base, job.out_base = fo, oo
            if job.counts.n_fits:
                rc = lib.gapro_schedule_export_fits(
                    job.schedule, job.feats_row_base, io, oo, si,
                    C.cast(C.byref(descs, fo * C.sizeof(FitDesc)), C.c_void_p), _ptr(h_idx[io:]))
                if rc != 0:
                    raise _lib.GaproError(rc, "gapro_schedule_export_fits")
            fo += job.counts.n_fits
            io += job.counts.n_fit_idx
            oo += job.counts.n_fit_out
        _mark("C export")
        state.n_fits, state.n_out, state.descs, state.h_idx = n_fits, n_out, descs, h_idx

    def _launch(self, state: BatchState):
        """Stage D: one (asynchronous) launch for every fit of every scene."""
        if state.n_fits:
            state.pending = self.fit_launch(state.feats_spp_all, state.descs, state.n_fits, state.h_idx, state.n_out,
                                            keep_debug=state.keep_debug, slot=state.slot,
                                            scene_keys=[j.scene_key for j in state.jobs],
                                            keep_models=state.keep_models or self.point_level,
                                            state_to_host=state.keep_models)
        state.mark("D launched")

    def _finish(self, state: BatchState, sync: bool = True):
        """Stages E-F: wait for the fit results, ordered merge on the host, broadcast on the device.  With
        sync=False the broadcast kernels are only enqueued (the outputs are ordered on the current stream)."""
        lib, ctx, be = self.lib, self.ctx, self.be
        jobs, keep_debug, _mark = state.jobs, state.keep_debug, state.mark
        _mark("finish")
        if not jobs:  # every scene of the batch was rejected (non-strict mode)
            self.last_stats = dict(n_fits=0, n_fit_out=0, fit=None)
            return [None for _ in state.all_jobs]
        res = self.fit_collect(state.pending, raise_on_failure=False) if state.pending is not None else None
        if res is not None:
            res = self._retry_timeouts(res, state.feats_spp_all, state.descs, state.h_idx, state.n_out,
                                       slot=state.slot, scene_keys=[j.scene_key for j in jobs],
                                       keep_state=self.point_level)
            if "retry_state" in res:  # the retried fits are predicted from the retry's states: copied into place
                d2, off2 = res["retry_state"]
                D = int(state.feats_spp_all.shape[1])
                for k, i in enumerate(res["retried"]):
                    nb = 8 * state_doubles(int(state.descs[i].m1 + state.descs[i].m2), D)
                    a, b = 8 * int(state.pending.state_off[i]), 8 * off2[k]
                    state.pending.d_state[a:a + nb].copy_(d2[b:b + nb], non_blocking=True)
        _mark("D fit")
        if state.keep_models:
            feats_all = _host(state.feats_spp_all)
            descs, h_idx = state.descs, state.h_idx
            for job in jobs:
                job.feats_spp = feats_all[job.feats_row_base:job.feats_row_base + job.n_spps].copy()
                job.fits = []
                for k in range(job.fit_base, job.fit_base + job.counts.n_fits):
                    d = descs[k]
                    io, m = int(d.idx_offset), int(d.m1 + d.m2)
                    job.fits.append(SceneFit(int(d.b1), int(d.b2), h_idx[io:io + m] - job.feats_row_base,
                                             h_idx[io + m:io + m + int(d.t)] - job.feats_row_base, res["models"][k],
                                             int(d.m1)))
        if res is not None and (res["status"] != 0).any():
            # per-fit status -> per-scene failure: only the scenes that own a failed fit are lost
            for job in jobs:
                st = res["status"][job.fit_base:job.fit_base + job.counts.n_fits]
                if (st != 0).any():
                    k = int(np.nonzero(st)[0][0])
                    job.error = _lib.GaproError(int(st[k]), "GP fit %d of %d of the scene failed (%d failed in all)"
                                                % (k, job.counts.n_fits, int((st != 0).sum())))
            if self.strict:
                raise next(j.error for j in jobs if j.error is not None)
        want_winner = self.point_level or state.keep_models
        tot_s = sum(job.n_spps for job in jobs)
        tables = self._pinned(state.slot + "labels", tot_s * 20)
        busy = self._pin_events.pop(state.slot + "labels", None)
        if busy is not None:
            busy.synchronize()  # the previous batch of this slot has uploaded its label tables
        d_tables = be.empty(tot_s * 20)
        tab_np = tables.numpy()
        offs, off = [], 0
        for job in jobs:
            offs.append(off)
            off += 20 * job.n_spps

        def merge_one(arg):
            job, off = arg
            S = job.n_spps
            sem_spp = tab_np[off:off + 4 * S].view(np.int32)
            inst_spp = tab_np[off + 4 * S:off + 8 * S].view(np.int32)
            prob_spp = tab_np[off + 8 * S:off + 12 * S].view(np.float32)
            mu_spp = tab_np[off + 12 * S:off + 16 * S].view(np.float32)
            var_spp = tab_np[off + 16 * S:off + 20 * S].view(np.float32)
            if job.counts.n_fits:
                a, b = job.out_base, job.out_base + job.counts.n_fit_out
                pn, lb, mu, var = (res["probs_new"][a:b], res["labels"][a:b], res["mu"][a:b], res["var"][a:b])
            else:
                pn = lb = mu = var = None
            winner = np.empty(S, dtype=np.int32) if want_winner else None
            rc = lib.gapro_schedule_merge_ex(job.schedule, _ptr(pn), _ptr(lb), _ptr(mu), _ptr(var),
                                             _ptr(job.boxes_cls), _ptr(job.boxes_volume), len(job.instance_box),
                                             job.instance_classes, _ptr(sem_spp), _ptr(inst_spp), _ptr(prob_spp),
                                             _ptr(mu_spp), _ptr(var_spp), _ptr(winner))
            if rc != 0:
                raise _lib.GaproError(rc, "gapro_schedule_merge_ex")
            job.host.update(sem_spp=sem_spp.copy(), inst_spp=inst_spp.copy(), prob_spp=prob_spp.copy())
            if want_winner:
                dict.__setitem__(job.host, "winner", winner)
                if state.keep_models:
                    job.winner = winner

        # the ordered merge of a scene is host C++ on that scene's own slices: one host thread per scene
        if len(jobs) >= 8:
            list(self._host_threads().map(merge_one, zip(jobs, offs)))
        else:
            for arg in zip(jobs, offs):
                merge_one(arg)
        # point_level: the row table of the predict launch is planned here, on the host, before anything is enqueued
        plan = refine_plan(self, state) if self.point_level else None
        d_tables.copy_(tables[:tot_s * 20], non_blocking=True)  # one H2D copy for the whole batch
        self._pin_events[state.slot + "labels"] = be.current_stream().record_event()
        tasks, d_tasks = state.tasks, state.d_tasks
        per_point = 20 if self.point_outputs else 12
        out_off, out_tot = self._carve([per_point * job.n_points for job in jobs], 16)
        d_out = be.empty(out_tot)  # [sem | inst | prob] per scene; point_level: [sem | inst | prob | mu | var]
        for t, job, off, oo in zip(tasks, jobs, offs, out_off):
            S, n = job.n_spps, job.n_points
            sem = d_out[oo:oo + 4 * n].view(be.i32)
            ins = d_out[oo + 4 * n:oo + 8 * n].view(be.i32)
            prb = d_out[oo + 8 * n:oo + 12 * n].view(be.f32)
            t.sem_spp = d_tables.data_ptr() + off
            t.inst_spp = d_tables.data_ptr() + off + 4 * S
            t.prob_spp = d_tables.data_ptr() + off + 8 * S
            t.sem, t.inst, t.prob = sem.data_ptr(), ins.data_ptr(), prb.data_ptr()
            mu_spp = d_tables[off + 12 * S:off + 16 * S].view(be.f32)
            var_spp = d_tables[off + 16 * S:off + 20 * S].view(be.f32)
            if self.point_outputs:
                job.outputs = (sem, ins, prb, d_out[oo + 12 * n:oo + 16 * n].view(be.f32),
                               d_out[oo + 16 * n:oo + 20 * n].view(be.f32))
                dict.__setitem__(job.dev, "mu_var_spp", (mu_spp, var_spp))
            else:
                job.outputs = (sem, ins, prb, mu_spp, var_spp)
            if not keep_debug:
                lib.gapro_schedule_free(job.schedule)
                job.schedule = None
        # point_level at superpoint length works on the superpoint tables, in front of the broadcast that reads them
        refined = None
        if self.point_level and not self.point_outputs:
            refined = refine_chain(self, state, plan, offs, d_tables)
        ev = self._part_event(jobs, "broadcast")
        ctx.check(lib.gapro_broadcast_labels_batch(ctx.handle, self._sh(), len(jobs),
                                                   C.cast(tasks, C.c_void_p), _ptr(d_tasks)))
        self._part_event_end(ev)
        if refined is not None:
            self._stage("labels")
        if self.point_outputs:  # ... and at point length on the broadcast's outputs, behind it
            refined = refine_chain(self, state, plan, offs, d_tables)
        # the task array must outlive the (possibly delayed) upload enqueued above
        self._keep[state.slot] = (tasks, d_tasks, refined)
        if sync:
            be.current_stream().synchronize()
        _mark("E+F merge/broadcast")
        self.last_stats = dict(n_fits=state.n_fits, n_fit_out=state.n_out, fit=res)
        for j in jobs:
            if j.error is not None:  # merged from a failed fit's garbage: not a result
                j.outputs = None
        return [j.outputs if j.error is None else None for j in state.all_jobs]
