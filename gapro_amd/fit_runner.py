"""The fit launcher on one GPU: every GP fit of a batch in ONE gapro_svgp_fit_batch launch (fit_launch / fit_collect /
fit_descs), the posterior of kept models at other inputs (predict_models), point-level fits whose training sets are
assembled on the device (train_sets / fit_points), and what goes with them: grow-only
workspaces, pinned staging, the timeout retry, the reproducibility probe, the FLOP accounting of a launch.  Nothing here
knows what a scene is: pipeline.py's Pipeline derives from FitRunner and adds the scene path.  Device memory, streams
and events come from a backend (devmem.py).
"""
from __future__ import annotations

import os
import sys
import threading
import time
import ctypes as C
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import FitDesc, PredictDesc, SceneHeader, TrainsetDesc
from .gp_model import GPModel


# A fit is "soft" when its outputs move by more than this (sigma^2 relative, p absolute) when the jitter on K_ZZ's diagonal
# is scaled by (1 + 1e-11) (FitRunner.reproducibility_probe): fifty Adam steps amplify last-bit differences ~1e9-fold on
# such a fit, in ANY float64 implementation.  Measured on the S3DIS-shaped test scene's 66 fits: the
# two soft ones move by 6.4e-5 / 6.8e-4, every other fit by 8e-8 .. 1.2e-6
REPRO_SOFT = 1.0e-5


def _ptr(t) -> C.c_void_p:
    if t is None:
        return C.c_void_p(0)
    if hasattr(t, "data_ptr"):  # torch.Tensor / devmem buffer
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


def _to_np(x, dtype):
    if hasattr(x, "detach"):  # torch.Tensor
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def _host(x) -> np.ndarray:
    """Blocking device -> host copy of a backend buffer (torch tensor or devmem.DevBuf) as a NumPy array."""
    h = x.cpu()
    return h if isinstance(h, np.ndarray) else h.numpy()


# ---------------------------------------------------------------------- result layouts
# The two blocks a launch's results travel in, each a struct of arrays over n entries (n = 0 is laid out as n = 1):
#   per test row  probs f32 | probs_new f32 | mu f32 | var f32 | labels u8   17 bytes per row
#   per fit       loss f64 | cond f64 | status i32                           20 bytes per fit
ROW_FIELDS = (("probs", "f32"), ("probs_new", "f32"), ("mu", "f32"), ("var", "f32"), ("labels", "u8"))
FIT_FIELDS = (("loss", "f64"), ("cond", "f64"), ("status", "i32"))
_NP = SimpleNamespace(u8=np.uint8, i32=np.int32, f32=np.float32, f64=np.float64)
_WIDTH = dict(u8=1, i32=4, f32=4, f64=8)


def block_bytes(fields, n: int) -> int:
    return max(int(n), 1) * sum(_WIDTH[t] for _, t in fields)


def block_views(fields, buf, n: int, ty=_NP) -> dict:
    """The typed views, by name, of a byte buffer that holds n entries of ROW_FIELDS / FIT_FIELDS.  `ty` names the
    dtypes of the buffer's kind: a backend (devmem.py) for its device buffers, NumPy's for a host array."""
    n, out, off = max(int(n), 1), {}, 0
    for name, t in fields:
        out[name] = buf[off:off + _WIDTH[t] * n].view(getattr(ty, t))
        off += _WIDTH[t] * n
    return out


# ---------------------------------------------------------------------- FLOP accounting
def _desc_table(descs, n_fits: int) -> np.ndarray:
    return np.frombuffer(descs, dtype=np.int32, count=n_fits * (C.sizeof(FitDesc) // 4)).reshape(n_fits, -1)


def fit_flops_each(descs, n_fits: int, feat_dim: int, training_iter: int) -> np.ndarray:
    """Algorithmic FLOPs of every fit of a batch, SURVEY.md section 8(d):
    F_fit = I (8.33 M^3 + 12 D M^2) + (M^3/3 + 2 M^2 T + 2 D (M^2 + M T)),  M = m1 + m2."""
    if n_fits <= 0:
        return np.zeros(0)
    raw = _desc_table(descs, n_fits)
    m = (raw[:, 0] + raw[:, 1]).astype(np.float64)
    t = raw[:, 2].astype(np.float64)
    d = float(feat_dim)
    return training_iter * (8.33 * m**3 + 12.0 * d * m * m) + (m**3 / 3.0 + 2.0 * m * m * t + 2.0 * d * (m * m + m * t))


def fit_flops(descs, n_fits: int, feat_dim: int, training_iter: int) -> float:
    return float(fit_flops_each(descs, n_fits, feat_dim, training_iter).sum())


# accounting class of every kernel route (gapro_fit_route): the generic kernel is booked with the staged one
ROUTE_CLASS = {0: "strip", 1: "staged", 2: "staged", 3: "small", 4: "cluster", 5: "wave"}


def fit_flops_by_class(descs, n_fits: int, feat_dim: int, training_iter: int, flags: int = 0) -> dict:
    """Algorithmic FLOPs of a launch per accounting class (strip, staged, small, cluster, wave), every fit booked under
    the kernel the library routes it to with `flags` in gapro_fit_options.reserved (gapro_fit_route_flags).  Needs the
    library, not a device."""
    out = dict.fromkeys(ROUTE_CLASS.values(), 0.0)
    if n_fits <= 0:
        return out
    each = fit_flops_each(descs, n_fits, feat_dim, training_iter)
    raw = _desc_table(descs, n_fits)
    m = raw[:, 0] + raw[:, 1]
    route = {int(v): int(_lib.load().gapro_fit_route_flags(int(v), int(feat_dim), int(flags))) for v in np.unique(m)}
    if min(route.values()) < 0:
        raise _lib.GaproError(min(route.values()), "gapro_fit_route_flags(flags=0x%x)" % int(flags))
    of = np.array([ROUTE_CLASS[route[int(v)]] for v in m])
    for name in out:
        out[name] = float(each[of == name].sum())
    return out


class FitTiming:
    """Device-side timing of one fit launch (gapro_fit_timing): HIP events recorded by the library on the
    streams its kernels run on.  read() blocks until the launch has finished."""

    def __init__(self, ctx, handle, flops: dict, m):
        self.ctx, self.handle, self.m = ctx, handle, m
        self.flops_strip, self.flops_staged, self.flops_small = flops["strip"], flops["staged"], flops["small"]
        self.flops_cluster, self.flops_wave = flops["cluster"], flops["wave"]
        self.ms = None

    @property
    def flops(self):
        return self.flops_strip + self.flops_staged + self.flops_small + self.flops_cluster + self.flops_wave

    def read(self):
        """(staged kernel ms, strip kernel ms, first start -> last end ms, small-fit strip kernel ms, cluster kernel
        ms, wave-per-fit kernels ms); the span covers all of them"""
        if self.ms is None:
            out = (C.c_float * 5)()
            self.ctx.check(self.ctx.lib.gapro_fit_timing_read(self.ctx.handle, self.handle, out))
            w = C.c_float(0.0)
            self.ctx.check(self.ctx.lib.gapro_fit_timing_read_wave(self.ctx.handle, self.handle, C.byref(w)))
            self.ms = (float(out[0]), float(out[1]), float(out[2]), float(out[3]), float(out[4]), float(w.value))
        return self.ms

    def cluster_info(self):
        """(clusters of more than one workgroup, those whose members did not share an XCD, member workgroups) of this
        launch's cluster kernel; read before 64 further launches."""
        out = (C.c_int32 * 3)()
        self.ctx.check(self.ctx.lib.gapro_fit_timing_cluster_info(self.ctx.handle, self.handle, out))
        return int(out[0]), int(out[1]), int(out[2])

    def offsets(self, ref):
        """(first kernel start, last kernel end) of this launch in ms after the start of launch `ref`."""
        out = (C.c_float * 2)()
        self.ctx.check(self.ctx.lib.gapro_fit_timing_offsets(self.ctx.handle, ref.handle, self.handle, out))
        return float(out[0]), float(out[1])

    def close(self):
        if self.handle is not None:
            self.ctx.lib.gapro_fit_timing_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


@dataclass
class PendingFit:
    """What fit_launch hands to fit_collect: a launch in flight and where its results arrive."""
    done: object  # event behind the result copies
    h_out: object  # pinned ROW_FIELDS block of `no` rows
    h_stat: object  # pinned FIT_FIELDS block of `n_fits` fits
    no: int
    n_fits: int
    ws_bytes: int
    keep: Optional[tuple]  # device buffers that stay alive until the launch has finished
    ws: object = None  # keep_debug: the workspace and the descriptors with their ws_offset
    descs: object = None
    h_state: object = None  # keep_models: pinned model states, their offsets (doubles) and size
    state_off: Optional[np.ndarray] = None
    state_bytes: int = 0
    d_state: object = None  # keep_models: the states where the launch leaves them (device)


def pack_point_problems(problems, n_points: int, npoint_nearest: int, spp_pool: bool):
    """Descriptors and the int32 index array [b1 | b2 | intersect] of point-level problems.  Every ValueError of the
    point-level API is raised here, on the host, before a device is touched."""
    if not spp_pool and not (1 <= int(npoint_nearest) <= _lib.TRAINSET_MAX_NEAREST):
        raise ValueError("npoint_nearest must be in [1, %d], got %r" % (_lib.TRAINSET_MAX_NEAREST, npoint_nearest))
    n = len(problems)
    if n == 0:
        raise ValueError("no problem given")
    if n > _lib.TRAINSET_MAX_PROBLEMS:
        raise ValueError("%d problems in one call: at most %d (split the batch)" % (n, _lib.TRAINSET_MAX_PROBLEMS))
    descs = (TrainsetDesc * n)()
    idx, io = [], 0
    for i, prob in enumerate(problems):
        b1, b2, it = (_to_np(x, np.int64).reshape(-1) for x in prob)
        if len(b1) == 0 or len(b2) == 0:
            raise ValueError("problem %d: fit_gp needs at least one point on each side" % i)
        for a in (b1, b2, it):
            if len(a) and (a.min() < 0 or a.max() >= n_points):
                raise ValueError("problem %d: a point index lies outside the %d points" % (i, n_points))
            if len(a) > _lib.TRAINSET_MAX_LIST_FACTOR * n_points:  # the exact int64 sums have room for 4 N terms
                raise ValueError("problem %d: a list of %d entries is longer than %d times the %d points"
                                 % (i, len(a), _lib.TRAINSET_MAX_LIST_FACTOR, n_points))
        if not spp_pool and len(it) == 0 and max(len(b1), len(b2)) > npoint_nearest:
            raise ValueError("problem %d: a side is longer than npoint_nearest and there is no intersection point to "
                             "take the centroid of" % i)
        d = descs[i]
        d.idx_offset, d.n1, d.n2, d.t, d.reserved = io, len(b1), len(b2), len(it), 0
        idx += [b1, b2, it]
        io += len(b1) + len(b2) + len(it)
    return descs, np.ascontiguousarray(np.concatenate(idx).astype(np.int32))


@dataclass
class TrainSets:
    """What train_sets leaves on the device: the table a fit launch reads with identity indices."""
    train: object  # f32[n_rows, D]
    sel: object  # i64[n_rows]: superpoint id (pool) or point index (nearest) of every row
    status: object  # i32[n problems]
    descs: object  # TrainsetDesc per problem with m1 / m2 / row_offset
    n_rows: int
    d_idx: object  # i32: every problem's [b1 | b2 | intersect] point indices
    feats: object  # f32[N, D]: the row table of the predictions
    keep: Optional[tuple] = None


class FitRunner:
    def __init__(self, device=0, training_iter=50, init_mean_std=0.0, seed=0, eval_stale_chol=False,
                 force_staged=False, precision="f64", cluster_all=False, backend="torch"):
        from .devmem import make_backend

        if not isinstance(device, int):
            import torch

            device = torch.device(device).index or 0
        # backend: "torch" (tensors in, tensors out) or "native" (the library's arena, no torch in the process);
        # either raises when there is no HIP device -- there is no CPU fallback
        self.be = make_backend(backend, device)
        self.device = self.be.device
        self.ctx = self.be.ctx
        self.lib = self.ctx.lib
        self.opt = _lib.default_fit_options(training_iter)
        self.opt.eval_stale_chol = 1 if eval_stale_chol else 0
        # reserved: 0 default dispatch (gapro_fit_route); force_staged = never the strip kernels (A/B runs, tests)
        self.opt.reserved = _lib.FIT_DBG_NO_STRIP if force_staged else 0
        # precision: "f64" (default, float64 throughout) or "mixed" (the reference's float32 / float64 split, run by
        # the cluster kernel; fits routed elsewhere stay float64).  cluster_all: the cluster kernel for every fit it
        # can take (precision sweeps, A/B runs)
        if precision not in ("f64", "mixed"):
            raise ValueError("precision must be 'f64' or 'mixed'")
        self.opt.precision = 1 if precision == "mixed" else 0
        if cluster_all:
            self.opt.reserved |= _lib.FIT_DBG_CLUSTER_ALL
        # A/B runs and tests only: further debug bits of gapro_fit_options.reserved (include/gapro_hip.h) from the
        # environment.  Never silent: a leaked variable changes the routing of every fit.
        env_flags = os.environ.get("GAPRO_FIT_FLAGS", "").strip()
        if env_flags:
            try:
                bits = int(env_flags, 0)
            except ValueError:
                raise ValueError("GAPRO_FIT_FLAGS=%r is not an integer (debug bits of gapro_fit_options.reserved)"
                                 % env_flags) from None
            if bits:
                print("[gapro_amd] GAPRO_FIT_FLAGS=0x%x: debug routing bits are ORed into every fit launch of this "
                      "process (measurement / test setting, not a product mode)" % bits, file=sys.stderr)
            self.opt.reserved |= bits
        # a fit that comes back GAPRO_ERR_TIMEOUT (a cluster member was not resident in time: transient, unlike a failed
        # factorisation) is run once more on the single-workgroup route before its scene is given up
        self.retry_timeouts = True
        self.timeout_retries = 0  # fits that went through the retry, over the life of this object

        self.init_mean_std = float(init_mean_std)
        self.seed = int(seed)
        self.trace = None  # set to a list to collect (time, batch id, stage) host timestamps
        self.workspace_headroom = 1.3  # growth factor of the fit workspaces over the need that triggers it
        self.serialize_fits = not os.environ.get("GAPRO_OVERLAP_FITS")  # fit launches never overlap (see fit_launch)
        self._last_fit_done = None
        self._ws_lock = threading.Lock()
        # optional HIP-event timing of the fit launches (bench.py): one FitTiming per launch
        self.profile_fit = False
        self.fit_events = []
        self.last_fit_m = None  # with profile_fit: M of every fit of the last launch
        self._pin_cache = {}
        self._ws = {}  # slot -> fit workspace (device, float64)
        self.stage_events = None  # set to a list: fit_points appends (stage, HIP event) at its stage boundaries

    def _sh(self) -> C.c_void_p:
        """raw handle of the backend's current stream"""
        return C.c_void_p(self.be.current_stream().cuda_stream)

    def _pinned(self, tag: str, nbytes: int):
        """Growable page-locked staging buffers, reused across batches (hipHostMalloc is slow)."""
        buf = self._pin_cache.get(tag)
        if buf is None or buf.numel() < nbytes:
            buf = self.be.pinned(max(nbytes, 1 << 16))
            self._pin_cache[tag] = buf
        return buf

    def warmup(self):
        """One small launch through every fit kernel family and the result path (a driver calls this while its first
        scenes are being read): the first launch of a process pays for code-object loading, kernel attributes and the
        allocator's first blocks -- ~0.2 s that would otherwise sit in front of the first batch."""
        rng = np.random.default_rng(0)
        sizes = [4, 12, 20, 30, 50, 75, 150, 280]
        feats = self.be.from_numpy(rng.normal(size=(2 * sum(sizes), 6)).astype(np.float32))
        descs = (FitDesc * len(sizes))()
        idx, io, oo, base = [], 0, 0, 0
        for k, m in enumerate(sizes):
            d = descs[k]
            d.m1, d.m2, d.t, d.b1, d.b2, d.scene = m, m, 4, 0, 1, 0
            d.idx_offset, d.out_offset, d.ws_offset = io, oo, 0
            idx.append(np.arange(base, base + 2 * m, dtype=np.int32))
            idx.append(np.arange(base, base + 4, dtype=np.int32))
            io += 2 * m + 4
            oo += 4
            base += 2 * m
        it, prof = self.opt.training_iter, self.profile_fit
        self.opt.training_iter, self.profile_fit = 2, False
        try:
            self.fit_descs(feats, descs, len(sizes), np.concatenate(idx), oo, raise_on_failure=False)
        finally:
            self.opt.training_iter, self.profile_fit = it, prof

    # ------------------------------------------------------------------ workspaces
    def prealloc_workspace(self, n_bytes: int, slot: str = "shared"):
        """Allocate the fit workspace ahead of its first use (a driver calls this from a helper thread while the first
        scenes are still being read: the hipMalloc + clear of ~25 GB takes 1.2 .. 2.4 s, a third of what a worker needs
        for the whole ScanNet train split).  A later need beyond this size grows it as usual."""
        with self.be.device_ctx():
            self._workspace(slot, max(1, int(n_bytes) // 8), headroom=1.0)

    def _workspace(self, slot: str, n_doubles: int, headroom: Optional[float] = None):
        """Grow-only fit workspace per pipeline slot.  Every registered slot grows together and new memory is
        touched once here: a slot first used inside a timed region would otherwise pay the allocation and the
        first-touch mapping of several GB inside its fit kernel."""
        with self._ws_lock:
            self._ws.setdefault(slot, None)
            cur = self._ws[slot]
            if cur is None or cur.numel() < n_doubles:
                if self._last_fit_done is not None:
                    # a launch that may still be running works in the memory about to be released (the fit kernels run
                    # on library-owned streams the caching allocator knows nothing about)
                    self._last_fit_done.synchronize()
                # 30 % headroom: the need of a batch of 256 scenes varies by ~10 %, and growing means a hipMalloc of
                # 10 .. 20 GB per slot plus its fill behind the running fit kernels -- 2 s on a freshly booted box,
                # inside whatever step first exceeds the old size (bench.py's sporadic 980 ms steps, 760 ms launches)
                size = int(n_doubles * (self.workspace_headroom if headroom is None else headroom)) + 1024
                if slot.endswith("retry"):  # a few timed-out fits: exactly their need, for one launch
                    self._ws[slot] = self.be.zeros(n_doubles + 1024, self.be.f64)
                    self.be.current_stream().synchronize()
                    return self._ws[slot][:n_doubles]
                if self.trace is not None:
                    self.trace.append((time.perf_counter(), 0, "workspace grows to %.1f GB per slot" % (8e-9 * size)))
                for k in list(self._ws):  # the requested slot, and every slot that is in use (they grow together)
                    if k != slot and (self._ws[k] is None or k.endswith("retry")):
                        continue
                    if self._ws[k] is None or self._ws[k].numel() < size:
                        self._ws[k] = None  # release before growing
                        self._ws[k] = self.be.zeros(size, self.be.f64)
                # the fill runs on the allocating thread's stream; the fit kernels that use this memory run on other
                # streams (another pipeline slot's, the library's): nobody may get the tensor before the fill is done
                self.be.current_stream().synchronize()
                if self.trace is not None:
                    self.trace.append((time.perf_counter(), 0, "workspace ready"))
            return self._ws[slot][:n_doubles]

    # ------------------------------------------------------------------ prediction from kept models
    def _predict_launch(self, d_state, h_m: np.ndarray, descs, feats, d_rows, no: int):
        """One gapro_svgp_predict_batch launch over states, features and rows that are on the device.  Enqueue only:
        returns the device block of ``no`` ROW_FIELDS rows (nothing is written for a model that fails before its rows)
        and the per-model status (device)."""
        lib, ctx, be = self.lib, self.ctx, self.be
        n, D, R = len(h_m), int(feats.shape[1]), int(feats.shape[0])
        ws_bytes = int(lib.gapro_svgp_predict_workspace_bytes(n, D, _ptr(h_m)))
        ws = be.empty(ws_bytes)
        out = be.empty(block_bytes(ROW_FIELDS, no))
        o = block_views(ROW_FIELDS, out, no, be)
        stat = be.empty(n * 4)
        ctx.check(lib.gapro_svgp_predict_batch(
            ctx.handle, self._sh(), n, D, _ptr(d_state), _ptr(h_m), C.cast(descs, C.c_void_p), _ptr(feats), R,
            _ptr(d_rows), C.byref(self.opt), _ptr(ws), ws_bytes, _ptr(o["probs"]), _ptr(o["probs_new"]),
            _ptr(o["labels"]), _ptr(o["mu"]), _ptr(o["var"]), _ptr(stat)))
        return out, stat

    def predict_models(self, models: Sequence[GPModel], feats, rows: Sequence, raise_on_failure: bool = True):
        """Posterior of every model at its own rows of ``feats`` (device f32[R, D]): one gapro_svgp_predict_batch
        launch.  ``rows[i]`` indexes ``feats`` (any order, repeats allowed).  Returns a dict like fit_collect's: probs,
        probs_new, mu, var f32 and labels u8 over all rows (model i at [offsets[i], offsets[i + 1])) and a per-model
        ``status``.  A model of a failed fit, or of another feature width, is refused: ValueError with
        ``raise_on_failure``, otherwise status BAD_ARG / the fit's own status for that model alone."""
        be = self.be
        n = len(models)
        D, R = int(feats.shape[1]), int(feats.shape[0])
        rows = [np.ascontiguousarray(_to_np(r, np.int64).reshape(-1)) for r in rows]
        if len(rows) != n:
            raise ValueError("predict_models: %d models but %d row vectors" % (n, len(rows)))
        pre = np.zeros(n, dtype=np.int32)
        for i, (mo, r) in enumerate(zip(models, rows)):
            if mo.d != D:
                if raise_on_failure:
                    raise ValueError("predict_models: model %d was trained at feature width %d, the features have %d"
                                     % (i, mo.d, D))
                pre[i] = -1
            elif mo.status != 0:
                if raise_on_failure:
                    raise ValueError("predict_models: model %d comes from a failed fit (status %d)" % (i, mo.status))
                pre[i] = mo.status
            if len(r) and (r.min() < 0 or r.max() >= R):
                raise ValueError("predict_models: rows of model %d reach outside the %d feature rows" % (i, R))
        live = [i for i in range(n) if pre[i] == 0]
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(r) for r in rows])
        tot = int(offsets[-1])
        res = dict({k: np.zeros(tot, getattr(_NP, t)) for k, t in ROW_FIELDS}, status=pre.copy(), offsets=offsets)
        if not live:
            return res
        nl = len(live)
        states = [models[i].to_state() for i in live]
        descs = (PredictDesc * nl)()
        h_m = np.array([models[i].m for i in live], dtype=np.int32)
        so = ro = 0
        for k, i in enumerate(live):
            d = descs[k]
            d.state_offset, d.row_offset, d.out_offset, d.t, d.reserved = so, ro, ro, len(rows[i]), 0
            so += len(states[k])
            ro += len(rows[i])
        no = max(ro, 1)
        d_state = be.from_numpy(np.concatenate(states))
        h_rows = np.concatenate([rows[i] for i in live]).astype(np.int32) if ro else np.zeros(1, np.int32)
        d_rows = be.from_numpy(h_rows)
        out, stat = self._predict_launch(d_state, h_m, descs, feats, d_rows, no)
        flat = block_views(ROW_FIELDS, _host(out), no)
        st = _host(stat).view(np.int32)
        ro = 0
        for k, i in enumerate(live):
            t = len(rows[i])
            res["status"][i] = st[k]
            if st[k] != _lib.GAPRO_ERR_CHOLESKY:
                for key in flat:
                    res[key][offsets[i]:offsets[i] + t] = flat[key][ro:ro + t]
            ro += t
        if raise_on_failure and (res["status"] != 0).any():
            bad = int(np.nonzero(res["status"])[0][0])
            raise _lib.GaproError(int(res["status"][bad]), "prediction of model %d of %d failed" % (bad, n))
        return res

    # ------------------------------------------------------------------ point-level fits
    def _stage(self, name: str):
        """HIP event on the current stream at a stage boundary of fit_points (tools/bench_fit_gp.py sets stage_events)."""
        ev = self.stage_events
        if ev is not None:
            e = self.be.event(enable_timing=True)
            e.record(self.be.current_stream())
            ev.append((name, e))

    def _to_device(self, x, np_dtype, be_dtype):
        if self.be.name == "torch" and hasattr(x, "is_cuda"):
            return x.to(device=self.be.device, dtype=be_dtype).contiguous()
        return self.be.from_numpy(_to_np(x, np_dtype))

    def train_sets(self, coords, feats, spp, descs, h_idx: np.ndarray, npoint_nearest: int = 800,
                   spp_pool: bool = True) -> TrainSets:
        """Training sets of point-level problems (pack_point_problems) on the device: gapro_partition_prepare on the
        whole input, then gapro_trainset_count / gapro_trainset_fill.  Pool mode reads the per-side row counts on the
        host once (its only synchronisation beside prepare's); nearest mode enqueues only.  A superpoint id range beyond
        the rank table raises (SPP_RANGE); non-finite input raises in pool mode and is a per-problem status in nearest
        mode: prepare's NOT_FINITE verdict on the whole input is set aside there, the centroid's fixed-point scale is
        taken from the finite coordinates by gapro_trainset_fill itself, and only the problems that meet the non-finite
        value fail."""
        lib, ctx, be = self.lib, self.ctx, self.be
        P = len(descs)
        d_coords = self._to_device(coords, np.float64, be.f64)
        d_feats = self._to_device(feats, np.float32, be.f32)
        d_spp = self._to_device(spp, np.int64, be.i64)
        N, D = int(d_feats.shape[0]), int(d_feats.shape[1])
        if tuple(d_coords.shape) != (N, 3) or int(d_spp.numel()) != N:
            raise ValueError("coords_float must be [N, 3], feats [N, D] and spp [N] for one N")
        self._stage("start")
        cap = max(4 * N, 1 << 20)
        pbytes = int(lib.gapro_partition_prepare_workspace_bytes(N, cap))
        prep_ws = be.empty(pbytes)
        spp_inv = be.empty(4 * N)
        hdr = SceneHeader()
        rc = lib.gapro_partition_prepare(ctx.handle, self._sh(), N, D, _ptr(d_coords), _ptr(d_feats), _ptr(d_spp), cap,
                                         _ptr(prep_ws), pbytes, _ptr(spp_inv), C.byref(hdr))
        if rc != 0 and not (rc == _lib.GAPRO_ERR_NOT_FINITE and not spp_pool):
            ctx.check(rc)
        self._stage("prepare")
        mode = _lib.TRAINSET_POOL if spp_pool else _lib.TRAINSET_NEAREST
        S = max(int(hdr.n_spps), 1)
        d_idx = be.from_numpy(h_idx)
        d_descs = be.empty(P * C.sizeof(TrainsetDesc))
        ws_bytes = int(lib.gapro_trainset_workspace_bytes(mode, C.cast(descs, C.c_void_p), P, S, D))
        ws = be.empty(ws_bytes)
        status = be.empty(4 * P)
        if spp_pool:
            counts = be.empty(8 * P)
            ctx.check(lib.gapro_trainset_count(ctx.handle, self._sh(), P, D, C.cast(descs, C.c_void_p), _ptr(d_descs), N,
                                               S, _ptr(spp_inv), _ptr(d_idx), _ptr(ws), ws_bytes, _ptr(counts),
                                               _ptr(status)))
            h_counts = _host(counts).view(np.int32)  # the call's one synchronisation beside prepare's
        rows = 0
        for i in range(P):
            d = descs[i]
            d.m1 = int(h_counts[2 * i]) if spp_pool else min(int(d.n1), int(npoint_nearest))
            d.m2 = int(h_counts[2 * i + 1]) if spp_pool else min(int(d.n2), int(npoint_nearest))
            d.row_offset = rows
            rows += d.m1 + d.m2
        train = be.empty(4 * rows * D)
        sel = be.empty(8 * rows)
        ctx.check(lib.gapro_trainset_fill(ctx.handle, self._sh(), mode, P, D, C.cast(descs, C.c_void_p), _ptr(d_descs), N,
                                          S, _ptr(d_coords), _ptr(d_feats), _ptr(d_spp), _ptr(spp_inv),
                                          int(hdr.fixed_shift), int(npoint_nearest), _ptr(d_idx), _ptr(ws), ws_bytes,
                                          rows, _ptr(train), _ptr(sel), _ptr(status)))
        self._stage("assemble")
        return TrainSets(train=train.view(be.f32).view(rows, D), sel=sel.view(be.i64), status=status.view(be.i32),
                         descs=descs, n_rows=rows, d_idx=d_idx, feats=d_feats,
                         keep=(d_coords, d_spp, spp_inv, prep_ws, ws, d_descs))

    def fit_points(self, coords, feats, spp, descs, h_idx: np.ndarray, npoint_nearest: int = 800, spp_pool: bool = True,
                   keep_models: bool = False, raise_on_failure: bool = True):
        """Point-level fits, on the device from end to end: train_sets, one fit launch on the assembled table (identity
        indices, zero initial variational mean), one predict launch that reads the trained states where the fit left
        them, at every intersection point's own feature row.  Returns a dict: probs, probs_new, mu, var f32 and labels
        u8 over all intersection points (problem i at [offsets[i], offsets[i + 1])), a per-problem ``status`` (the
        assembly's, else the fit's, else the prediction's) and, with ``keep_models``, ``models``."""
        ts = self.train_sets(coords, feats, spp, descs, h_idx, npoint_nearest, spp_pool)
        P = len(descs)
        # the fit launch's own test set is not wanted: every fit gets its first training row as a throw-away test row
        fd = (FitDesc * P)()
        pd = (PredictDesc * P)()
        fidx, io, oo = [], 0, 0
        offsets = np.zeros(P + 1, dtype=np.int64)
        for i in range(P):
            t, f = descs[i], fd[i]
            m = int(t.m1 + t.m2)
            f.m1, f.m2, f.t, f.b1, f.b2, f.scene = t.m1, t.m2, 1, 0, 1, i
            f.idx_offset, f.out_offset, f.ws_offset = io, i, 0
            fidx.append(np.arange(t.row_offset, t.row_offset + m + 1, dtype=np.int32))
            fidx[-1][m] = t.row_offset
            io += m + 1
            q = pd[i]
            q.row_offset, q.out_offset, q.t, q.reserved = t.idx_offset + t.n1 + t.n2, oo, t.t, 0
            oo += int(t.t)
            offsets[i + 1] = oo
        fidx = np.concatenate(fidx)
        h_m = np.array([descs[i].m1 + descs[i].m2 for i in range(P)], dtype=np.int32)
        no = max(oo, 1)
        flags0, prof = self.opt.reserved, self.profile_fit
        try:
            for attempt in range(2):
                pend = self.fit_launch(ts.train, fd, P, fidx, P, keep_models=True, state_to_host=keep_models)
                self._stage("fit")
                for i in range(P):
                    pd[i].state_offset = int(pend.state_off[i])
                out, pstat = self._predict_launch(pend.d_state, h_m, pd, ts.feats, ts.d_idx, no)
                self._stage("predict")
                flat = block_views(ROW_FIELDS, _host(out), no)
                st_pred = _host(pstat).view(np.int32)
                st_asm = _host(ts.status).view(np.int32)
                fit = self.fit_collect(pend, raise_on_failure=False)
                timed_out = fit["status"] == _lib.GAPRO_ERR_TIMEOUT
                if attempt or not timed_out.any() or not self.retry_timeouts:
                    break
                # a cluster member was not resident in time (transient): the launch once more on one workgroup per fit
                print("[gapro_amd] %d GP fit(s) timed out at a cluster barrier; retrying on one workgroup each"
                      % int(timed_out.sum()), file=sys.stderr)
                self.timeout_retries += int(timed_out.sum())
                self.opt.reserved = (int(flags0) | _lib.FIT_DBG_NO_CLUSTER) & ~_lib.FIT_DBG_CLUSTER_STALL
                self.profile_fit = False
        finally:
            self.opt.reserved, self.profile_fit = flags0, prof
        status = np.where(st_asm != 0, st_asm, np.where(fit["status"] != 0, fit["status"], st_pred)).astype(np.int32)
        res = {k: flat[k][:oo].copy() for k in flat}
        for i in np.nonzero(status)[0]:  # a failed problem's rows may not have been written at all
            for k in flat:
                res[k][offsets[i]:offsets[i + 1]] = 0
        res.update(status=status, offsets=offsets, loss=fit["loss"], train_sets=ts)
        if keep_models:
            res["models"] = fit["models"]
        if raise_on_failure and (status != 0).any():
            bad = int(np.nonzero(status)[0][0])
            raise _lib.GaproError(int(status[bad]), "point-level fit %d of %d failed" % (bad, P))
        return res

    # ------------------------------------------------------------------ stage D
    def fit_descs(self, feats_spp, descs, n_fits: int, h_idx: np.ndarray, n_out: int,
                  init_mean: Optional[np.ndarray] = None, keep_debug: bool = False, raise_on_failure: bool = True,
                  keep_models: bool = False):
        """Launch a batch of fits and wait for the results (numpy arrays); with ``keep_models`` also res["models"], the
        trained GPModel of every fit."""
        res = self.fit_collect(self.fit_launch(feats_spp, descs, n_fits, h_idx, n_out, init_mean, keep_debug,
                                               keep_models=keep_models), raise_on_failure=False)
        res = self._retry_timeouts(res, feats_spp, descs, h_idx, n_out, init_mean=init_mean)
        if raise_on_failure and (res["status"] != 0).any():
            bad = int(np.nonzero(res["status"])[0][0])
            raise _lib.GaproError(int(res["status"][bad]), "fit %d of %d failed" % (bad, n_fits))
        return res

    def reproducibility_probe(self, feats_spp, descs, n_fits: int, h_idx: np.ndarray, n_out: int, res=None,
                              init_mean: Optional[np.ndarray] = None, rel: float = 1e-11):
        """How far do a fit's outputs move when nothing but rounding-sized quantities change?  The same fits once more
        with the jitter on K_ZZ's diagonal scaled by (1 + rel) -- 1e-15 absolute on entries of size 0.7, a few ulps --
        compared with `res` (the unperturbed run; computed here when not given).  Returns (dv, dp) per fit: the largest
        relative change of sigma^2 and absolute change of p over the fit's test superpoints.  Well-behaved fits come
        back at 1e-7 .. 1e-6 (float32 output rounding and a little more); a fit beyond REPRO_SOFT amplifies last-bit differences ~1e9-fold over
        its fifty Adam steps, and NO float64 implementation reproduces its sigma^2 to north_star's 1e-4 -- the reference
        against itself on another BLAS included (on the S3DIS-shaped test scene: 2 of 66 fits, the
        two the oracle's own implementations disagree on).  Twice the work of the fits: a caller's choice
        (fit_gp_spp_batch(..., reproducibility_probe=True)), not the default.  (Perturbing the initial variational mean
        instead is useless as a probe: at 1e-13 it moves EVERY fit's sigma^2 by 1e-4 .. 9e-2 -- the optimisation is
        that sensitive to its starting point, which is why the reference's unseeded 1e-3 * randn start is switched off
        by default -- LABNOTES R6.)"""
        if res is None:
            res = self.fit_descs(feats_spp, descs, n_fits, h_idx, n_out, init_mean=init_mean, raise_on_failure=False)
        jit = float(self.opt.jitter)
        self.opt.jitter = jit * (1.0 + rel)
        try:
            r2 = self.fit_descs(feats_spp, descs, n_fits, h_idx, n_out, init_mean=init_mean, raise_on_failure=False)
        finally:
            self.opt.jitter = jit
        dv, dp = np.zeros(n_fits), np.zeros(n_fits)
        for k in range(n_fits):
            d = descs[k]
            a, b = int(d.out_offset), int(d.out_offset) + int(d.t)
            if b > a:
                v1, v2 = res["var"][a:b].astype(np.float64), r2["var"][a:b].astype(np.float64)
                dv[k] = float(np.max(np.abs(v1 - v2) / np.maximum(np.abs(v1), 1e-30)))
                dp[k] = float(np.max(np.abs(res["probs"][a:b].astype(np.float64) - r2["probs"][a:b].astype(np.float64))))
        return dv, dp

    def _retry_timeouts(self, res, feats_spp, descs, h_idx, n_out, init_mean=None, slot="s0", scene_keys=None,
                        keep_state=False):
        """Fits whose status is GAPRO_ERR_TIMEOUT are launched once more with the cluster kernel switched off
        (FIT_DBG_NO_CLUSTER: the LDS-staged kernel up to M_p = 512, the generic kernel beyond -- one
        workgroup each, no cross-workgroup barrier that could time out) and their outputs, status and loss replace the
        first attempt's.  A timeout says that a member of the fit's cluster was not given a CU within
        GAPRO_CLUSTER_BARRIER_TIMEOUT_MS; the arithmetic never ran to an end, so there is nothing deterministic about
        the failure and the second attempt computes what the first one would have (the per-fit result does not
        depend on the kernel beyond float64 round-off: tests/test_fit_gpu.py).  Same descriptors, same index array,
        same output offsets; only the workspace is the retry's own.  With ``keep_state`` the retry keeps its trained
        states on the device: res["retry_state"] = (state buffer, offset in doubles of every retried fit, in the order of
        res["retried"]), for a caller that predicts from the states where the launches left them."""
        bad = np.nonzero(res["status"] == _lib.GAPRO_ERR_TIMEOUT)[0]
        if not len(bad) or not self.retry_timeouts:
            return res
        sub = (FitDesc * len(bad))()
        for k, i in enumerate(bad):
            C.memmove(C.byref(sub, k * C.sizeof(FitDesc)), C.byref(descs, int(i) * C.sizeof(FitDesc)), C.sizeof(FitDesc))
        print("[gapro_amd] %d GP fit(s) timed out at a cluster barrier; retrying them on one workgroup each"
              % len(bad), file=sys.stderr)
        old, prof = self.opt.reserved, self.profile_fit
        self.opt.reserved = (int(old) | _lib.FIT_DBG_NO_CLUSTER) & ~_lib.FIT_DBG_CLUSTER_STALL
        self.profile_fit = False  # the retry is not a step of whoever is timing the launches
        try:
            pend = self.fit_launch(feats_spp, sub, len(bad), h_idx, n_out, init_mean, slot=slot + "retry",
                                   scene_keys=scene_keys, keep_models=keep_state or "models" in res,
                                   state_to_host="models" in res)
            r2 = self.fit_collect(pend, raise_on_failure=False)
        finally:
            self.opt.reserved, self.profile_fit = old, prof
            with self._ws_lock:
                self._ws.pop(slot + "retry", None)  # its workspace goes back to the allocator
        for k, i in enumerate(bad):
            d = descs[int(i)]
            a, b = int(d.out_offset), int(d.out_offset) + int(d.t)
            for key, _ in ROW_FIELDS:
                res[key][a:b] = r2[key][a:b]
            for key, _ in FIT_FIELDS:
                res[key][i] = r2[key][k]
            if "models" in res:
                res["models"][int(i)] = r2["models"][k]
        self.timeout_retries += len(bad)
        res["retried"] = [int(i) for i in bad]
        if keep_state:
            res["retry_state"] = (pend.d_state, [int(pend.state_off[k]) for k in range(len(bad))])
        return res

    def fit_launch(self, feats_spp, descs, n_fits: int, h_idx: np.ndarray, n_out: int,
                   init_mean: Optional[np.ndarray] = None, keep_debug: bool = False, slot: str = "s0",
                   scene_keys: Optional[Sequence[int]] = None, keep_models: bool = False,
                   state_to_host: bool = True) -> PendingFit:
        """Enqueue one launch.  ``keep_models`` keeps the trained states (PendingFit.d_state, on the device);
        ``state_to_host`` also brings them to the host, where fit_collect turns them into GPModels."""
        lib, ctx, be = self.lib, self.ctx, self.be
        D = int(feats_spp.shape[1])
        ws_bytes = int(lib.gapro_fit_plan_workspace(C.cast(descs, C.c_void_p), n_fits, D))
        if init_mean is None and self.init_mean_std > 0.0:
            # gpytorch: variational mean <- 0 + mean_init_std * randn on first call.  The noise of a
            # fit is a function of (seed, scene key, box pair) only, so a scene's result depends neither on the
            # batch it travels in nor on its position there, and a resumed run reproduces it.
            init_mean = np.zeros(len(h_idx))
            for k in range(n_fits):
                d = descs[k]
                key = int(scene_keys[d.scene]) if scene_keys is not None else int(d.scene)
                rng = np.random.default_rng([self.seed, key & 0xFFFFFFFF, int(d.b1), int(d.b2)])
                m = int(d.m1 + d.m2)
                init_mean[d.idx_offset:d.idx_offset + m] = self.init_mean_std * rng.standard_normal(m)
        d_descs = be.empty(n_fits * C.sizeof(FitDesc))
        d_idx = be.from_numpy(h_idx)
        d_init = be.from_numpy(np.ascontiguousarray(init_mean, dtype=np.float64)) if init_mean is not None else None
        # ONE workspace for all pipeline slots while launches are serialised (round 4): launch i + 1 starts on the device
        # when launch i has ended, nothing on the host reads a workspace (results leave through `out` / `stat`), and every
        # kernel initialises what it reads -- slots were already reused by other fits every third launch.  A worker's
        # first batches no longer pay three hipMallocs of ~18 GB (~2 s each: the driver clears VRAM on allocation; a
        # 1201-scene job is 3.5 s of GPU work), and a 256-scene pipeline holds 14 GB of workspace instead of 42.
        # Tests that inspect trained parameters (keep_debug) and overlapping launches keep a workspace per slot.
        ws_slot = "shared" if (self.serialize_fits and not keep_debug and not slot.endswith("retry")) else slot
        ws = self._workspace(ws_slot, ws_bytes // 8)
        no = max(n_out, 1)
        out = be.empty(block_bytes(ROW_FIELDS, no))  # per-test-superpoint outputs in one device block
        stat = be.empty(block_bytes(FIT_FIELDS, n_fits))  # per-fit loss, conditioning figure and status in another
        o, s = block_views(ROW_FIELDS, out, no, be), block_views(FIT_FIELDS, stat, n_fits, be)
        if self.profile_fit:
            tm = C.c_void_p()
            ctx.check(lib.gapro_fit_timing_create(ctx.handle, C.byref(tm)))
            ctx.check(lib.gapro_fit_timing_arm(ctx.handle, tm))
        # One fit launch at a time.  The software pipeline launches fit(i) when the partition kernels of batch i+1 have
        # completed, and those normally complete when fit(i-1) drains -- but now and then they slip in earlier, fit(i)
        # is enqueued with most of fit(i-1) still to run, and the members of its cluster fits become resident one by
        # one as CUs free up, spinning at their first barrier for hundreds of ms on CUs that fit(i-1) could use
        # (bench.py --steps 20: cluster kernels of 1.2 .. 1.5 s beside the usual 0.23 s, launches 12 % longer).
        prev = self._last_fit_done if self.serialize_fits else None
        if prev is not None:
            be.current_stream().wait_event(prev)
        # (_ex: the per-fit conditioning figure travels with the status)
        args = (ctx.handle, self._sh(), n_fits, D, _ptr(feats_spp), _ptr(d_idx), C.cast(descs, C.c_void_p),
                _ptr(d_descs), _ptr(d_init), C.byref(self.opt), _ptr(ws), ws_bytes, _ptr(o["probs"]),
                _ptr(o["probs_new"]), _ptr(o["labels"]), _ptr(o["mu"]), _ptr(o["var"]), _ptr(s["status"]),
                _ptr(s["loss"]), _ptr(s["cond"]))
        d_state, state_off, state_bytes = None, None, 0
        if not keep_models:
            ctx.check(lib.gapro_svgp_fit_batch_ex(*args))
        else:  # the same launch, and behind it the trained model of every fit in one route-independent layout
            state_off = np.zeros(max(n_fits, 1), dtype=np.int64)
            state_bytes = int(lib.gapro_gp_state_plan(C.cast(descs, C.c_void_p), n_fits, D, _ptr(state_off)))
            d_state = be.empty(max(state_bytes, 8))
            ctx.check(lib.gapro_svgp_fit_batch_state(*args, _ptr(d_state), _ptr(state_off), state_bytes))
        if self.profile_fit:
            raw = _desc_table(descs, n_fits)
            m = (raw[:, 0] + raw[:, 1]).copy()
            self.fit_events.append(FitTiming(ctx, tm, fit_flops_by_class(descs, n_fits, D, int(self.opt.training_iter),
                                                                         int(self.opt.reserved)), m))
            self.last_fit_m = m
        # results travel to pinned host memory on the same stream; nobody waits here
        h_out = self._pinned(slot + "fit_out", out.numel())
        h_stat = self._pinned(slot + "fit_stat", stat.numel())
        h_out[:out.numel()].copy_(out, non_blocking=True)
        h_stat[:stat.numel()].copy_(stat, non_blocking=True)
        h_state = None
        if d_state is not None and state_to_host:
            h_state = self._pinned(slot + "fit_state", max(state_bytes, 8))
            h_state[:max(state_bytes, 8)].copy_(d_state, non_blocking=True)
        done = be.event()
        done.record(be.current_stream())
        # The next launch stays ordered behind the result COPIES of this one, as in round 3.  ADVICE r03 suggested the
        # kernels' end instead (so that the host blocks for less inside the next gapro_svgp_fit_batch); measured, same
        # box, alternating, 10 steps: 322.8 / 327.3 scenes/s with it against 331.3 / 336.7 without (-2.7 %): the next
        # launch's descriptor upload and first workgroups then compete with this launch's copies and the host work
        # that follows them.
        self._last_fit_done = done
        keep = (d_descs, d_idx, d_init, ws, out, stat, feats_spp, d_state)  # alive until the launch has finished
        return PendingFit(done=done, h_out=h_out, h_stat=h_stat, no=no, n_fits=n_fits, ws_bytes=ws_bytes, keep=keep,
                          ws=ws if keep_debug else None, descs=descs if keep_debug else None, h_state=h_state,
                          state_off=state_off, state_bytes=state_bytes, d_state=d_state)

    def fit_collect(self, p: PendingFit, raise_on_failure: bool = True):
        """Results of a launch.  The library reports a gapro_status per fit and never fails the batch; with
        raise_on_failure (the fit_gp_spp API: gpytorch raises NotPSDError / NanError there) the first failed fit
        raises, otherwise the caller reads res["status"]."""
        p.done.synchronize()
        n_fits = p.n_fits
        # (cond: (max L_jj / min L_jj)^2 of every fit's last factorisation, a diagnostic: see reproducibility_probe)
        per_fit = {k: v[:n_fits].copy() for k, v in block_views(FIT_FIELDS, p.h_stat.numpy(), n_fits).items()}
        st = per_fit["status"]
        if raise_on_failure and (st != 0).any():
            bad = int(np.nonzero(st)[0][0])
            raise _lib.GaproError(int(st[bad]), "fit %d of %d failed" % (bad, n_fits))
        res = {k: v.copy() for k, v in block_views(ROW_FIELDS, p.h_out.numpy(), p.no).items()}
        res.update(per_fit, ws_bytes=p.ws_bytes)
        if p.h_state is not None:
            flat = p.h_state.numpy()[:p.state_bytes].view(np.float64)
            off = p.state_off
            res["models"] = [GPModel.from_state(flat[int(off[i]):]) for i in range(n_fits)]
        if p.ws is not None:
            res["workspace"] = p.ws.clone()  # the slot's workspace is reused by the next launch
            res["descs"] = p.descs
        p.keep = None
        return res
