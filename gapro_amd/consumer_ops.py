"""Consumer-side label ops on the GPU: the first thing ISBNet / SPFormer do with
the pseudo labels this package generates.  Same semantics as the reference lines cited per function; the work is
done by gapro_amd/csrc/consumer.hip behind the C ABI; the losses are ``torch.autograd.Function``s whose backward
uses the gradients the forward launch already produced.  There is no CPU path, with one exception:
``voxelization_idx`` on CPU tensors takes the library's host path (csrc/voxelize_host.cc), for DataLoader workers.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import Context, GaproError


# ---- the argument vocabulary: what every family refuses "before a device is touched", said once ---------------------
# A family raises its ValueErrors first and the RuntimeError for host tensors (_need_device) once they have passed.
_F32, _INT = (torch.float32,), (torch.int32, torch.int64)
_KINDS = {_F32: "a float32", _INT: "an int32 or int64"}
_INDEX_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)


def _need_device(*tensors):
    """The module's one refusal of host tensors; ``None`` stands for an argument that was not given."""
    if not all(t is None or t.is_cuda for t in tensors):
        raise RuntimeError("gapro_amd.consumer_ops works on HIP device tensors; there is no CPU fallback")


def _tensor_arg(who, name, t, shape, dtypes=_F32, nonempty=False, text=None):
    """``t`` must be a tensor of one of ``dtypes`` and of ``shape``, in which a str names a dimension of any size
    (``(N, "F")`` reads ``[5, F]`` in the message; ``text`` words the shape otherwise)."""
    ok = isinstance(t, torch.Tensor) and t.dtype in dtypes
    if ok:
        have = t.shape
        if have != shape:  # the wrong shape, or a named dimension (a plain loop: these checks run per sample and step)
            ok = len(have) == len(shape)
            for h, want in zip(have, shape):
                ok = ok and (h == want or want.__class__ is str)
        ok = ok and not (nonempty and 0 in have)
    if not ok:
        raise ValueError("%s: %s must be %s tensor of shape %s"
                         % (who, name, "a non-empty float32" if nonempty else _KINDS[dtypes],
                            text or "[%s]" % ", ".join(str(v) for v in shape)))


def _f32_arg(t, name, who, shape):
    """The predicted-instance families refuse a host tensor argument by argument, not behind all their ValueErrors."""
    _tensor_arg(who, name, t, shape, text=tuple(shape))
    _need_device(t)
    return t.contiguous()


def _one_device(who, dev, tensors):
    for t in tensors:
        if t.device != dev:
            raise ValueError("%s: tensors on %s and on %s; one device is expected" % (who, dev, t.device))


def _is_int(v, types=int):
    return isinstance(v, types) and not isinstance(v, bool)


def _is_finite(v):
    return _is_int(v, (int, float)) and v == v and abs(v) != float("inf")


def _finite_arg(who, name, v):
    if not _is_finite(v):
        raise ValueError("%s: %s must be a finite number" % (who, name))


def _positive_int_arg(who, name, v, types=int):
    if not _is_int(v, types) or v < 1:
        raise ValueError("%s: %s must be a positive int" % (who, name))


def _index_check(who, name, t):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype not in _INDEX_DTYPES:
        raise ValueError("%s: %s must be a 1-D integer tensor" % (who, name))


def _as_index(t):
    """An integer tensor as the kernels read it: contiguous int32 / int64, and whether it is int64."""
    if t.dtype not in _INT:
        t = t.to(torch.int32)
    return t.contiguous(), int(t.dtype == torch.int64)


def _index_arg(t, name, who, n=None):
    """A 1-D integer device tensor as contiguous int32 / int64, and whether it is int64."""
    _index_check(who, name, t)
    if n is not None and int(t.shape[0]) != n:
        raise ValueError("%s: %s has %d entries, expected %d" % (who, name, int(t.shape[0]), n))
    _need_device(t)
    return _as_index(t)


def _host_offsets_arg(who, batch_offsets, B, N):
    """``batch_offsets`` as ``B + 1`` host ints that do not decrease and stay inside ``[0, N]``."""
    if isinstance(batch_offsets, torch.Tensor):
        if batch_offsets.device.type != "cpu":
            raise ValueError("%s: batch_offsets must be on the host (a sequence, a NumPy array or a CPU tensor)" % who)
        batch_offsets = batch_offsets.tolist()
    try:
        off = [int(v) for v in batch_offsets]
        if any(o != v for o, v in zip(off, batch_offsets)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("%s: batch_offsets must be a host sequence of integers" % who) from None
    if len(off) != B + 1:
        raise ValueError("%s: %d batch offsets for batch_size %d; batch_size + 1 are expected" % (who, len(off), B))
    if off[0] < 0 or off[-1] > N or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError("%s: batch_offsets must not decrease and must stay inside [0, %d]" % (who, N))
    return off


def _n_spps_arg(who, n_spps, spps):
    """The bound of the superpoint ids: the caller's positive int, or ``max(spps) + 1`` of the device tensor."""
    if n_spps is not None:
        _positive_int_arg(who, "n_spps", n_spps)
    _need_device(spps)
    if n_spps is None:
        n_spps = max(int(spps.max()) + 1, 1)  # a host read; a negative id is refused by the device below
    return n_spps


def _ptr(t):
    """The address of a tensor for the C ABI; NULL for one that is absent or empty."""
    return t.data_ptr() if t is not None and t.numel() > 0 else None


def _row_contiguous(x):
    """A 2-D tensor whose rows the kernels can read in place (unit column stride, rows of any stride), else a copy."""
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def _ctx_stream(t):
    _need_device(t)
    ctx = Context.get(t.device.index or 0)
    return ctx, C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


# ---- the launch scaffold: workspace, status / header pair, the call's one host read ----------------------------------
def _workspace(who, nbytes, dev, beyond=None):
    """The bytes the library asked for as a device tensor.  0 bytes is the library's word for sizes beyond its bounds:
    a family that has such bounds names the sizes in ``beyond``."""
    if nbytes == 0 and beyond:
        raise ValueError("%s: %s beyond the library's bounds" % (who, beyond))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _status_pair(dev, count, dtype=torch.uint8, read=True):
    """A status / header buffer on the device and its page-locked twin (``None`` for a call that will not read it)."""
    return (torch.empty(count, dtype=dtype, device=dev),
            torch.empty(count, dtype=dtype, pin_memory=True) if read else None)


def _host_read(dev, h_buf, header=None):
    """The call's one host read: synchronise the current stream, then decode the page-locked buffer as the ``header``
    struct and the raw bytes behind it, or as status words."""
    torch.cuda.current_stream(dev).synchronize()
    if header is None:
        return h_buf.tolist()
    raw = h_buf.numpy().tobytes()
    return header.from_buffer_copy(raw), raw


def _refuse(who, status, flags, causes):
    """A non-zero status as the ``GaproError`` of the first cause whose bit is set."""
    if status != 0:
        raise GaproError(status, "%s: %s" % (who, next(text for bit, text in causes if flags & bit)))


def _predict_run(who, chain, anchor, inputs, params, keep, n_points, want_rows=True, want_masks=False, has_runs=True):
    """The protocol of the two predicted-instance chains: ``count``, the call's one host read of its header, ``fill``
    into tensors of the sizes read.  ``chain`` is (the prefix of the entry points, the header struct, the cause table,
    the result namedtuple); ``keep`` holds the tensors the structs point to.  Returns the namedtuple of device tensors,
    ``None`` where they were not asked for or the mode has no runs; ``n_runs``, the rows' run counts, came with the
    header."""
    prefix, header, causes, result = chain
    ctx, stream = _ctx_stream(anchor)
    lib, dev = ctx.lib, anchor.device
    pin, ppar = C.byref(inputs), C.byref(params)
    with torch.cuda.device(dev):
        ws_bytes, hdr_bytes = int(getattr(lib, prefix + "workspace_bytes")(pin, ppar)), int(
            getattr(lib, prefix + "header_bytes")(pin, ppar))
        ws = _workspace(who, ws_bytes, dev, "the sizes or parameters are")
        d_hdr, h_hdr = _status_pair(dev, hdr_bytes)
        ctx.check(getattr(lib, prefix + "count")(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws_bytes,
                                                 d_hdr.data_ptr(), h_hdr.data_ptr()))
        hdr, raw = _host_read(dev, h_hdr, header)
        _refuse(who, hdr.status, hdr.flags, causes)
        rows, runs = int(hdr.n_rows), int(hdr.total_runs)
        conf = torch.empty(rows, dtype=torch.float32, device=dev) if want_rows else None
        label = torch.empty(rows, dtype=torch.int32, device=dev) if want_rows else None
        box = torch.empty((rows, 6), dtype=torch.float32, device=dev) if want_rows else None
        query = torch.empty(rows, dtype=torch.int32, device=dev) if want_rows else None
        run_off = torch.zeros(rows + 1, dtype=torch.int64, device=dev) if has_runs else None
        d_runs = torch.empty(2 * runs, dtype=torch.int64, device=dev) if has_runs else None
        masks = torch.empty((rows, n_points), dtype=torch.uint8, device=dev) if want_masks else None
        if rows > 0:
            ctx.check(getattr(lib, prefix + "fill")(ctx.handle, stream, pin, ppar, ws.data_ptr(), ws_bytes, _ptr(conf),
                                                    _ptr(label), _ptr(box), _ptr(query), rows, _ptr(run_off),
                                                    _ptr(d_runs), runs, _ptr(masks), None))
    del keep
    n_runs = np.frombuffer(raw, dtype=np.int32, count=rows, offset=C.sizeof(header))
    return result(conf, label, box, query, run_off, d_runs, masks, hdr, n_runs)


def _counts_of(run_off, runs):
    """The rows' ``counts`` arrays (views of one host copy) from two host arrays."""
    return [runs[2 * int(run_off[r]):2 * int(run_off[r + 1])] for r in range(len(run_off) - 1)]


_constants = {}  # (device, the values) -> the float32 tensor on the device


def _device_constant(dev, values, dtype=torch.float32):
    """A tuple of numbers as a float32 (or ``dtype``) tensor on ``dev``: uploaded once per device and kept."""
    key = (dev, values) if dtype == torch.float32 else (dev, values, dtype)
    if key not in _constants:
        _constants[key] = torch.tensor(values, dtype=dtype).to(dev)
    return _constants[key]


def pool_labels_to_superpoints(prob_labels, mu_labels, var_labels, spps, n_out=None):
    """``custom_scatter_mean`` (ISBNet/isbnet/model/model_utils.py:600-613) of the three label channels in one
    pass (isbnet.py:387-389): float32 means per superpoint index, output length ``max(spps) + 1`` unless given.
    An index below 0 or at or above the output length is a ``ValueError``."""
    ctx, stream = _ctx_stream(prob_labels)
    dev = prob_labels.device
    idx = spps.to(device=dev, dtype=torch.int64).contiguous()
    chans = [t.to(device=dev, dtype=torch.float32).contiguous() for t in (prob_labels, mu_labels, var_labels)]
    n = int(idx.numel())
    lo, hi = (int(v) for v in torch.aminmax(idx)) if n else (0, -1)
    if n_out is None:
        n_out = hi + 1
    if n and (lo < 0 or hi >= n_out):
        raise ValueError("pool_labels_to_superpoints: superpoint indices span [%d, %d], outside [0, %d)" % (lo, hi, n_out))
    outs = [torch.zeros(n_out, dtype=torch.float32, device=dev) for _ in range(3)]
    if n == 0 or n_out == 0:
        return tuple(outs)
    sums = torch.empty(3 * n_out, dtype=torch.float64, device=dev)
    counts = torch.empty(n_out, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ctx.check(ctx.lib.gapro_label_pool_mean(ctx.handle, stream, n, n_out, idx.data_ptr(), chans[0].data_ptr(),
                                                chans[1].data_ptr(), chans[2].data_ptr(), sums.data_ptr(),
                                                counts.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                outs[2].data_ptr()))
    return tuple(outs)


class _WeightedBCE(torch.autograd.Function):
    @staticmethod
    def forward(fctx, logits, targets, weights):
        ctx, stream = _ctx_stream(logits)
        x = logits.to(torch.float32).contiguous()
        y = targets.to(device=x.device, dtype=torch.float32).contiguous()
        w = weights.to(device=x.device, dtype=torch.float32).contiguous()
        G, P = x.shape
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        grad = torch.empty_like(x) if logits.requires_grad else None
        acc = torch.empty(2, dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            ctx.check(ctx.lib.gapro_weighted_bce_with_logits(ctx.handle, stream, G, P, x.data_ptr(), y.data_ptr(),
                                                             w.data_ptr(), 1.0, acc.data_ptr(), loss.data_ptr(),
                                                             grad.data_ptr() if grad is not None else None))
        fctx.grad = grad
        fctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(fctx, grad_out):
        g = fctx.grad * grad_out if fctx.grad is not None else None
        return (g.to(fctx.in_dtype) if g is not None else None), None, None


def prob_weighted_bce_with_logits(mask_logit_pred, inst_label, prob_labels):
    """``(bce * prob_labels).sum() / prob_labels.sum() / (num_gt + 1e-6)`` with ``bce =
    F.binary_cross_entropy_with_logits(mask_logit_pred, inst_label, reduction="none")`` over [num_gt, n_points]
    (ISBNet/isbnet/model/criterion.py:287-288)."""
    return _WeightedBCE.apply(mask_logit_pred, inst_label, prob_labels)


class _KLToGP(torch.autograd.Function):
    @staticmethod
    def forward(fctx, mu_pred, logvar_pred, mu_labels, var_labels, weight, epsilon):
        ctx, stream = _ctx_stream(mu_pred)
        dev = mu_pred.device
        mp = mu_pred.to(torch.float32).contiguous().view(-1)
        lp = logvar_pred.to(torch.float32).contiguous().view(-1)
        ml = mu_labels.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        vl = var_labels.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        n = int(mp.numel())
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        need = mu_pred.requires_grad or logvar_pred.requires_grad
        gm = torch.empty_like(mp) if need else None
        gl = torch.empty_like(lp) if need else None
        if n:
            acc = torch.empty(4, dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                ctx.check(ctx.lib.gapro_kl_gp_loss(ctx.handle, stream, n, ml.data_ptr(), vl.data_ptr(), mp.data_ptr(),
                                                   lp.data_ptr(), float(epsilon), float(weight), 1.0, acc.data_ptr(),
                                                   loss.data_ptr(), gm.data_ptr() if need else None,
                                                   gl.data_ptr() if need else None))
        fctx.grads = (gm, gl)
        fctx.shapes = (mu_pred.shape, logvar_pred.shape, mu_pred.dtype, logvar_pred.dtype)
        return loss

    @staticmethod
    def backward(fctx, grad_out):
        gm, gl = fctx.grads
        s_mu, s_lv, d_mu, d_lv = fctx.shapes
        if gm is None:
            return None, None, None, None, None, None
        return ((gm * grad_out).view(s_mu).to(d_mu), (gl * grad_out).view(s_lv).to(d_lv), None, None, None, None)


def kl_to_gp_loss(mu_pred, logvar_pred, mu_labels, var_labels, weight=1.0, epsilon=1e-4):
    """The KL-to-GP auxiliary loss of ISBNet/isbnet/model/criterion.py:435-463 (``weight`` = loss_weight["kl_loss"])."""
    return _KLToGP.apply(mu_pred, logvar_pred, mu_labels, var_labels, weight, epsilon)


# ---- instance-label preparation (gapro_amd/csrc/inst_prep.hip) ----------------------------------------
ID_TABLE = 1024  # ids the first launch of a call has room for; a larger id regrows the table from the data
InstanceLabels = namedtuple("InstanceLabels", ["instance_labels", "instance_cls", "instance_box", "instance_pointnum",
                                               "centroid_offset_labels", "corners_offset_labels"])
_LABEL_CODES = {torch.float64: _lib.GAPRO_LABEL_F64, torch.int32: _lib.GAPRO_LABEL_I32,
                torch.int64: _lib.GAPRO_LABEL_I64}


def _label_code(t, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: a tensor is expected, not %s" % (what, type(t).__name__))
    if t.dtype not in _LABEL_CODES:
        raise ValueError("%s: dtype %s; int32, int64 or float64 is expected" % (what, t.dtype))
    if t.dim() != 1:
        raise ValueError("%s: shape %s; one label per point is expected" % (what, tuple(t.shape)))
    return _LABEL_CODES[t.dtype]


def _check_info_args(coords_float, instance_labels, semantic_labels, who):
    """What is refused before a device is touched."""
    _tensor_arg(who, "coords_float", coords_float, ("V", 3))
    _label_code(instance_labels, who + ": instance_labels")
    _label_code(semantic_labels, who + ": semantic_labels")
    v = int(coords_float.shape[0])
    if int(instance_labels.shape[0]) != v or int(semantic_labels.shape[0]) != v:
        raise ValueError("%s: %d points, %d instance labels, %d semantic labels"
                         % (who, v, int(instance_labels.shape[0]), int(semantic_labels.shape[0])))
    if v == 0:
        raise ValueError("%s: no points" % who)
    _need_device(coords_float, instance_labels, semantic_labels)


def _refusal(who, hdr):
    if hdr.max_id >= _lib.INST_PREP_MAX_IDS:
        why = "an instance id at or beyond %d" % _lib.INST_PREP_MAX_IDS
    elif hdr.status == _lib.GAPRO_ERR_NOT_FINITE:
        why = "a non-finite coordinate on a point that carries an instance id"
    elif hdr.flags & 2:
        why = "a float64 label that is no integer"
    elif hdr.n_ids == 0:
        why = "no instance id >= 0"
    else:
        why = "%d distinct ids below the largest id %d: an id in between is empty" % (hdr.n_ids, hdr.max_id)
    return GaproError(hdr.status, "%s: %s" % (who, why))


def _inst_prep(who, labels, coords=None, sem=None, label_shift=0, crop=True):
    """One chain of gapro_inst_crop / gapro_inst_info / gapro_inst_prepare on the caller's stream and the one read of
    its header; an id beyond the id table regrows the table from the header's largest id and runs again (a refused
    call has written nothing).  ``labels`` is contiguous and is overwritten when ``crop``."""
    ctx, stream = _ctx_stream(labels)
    lib, dev = ctx.lib, labels.device
    n = int(labels.shape[0])
    info = coords is not None
    cap = ID_TABLE
    with torch.cuda.device(dev):
        while True:
            ws = _workspace(who, int(lib.gapro_inst_prep_workspace_bytes(cap)), dev)
            ws_bytes = ws.numel()
            d_hdr, h_hdr = _status_pair(dev, C.sizeof(_lib.InstPrepHeader))
            outs = None
            if info:
                outs = (torch.empty(cap, dtype=torch.int64, device=dev),
                        torch.empty((cap, 6), dtype=torch.float32, device=dev),
                        torch.empty(cap, dtype=torch.int32, device=dev),
                        torch.empty((n, 3), dtype=torch.float32, device=dev),
                        torch.empty((n, 6), dtype=torch.float32, device=dev))
                fn = lib.gapro_inst_prepare if crop else lib.gapro_inst_info
                ctx.check(fn(ctx.handle, stream, n, coords.data_ptr(), labels.data_ptr(), _LABEL_CODES[labels.dtype],
                             sem.data_ptr(), _LABEL_CODES[sem.dtype], int(label_shift), cap, ws.data_ptr(), ws_bytes,
                             *(o.data_ptr() for o in outs), d_hdr.data_ptr(), h_hdr.data_ptr()))
            else:
                ctx.check(lib.gapro_inst_crop(ctx.handle, stream, n, labels.data_ptr(), _LABEL_CODES[labels.dtype], cap,
                                              ws.data_ptr(), ws_bytes, d_hdr.data_ptr(), h_hdr.data_ptr()))
            hdr, _ = _host_read(dev, h_hdr, _lib.InstPrepHeader)
            if hdr.status == _lib.GAPRO_ERR_WORKSPACE and cap <= hdr.max_id < _lib.INST_PREP_MAX_IDS:
                cap = hdr.max_id + 1
                continue
            if hdr.status != 0:
                raise _refusal(who, hdr)
            return hdr, outs


def get_cropped_instance_label(instance_label, valid_idxs=None):
    """``get_cropped_instance_label`` (ISBNet/isbnet/model/model_utils.py:589-597) without its loop over the ids: the
    holes of [0, K), K = the number of distinct ids >= 0, take the ids >= K, the largest first.  As in the reference the
    given tensor is overwritten and returned; with ``valid_idxs`` the indexed copy is.  int32, int64 or float64 labels."""
    _label_code(instance_label, "get_cropped_instance_label: instance_label")
    if valid_idxs is not None:
        instance_label = instance_label[valid_idxs]
    if instance_label.numel() == 0:
        raise ValueError("get_cropped_instance_label: no labels")
    work = instance_label if instance_label.is_contiguous() else instance_label.contiguous()
    _inst_prep("get_cropped_instance_label", work)
    if work is not instance_label:
        instance_label.copy_(work)
    return instance_label


def get_instance_info(coords_float, instance_labels, semantic_labels, label_shift=0):
    """``get_instance_info`` (ISBNet/isbnet/model/model_utils.py:519-555) in one pass over the points: ``(instance_cls
    i64[I], instance_box f32[I,6], centroid_offset_labels f32[V,3], corners_offset_labels f32[V,6])``, I = max id + 1.
    The centroid is the exact mean rounded once, everything else the reference's bits.  Labels with an
    empty id below the largest, or without an id >= 0, are refused, where the reference fails."""
    _check_info_args(coords_float, instance_labels, semantic_labels, "get_instance_info")
    hdr, (cls, box, _, cen, cor) = _inst_prep("get_instance_info", instance_labels.contiguous(),
                                              coords_float.contiguous(), semantic_labels.contiguous(), label_shift,
                                              crop=False)
    num = int(hdr.instance_num)
    return cls[:num], box[:num], cen, cor


def prepare_instance_labels(coords_float, instance_labels, semantic_labels, label_shift=0):
    """``get_cropped_instance_label`` followed by ``get_instance_info`` (isbnet.py:254-270) as one chain of kernels with
    one host read: an ``InstanceLabels`` tuple of the compacted labels (a new tensor), the class, box and point count
    per instance and the two offset tables."""
    _check_info_args(coords_float, instance_labels, semantic_labels, "prepare_instance_labels")
    labels = instance_labels.clone(memory_format=torch.contiguous_format)
    hdr, (cls, box, num_pts, cen, cor) = _inst_prep("prepare_instance_labels", labels, coords_float.contiguous(),
                                                    semantic_labels.contiguous(), label_shift)
    num = int(hdr.instance_num)
    return InstanceLabels(labels, cls[:num], box[:num], num_pts[:num], cen, cor)


# ---- ground-truth instance masks per sample (gapro_amd/csrc/spp_gt.hip) ----------------------------------
_GT_CAUSES = ((1, "batch offsets that decrease or leave [0, n_points]"),
              (2, "a subsample index outside the labels"),
              (4, "an instance label that is not ignore_label and is negative, at or beyond len(instance_cls), or no "
                  "integer"),
              (8, "a superpoint id outside [0, n_spps)"))


def _offsets_arg(batch_offsets, batch_size, who):
    """The offsets as the host sees them before a device is touched: a tensor (device or host) or a sequence."""
    if isinstance(batch_offsets, torch.Tensor):
        if batch_offsets.dim() != 1 or batch_offsets.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s: batch_offsets must be a 1-D int32 or int64 tensor" % who)
        off = batch_offsets
    else:
        try:
            off = torch.as_tensor([int(v) for v in batch_offsets], dtype=torch.int64)
        except (TypeError, ValueError):
            raise ValueError("%s: batch_offsets must be an integer tensor or a sequence of integers" % who) from None
    if int(off.shape[0]) != batch_size + 1:
        raise ValueError("%s: %d batch offsets for batch_size %d; batch_size + 1 are expected"
                         % (who, int(off.shape[0]), batch_size))
    return off


def _check_gt_args(who, instance_labels, instance_cls, instance_box, batch_size):
    """What both functions refuse before a device is touched; returns the label and class codes."""
    code = _label_code(instance_labels, who + ": instance_labels")
    cls_code = _label_code(instance_cls, who + ": instance_cls")
    if not _is_int(batch_size):
        raise ValueError("%s: batch_size must be an int" % who)
    if not 1 <= batch_size <= _lib.SPP_GT_MAX_SAMPLES:
        raise ValueError("%s: batch_size %d outside [1, %d]" % (who, batch_size, _lib.SPP_GT_MAX_SAMPLES))
    n_cls = int(instance_cls.shape[0])
    if not isinstance(instance_box, torch.Tensor) or instance_box.dtype != torch.float32 \
            or instance_box.dim() != 2 or tuple(instance_box.shape) != (n_cls, 6):
        raise ValueError("%s: instance_box must be a float32 tensor of shape [%d, 6], one row per instance_cls entry"
                         % (who, n_cls))
    if int(instance_labels.shape[0]) == 0:
        raise ValueError("%s: no points" % who)
    if n_cls == 0 or n_cls > _lib.INST_PREP_MAX_IDS:
        raise ValueError("%s: %d instance_cls entries outside [1, %d]" % (who, n_cls, _lib.INST_PREP_MAX_IDS))
    return code, cls_code


def _gt_run(who, labels, gather, spps, n_spps, cls, box, offsets, batch_size, ignore_label, rule, return_ids):
    """gapro_spp_gt_count, the call's one host read of its header, gapro_spp_gt_fill; the per-sample views."""
    _need_device(labels, cls, box, gather, spps)
    ctx, stream = _ctx_stream(labels)
    lib, dev = ctx.lib, labels.device
    labels, cls, box = labels.contiguous(), cls.contiguous(), box.contiguous()
    off = offsets.to(device=dev, dtype=torch.int64).contiguous()
    if gather is not None:
        gather = gather.to(dtype=torch.int64).contiguous()
    spps, spp_i64 = (None, 0) if spps is None else _as_index(spps)
    n = int(gather.shape[0]) if gather is not None else int(labels.shape[0])
    n_cls = int(cls.shape[0])
    with torch.cuda.device(dev):
        ws = _workspace(who, int(lib.gapro_spp_gt_workspace_bytes(n, batch_size, n_cls, n_spps)), dev,
                        "%d points, batch_size %d and %d superpoint ids are" % (n, batch_size, n_spps))
        ws_bytes = ws.numel()
        d_hdr, h_hdr = _status_pair(dev, C.sizeof(_lib.SppGtHeader) + 8 * batch_size)
        common = (n, int(labels.shape[0]), labels.data_ptr(), _LABEL_CODES[labels.dtype], _ptr(gather), _ptr(spps),
                  spp_i64, n_spps, cls.data_ptr(), _LABEL_CODES[cls.dtype], n_cls)
        ctx.check(lib.gapro_spp_gt_count(ctx.handle, stream, *common, off.data_ptr(), batch_size, int(ignore_label),
                                         ws.data_ptr(), ws_bytes, d_hdr.data_ptr(), h_hdr.data_ptr()))
        hdr, raw = _host_read(dev, h_hdr, _lib.SppGtHeader)
        _refuse("%s: sample %d" % (who, hdr.bad_sample), hdr.status, hdr.flags, _GT_CAUSES)
        counts = (C.c_int32 * (2 * batch_size)).from_buffer_copy(raw, C.sizeof(_lib.SppGtHeader))
        if hdr.total_rows == 0:
            return [None] * batch_size
        cells, rows = max(int(hdr.total_cells), 1), int(hdr.total_rows)
        mask = torch.empty(cells, dtype=torch.float32, device=dev)
        out_cls = torch.empty(rows, dtype=cls.dtype, device=dev)
        out_box = torch.empty((rows, 6), dtype=torch.float32, device=dev)
        out_ids = torch.empty(rows, dtype=torch.int64, device=dev) if return_ids else None
        ctx.check(lib.gapro_spp_gt_fill(ctx.handle, stream, *common, box.data_ptr(), off.data_ptr(), batch_size,
                                        int(ignore_label), rule, ws.data_ptr(), ws_bytes, mask.data_ptr(), cells,
                                        out_cls.data_ptr(), out_box.data_ptr(), _ptr(out_ids), rows, None))
    out, r0, c0 = [], 0, 0
    for b in range(batch_size):
        ni, ns = int(counts[2 * b]), int(counts[2 * b + 1])
        if ni == 0:
            out.append(None)
            continue
        entry = {"mask": mask[c0:c0 + ni * ns].view(ni, ns), "cls": out_cls[r0:r0 + ni], "box": out_box[r0:r0 + ni]}
        if return_ids:
            entry["ids"] = out_ids[r0:r0 + ni]
        out.append(entry)
        r0 += ni
        c0 += ni * ns
    return out


def get_spp_gt(instance_labels, spps, instance_cls, instance_box, batch_offsets, batch_size, ignore_label=-100,
               pool=True, *, n_spps=None, strict=False, return_ids=False):
    """``get_spp_gt`` (ISBNet/isbnet/model/model_utils.py:692-738, called at isbnet.py:377-385) without its loops over
    the samples and the instance ids: a list of ``batch_size`` entries, ``None`` for a sample without a kept instance
    (or without points), else ``{"mask": f32[n_inst_gt, n_spp], "cls": instance_cls[ids], "box": instance_box[ids]}``
    and, with ``return_ids``, ``"ids"`` (int64).  All masks of a call are views into one allocation; so are all
    ``cls``, ``box`` and ``ids``.

    Sample ``b`` holds the points ``[batch_offsets[b], batch_offsets[b + 1])``.  Its columns are the distinct superpoint
    ids of its points, ascending; its rows the distinct labels, ascending, that differ from ``ignore_label`` and have
    ``instance_cls[id] >= 0``.  With c(i, s) the points of superpoint s labelled i and n(s) all points of s, ignored
    ones included, ``mask[i, s] = 1`` iff ``2 c >= n`` -- with ``strict`` iff ``2 c > n`` (the ``> 0.5`` of
    SPFormer/spformer/dataset/scannetv2.py:252-253).  For n(s) < 2^24 the integer rule is the reference's float32
    ``scatter_mean(mask) >= 0.5`` to the bit; beyond that count the integer rule is the definition.

    ``n_spps`` bounds the ids (``[0, n_spps)``); ``None`` takes ``int(spps.max()) + 1``, a second host read beside the
    call's one -- ISBNet callers pass the pooled length they hold.  ``batch_offsets`` is an int32 / int64 tensor on
    either side or a sequence.  ``pool=False`` is what ``get_subsample_gt`` does.  Data the reference would mis-index
    or fail on (a label outside ``instance_cls``, a superpoint id outside the bound, offsets out of order) is a
    ``GaproError`` and nothing is written.  No autograd: these are targets."""
    who = "get_spp_gt"
    if not pool:
        raise ValueError("get_spp_gt: pool=False makes every point its own column, which is get_subsample_gt (with "
                         "subsample_idxs = arange): call get_subsample_gt")
    _check_gt_args(who, instance_labels, instance_cls, instance_box, batch_size)
    _index_check(who, "spps", spps)
    if int(spps.shape[0]) != int(instance_labels.shape[0]):
        raise ValueError("%s: %d labels, %d superpoint ids" % (who, int(instance_labels.shape[0]), int(spps.shape[0])))
    off = _offsets_arg(batch_offsets, batch_size, who)
    n_spps = _n_spps_arg(who, n_spps, spps)
    return _gt_run(who, instance_labels, None, spps, n_spps, instance_cls, instance_box, off, batch_size, ignore_label,
                   _lib.SPP_GT_STRICT if strict else _lib.SPP_GT_HALF, return_ids)


def get_subsample_gt(instance_labels, subsample_idxs, instance_cls, instance_box, subsample_batch_offsets, batch_size,
                     ignore_label=-100, *, return_ids=False):
    """``get_subsample_gt`` (ISBNet/isbnet/model/model_utils.py:647-689, isbnet.py:399-401): the rows of ``get_spp_gt``
    over the sample's subsampled points, ``mask[i, p] = (instance_labels[subsample_idxs[p]] == id_i)`` for the ``p`` of
    ``[subsample_batch_offsets[b], subsample_batch_offsets[b + 1])``.  Same return, refusals and single host read."""
    who = "get_subsample_gt"
    _check_gt_args(who, instance_labels, instance_cls, instance_box, batch_size)
    _index_check(who, "subsample_idxs", subsample_idxs)
    if int(subsample_idxs.shape[0]) == 0:
        raise ValueError("%s: no points" % who)
    off = _offsets_arg(subsample_batch_offsets, batch_size, who)
    return _gt_run(who, instance_labels, subsample_idxs, None, 0, instance_cls, instance_box, off, batch_size,
                   ignore_label, _lib.SPP_GT_HALF, return_ids)


# ---- the Hungarian matcher (gapro_amd/csrc/match_cost.hip, lsap.cc) --------------------------------------
MATCH_WEIGHTS = (0.5, 1.0, 1.0, 0.2, 0.2)  # class, dice, bce, conf, giou (ISBNet/isbnet/model/matcher.py:192)
_WEIGHT_NAMES = ("class", "dice", "bce", "conf", "giou")
_MATCH_CAUSES = ((1, "a class label outside [0, n_classes)"), (2, "a mask value that is neither 0 nor 1"))
_GT_KEYS = ("row_indices", "inst_labels", "cls_labels", "box_labels")


def _weights_arg(weights, who):
    if weights is None:
        return None
    try:
        vals = [float(weights[k]) for k in _WEIGHT_NAMES] if isinstance(weights, dict) else [float(v) for v in weights]
    except (TypeError, ValueError, KeyError):
        raise ValueError("%s: weights must be five numbers (class, dice, bce, conf, giou) or a dict with these keys"
                         % who) from None
    if len(vals) != 5 or (isinstance(weights, dict) and len(weights) != 5):
        raise ValueError("%s: weights must be five numbers (class, dice, bce, conf, giou) or a dict with these keys" % who)
    if any(not _is_finite(v) or v < 0.0 for v in vals):
        raise ValueError("%s: a weight is negative or not finite" % who)
    return _lib.MatchWeights(*vals)


def _heads_arg(who, cls_logits, conf_logits, box_preds, **lists):
    """The prediction heads the matcher and the matched losses take, and the per-sample ``lists`` beside them; returns
    B, Q and C."""
    _tensor_arg(who, "cls_logits", cls_logits, ("B", "Q", "C"), nonempty=True)
    B, Q, n_classes = (int(v) for v in cls_logits.shape)
    _tensor_arg(who, "conf_logits", conf_logits, (B, Q))
    _tensor_arg(who, "box_preds", box_preds, (B, Q, 6))
    if B > _lib.SPP_GT_MAX_SAMPLES:
        raise ValueError("%s: batch size %d beyond %d" % (who, B, _lib.SPP_GT_MAX_SAMPLES))
    for name, seq in lists.items():
        if not isinstance(seq, (list, tuple)) or len(seq) != B:
            raise ValueError("%s: %s must be a list of %d entries, one per sample" % (who, name, B))
    return B, Q, n_classes


def _sample_labels_arg(who, cls_name, cls, box_name, box, n, cls_dtype):
    """A sample's class and box labels, ``n`` rows each, the classes of the dtype of every earlier sample's."""
    _tensor_arg(who, cls_name, cls, (n,), _INT)
    if cls_dtype not in (None, cls.dtype):
        raise ValueError("%s: %s is %s, an earlier sample's %s" % (who, cls_name, cls.dtype, cls_dtype))
    _tensor_arg(who, box_name, box, (n, 6))
    return cls.dtype


def _sample_logits_arg(who, x, Q, n_cols, column):
    """A sample's mask logits: one row per query and one column per ``column``."""
    _tensor_arg(who, "mask_logits", x, ("Q", "S"))
    if x.shape != (Q, n_cols) or n_cols == 0:
        raise ValueError("%s: mask_logits is %s, [%d, %d] is expected: one row per query and one column per %s"
                         % (who, tuple(x.shape), Q, n_cols, column))


def _check_match_args(who, cls_logits, mask_logits, conf_logits, box_preds, dc_inst_mask_arr):
    """What is refused before a device is touched; returns the samples that have instances and the class dtype."""
    _, Q, _ = _heads_arg(who, cls_logits, conf_logits, box_preds, mask_logits=mask_logits,
                         dc_inst_mask_arr=dc_inst_mask_arr)
    tensors = [conf_logits, box_preds]
    kept, cls_dtype = [], None
    for b, entry in enumerate(dc_inst_mask_arr):
        if entry is None:
            continue
        who_b = "%s: sample %d" % (who, b)
        if not isinstance(entry, dict) or any(not isinstance(entry.get(k), torch.Tensor) for k in ("mask", "cls", "box")):
            raise ValueError("%s: a dict with the tensors mask, cls and box, or None, is expected" % who_b)
        mask, cls, box, x = entry["mask"], entry["cls"], entry["box"], mask_logits[b]
        _tensor_arg(who_b, "mask", mask, ("I", "S"), nonempty=True)
        n_inst, n_cols = (int(v) for v in mask.shape)
        cls_dtype = _sample_labels_arg(who_b, "cls", cls, "box", box, n_inst, cls_dtype)
        _sample_logits_arg(who_b, x, Q, n_cols, "column of the mask")
        tensors += [mask, cls, box, x]
        kept.append(b)
    _one_device(who, cls_logits.device, tensors)
    return kept, cls_dtype


def _match_run(who, cls_logits, mask_logits, conf_logits, box_preds, entries, kept, cls_dtype, weights, pinned):
    """One gapro_match_cost on the caller's stream and one synchronisation for its status (and, with ``pinned``, the
    cost in page-locked memory): the per-sample device views and the host array."""
    ctx, stream = _ctx_stream(cls_logits)
    lib, dev = ctx.lib, cls_logits.device
    B, Q, n_classes = (int(v) for v in cls_logits.shape)
    cls_logits, conf_logits, box_preds = cls_logits.contiguous(), conf_logits.contiguous(), box_preds.contiguous()
    tasks = (_lib.MatchTask * B)()
    keep, offsets, total, total_inst, total_cols = [], {}, 0, 0, 0
    for b in kept:
        e, x = entries[b], _row_contiguous(mask_logits[b])
        mask, cls, box = e["mask"].contiguous(), e["cls"].contiguous(), e["box"].contiguous()
        keep += [x, mask, cls, box]  # alive until the call has been enqueued and synchronised
        n_inst, n_cols = (int(v) for v in mask.shape)
        tasks[b] = _lib.MatchTask(x.data_ptr(), int(x.stride(0)), mask.data_ptr(), cls.data_ptr(), box.data_ptr(),
                                  n_inst, n_cols, total)
        offsets[b] = (total, n_inst)
        total += Q * n_inst
        total_inst += n_inst
        total_cols += n_cols
    with torch.cuda.device(dev):
        ws = _workspace(who, int(lib.gapro_match_cost_workspace_bytes(B, Q, total_inst, total_cols)), dev,
                        "%d samples, %d queries and %d instances are" % (B, Q, total_inst))
        cost = torch.empty(total, dtype=torch.float32, device=dev)
        d_status, h_status = _status_pair(dev, _lib.MATCH_STATUS_WORDS, torch.int32)
        h_cost = torch.empty(total, dtype=torch.float32, pin_memory=True) if pinned else None
        ctx.check(lib.gapro_match_cost(ctx.handle, stream, C.cast(tasks, C.c_void_p), B, Q, n_classes,
                                       _LABEL_CODES[cls_dtype], cls_logits.data_ptr(), conf_logits.data_ptr(),
                                       box_preds.data_ptr(), C.byref(weights) if weights is not None else None,
                                       ws.data_ptr(), ws.numel(), cost.data_ptr(), total, _ptr(h_cost),
                                       d_status.data_ptr(), h_status.data_ptr()))
        status, bad, flags = _host_read(dev, h_status)[:3]
    _refuse("%s: sample %d" % (who, bad), status, flags, _MATCH_CAUSES)
    views = [None] * B
    host = [None] * B
    for b, (off, n_inst) in offsets.items():
        views[b] = cost[off:off + Q * n_inst].view(Q, n_inst)
        if pinned:
            host[b] = h_cost.numpy()[off:off + Q * n_inst].reshape(Q, n_inst)
    return views, host


def match_cost(cls_logits, mask_logits, conf_logits, box_preds, dc_inst_mask_arr, *, weights=None):
    """The cost matrices of ``HungarianMatcher.get_match`` (ISBNet/isbnet/model/matcher.py:156-197) for a whole batch in
    one call: a list with ``None`` (a sample whose ``dc_inst_mask_arr`` entry is ``None``) or a device ``f32[Q, I_b]``
    tensor per sample, all of them views into one allocation.

    ``cls_logits`` is ``f32[B, Q, C]``, ``conf_logits`` ``f32[B, Q]``, ``box_preds`` ``f32[B, Q, 6]``; ``mask_logits``
    the reference's list (``None`` or ``f32[Q, S_b]`` per sample; an entry whose rows are not contiguous is copied);
    ``dc_inst_mask_arr`` what ``get_spp_gt`` / ``get_subsample_gt`` return.  ``weights`` are five numbers (class, dice,
    bce, conf, giou) or a dict with these keys; ``None`` is the reference's 0.5, 1, 1, 0.2, 0.2.

    Every term is evaluated in float64 and the cost rounded to float32 once; an entry that is then NaN
    or infinite becomes 100000.  Shape, dtype and device mismatches are ``ValueError``s before a device is touched; a
    class label outside ``[0, C)`` or a mask value other than 0 / 1 is a ``GaproError`` and nothing is written.  One
    host read (the status).  No autograd: the reference runs this under ``no_grad``."""
    who = "match_cost"
    kept, cls_dtype = _check_match_args(who, cls_logits, mask_logits, conf_logits, box_preds, dc_inst_mask_arr)
    w = _weights_arg(weights, who)
    if not kept:
        return [None] * len(dc_inst_mask_arr)
    return _match_run(who, cls_logits.detach(), [None if x is None else x.detach() for x in mask_logits],
                      conf_logits.detach(), box_preds.detach(), dc_inst_mask_arr, kept, cls_dtype, w, False)[0]


def linear_sum_assignment(cost, dup=1):
    """``scipy.optimize.linear_sum_assignment`` of a float32 NumPy matrix by the library's own solver (no device):
    ``(rows, cols)`` as int64 arrays, rows ascending.  ``dup > 1`` solves ``np.tile(cost, (1, dup))`` without building
    it and returns the ORIGINAL column ``j % cost.shape[1]`` of every pair.  Among equal-cost optima the choice is the
    solver's own (include/gapro_hip.h) and the same for every run.  A non-finite entry is a ``GaproError``."""
    who = "linear_sum_assignment"
    if not isinstance(cost, np.ndarray) or cost.ndim != 2 or cost.dtype != np.float32:
        raise ValueError("%s: a two-dimensional float32 NumPy array is expected" % who)
    _positive_int_arg(who, "dup", dup, (int, np.integer))
    n_rows, n_cols = cost.shape
    if n_rows == 0 or n_cols == 0:
        raise ValueError("%s: an empty matrix" % who)
    if cost.strides[1] != 4 or cost.strides[0] < 4 * n_cols or cost.strides[0] % 4:
        cost = np.ascontiguousarray(cost)
    n = min(n_rows, int(dup) * n_cols)
    rows, cols, n_out = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), C.c_int32(0)
    rc = _lib.load().gapro_lsap_solve(n_rows, n_cols, cost.ctypes.data, cost.strides[0] // 4, int(dup), C.byref(n_out),
                                      rows.ctypes.data, cols.ctypes.data)
    if rc != 0:
        raise GaproError(rc, "%s: %s" % (who, "a non-finite cost" if rc == _lib.GAPRO_ERR_NOT_FINITE else "bad argument"))
    assert n_out.value == n
    return rows.astype(np.int64), cols.astype(np.int64)


MATCH_SOLVER_THREADS = 4  # host threads hungarian_match solves a batch's assignments on; 1: in the caller's thread
_solver_pool = None


def _solve_all(problems):
    """``linear_sum_assignment(cost, dup)`` of every problem, in their order.  The solver is a C call that holds no
    Python state, so the problems of a batch (two per sample, independent) run on a few threads: the largest first."""
    global _solver_pool
    if MATCH_SOLVER_THREADS <= 1 or len(problems) < 2:
        return [linear_sum_assignment(c, d) for c, d in problems]
    if _solver_pool is None or _solver_pool[0] != MATCH_SOLVER_THREADS:
        from concurrent.futures import ThreadPoolExecutor

        _solver_pool = (MATCH_SOLVER_THREADS,
                        ThreadPoolExecutor(max_workers=MATCH_SOLVER_THREADS, thread_name_prefix="gapro-lsap"))
    order = sorted(range(len(problems)), key=lambda k: -min(problems[k][0].shape[0],
                                                            problems[k][1] * problems[k][0].shape[1]))
    futures = {k: _solver_pool[1].submit(linear_sum_assignment, *problems[k]) for k in order}
    return [futures[k].result() for k in range(len(problems))]


def hungarian_match(cls_logits, mask_logits, conf_logits, box_preds, dc_inst_mask_arr, dup_gt=1):
    """``HungarianMatcher.forward_dup`` (ISBNet/isbnet/model/matcher.py:208-284, called at criterion.py:398) without its
    loop of small launches and host copies: ``(gt_dict, aux_gt_dict)``, each with the lists ``row_indices`` (NumPy
    int64, as the reference's), ``inst_labels``, ``cls_labels`` and ``box_labels`` (device tensors: the matched rows of
    the sample's mask, cls and box), ``None`` for a sample without an instance.  ``aux_gt_dict`` is the assignment with
    every instance offered ``dup_gt`` times.

    One ``match_cost`` call writes the batch's costs into page-locked memory, ONE stream synchronisation covers the whole
    batch, the ``2 B`` assignments are solved by the library on the host (on ``MATCH_SOLVER_THREADS`` threads; the
    result does not depend on their number), and one upload carries all matched columns to the gathers.  A batch of
    ``None``s returns without a launch.  Among equal-cost optima the assignment is the solver's own, not necessarily
    SciPy's."""
    who = "hungarian_match"
    kept, cls_dtype = _check_match_args(who, cls_logits, mask_logits, conf_logits, box_preds, dc_inst_mask_arr)
    _positive_int_arg(who, "dup_gt", dup_gt)
    B = len(dc_inst_mask_arr)
    gt, aux = ({k: [None] * B for k in _GT_KEYS} for _ in range(2))
    if not kept:
        return gt, aux
    _, host = _match_run(who, cls_logits.detach(), [None if x is None else x.detach() for x in mask_logits],
                         conf_logits.detach(), box_preds.detach(), dc_inst_mask_arr, kept, cls_dtype, None, True)
    problems = [(out, b, dup) for b in kept for out, dup in ((gt, 1), (aux, dup_gt))]
    solved = _solve_all([(host[b], dup) for _, b, dup in problems])
    picks = []  # (dict, sample, first, count) of the columns in `cols`
    cols, n = [], 0
    for (out, b, _), (r, c) in zip(problems, solved):
        out["row_indices"][b] = r
        picks.append((out, b, n, len(c)))
        cols.append(c)
        n += len(c)
    dev = cls_logits.device
    staged = torch.empty(n, dtype=torch.int64, pin_memory=True)
    staged.numpy()[:] = np.concatenate(cols)
    index = staged.to(dev, non_blocking=True)  # the one upload
    for out, b, first, count in picks:
        idx, e = index[first:first + count], dc_inst_mask_arr[b]
        out["inst_labels"][b] = e["mask"].index_select(0, idx)
        out["cls_labels"][b] = e["cls"].index_select(0, idx)
        out["box_labels"][b] = e["box"].index_select(0, idx)
    return gt, aux


# ---- the matched losses (gapro_amd/csrc/match_loss.hip) -------------------------------------------------
LOSS_NAMES = ("dice_loss", "bce_loss", "cls_loss", "iou_loss", "box_loss", "giou_loss", "levelset_loss")


def _check_loss_args(who, cls_logits, mask_logits, conf_logits, box_preds, prob_labels, batch_offsets, levelset_feats,
                     levelset_coords, gt_dict, empty_weight, voxel_scale):
    """What is refused before a device is touched; returns the kept samples, their host row indices (int32 NumPy), the
    offsets as ints and the class dtype."""
    B, Q, n_classes = _heads_arg(who, cls_logits, conf_logits, box_preds, mask_logits=mask_logits)
    if not isinstance(gt_dict, dict) or any(not isinstance(gt_dict.get(k), (list, tuple)) or len(gt_dict[k]) != B
                                            for k in _GT_KEYS):
        raise ValueError("%s: gt_dict must hold the lists %s of %d entries, as hungarian_match returns them"
                         % (who, ", ".join(_GT_KEYS), B))
    _tensor_arg(who, "prob_labels", prob_labels, ("N",), nonempty=True)
    N = int(prob_labels.shape[0])
    _tensor_arg(who, "levelset_feats", levelset_feats, (N, "F"))
    if not 1 <= int(levelset_feats.shape[1]) <= _lib.MATCH_LOSS_MAX_FEATS:
        raise ValueError("%s: %d level-set features; 1 to %d are expected"
                         % (who, int(levelset_feats.shape[1]), _lib.MATCH_LOSS_MAX_FEATS))
    _tensor_arg(who, "levelset_coords", levelset_coords, (N, 3))
    if empty_weight is not None:
        _tensor_arg(who, "empty_weight", empty_weight, (n_classes,))
    _finite_arg(who, "voxel_scale", voxel_scale)
    off = _host_offsets_arg(who, batch_offsets, B, N)
    tensors = [conf_logits, box_preds, prob_labels, levelset_feats, levelset_coords]
    if empty_weight is not None:
        tensors.append(empty_weight)
    kept, rows_host, cls_dtype = [], {}, None
    for b in range(B):
        x, rows = mask_logits[b], gt_dict["row_indices"][b]
        if x is None or rows is None:
            continue
        who_b = "%s: sample %d" % (who, b)
        if isinstance(rows, torch.Tensor):
            if rows.device.type != "cpu":
                raise ValueError("%s: row_indices must be on the host (NumPy or a CPU tensor)" % who_b)
            rows = rows.numpy()
        if not isinstance(rows, np.ndarray) or rows.ndim != 1 or rows.dtype.kind not in "iu":
            raise ValueError("%s: row_indices must be a 1-D integer NumPy array or CPU tensor" % who_b)
        n_gt = int(rows.shape[0])
        if n_gt == 0:
            raise ValueError("%s: row_indices is empty; a sample without a match is None" % who_b)
        if int(rows.min()) < 0 or int(rows.max()) >= Q:
            raise ValueError("%s: a row index outside [0, %d)" % (who_b, Q))
        if len(np.unique(rows)) != n_gt:
            raise ValueError("%s: a row index is listed twice" % who_b)
        n_cols = off[b + 1] - off[b]
        _sample_logits_arg(who_b, x, Q, n_cols, "point of batch_offsets, at least one")
        inst, cls, box = (gt_dict[k][b] for k in ("inst_labels", "cls_labels", "box_labels"))
        _tensor_arg(who_b, "inst_labels", inst, (n_gt, n_cols))
        cls_dtype = _sample_labels_arg(who_b, "cls_labels", cls, "box_labels", box, n_gt, cls_dtype)
        tensors += [x, inst, cls, box]
        kept.append(b)
        rows_host[b] = rows.astype(np.int32)
    _one_device(who, cls_logits.device, tensors)
    return kept, rows_host, off, cls_dtype


class _MatchedLosses(torch.autograd.Function):
    """The one autograd node of ``matched_losses``: ``f32[7]`` forward, one kernel backward."""

    @staticmethod
    def forward(fctx, plan, cls_logits, conf_logits, box_preds, *mask_logits):
        who = "matched_losses"
        ctx, stream = _ctx_stream(cls_logits)
        lib, dev = ctx.lib, cls_logits.device
        B, Q, n_classes = (int(v) for v in cls_logits.shape)
        cls_logits, conf_logits, box_preds = cls_logits.contiguous(), conf_logits.contiguous(), box_preds.contiguous()
        gt, off = plan["gt"], plan["off"]
        tasks = (_lib.MatchLossTask * B)()
        keep, xs, total_gt, grad_spans, grad_floats = [], [], 0, [], 0
        for b, x in zip(plan["kept"], mask_logits):
            x = _row_contiguous(x)
            inst, cls, box = (gt[k][b].contiguous() for k in ("inst_labels", "cls_labels", "box_labels"))
            keep += [inst, cls, box]  # alive until the backward has run
            xs.append(x)
            n_gt, n_cols = (int(v) for v in inst.shape)
            tasks[b] = _lib.MatchLossTask(x.data_ptr(), int(x.stride(0)), inst.data_ptr(), cls.data_ptr(),
                                          box.data_ptr(), n_gt, n_cols, off[b], total_gt)
            total_gt += n_gt
            grad_spans.append((grad_floats, n_cols))
            grad_floats += Q * n_cols
        rows = np.ascontiguousarray(np.concatenate([plan["rows"][b] for b in plan["kept"]]), dtype=np.int32)
        prob, feats, coords = (plan[k].contiguous() for k in ("prob", "feats", "coords"))
        weight = plan["weight"].contiguous()
        with torch.cuda.device(dev):
            ws = _workspace(who, int(lib.gapro_match_loss_workspace_bytes(B, Q, total_gt)), dev,
                            "%d samples, %d queries and %d matched rows are" % (B, Q, total_gt))
            ws_bytes = ws.numel()
            out = torch.empty(_lib.MATCH_LOSS_N, dtype=torch.float32, device=dev)
            d_status, h_status = _status_pair(dev, _lib.MATCH_STATUS_WORDS, torch.int32, read=plan["check"])
            args = (B, Q, n_classes, _LABEL_CODES[plan["cls_dtype"]], int(feats.shape[1]))
            ctx.check(lib.gapro_match_loss_forward(ctx.handle, stream, C.cast(tasks, C.c_void_p), rows.ctypes.data,
                                                   *args, cls_logits.data_ptr(), conf_logits.data_ptr(),
                                                   box_preds.data_ptr(), prob.data_ptr(), feats.data_ptr(),
                                                   coords.data_ptr(), int(prob.shape[0]), weight.data_ptr(),
                                                   plan["voxel_scale"], ws.data_ptr(), ws_bytes, out.data_ptr(),
                                                   d_status.data_ptr(), _ptr(h_status)))
            if h_status is not None:  # the call's one host read, asked for by check=True
                status, bad = _host_read(dev, h_status)[:2]
                if status != 0:
                    raise GaproError(status, "%s: sample %d: a class label outside [0, n_classes)" % (who, bad))
        fctx.save_for_backward(cls_logits, conf_logits, box_preds, *xs)
        fctx.held = (keep, prob, feats, coords, weight, ws, ws_bytes, args, total_gt, plan["voxel_scale"],
                     grad_spans, grad_floats)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out):
        cls_logits, conf_logits, box_preds, *xs = fctx.saved_tensors
        _, prob, feats, coords, weight, ws, ws_bytes, args, total_gt, voxel_scale, grad_spans, grad_floats = fctx.held
        ctx, stream = _ctx_stream(cls_logits)
        dev = cls_logits.device
        need = fctx.needs_input_grad
        B, Q = args[0], args[1]
        grad_out = grad_out.to(dtype=torch.float32).contiguous()
        g_cls = torch.empty_like(cls_logits) if need[1] else None
        g_conf = torch.empty_like(conf_logits) if need[2] else None
        g_box = torch.empty_like(box_preds) if need[3] else None
        g_mask = torch.empty(grad_floats, dtype=torch.float32, device=dev) if any(need[4:]) else None
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.gapro_match_loss_backward(ctx.handle, stream, *args, total_gt, cls_logits.data_ptr(),
                                                        conf_logits.data_ptr(), box_preds.data_ptr(), prob.data_ptr(),
                                                        feats.data_ptr(), coords.data_ptr(), weight.data_ptr(),
                                                        voxel_scale, ws.data_ptr(), ws_bytes, grad_out.data_ptr(),
                                                        _ptr(g_cls), _ptr(g_mask), _ptr(g_conf), _ptr(g_box)))
        masks = [g_mask[first:first + Q * n_cols].view(Q, n_cols) if need[4 + k] else None
                 for k, (first, n_cols) in enumerate(grad_spans)]
        return (None, g_cls, g_conf, g_box, *masks)


def matched_losses(cls_logits, mask_logits, conf_logits, box_preds, prob_labels, batch_offsets, levelset_feats,
                   levelset_coords, gt_dict, *, empty_weight=None, voxel_scale=50, check=True):
    """The seven main losses of ``Criterion.single_layer_loss`` (ISBNet/isbnet/model/criterion.py:235-331, called at
    :414) for a whole batch: a dict with the reference's keys ``dice_loss``, ``bce_loss``, ``cls_loss``, ``iou_loss``,
    ``box_loss``, ``giou_loss``, ``levelset_loss`` (device scalars, selections of ONE ``f32[7]`` of one autograd node)
    and ``kl_loss``, a constant zero.  Two kernels forward; ``sum(w[k] * losses[k]).backward()`` runs one kernel, which
    reads the upstream ``f32[7]`` on the device, and gives gradients for ``cls_logits``, every ``mask_logits[b]``,
    ``conf_logits`` and ``box_preds`` (zeros in the rows no instance matched; ``None`` for a skipped sample's logits).

    The arguments are ``single_layer_loss``'s with the four label lists taken as ``gt_dict``, what ``hungarian_match``
    returns: ``prob_labels`` ``f32[N]``, ``batch_offsets`` ``B + 1`` host integers with ``mask_logits[b]`` of
    ``batch_offsets[b + 1] - batch_offsets[b]`` columns, ``levelset_feats`` ``f32[N, F]`` (1 <= F <= 8),
    ``levelset_coords`` ``f32[N, 3]``.  ``empty_weight`` is ``Criterion.empty_weight`` (``f32[C]``; ``None``: ones with
    the last entry 0.1).  A sample whose ``mask_logits[b]`` or ``row_indices[b]`` is ``None`` is skipped as in the
    reference: nothing is added for it, and it counts in the division by B.  A batch of skipped samples returns zeros
    without a launch of the library.

    Float64 from the float32 inputs, rounded once; no floating-point atomics, so two calls give equal
    bytes.  Mismatched shapes, dtypes or devices, row indices that are empty, on the device, out of ``[0, Q)`` or listed
    twice, offsets out of order and a ``voxel_scale`` that is not finite are ``ValueError``s before a device is touched.
    A class label outside ``[0, C)`` is refused by the device: with ``check=True`` the status is read behind the kernels
    (the call's one synchronisation) and a ``GaproError`` raised; with ``check=False`` the call only enqueues, the seven
    losses are NaN and the backward writes zeros."""
    who = "matched_losses"
    kept, rows_host, off, cls_dtype = _check_loss_args(who, cls_logits, mask_logits, conf_logits, box_preds,
                                                       prob_labels, batch_offsets, levelset_feats, levelset_coords,
                                                       gt_dict, empty_weight, voxel_scale)
    dev = cls_logits.device
    if not kept:
        zeros = torch.zeros(_lib.MATCH_LOSS_N + 1, dtype=torch.float32, device=dev)
        return {name: zeros[k] for k, name in enumerate(LOSS_NAMES + ("kl_loss",))}
    _need_device(cls_logits)
    if empty_weight is None:
        empty_weight = _empty_weight_of(dev, int(cls_logits.shape[2]) - 1, 0.1, None)
    weight = empty_weight.detach()
    plan = {"kept": kept, "rows": rows_host, "off": off, "cls_dtype": cls_dtype, "gt": gt_dict,
            "prob": prob_labels.detach(), "feats": levelset_feats.detach(), "coords": levelset_coords.detach(),
            "weight": weight, "voxel_scale": float(voxel_scale), "check": bool(check)}
    out = _MatchedLosses.apply(plan, cls_logits, conf_logits, box_preds, *[mask_logits[b] for b in kept])
    losses = dict(zip(LOSS_NAMES, out.unbind(0)))  # one node between the dict and the function
    losses["kl_loss"] = torch.zeros((), dtype=torch.float32, device=dev)
    return losses


# ---- the point-wise losses (gapro_amd/csrc/point_loss.hip) -----------------------------------------------
POINT_LOSS_NAMES = ("pw_sem_loss", "pw_corners_loss", "pw_giou_loss", "pw_conf_loss")


def _semantic_weight_arg(who, semantic_weight, n_classes, dev):
    """``None``, a float32 tensor of shape [C] or a sequence of C numbers (what ``Criterion`` holds) -> ``None`` or the
    tensor on ``dev``; a sequence is uploaded once per device and kept."""
    if semantic_weight is None:
        return None
    if isinstance(semantic_weight, torch.Tensor):
        _tensor_arg(who, "semantic_weight", semantic_weight, (n_classes,))
        _one_device(who, dev, [semantic_weight])
        return semantic_weight.detach()
    try:
        vals = tuple(float(v) for v in semantic_weight)
    except (TypeError, ValueError):
        raise ValueError("%s: semantic_weight must be None, a float32 tensor or a sequence of numbers" % who) from None
    if not vals:
        return None  # the reference tests the list's truth
    if len(vals) != n_classes:
        raise ValueError("%s: %d semantic weights for %d classes" % (who, len(vals), n_classes))
    return _device_constant(dev, vals)


def _check_point_args(who, semantic_scores, corners_offset, box_conf, semantic_labels, instance_labels,
                      corners_offset_labels, coords_float, ignore_label, voxel_scale):
    """What is refused before a device is touched; returns N and C."""
    _tensor_arg(who, "semantic_scores", semantic_scores, ("N", "C"))
    N, n_classes = (int(v) for v in semantic_scores.shape)
    if not _lib.POINT_LOSS_MIN_CLASSES <= n_classes <= _lib.POINT_LOSS_MAX_CLASSES:
        raise ValueError("%s: %d classes; %d to %d are expected"
                         % (who, n_classes, _lib.POINT_LOSS_MIN_CLASSES, _lib.POINT_LOSS_MAX_CLASSES))
    if N > _lib.POINT_LOSS_MAX_POINTS:
        raise ValueError("%s: %d points are beyond the library's bound of %d" % (who, N, _lib.POINT_LOSS_MAX_POINTS))
    for name, t, width in (("corners_offset", corners_offset, 6), ("corners_offset_labels", corners_offset_labels, 6),
                           ("coords_float", coords_float, 3)):
        _tensor_arg(who, name, t, (N, width))
    if not isinstance(box_conf, torch.Tensor) or box_conf.dtype != torch.float32 \
            or tuple(box_conf.shape) not in ((N,), (N, 1)):
        raise ValueError("%s: box_conf must be a float32 tensor of shape [%d] or [%d, 1]" % (who, N, N))
    for name, t in (("semantic_labels", semantic_labels), ("instance_labels", instance_labels)):
        _tensor_arg(who, name, t, (N,), _INT)
    if not _is_int(ignore_label) or not -2 ** 63 <= ignore_label < 2 ** 63:
        raise ValueError("%s: ignore_label must be an int" % who)
    _finite_arg(who, "voxel_scale", voxel_scale)
    _one_device(who, semantic_scores.device, (corners_offset, box_conf, semantic_labels, instance_labels,
                                              corners_offset_labels, coords_float))
    return N, n_classes


class _PointWiseLosses(torch.autograd.Function):
    """The one autograd node of ``point_wise_losses``: ``f32[4]`` forward, one kernel backward."""

    @staticmethod
    def forward(fctx, plan, semantic_scores, corners_offset, box_conf):
        who = "point_wise_losses"
        ctx, stream = _ctx_stream(semantic_scores)
        lib, dev = ctx.lib, semantic_scores.device
        N, n_classes = (int(v) for v in semantic_scores.shape)
        z = _row_contiguous(semantic_scores)
        corners, conf = corners_offset.contiguous(), box_conf.contiguous()
        sem, inst, labels, coords, weight = (None if plan[k] is None else plan[k].contiguous()
                                             for k in ("sem", "inst", "labels", "coords", "weight"))
        with torch.cuda.device(dev):
            ws = _workspace(who, int(lib.gapro_point_loss_workspace_bytes(N, n_classes)), dev,
                            "%d points and %d classes are" % (N, n_classes))
            out = torch.empty(_lib.POINT_LOSS_N, dtype=torch.float32, device=dev)
            d_status, h_status = _status_pair(dev, _lib.MATCH_STATUS_WORDS, torch.int32, read=plan["check"])
            args = (N, n_classes, z.data_ptr(), int(z.stride(0)), sem.data_ptr(), _LABEL_CODES[sem.dtype],
                    inst.data_ptr(), _LABEL_CODES[inst.dtype], corners.data_ptr(), conf.data_ptr(), labels.data_ptr(),
                    coords.data_ptr(), _ptr(weight), plan["ignore_label"], plan["voxel_scale"], ws.data_ptr(),
                    ws.numel())
            ctx.check(lib.gapro_point_loss_forward(ctx.handle, stream, *args, out.data_ptr(), d_status.data_ptr(),
                                                   _ptr(h_status)))
            if h_status is not None:  # the call's one host read, asked for by check=True
                status, bad = _host_read(dev, h_status)[:2]
                if status != 0:
                    raise GaproError(status, "%s: point %d: a semantic label that is neither ignore_label nor in "
                                             "[0, %d)" % (who, bad, n_classes))
        fctx.save_for_backward(z, corners, conf)
        fctx.held = (sem, inst, labels, coords, weight, ws, args)  # alive until the backward has run
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out):
        z, corners, conf = fctx.saved_tensors
        args = fctx.held[-1]
        ctx, stream = _ctx_stream(z)
        dev = z.device
        need = fctx.needs_input_grad
        grad_out = grad_out.to(dtype=torch.float32).contiguous()
        g_z = torch.empty((args[0], args[1]), dtype=torch.float32, device=dev) if need[1] else None
        g_corners = torch.empty_like(corners) if need[2] else None
        g_conf = torch.empty_like(conf) if need[3] else None
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.gapro_point_loss_backward(ctx.handle, stream, *args, grad_out.data_ptr(), _ptr(g_z),
                                                        _ptr(g_corners), _ptr(g_conf)))
        return None, g_z, g_corners, g_conf


def point_wise_losses(semantic_scores, corners_offset, box_conf, semantic_labels, instance_labels,
                      corners_offset_labels, coords_float, *, semantic_weight=None, ignore_label=-100, voxel_scale=50,
                      check=True):
    """The four point-wise losses of ``Criterion.cal_point_wise_loss`` (ISBNet/isbnet/model/criterion.py:136-191, called
    at :357) over all N voxels of a batch, in its argument order: a dict with the reference's keys ``pw_sem_loss``,
    ``pw_corners_loss``, ``pw_giou_loss``, ``pw_conf_loss`` (device scalars, selections of ONE ``f32[4]`` of one
    autograd node).  Two kernels forward and no host read: the reference's six boolean-mask gathers and its
    ``total_pos_inds == 0`` test are gone.  ``sum(w[k] * losses[k]).backward()`` runs one kernel, which reads the
    upstream ``f32[4]`` on the device and writes whole gradients for ``semantic_scores``, ``corners_offset`` and
    ``box_conf`` (zeros where a label is ignored).

    ``semantic_scores`` is ``f32[N, C]`` with 2 <= C <= 64 (rows of any stride are read in place; other layouts are
    copied), ``corners_offset`` and ``corners_offset_labels`` ``f32[N, 6]``, ``box_conf`` ``f32[N]`` or ``f32[N, 1]``,
    the two label arrays int32 or int64 ``[N]`` (each its own type), ``coords_float`` ``f32[N, 3]``;
    ``semantic_weight`` is ``None``, ``f32[C]`` or a sequence of C numbers.

    Float64 from the float32 inputs, rounded once; no floating-point atomics, so two calls give equal
    bytes.  When no instance label differs from ``ignore_label`` the last three losses are exactly 0 with zero gradients
    (the reference's ``0 * corners_offset.sum()`` would be NaN for non-finite inputs); when every semantic label is
    ignored ``pw_sem_loss`` is NaN and its gradient zero, as ``F.cross_entropy``.  ``N == 0`` returns that NaN and three
    zeros without a launch.  Mismatched shapes, dtypes or devices, C outside its range, an ``ignore_label`` that is not
    an int and a ``voxel_scale`` that is not finite are ``ValueError``s before a device is touched.  A semantic label
    that is neither ``ignore_label`` nor in ``[0, C)`` is refused by the device: with ``check=True`` the status is read
    behind the kernels (the call's one synchronisation) and a ``GaproError`` names the lowest such point; with
    ``check=False`` the call only enqueues, the four losses are NaN and the backward writes zeros."""
    who = "point_wise_losses"
    N, n_classes = _check_point_args(who, semantic_scores, corners_offset, box_conf, semantic_labels, instance_labels,
                                     corners_offset_labels, coords_float, ignore_label, voxel_scale)
    dev = semantic_scores.device
    weight = _semantic_weight_arg(who, semantic_weight, n_classes, dev)
    if N == 0:
        out = torch.tensor([float("nan"), 0.0, 0.0, 0.0], dtype=torch.float32).to(dev)
        return dict(zip(POINT_LOSS_NAMES, out.unbind(0)))
    _need_device(semantic_scores)
    plan = {"sem": semantic_labels, "inst": instance_labels, "labels": corners_offset_labels.detach(),
            "coords": coords_float.detach(), "weight": weight, "ignore_label": int(ignore_label),
            "voxel_scale": float(voxel_scale), "check": bool(check)}
    out = _PointWiseLosses.apply(plan, semantic_scores, corners_offset, box_conf)
    return dict(zip(POINT_LOSS_NAMES, out.unbind(0)))  # one node between the dict and the function


# ---- the whole criterion: a composition, no kernel of its own ------------------------------------------
LOSS_WEIGHT = {"dice_loss": 1, "bce_loss": 1, "cls_loss": 0.5, "iou_loss": 0.5, "box_loss": 0.5, "giou_loss": 0.5,
               "levelset_loss": 0.5, "kl_loss": 0.1}  # Criterion.loss_weight (criterion.py:125-134)
_BATCH_KEYS = ("semantic_labels", "instance_labels")
_PW_BATCH_KEYS = ("coords_float", "corners_offset_labels")
_PW_MODEL_KEYS = ("semantic_scores", "corners_offset", "box_conf")
_MAIN_MODEL_KEYS = ("cls_logits", "mask_logits", "conf_logits", "box_preds", "dc_inst_mask_arr", "dc_prob_labels",
                    "dc_batch_offsets", "dc_rgb_feats", "dc_coords_float", "dc_mu_labels", "dc_var_labels", "mu_pred",
                    "logvar_pred")


def _empty_weight_of(dev, instance_classes, eos_coef, semantic_weight):
    """``Criterion.__init__``'s ``empty_weight`` (criterion.py:107-111): ones, ``eos_coef`` last, and the semantic
    weights shifted by ``label_shift = 1`` when given."""
    classes = range(1, instance_classes + 1)
    return _device_constant(dev, tuple(float(semantic_weight[i]) if semantic_weight else 1.0 for i in classes)
                            + (float(eos_coef),))


def criterion_losses(batch_inputs, model_outputs, *, instance_classes=18, semantic_weight=None, ignore_label=-100,
                     eos_coef=0.1, semantic_only=True, trainall=False, voxel_scale=50, loss_weight=None, dup_gt=4,
                     check=True):
    """What ``Criterion.forward`` (ISBNet/isbnet/model/criterion.py:333-465) means, with the constructor's arguments as
    keywords: it reads the same keys of ``batch_inputs`` and ``model_outputs``, takes the same branches and returns the
    same keys in the same insertion order.  (As released, ``forward`` passes ``cls_logits.shape[:1]`` as
    ``batch_size`` and stops with a ``TypeError``; this is the call with the int.)

    1. ``model_outputs is None``: ``{"Placeholder": 0}``, a leaf with ``requires_grad``.
    2. ``semantic_only or trainall``: ``point_wise_losses``; with ``semantic_only`` they are returned here, unscaled.
    3. Every key containing ``"pw"`` is multiplied by 0.25.
    4. ``hungarian_match(..., dup_gt=dup_gt)``, then ``matched_losses`` with ``Criterion.empty_weight`` (ones,
       ``eos_coef`` last, ``semantic_weight[i]`` at ``i - 1`` when given), each value times ``loss_weight`` (default
       ``LOSS_WEIGHT``, the reference's eight values).
    5. ``kl_loss = kl_to_gp_loss(mu_pred, logvar_pred, dc_mu_labels, dc_var_labels, weight=loss_weight["kl_loss"])``.

    Pure composition: no kernel and no arithmetic rule of its own.  ``semantic_weight`` is ``None`` or a sequence of
    numbers, one per semantic class.  ``dc_batch_offsets`` may be host integers or a tensor; a DEVICE tensor costs one
    host read.  ``check=True`` adds the one status read of each of the two loss calls (``hungarian_match`` always has
    one).  A missing key, a ``loss_weight`` without exactly the eight keys or with a value that is not finite, and an
    ``instance_classes`` or ``dup_gt`` that is not a positive int are ``ValueError``s before a device is touched, as is
    everything the composed calls refuse."""
    who = "criterion_losses"
    if not isinstance(batch_inputs, dict):
        raise ValueError("%s: batch_inputs must be a dict" % who)
    if model_outputs is not None and not isinstance(model_outputs, dict):
        raise ValueError("%s: model_outputs must be a dict or None" % who)
    _positive_int_arg(who, "instance_classes", instance_classes)
    _positive_int_arg(who, "dup_gt", dup_gt)
    _finite_arg(who, "eos_coef", eos_coef)
    weights = dict(LOSS_WEIGHT) if loss_weight is None else loss_weight
    if not isinstance(weights, dict) or list(weights) != list(LOSS_WEIGHT) \
            or any(not _is_finite(v) for v in weights.values()):
        raise ValueError("%s: loss_weight must be a dict of finite numbers with the keys %s, in this order"
                         % (who, ", ".join(LOSS_WEIGHT)))
    if semantic_weight is not None:
        try:
            semantic_weight = tuple(float(v) for v in semantic_weight) or None
        except (TypeError, ValueError):
            raise ValueError("%s: semantic_weight must be None or a sequence of numbers" % who) from None
    pointwise, main = bool(semantic_only or trainall), not semantic_only
    need = [(batch_inputs, "batch_inputs", _BATCH_KEYS)]
    if model_outputs is not None:
        if pointwise:
            need += [(batch_inputs, "batch_inputs", _PW_BATCH_KEYS), (model_outputs, "model_outputs", _PW_MODEL_KEYS)]
        if main:
            need.append((model_outputs, "model_outputs", _MAIN_MODEL_KEYS))
    for d, name, keys in need:
        for k in keys:
            if k not in d:
                raise ValueError("%s: %s lacks %r" % (who, name, k))
    semantic_labels, instance_labels = batch_inputs["semantic_labels"], batch_inputs["instance_labels"]
    if not isinstance(semantic_labels, torch.Tensor) or not isinstance(instance_labels, torch.Tensor):
        raise ValueError("%s: semantic_labels and instance_labels must be tensors" % who)
    if main and model_outputs is not None and semantic_weight is not None and len(semantic_weight) <= instance_classes:
        raise ValueError("%s: %d semantic weights; empty_weight reads the entries 1 to %d"
                         % (who, len(semantic_weight), instance_classes))
    dev = semantic_labels.device
    loss_dict = {}
    if model_outputs is None:
        loss_dict["Placeholder"] = torch.tensor(0.0, requires_grad=True, device=dev, dtype=torch.float32)
        return loss_dict
    if pointwise:
        loss_dict.update(point_wise_losses(
            model_outputs["semantic_scores"], model_outputs["corners_offset"], model_outputs["box_conf"],
            semantic_labels, instance_labels, batch_inputs["corners_offset_labels"], batch_inputs["coords_float"],
            semantic_weight=semantic_weight, ignore_label=ignore_label, voxel_scale=voxel_scale, check=check))
        if semantic_only:
            return loss_dict
    for k in loss_dict:
        if "pw" in k:
            loss_dict[k] = loss_dict[k] * 0.25
    cls_logits, mask_logits = model_outputs["cls_logits"], model_outputs["mask_logits"]
    conf_logits, box_preds = model_outputs["conf_logits"], model_outputs["box_preds"]
    gt_dict, _ = hungarian_match(cls_logits, mask_logits, conf_logits, box_preds, model_outputs["dc_inst_mask_arr"],
                                 dup_gt=dup_gt)
    offsets = model_outputs["dc_batch_offsets"]
    if isinstance(offsets, torch.Tensor) and offsets.device.type != "cpu":
        offsets = offsets.tolist()  # the one host read of a device tensor
    main_losses = matched_losses(cls_logits, mask_logits, conf_logits, box_preds, model_outputs["dc_prob_labels"],
                                 offsets, model_outputs["dc_rgb_feats"], model_outputs["dc_coords_float"], gt_dict,
                                 empty_weight=_empty_weight_of(cls_logits.device, instance_classes, float(eos_coef),
                                                               semantic_weight),
                                 voxel_scale=voxel_scale, check=check)
    for k, v in weights.items():
        loss_dict[k] = main_losses[k] * v
    loss_dict["kl_loss"] = kl_to_gp_loss(model_outputs["mu_pred"], model_outputs["logvar_pred"],
                                         model_outputs["dc_mu_labels"], model_outputs["dc_var_labels"],
                                         weight=weights["kl_loss"])
    return loss_dict


# ---- predicted instances: the inference post-processing (csrc/proposals.hip) ------------------------------------------
_NMS_TYPES = {"matrix": _lib.PROPOSALS_NMS_MATRIX, "standard": _lib.PROPOSALS_NMS_STANDARD}
_LABEL_SHIFTS = {"scannetv2": 1, "s3dis": 3}
_PROPOSAL_CAUSES = ((1, "a non-finite cls_logits, conf_logits or score entry"),
                    (2, "a non-finite mask_logits entry in the row of a candidate"),
                    (4, "a v2p_map entry outside the voxels"),
                    (8, "a voxel_spps entry outside the columns of mask_logits"),
                    (16, "a superpoint id outside [0, n_spps)"))
ProposalArrays = namedtuple("ProposalArrays", "conf label_id box query run_offsets runs masks header n_runs")


_PROPOSALS_CHAIN = ("gapro_proposals_", _lib.ProposalsHeader, _PROPOSAL_CAUSES, ProposalArrays)


def get_instance(scan_id, cls_logits, mask_logits, conf_logits, box_preds, v2p_map, semantic_scores_preds, spps,
                 logit_thresh=0.0, score_thresh=0.1, npoint_thresh=100, *, instance_classes, test_cfg=None,
                 type_nms="matrix", topk=100, nms_threshold=0.2, sem2ins_classes=(), dataset_name="scannetv2",
                 voxel_spps=None, n_spps=None, pre_topk=300, return_arrays=False, return_masks=False):
    """``ISBNet.get_instance`` (ISBNet/isbnet/model/isbnet.py:887-1005) with the ``nms``, ``custom_scatter_mean``,
    ``superpoint_align`` and ``rle_encode_gpu_batch`` it calls, as one chain of integer kernels (include/gapro_hip.h,
    "Predicted instances"): the list of ``{"scan_id", "label_id", "conf", "pred_mask": {"length": N,
    "counts": int64 array}}``, the ``sem2ins_classes`` rows first (``conf`` 1.0), then the kept proposals -- in
    descending updated score for matrix NMS, in descending score for standard NMS; equal values in the order of the
    flat index ``query * instance_classes + class``.  The reference leaves that order to ``torch.topk`` and an unstable
    ``argsort``.

    ``mask_logits`` is ``f32[Q, V]``, or ``f32[Q, S_v]`` with ``voxel_spps`` (``int[V]`` in ``[0, S_v)``): the form the
    reference holds before isbnet.py:610 expands it, and the one to pass.  ``semantic_scores_preds`` (``int[V]``) is
    read with ``sem2ins_classes`` only and may be ``None`` without.  ``score_thresh`` is accepted and unused, as in the
    reference.  ``test_cfg`` (an object with ``type_nms``, ``topk``, ``nms_threshold``) overrides the three keywords.
    ``n_spps=None`` costs a host read of ``spps.max()``.  ``return_arrays`` gives the device tensors (``ProposalArrays``;
    ``masks`` u8[K, N] with ``return_masks``) instead of the list.  Non-finite logits a candidate reads and indices out
    of range are a ``GaproError``; the reference's case of ``spps`` holding only ``ignore_label`` is not built."""
    who = "get_instance"
    if test_cfg is not None:
        type_nms = getattr(test_cfg, "type_nms", type_nms)
        topk = getattr(test_cfg, "topk", topk)
        nms_threshold = getattr(test_cfg, "nms_threshold", nms_threshold)
    if type_nms not in _NMS_TYPES:
        raise RuntimeError("Invalid nms type")
    if dataset_name not in _LABEL_SHIFTS:
        raise Exception("Invalid dataset name")
    C_ = int(instance_classes)
    if not isinstance(cls_logits, torch.Tensor) or cls_logits.dim() != 2 or int(cls_logits.shape[1]) != C_ + 1:
        raise ValueError("%s: cls_logits must be f32[Q, instance_classes + 1]" % who)
    Q = int(cls_logits.shape[0])
    if Q < 1 or C_ < 1:
        raise ValueError("%s: no queries or no classes" % who)
    if int(npoint_thresh) < 1:
        raise ValueError("%s: npoint_thresh must be at least 1" % who)
    if not 1 <= int(pre_topk) <= _lib.PROPOSALS_MAX_PRE_TOPK:
        raise ValueError("%s: pre_topk must lie in [1, %d]" % (who, _lib.PROPOSALS_MAX_PRE_TOPK))
    if int(topk) < -1:
        raise ValueError("%s: topk must be -1 or a count" % who)
    sem = [int(i) for i in sem2ins_classes]
    if len(sem) > _lib.PROPOSALS_MAX_SEM2INS:
        raise ValueError("%s: at most %d sem2ins classes" % (who, _lib.PROPOSALS_MAX_SEM2INS))
    cls_logits = _f32_arg(cls_logits, "cls_logits", who, (Q, C_ + 1))
    conf_logits = _f32_arg(conf_logits.reshape(-1) if isinstance(conf_logits, torch.Tensor) else conf_logits,
                           "conf_logits", who, (Q,))
    box_preds = _f32_arg(box_preds, "box_preds", who, (Q, 6))
    v2p, v2p_i64 = _index_arg(v2p_map, "v2p_map", who)
    N = int(v2p.shape[0])
    sp, sp_i64 = _index_arg(spps, "spps", who, N)
    if N < 1:
        raise ValueError("%s: no points" % who)
    if not isinstance(mask_logits, torch.Tensor) or mask_logits.dim() != 2 or int(mask_logits.shape[0]) != Q:
        raise ValueError("%s: mask_logits must be f32[Q, columns]" % who)
    cols = int(mask_logits.shape[1])
    mask_logits = _f32_arg(mask_logits, "mask_logits", who, (Q, cols))
    vs, vs_i64 = (None, 0) if voxel_spps is None else _index_arg(voxel_spps, "voxel_spps", who)
    V = cols if vs is None else int(vs.shape[0])
    if V < 1 or cols < 1:
        raise ValueError("%s: no voxels" % who)
    sm, sm_i64 = (None, 0)
    if sem:
        sm, sm_i64 = _index_arg(semantic_scores_preds, "semantic_scores_preds", who, V)
    n_spps = _n_spps_arg(who, n_spps, sp)
    inputs = _lib.ProposalsInputs(
        n_queries=Q, n_voxels=V, n_points=N, n_spps=n_spps, n_mask_cols=0 if vs is None else cols,
        cls_logits=cls_logits.data_ptr(), conf_logits=conf_logits.data_ptr(), box_preds=box_preds.data_ptr(),
        mask_logits=mask_logits.data_ptr(), voxel_spps=None if vs is None else vs.data_ptr(), v2p_map=v2p.data_ptr(),
        spps=sp.data_ptr(), semantic_preds=None if sm is None else sm.data_ptr(), mask_type=_lib.PROPOSALS_MASK_F32,
        voxel_spps_i64=vs_i64, v2p_i64=v2p_i64, spps_i64=sp_i64, semantic_i64=sm_i64)
    params = _lib.ProposalsParams(
        mode=_lib.PROPOSALS_FULL, instance_classes=C_, pre_topk=int(pre_topk), type_nms=_NMS_TYPES[type_nms],
        topk=int(topk), npoint_thresh=int(npoint_thresh), label_shift=_LABEL_SHIFTS[dataset_name], n_sem2ins=len(sem),
        logit_thresh=float(logit_thresh), final_score_thresh=0.1, nms_threshold=float(nms_threshold))
    for i, c in enumerate(sem):
        params.sem2ins_classes[i] = c
    out = _predict_run(who, _PROPOSALS_CHAIN, cls_logits, inputs, params,
                       (cls_logits, conf_logits, box_preds, mask_logits, vs, v2p, sp, sm), N, want_masks=return_masks)
    if return_arrays:
        return out
    rows = int(out.header.n_rows)
    if rows == 0:
        return []
    small = torch.cat([out.conf.view(torch.int32).to(torch.int64), out.label_id.to(torch.int64), out.run_offsets])
    small = small.cpu().numpy()  # the small arrays: one copy
    runs = out.runs.cpu().numpy()  # the runs: the other
    conf = small[:rows].astype(np.int32).view(np.float32)
    label, run_off = small[rows:2 * rows], small[2 * rows:]
    counts = _counts_of(run_off, runs)
    n_sem = int(out.header.n_sem2ins)
    return [{"scan_id": scan_id, "label_id": int(label[r]) if r < n_sem else label[r],
             "conf": 1.0 if r < n_sem else conf[r], "pred_mask": {"length": N, "counts": counts[r]}}
            for r in range(rows)]


def mask_nms(proposals_pred, categories, scores, boxes, test_cfg):
    """The reference's ``nms`` (ISBNet/isbnet/model/model_utils.py:163-169) for a caller that holds bool masks
    ``[n, V]``: stages 3-4 of ``get_instance`` on the masks packed by the same kernel.  Returns the reference's 4-tuple
    ``(masks, categories, scores, boxes)`` of the kept proposals in the order ``get_instance`` defines (matrix: descending
    updated score; standard: descending score; equal values by row).  ``test_cfg`` has ``type_nms``, ``topk`` and
    ``nms_threshold``.  At most 1024 proposals."""
    who = "mask_nms"
    type_nms = getattr(test_cfg, "type_nms", "matrix")
    if type_nms not in _NMS_TYPES:
        raise RuntimeError("Invalid nms type")
    if not isinstance(proposals_pred, torch.Tensor) or proposals_pred.dim() != 2:
        raise ValueError("%s: proposals_pred must be a [n, V] mask tensor" % who)
    n, V = int(proposals_pred.shape[0]), int(proposals_pred.shape[1])
    if n == 0:
        return proposals_pred, categories, scores, boxes
    if n > _lib.PROPOSALS_MAX_PRE_TOPK or V < 1:
        raise ValueError("%s: %d proposals over %d voxels are beyond the library's bounds" % (who, n, V))
    _need_device(proposals_pred)
    masks = (proposals_pred if proposals_pred.dtype in (torch.bool, torch.uint8) else proposals_pred != 0).contiguous()
    sc = _f32_arg(scores, "scores", who, (n,))
    cat = categories.to(torch.int32).contiguous()
    if tuple(cat.shape) != (n,):
        raise ValueError("%s: categories must have one entry a proposal" % who)
    inputs = _lib.ProposalsInputs(n_queries=n, n_voxels=V, n_points=0, mask_logits=masks.data_ptr(),
                                  cand_scores=sc.data_ptr(), cand_classes=cat.data_ptr(),
                                  mask_type=_lib.PROPOSALS_MASK_U8)
    params = _lib.ProposalsParams(mode=_lib.PROPOSALS_NMS, type_nms=_NMS_TYPES[type_nms],
                                  topk=int(getattr(test_cfg, "topk", -1)), npoint_thresh=1, final_score_thresh=0.1,
                                  nms_threshold=float(getattr(test_cfg, "nms_threshold", 0.2)))
    out = _predict_run(who, _PROPOSALS_CHAIN, sc, inputs, params, (masks, sc, cat), 0, has_runs=False)
    idx = out.query.to(torch.int64)
    return proposals_pred[idx], categories[idx], out.conf, boxes[idx]


def rle_encode_gpu_batch(masks):
    """``rle_encode_gpu_batch`` (ISBNet/isbnet/util/rle.py:47-69) without its loop: the list of ``{"length": N,
    "counts": int64 array}`` of a device bool ``[K, N]``, from one read of the counts and one copy of the runs (a read
    and a copy per 1032 rows beyond that many)."""
    who = "rle_encode_gpu_batch"
    if not isinstance(masks, torch.Tensor) or masks.dim() != 2 or masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s: masks must be a bool [K, N] tensor" % who)
    _need_device(masks)
    K, N = int(masks.shape[0]), int(masks.shape[1])
    if N < 1:
        raise ValueError("%s: no points" % who)
    step, rles = _lib.PROPOSALS_MAX_PRE_TOPK + _lib.PROPOSALS_MAX_SEM2INS, []
    for k0 in range(0, K, step):
        part = masks[k0:k0 + step].contiguous()
        inputs = _lib.ProposalsInputs(n_queries=int(part.shape[0]), n_voxels=0, n_points=N, mask_logits=part.data_ptr(),
                                      mask_type=_lib.PROPOSALS_MASK_U8)
        params = _lib.ProposalsParams(mode=_lib.PROPOSALS_RLE)
        out = _predict_run(who, _PROPOSALS_CHAIN, part, inputs, params, (part,), N, want_rows=False)
        offs = np.concatenate([[0], np.cumsum(out.n_runs, dtype=np.int64)])  # the counts came with the header
        runs = out.runs.cpu().numpy()
        rles += [{"length": N, "counts": c} for c in _counts_of(offs, runs)]
    return rles


# ---- query sampling: the Point Aggregator's index work (csrc/query_sample.hip) -------------------------
_QS_CAUSES = ((1, "offsets that decrease or leave [0, the number of points] / [0, the number of outputs]"),
              (2, "a sample with outputs and no points (its outputs are -1)"),
              (4, "a coordinate that is not finite"))
_uniform = {}  # (device, entries, step) -> int32 step, 2 step, .., entries * step on the device


def fps_plan(n_max):
    """``gapro_fps_plan`` without a device: ``(path, xyz_capacity, capacity)`` for a sample of ``n_max`` points -- the
    path is "resident" (coordinates and running minima in registers, up to ``xyz_capacity`` points), "streamed" (the
    minima in registers, up to ``capacity``) or "global" (the minima in device memory).  The results are the same."""
    if not _is_int(n_max) or n_max < 0:
        raise ValueError("fps_plan: n_max must be a non-negative int")
    xyz_cap, cap = C.c_int64(0), C.c_int64(0)
    path = _lib.load().gapro_fps_plan(int(n_max), C.byref(xyz_cap), C.byref(cap))
    if path < 0:
        raise ValueError("fps_plan: %d points are beyond the library's bounds" % n_max)
    return _lib.FPS_PATHS[path], int(xyz_cap.value), int(cap.value)


def _uniform_offsets(dev, entries, step):
    """``step * (i + 1)`` for ``i < entries`` as an int32 device tensor: made once per device and shape, no host read."""
    key = (dev, entries, step)
    if key not in _uniform:
        if entries * step > 2 ** 31 - 1:
            raise ValueError("%d samples of %d entries are beyond the library's bounds" % (entries, step))
        _uniform[key] = torch.arange(step, step * entries + 1, step, dtype=torch.int32, device=dev) if step > 0 \
            else torch.zeros(entries, dtype=torch.int32, device=dev)
    return _uniform[key]


def _samples_arg(who, offset, new_offset, n_sample, m_known=None):
    """The two offset tables of a batch-flat call as the kernels read them, and the number of outputs: ``new_offset``
    as given (its last entry is the number of outputs: the call's host read unless ``m_known``) or ``n_sample * (i +
    1)``, which needs no read."""
    _index_check(who, "offset", offset)
    n_samples = int(offset.shape[0])
    if not 1 <= n_samples <= _lib.QS_MAX_SAMPLES:
        raise ValueError("%s: %d offsets outside [1, %d]" % (who, n_samples, _lib.QS_MAX_SAMPLES))
    if (new_offset is None) == (n_sample is None):
        raise ValueError("%s: one of new_offset and n_sample= is expected" % who)
    if n_sample is not None:
        if not _is_int(n_sample) or n_sample < 0:
            raise ValueError("%s: n_sample must be a non-negative int" % who)
        _need_device(offset)
        return offset, _uniform_offsets(offset.device, n_samples, n_sample), n_samples * n_sample
    _index_check(who, "new_offset", new_offset)
    if int(new_offset.shape[0]) != n_samples:
        raise ValueError("%s: %d offsets, %d new offsets" % (who, n_samples, int(new_offset.shape[0])))
    _need_device(offset, new_offset)
    m = m_known if m_known is not None else max(int(new_offset[-1]), 0)  # the host read, as the reference's
    return offset, new_offset, m


def _qs_status(who, dev, h_status):
    if h_status is not None:  # the call's host read of its status, asked for by check=True
        status, flags = _host_read(dev, h_status)[:2]
        _refuse(who, status, flags, _QS_CAUSES)


def _fps_run(who, xyz, offset, new_offset, m, flags, check, return_dist):
    ctx, stream = _ctx_stream(xyz)
    lib, dev = ctx.lib, xyz.device
    xyz = xyz.detach().contiguous()
    n = int(xyz.shape[0])
    off, off_i64 = _as_index(offset)
    new_off, new_i64 = _as_index(new_offset)
    _one_device(who, dev, (off, new_off))
    with torch.cuda.device(dev):
        ws = _workspace(who, int(lib.gapro_fps_workspace_bytes(n)), dev, "%d points are" % n)
        idx = torch.empty(m, dtype=torch.int32, device=dev)
        dist = torch.empty(n, dtype=torch.float32, device=dev) if return_dist else None
        d_status, h_status = _status_pair(dev, _lib.QS_STATUS_WORDS, torch.int32, read=check)
        ctx.check(lib.gapro_fps_batch(ctx.handle, stream, n, _ptr(xyz), int(off.shape[0]), off.data_ptr(), off_i64,
                                      new_off.data_ptr(), new_i64, m, flags, ws.data_ptr(), ws.numel(), _ptr(idx),
                                      _ptr(dist), d_status.data_ptr(), _ptr(h_status)))
        _qs_status(who, dev, h_status)
    return idx, dist


def _ball_run(who, radius, nsample, xyz, new_xyz, offset, new_offset, flags, check, return_counts):
    ctx, stream = _ctx_stream(xyz)
    lib, dev = ctx.lib, xyz.device
    xyz, new_xyz = xyz.detach().contiguous(), new_xyz.detach().contiguous()
    n, m = int(xyz.shape[0]), int(new_xyz.shape[0])
    off, off_i64 = _as_index(offset)
    new_off, new_i64 = _as_index(new_offset)
    _one_device(who, dev, (new_xyz, off, new_off))
    if n > 2 ** 31 - 1 or m * nsample > 2 ** 31 - 1:
        raise ValueError("%s: %d points and %d x %d indices are beyond the library's bounds" % (who, n, m, nsample))
    with torch.cuda.device(dev):
        idx = torch.empty((m, nsample), dtype=torch.int32, device=dev)
        counts = torch.empty(m, dtype=torch.int32, device=dev) if return_counts else None
        d_status, h_status = _status_pair(dev, _lib.QS_STATUS_WORDS, torch.int32, read=check)
        ctx.check(lib.gapro_ball_query_batch(ctx.handle, stream, n, _ptr(xyz), m, _ptr(new_xyz), int(off.shape[0]),
                                             off.data_ptr(), off_i64, new_off.data_ptr(), new_i64, float(radius),
                                             nsample, flags, _ptr(idx), _ptr(counts), d_status.data_ptr(),
                                             _ptr(h_status)))
        _qs_status(who, dev, h_status)
    return idx, counts


def _ball_args(who, radius, nsample):
    _finite_arg(who, "radius", radius)
    _positive_int_arg(who, "nsample", nsample)
    if nsample > _lib.BALL_QUERY_MAX_NSAMPLE:
        raise ValueError("%s: nsample beyond %d" % (who, _lib.BALL_QUERY_MAX_NSAMPLE))


def furthestsampling_batchflat(xyz, offset, new_offset=None, *, n_sample=None, check=True, return_dist=False):
    """``isbnet.ops.furthestsampling_batchflat`` (called at ISBNet/isbnet/model/aggregator.py:69): ``int32[m]`` indices
    into ``xyz`` (``f32[n, 3]``), the furthest point sampling of every sample in one launch.  Sample ``i`` owns the points
    ``offset[i - 1] .. offset[i]`` and the outputs ``new_offset[i - 1] .. new_offset[i]`` (``offset[-1] = 0``; the
    reference's tables with a leading 0 have an empty first sample and are read by the same rule).

    The definition: a sample's first output is its first point; each later one the point with the
    largest running minimum of the float32 squared distances ``((dx*dx + dy*dy) + dz*dz)``, every operation rounded on
    its own, to the outputs before it; AMONG EQUAL MAXIMA THE LOWEST INDEX wins (the reference leaves that to its block
    size).  More outputs than points repeat indices.

    ``new_offset`` costs one host read of its last entry, as in the reference; ``n_sample=`` stands for the table
    ``n_sample * (i + 1)`` over the entries of ``offset`` (so ``offset`` WITHOUT a leading 0) and reads nothing.  With
    ``check=True`` the status is read behind the kernel: offsets that decrease or leave their range, a sample with
    outputs and no points (its outputs are -1) and a non-finite coordinate are a ``GaproError``; with ``check=False``
    the call only enqueues, and in all three cases every index written is inside its sample's range or -1.
    ``return_dist`` adds ``f32[n]``: every point's running minimum as the last iteration left it (over all outputs of
    its sample but the last).  No autograd: these are indices."""
    who = "furthestsampling_batchflat"
    _tensor_arg(who, "xyz", xyz, ("n", 3))
    off, new_off, m = _samples_arg(who, offset, new_offset, n_sample)
    _need_device(xyz)
    idx, dist = _fps_run(who, xyz, off, new_off, m, 0, check, return_dist)
    return (idx, dist) if return_dist else idx


def ballquery_batchflat(radius, nsample, xyz, new_xyz, offset, new_offset=None, *, n_sample=None, check=True,
                        return_counts=False):
    """``isbnet.ops.ballquery_batchflat`` (aggregator.py:75-77): ``int32[m, nsample]`` indices into ``xyz``, per query
    of ``new_xyz`` (``f32[m, 3]``; ``None`` means ``xyz``, with ``offset`` for its samples) the first ``nsample`` points
    of the query's own sample, in ascending index, with ``d2 < r2`` -- the float32 distance of
    ``furthestsampling_batchflat``, ``r2 = float32(radius) * float32(radius)``, strictly: a point at exactly the radius
    is no hit.  The remaining slots repeat the first hit.  A QUERY WITHOUT A HIT HAS A ROW OF ZEROS, index 0 of the
    whole table, as the reference's zero-initialised output.  A point of a neighbouring sample is never returned.
    The query's sample comes from ``new_offset`` (or ``n_sample=``) by the rule of ``furthestsampling_batchflat``;
    neither costs a host read here.  ``return_counts`` adds ``int32[m]``, the hits of each query, at most ``nsample``.
    ``check=True`` reads the status (offsets that decrease or leave their range; a query beyond the last offset)."""
    who = "ballquery_batchflat"
    _ball_args(who, radius, nsample)
    _tensor_arg(who, "xyz", xyz, ("n", 3))
    if new_xyz is None:
        new_xyz = xyz
        if new_offset is None and n_sample is None:
            new_offset = offset
    _tensor_arg(who, "new_xyz", new_xyz, ("m", 3))
    off, new_off, m = _samples_arg(who, offset, new_offset, n_sample, m_known=int(new_xyz.shape[0]))
    _need_device(xyz, new_xyz)
    if n_sample is not None and m != int(new_xyz.shape[0]):
        raise ValueError("%s: %d queries, %d samples of n_sample=%d" % (who, int(new_xyz.shape[0]),
                                                                       int(off.shape[0]), n_sample))
    idx, counts = _ball_run(who, radius, nsample, xyz, new_xyz, off, new_off, 0, check, return_counts)
    return (idx, counts) if return_counts else idx


def _batched_arg(who, name, t):
    _tensor_arg(who, name, t, ("B", "N", 3))
    B, N = int(t.shape[0]), int(t.shape[1])
    if not 1 <= B <= _lib.QS_MAX_SAMPLES:
        raise ValueError("%s: batch size %d outside [1, %d]" % (who, B, _lib.QS_MAX_SAMPLES))
    return B, N


def furthest_point_sample(xyz, npoint, *, check=False):
    """pointnet2's ``furthest_point_sample`` (aggregator.py:170): ``int32[B, npoint]`` indices into each sample of
    ``xyz`` (``f32[B, N, 3]``), by the kernel and the definition of ``furthestsampling_batchflat`` with pointnet2's
    near-origin skip: a point with ``x*x + y*y + z*z <= 1e-3f`` is never a candidate (it can still be the first output,
    which is point 0); without a candidate point 0 is the answer.  No host read unless ``check``."""
    who = "furthest_point_sample"
    B, N = _batched_arg(who, "xyz", xyz)
    if not _is_int(npoint) or npoint < 0:
        raise ValueError("%s: npoint must be a non-negative int" % who)
    if N == 0 and npoint > 0:
        raise ValueError("%s: no points" % who)
    _need_device(xyz)
    dev = xyz.device
    idx, _ = _fps_run(who, xyz.reshape(B * N, 3), _uniform_offsets(dev, B, N), _uniform_offsets(dev, B, npoint),
                      B * npoint, _lib.FPS_SKIP_ORIGIN | _lib.QS_LOCAL_INDEX, check, False)
    return idx.view(B, npoint)


def ball_query(radius, nsample, xyz, new_xyz, *, return_counts=False):
    """pointnet2's ``ball_query`` (aggregator.py:115, 176): ``int32[B, M, nsample]`` indices into each sample of ``xyz``
    (``f32[B, N, 3]``) per query of ``new_xyz`` (``f32[B, M, 3]``), by the kernel and the definition of
    ``ballquery_batchflat``; a query without a hit has a row of zeros.  No host read."""
    who = "ball_query"
    _ball_args(who, radius, nsample)
    B, N = _batched_arg(who, "xyz", xyz)
    _tensor_arg(who, "new_xyz", new_xyz, (B, "M", 3))
    M = int(new_xyz.shape[1])
    _need_device(xyz, new_xyz)
    dev = xyz.device
    idx, counts = _ball_run(who, radius, nsample, xyz.reshape(B * N, 3), new_xyz.reshape(B * M, 3),
                            _uniform_offsets(dev, B, N), _uniform_offsets(dev, B, M), _lib.QS_LOCAL_INDEX, False,
                            return_counts)
    idx = idx.view(B, M, nsample)
    return (idx, counts.view(B, M)) if return_counts else idx


def sample_queries(locs, batch_offsets, batch_size, n_sample, radius, n_neighbor, n_neighbor_post, *, check=False):
    """The index work of ``LocalAggregator.forward_batchflat`` (aggregator.py:63-115) in one call with no host read:
    ``(fps_inds int32[B * n_sample], neighbor_inds int32[B * n_sample, n_neighbor], neighbor_inds_post int32[B,
    n_sample, n_neighbor_post])`` -- the furthest point sampling of ``n_sample`` points per sample, the batch-flat ball
    query of radius ``radius`` around them, and the batched ball query of radius ``2 * radius`` among them (indices
    into the sample's ``n_sample`` queries).  ``locs`` is ``f32[n, 3]``; ``batch_offsets`` the reference's ``B + 1``
    entries with the leading 0 (an int32 / int64 tensor or a sequence).  The gathers and the MLPs stay torch.
    ``check=True`` reads the status of the first two calls (two host reads)."""
    who = "sample_queries"
    _tensor_arg(who, "locs", locs, ("n", 3))
    _positive_int_arg(who, "batch_size", batch_size)
    _positive_int_arg(who, "n_sample", n_sample)
    _ball_args(who, radius, n_neighbor)
    _ball_args(who, radius, n_neighbor_post)
    off = _offsets_arg(batch_offsets, batch_size, who)
    _need_device(locs)
    off = off.to(locs.device)[1:]
    fps_inds = furthestsampling_batchflat(locs, off, n_sample=n_sample, check=check)
    fps_locs = locs.detach().index_select(0, fps_inds.clamp(min=0).to(torch.int64))  # -1: a sample without points
    neighbor_inds = ballquery_batchflat(radius, n_neighbor, locs, fps_locs, off, n_sample=n_sample, check=check)
    fps_locs = fps_locs.view(batch_size, n_sample, 3)
    return fps_inds, neighbor_inds, ball_query(2 * radius, n_neighbor_post, fps_locs, fps_locs)


# ---- voxelisation: the first tensors of a consumer's step (csrc/voxelize.hip, csrc/voxelize_host.cc) ---
_VOX_CAUSES = ((1, "a negative batch index"),
               (2, "mode 0 and a voxel that holds two points"),
               (4, "a table that is not the count's"))
_POOL_CAUSES = ((1, "a count outside [0, max_active]"),
                (2, "a point index outside [0, n_points)"),
                (4, "a point listed twice"))


def voxelize_plan(n_points):
    """``gapro_voxelize_plan`` without a device: the slots of the device path's table for ``n_points`` points (a power
    of two); the slot a row starts its probes at is ``voxelize_hash(row) & (slots - 1)``."""
    if not _is_int(n_points) or not 1 <= n_points <= 2 ** 31 - 1:
        raise ValueError("voxelize_plan: n_points must be an int in [1, 2^31 - 1]")
    return int(_lib.load().gapro_voxelize_plan(n_points))


def voxelize_hash(coords):
    """``gapro_voxelize_hash`` of every row of an int64 ``[n, 3]`` / ``[n, 4]`` array: ``uint64[n]`` (a host loop: for
    tests and tools)."""
    rows = np.ascontiguousarray(coords, dtype=np.int64)
    if rows.ndim != 2 or rows.shape[1] not in (3, 4):
        raise ValueError("voxelize_hash: coords must be an int64 array of shape [n, 3] or [n, 4]")
    fn, cols, base = _lib.load().gapro_voxelize_hash, rows.shape[1], rows.ctypes.data
    return np.array([fn(base + 8 * cols * i, cols) for i in range(rows.shape[0])], dtype=np.uint64)


def voxel_table_shape(mode, n_voxels, max_active):
    """The header arithmetic of ``voxelization_idx`` (``gapro_voxelize_table_shape``; nothing is allocated): the width
    of ``output_map`` for a header that reports ``n_voxels`` and ``max_active``, ``max_active + 1`` in modes 3 and 4 and 2
    otherwise.  A ``ValueError`` for what the call refuses from its header: ``max_active`` beyond
    ``GAPRO_VOXELIZE_MAX_ACTIVE`` (modes 3, 4), ``n_voxels * width`` beyond 2^31 - 1, two points in a voxel in mode 0."""
    who = "voxelization_idx"
    if not _is_int(mode) or not 0 <= mode <= 4:
        raise ValueError("%s: mode must be an int in 0..4" % who)
    width = C.c_int64(0)
    if _lib.load().gapro_voxelize_table_shape(mode, int(n_voxels), int(max_active), C.byref(width)) != _lib.GAPRO_OK:
        raise ValueError("%s: %d voxels of at most %d points in mode %d: beyond the library's bounds (%d points a voxel, "
                         "2^31 - 1 table entries, one point a voxel in mode 0)"
                         % (who, n_voxels, max_active, mode, _lib.VOXELIZE_MAX_ACTIVE))
    return int(width.value)


def _vox_header(who, hdr, mode):
    _refuse(who, hdr.status, hdr.flags, _VOX_CAUSES)
    return int(hdr.n_voxels), voxel_table_shape(mode, hdr.n_voxels, hdr.max_active)


def voxelization_idx(coords, batchsize, mode=4):
    """``isbnet.ops.voxelization_idx`` / ``pointgroup_ops.voxelization_idx`` (ISBNet/isbnet/data/custom.py:296,
    SPFormer/spformer/dataset/scannetv2.py:363): ``(output_coords int64[M, cols], input_map int32[N], output_map
    int32[M, width])`` of ``coords``, int64 ``[N, 3]`` or ``[N, 4]`` with the batch index in column 0.

    The definition: a voxel is a distinct row over all columns and all 64 bits; VOXELS ARE NUMBERED BY
    THE INDEX OF THEIR FIRST POINT, ascending (the reference's hash map in insertion order, not ``torch.unique``'s
    sorted order); ``input_map`` is the voxel of each point, ``output_coords`` the row of each voxel's first point.
    Modes 3 and 4: ``width = max_active + 1`` and a row of ``output_map`` is ``[count, its points ascending, zeros]``;
    mode 1: ``[1, first point]``; mode 2: ``[1, last point]`` (the code of the reference, not its comment); mode 0: as
    mode 1, and two points in a voxel are refused.  ``batchsize`` only sizes a vector in the reference: a positive int,
    otherwise ignored.  ``N = 0`` returns empty tensors of shapes ``(0, cols)``, ``(0,)`` and ``(0, 2)``.

    CPU tensors take the host path (``gapro_voxelize_host_*``: an ordinary hash map, no device in the process -- what a
    DataLoader worker calls) and return CPU tensors; device tensors take the device path (count, ONE host read of the
    header, fill) and return device tensors.  Both give the same bits.  A ``GaproError``: a negative batch index, mode 0
    on a duplicate.  A ``ValueError``: a bad argument, and what the header refuses (``voxel_table_shape``)."""
    who = "voxelization_idx"
    if not isinstance(coords, torch.Tensor) or coords.dtype != torch.int64 or coords.dim() != 2 or \
            coords.shape[1] not in (3, 4):
        raise ValueError("%s: coords must be an int64 tensor of shape [N, 3] or [N, 4]" % who)
    _positive_int_arg(who, "batchsize", batchsize)
    if not _is_int(mode) or not 0 <= mode <= 4:
        raise ValueError("%s: mode must be an int in 0..4" % who)
    n, cols = int(coords.shape[0]), int(coords.shape[1])
    if n > 2 ** 31 - 1:
        raise ValueError("%s: %d points are beyond the library's bounds" % (who, n))
    dev = coords.device
    if n == 0:
        return (torch.empty((0, cols), dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty((0, 2), dtype=torch.int32, device=dev))
    coords = coords.detach().contiguous()
    if not coords.is_cuda:
        lib = _lib.load()
        input_map = torch.empty(n, dtype=torch.int32)
        hdr, handle = _lib.VoxelizeHeader(), C.c_void_p()
        rc = lib.gapro_voxelize_host_count(coords.data_ptr(), n, cols, mode, input_map.data_ptr(), C.byref(hdr),
                                           C.byref(handle))
        try:
            if rc != _lib.GAPRO_OK:
                raise GaproError(rc, who)
            M, width = _vox_header(who, hdr, mode)
            out_coords = torch.empty((M, cols), dtype=torch.int64)
            out_map = torch.empty((M, width), dtype=torch.int32)
            rc = lib.gapro_voxelize_host_fill(handle, coords.data_ptr(), input_map.data_ptr(), out_coords.data_ptr(),
                                              out_map.data_ptr())
            if rc != _lib.GAPRO_OK:
                raise GaproError(rc, who)
        finally:
            lib.gapro_voxelize_host_free(handle)
        return out_coords, input_map, out_map
    ctx, stream = _ctx_stream(coords)
    lib = ctx.lib
    with torch.cuda.device(dev):
        ws = _workspace(who, int(lib.gapro_voxelize_workspace_bytes(n)), dev, "%d points are" % n)
        input_map = torch.empty(n, dtype=torch.int32, device=dev)
        d_hdr, h_hdr = _status_pair(dev, C.sizeof(_lib.VoxelizeHeader))
        ctx.check(lib.gapro_voxelize_count(ctx.handle, stream, n, cols, coords.data_ptr(), mode, ws.data_ptr(),
                                           ws.numel(), input_map.data_ptr(), d_hdr.data_ptr(), h_hdr.data_ptr()))
        hdr, _ = _host_read(dev, h_hdr, _lib.VoxelizeHeader)  # the call's one host read
        M, width = _vox_header(who, hdr, mode)
        out_coords = torch.empty((M, cols), dtype=torch.int64, device=dev)
        out_map = torch.empty((M, width), dtype=torch.int32, device=dev)
        d_status, _ = _status_pair(dev, _lib.VOXELIZE_STATUS_WORDS, torch.int32, read=False)
        ctx.check(lib.gapro_voxelize_fill(ctx.handle, stream, n, cols, coords.data_ptr(), mode, M, hdr.max_active,
                                          ws.data_ptr(), ws.numel(), input_map.data_ptr(), out_coords.data_ptr(),
                                          out_map.data_ptr(), d_status.data_ptr(), None))
    return out_coords, input_map, out_map


class Voxelization(torch.autograd.Function):
    """``isbnet.ops.functions.Voxelization``: see ``voxelization``, which checks the arguments first."""

    @staticmethod
    def forward(fctx, feats, map_rule, mode=4, check=True):
        who = "voxelization"
        N, Cn = int(feats.shape[0]), int(feats.shape[1])
        M, A = int(map_rule.shape[0]), int(map_rule.shape[1]) - 1
        dev = feats.device
        feats, map_rule = feats.detach().contiguous(), map_rule.contiguous()
        fctx.plan = (map_rule, mode, N, Cn, M, A)
        out = torch.empty((M, Cn), dtype=torch.float32, device=dev)
        if M == 0:
            return out
        if N == 0:  # every listed index is out of range; the rows pool to zeros as flagged rows do
            return out.zero_()
        ctx, stream = _ctx_stream(feats)
        lib = ctx.lib
        with torch.cuda.device(dev):
            ws = _workspace(who, int(lib.gapro_voxel_pool_workspace_bytes(N)), dev) if check else None
            d_status, h_status = _status_pair(dev, _lib.VOXELIZE_STATUS_WORDS, torch.int32, read=check)
            ctx.check(lib.gapro_voxel_pool_forward(ctx.handle, stream, N, Cn, feats.data_ptr(), M, A,
                                                   map_rule.data_ptr(), mode, int(check), _ptr(ws),
                                                   ws.numel() if check else 0, out.data_ptr(), d_status.data_ptr(),
                                                   _ptr(h_status)))
            if h_status is not None:  # the call's host read of its status, asked for by check=True
                status, flags = _host_read(dev, h_status)[:2]
                _refuse(who, status, flags, _POOL_CAUSES)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out):
        map_rule, mode, N, Cn, M, A = fctx.plan
        dev = grad_out.device
        if M == 0 or N == 0:
            return torch.zeros((N, Cn), dtype=torch.float32, device=dev), None, None, None
        grad_out = grad_out.contiguous()
        ctx, stream = _ctx_stream(grad_out)
        with torch.cuda.device(dev):
            d_feats = torch.empty((N, Cn), dtype=torch.float32, device=dev)
            d_status, _ = _status_pair(dev, _lib.VOXELIZE_STATUS_WORDS, torch.int32, read=False)
            ctx.check(ctx.lib.gapro_voxel_pool_backward(ctx.handle, stream, N, Cn, grad_out.data_ptr(), M, A,
                                                        map_rule.data_ptr(), mode, d_feats.data_ptr(),
                                                        d_status.data_ptr(), None))
        return d_feats, None, None, None


def voxelization(feats, map_rule, mode=4, *, check=True, n_points=None):
    """``isbnet.ops.voxelization`` / ``pointgroup_ops.voxelization`` (ISBNet/isbnet/model/isbnet.py:265, 478, 672;
    SPFormer/spformer/model/spformer.py:115-120): ``f32[M, C]``, the rows of ``feats`` (``f32[N, C]``) pooled into voxel
    rows through ``map_rule`` (``int32[M, A + 1]``, the ``output_map`` of ``voxelization_idx`` or any table of that
    shape), both on the device; a ``torch.autograd.Function`` (``Voxelization``).

    Forward, for row ``v`` with ``n = map_rule[v, 0]``: ``mult = 1.0f / n`` when ``mode == 4`` and ``n > 0``, else 1;
    ``out[v, c] = ((0 + fl(mult * x_1)) + fl(mult * x_2)) + ...`` IN THE ROW'S ORDER, in float32, product and sum each
    rounded on their own -- the order of the reference's atomic adds into a zeroed buffer.  Not "sum, then divide", not
    a fused multiply-add; a single ``-0.0`` input gives ``+0.0``.  A row with ``n = 0`` is zeros.  Every mode runs this
    kernel; modes other than 4 sum the rows as given.
    Backward: ``d_feats[p, c] = fl(mult * d_out[v, c])`` for every point ``p`` listed in row ``v``, 0 for every unlisted
    point: the array is cleared and the rows stored, with no floating-point atomics.  THE CONTRACT: this equals the
    reference for every table in which a point is listed at most once, which holds for every table
    ``voxelization_idx`` produces; a point listed twice receives one of its rows' gradients, not their sum.

    ``check=True`` reads a status word behind the forward kernel (the call's one host read): a count outside ``[0,
    A]``, a point index outside ``[0, N)`` and a point listed twice are a ``GaproError``.  With ``check=False`` the call
    only enqueues; a flagged row pools to zeros, a flagged entry is skipped, nothing is touched out of range.  The
    backward never reads.  ``n_points=`` states the number of points the table was built for: a ``ValueError`` when
    ``feats`` has another number of rows.  Only float32 is built."""
    who = "voxelization"
    _tensor_arg(who, "feats", feats, ("N", "C"))
    if not isinstance(map_rule, torch.Tensor) or map_rule.dtype != torch.int32 or map_rule.dim() != 2:
        raise ValueError("%s: map_rule must be an int32 tensor of shape [M, A + 1]" % who)
    if int(feats.shape[1]) < 1 or int(map_rule.shape[1]) < 2:
        raise ValueError("%s: feats needs a channel and map_rule a count and an index column" % who)
    if not _is_int(mode) or not 0 <= mode <= 4:
        raise ValueError("%s: mode must be an int in 0..4" % who)
    if not isinstance(check, bool):
        raise ValueError("%s: check must be a bool" % who)
    if n_points is not None and (not _is_int(n_points) or n_points != int(feats.shape[0])):
        raise ValueError("%s: feats has %d rows, n_points=%r" % (who, int(feats.shape[0]), n_points))
    if int(map_rule.shape[0]) * int(map_rule.shape[1]) > 2 ** 31 - 1 or int(feats.shape[0]) > 2 ** 31 - 1:
        raise ValueError("%s: a table or a point count beyond the library's bounds" % who)
    _need_device(feats, map_rule)
    _one_device(who, feats.device, (map_rule,))
    return Voxelization.apply(feats, map_rule, mode, check)


# ---- superpoint pooling: torch_scatter's scatter_mean / scatter_max with grad (csrc/spp_pool.hip) ------
_SPP_CAUSES = ((_lib.SPP_FLAG_INDEX, "a superpoint index outside [0, n_spps)"),
               (_lib.SPP_FLAG_MAP, "a point_map value outside [0, n_rows)"))
_SPP_REDUCE = {"mean": _lib.SPP_MEAN, "max": _lib.SPP_MAX}


class SuperpointPlan:
    """What ``superpoint_plan`` built: ``n_points``, ``n_spps``, ``n_rows`` (0 without a point map), ``counts``
    int32 ``[S]``, the CSR by superpoint ``seg_off`` int32 ``[S + 1]`` / ``seg_pts`` int32 ``[N]``, with a point map
    the CSR by source row ``row_off`` / ``row_pts`` and ``seg_rows``, and ``spp_batch_offsets`` int64 ``[B + 1]`` (or
    ``None``).  It keeps the index tensors it was built from: they must not be written while it is in use."""
    __slots__ = ("n_points", "n_spps", "n_rows", "index", "point_map", "counts", "seg_off", "seg_pts", "row_off",
                 "row_pts", "seg_rows", "spp_batch_offsets", "device", "_struct")

    def struct(self):
        return C.byref(self._struct)


def _empty_plan(dev, S, R, B):
    plan = SuperpointPlan()
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    plan.n_points, plan.n_spps, plan.n_rows, plan.device = 0, S, R, dev
    plan.index = plan.point_map = plan._struct = None
    plan.counts, plan.seg_off, plan.seg_pts = z(S), z(S + 1), z(0)
    plan.row_off, plan.row_pts, plan.seg_rows = (z(R + 1), z(0), z(0)) if R else (None, None, None)
    plan.spp_batch_offsets = z(B + 1, torch.int64) if B else None
    return plan


def superpoint_plan(superpoints, *, n_spps=None, point_map=None, n_rows=None, batch_offsets=None, check=True):
    """The plan of a step's superpoint pooling (``gapro_spp_plan_build``), built once and shared by
    every tensor that ``superpoint_pool`` pools: a ``SuperpointPlan``.

    ``superpoints`` is a 1-D integer device tensor ``[N]`` with values in ``[0, n_spps)``; ``n_spps=None`` reads
    ``max(superpoints) + 1`` from the device (one host read).  ``point_map`` (1-D integer ``[N]``, values in ``[0,
    n_rows)``, ``n_rows`` needed) makes point ``p`` read row ``point_map[p]`` of the pooled tensor -- the fused form of
    ``x[v2p_map]`` followed by the scatter.  ``batch_offsets`` (1-D integer ``[B + 1]``, the point offsets of the
    samples) adds ``spp_batch_offsets``: per sample the number of non-empty superpoints whose first point lies in it,
    which is ISBNet's loop of ``torch.unique`` (isbnet.py:736-742) when no id is shared between samples, without a host
    read.  ``check=True`` reads the status word (the call's host read): an index outside ``[0, n_spps)`` or a map value
    outside ``[0, n_rows)`` is a ``GaproError``; with ``check=False`` the call only enqueues and such a point is left
    out of every superpoint.  Bounds: ``n_spps`` and ``n_rows`` up to 2^24, ``N`` up to 2^31 - 1."""
    who = "superpoint_plan"
    _index_check(who, "superpoints", superpoints)
    N = int(superpoints.shape[0])
    if point_map is not None:
        _index_check(who, "point_map", point_map)
        if int(point_map.shape[0]) != N:
            raise ValueError("%s: point_map has %d entries, expected %d" % (who, int(point_map.shape[0]), N))
        _positive_int_arg(who, "n_rows", n_rows)
    elif n_rows is not None:
        raise ValueError("%s: n_rows is the row count of point_map's target and needs point_map" % who)
    if batch_offsets is not None:
        _index_check(who, "batch_offsets", batch_offsets)
        if int(batch_offsets.shape[0]) < 2:
            raise ValueError("%s: batch_offsets needs at least two entries" % who)
    if not isinstance(check, bool):
        raise ValueError("%s: check must be a bool" % who)
    if n_spps is None and N == 0:
        raise ValueError("%s: n_spps is needed for an empty superpoints tensor" % who)
    B = int(batch_offsets.shape[0]) - 1 if batch_offsets is not None else 0
    R = int(n_rows) if point_map is not None else 0
    if n_spps is not None:
        _positive_int_arg(who, "n_spps", n_spps)
    if N > 2 ** 31 - 1 or R > _lib.SPP_MAX_SEGMENTS or B > _lib.SPP_MAX_BATCHES or \
            (n_spps is not None and n_spps > _lib.SPP_MAX_SEGMENTS):
        raise ValueError("%s: %d points, %r superpoints, %d rows, %d samples: beyond the library's bounds (2^31 - 1 "
                         "points, 2^24 superpoints and rows, 65536 samples)" % (who, N, n_spps, R, B))
    _need_device(superpoints, point_map, batch_offsets)
    dev = superpoints.device
    _one_device(who, dev, [t for t in (point_map, batch_offsets) if t is not None])
    S = _n_spps_arg(who, n_spps, superpoints)
    if S > _lib.SPP_MAX_SEGMENTS:
        raise ValueError("%s: %d superpoints are beyond the library's bounds (2^24)" % (who, S))
    if N == 0:
        return _empty_plan(dev, S, R, B)
    ctx, stream = _ctx_stream(superpoints)
    lib = ctx.lib
    plan = SuperpointPlan()
    plan.n_points, plan.n_spps, plan.n_rows, plan.device = N, S, R, dev
    plan.index, index_i64 = _as_index(superpoints.detach())
    plan.point_map, map_i64 = _as_index(point_map.detach()) if R else (None, 0)
    with torch.cuda.device(dev):
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
        plan.counts, plan.seg_off, plan.seg_pts = i32(S), i32(S + 1), i32(N)
        plan.row_off, plan.row_pts, plan.seg_rows = (i32(R + 1), i32(N), i32(N)) if R else (None, None, None)
        plan.spp_batch_offsets = torch.empty(B + 1, dtype=torch.int64, device=dev) if B else None
        offsets, offsets_i64 = _as_index(batch_offsets.detach()) if B else (None, 0)
        plan._struct = _lib.SppPlan(N, S, R, _ptr(plan.index), _ptr(plan.point_map), index_i64, map_i64,
                                    _ptr(plan.seg_off), _ptr(plan.seg_pts), _ptr(plan.counts), _ptr(plan.row_off),
                                    _ptr(plan.row_pts), _ptr(plan.seg_rows))
        ws = _workspace(who, int(lib.gapro_spp_plan_workspace_bytes(N, B)), dev, "%d points are" % N)
        d_status, h_status = _status_pair(dev, _lib.SPP_STATUS_WORDS, torch.int32, read=check)
        ctx.check(lib.gapro_spp_plan_build(ctx.handle, stream, plan.struct(), B, _ptr(offsets), offsets_i64,
                                           _ptr(plan.spp_batch_offsets), ws.data_ptr(), ws.numel(),
                                           d_status.data_ptr(), _ptr(h_status)))
        if h_status is not None:  # the call's host read of its status, asked for by check=True
            status, flags = _host_read(dev, h_status)[:2]
            _refuse(who, status, flags, _SPP_CAUSES)
    return plan


class _SuperpointPool(torch.autograd.Function):
    """Both reductions of ``superpoint_pool``, which checks the arguments first: ``(out, arg)``, ``arg`` None for the
    mean."""

    @staticmethod
    def forward(fctx, x, plan, reduce, mapped):
        Cn, S, dev = int(x.shape[1]), plan.n_spps, x.device
        fctx.plan, fctx.reduce, fctx.mapped, fctx.shape = plan, reduce, mapped, tuple(x.shape)
        out = torch.empty((S, Cn), dtype=torch.float32, device=dev)
        arg = torch.empty((S, Cn), dtype=torch.int64, device=dev) if reduce == _lib.SPP_MAX else None
        if plan.n_points == 0:
            out.zero_()
            if arg is not None:
                arg.zero_()  # N = 0: the fill value
        else:
            x = _row_contiguous(x.detach())
            ctx, stream = _ctx_stream(x)
            with torch.cuda.device(dev):
                ctx.check(ctx.lib.gapro_spp_pool_forward(ctx.handle, stream, plan.struct(), x.data_ptr(),
                                                         int(x.shape[0]), int(x.stride(0)), Cn, reduce, int(mapped),
                                                         out.data_ptr(), _ptr(arg)))
        if arg is not None:
            fctx.mark_non_differentiable(arg)
            fctx.save_for_backward(arg)
        return out, arg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out, _grad_arg=None):
        plan, reduce, mapped = fctx.plan, fctx.reduce, fctx.mapped
        dev = grad_out.device
        if plan.n_points == 0 or 0 in fctx.shape:
            return torch.zeros(fctx.shape, dtype=torch.float32, device=dev), None, None, None
        arg = fctx.saved_tensors[0] if reduce == _lib.SPP_MAX else None
        grad_out = grad_out.contiguous()
        ctx, stream = _ctx_stream(grad_out)
        with torch.cuda.device(dev):
            d_x = torch.empty(fctx.shape, dtype=torch.float32, device=dev)
            ctx.check(ctx.lib.gapro_spp_pool_backward(ctx.handle, stream, plan.struct(), grad_out.data_ptr(),
                                                      fctx.shape[1], reduce, int(mapped), _ptr(arg), d_x.data_ptr()))
        return d_x, None, None, None


def superpoint_pool(x, plan, reduce="mean", *, return_arg=False, through_map=None):
    """``torch_scatter.scatter_mean`` / ``scatter_max`` of ``x`` (float32 ``[R, C]`` or ``[R]``, on the plan's device)
    to the superpoints of ``plan``: float32 ``[S, C]`` (``[S]``), differentiable in ``x``; with ``return_arg=True``
    (max only) also ``arg`` int64 of the same shape.

    The definition.  A superpoint's points are taken IN ASCENDING POINT INDEX.  ``mean``: ``((+0 +
    x_1) + x_2) + ...`` in float32, each sum rounded on its own, then a true division by ``float32(n)``; an empty
    superpoint is ``+0.0``.  ``max``: the first value, replaced by a later one only if it is greater -- the lowest point
    wins ties, a NaN never replaces and a leading NaN stays; an empty superpoint is ``+0.0`` with ``arg = N``.  The
    gradient of the mean is ``fl(g / float32(n))`` per point, of the max ``g`` at ``arg``; through a point map the
    points of a row are added in ascending point order from ``+0``.  Everything is bit for bit reproducible: there are
    no floating-point atomics.

    ``through_map`` (default: whether the plan has a point map) says whether ``x`` has the map's ``n_rows`` rows and is
    read through it, or one row a point -- a plan with a map serves both."""
    who = "superpoint_pool"
    if not isinstance(plan, SuperpointPlan):
        raise ValueError("%s: plan must come from superpoint_plan" % who)
    if reduce not in _SPP_REDUCE:
        raise ValueError("%s: reduce must be 'mean' or 'max'; other reductions are not built" % who)
    if not isinstance(return_arg, bool) or (return_arg and reduce != "max"):
        raise ValueError("%s: return_arg must be a bool, and True only with reduce='max'" % who)
    if through_map is None:
        through_map = plan.n_rows > 0
    if not isinstance(through_map, bool) or (through_map and plan.n_rows == 0):
        raise ValueError("%s: through_map must be a bool, and True only for a plan with a point_map" % who)
    rows = plan.n_rows if through_map else plan.n_points
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() not in (1, 2) or \
            int(x.shape[0]) != rows or (x.dim() == 2 and int(x.shape[1]) < 1):
        raise ValueError("%s: x must be a float32 tensor of shape [%d] or [%d, C], C >= 1" % (who, rows, rows))
    _need_device(x)
    _one_device(who, plan.device, (x,))
    flat = x.dim() == 1
    out, arg = _SuperpointPool.apply(x[:, None] if flat else x, plan, _SPP_REDUCE[reduce], through_map)
    if flat:
        out, arg = out[:, 0], (arg[:, 0] if arg is not None else None)
    return (out, arg) if return_arg else out


def _scatter_args(who, src, index, dim, dim_size):
    if not isinstance(src, torch.Tensor) or src.dim() not in (1, 2):
        raise ValueError("%s: src must be a 1-D or 2-D tensor; other ranks are not built" % who)
    if not _is_int(dim) or not (dim == 0 or (dim == -1 and src.dim() == 1)):
        raise ValueError("%s: dim=%r is not built; only dim=0, and dim=-1 of a 1-D src" % (who, dim))
    if not isinstance(index, torch.Tensor) or index.dtype not in _INDEX_DTYPES:
        raise ValueError("%s: index must be an integer tensor" % who)
    if index.dim() == 2 and src.dim() == 2 and index.shape == src.shape and \
            (index.stride(1) == 0 or index.shape[1] == 1):
        index = index[:, 0]  # the reference's index[:, None].expand_as(src)
    if index.dim() != 1 or index.shape[0] != src.shape[0]:
        raise ValueError("%s: index must be 1-D of src's length, or that vector expanded along dim 1; a general "
                         "element-wise index is not built" % who)
    if dim_size is not None:
        _positive_int_arg(who, "dim_size", dim_size)
    return index


def scatter_mean(src, index, dim=0, dim_size=None):
    """``torch_scatter.scatter_mean(src, index, dim=0, dim_size=dim_size)`` for a float32 device ``src`` of shape ``[N]``
    or ``[N, C]`` and a 1-D ``index`` (or its ``[:, None].expand_as(src)`` form), differentiable in ``src``, by
    ``superpoint_pool``'s definition.  Anything else is a ``ValueError`` that names what is not built.  ``dim_size=None``
    reads ``max(index) + 1`` from the device; an index out of range is a ``GaproError``."""
    who = "scatter_mean"
    index = _scatter_args(who, src, index, dim, dim_size)
    if src.dtype != torch.float32:
        raise ValueError("%s: only a float32 src is built" % who)
    return superpoint_pool(src, superpoint_plan(index, n_spps=dim_size), "mean")


def scatter_max(src, index, dim=0, dim_size=None):
    """``torch_scatter.scatter_max``: ``(out, arg)``; see ``scatter_mean`` for what is built and ``superpoint_pool`` for
    the definition (``arg`` int64: the lowest point index among equal maxima, ``N`` for an empty segment)."""
    who = "scatter_max"
    index = _scatter_args(who, src, index, dim, dim_size)
    if src.dtype != torch.float32:
        raise ValueError("%s: only a float32 src is built" % who)
    return superpoint_pool(src, superpoint_plan(index, n_spps=dim_size), "max", return_arg=True)


def _pool_cast(x, plan, output_type=None, **kw):
    """A pool of a float32 / half / bfloat16 tensor, computed in float32 and cast to ``output_type`` or back."""
    out = superpoint_pool(x if x.dtype == torch.float32 else x.to(torch.float32), plan, "mean", **kw)
    want = x.dtype if output_type is None else output_type
    return out if want == torch.float32 else out.to(want)


_SPP_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def custom_scatter_mean(input_feats, indices, dim=0, pool=True, output_type=None):
    """``custom_scatter_mean`` of ISBNet (isbnet/model/model_utils.py:600-613): ``scatter_mean`` of ``input_feats``
    (float32, half or bfloat16) computed in float32 and cast back to the input's dtype or to ``output_type``;
    ``pool=False`` returns the input."""
    who = "custom_scatter_mean"
    if not pool:
        return input_feats
    if not isinstance(input_feats, torch.Tensor) or input_feats.dtype not in _SPP_FLOATS:
        raise ValueError("%s: input_feats must be a float32, half or bfloat16 tensor" % who)
    if output_type is not None and not isinstance(output_type, torch.dtype):
        raise ValueError("%s: output_type must be a torch.dtype" % who)
    indices = _scatter_args(who, input_feats, indices, dim, None)
    return _pool_cast(input_feats, superpoint_plan(indices), output_type)


def isbnet_spp_pool(voxel_coords_float, voxel_output_feats, voxel_box_preds, voxel_spps, voxel_batch_offsets, *,
                    n_spps=None, use_spp_pool=True, check=False):
    """``ISBNet.spp_pool`` (isbnet/model/isbnet.py:735-748): ``(spp_coords_float, spp_output_feats, spp_box_preds,
    spp_batch_offsets)`` from ONE plan and three pools.  ``spp_batch_offsets`` (int64 ``[B + 1]``, on the device) comes
    from the plan instead of ``B`` blocking ``torch.unique`` calls.  With ``n_spps`` given the call makes no host read
    (``check=True`` adds the read of the status word); ``use_spp_pool=False`` returns the three tensors as they are."""
    who = "isbnet_spp_pool"
    feats = (voxel_coords_float, voxel_output_feats, voxel_box_preds)
    for name, t in zip(("voxel_coords_float", "voxel_output_feats", "voxel_box_preds"), feats):
        if not isinstance(t, torch.Tensor) or t.dtype not in _SPP_FLOATS or t.dim() not in (1, 2):
            raise ValueError("%s: %s must be a 1-D or 2-D float32, half or bfloat16 tensor" % (who, name))
    if not isinstance(use_spp_pool, bool):
        raise ValueError("%s: use_spp_pool must be a bool" % who)
    _index_check(who, "voxel_spps", voxel_spps)
    for name, t in zip(("voxel_coords_float", "voxel_output_feats", "voxel_box_preds"), feats):
        if int(t.shape[0]) != int(voxel_spps.shape[0]):
            raise ValueError("%s: %s has %d rows, voxel_spps %d entries" % (who, name, int(t.shape[0]),
                                                                           int(voxel_spps.shape[0])))
    plan = superpoint_plan(voxel_spps, n_spps=n_spps, batch_offsets=voxel_batch_offsets, check=check)
    _need_device(*feats)
    if not use_spp_pool:
        return voxel_coords_float, voxel_output_feats, voxel_box_preds, plan.spp_batch_offsets
    return tuple(_pool_cast(t, plan) for t in feats) + (plan.spp_batch_offsets,)


def spformer_pool(x, coords_float, rgb_feats, superpoints, v2p_map, prob_labels=None, mu_labels=None, var_labels=None,
                  *, pool="mean", n_spps=None, check=False):
    """Lines 251-280 of SPFormer's ``extract_feat`` (spformer/model/spformer.py): the gathers ``x[v2p_map]``,
    ``coords_float[v2p_map]``, ``rgb_feats[v2p_map]`` fused into their ``scatter_mean`` / ``scatter_max`` through the
    plan's point map, and the three per-point label channels pooled by the same plan.  ``x`` (the backbone's
    ``features``), ``coords_float`` and ``rgb_feats`` are per voxel, the labels per point.  Returns the reference's
    3-tuple, or its 6-tuple when ``prob_labels`` is given; the gradient reaches ``x`` only.  With ``n_spps`` given the
    call makes no host read (``check=True`` adds the read of the status word)."""
    who = "spformer_pool"
    _tensor_arg(who, "x", x, ("R", "C"))
    R = int(x.shape[0])
    _tensor_arg(who, "coords_float", coords_float, (R, "D"))
    _tensor_arg(who, "rgb_feats", rgb_feats, (R, "D"))
    if pool not in _SPP_REDUCE:
        raise ValueError("%s: pool must be 'mean' or 'max'" % who)
    labels = (prob_labels, mu_labels, var_labels)
    if any(t is None for t in labels) and prob_labels is not None:
        raise ValueError("%s: prob_labels comes with mu_labels and var_labels" % who)
    _index_check(who, "superpoints", superpoints)
    N = int(superpoints.shape[0])
    if prob_labels is not None:
        for name, t in zip(("prob_labels", "mu_labels", "var_labels"), labels):
            _tensor_arg(who, name, t, (N,))
    if R < 1 or int(x.shape[1]) < 1:
        raise ValueError("%s: x needs a row and a channel" % who)
    plan = superpoint_plan(superpoints, n_spps=n_spps, point_map=v2p_map, n_rows=R, check=check)
    outs = [superpoint_pool(x, plan, pool), superpoint_pool(coords_float.detach(), plan, pool),
            superpoint_pool(rgb_feats.detach(), plan, pool)]
    if prob_labels is not None:
        outs += [superpoint_pool(t.detach(), plan, pool, through_map=False) for t in labels]
    return tuple(outs)


# ---- ISBNet's dynamic-convolution mask head (gapro_amd/csrc/dyco_head.hip) ------------------------------
def dyco_param_count(mask_dim_out):
    """The length P of a controller row for ``mask_dim_out`` channels: ``(C + 6) C + C C/2 + C/2 + C + C/2 + 1`` (1793
    at C = 32, 513 at C = 16).  Any other C is a ``ValueError``: it is not built."""
    ok = _is_int(mask_dim_out) and 0 < mask_dim_out < 2 ** 31
    P = int(_lib.load().gapro_dyco_param_count(mask_dim_out)) if ok else 0
    if P == 0:
        raise ValueError("dyco_param_count: mask_dim_out must be 16 or 32; %r is not built" % (mask_dim_out,))
    return P


def _float_arg(who, name, t, shape):
    """A float32, half or bfloat16 tensor of ``shape`` (a str names a dimension of any size)."""
    ok = isinstance(t, torch.Tensor) and t.dtype in _SPP_FLOATS and t.dim() == len(shape)
    if ok:
        ok = all(h == want or want.__class__ is str for h, want in zip(t.shape, shape))
    if not ok:
        raise ValueError("%s: %s must be a float32, half or bfloat16 tensor of shape [%s]"
                         % (who, name, ", ".join(str(v) for v in shape)))


class _DynamicMaskHead(torch.autograd.Function):
    """The one autograd node of ``dynamic_mask_head``, which checks the arguments first: the packed logits forward, at
    most two kernels backward."""

    @staticmethod
    def forward(fctx, off, controllers, mask_features, locs_float, box_preds, queries_locs, queries_box_preds):
        B, Q, _ = (int(v) for v in controllers.shape)
        N, Cn = (int(v) for v in mask_features.shape)
        dev = controllers.device
        tensors = [t.detach().contiguous() for t in (controllers, locs_float, box_preds, queries_locs,
                                                     queries_box_preds)]
        feats = _row_contiguous(mask_features.detach())
        h_off = (C.c_int64 * (B + 1))(*off)
        out = torch.empty(Q * (off[-1] - off[0]), dtype=torch.float32, device=dev)
        fctx.dims = (B, Q, Cn, h_off, N, int(feats.stride(0)))
        if out.numel() > 0:
            ctx, stream = _ctx_stream(controllers)
            with torch.cuda.device(dev):
                ctx.check(ctx.lib.gapro_dyco_forward(ctx.handle, stream, B, Q, Cn, h_off, N, tensors[0].data_ptr(),
                                                     feats.data_ptr(), int(feats.stride(0)), tensors[1].data_ptr(),
                                                     tensors[2].data_ptr(), tensors[3].data_ptr(),
                                                     tensors[4].data_ptr(), None, 0, out.data_ptr()))
        fctx.save_for_backward(feats, *tensors)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out):
        feats, controllers, locs_float, box_preds, queries_locs, queries_box_preds = fctx.saved_tensors
        B, Q, Cn, h_off, N, ld = fctx.dims
        need = fctx.needs_input_grad
        dev = controllers.device
        grad_out = grad_out.to(dtype=torch.float32).contiguous()
        ctx, stream = _ctx_stream(controllers)
        with torch.cuda.device(dev):
            g_ctrl = torch.empty_like(controllers) if need[1] else None
            g_feat = torch.empty((N, Cn), dtype=torch.float32, device=dev) if need[2] else None
            g_box = torch.empty_like(box_preds) if need[4] else None
            g_qbox = torch.empty_like(queries_box_preds) if need[6] else None
            ctx.check(ctx.lib.gapro_dyco_backward(ctx.handle, stream, B, Q, Cn, h_off, N, controllers.data_ptr(),
                                                  _ptr(feats), ld, _ptr(locs_float), _ptr(box_preds),
                                                  queries_locs.data_ptr(), queries_box_preds.data_ptr(),
                                                  _ptr(grad_out), None, 0, _ptr(g_ctrl), _ptr(g_qbox), _ptr(g_feat),
                                                  _ptr(g_box)))
        return None, g_ctrl, g_feat, None, g_box, None, g_qbox


def dynamic_mask_head(controllers, mask_features, locs_float, box_preds, queries_locs, queries_box_preds,
                      batch_offsets, *, check=True):
    """The dynamic-convolution loop of ``ISBNet.forward_head`` (isbnet/model/isbnet.py:783-828, with
    ``parse_dynamic_params`` :834-853 and ``mask_heads_forward`` :855-885) for a whole batch: ``mask_logits``, a list of B
    entries, ``None`` for a sample without points and otherwise ``f32[Q, N_b]``, a view into ONE packed output -- what
    ``hungarian_match``, ``matched_losses`` and ``get_instance`` take.  One launch forward; nothing of the reference's
    ``[Q, C + 6, N_b]`` input exists, forward or backward.

    ``controllers`` ``[B, Q, P]`` is the controller head's output as it stands (``P = dyco_param_count(C)``: W1, W2, W3,
    b1, b2, b3 in ``parse_dynamic_params``'s order; b3 is not read), ``mask_features`` ``[N, C]`` or ``[N, C, 1]`` with C
    16 or 32, ``locs_float`` ``[N, 3]``, ``box_preds`` ``[N, 6]``, ``queries_locs`` ``[B, Q, 3]``, ``queries_box_preds``
    ``[B, Q, 6]``, ``batch_offsets`` ``B + 1`` host integers.  Float32, half or bfloat16 tensors, computed from their
    float32 values; the logits are float32.

    Float64 from the float32 inputs on the FP64 matrix cores, rounded once; no floating-point atomics,
    so two calls give equal bytes.  Differentiable in ``controllers`` (the b3 column gets exact zeros), ``mask_features``,
    ``box_preds`` and ``queries_box_preds`` by hand-derived kernels that recompute the hidden layers; ``locs_float`` and
    ``queries_locs`` get ``None``, as they carry no gradient in the reference's step.  relu' at 0 and the derivative of
    ``|d|`` at 0 are 0, as torch's.  Bad shapes, dtypes, devices or offsets, a C that is not built, a P that does not
    match C and more than 64 samples are ``ValueError``s before a device is touched.  The call only enqueues; ``check``
    is accepted for the family's signature and has nothing to read back."""
    who = "dynamic_mask_head"
    if not isinstance(check, bool):
        raise ValueError("%s: check must be a bool" % who)
    _float_arg(who, "controllers", controllers, ("B", "Q", "P"))
    B, Q, P = (int(v) for v in controllers.shape)
    if B < 1 or Q < 1:
        raise ValueError("%s: controllers needs a sample and a query" % who)
    if B > _lib.DYCO_MAX_BATCH:
        raise ValueError("%s: %d samples; at most %d are built" % (who, B, _lib.DYCO_MAX_BATCH))
    if isinstance(mask_features, torch.Tensor) and mask_features.dim() == 3 and mask_features.shape[2] == 1:
        mask_features = mask_features[:, :, 0]
    _float_arg(who, "mask_features", mask_features, ("N", "C"))
    N, Cn = (int(v) for v in mask_features.shape)
    if Cn not in (16, 32):
        raise ValueError("%s: mask_features has %d channels; 16 and 32 are built" % (who, Cn))
    if P != dyco_param_count(Cn):
        raise ValueError("%s: controllers rows hold %d parameters; %d channels need %d"
                         % (who, P, Cn, dyco_param_count(Cn)))
    _float_arg(who, "locs_float", locs_float, (N, 3))
    _float_arg(who, "box_preds", box_preds, (N, 6))
    _float_arg(who, "queries_locs", queries_locs, (B, Q, 3))
    _float_arg(who, "queries_box_preds", queries_box_preds, (B, Q, 6))
    off = _host_offsets_arg(who, batch_offsets, B, N)
    tensors = (controllers, mask_features, locs_float, box_preds, queries_locs, queries_box_preds)
    _one_device(who, controllers.device, tensors)
    _need_device(*tensors)
    tensors = [t if t.dtype == torch.float32 else t.to(torch.float32) for t in tensors]
    out = _DynamicMaskHead.apply(off, *tensors)
    if off[-1] - off[0] == off[1] - off[0] > 0:
        return [out.view(Q, off[1] - off[0])] + [None] * (B - 1)  # one sample holds every point: no slice node
    return [out[Q * (a - off[0]):Q * (b - off[0])].view(Q, b - a) if b > a else None for a, b in zip(off, off[1:])]


def mask_heads_forward(mask_features, weights, biases, num_insts, coords_, boxes_, queries_coords, queries_boxes):
    """``ISBNet.mask_heads_forward`` (isbnet/model/isbnet.py:855-885) for one sample, for the inference path and for
    callers that hold the parameters as ``parse_dynamic_params`` split them: ``mask_features`` ``[N, C, 1]`` (or
    ``[N, C]``), ``weights`` ``[n, C + 6, C]``, ``[n, C, C/2]``, ``[n, C/2, 1]``, ``biases`` ``[n, C]``, ``[n, C/2]``,
    ``[n, 1]``, ``coords_`` ``[N, 3]``, ``boxes_`` ``[N, 6]``, ``queries_coords`` ``[n, 3]``, ``queries_boxes``
    ``[n, 6]``; returns ``f32[n, N]``.  The parameters are packed back into controller rows with torch ops, so autograd
    reaches them, and ``dynamic_mask_head`` does the rest; the reference's sixteen S3DIS chunks are not needed, since
    nothing of size ``n x C x N`` is materialised."""
    who = "mask_heads_forward"
    if not isinstance(weights, (list, tuple)) or not isinstance(biases, (list, tuple)) or len(weights) != 3 or \
            len(biases) != 3 or not all(isinstance(t, torch.Tensor) and t.dim() >= 1 for t in (*weights, *biases)):
        raise ValueError("%s: weights and biases must be the three tensors each of parse_dynamic_params" % who)
    if not _is_int(num_insts) or any(int(t.shape[0]) != num_insts for t in (*weights, *biases)):
        raise ValueError("%s: every weight and bias must have num_insts rows" % who)
    if num_insts < 1:
        raise ValueError("%s: num_insts must be positive" % who)
    controllers = torch.cat([t.reshape(num_insts, -1) for t in (*weights, *biases)], dim=1)[None]
    for name, t in (("queries_coords", queries_coords), ("queries_boxes", queries_boxes)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError("%s: %s must be a 2-D tensor" % (who, name))
    n_points = int(mask_features.shape[0]) if isinstance(mask_features, torch.Tensor) and mask_features.dim() else 0
    out = dynamic_mask_head(controllers, mask_features, coords_, boxes_, queries_coords[None], queries_boxes[None],
                            [0, n_points])[0]
    return out if out is not None else controllers.new_zeros((num_insts, 0), dtype=torch.float32)


# ---- SPFormer's criterion (gapro_amd/csrc/spf_loss.hip, match_cost.hip, lsap.cc) ------------------------
SPF_LOSS_NAMES = ("cls_loss", "mask_bce_loss", "mask_dice_loss", "score_loss", "levelset_loss")  # the table's columns
_SPF_OUT_NAMES = ("cls_loss", "score_loss", "mask_bce_loss", "mask_dice_loss", "levelset_loss")  # loss_out's order
_SPF_CAUSES = ((1, "a GT label outside [0, num_class)"), (2, "a GT mask value that is neither 0 nor 1"))
_SPF_PRED_KEYS = ("labels", "scores", "masks", "sp_coords", "sp_rgb_feats", "batch_offsets", "sp_prob_labels",
                  "sp_mu_labels", "sp_var_labels", "sp_mu_preds", "sp_logvar_preds")
_SPF_MASK_DTYPES = (torch.float32, torch.bool, torch.uint8, torch.int32, torch.int64)
_spf_zeros = {}  # device -> the float32 zeros that stand in for the confidences and boxes SPFormer's matcher lacks


def _spf_zero_buffer(dev, n):
    if dev not in _spf_zeros or _spf_zeros[dev].numel() < n:
        _spf_zeros[dev] = torch.zeros(n, dtype=torch.float32, device=dev)
    return _spf_zeros[dev]


def _spf_insts_arg(who, insts):
    """The GT of every sample, duck-typed (an object or a dict with ``gt_labels``, ``gt_spmasks``, ``gt_boxes``):
    ``None`` for a sample without an instance (the reference's ``len(inst) == 0``), else ``(labels, masks, boxes)`` as
    given; returns them, the tensors and the labels' dtype."""
    if not isinstance(insts, (list, tuple)) or not insts:
        raise ValueError("%s: insts must be a non-empty list, one entry per sample" % who)
    out, tensors, cls_dtype = [], [], None
    for b, inst in enumerate(insts):
        who_b = "%s: sample %d" % (who, b)
        try:
            cls, mask, box = ((inst[k] for k in ("gt_labels", "gt_spmasks", "gt_boxes")) if isinstance(inst, dict)
                              else (inst.gt_labels, inst.gt_spmasks, inst.gt_boxes))
            n = len(cls) if isinstance(inst, dict) else len(inst)
        except (AttributeError, KeyError, TypeError):
            raise ValueError("%s: an object or dict with gt_labels, gt_spmasks, gt_boxes and a length is expected"
                             % who_b) from None
        if n == 0:
            out.append(None)
            continue
        if not isinstance(mask, torch.Tensor) or mask.dim() != 2 or mask.dtype not in _SPF_MASK_DTYPES \
                or mask.shape[0] != n or mask.shape[1] == 0:
            raise ValueError("%s: gt_spmasks must be a float32, bool or integer tensor of shape [%d, S]" % (who_b, n))
        cls_dtype = _sample_labels_arg(who_b, "gt_labels", cls, "gt_boxes", box, n, cls_dtype)
        out.append((cls, mask, box))
        tensors += [cls, mask, box]
    return out, tensors, cls_dtype


def _spf_heads_arg(who, pred_labels, pred_masks, B, pred_scores=None):
    """One head's tensors or lists over heads, as lists over heads; returns them with L1, Q, C and the tensors."""
    single = isinstance(pred_labels, torch.Tensor)
    labels = [pred_labels] if single else pred_labels
    masks = [pred_masks] if single else pred_masks
    scores = None if pred_scores is None else ([pred_scores] if single else pred_scores)
    if not isinstance(labels, (list, tuple)) or not labels:
        raise ValueError("%s: pred_labels must be a tensor or a non-empty list of tensors, one per head" % who)
    L1 = len(labels)
    for name, seq in (("pred_masks", masks), ("pred_scores", scores)):
        if seq is not None and (not isinstance(seq, (list, tuple)) or len(seq) != L1):
            raise ValueError("%s: %s must follow pred_labels: one head's, or a list of %d heads" % (who, name, L1))
    _tensor_arg(who, "pred_labels", labels[0], (B, "Q", "C"), nonempty=True)
    _, Q, n_classes = (int(v) for v in labels[0].shape)
    if n_classes < 2:
        raise ValueError("%s: pred_labels needs a class beside \"no object\"" % who)
    if L1 * B > _lib.SPP_GT_MAX_SAMPLES:
        raise ValueError("%s: %d heads of %d samples; heads * samples beyond %d" % (who, L1, B, _lib.SPP_GT_MAX_SAMPLES))
    tensors = []
    for h in range(L1):
        who_h = "%s: head %d" % (who, h)
        _tensor_arg(who_h, "pred_labels", labels[h], (B, Q, n_classes))
        if not isinstance(masks[h], (list, tuple)) or len(masks[h]) != B:
            raise ValueError("%s: pred_masks must be a list of %d tensors, one per sample" % (who_h, B))
        for x in masks[h]:
            _tensor_arg(who_h, "pred_masks", x, (Q, "S"))
        tensors += [labels[h], *masks[h]]
        if scores is not None:
            s = scores[h]
            if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or tuple(s.shape) not in ((B, Q), (B, Q, 1)):
                raise ValueError("%s: pred_scores must be a float32 tensor of shape [%d, %d, 1] or [%d, %d]"
                                 % (who_h, B, Q, B, Q))
            tensors.append(s)
    return single, labels, masks, scores, L1, Q, n_classes, tensors


def _spf_widths_arg(who, masks, gts, Q):
    """The number of columns of every sample: every head's mask logits and the sample's GT masks agree on it."""
    widths = [int(x.shape[1]) for x in masks[0]]
    for h, head in enumerate(masks):
        for b, x in enumerate(head):
            want = int(gts[b][1].shape[1]) if gts[b] is not None else widths[b]
            if int(x.shape[1]) != want or (want == 0 and gts[b] is not None):
                raise ValueError("%s: head %d, sample %d: pred_masks is %s, [%d, %d] is expected: one row per query and "
                                 "one column per superpoint" % (who, h, b, tuple(x.shape), Q, want))
    return [int(gts[b][1].shape[1]) if gts[b] is not None else widths[b] for b in range(len(widths))]


def _three_weights_arg(who, cost_weight):
    try:
        vals = [float(v) for v in cost_weight]
    except (TypeError, ValueError):
        vals = []
    if len(vals) != 3 or any(not _is_finite(v) or v < 0.0 for v in vals):
        raise ValueError("%s: cost_weight must be three finite, non-negative numbers (class, mask BCE, dice)" % who)
    return vals


def spformer_match(pred_labels, pred_masks, insts, cost_weight=(1.0, 1.0, 1.0)):
    """SPFormer's ``HungarianMatcher.forward`` (SPFormer/spformer/model/loss.py:198-222) for every prediction head of a
    step at once: per head and sample the reference's ``(rows, cols)`` pair of int64 CPU tensors, ``([], [])`` as two
    empty tensors for a sample without an instance.  ``pred_labels`` is one head's ``f32[B, Q, C]`` and ``pred_masks``
    its list of ``f32[Q, S_b]`` (the result is then a list over the samples), or both are lists over the heads (a list
    over the heads of such lists).  ``insts`` holds per sample any object with ``gt_labels`` (int32 / int64 ``[n]``),
    ``gt_spmasks`` (``[n, S_b]`` of 0 / 1: float32, bool or integer), ``gt_boxes`` (``f32[n, 6]``) and ``len()``, or a
    dict with these keys.  ``cost_weight`` is the reference's: class, mask BCE, dice.

    All heads x samples are the "samples" of ONE ``gapro_match_cost`` call (the cost terms are the ISBNet matcher's
    class, BCE and dice terms; its confidence and GIoU terms get the weight 0 and a buffer of zeros, and a weight of 0
    times a finite term adds an exact zero, so nothing of ``gt_boxes`` reaches the cost).  The costs go to page-locked
    memory behind the kernels, one stream synchronisation covers them all, and the assignments are solved by the
    library on the host.  The matched pairs stay on the host: ``spformer_layer_losses`` uploads them inside its one
    table.  A cost that is NaN or infinite becomes 100000, which the reference does not do (SciPy refuses such a
    matrix).  No autograd.  Mismatched shapes, dtypes or devices, and more than ``1024`` heads x samples, are
    ``ValueError``s before a device is touched; a label outside ``[0, C)`` or a mask value other than 0 / 1 is a
    ``GaproError``."""
    who = "spformer_match"
    gts, tensors, cls_dtype = _spf_insts_arg(who, insts)
    B = len(gts)
    single, labels, masks, _, L1, Q, n_classes, head_tensors = _spf_heads_arg(who, pred_labels, pred_masks, B)
    _spf_widths_arg(who, masks, gts, Q)
    cw = _three_weights_arg(who, cost_weight)
    dev = labels[0].device
    _one_device(who, dev, tensors + head_tensors)
    empty = (torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64))
    out = [[empty] * B for _ in range(L1)]
    kept = [h * B + b for h in range(L1) for b in range(B) if gts[b] is not None]
    if kept:
        _need_device(labels[0])
        T = L1 * B
        zeros = _spf_zero_buffer(dev, max(T * Q, max(len(g[0]) for g in gts if g is not None)) * 6)
        entries = [None if g is None else {"mask": g[1] if g[1].dtype == torch.float32 else g[1].float(), "cls": g[0],
                                           "box": zeros[:len(g[0]) * 6].view(-1, 6)} for g in gts]
        stacked = labels[0].detach() if L1 == 1 else torch.cat([z.detach() for z in labels])
        _, host = _match_run(who, stacked, [x.detach() for head in masks for x in head], zeros[:T * Q].view(T, Q),
                             zeros[:T * Q * 6].view(T, Q, 6), entries * L1, kept, cls_dtype,
                             _lib.MatchWeights(cw[0], cw[2], cw[1], 0.0, 0.0), True)
        for k, (r, c) in zip(kept, _solve_all([(host[k], 1) for k in kept])):
            out[k // B][k % B] = (torch.from_numpy(r), torch.from_numpy(c))
    return out[0] if single else out


def _spf_indices_arg(who, indices, single, L1, gts, Q):
    """The matched pairs as int32 NumPy arrays per (head, sample); ``None`` for a skipped sample."""
    indices = [indices] if single else indices
    B = len(gts)
    if not isinstance(indices, (list, tuple)) or len(indices) != L1 \
            or any(not isinstance(head, (list, tuple)) or len(head) != B for head in indices):
        raise ValueError("%s: indices must hold, per head, one (rows, cols) pair per sample, as spformer_match returns "
                         "them" % who)
    out = []
    for h, head in enumerate(indices):
        for b, pair in enumerate(head):
            who_b = "%s: head %d, sample %d" % (who, h, b)
            try:
                rows, cols = pair
                if any(isinstance(v, torch.Tensor) and v.device.type != "cpu" for v in pair):
                    raise TypeError
                rows, cols = np.asarray(rows), np.asarray(cols)
                if rows.size == 0 and cols.size == 0:
                    rows = cols = np.empty(0, dtype=np.int64)
                if rows.ndim != 1 or rows.shape != cols.shape or rows.dtype.kind not in "iu" or cols.dtype.kind not in "iu":
                    raise TypeError
            except (TypeError, ValueError):
                raise ValueError("%s: a (rows, cols) pair of 1-D integer host arrays of one length is expected"
                                 % who_b) from None
            if gts[b] is None:
                if rows.size:
                    raise ValueError("%s: matched pairs for a sample without an instance" % who_b)
                out.append(None)
                continue
            n_inst = len(gts[b][0])
            if rows.size == 0:
                raise ValueError("%s: no matched pair for a sample with instances" % who_b)
            if int(rows.min()) < 0 or int(rows.max()) >= Q or len(np.unique(rows)) != rows.size:
                raise ValueError("%s: the rows must be distinct and inside [0, %d)" % (who_b, Q))
            if int(cols.min()) < 0 or int(cols.max()) >= n_inst:
                raise ValueError("%s: a column outside [0, %d)" % (who_b, n_inst))
            out.append((rows.astype(np.int32), cols.astype(np.int32)))
    return out


def _spf_offsets_arg(who, batch_offsets, widths, n_points):
    """The first column of every sample.  ``None`` (and a device tensor, which is not read): the samples' columns follow
    each other from 0, the one layout the reference's ``[b_s:b_e]`` slices allow; host integers are checked against it."""
    off = [0]
    for wd in widths:
        off.append(off[-1] + wd)
    if isinstance(batch_offsets, torch.Tensor):
        batch_offsets = batch_offsets.tolist() if batch_offsets.device.type == "cpu" else None
    if batch_offsets is not None:
        try:
            given = [int(v) for v in batch_offsets]
            if any(g != v for g, v in zip(given, batch_offsets)):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("%s: batch_offsets must be integers" % who) from None
        if len(given) != len(off) or any(b - a != wd for a, b, wd in zip(given, given[1:], widths)) or given[0] < 0:
            raise ValueError("%s: batch_offsets must hold batch_size + 1 integers whose steps are the samples' numbers of "
                             "mask columns" % who)
        off = given
    if off[-1] > n_points:
        raise ValueError("%s: the samples have %d columns, sp_prob_labels %d entries" % (who, off[-1], n_points))
    return off


class _SpfLayerLosses(torch.autograd.Function):
    """The one autograd node of ``spformer_layer_losses``: ``f32[L1, 5]`` forward, one kernel backward."""

    @staticmethod
    def forward(fctx, plan, *heads):
        who = "spformer_layer_losses"
        L1, B, Q, n_classes = plan["L1"], plan["B"], plan["Q"], plan["C"]
        labels = [z.contiguous() for z in heads[:L1]]
        scores = [s.contiguous() for s in heads[L1:2 * L1]]
        masks = iter(heads[2 * L1:])
        ctx, stream = _ctx_stream(labels[0])
        lib, dev = ctx.lib, labels[0].device
        gts, off, pairs = plan["gts"], plan["off"], plan["pairs"]
        T = L1 * B
        tasks = (_lib.SpfLossTask * T)()
        xs, rows, cols, total_gt, grad_spans, grad_floats = [], [], [], 0, [], 0
        for h in range(L1):
            for b in range(B):
                z_ptr, s_ptr = labels[h].data_ptr() + 4 * b * Q * n_classes, scores[h].data_ptr() + 4 * b * Q
                if gts[b] is None:
                    tasks[h * B + b] = _lib.SpfLossTask(z_ptr, s_ptr, None, 0, None, None, None, 0, 0, 0, 0, 0, total_gt)
                    continue
                x = _row_contiguous(next(masks))
                xs.append(x)
                cls, mask, box = gts[b]
                r, c = pairs[h * B + b]
                n_inst, n_cols = (int(v) for v in mask.shape)
                tasks[h * B + b] = _lib.SpfLossTask(z_ptr, s_ptr, x.data_ptr(), int(x.stride(0)), mask.data_ptr(),
                                                    cls.data_ptr(), box.data_ptr(), len(r), n_inst, n_cols, 0, off[b],
                                                    total_gt)
                rows.append(r)
                cols.append(c)
                total_gt += len(r)
                grad_spans.append((grad_floats, n_cols))
                grad_floats += Q * n_cols
        rows = np.ascontiguousarray(np.concatenate(rows), dtype=np.int32) if rows else np.zeros(1, dtype=np.int32)
        cols = np.ascontiguousarray(np.concatenate(cols), dtype=np.int32) if cols else np.zeros(1, dtype=np.int32)
        prob, feats, coords = plan["prob"], plan["feats"], plan["coords"]
        dims = _lib.SpfLossDims(L1, B, Q, n_classes, _LABEL_CODES[plan["cls_dtype"]], int(feats.shape[1]),
                                plan["min_points"], plan["flags"], plan["non_object_weight"])
        with torch.cuda.device(dev):
            ws = _workspace(who, int(lib.gapro_spf_loss_workspace_bytes(L1, B, Q, total_gt)), dev,
                            "%d heads, %d samples and %d queries are" % (L1, B, Q))
            out = torch.empty((L1, _lib.SPF_LOSS_N), dtype=torch.float32, device=dev)
            d_status, h_status = _status_pair(dev, _lib.MATCH_STATUS_WORDS, torch.int32, read=plan["check"])
            ctx.check(lib.gapro_spf_loss_forward(ctx.handle, stream, C.byref(dims), C.cast(tasks, C.c_void_p),
                                                 rows.ctypes.data, cols.ctypes.data, prob.data_ptr(), feats.data_ptr(),
                                                 coords.data_ptr(), int(prob.shape[0]), ws.data_ptr(), ws.numel(),
                                                 out.data_ptr(), d_status.data_ptr(), _ptr(h_status)))
            if h_status is not None:  # the call's one host read, asked for by check=True
                status, bad, flags = _host_read(dev, h_status)[:3]
                _refuse("%s: head %d, sample %d" % (who, bad // B, bad % B), status, flags, _SPF_CAUSES)
        fctx.save_for_backward(*labels, *scores, *xs)
        fctx.held = (gts, prob, feats, coords, ws, dims, total_gt, grad_spans, grad_floats,
                     [s.shape for s in heads[L1:2 * L1]])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out):
        _, prob, feats, coords, ws, dims, total_gt, grad_spans, grad_floats, score_shapes = fctx.held
        L1, B, Q, n_classes = dims.n_heads, dims.batch_size, dims.n_queries, dims.n_classes
        saved = fctx.saved_tensors
        ctx, stream = _ctx_stream(saved[0])
        dev = saved[0].device
        need = fctx.needs_input_grad[1:]
        grad_out = grad_out.to(dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            g_labels = torch.empty((L1, B, Q, n_classes), dtype=torch.float32, device=dev) if any(need[:L1]) else None
            g_scores = torch.empty((L1, B, Q), dtype=torch.float32, device=dev) if any(need[L1:2 * L1]) else None
            g_mask = torch.empty(grad_floats, dtype=torch.float32, device=dev) \
                if grad_floats and any(need[2 * L1:]) else None
            ctx.check(ctx.lib.gapro_spf_loss_backward(ctx.handle, stream, C.byref(dims), total_gt, prob.data_ptr(),
                                                      feats.data_ptr(), coords.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      grad_out.data_ptr(), _ptr(g_labels), _ptr(g_scores),
                                                      _ptr(g_mask)))
        grads = [g_labels[h] if need[h] else None for h in range(L1)]
        grads += [g_scores[h].view(score_shapes[h]) if need[L1 + h] else None for h in range(L1)]
        grads += [g_mask[first:first + Q * n_cols].view(Q, n_cols) if need[2 * L1 + k] else None
                  for k, (first, n_cols) in enumerate(grad_spans)]
        return (None, *grads)


def spformer_layer_losses(pred_labels, pred_scores, pred_masks, insts, indices, sp_coords, sp_rgb_feats,
                          sp_prob_labels, batch_offsets=None, *, non_object_weight=0.1, num_class=None,
                          weighted_bce=False, dice_div_main=False, min_points=100, check=True):
    """The five losses of every prediction head of SPFormer's ``Criterion`` (SPFormer/spformer/model/loss.py:415-499 for
    the main head, :263-349 for an aux head) in two kernels: ``f32[L1, 5]`` with the columns ``SPF_LOSS_NAMES`` (cls,
    mask_bce, mask_dice, score, levelset), one autograd node; its backward is one kernel, which reads the upstream
    ``f32[L1, 5]`` on the device and writes every element of every head's label, score and mask-logit gradients.

    ``pred_labels`` / ``pred_scores`` / ``pred_masks`` are one head's ``f32[B, Q, C]``, ``f32[B, Q, 1]`` (or ``[B, Q]``)
    and list of ``f32[Q, S_b]``, or lists over the heads with THE MAIN HEAD LAST (``aux_outputs[i]`` is head ``i``).
    ``insts`` and ``indices`` are ``spformer_match``'s argument and result.  ``sp_coords`` ``f32[N, 3]``,
    ``sp_rgb_feats`` ``f32[N, F]`` (1 <= F <= 8) and ``sp_prob_labels`` ``f32[N]`` hold the samples' superpoints one
    after the other; ``batch_offsets`` is ``None``, ``B + 1`` host integers (checked against the masks' widths) or a
    device tensor, which is NOT read: the samples' columns then follow each other from 0.

    The rule is include/gapro_hip.h's ("SPFormer's criterion"): float64 from the float32 inputs, one
    rounding, no floating-point atomics.  Two quirks of the released code are reproduced by default:
    ``mask_bce`` is the plain mean BCE (``reduce="none"`` is the legacy boolean and selects the mean), times
    ``sum(w) / sum(w)``, which is 1, or NaN for a weight sum that is 0 or not finite; ``weighted_bce=True`` gives the
    ``sp_prob_labels``-weighted mean the code means.  ``mask_dice`` of the main head is not divided by B while the aux
    heads' is; ``dice_div_main=True`` divides it too.  ``min_points`` is the reference's 100: a box with fewer columns
    inside takes no part in the level-set term.  A sample without an instance adds its Q "no object" rows to the class
    loss and nothing else; a batch of such samples is legitimate.

    Shapes, dtypes, devices, offsets, pairs out of range and ``F`` outside 1 .. 8 are ``ValueError``s before a device
    is touched.  A GT label outside ``[0, num_class)`` or a matched mask value other than 0 / 1 is refused by the device:
    with ``check=True`` the status is read behind the kernels (the call's one synchronisation) and a ``GaproError``
    raised; with ``check=False`` the call only enqueues, every loss is NaN and the backward writes zeros."""
    who = "spformer_layer_losses"
    gts, tensors, cls_dtype = _spf_insts_arg(who, insts)
    B = len(gts)
    single, labels, masks, scores, L1, Q, n_classes, head_tensors = _spf_heads_arg(who, pred_labels, pred_masks, B,
                                                                                   pred_scores)
    if pred_scores is None:
        raise ValueError("%s: pred_scores is missing" % who)
    widths = _spf_widths_arg(who, masks, gts, Q)
    pairs = _spf_indices_arg(who, indices, single, L1, gts, Q)
    _tensor_arg(who, "sp_prob_labels", sp_prob_labels, ("N",), nonempty=True)
    N = int(sp_prob_labels.shape[0])
    _tensor_arg(who, "sp_rgb_feats", sp_rgb_feats, (N, "F"))
    if not 1 <= int(sp_rgb_feats.shape[1]) <= _lib.MATCH_LOSS_MAX_FEATS:
        raise ValueError("%s: %d level-set features; 1 to %d are expected"
                         % (who, int(sp_rgb_feats.shape[1]), _lib.MATCH_LOSS_MAX_FEATS))
    _tensor_arg(who, "sp_coords", sp_coords, (N, 3))
    off = _spf_offsets_arg(who, batch_offsets, widths, N)
    _finite_arg(who, "non_object_weight", non_object_weight)
    _positive_int_arg(who, "min_points", min_points)
    if num_class is not None and (not _is_int(num_class) or num_class != n_classes - 1):
        raise ValueError("%s: num_class=%r, pred_labels has %d classes (num_class + 1 is expected)"
                         % (who, num_class, n_classes))
    for name, v in (("weighted_bce", weighted_bce), ("dice_div_main", dice_div_main), ("check", check)):
        if not isinstance(v, bool):
            raise ValueError("%s: %s must be a bool" % (who, name))
    dev = labels[0].device
    _one_device(who, dev, tensors + head_tensors + [sp_prob_labels, sp_rgb_feats, sp_coords])
    _need_device(labels[0])
    kept = [b for b in range(B) if gts[b] is not None]
    dev_gts = [None if g is None else (g[0].contiguous(), (g[1] if g[1].dtype == torch.float32 else g[1].float())
                                       .contiguous(), g[2].contiguous()) for g in gts]
    plan = {"L1": L1, "B": B, "Q": Q, "C": n_classes, "gts": dev_gts, "off": off, "pairs": pairs,
            "cls_dtype": cls_dtype or torch.int64, "prob": sp_prob_labels.detach().contiguous(),
            "feats": sp_rgb_feats.detach().contiguous(), "coords": sp_coords.detach().contiguous(),
            "min_points": int(min_points), "non_object_weight": float(non_object_weight), "check": check,
            "flags": (_lib.SPF_WEIGHTED_BCE if weighted_bce else 0) | (_lib.SPF_DICE_DIV_MAIN if dice_div_main else 0)}
    return _SpfLayerLosses.apply(plan, *labels, *scores, *[masks[h][b] for h in range(L1) for b in kept])


def spformer_criterion(pred, insts, *, loss_weight=(1.0, 1.0, 1.0, 1.0, 0.5), cost_weight=(1.0, 1.0, 1.0),
                       non_object_weight=0.1, num_class=18, weighted_bce=False, dice_div_main=False, min_points=100,
                       check=True, as_floats=False):
    """SPFormer's ``Criterion.forward`` (SPFormer/spformer/model/loss.py:393-556) with the constructor's arguments as
    keywords: it reads the same keys of ``pred`` (``labels``, ``scores``, ``masks``, ``sp_coords``, ``sp_rgb_feats``,
    ``batch_offsets``, ``sp_prob_labels``, ``sp_mu_labels``, ``sp_var_labels``, ``sp_mu_preds``, ``sp_logvar_preds`` and,
    when present, ``aux_outputs``: a list of dicts with ``labels``, ``scores``, ``masks``) and returns ``(loss,
    loss_out)``.  ``loss_out`` has the reference's keys in its order: ``cls_loss``, ``score_loss``, ``mask_bce_loss``,
    ``mask_dice_loss``, ``levelset_loss``, ``kl_loss``, then ``layer_{i}_`` + the first five for each aux head, then
    ``loss``; its values are detached 0-dim device tensors, or with ``as_floats=True`` Python floats from ONE host copy
    of the whole table (the reference's ``.item()``s, about 35 of them at the released configuration).

    Pure composition: ``spformer_match`` over all heads, ``spformer_layer_losses`` (``loss_weight`` is cls, mask BCE,
    dice, score, level set, applied to every head), and ``kl_to_gp_loss(..., weight=0.1)``.  As released the main head's
    dice loss is not divided by the batch size and the mask BCE is unweighted; see ``spformer_layer_losses`` for the two
    switches.  A ``batch_offsets`` on the device is not read.  With ``check=False`` the only host synchronisation of
    the call is the matcher's.  A missing key, a ``loss_weight`` that is not five finite numbers and everything the
    composed calls refuse are ``ValueError``s before a device is touched."""
    who = "spformer_criterion"
    if not isinstance(pred, dict):
        raise ValueError("%s: pred must be a dict" % who)
    for k in _SPF_PRED_KEYS:
        if k not in pred:
            raise ValueError("%s: pred lacks %r" % (who, k))
    aux = pred.get("aux_outputs", [])
    if not isinstance(aux, (list, tuple)) or any(not isinstance(a, dict) or any(k not in a for k in _SPF_PRED_KEYS[:3])
                                                 for a in aux):
        raise ValueError("%s: aux_outputs must be a list of dicts with labels, scores and masks" % who)
    try:
        lw = tuple(float(v) for v in loss_weight)
    except (TypeError, ValueError):
        lw = ()
    if len(lw) != 5 or any(not _is_finite(v) for v in lw):
        raise ValueError("%s: loss_weight must be five finite numbers (cls, mask BCE, dice, score, level set)" % who)
    _positive_int_arg(who, "num_class", num_class)
    if not isinstance(as_floats, bool):
        raise ValueError("%s: as_floats must be a bool" % who)
    heads = list(aux) + [pred]  # the main head last
    labels, scores, masks = ([h[k] for h in heads] for k in ("labels", "scores", "masks"))
    if isinstance(labels[0], torch.Tensor) and labels[0].dim() == 3 and int(labels[0].shape[2]) != num_class + 1:
        raise ValueError("%s: num_class=%r, pred_labels has %d classes (num_class + 1 is expected)"
                         % (who, num_class, int(labels[0].shape[2])))
    indices = spformer_match(labels, masks, insts, cost_weight)
    table = spformer_layer_losses(labels, scores, masks, insts, indices, pred["sp_coords"], pred["sp_rgb_feats"],
                                  pred["sp_prob_labels"], pred["batch_offsets"], non_object_weight=non_object_weight,
                                  num_class=num_class, weighted_bce=weighted_bce, dice_div_main=dice_div_main,
                                  min_points=min_points, check=check)
    dev = table.device
    kl = kl_to_gp_loss(pred["sp_mu_preds"], pred["sp_logvar_preds"], pred["sp_mu_labels"], pred["sp_var_labels"],
                       weight=0.1)
    # the total in float64 from the float32 losses, rounded once: the rule of the kernels, kept to the last addition
    loss = ((table.double() * _device_constant(dev, lw, torch.float64)).sum() + kl.double()).float()
    flat = torch.cat([table.detach().reshape(-1), kl.detach().reshape(1), loss.detach().reshape(1)])
    values = flat.tolist() if as_floats else flat.unbind(0)  # as_floats: the one host copy
    L1 = len(heads)
    order = [SPF_LOSS_NAMES.index(k) for k in _SPF_OUT_NAMES]
    loss_out = {k: values[(L1 - 1) * 5 + j] for k, j in zip(_SPF_OUT_NAMES, order)}
    loss_out["kl_loss"] = values[L1 * 5]
    for i in range(L1 - 1):
        loss_out.update({"layer_%d_%s" % (i, k): values[i * 5 + j] for k, j in zip(_SPF_OUT_NAMES, order)})
    loss_out["loss"] = values[L1 * 5 + 1]
    return loss, loss_out


# ---- SPFormer's predicted instances: its inference post-processing (csrc/spf_predict.hip) --------------
_SPF_PREDICT_CAUSES = ((1, "a non-finite labels or scores entry"),
                       (2, "a non-finite masks entry in the row of a candidate"),
                       (4, "a non-finite coords_float entry"),
                       (8, "a superpoint id outside the columns of masks"))
SpfInstanceArrays = namedtuple("SpfInstanceArrays", "conf label_id box query run_offsets runs masks header n_runs")
_SPF_PREDICT_CHAIN = ("gapro_spf_predict_", _lib.SpfPredictHeader, _SPF_PREDICT_CAUSES, SpfInstanceArrays)


def spformer_instances(scan_id, pred_labels, pred_scores, pred_masks, superpoints, coords_float, *, num_class,
                       topk_insts, score_thr, npoint_thr, return_arrays=False, return_masks=False):
    """``SPFormer.predict_by_feat`` (SPFormer/spformer/model/spformer.py:180-242) on the tensors of one scene:
    ``pred_labels f32[Q, num_class + 1]``, ``pred_scores f32[Q]`` or ``[Q, 1]``, ``pred_masks f32[Q, S]`` (logits over
    the superpoints), ``superpoints int[N]`` in ``[0, S)``, ``coords_float f32[N, 3]``.  One chain of integer kernels
    (include/gapro_hip.h, "SPFormer's predicted instances") with one host read and at most two copies
    behind it; the reference's ``[topk_insts, N]`` expansion is never built.  Returns the list of ``{"scan_id",
    "label_id" (np.int64), "conf" (np.float32), "pred_mask": {"length": N, "counts": int64 array}, "box"
    (np.float32[6]: min xyz, max xyz of the instance's points)}`` in descending ``conf``, equal values in the order of
    the class scores (descending, then the flat index ``query * num_class + class``).  The reference's own order is
    undefined: it is what ``torch.topk(sorted=False)`` returns.

    ``return_arrays`` gives the device tensors (``SpfInstanceArrays``; ``masks`` u8[K', N] with ``return_masks``)
    instead of the list.  Non-finite inputs and superpoint ids out of range are a ``GaproError`` naming the cause."""
    who = "spformer_instances"
    _positive_int_arg(who, "num_class", num_class)
    if not _is_int(topk_insts) or not 1 <= topk_insts <= _lib.PROPOSALS_MAX_PRE_TOPK:
        raise ValueError("%s: topk_insts must be an int in [1, %d]" % (who, _lib.PROPOSALS_MAX_PRE_TOPK))
    _finite_arg(who, "score_thr", score_thr)
    if not _is_int(npoint_thr) or npoint_thr < 0:
        raise ValueError("%s: npoint_thr must be a non-negative int" % who)
    if not isinstance(pred_labels, torch.Tensor) or pred_labels.dim() != 2 or int(pred_labels.shape[1]) != num_class + 1:
        raise ValueError("%s: pred_labels must be f32[Q, num_class + 1]" % who)
    Q = int(pred_labels.shape[0])
    if Q < 1:
        raise ValueError("%s: no queries" % who)
    labels = _f32_arg(pred_labels, "pred_labels", who, (Q, num_class + 1))
    if isinstance(pred_scores, torch.Tensor) and pred_scores.dim() == 2 and int(pred_scores.shape[1]) == 1:
        pred_scores = pred_scores.reshape(-1)
    scores = _f32_arg(pred_scores, "pred_scores", who, (Q,))
    if not isinstance(pred_masks, torch.Tensor) or pred_masks.dim() != 2 or int(pred_masks.shape[0]) != Q:
        raise ValueError("%s: pred_masks must be f32[Q, superpoints]" % who)
    S = int(pred_masks.shape[1])
    masks = _f32_arg(pred_masks, "pred_masks", who, (Q, S))
    sp, sp_i64 = _index_arg(superpoints, "superpoints", who)
    N = int(sp.shape[0])
    coords = _f32_arg(coords_float, "coords_float", who, (N, 3))
    if S < 1 or N < 1:
        raise ValueError("%s: no superpoints or no points" % who)
    keep = (labels, scores, masks, sp, coords)
    _one_device(who, labels.device, keep)
    inputs = _lib.SpfPredictInputs(n_queries=Q, n_spps=S, n_points=N, labels=labels.data_ptr(),
                                   pred_scores=scores.data_ptr(), masks=masks.data_ptr(), superpoints=sp.data_ptr(),
                                   coords_float=coords.data_ptr(), superpoints_i64=sp_i64)
    params = _lib.SpfPredictParams(num_class=num_class, topk_insts=topk_insts, npoint_thr=npoint_thr,
                                   score_thr=float(score_thr))
    out = _predict_run(who, _SPF_PREDICT_CHAIN, labels, inputs, params, keep, N, want_masks=return_masks)
    if return_arrays:
        return out
    rows = int(out.header.n_rows)
    if rows == 0:
        return []
    small = torch.cat([out.conf.view(torch.int32), out.label_id, out.box.view(torch.int32).reshape(-1)])
    small = small.cpu().numpy()  # the small arrays: one copy
    host_runs = out.runs.cpu().numpy()  # the runs: the other
    conf_h, label_h = small[:rows].view(np.float32), small[rows:2 * rows].astype(np.int64)
    box_h = small[2 * rows:].view(np.float32).reshape(rows, 6)
    counts = _counts_of(np.concatenate([[0], np.cumsum(out.n_runs, dtype=np.int64)]), host_runs)  # came with the header
    return [{"scan_id": scan_id, "label_id": label_h[r], "conf": conf_h[r],
             "pred_mask": {"length": N, "counts": counts[r]}, "box": box_h[r].copy()} for r in range(rows)]


def spformer_predict(scan_ids, out, superpoints, insts, coords_float, *, num_class=18, test_cfg=None, topk_insts=100,
                     score_thr=0.0, npoint_thr=100):
    """``SPFormer.predict_by_feat`` with its positional signature (SPFormer/spformer/model/spformer.py:180): reads
    sample 0 of ``out["labels"]``, ``out["scores"]`` and ``out["masks"]`` as the reference does ("only batch 1 when
    test") and returns ``dict(scan_id=scan_ids[0], pred_instances=[...], gt_instances=insts[0].gt_instances)``; the
    instances and their order are ``spformer_instances``'.  ``test_cfg`` (an object with ``topk_insts``, ``score_thr``,
    ``npoint_thr``) overrides the three keywords."""
    who = "spformer_predict"
    if test_cfg is not None:
        topk_insts = getattr(test_cfg, "topk_insts", topk_insts)
        score_thr = getattr(test_cfg, "score_thr", score_thr)
        npoint_thr = getattr(test_cfg, "npoint_thr", npoint_thr)
    if not isinstance(out, dict) or any(k not in out for k in ("labels", "scores", "masks")):
        raise ValueError("%s: out must be a dict with labels, scores and masks" % who)
    if len(scan_ids) < 1 or len(insts) < 1:
        raise ValueError("%s: no scene" % who)
    for k in ("labels", "scores", "masks"):
        if len(out[k]) < 1:
            raise ValueError("%s: out[%r] holds no sample" % (who, k))
    pred = spformer_instances(scan_ids[0], out["labels"][0], out["scores"][0], out["masks"][0], superpoints,
                              coords_float, num_class=num_class, topk_insts=topk_insts, score_thr=score_thr,
                              npoint_thr=npoint_thr)
    return dict(scan_id=scan_ids[0], pred_instances=pred, gt_instances=insts[0].gt_instances)


# ---- sparse convolutions: spconv's three layers of the consumers' U-Nets (csrc/spconv.hip) ---------------
_SPCONV_CAUSES = ((1, "two rows of coords with the same coordinates"),
                  (2, "a coordinate outside spatial_shape"),
                  (4, "a batch index outside [0, batch_size)"),
                  (8, "a workspace that is not the count's"))


class SparseConvPlan:
    """The rulebook of one ``indice_key``: built once a step by ``subm_plan`` or ``downsample_plan`` and passed to every
    layer of its level.  ``kind`` is ``"subm"`` (``neighbours int32[27, V]``) or ``"down"`` (``children int32[8, V_c]``,
    ``parent int32[V]``, ``child_slot int32[V]``); ``n_in`` / ``n_out`` are the rows of the strided (or submanifold)
    layer's input and output, ``coords`` (int32 ``[n_out, 4]``) and ``spatial_shape`` those of its output -- what the
    next level's plans take."""
    __slots__ = ("kind", "device", "n_in", "n_out", "batch_size", "in_shape", "spatial_shape", "coords", "neighbours",
                 "children", "parent", "child_slot")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _plan_args(who, coords, spatial_shape, batch_size, check):
    if not isinstance(coords, torch.Tensor) or coords.dtype not in _INT or coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError("%s: coords must be an int32 or int64 tensor of shape [V, 4]" % who)
    try:
        shape = tuple(spatial_shape)
    except TypeError:
        shape = ()
    if len(shape) != 3 or not all(_is_int(d, (int, np.integer)) and 1 <= d <= 2 ** 31 - 3 for d in shape):
        raise ValueError("%s: spatial_shape must be three positive ints (Dz, Dy, Dx)" % who)
    _positive_int_arg(who, "batch_size", batch_size, (int, np.integer))
    if not isinstance(check, bool):
        raise ValueError("%s: check must be a bool" % who)
    shape, batch_size = tuple(int(d) for d in shape), int(batch_size)
    if batch_size * (shape[0] + 2) * (shape[1] + 2) * (shape[2] + 2) >= 2 ** 63:
        raise ValueError("%s: batch_size and spatial_shape are beyond the 63-bit coordinate key" % who)
    if int(coords.shape[0]) > _lib.SPCONV_MAX_ROWS:
        raise ValueError("%s: %d rows are beyond the library's bounds" % (who, int(coords.shape[0])))
    _need_device(coords)
    return coords.detach().contiguous(), shape, batch_size


def subm_plan(coords, spatial_shape, batch_size, *, check=True):
    """The plan of ``SubMConv3d(k=3, padding=1)`` layers that share an ``indice_key``: ``coords`` is int ``[V, 4]``
    with columns (batch, z, y, x) and unique rows, as ``voxelization_idx`` returns it and ``SparseConvTensor`` takes it.
    ``neighbours[k, r]`` is the row at ``p_r + d_k`` (``k = (dz + 1) 9 + (dy + 1) 3 + (dx + 1)``) in the same sample and
    inside the grid, or -1.  The call only enqueues; ``check=True`` adds ONE host read of the status word: a duplicate
    row, a coordinate outside ``spatial_shape`` and a batch index outside ``[0, batch_size)`` are a ``GaproError``."""
    who = "subm_plan"
    coords, shape, batch_size = _plan_args(who, coords, spatial_shape, batch_size, check)
    V, dev = int(coords.shape[0]), coords.device
    plan = SparseConvPlan(kind="subm", device=dev, n_in=V, n_out=V, batch_size=batch_size, in_shape=shape,
                          spatial_shape=shape, coords=coords,
                          neighbours=torch.empty((27, V), dtype=torch.int32, device=dev))
    if V == 0:
        return plan
    ctx, stream = _ctx_stream(coords)
    lib = ctx.lib
    h_shape = (C.c_int32 * 3)(*shape)
    with torch.cuda.device(dev):
        ws = _workspace(who, int(lib.gapro_spconv_subm_plan_workspace_bytes(V)), dev, "%d rows are" % V)
        d_status, h_status = _status_pair(dev, _lib.SPCONV_STATUS_WORDS, torch.int32, read=check)
        ctx.check(lib.gapro_spconv_subm_plan(ctx.handle, stream, V, coords.data_ptr(),
                                             int(coords.dtype == torch.int64), h_shape, batch_size, ws.data_ptr(),
                                             ws.numel(), plan.neighbours.data_ptr(), d_status.data_ptr(),
                                             _ptr(h_status)))
        if h_status is not None:  # the call's host read of its status, asked for by check=True
            status, flags = _host_read(dev, h_status)[:2]
            _refuse(who, status, flags, _SPCONV_CAUSES)
    return plan


def downsample_plan(coords, spatial_shape, batch_size, *, check=True):
    """The plan of ``SparseConv3d(k=2, stride=2)`` and of the ``SparseInverseConv3d(k=2)`` on the same ``indice_key``.
    The coarse voxel of a row is ``(b, z >> 1, y >> 1, x >> 1)``; a row in the last slice of an odd extent is in none
    (``parent = -1``).  COARSE ROWS ARE NUMBERED BY THEIR FIRST CHILD IN ASCENDING INPUT ROW.  ``.coords`` (int32
    ``[n_out, 4]``), ``.spatial_shape`` (``(D - 2) // 2 + 1`` per axis) and ``.n_out`` describe the coarse level.  One
    host read (the header: status and ``n_out``); with ``check=True`` a duplicate row, a coordinate outside
    ``spatial_shape`` and a batch index outside ``[0, batch_size)`` are a ``GaproError``, with ``check=False`` such rows
    simply have no pairs."""
    who = "downsample_plan"
    coords, shape, batch_size = _plan_args(who, coords, spatial_shape, batch_size, check)
    V, dev = int(coords.shape[0]), coords.device
    out_shape = tuple((d - 2) // 2 + 1 if d >= 2 else 0 for d in shape)
    plan = SparseConvPlan(kind="down", device=dev, n_in=V, n_out=0, batch_size=batch_size, in_shape=shape,
                          spatial_shape=out_shape, parent=torch.empty(V, dtype=torch.int32, device=dev),
                          child_slot=torch.empty(V, dtype=torch.int32, device=dev))
    if V > 0:
        ctx, stream = _ctx_stream(coords)
        lib = ctx.lib
        h_shape = (C.c_int32 * 3)(*shape)
        i64 = int(coords.dtype == torch.int64)
        with torch.cuda.device(dev):
            ws = _workspace(who, int(lib.gapro_spconv_down_plan_workspace_bytes(V)), dev, "%d rows are" % V)
            d_hdr, h_hdr = _status_pair(dev, _lib.SPCONV_STATUS_WORDS, torch.int32)
            ctx.check(lib.gapro_spconv_down_count(ctx.handle, stream, V, coords.data_ptr(), i64, h_shape, batch_size,
                                                  ws.data_ptr(), ws.numel(), d_hdr.data_ptr(), h_hdr.data_ptr()))
            status, flags, n_out = _host_read(dev, h_hdr)[:3]  # the call's one host read
            if check:
                _refuse(who, status, flags, _SPCONV_CAUSES)
            plan.n_out = int(n_out)
            plan.coords = torch.empty((plan.n_out, 4), dtype=torch.int32, device=dev)
            plan.children = torch.empty((8, plan.n_out), dtype=torch.int32, device=dev)
            d_status, _ = _status_pair(dev, _lib.SPCONV_STATUS_WORDS, torch.int32, read=False)
            ctx.check(lib.gapro_spconv_down_fill(ctx.handle, stream, V, coords.data_ptr(), i64, h_shape, batch_size,
                                                 plan.n_out, ws.data_ptr(), ws.numel(), _ptr(plan.coords),
                                                 _ptr(plan.children), plan.parent.data_ptr(),
                                                 plan.child_slot.data_ptr(), d_status.data_ptr(), None))
    else:
        plan.coords = torch.empty((0, 4), dtype=torch.int32, device=dev)
        plan.children = torch.empty((8, 0), dtype=torch.int32, device=dev)
    return plan


# layer -> (plan kind, kernel edge, then per direction the table's (attribute, one-of attribute, reverse_k))
_SPCONV_LAYERS = {"subm": ("subm", 3, ("neighbours", None), ("neighbours", None, 1)),
                  "down": ("down", 2, ("children", None), ("parent", "child_slot", 0)),
                  "inverse": ("down", 2, ("parent", "child_slot"), ("children", None, 0))}


class _SparseConv(torch.autograd.Function):
    """The one autograd node of the three layers, which ``_sparse_conv`` calls with checked arguments: one gather-GEMM
    launch forward; backward the same kernel on the transposed table and the two stages of the weight gradient."""

    @staticmethod
    def forward(fctx, feats, weight, bias, plan, layer):
        _, _, fwd, _ = _SPCONV_LAYERS[layer]
        rows_in, rows_out = (plan.n_out, plan.n_in) if layer == "inverse" else (plan.n_in, plan.n_out)
        Co, Ci = int(weight.shape[0]), int(weight.shape[-1])
        K = weight.numel() // (Co * Ci)
        dev = feats.device
        feats, weight = feats.detach().contiguous(), weight.detach().contiguous()
        bias = None if bias is None else bias.detach().contiguous()
        fctx.plan, fctx.layer, fctx.dims, fctx.has_bias = plan, layer, (rows_out, rows_in, K, Ci, Co), bias is not None
        fctx.save_for_backward(feats, weight)
        out = torch.empty((rows_out, Co), dtype=torch.float32, device=dev)
        if rows_out == 0:
            return out
        if rows_in == 0:  # no coarse row: bias alone
            return out.zero_() if bias is None else out.copy_(bias.expand(rows_out, Co))
        ctx, stream = _ctx_stream(feats)
        with torch.cuda.device(dev):
            ctx.check(ctx.lib.gapro_spconv_forward(ctx.handle, stream, rows_out, rows_in, K,
                                                   getattr(plan, fwd[0]).data_ptr(),
                                                   _ptr(getattr(plan, fwd[1])) if fwd[1] else None, Ci, Co,
                                                   feats.data_ptr(), weight.data_ptr(), _ptr(bias), out.data_ptr()))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_out):
        feats, weight = fctx.saved_tensors
        plan, layer = fctx.plan, fctx.layer
        rows_out, rows_in, K, Ci, Co = fctx.dims
        _, _, fwd, bwd = _SPCONV_LAYERS[layer]
        need = fctx.needs_input_grad
        dev = feats.device
        grad_out = grad_out.to(dtype=torch.float32).contiguous()
        g_feats = torch.empty((rows_in, Ci), dtype=torch.float32, device=dev) if need[0] else None
        g_weight = torch.empty_like(weight) if need[1] else None
        g_bias = torch.empty(Co, dtype=torch.float32, device=dev) if fctx.has_bias and need[2] else None
        if rows_out == 0 or rows_in == 0:
            for g in (g_feats, g_weight):
                if g is not None:
                    g.zero_()
            if g_bias is not None:
                g_bias.copy_(grad_out.sum(0)) if rows_out else g_bias.zero_()
            return g_feats, g_weight, g_bias, None, None
        ctx, stream = _ctx_stream(feats)
        lib = ctx.lib
        with torch.cuda.device(dev):
            if g_feats is not None:
                ctx.check(lib.gapro_spconv_backward_input(ctx.handle, stream, rows_in, rows_out, K,
                                                          getattr(plan, bwd[0]).data_ptr(),
                                                          _ptr(getattr(plan, bwd[1])) if bwd[1] else None, bwd[2], Ci,
                                                          Co, grad_out.data_ptr(), weight.data_ptr(),
                                                          g_feats.data_ptr()))
            if g_weight is not None or g_bias is not None:
                ws = _workspace("sparse convolution", int(lib.gapro_spconv_workspace_bytes(rows_out, K, Ci, Co)), dev)
                ctx.check(lib.gapro_spconv_backward_weight(ctx.handle, stream, rows_out, rows_in, K,
                                                           getattr(plan, fwd[0]).data_ptr(),
                                                           _ptr(getattr(plan, fwd[1])) if fwd[1] else None, Ci, Co,
                                                           feats.data_ptr(), grad_out.data_ptr(), ws.data_ptr(),
                                                           ws.numel(), _ptr(g_weight), _ptr(g_bias)))
        return g_feats, g_weight, g_bias, None, None


def _sparse_conv(who, layer, feats, weight, plan, bias):
    kind, edge, _, _ = _SPCONV_LAYERS[layer]
    if not isinstance(plan, SparseConvPlan) or plan.kind != kind:
        raise ValueError("%s: plan must be the SparseConvPlan of %s" % (who, "subm_plan" if kind == "subm"
                                                                        else "downsample_plan"))
    rows = plan.n_out if layer == "inverse" else plan.n_in
    _float_arg(who, "feats", feats, ("V", "C_in"))
    if int(feats.shape[0]) != rows:
        raise ValueError("%s: feats has %d rows, the plan was built for %d" % (who, int(feats.shape[0]), rows))
    Ci = int(feats.shape[1])
    _float_arg(who, "weight", weight, ("C_out", edge, edge, edge, Ci))
    Co = int(weight.shape[0])
    if not 1 <= Ci <= _lib.SPCONV_MAX_CHANNELS or not 1 <= Co <= _lib.SPCONV_MAX_CHANNELS:
        raise ValueError("%s: 1 .. %d channels are built; C_in = %d, C_out = %d"
                         % (who, _lib.SPCONV_MAX_CHANNELS, Ci, Co))
    if bias is not None:
        _float_arg(who, "bias", bias, (Co,))
    tensors = tuple(t for t in (feats, weight, bias) if t is not None)
    _one_device(who, plan.device, tensors)
    _need_device(*tensors)
    cast = [t if t is None or t.dtype == torch.float32 else t.to(torch.float32) for t in (feats, weight, bias)]
    out = _SparseConv.apply(cast[0], cast[1], cast[2], plan, layer)
    return out if feats.dtype == torch.float32 else out.to(feats.dtype)


def subm_conv3d(feats, weight, plan, bias=None):
    """``spconv.SubMConv3d(C_in, C_out, kernel_size=3, padding=1)`` as a function: ``feats`` ``[V, C_in]`` in the row
    order of the plan's ``coords``, ``weight`` ``[C_out, 3, 3, 3, C_in]`` (spconv 2.x's layout), ``bias`` ``[C_out]`` or
    ``None``; returns ``[V, C_out]`` on the same rows.  ``y[r] = bias + sum_d W[:, d + 1, :] x[row(b_r, p_r + d)]``: the
    dense cross-correlation ``conv3d(padding=1)`` read at the active sites.  Float64 inside, one rounding; float32, half
    or bfloat16 tensors are computed from their float32 values and the result is cast back.  Differentiable in
    ``feats``, ``weight`` and ``bias``.  A plan of another kind or row count is a ``ValueError``."""
    return _sparse_conv("subm_conv3d", "subm", feats, weight, plan, bias)


def sparse_conv3d(feats, weight, plan, bias=None):
    """``spconv.SparseConv3d(C_in, C_out, kernel_size=2, stride=2)`` on a ``downsample_plan``: ``feats`` ``[plan.n_in,
    C_in]``, ``weight`` ``[C_out, 2, 2, 2, C_in]``; returns ``[plan.n_out, C_out]`` on the rows of ``plan.coords``.
    ``y[q] = bias + sum over the children of q of W[:, p_child & 1, :] x[child]``."""
    return _sparse_conv("sparse_conv3d", "down", feats, weight, plan, bias)


def sparse_inverse_conv3d(feats, weight, plan, bias=None):
    """``spconv.SparseInverseConv3d(C_in, C_out, kernel_size=2)`` on the ``downsample_plan`` of the strided layer it
    undoes: ``feats`` ``[plan.n_out, C_in]`` on the coarse rows, ``weight`` ``[C_out, 2, 2, 2, C_in]``; returns
    ``[plan.n_in, C_out]`` on the strided layer's input rows.  ``y[i] = bias + W[:, p_i & 1, :] x[parent(i)]``; a row
    without a parent gets ``bias`` alone."""
    return _sparse_conv("sparse_inverse_conv3d", "inverse", feats, weight, plan, bias)
