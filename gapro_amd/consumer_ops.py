"""Consumer-side label ops on the GPU: the first thing ISBNet / SPFormer do with
the pseudo labels this package generates.  Same semantics as the reference lines cited per function; the work is
done by gapro_amd/csrc/consumer.hip behind the C ABI; the losses are ``torch.autograd.Function``s whose backward
uses the gradients the forward launch already produced.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from ._lib import Context, GaproError


def _ctx_stream(t):
    if not t.is_cuda:
        raise RuntimeError("gapro_amd.consumer_ops works on HIP device tensors; there is no CPU fallback")
    ctx = Context.get(t.device.index or 0)
    return ctx, C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


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
    if not isinstance(coords_float, torch.Tensor) or coords_float.dim() != 2 or coords_float.shape[1] != 3 \
            or coords_float.dtype != torch.float32:
        raise ValueError("%s: coords_float must be a float32 tensor of shape [V, 3]" % who)
    _label_code(instance_labels, who + ": instance_labels")
    _label_code(semantic_labels, who + ": semantic_labels")
    v = int(coords_float.shape[0])
    if int(instance_labels.shape[0]) != v or int(semantic_labels.shape[0]) != v:
        raise ValueError("%s: %d points, %d instance labels, %d semantic labels"
                         % (who, v, int(instance_labels.shape[0]), int(semantic_labels.shape[0])))
    if v == 0:
        raise ValueError("%s: no points" % who)
    if not (coords_float.is_cuda and instance_labels.is_cuda and semantic_labels.is_cuda):
        raise RuntimeError("gapro_amd.consumer_ops works on HIP device tensors; there is no CPU fallback")


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
            ws_bytes = int(lib.gapro_inst_prep_workspace_bytes(cap))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            d_hdr = torch.empty(C.sizeof(_lib.InstPrepHeader), dtype=torch.uint8, device=dev)
            h_hdr = torch.empty(C.sizeof(_lib.InstPrepHeader), dtype=torch.uint8, pin_memory=True)
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
            torch.cuda.current_stream(dev).synchronize()  # the call's one host read
            hdr = _lib.InstPrepHeader.from_buffer_copy(h_hdr.numpy().tobytes())
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
_SPP_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)
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
    if isinstance(batch_size, bool) or not isinstance(batch_size, int):
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
    if not (labels.is_cuda and cls.is_cuda and box.is_cuda and (gather is None or gather.is_cuda)
            and (spps is None or spps.is_cuda)):
        raise RuntimeError("gapro_amd.consumer_ops works on HIP device tensors; there is no CPU fallback")
    ctx, stream = _ctx_stream(labels)
    lib, dev = ctx.lib, labels.device
    labels, cls, box = labels.contiguous(), cls.contiguous(), box.contiguous()
    off = offsets.to(device=dev, dtype=torch.int64).contiguous()
    if gather is not None:
        gather = gather.to(dtype=torch.int64).contiguous()
    spp_i64 = 0
    if spps is not None:
        if spps.dtype not in (torch.int32, torch.int64):
            spps = spps.to(torch.int32)
        spps = spps.contiguous()
        spp_i64 = int(spps.dtype == torch.int64)
    n = int(gather.shape[0]) if gather is not None else int(labels.shape[0])
    n_cls = int(cls.shape[0])
    hdr_bytes = C.sizeof(_lib.SppGtHeader) + 8 * batch_size
    with torch.cuda.device(dev):
        ws_bytes = int(lib.gapro_spp_gt_workspace_bytes(n, batch_size, n_cls, n_spps))
        if ws_bytes == 0:
            raise ValueError("%s: %d points, batch_size %d and %d superpoint ids are beyond the library's bounds"
                             % (who, n, batch_size, n_spps))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        d_hdr = torch.empty(hdr_bytes, dtype=torch.uint8, device=dev)
        h_hdr = torch.empty(hdr_bytes, dtype=torch.uint8, pin_memory=True)
        common = (n, int(labels.shape[0]), labels.data_ptr(), _LABEL_CODES[labels.dtype],
                  gather.data_ptr() if gather is not None else None, spps.data_ptr() if spps is not None else None,
                  spp_i64, n_spps, cls.data_ptr(), _LABEL_CODES[cls.dtype], n_cls)
        ctx.check(lib.gapro_spp_gt_count(ctx.handle, stream, *common, off.data_ptr(), batch_size, int(ignore_label),
                                         ws.data_ptr(), ws_bytes, d_hdr.data_ptr(), h_hdr.data_ptr()))
        torch.cuda.current_stream(dev).synchronize()  # the call's one host read
        raw = h_hdr.numpy().tobytes()
        hdr = _lib.SppGtHeader.from_buffer_copy(raw)
        if hdr.status != 0:
            why = next(text for bit, text in _GT_CAUSES if hdr.flags & bit)
            raise GaproError(hdr.status, "%s: sample %d: %s" % (who, hdr.bad_sample, why))
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
                                        out_cls.data_ptr(), out_box.data_ptr(),
                                        out_ids.data_ptr() if return_ids else None, rows, None))
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
    if not isinstance(spps, torch.Tensor) or spps.dim() != 1 or spps.dtype not in _SPP_DTYPES:
        raise ValueError("%s: spps must be a 1-D integer tensor" % who)
    if int(spps.shape[0]) != int(instance_labels.shape[0]):
        raise ValueError("%s: %d labels, %d superpoint ids" % (who, int(instance_labels.shape[0]), int(spps.shape[0])))
    off = _offsets_arg(batch_offsets, batch_size, who)
    if n_spps is not None and (isinstance(n_spps, bool) or not isinstance(n_spps, int) or n_spps < 1):
        raise ValueError("%s: n_spps must be a positive int" % who)
    if not spps.is_cuda:
        raise RuntimeError("gapro_amd.consumer_ops works on HIP device tensors; there is no CPU fallback")
    if n_spps is None:
        n_spps = max(int(spps.max()) + 1, 1)  # a host read; a negative id is refused by the device below
    return _gt_run(who, instance_labels, None, spps, n_spps, instance_cls, instance_box, off, batch_size, ignore_label,
                   _lib.SPP_GT_STRICT if strict else _lib.SPP_GT_HALF, return_ids)


def get_subsample_gt(instance_labels, subsample_idxs, instance_cls, instance_box, subsample_batch_offsets, batch_size,
                     ignore_label=-100, *, return_ids=False):
    """``get_subsample_gt`` (ISBNet/isbnet/model/model_utils.py:647-689, isbnet.py:399-401): the rows of ``get_spp_gt``
    over the sample's subsampled points, ``mask[i, p] = (instance_labels[subsample_idxs[p]] == id_i)`` for the ``p`` of
    ``[subsample_batch_offsets[b], subsample_batch_offsets[b + 1])``.  Same return, refusals and single host read."""
    who = "get_subsample_gt"
    _check_gt_args(who, instance_labels, instance_cls, instance_box, batch_size)
    if not isinstance(subsample_idxs, torch.Tensor) or subsample_idxs.dim() != 1 \
            or subsample_idxs.dtype not in _SPP_DTYPES:
        raise ValueError("%s: subsample_idxs must be a 1-D integer tensor" % who)
    if int(subsample_idxs.shape[0]) == 0:
        raise ValueError("%s: no points" % who)
    off = _offsets_arg(subsample_batch_offsets, batch_size, who)
    return _gt_run(who, instance_labels, subsample_idxs, None, 0, instance_cls, instance_box, off, batch_size,
                   ignore_label, _lib.SPP_GT_HALF, return_ids)
