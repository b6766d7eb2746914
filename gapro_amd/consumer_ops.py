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
