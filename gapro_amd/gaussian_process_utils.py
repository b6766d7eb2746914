"""Same-name mirror of reference gapro/gaussian_process_utils.py for its two single-model fitters.

``fit_gp_spp`` (the generator's fitter, on pooled superpoint features) keeps the reference signature
(gaussian_process_utils.py:382) and return order (:445):
(pred_probs f32[T], pred_probs_new f32[T], pred_labels bool[T], pred_mu f32[T], pred_variance f32[T]).
``fit_gp`` (:28-116) is the point-level fitter: point index sets in, the training set assembled on the device, every
intersection point predicted from its own feature row; it returns (pred_probs, pred_probs_new, pred_labels,
pred_variance) with the Bernoulli variance p (1 - p).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import FitDesc, GaproError
from .fit_runner import _host, pack_point_problems
from .gen_ps_utils import _pick_device, _pipeline
from .gp_model import GPModel, load_models, save_models  # noqa: F401  (re-exported: the models of return_models=True)


def fit_gp_spp_batch(feats_spp, problems, training_iter=50, init_mean=None, device=None, keep_debug=False,
                     return_status=False, reproducibility_probe=False, return_models=False, **pipe_kw):
    """Fit many independent GPs in one launch.

    feats_spp  f32[S,D] (torch or numpy); problems = list of (b1_inds, b2_inds, intersect_inds).
    init_mean  optional list of per-problem initial variational means (length m1+m2 each).
    Returns a list of 5-tuples of numpy arrays in the reference's order, plus (if keep_debug) the raw
    result dict as a second value.  A fit that fails (non-finite input, K_ZZ not positive definite after the
    jitter retries of gpytorch's psd_safe_cholesky) raises GaproError, as gpytorch raises there; with
    ``return_status=True`` nothing is raised and the per-fit gapro_status array (0 = ok) comes back as the last
    value: a failed fit does not affect the other fits of the launch.
    The raw result dict carries ``cond``, a per-fit conditioning figure of the last Cholesky factor (a diagnostic), and
    with ``reproducibility_probe=True`` (implies keep_debug; twice the work) ``repro_dv`` / ``repro_dp``: how far each
    fit's sigma^2 (relative) and p (absolute) move when the jitter on K_ZZ is scaled by (1 + 1e-11) -- beyond
    fit_runner.REPRO_SOFT (1e-5) a fit's variances are reproducible by no float64 implementation to 1e-4.
    With ``return_models=True`` one more value follows the list of outputs: the list of trained ``GPModel`` (one per
    problem; predict_gp_batch evaluates them at other inputs).  The other results are the same bits either way.
    """
    dev = _pick_device(feats_spp, device)
    pipe = _pipeline(dev, training_iter, **pipe_kw)
    f = feats_spp if isinstance(feats_spp, torch.Tensor) else torch.from_numpy(np.asarray(feats_spp))
    f = f.to(device=dev, dtype=torch.float32).contiguous()
    n = len(problems)
    descs = (FitDesc * max(n, 1))()
    idx, init = [], []
    io = oo = 0
    for i, (b1, b2, it) in enumerate(problems):
        b1 = np.asarray(b1.cpu() if isinstance(b1, torch.Tensor) else b1, dtype=np.int32).reshape(-1)
        b2 = np.asarray(b2.cpu() if isinstance(b2, torch.Tensor) else b2, dtype=np.int32).reshape(-1)
        it = np.asarray(it.cpu() if isinstance(it, torch.Tensor) else it, dtype=np.int32).reshape(-1)
        if len(b1) == 0 or len(b2) == 0:
            raise ValueError("fit_gp_spp needs at least one superpoint on each side")
        d = descs[i]
        d.m1, d.m2, d.t, d.b1, d.b2, d.scene = len(b1), len(b2), len(it), 0, 1, i
        d.idx_offset, d.out_offset, d.ws_offset = io, oo, 0
        idx += [b1, b2, it]
        if init_mean is not None:
            im = np.zeros(len(b1) + len(b2) + len(it))
            im[:len(b1) + len(b2)] = np.asarray(init_mean[i], dtype=np.float64)
            init.append(im)
        io += len(b1) + len(b2) + len(it)
        oo += len(it)
    h_idx = np.ascontiguousarray(np.concatenate(idx)) if idx else np.zeros(1, np.int32)
    h_init = np.concatenate(init) if init else None
    keep_debug = keep_debug or reproducibility_probe
    res = pipe.fit_descs(f, descs, n, h_idx, oo, init_mean=h_init, keep_debug=keep_debug,
                         raise_on_failure=not return_status, keep_models=return_models)
    if reproducibility_probe:
        res["repro_dv"], res["repro_dp"] = pipe.reproducibility_probe(f, descs, n, h_idx, oo, res=res, init_mean=h_init)
    outs = []
    for i in range(n):
        a, b = descs[i].out_offset, descs[i].out_offset + descs[i].t
        outs.append((res["probs"][a:b], res["probs_new"][a:b], res["labels"][a:b].astype(bool), res["mu"][a:b],
                     res["var"][a:b]))
    ret = (outs,) + ((res["models"][:n],) if return_models else ()) + ((res,) if keep_debug else ()) + \
        ((res["status"],) if return_status else ())
    return ret if len(ret) > 1 else outs


def predict_gp_batch(models, feats, rows, device=None, return_status=False, **pipe_kw):
    """Posterior of trained models at other inputs: model i at ``feats[rows[i]]``.

    models  list of GPModel (fit_gp_spp_batch(..., return_models=True), GPModel.load, ...);
    feats   f32[R, D] torch or NumPy -- pooled superpoint features or per-point features alike;
    rows    one index vector per model (any order, repeats allowed, may be empty).
    Returns, per model, the reference's 5-tuple (pred_probs f32[T], pred_probs_new f32[T], pred_labels bool[T],
    pred_mu f32[T], pred_variance f32[T]) as NumPy arrays, like fit_gp_spp_batch.  K_ZZ is factored afresh from the
    model (psd_safe_cholesky's retry rule) with the model's own variational jitter.  A feature width that differs
    from a model's, a model of a failed fit, or non-finite features raise ValueError / GaproError; with
    ``return_status=True`` nothing is raised for them, the per-model gapro_status array is the last value and the
    other models' results are intact.
    """
    models = list(models)
    D = int(feats.shape[1]) if getattr(feats, "ndim", 0) == 2 else -1
    if D < 0:
        raise ValueError("predict_gp_batch: feats must be [R, D]")
    if not return_status:  # before a device is touched
        for i, mo in enumerate(models):
            if mo.d != D:
                raise ValueError("predict_gp_batch: model %d was trained at feature width %d, the features have %d"
                                 % (i, mo.d, D))
    if len(rows) != len(models):
        raise ValueError("predict_gp_batch: %d models but %d row vectors" % (len(models), len(rows)))
    dev = _pick_device(feats, device)
    pipe = _pipeline(dev, 50, **pipe_kw)
    f = feats if isinstance(feats, torch.Tensor) else torch.from_numpy(np.asarray(feats))
    f = f.to(device=dev, dtype=torch.float32).contiguous()
    rows = [r.cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r) for r in rows]
    res = pipe.predict_models(models, f, rows, raise_on_failure=not return_status)
    outs, off = [], res["offsets"]
    for i in range(len(models)):
        a, b = int(off[i]), int(off[i + 1])
        outs.append((res["probs"][a:b], res["probs_new"][a:b], res["labels"][a:b].astype(bool), res["mu"][a:b],
                     res["var"][a:b]))
    return (outs, res["status"]) if return_status else outs


def fit_gp_spp(coords_float_spp, feats_spp, b1_inds, b2_inds, intersect_inds, training_iter=50, *,
               init_mean=None, device=None, **pipe_kw):
    """Reference gaussian_process_utils.py:382-445.  ``coords_float_spp`` is accepted and unused, as in
    the reference.  Returns torch tensors on the device of ``feats_spp``."""
    dev = _pick_device(feats_spp, device)
    out = fit_gp_spp_batch(feats_spp, [(b1_inds, b2_inds, intersect_inds)], training_iter,
                           init_mean=None if init_mean is None else [init_mean], device=dev, **pipe_kw)[0]
    keep_cpu = isinstance(feats_spp, torch.Tensor) and not feats_spp.is_cuda
    tens = tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)
    return tens if keep_cpu else tuple(t.to(dev) for t in tens)


# ---------------------------------------------------------------------- point-level fits (reference :28-116)
def _n_points(coords_float, feats, spp):
    shp = tuple(getattr(feats, "shape", ()))
    if len(shp) != 2:
        raise ValueError("feats must be [N, D]")
    if tuple(coords_float.shape) != (shp[0], 3) or len(spp) != shp[0]:
        raise ValueError("coords_float must be [N, 3], feats [N, D] and spp [N] for one N")
    return int(shp[0])


def gp_train_sets(coords_float, feats, spp, problems, npoint_nearest=800, spp_pool=True, device=None, **pipe_kw):
    """The training sets ``fit_gp_batch`` fits, assembled on the device (assembly only).

    problems = list of (b1_inds, b2_inds, intersect_inds), POINT indices in any order (an index listed twice counts
    twice).  Returns, per problem, ``(train_x f32[M, D], m1, m2, sel1, sel2)``: side 1's rows (label -1), then side
    2's (+1).  ``spp_pool=True``: a side's rows are its distinct superpoints in ascending id order, each the exact
    fixed-point mean of the side's points of that superpoint (``npoint_nearest`` is ignored); ``sel`` holds the ids.
    ``spp_pool=False``: a side of at most ``npoint_nearest`` (1 .. 1024) points is kept as given, a longer one keeps the
    points nearest to the centroid of the intersection's points, ordered by (distance, position in the list); ``sel``
    holds the chosen point indices.  DESIGN.md 4.4 has the arithmetic.  A problem that meets a non-finite coordinate
    or row raises GaproError (``fit_gp_batch(..., return_status=True)`` reports it per problem instead)."""
    n = _n_points(coords_float, feats, spp)
    descs, h_idx = pack_point_problems(problems, n, npoint_nearest, spp_pool)
    dev = _pick_device(feats, device)
    pipe = _pipeline(dev, 50, **pipe_kw)
    ts = pipe.train_sets(coords_float, feats, spp, descs, h_idx, npoint_nearest, spp_pool)
    status = _host(ts.status).copy()
    if (status != 0).any():
        bad = int(np.nonzero(status)[0][0])
        raise GaproError(int(status[bad]), "training set of problem %d of %d" % (bad, len(descs)))
    train, sel = _host(ts.train), _host(ts.sel)
    outs = []
    for d in descs:
        a, b, c = int(d.row_offset), int(d.row_offset + d.m1), int(d.row_offset + d.m1 + d.m2)
        outs.append((train[a:c].copy(), int(d.m1), int(d.m2), sel[a:b].copy(), sel[b:c].copy()))
    return outs


def fit_gp_batch(coords_float, feats, spp, problems, training_iter=50, npoint_nearest=800, spp_pool=True, device=None,
                 return_latent=False, return_models=False, return_status=False, **pipe_kw):
    """Point-level GP fits of many problems, on the device from the index sets to the predictions: the training sets
    of ``gp_train_sets``, one fit launch on them (zero initial variational mean, the default options, as
    ``fit_gp_spp``), one predict launch at ``feats[intersect_inds]`` from the trained states where the fit left them.

    Returns a list of 4-tuples of NumPy arrays, one per problem: (pred_probs f32[T], pred_probs_new f32[T],
    pred_labels bool[T], pred_variance f32[T]) with pred_variance = p (1 - p) in float32 (the Bernoulli variance,
    reference :112); ``return_latent`` appends the latent mean and variance (6-tuples).  Then, as in
    ``fit_gp_spp_batch``: with ``return_models`` the list of trained GPModel, with ``return_status`` the per-problem
    gapro_status array (nothing is raised; a failed problem does not affect the others)."""
    n = _n_points(coords_float, feats, spp)
    descs, h_idx = pack_point_problems(problems, n, npoint_nearest, spp_pool)
    dev = _pick_device(feats, device)
    pipe = _pipeline(dev, training_iter, **pipe_kw)
    res = pipe.fit_points(coords_float, feats, spp, descs, h_idx, npoint_nearest, spp_pool, keep_models=return_models,
                          raise_on_failure=not return_status)
    outs, off = [], res["offsets"]
    for i in range(len(descs)):
        a, b = int(off[i]), int(off[i + 1])
        p = res["probs"][a:b]
        tup = (p, res["probs_new"][a:b], res["labels"][a:b].astype(bool), p * (np.float32(1.0) - p))
        outs.append(tup + ((res["mu"][a:b], res["var"][a:b]) if return_latent else ()))
    ret = (outs,) + ((res["models"],) if return_models else ()) + ((res["status"],) if return_status else ())
    return ret if len(ret) > 1 else outs


def fit_gp(coords_float, feats, spp, b1_inds, b2_inds, intersect_inds, training_iter=50, npoint_nearest=800,
           spp_pool=True, *, device=None, **pipe_kw):
    """Reference gaussian_process_utils.py:28-116: (pred_probs f32[T], pred_probs_new f32[T], pred_labels bool[T],
    pred_variance f32[T]) as torch tensors on the device of ``feats``."""
    out = fit_gp_batch(coords_float, feats, spp, [(b1_inds, b2_inds, intersect_inds)], training_iter, npoint_nearest,
                       spp_pool, device=device, **pipe_kw)[0]
    dev = _pick_device(feats, device)
    keep_cpu = isinstance(feats, torch.Tensor) and not feats.is_cuda
    tens = tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)
    return tens if keep_cpu else tuple(t.to(dev) for t in tens)
