"""A trained GP of the batched fit as plain NumPy arrays: what gapro_svgp_fit_batch_state exports per fit.

State layout (include/gapro_hip.h): 8 header doubles [M, D, status, jitter, c, rho_s, rho_l, 0], then Z f64[M, D],
the variational mean f64[M] and tril(L_S) f64[M, M] row-major.  The layout depends on (M, D) only.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

STATE_HEADER = 8


def state_doubles(m: int, d: int) -> int:
    return STATE_HEADER + m * d + m + m * m


def _softplus(x: float) -> float:
    return float(np.log1p(np.exp(-abs(x))) + max(x, 0.0))


class GPModel:
    """Whitened SVGP classifier after training: inducing points ``Z`` f64[M, D], variational mean ``mean`` f64[M],
    ``LS`` = tril(L_S) f64[M, M], constant mean ``c``, raw output scale ``rho_s`` and length scale ``rho_l`` (the kernel
    uses their softplus: ``outputscale`` / ``lengthscale``), the variational ``jitter`` it was trained with and the
    ``status`` of its fit (0 = ok)."""

    __slots__ = ("Z", "mean", "LS", "c", "rho_s", "rho_l", "jitter", "status")

    def __init__(self, Z, mean, LS, c, rho_s, rho_l, jitter, status=0):
        self.Z = np.ascontiguousarray(Z, dtype=np.float64)
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.LS = np.ascontiguousarray(LS, dtype=np.float64)
        if self.Z.ndim != 2 or self.mean.shape != (self.Z.shape[0],) or self.LS.shape != (self.Z.shape[0],) * 2:
            raise ValueError("GPModel: Z [M, D], mean [M] and LS [M, M] do not agree")
        self.c, self.rho_s, self.rho_l = float(c), float(rho_s), float(rho_l)
        self.jitter, self.status = float(jitter), int(status)

    @property
    def m(self) -> int:
        return int(self.Z.shape[0])

    @property
    def d(self) -> int:
        return int(self.Z.shape[1])

    @property
    def outputscale(self) -> float:
        return _softplus(self.rho_s)

    @property
    def lengthscale(self) -> float:
        return _softplus(self.rho_l)

    # ---- the exported state -------------------------------------------------------------------------------------
    @classmethod
    def from_state(cls, state: np.ndarray) -> "GPModel":
        """One model from its state vector (float64; a copy is taken)."""
        m, d = int(state[0]), int(state[1])
        if m <= 0 or d <= 0 or len(state) < state_doubles(m, d):
            raise ValueError("GPModel.from_state: not a model state (M = %d, D = %d, %d doubles)" % (m, d, len(state)))
        o = STATE_HEADER
        Z = state[o:o + m * d].reshape(m, d).copy()
        mean = state[o + m * d:o + m * d + m].copy()
        LS = state[o + m * d + m:o + m * d + m + m * m].reshape(m, m).copy()
        return cls(Z, mean, LS, state[4], state[5], state[6], state[3], int(state[2]))

    def to_state(self) -> np.ndarray:
        m, d = self.m, self.d
        out = np.empty(state_doubles(m, d))
        out[:STATE_HEADER] = [m, d, self.status, self.jitter, self.c, self.rho_s, self.rho_l, 0.0]
        o = STATE_HEADER
        out[o:o + m * d] = self.Z.reshape(-1)
        out[o + m * d:o + m * d + m] = self.mean
        out[o + m * d + m:] = np.tril(self.LS).reshape(-1)
        return out

    # ---- files --------------------------------------------------------------------------------------------------
    def save(self, path):
        """One model as .npz (NumPy arrays only)."""
        save_models(path, [self])

    @classmethod
    def load(cls, path) -> "GPModel":
        models = load_models(path)
        if len(models) != 1:
            raise ValueError("GPModel.load: %s holds %d models; use load_models" % (path, len(models)))
        return models[0]

    save_list = staticmethod(lambda path, models: save_models(path, models))
    load_list = staticmethod(lambda path: load_models(path))


def save_models(path, models):
    """Many models in one .npz: their states back to back plus the offsets (bit-exact round trip)."""
    states = [m.to_state() for m in models]
    offsets = np.zeros(len(states) + 1, dtype=np.int64)
    if states:
        offsets[1:] = np.cumsum([len(s) for s in states])
    flat = np.concatenate(states) if states else np.zeros(0)
    with open(path, "wb") as fh:  # (a file object: np.savez would append ".npz" to a bare name)
        np.savez(fh, gapro_gp_models=np.int64(1), offsets=offsets, states=flat)


def load_models(path):
    with np.load(path) as z:
        if "gapro_gp_models" not in z:
            raise ValueError("%s is not a GPModel file" % (path,))
        offsets, flat = z["offsets"], z["states"]
    return [GPModel.from_state(flat[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])]


class SceneFit(namedtuple("SceneFit", "b1 b2 train test model")):
    """One GP fit of a scene (Pipeline.run(..., keep_models=True)): the two boxes, the training superpoint ranks
    [b1_inds | b2_inds], the test superpoint ranks (intersect_inds) and the trained GPModel.  A 5-tuple; ``m1`` says
    where the training ranks split (the first m1 belong to box b1, label -1)."""

    def __new__(cls, b1, b2, train, test, model, m1):
        self = super().__new__(cls, b1, b2, train, test, model)
        self.m1 = int(m1)
        return self
