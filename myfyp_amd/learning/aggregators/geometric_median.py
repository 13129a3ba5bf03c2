"""Geometric median (RFA: Pillutla et al., 2019, smoothed Weiszfeld): robust aggregation for the
FYP Byzantine harness that needs no bound on the attackers, honours sample weights and
down-weights an outlier instead of gating it. Not in the reference."""

from __future__ import annotations

from typing import List, Sequence

import numpy as np

from myfyp_amd.learning.aggregators._math import _is_torch, flatten
from myfyp_amd.learning.aggregators.aggregator import Aggregator, NoModelsToAggregateError
from myfyp_amd.learning.frameworks.p2pfl_model import P2PFLModel

MAX_ITERS = 32


def geometric_median_numpy(rows: Sequence[np.ndarray], weights: Sequence[float], iters: int = 3, nu: float = 1e-6):
    """``ops.geometric_median_into``'s definition over float64 numpy rows: ``(out, coef float32,
    dist float64, objective float64)``."""
    k = len(rows)
    iters = int(iters)
    if len(weights) != k:
        raise ValueError(f"{k} rows but {len(weights)} weights")
    if not 1 <= iters <= MAX_ITERS:
        raise ValueError(f"iters must be in 1..{MAX_ITERS}, got {iters}")
    if not (nu > 0 and np.isfinite(nu)):
        raise ValueError(f"nu must be finite and > 0, got {nu}")
    w = np.asarray([float(x) for x in weights], dtype=np.float64)
    if not np.all((w >= 0) & np.isfinite(w)):
        raise ValueError("weights must be finite and >= 0")
    x = [np.asarray(r, dtype=np.float64).ravel() for r in rows]
    with np.errstate(all="ignore"):
        valid = np.isfinite(np.array([(xi * xi).sum() for xi in x]).astype(np.float32))
        dist = np.full(k, np.nan)
        obj = np.zeros(iters)
        if not valid.any():
            coef = (w / w.sum() if w.sum() > 0 else np.full(k, 1.0 / k)).astype(np.float32)
            iters = 0
        else:
            what = np.where(valid, w, 0.0)
            if what.sum() == 0:
                what = valid.astype(np.float64)
            coef = (what / what.sum()).astype(np.float32)
        for t in range(iters):
            c = coef.astype(np.float64)
            nz = [j for j in range(k) if c[j] != 0]
            xr = x[nz[0]]
            m = np.zeros_like(xr)
            for j in nz:
                m += c[j] * (x[j] - xr)
            dist = np.array([np.sqrt((((xi - xr) - m) ** 2).sum()) for xi in x])
            live = what != 0
            obj[t] = (what[live] * dist[live]).sum()
            beta = np.where(np.isfinite(dist), what / np.maximum(dist, nu), 0.0)
            bs = beta.sum()
            if bs > 0 and np.isfinite(bs):
                coef = (beta / bs).astype(np.float32)
        out = np.zeros_like(x[0])
        for j in range(k):
            if coef[j] != 0:
                out += float(coef[j]) * x[j]
    return out, coef, dist, obj


class GeometricMedian(Aggregator):
    """The point that minimises the sample-weighted sum of distances to the models, by ``iters``
    smoothed Weiszfeld steps from the weighted mean; a model with NaN or Inf gets weight 0."""

    collective_kind = "geometric_median"

    def __init__(self, node_name: str = "unknown", iters: int = 3, nu: float = 1e-6) -> None:
        super().__init__(node_name)
        if not 1 <= int(iters) <= MAX_ITERS:
            raise ValueError(f"iters must be in 1..{MAX_ITERS}, got {iters}")
        self.iters = int(iters)
        self.nu = float(nu)
        self.partial_aggregation = False
        # set after an aggregation: (trainer addresses in row order, coef); after a device
        # aggregation coef is the device tensor, and reading it synchronises
        self.last_weights = None

    def aggregate(self, models: List[P2PFLModel]) -> P2PFLModel:
        if not models:
            raise NoModelsToAggregateError(f"({self.node_name}) Trying to aggregate models when there is no models")
        params = [m.get_parameters() for m in models]
        flats = [flatten(p) for p in params]
        ws = [float(m.get_num_samples()) for m in models]
        if _is_torch(flats[0]):
            import torch

            from myfyp_amd import ops

            out = torch.empty_like(flats[0])
            coef, _, _ = ops.geometric_median_into([f_.contiguous() for f_ in flats], [out], ws, self.iters, self.nu)
            pieces, at = [], 0
            for p in params[0]:
                pieces.append(out[at : at + p.numel()].view_as(p).to(p.dtype))
                at += p.numel()
        else:
            out, coef, _, _ = geometric_median_numpy(flats, ws, self.iters, self.nu)
            pieces, at = [], 0
            for p in params[0]:
                p = np.asarray(p)
                pieces.append(out[at : at + p.size].reshape(p.shape).astype(p.dtype))
                at += p.size
        contributors: List[str] = []
        for m in models:
            contributors += m.get_contributors()
        self.last_weights = ([(m.get_contributors() or [None])[0] for m in models], coef)
        return models[0].build_copy(params=pieces, num_samples=sum(m.get_num_samples() for m in models), contributors=contributors)
