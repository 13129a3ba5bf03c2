"""Divide-and-Conquer (DnC; Shejwalkar & Houmansadr, NDSS 2021): the spectral defence the min-max
and min-sum attacks of the Byzantine harness were designed against. Krum, the geometric median,
Bulyan's first stage and ClippedGossip judge a model by its L2 distance, the median and the trimmed
mean coordinate by coordinate; μ − γσ attacks stay inside the honest models' distance envelope.
Colluding models all shift along one common direction: it is the top singular direction of the
centred model matrix, and DnC drops the models with the largest projection on it. With K <= 16
models the spectral step is a K × K problem: ⟨x_i − μ, v⟩² = λ·u_i², (λ, u) the top eigenpair of the
centred Gram matrix G = −½·J·D·J, D the squared distances, J = I − 11ᵀ/K. Not in the reference.

Deviations from the paper: the coordinates are subsampled per tile of 256 by a Bernoulli draw (plus
one forced tile), not as exactly ``subsample_dims`` coordinates; the subsample is a function of
``(seed, round, iteration)``, so every rank draws the same one. On the gossip plane ``round`` counts
the calls of :meth:`DnC.clear` from 0: a resumed run restarts the counter."""

from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from myfyp_amd.learning.aggregators._math import _is_torch, flatten
from myfyp_amd.learning.aggregators.aggregator import Aggregator, NoModelsToAggregateError
from myfyp_amd.learning.frameworks.p2pfl_model import P2PFLModel

DNC_MAX_ITERS = 8
DNC_TILE = 256
DNC_SQUARINGS = 20
_M64 = (1 << 64) - 1


def _sm64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def dnc_check(k: int, f, filter_frac, iters, subsample_dims) -> int:
    """``ops.dnc_check``: f an integer >= 0, filter_frac finite and >= 0, 1 <= iters <= 8,
    subsample_dims None or an integer >= 1, iters · m < K; returns m = ceil(filter_frac · f)."""
    if isinstance(f, bool) or int(f) != f or f < 0:
        raise ValueError(f"DnC: the attacker bound f must be an integer >= 0, got f = {f} (K = {k})")
    ff = float(filter_frac)
    if not math.isfinite(ff) or ff < 0:
        raise ValueError(f"DnC: filter_frac must be finite and >= 0, got {filter_frac}")
    if isinstance(iters, bool) or int(iters) != iters or not 1 <= iters <= DNC_MAX_ITERS:
        raise ValueError(f"DnC: iters must be an integer in [1, {DNC_MAX_ITERS}], got {iters}")
    if subsample_dims is not None and (isinstance(subsample_dims, bool) or int(subsample_dims) != subsample_dims or subsample_dims < 1):
        raise ValueError(f"DnC: subsample_dims must be None or an integer >= 1, got {subsample_dims}")
    m = int(math.ceil(ff * int(f)))
    if k < 1 or int(iters) * m >= k:
        raise ValueError(f"DnC needs iters · m < K models: K = {k}, iters = {iters}, m = ceil({filter_frac} · {f}) = {m}")
    return m


def dnc_coordinates(n: int, seed: int, round: int, t: int, subsample_dims: Optional[int]) -> np.ndarray:
    """Boolean mask [n] of the coordinates iteration ``t`` measures (``ops.dnc_tiles``' rule)."""
    if subsample_dims is None or n <= subsample_dims:
        return np.ones(n, dtype=bool)
    tiles = (n + DNC_TILE - 1) // DNC_TILE
    thr = min(_M64, (int(subsample_dims) << 64) // n)
    kt = _sm64(_sm64(_sm64(int(seed) & _M64) ^ (int(round) & _M64)) ^ t)
    forced = _sm64(kt ^ _M64) % tiles
    take = np.fromiter((_sm64(kt ^ tau) < thr or tau == forced for tau in range(tiles)), dtype=bool, count=tiles)
    return np.repeat(take, DNC_TILE)[:n]


def _dnc_scores(d: np.ndarray):
    """One iteration's ``(score [K], lam, screened [K] bool)`` from squared distances ``d [K, K]``."""
    k = d.shape[0]
    fin = np.isfinite(d) | np.eye(k, dtype=bool)
    scr = (~fin).sum(1) * 2 > k - 1
    for b in range(1, k):
        if not scr[b] and any(not scr[a] and not fin[a, b] for a in range(b)):
            scr[b] = True
    v = np.flatnonzero(~scr)
    score = np.where(scr, np.inf, 0.0)
    lam = 0.0
    if len(v) > 1:
        kv = len(v)
        j = np.eye(kv) - np.full((kv, kv), 1.0 / kv)
        g = -0.5 * (j @ d[np.ix_(v, v)] @ j)
        g = 0.5 * (g + g.T)
        tr = float(np.trace(g))
        if tr > 0.0:
            mm = g / tr
            for _ in range(DNC_SQUARINGS):
                mm = mm @ mm
                mm = mm / np.trace(mm)
            col = mm[:, int(np.argmax(np.diag(mm)))]
            u = col / np.linalg.norm(col)
            lam = float(u @ g @ u)
            score[v] = lam * u * u
    return score, lam, scr


def dnc_numpy(rows: Sequence[np.ndarray], weights: Sequence[float], f: int, filter_frac: float = 1.0, iters: int = 1,
              subsample_dims: Optional[int] = 10000, seed: int = 0, round: int = 0):
    """``ops.dnc_into``'s definition over numpy rows in float64, any K: ``(out float32, coef float32,
    removed int32, dist float64 [iters, K, K], score float64 [iters, K], lam float64 [iters])``."""
    k = len(rows)
    if len(weights) != k:
        raise ValueError(f"{k} rows but {len(weights)} weights")
    m = dnc_check(k, f, filter_frac, iters, subsample_dims)
    iters = int(iters)
    n = np.asarray(rows[0]).size
    if n < 1 or any(np.asarray(r).size != n for r in rows):
        raise ValueError(f"DnC: rows must share one length >= 1, got {[np.asarray(r).size for r in rows]}")
    with np.errstate(all="ignore"):
        x = np.stack([np.asarray(r, dtype=np.float64).ravel() for r in rows])
        dist = np.zeros((iters, k, k))
        score = np.zeros((iters, k))
        lam = np.zeros(iters)
        removed = np.full(k, -1, dtype=np.int32)
        for t in range(iters):
            xt = x[:, dnc_coordinates(n, seed, round, t, subsample_dims)]
            for i in range(k):
                for j in range(i + 1, k):
                    dist[t, i, j] = dist[t, j, i] = ((xt[i] - xt[j]) ** 2).sum()
            score[t], lam[t], scr = _dnc_scores(dist[t])
            order = sorted(range(k), key=lambda a: (-score[t, a], -a))  # highest first, the higher row among equals
            for a in range(k):
                if (scr[a] or a in order[:m]) and removed[a] < 0:
                    removed[a] = t
        w = np.asarray([float(v) for v in weights], dtype=np.float64)
        kept = removed < 0
        if not kept.any():
            kept = np.ones(k, dtype=bool)
        ws = w[kept].sum()
        coef = np.where(kept, w / ws if ws > 0 else 1.0 / kept.sum(), 0.0).astype(np.float32)
        out = np.zeros(n)
        for a in range(k):
            if coef[a] != 0:  # a row of coefficient 0 never enters the sum
                out += np.float64(coef[a]) * x[a]
    return out.astype(np.float32), coef, removed, dist, score, lam


class DnC(Aggregator):
    """``iters`` times, on a fresh coordinate subsample: the models' projections on the top singular
    direction of the centred model matrix, the ``ceil(filter_frac · num_byzantine)`` largest
    removed; then the sample-weighted mean of the models every iteration kept. Needs
    ``iters · ceil(filter_frac · num_byzantine) < K`` models."""

    collective_kind = "dnc"

    def __init__(self, node_name: str = "unknown", num_byzantine: int = 1, filter_frac: float = 1.0, iters: int = 1,
                 subsample_dims: Optional[int] = 10000, seed: int = 0) -> None:
        super().__init__(node_name)
        dnc_check(1 << 30, num_byzantine, filter_frac, iters, subsample_dims)  # everything but iters · m < K, which needs K
        self.f = int(num_byzantine)
        self.filter_frac = float(filter_frac)
        self.iters = int(iters)
        self.subsample_dims = None if subsample_dims is None else int(subsample_dims)
        self.seed = int(seed)
        # the round the subsample is drawn for: the collective plane sets it from the workflow's
        # round; on the gossip plane clear() counts it up from 0 (a resumed run restarts it)
        self.round = 0
        self.partial_aggregation = False
        # set after an aggregation: (trainer addresses in row order, coef); coef[i] == 0 means peer
        # i was removed. After a device aggregation coef is the device tensor: reading it synchronises.
        self.last_selection = None

    def clear(self) -> None:
        super().clear()
        self.round += 1

    def aggregate(self, models: List[P2PFLModel]) -> P2PFLModel:
        if not models:
            raise NoModelsToAggregateError(f"({self.node_name}) Trying to aggregate models when there is no models")
        dnc_check(len(models), self.f, self.filter_frac, self.iters, self.subsample_dims)
        params = [m.get_parameters() for m in models]
        flats = [flatten(p) for p in params]
        ws = [float(m.get_num_samples()) for m in models]
        if _is_torch(flats[0]):
            import torch

            from myfyp_amd import ops

            rows = [f_.contiguous().float() for f_ in flats]
            out = torch.empty_like(rows[0])
            coef = ops.dnc_into(rows, [out], ws, self.f, self.filter_frac, self.iters, self.subsample_dims, self.seed, self.round)[4]
            pieces, at = [], 0
            for p in params[0]:
                pieces.append(out[at : at + p.numel()].view_as(p).to(p.dtype))
                at += p.numel()
        else:
            out, coef, _, _, _, _ = dnc_numpy(flats, ws, self.f, self.filter_frac, self.iters, self.subsample_dims, self.seed, self.round)
            pieces, at = [], 0
            for p in params[0]:
                p = np.asarray(p)
                pieces.append(out[at : at + p.size].reshape(p.shape).astype(p.dtype))
                at += p.size
        contributors: List[str] = []
        for m in models:
            contributors += m.get_contributors()
        self.last_selection = ([(m.get_contributors() or [None])[0] for m in models], coef)
        return models[0].build_copy(params=pieces, num_samples=sum(m.get_num_samples() for m in models), contributors=contributors)
