"""Bulyan (El Mhamdi, Guerraoui, Rouault, 2018): robust aggregation for the FYP Byzantine harness
that closes the gap between the distance-based defences and the coordinate-wise ones. Krum and the
geometric median judge a model by its L2 distance alone, so one coordinate may carry an error of
order √D·σ unnoticed; the trimmed mean never rejects a peer as a whole. Bulyan picks K − 2f models
by iterated Krum and then, per coordinate, averages the K − 4f picked values closest to their
median. Not in the reference."""

from __future__ import annotations

from typing import List, Sequence

import numpy as np

from myfyp_amd.learning.aggregators._math import _is_torch, flatten
from myfyp_amd.learning.aggregators.aggregator import Aggregator, NoModelsToAggregateError
from myfyp_amd.learning.frameworks.p2pfl_model import P2PFLModel


def bulyan_check(k: int, f: int) -> int:
    """``f >= 0`` and ``K >= 4f + 3``; with ``f == 0`` (nothing rejected, nothing trimmed: the plain
    mean) any ``K >= 1`` does."""
    if int(f) != f or f < 0:
        raise ValueError(f"Bulyan: the attacker bound f must be an integer >= 0, got f = {f} (K = {k})")
    f = int(f)
    if k < 1 or (f > 0 and k < 4 * f + 3):
        raise ValueError(f"Bulyan needs K >= 4f + 3 models: K = {k}, f = {f} needs {4 * f + 3}")
    return f


def bulyan_numpy(rows: Sequence[np.ndarray], f: int):
    """``ops.bulyan_into``'s definition over numpy rows, any K: ``(out float32, coef float32, pick
    int32, dist float64 [K, K], score float64)``. Distances in float64 from differences; stage 2 on
    the rows as float32, in float32."""
    k = len(rows)
    f = bulyan_check(k, f)
    n = np.asarray(rows[0]).size
    if n < 1 or any(np.asarray(r).size != n for r in rows):
        raise ValueError(f"Bulyan: rows must share one length >= 1, got {[np.asarray(r).size for r in rows]}")
    theta, beta = k - 2 * f, k - 4 * f
    inf = float("inf")
    with np.errstate(all="ignore"):
        x = [np.asarray(r, dtype=np.float64).ravel() for r in rows]
        dist = np.zeros((k, k))
        for i in range(k):
            for j in range(i + 1, k):
                dist[i, j] = dist[j, i] = ((x[i] - x[j]) ** 2).sum()
        remaining = list(range(k))
        pick = np.full(k, -1, dtype=np.int32)
        score = np.zeros(k)
        for it in range(theta):
            r = len(remaining)
            cnt = min(max(r - f - 2, 1), r - 1)
            sc = {}
            for i in remaining:
                others = sorted((float(dist[i, j]) for j in remaining if j != i), key=lambda v: inf if v != v else v)
                sc[i] = float(sum(others[:cnt]))  # ascending order
            if it == 0:
                score = np.array([sc[i] for i in range(k)])
            best = min(remaining, key=lambda i: (inf if sc[i] != sc[i] else sc[i], i))
            pick[best] = it
            remaining.remove(best)
        coef = np.where(pick >= 0, np.float32(1) / np.float32(theta), np.float32(0)).astype(np.float32)
        v = np.sort(np.stack([np.asarray(rows[i], dtype=np.float32).ravel() for i in range(k) if pick[i] >= 0]), axis=0)
        m = v[(theta - 1) // 2] if theta % 2 else np.float32(0.5) * (v[theta // 2 - 1] + v[theta // 2])
        best_cost = mean = None
        for s in range(2 * f + 1):
            cost = np.maximum(m - v[s], v[s + beta - 1] - m)
            acc = v[s].copy()
            for j in range(1, beta):
                acc = acc + v[s + j]
            if best_cost is None:
                best_cost, mean = cost, acc
            else:
                better = cost < best_cost
                best_cost = np.where(better, cost, best_cost)
                mean = np.where(better, acc, mean)
        out = (mean / np.float32(beta)).astype(np.float32)
    return out, coef, pick, dist, score


class Bulyan(Aggregator):
    """K − 2f models picked by iterated Krum, then per coordinate the mean of the K − 4f picked
    values closest to their median; needs ``K >= 4f + 3`` models. Sample weights are not used."""

    collective_kind = "bulyan"

    def __init__(self, node_name: str = "unknown", num_byzantine: int = 1) -> None:
        super().__init__(node_name)
        if int(num_byzantine) != num_byzantine or num_byzantine < 0:
            raise ValueError(f"num_byzantine must be an integer >= 0, got {num_byzantine}")
        self.f = int(num_byzantine)
        self.partial_aggregation = False
        # set after an aggregation: (trainer addresses in row order, coef); coef[i] == 0 means peer
        # i was rejected. After a device aggregation coef is the device tensor: reading it synchronises.
        self.last_selection = None

    def aggregate(self, models: List[P2PFLModel]) -> P2PFLModel:
        if not models:
            raise NoModelsToAggregateError(f"({self.node_name}) Trying to aggregate models when there is no models")
        bulyan_check(len(models), self.f)
        params = [m.get_parameters() for m in models]
        flats = [flatten(p) for p in params]
        if _is_torch(flats[0]):
            import torch

            from myfyp_amd import ops

            rows = [f_.contiguous().float() for f_ in flats]
            out = torch.empty_like(rows[0])
            _, _, coef, _ = ops.bulyan_into(rows, [out], self.f)
            pieces, at = [], 0
            for p in params[0]:
                pieces.append(out[at : at + p.numel()].view_as(p).to(p.dtype))
                at += p.numel()
        else:
            out, coef, _, _, _ = bulyan_numpy(flats, self.f)
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
