"""(Multi-)Krum (Blanchard et al., 2017): robust selection for the FYP Byzantine harness
(``exp_SAVE3.txt:60-234``). Not in the reference."""

from __future__ import annotations

from typing import List

import numpy as np

from myfyp_amd.learning.aggregators._math import _is_torch, flatten, weighted_mean
from myfyp_amd.learning.aggregators.aggregator import Aggregator, NoModelsToAggregateError
from myfyp_amd.learning.frameworks.p2pfl_model import P2PFLModel


def _nan_last(v: float) -> float:
    return float("inf") if v != v else float(v)


class Krum(Aggregator):
    """Score each model by the summed squared distance to its ``n - f - 2`` nearest peers; average
    the ``m`` best (m=1 → classic Krum)."""

    collective_kind = "krum"

    def __init__(self, node_name: str = "unknown", num_byzantine: int = 1, multi: int = 1) -> None:
        super().__init__(node_name)
        self.f = num_byzantine
        self.m = multi
        self.partial_aggregation = False
        # set by the collective plane after a device aggregation: (trainer addresses in row order,
        # coef device tensor); coef[i] == 0 means peer i was rejected. Reading coef synchronises.
        self.last_selection = None

    def aggregate(self, models: List[P2PFLModel]) -> P2PFLModel:
        if not models:
            raise NoModelsToAggregateError(f"({self.node_name}) Trying to aggregate models when there is no models")
        n = len(models)
        flats = [flatten(m.get_parameters()) for m in models]
        if _is_torch(flats[0]):
            from myfyp_amd import ops

            # distances (from differences) and scores on the rows' device; only K scores reach the host
            _, score, _ = ops.krum_into([f_.contiguous() for f_ in flats], [], [float(m.get_num_samples()) for m in models], self.f, self.m)
            scores = score.cpu().numpy()
        else:
            # as ops.krum_into: distances from differences (a row of ±inf is at +inf or NaN of the
            # others, never at a cancelled finite value), a NaN ordering as +inf
            X = np.stack(flats)
            d = np.zeros((n, n))
            with np.errstate(invalid="ignore", over="ignore"):
                for i in range(n):
                    for j in range(i + 1, n):
                        d[i, j] = d[j, i] = np.square(X[i] - X[j]).sum()
                k = min(max(1, n - self.f - 2), n - 1)
                scores = []
                for i in range(n):
                    near = sorted((j for j in range(n) if j != i), key=lambda j: (_nan_last(d[i, j]), j))[:k]
                    scores.append(float(sum(d[i, j] for j in near)))
        # the lower index wins a tie, a NaN score orders last (with +inf)
        order = sorted(range(n), key=lambda i: (_nan_last(scores[i]), i))
        chosen = [models[i] for i in order[: max(1, min(self.m, n))]]
        params = weighted_mean([m.get_parameters() for m in chosen], [m.get_num_samples() for m in chosen])
        contributors: List[str] = []
        for m in models:
            contributors += m.get_contributors()
        return models[0].build_copy(params=params, num_samples=sum(m.get_num_samples() for m in models), contributors=contributors)
