"""ClippedGossip (He, Karimireddy, Jaggi, 2022, "Byzantine-robust decentralized learning via
ClippedGossip" — https://arxiv.org/abs/2202.01545): neighbour mixing over a static graph that one
hostile neighbour cannot drag. Not in the reference.

``NeighborAvg`` mixes a neighbour's row at full weight, so one scaled or NaN row spreads round a
ring in a few rounds. Here every peer keeps its own model and moves towards each neighbour by at
most a radius τ_i::

    x_i ← x_i + Σ_{j∈N_i} W_ij · s_ij · (x_j − x_i),   s_ij = min(1, τ_i / ‖x_j − x_i‖)

The radius is fixed (``tau``) or adaptive (``num_byzantine = b``): the b farthest neighbours F_i are
set aside and τ_i² = Σ_{N_i∖F_i} W_ij ‖x_j − x_i‖² / Σ_{F_i} W_ij. ``b = 0`` is plain mixing in
difference form; a peer whose whole neighbourhood may be hostile (b ≥ |N_i|) keeps its own model.
Nothing is kept between rounds.

Collective plane (``collective_kind = "neighbor"``, as ``NeighborAvg``): the weights plane hands the
co-located rows (and those received from other ranks, as sources only) to
``ops.clipped_gossip_into``: three launches on the GPU, in place.
"""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from myfyp_amd.learning.aggregators._math import flatten, to_numpy_list
from myfyp_amd.learning.aggregators.aggregator import NoModelsToAggregateError
from myfyp_amd.learning.aggregators.neighbor_avg import NeighborAvg
from myfyp_amd.learning.frameworks.p2pfl_model import P2PFLModel


def clipped_gossip_numpy(rows: Sequence[np.ndarray], w, tau: Optional[float] = None, num_byzantine: Optional[int] = None):
    """``ops.clipped_gossip_into``'s definition over numpy rows, any K, in float64: ``(out rows
    float64 [K, n], tau float64 [K], w_eff float32 [K, K], dist float64 [K, K])``. The rows are not
    modified; a row that is not written comes back as it is."""
    from myfyp_amd.ops import clip_plan

    k = len(rows)
    w = np.asarray(w, dtype=np.float32)  # the shares as the device takes them
    with np.errstate(all="ignore"):
        x = [np.asarray(r, dtype=np.float64).ravel() for r in rows]
        dist = np.zeros((k, k))
        for i in range(k):
            for j in range(i + 1, k):
                dist[i, j] = dist[j, i] = ((x[i] - x[j]) ** 2).sum()
        taus, w_eff = clip_plan(dist, w, tau, num_byzantine)
        out = []
        for p in range(k):
            acc = np.zeros_like(x[p])
            for q in range(k):
                if w_eff[p, q] != 0:  # a source of weight 0 is never read into the sum
                    acc = acc + float(w_eff[p, q]) * (x[q] - x[p])
            out.append(x[p] + acc if w_eff[p].any() else x[p].copy())
    return np.stack(out), taus, w_eff, dist


class ClippedGossip(NeighborAvg):
    """``NeighborAvg`` with every neighbour's pull clipped to a radius: fixed (``tau``) or adaptive for
    at most ``num_byzantine`` hostile neighbours per peer (used when ``tau`` is None)."""

    clipped = True  # the weights plane's switch from the plain mix to ops.clipped_gossip_into

    def __init__(self, node_name: str = "unknown", topology: str = "ring", weights: str = "metropolis", adjacency=None, tau: Optional[float] = None,
                 num_byzantine: int = 1) -> None:
        super().__init__(node_name, topology=topology, weights=weights, adjacency=adjacency)
        if tau is not None and not float(tau) >= 0:
            raise ValueError(f"tau must be >= 0, got {tau}")
        if tau is None and (int(num_byzantine) != num_byzantine or num_byzantine < 0):
            raise ValueError(f"num_byzantine must be an integer >= 0, got {num_byzantine}")
        self.tau = None if tau is None else float(tau)
        self.f = int(num_byzantine)
        self.partial_aggregation = False  # clipping a partial mix has no meaning
        # set after a device round: (peer addresses in row order, tau [K], w_eff [K, K]) as device
        # tensors; w_eff[p, q] / W[p, q] is the scale peer p applied to neighbour q. Reading them synchronises.
        self.last_clipping = None

    def radius_args(self) -> dict:
        """The keyword that selects the radius in ``ops.clipped_gossip_into`` / ``clipped_gossip_numpy``."""
        return {"tau": self.tau} if self.tau is not None else {"num_byzantine": self.f}

    def aggregate(self, models: List[P2PFLModel]) -> P2PFLModel:
        """Gossip plane: centred on this node's own model when it is among ``models`` (every other
        model a neighbour of share 1/len(models)); otherwise the plain mean, as ``NeighborAvg``."""
        if not models:
            raise NoModelsToAggregateError(f"({self.node_name}) Trying to aggregate models when there is no models")
        own = [i for i, m in enumerate(models) if m.get_contributors() == [self.node_name]]
        if len(own) != 1:
            return super().aggregate(models)
        order = [own[0]] + [i for i in range(len(models)) if i != own[0]]
        params = [to_numpy_list(models[i].get_parameters()) for i in order]
        k = len(order)
        w = np.zeros((k, k))
        w[0, 1:] = 1.0 / k
        out, taus, w_eff, _ = clipped_gossip_numpy([flatten(p) for p in params], w, **self.radius_args())
        self.last_clipping = ([(models[i].get_contributors() or [None])[0] for i in order], taus, w_eff)
        pieces, at = [], 0
        for p in params[0]:
            pieces.append(out[0][at : at + p.size].reshape(p.shape).astype(p.dtype))
            at += p.size
        contributors: List[str] = []
        for m in models:
            contributors += m.get_contributors()
        return models[own[0]].build_copy(params=pieces, num_samples=int(sum(m.get_num_samples() for m in models)), contributors=contributors)
