"""torchrun worker: 3 peers per rank; one device geometric-median step across the ranks, checked
against the float64 definition every rank can compute from the shared seeds — so both ranks must
have reached the same coefficients."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol  # noqa: E402
from myfyp_amd.learning.aggregators import GeometricMedian  # noqa: E402
from myfyp_amd.learning.aggregators.geometric_median import geometric_median_numpy  # noqa: E402
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist  # noqa: E402
from myfyp_amd.learning.frameworks.torch import TorchModel  # noqa: E402
from myfyp_amd.models import MLP  # noqa: E402
from myfyp_amd.node import Node  # noqa: E402
from myfyp_amd.parallel import weights_plane  # noqa: E402
from myfyp_amd.parallel.federation import Federation  # noqa: E402
from myfyp_amd.settings import Settings  # noqa: E402

PPR = 3
FLIPPED = 4  # a trainer on rank 1


def _vec(seed, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _row(g, n, offset):
    """Peer g's model: one shared vector plus ~1e-3 of noise; the flipped trainer sends its negation."""
    r = _vec(1, n) + 1e-3 * (1 + 0.15 * g) * _vec(offset + g, n)
    return -r if g == FLIPPED else r


def main() -> None:
    Settings.DEVICE = os.environ.get("AGG_DEVICE", "cpu")
    fed = Federation.init()
    world = fed.world
    gids = [fed.rank * PPR + j for j in range(PPR)]
    data = synthetic_mnist(200, 50)
    weights = {g: float(g % 3) for g in range(world * PPR)}  # peers 0 and 3 are non-trainers
    hidden = [8, 8] if Settings.DEVICE == "cpu" else [256, 128]  # fused MLP engine rows on the GPU
    gm = [Node(TorchModel(MLP(hidden_sizes=hidden)), data, address=f"g{g}", aggregator=GeometricMedian(iters=3), protocol=CollectiveCommunicationProtocol) for g in gids]
    for nd in gm:
        nd.start()
    fed.finalize()
    n = gm[0].learner.flat_params().numel()
    tr = [g for g in range(world * PPR) if weights[g] > 0]

    def generic(*a, **k):
        raise AssertionError("the generic (wire model) path was taken")

    weights_plane.aggregate_generic = generic

    for g, nd in zip(gids, gm):
        with torch.no_grad():
            nd.learner.flat_params().copy_(_row(g, n, 100).to(nd.learner.flat_params().device))
    weights_plane.aggregate_geometric_median(fed, {nd.addr: (weights[g], None) for g, nd in zip(gids, gm)}, gm[0].aggregator)
    exp, coef_ref, _, _ = geometric_median_numpy([_row(g, n, 100).double().numpy() for g in tr], [weights[g] for g in tr], 3, 1e-6)
    share = weights[FLIPPED] / sum(weights[g] for g in tr)
    assert coef_ref[tr.index(FLIPPED)] < 0.1 * share
    got = []
    for nd in gm:
        assert np.abs(nd.learner.flat_params().double().cpu().numpy() - exp).max() < 1e-5
        addrs, coef = nd.aggregator.last_weights
        assert addrs == [f"g{g}" for g in tr]  # rank, then local order
        got.append(coef.cpu().numpy())
        np.testing.assert_allclose(got[-1], coef_ref, rtol=1e-4)
    # every rank holds the same coefficients, bit for bit
    mine = got[0].tolist()
    assert all(np.array_equal(c, got[0]) for c in got)
    assert all(other == mine for other in fed.all_gather_object(mine))
    print(f"rank {fed.rank} OK", flush=True)
    for nd in gm:
        nd.stop()
    fed.shutdown()


if __name__ == "__main__":
    main()
