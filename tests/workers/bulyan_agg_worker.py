"""torchrun worker: 4 peers per rank; one device Bulyan aggregation across the ranks, checked
against the definition every rank can compute from the shared seeds — so both ranks must have
picked the same peers. Before it, an attacker bound too large for the round's trainers must raise
on every rank (the check runs on the gathered K, before any tensor collective)."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol  # noqa: E402
from myfyp_amd.learning.aggregators import Bulyan  # noqa: E402
from myfyp_amd.learning.aggregators.bulyan import bulyan_numpy  # noqa: E402
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist  # noqa: E402
from myfyp_amd.learning.frameworks.torch import TorchModel  # noqa: E402
from myfyp_amd.models import MLP  # noqa: E402
from myfyp_amd.node import Node  # noqa: E402
from myfyp_amd.parallel import weights_plane  # noqa: E402
from myfyp_amd.parallel.federation import Federation  # noqa: E402
from myfyp_amd.settings import Settings  # noqa: E402

PPR = 4
FLIPPED = 5  # a trainer on rank 1
F = 1


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
    weights = {g: float(min(g, 3)) for g in range(world * PPR)}  # peer 0 is a non-trainer: 7 trainers = 4F + 3
    hidden = [8, 8] if Settings.DEVICE == "cpu" else [256, 128]  # fused MLP engine rows on the GPU
    bl = [Node(TorchModel(MLP(hidden_sizes=hidden)), data, address=f"g{g}", aggregator=Bulyan(num_byzantine=F), protocol=CollectiveCommunicationProtocol) for g in gids]
    for nd in bl:
        nd.start()
    fed.finalize()
    n = bl[0].learner.flat_params().numel()
    tr = [g for g in range(world * PPR) if weights[g] > 0]

    def generic(*a, **k):
        raise AssertionError("the generic (wire model) path was taken")

    weights_plane.aggregate_generic = generic

    for g, nd in zip(gids, bl):
        with torch.no_grad():
            nd.learner.flat_params().copy_(_row(g, n, 100).to(nd.learner.flat_params().device))
    arrived = {nd.addr: (weights[g], None) for g, nd in zip(gids, bl)}
    # K = 7 < 4·2 + 3: every rank raises, none has entered the tensor all-gather, no row is written
    try:
        weights_plane.aggregate_bulyan(fed, arrived, Bulyan(num_byzantine=2))
        raised = ""
    except ValueError as e:
        raised = str(e)
    assert "K = 7" in raised and "f = 2" in raised, raised
    assert all(fed.all_gather_object(bool(raised)))
    for g, nd in zip(gids, bl):
        assert torch.equal(nd.learner.flat_params().cpu(), _row(g, n, 100))

    weights_plane.aggregate_bulyan(fed, arrived, bl[0].aggregator)
    x = np.stack([_row(g, n, 100).numpy() for g in tr])
    exp, coef_ref, _, _, _ = bulyan_numpy(list(x), F)
    assert coef_ref[tr.index(FLIPPED)] == 0
    atol = 2 * (len(tr) - 4 * F) * 2.0**-24 * float(np.abs(x).max())  # tests/test_bulyan_kernels_gpu.py: device and oracle around one window mean
    got = []
    for nd in bl:
        assert np.abs(nd.learner.flat_params().double().cpu().numpy() - exp).max() <= atol
        addrs, coef = nd.aggregator.last_selection
        assert addrs == [f"g{g}" for g in tr]  # rank, then local order
        got.append(coef.cpu().numpy())
        assert np.array_equal(got[-1], coef_ref)
    # every rank holds the same aggregate, bit for bit
    mine = bl[0].learner.flat_params().cpu().numpy().tobytes()
    assert all(nd.learner.flat_params().cpu().numpy().tobytes() == mine for nd in bl)
    assert all(other == mine for other in fed.all_gather_object(mine))
    print(f"rank {fed.rank} OK", flush=True)
    for nd in bl:
        nd.stop()
    fed.shutdown()


if __name__ == "__main__":
    main()
