"""torchrun worker: 3 peers per rank; one device Krum step and one device trimmed-mean step across
the ranks, checked against the closed forms every rank can compute from the shared seeds — so both
ranks must have chosen the same peers."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol  # noqa: E402
from myfyp_amd.learning.aggregators import Krum, TrimmedMean  # noqa: E402
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
    kr = [Node(TorchModel(MLP(hidden_sizes=hidden)), data, address=f"k{g}", aggregator=Krum(num_byzantine=1, multi=2), protocol=CollectiveCommunicationProtocol) for g in gids]
    tm = [Node(TorchModel(MLP(hidden_sizes=hidden)), data, address=f"t{g}", aggregator=TrimmedMean(beta=0.25), protocol=CollectiveCommunicationProtocol) for g in gids]
    for nd in kr + tm:
        nd.start()
    fed.finalize()
    n = kr[0].learner.flat_params().numel()
    tr = [g for g in range(world * PPR) if weights[g] > 0]

    def generic(*a, **k):
        raise AssertionError("the generic (wire model) path was taken")

    weights_plane.aggregate_generic = generic

    # Krum: f = 1, m = 2 over the 4 trainers
    for g, nd in zip(gids, kr):
        with torch.no_grad():
            nd.learner.flat_params().copy_(_row(g, n, 100).to(nd.learner.flat_params().device))
    weights_plane.aggregate_krum(fed, {nd.addr: (weights[g], None) for g, nd in zip(gids, kr)}, kr[0].aggregator)
    x = [_row(g, n, 100).double().numpy() for g in tr]
    d = np.array([[((a - b) ** 2).sum() for b in x] for a in x])
    cnt = max(1, len(tr) - 1 - 2)
    scores = np.array([np.sort(np.delete(d[i], i))[:cnt].sum() for i in range(len(tr))])
    chosen = sorted(np.argsort(scores, kind="stable")[:2])
    assert tr.index(FLIPPED) not in chosen
    tot = sum(weights[tr[i]] for i in chosen)
    exp = sum(weights[tr[i]] / tot * x[i] for i in chosen)
    for nd in kr:
        assert np.abs(nd.learner.flat_params().double().cpu().numpy() - exp).max() < 1e-6
        addrs, coef = nd.aggregator.last_selection
        assert addrs == [f"k{g}" for g in tr]  # rank, then local order
        coef = coef.cpu().numpy()
        assert [i for i in range(len(tr)) if coef[i] != 0] == chosen and coef[tr.index(FLIPPED)] == 0

    # trimmed mean: beta = 0.25 over the 4 trainers drops one value from each end
    for g, nd in zip(gids, tm):
        with torch.no_grad():
            nd.learner.flat_params().copy_(_row(g, n, 300).to(nd.learner.flat_params().device))
    weights_plane.aggregate_trimmed_mean(fed, {nd.addr: (weights[g], None) for g, nd in zip(gids, tm)}, tm[0].aggregator)
    s = np.sort(np.stack([_row(g, n, 300).double().numpy() for g in tr]), axis=0)
    exp = s[1:3].mean(axis=0)
    for nd in tm:
        assert np.abs(nd.learner.flat_params().double().cpu().numpy() - exp).max() < 1e-6
    print(f"rank {fed.rank} OK", flush=True)
    for nd in kr + tm:
        nd.stop()
    fed.shutdown()


if __name__ == "__main__":
    main()
