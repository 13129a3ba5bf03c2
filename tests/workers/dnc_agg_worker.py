"""torchrun worker: 4 peers per rank; one device DnC aggregation across the ranks, checked against
the definition every rank can compute from the shared seeds — so both ranks must have removed the
same peers. Before it, parameters too large for the round's trainers must raise on every rank (the
check runs on the gathered K, before any tensor collective)."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _collude_ref as cref  # noqa: E402
from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol  # noqa: E402
from myfyp_amd.learning.aggregators import DnC  # noqa: E402
from myfyp_amd.learning.aggregators.dnc import dnc_numpy  # noqa: E402
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist  # noqa: E402
from myfyp_amd.learning.frameworks.torch import TorchModel  # noqa: E402
from myfyp_amd.models import MLP  # noqa: E402
from myfyp_amd.node import Node  # noqa: E402
from myfyp_amd.parallel import weights_plane  # noqa: E402
from myfyp_amd.parallel.federation import Federation  # noqa: E402
from myfyp_amd.settings import Settings  # noqa: E402

PPR = 4
BAD = [2, 5]  # colluding trainers, one on each rank
F = 2
ITERS, DIMS, SEED, ROUND = 2, 2000, 3, 6


def _rows(world, n, weights):
    """Every peer's model from the shared seed: one vector plus 1e-3 of noise, the colluders at μ − 3γσ."""
    rng = np.random.default_rng(17)
    base = rng.standard_normal(n)
    rows = [(base + 1e-3 * rng.standard_normal(n)).astype(np.float32) for _ in range(world * PPR)]
    honest = np.stack([r for g, r in enumerate(rows) if g not in BAD and weights[g] > 0]).astype(np.float64)
    _, gam, st = cref.oracle(honest, "min_max")
    for g in BAD:
        rows[g] = (st["mu"] - 3.0 * gam * st["sigma"]).astype(np.float32)
    return rows


def main() -> None:
    Settings.DEVICE = os.environ.get("AGG_DEVICE", "cpu")
    fed = Federation.init()
    world = fed.world
    gids = [fed.rank * PPR + j for j in range(PPR)]
    data = synthetic_mnist(200, 50)
    weights = {g: float(min(g, 3)) for g in range(world * PPR)}  # peer 0 is a non-trainer: 7 trainers
    hidden = [8, 8] if Settings.DEVICE == "cpu" else [256, 128]  # fused MLP engine rows on the GPU
    mk = lambda: DnC(num_byzantine=F, iters=ITERS, subsample_dims=DIMS, seed=SEED)  # noqa: E731
    dn = [Node(TorchModel(MLP(hidden_sizes=hidden)), data, address=f"g{g}", aggregator=mk(), protocol=CollectiveCommunicationProtocol) for g in gids]
    for nd in dn:
        nd.start()
    fed.finalize()
    n = dn[0].learner.flat_params().numel()
    assert n > DIMS
    tr = [g for g in range(world * PPR) if weights[g] > 0]
    rows = _rows(world, n, weights)

    def generic(*a, **k):
        raise AssertionError("the generic (wire model) path was taken")

    weights_plane.aggregate_generic = generic

    for g, nd in zip(gids, dn):
        with torch.no_grad():
            nd.learner.flat_params().copy_(torch.from_numpy(rows[g]).to(nd.learner.flat_params().device))
    arrived = {nd.addr: (weights[g], None) for g, nd in zip(gids, dn)}
    # K = 7 = 1 · ceil(1.0 · 7): every rank raises, none has entered the tensor all-gather, no row is written
    try:
        weights_plane.aggregate_dnc(fed, arrived, DnC(num_byzantine=7), ROUND)
        raised = ""
    except ValueError as e:
        raised = str(e)
    assert "K = 7" in raised and "iters" in raised, raised
    assert all(fed.all_gather_object(bool(raised)))
    for g, nd in zip(gids, dn):
        assert np.array_equal(nd.learner.flat_params().cpu().numpy(), rows[g])

    weights_plane.aggregate_dnc(fed, arrived, dn[0].aggregator, ROUND)
    x = np.stack([rows[g] for g in tr])
    exp, coef_ref, removed, _, _, _ = dnc_numpy(list(x), [weights[g] for g in tr], F, 1.0, ITERS, DIMS, SEED, ROUND)
    assert sorted(tr[i] for i in np.flatnonzero(removed >= 0)) == BAD
    atol = 2 * int((coef_ref != 0).sum()) * 2.0**-24 * float(np.abs(x).max())  # tests/test_dnc_kernels_gpu.py: both around the float64 mean
    for nd in dn:
        assert np.abs(nd.learner.flat_params().double().cpu().numpy() - exp).max() <= atol
        assert nd.aggregator.round == ROUND
        addrs, coef = nd.aggregator.last_selection
        assert addrs == [f"g{g}" for g in tr]  # rank, then local order
        assert np.array_equal(coef.cpu().numpy(), coef_ref)
    # every rank holds the same aggregate, bit for bit
    mine = dn[0].learner.flat_params().cpu().numpy().tobytes()
    assert all(nd.learner.flat_params().cpu().numpy().tobytes() == mine for nd in dn)
    assert all(other == mine for other in fed.all_gather_object(mine))
    print(f"rank {fed.rank} OK", flush=True)
    for nd in dn:
        nd.stop()
    fed.shutdown()


if __name__ == "__main__":
    main()
