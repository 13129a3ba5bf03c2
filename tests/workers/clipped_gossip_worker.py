"""torchrun worker: 3 peers per rank on a ring of 6, one of them holding −10 times the shared model;
one ClippedGossip step (adaptive radius, b = 1) against the float64 oracle. The rows a rank
receives from the other are sources only: every rank writes its own three peers."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _clip_ref as ref  # noqa: E402
from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol  # noqa: E402
from myfyp_amd.learning.aggregators import ClippedGossip  # noqa: E402
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist  # noqa: E402
from myfyp_amd.learning.frameworks.torch import TorchModel  # noqa: E402
from myfyp_amd.models import MLP  # noqa: E402
from myfyp_amd.node import Node  # noqa: E402
from myfyp_amd.parallel import weights_plane  # noqa: E402
from myfyp_amd.parallel.federation import Federation  # noqa: E402
from myfyp_amd.settings import Settings  # noqa: E402

BAD = 4


def main() -> None:
    Settings.DEVICE = os.environ.get("AGG_DEVICE", "cpu")
    fed = Federation.init()
    ppr = 3
    data = synthetic_mnist(200, 50)
    gids = [fed.rank * ppr + j for j in range(ppr)]
    nodes = [Node(TorchModel(MLP(hidden_sizes=[8, 8], seed=g)), data, address=f"p{g}", aggregator=ClippedGossip(topology="ring", num_byzantine=1),
                  protocol=CollectiveCommunicationProtocol) for g in gids]
    for nd in nodes:
        nd.start()
    fed.finalize()
    peers = fed.all_peers()
    k = len(peers)
    n = nodes[0].learner.flat_params().numel()
    rng = np.random.default_rng(11)  # the same rows on every rank
    base = rng.standard_normal(n)
    by_gid = np.stack([base + 1e-3 * rng.standard_normal(n) for _ in range(k)]).astype(np.float32)
    by_gid[BAD] = (-10.0 * base).astype(np.float32)
    for g, nd in zip(gids, nodes):
        with torch.no_grad():
            nd.learner.flat_params().copy_(torch.from_numpy(by_gid[g].copy()))
    x32 = np.stack([by_gid[int(p[1:])] for p in peers])  # peer (row) order
    agg = nodes[0].aggregator
    w = agg.mixing_matrix(k)
    shares = w.copy()
    np.fill_diagonal(shares, 0.0)
    shares = shares.astype(np.float32)
    want, d, tau_ref, _, w_ref = ref.clipped_gossip(x32, shares, b=1)
    bad = peers.index(f"p{BAD}")
    # the attacker sees every honest row equally far: its own choice is a coin toss and is not compared
    assert ref.selection_gap(d, shares, 1, rows=[i for i in range(k) if i != bad]) > 1e-3
    weights_plane.aggregate_neighbors(fed, {nd.addr: None for nd in nodes}, agg)
    addrs, tau, w_eff = agg.last_clipping
    rows = [peers.index(a) for a in addrs]
    assert rows == sorted(rows) and set(nd.addr for nd in nodes) <= set(addrs) and len(addrs) == ppr + 2  # its three and the two ring neighbours
    tau, w_eff = tau.cpu().numpy(), w_eff.cpu().numpy()
    bound = ref.mix_bound(x32, w_ref)
    for nd in nodes:
        i = peers.index(nd.addr)
        p = addrs.index(nd.addr)
        if i == bad:
            continue
        np.testing.assert_allclose(w_eff[p], w_ref[i][rows], rtol=2e-5, atol=0)
        np.testing.assert_allclose(tau[p], tau_ref[i], rtol=2e-5, atol=0)
        got = nd.learner.flat_params().detach().cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - want[i]) <= bound[i]), (nd.addr, float(np.abs(got - want[i]).max()))
    for a in addrs:  # a received row is a source only: an all-zero row of the plan
        if a not in fed.local_nodes:
            assert not w_eff[addrs.index(a)].any()
    for nd in nodes:
        i = peers.index(nd.addr)
        if shares[i, bad] > 0:
            assert w_eff[addrs.index(nd.addr), addrs.index(f"p{BAD}")] < 0.01 * shares[i, bad]
    print(f"rank {fed.rank} OK", flush=True)
    for nd in nodes:
        nd.stop()
    fed.shutdown()


if __name__ == "__main__":
    main()
