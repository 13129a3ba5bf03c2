"""torchrun worker: 4 peers per rank, attackers on both ranks; one colluding attack across the
ranks per kind, checked against the float64 oracle every rank can compute from the shared seeds.
Both ranks must hold the same γ and write the same row, bit for bit."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _collude_ref as cr  # noqa: E402
from myfyp_amd import fault_injection  # noqa: E402
from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol  # noqa: E402
from myfyp_amd.learning.aggregators import Krum  # noqa: E402
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist  # noqa: E402
from myfyp_amd.learning.frameworks.torch import TorchModel  # noqa: E402
from myfyp_amd.models import MLP  # noqa: E402
from myfyp_amd.node import Node  # noqa: E402
from myfyp_amd.parallel.federation import Federation  # noqa: E402
from myfyp_amd.settings import Settings  # noqa: E402

PPR = 4
ATTACKERS = [1, 6, 7]  # one on rank 0, two on rank 1; peer 7 does not train


def _vec(seed, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _row(g, n):
    return _vec(1, n) + 1e-3 * (1 + 0.15 * g) * _vec(100 + g, n)


def main() -> None:
    Settings.DEVICE = os.environ.get("AGG_DEVICE", "cpu")
    fed = Federation.init()
    world = fed.world
    gids = [fed.rank * PPR + j for j in range(PPR)]
    data = synthetic_mnist(200, 50)
    weights = {g: 0.0 if g in (3, 7) else float(1 + g % 3) for g in range(world * PPR)}
    hidden = [8, 8] if Settings.DEVICE == "cpu" else [256, 128]
    nodes = [Node(TorchModel(MLP(hidden_sizes=hidden)), data, address=f"g{g}", aggregator=Krum(num_byzantine=2), protocol=CollectiveCommunicationProtocol) for g in gids]
    for nd in nodes:
        nd.start()
    fed.finalize()
    n = nodes[0].learner.flat_params().numel()
    honest = [g for g in range(world * PPR) if weights[g] > 0 and g not in ATTACKERS]
    attacking = [g for g in ATTACKERS if weights[g] > 0]
    x64 = np.stack([_row(g, n).double().numpy() for g in honest])
    start = (_vec(1, n) + 2e-3).numpy()

    for kind in cr.KINDS:
        attack = fault_injection.ColludingAttack(fed, [f"g{g}" for g in ATTACKERS], kind, z=1.0)
        if kind == "ipm":
            for nd in nodes:
                with torch.no_grad():
                    nd.learner.flat_params().copy_(torch.from_numpy(start))
            for hook in list(fed.round_start_hooks):
                hook(0, fed)
        for g, nd in zip(gids, nodes):
            with torch.no_grad():
                nd.learner.flat_params().copy_(_row(g, n).to(nd.learner.flat_params().device))
        fed.pre_aggregation_hooks[0](0, fed, {nd.addr: weights[g] for g, nd in zip(gids, nodes)})
        order, att, gamma, stat = attack.last
        assert order == [f"g{g}" for g in honest]  # rank, then local order
        assert att == [f"g{g}" for g in attacking]
        m, gam, st = cr.oracle(x64, kind, n_out=len(attacking), z=1.0, ref=start.astype(np.float64))
        assert abs(float(gamma.cpu()[0]) - gam) <= 2.0**-23 * abs(gam)
        for g, nd in zip(gids, nodes):
            got = nd.learner.flat_params().detach().cpu().numpy()
            if g in attacking:
                assert np.abs(got.astype(np.float64) - m).max() <= 2.0**-23 * np.abs(m).max()
            else:
                assert np.array_equal(got, _row(g, n).numpy())
        # every rank holds the same γ and the same crafted row, bit for bit
        mine = (gamma.cpu().numpy().tobytes(), stat.cpu().numpy().tobytes(),
                [nd.learner.flat_params().detach().cpu().numpy().tobytes() for g, nd in zip(gids, nodes) if g in attacking])
        everyone = fed.all_gather_object(mine)
        assert all(o[0] == mine[0] and o[1] == mine[1] for o in everyone)
        rows = [r for o in everyone for r in o[2]]
        assert len(rows) == len(attacking) and all(r == rows[0] for r in rows)
        attack.remove()
    print(f"rank {fed.rank} OK", flush=True)
    for nd in nodes:
        nd.stop()
    fed.shutdown()


if __name__ == "__main__":
    main()
