"""GeometricMedian on the collective plane (``weights_plane.aggregate_geometric_median``) against
the host aggregator on wire copies of the same models and against the float64 definition.

The device path never builds wire models: the trainers' flat rows are screened, measured and
reweighted by the kernels behind ``ops.geometric_median_into`` and the weighted mean is written into
every local peer. CPU (in-process, and a 2-device host mesh) here, the same checks on ``cuda:0``
under the gpu marker (fused MLP engine rows), and a 2-rank gloo run through ``tests/workers``.
"""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

from _ports import free_port
import torch

from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol
from myfyp_amd.learning.aggregators import GeometricMedian
from myfyp_amd.learning.aggregators.geometric_median import geometric_median_numpy
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP
from myfyp_amd.node import Node
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [4.0, 0.0, 2.0, 1.0, 3.0]  # peer 1 is a non-trainer
FLIPPED = 3  # a trainer, a tenth of the samples


class _BNNet(torch.nn.Module):
    """A model with BatchNorm buffers (running statistics and the integer batch counter)."""

    def __init__(self, seed: int = 0) -> None:
        super().__init__()
        torch.manual_seed(seed)
        self.fc1 = torch.nn.Linear(784, 8)
        self.bn = torch.nn.BatchNorm1d(8)
        self.fc2 = torch.nn.Linear(8, 10)

    def forward(self, x):
        return self.fc2(torch.relu(self.bn(self.fc1(x.flatten(1)))))


def _nodes(k, hidden, module=None):
    data = synthetic_mnist(200, 50)
    tag = time.time_ns()
    if module is None:
        module = (lambda i: MLP(seed=i)) if hidden is None else (lambda i: MLP(hidden_sizes=hidden, seed=i))
    return [Node(TorchModel(module(i)), data, address=f"gm{tag}-{i}", aggregator=GeometricMedian(iters=3), protocol=CollectiveCommunicationProtocol)
            for i in range(k)]


def _flat64(t):
    return t.detach().double().cpu().numpy().ravel()


def _close_rows(nodes, seed, flipped=FLIPPED):
    """Every peer one shared model plus ~1e-3 of noise; the trainer ``flipped`` sends its negation."""
    g = torch.Generator().manual_seed(seed)
    n = nodes[0].learner.flat_params().numel()
    base = torch.randn(n, generator=g)
    rows = []
    for i, nd in enumerate(nodes):
        r = base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g)
        if i == flipped:
            r = -r
        with torch.no_grad():
            nd.learner.flat_params().copy_(r)
        rows.append(r.double().numpy())
    return rows


def _wire(nodes, idx, weights):
    return [nodes[i].learner.get_model().build_copy(params=[p.copy() for p in nodes[i].learner.get_model().get_parameters()], num_samples=int(weights[i]),
                                                    contributors=[nodes[i].addr]) for i in idx]


def _start(device, hidden, module=None, devices=None, k=len(WEIGHTS)):
    Settings.DEVICE = device
    Federation.reset()
    fed = Federation.init(devices=devices) if devices else Federation.init()
    nodes = _nodes(k, hidden, module)
    for nd in nodes:
        nd.start()
    fed.finalize()
    return fed, nodes


def _stop(nodes):
    for nd in nodes:
        nd.stop()
    Federation.reset()
    Settings.DEVICE = "auto"


def _no_generic(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the generic (wire model) path was taken")

    monkeypatch.setattr(weights_plane, "aggregate_generic", boom)


def _case(device, hidden, monkeypatch, devices=None):
    fed, nodes = _start(device, hidden, devices=devices)
    try:
        _no_generic(monkeypatch)
        rows = _close_rows(nodes, seed=9)
        tr = [i for i, w in enumerate(WEIGHTS) if w > 0]
        ws = [WEIGHTS[i] for i in tr]
        exp, coef, _, _ = geometric_median_numpy([rows[i] for i in tr], ws, 3, 1e-6)
        share = WEIGHTS[FLIPPED] / sum(ws)
        assert coef[tr.index(FLIPPED)] < 0.01 * share  # the definition down-weights the flipped trainer
        host = GeometricMedian(iters=3).aggregate(_wire(nodes, tr, WEIGHTS))
        host_flat = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in host.get_parameters()])
        np.testing.assert_allclose(host_flat[: exp.size], exp, rtol=0, atol=1e-6)
        weights_plane.aggregate_geometric_median(fed, {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}, nodes[0].aggregator)
        for nd in nodes:  # the non-trainer (weight 0) receives the aggregate too
            np.testing.assert_allclose(_flat64(nd.learner.flat_params()), exp, rtol=0, atol=1e-6)
        for nd in nodes:
            addrs, c = nd.aggregator.last_weights
            # row order: the trainers in local order (on a mesh: device by device)
            assert sorted(addrs) == sorted(nodes[i].addr for i in tr) and (devices or addrs == [nodes[i].addr for i in tr])
            assert c.device.type == nd.learner.flat_params().device.type  # stayed on the device
            by_addr = dict(zip(addrs, c.cpu().numpy()))
            assert by_addr[nodes[FLIPPED].addr] < 0.01 * share
            # three steps in fp32 on the GPU, each within ~1e-6 of the float64 step (tests/test_geomed_kernels_gpu.py)
            np.testing.assert_allclose([by_addr[nodes[i].addr] for i in tr], coef, rtol=1e-4, atol=0)
            assert getattr(nd.aggregator, "last_selection", None) is None
    finally:
        _stop(nodes)


def test_geomed_device_plane_cpu(monkeypatch):
    _case("cpu", [8, 8], monkeypatch)


def test_geomed_device_plane_cpu_mesh(monkeypatch):
    """Two host-mesh devices: ``_mesh_robust`` (one mesh all-gather, the op per device)."""
    _case("cpu", [8, 8], monkeypatch, devices=["cpu", "cpu"])


def test_geomed_batchnorm_buffers_cpu(monkeypatch):
    """``get_parameters()`` is the whole ``state_dict``: the host ``GeometricMedian`` also measures
    BatchNorm's running statistics and its integer batch counter, so the device rows carry them too
    (the packed path). One trainer's counter is far from the others': both must down-weight it."""
    fed, nodes = _start("cpu", None, module=lambda i: _BNNet(seed=i))
    try:
        _no_generic(monkeypatch)
        _close_rows(nodes, seed=13, flipped=None)
        odd = 2
        g = torch.Generator().manual_seed(17)
        for i, nd in enumerate(nodes):
            bn = nd.learner.model.get_model().bn
            with torch.no_grad():
                bn.running_mean.copy_(0.01 * torch.randn(8, generator=g))
                bn.running_var.copy_(1 + 0.01 * torch.randn(8, generator=g))
                bn.num_batches_tracked.fill_(40 if i == odd else 3)
        tr = [i for i, w in enumerate(WEIGHTS) if w > 0]
        ws = [WEIGHTS[i] for i in tr]
        full = [np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in nodes[i].learner.get_model().get_parameters()]) for i in tr]
        _, coef, _, _ = geometric_median_numpy(full, ws, 3, 1e-6)
        flats = [_flat64(nodes[i].learner.flat_params()) for i in tr]
        _, coef_flat, _, _ = geometric_median_numpy(flats, ws, 3, 1e-6)
        o = tr.index(odd)
        assert coef[o] < 0.1 * coef_flat[o]  # the buffers decide
        host = GeometricMedian(iters=3).aggregate(_wire(nodes, tr, WEIGHTS))
        host_state = host.get_parameters()
        weights_plane.aggregate_geometric_median(fed, {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}, nodes[0].aggregator)
        c = nodes[1].aggregator.last_weights[1].numpy()
        np.testing.assert_allclose(c, coef, rtol=1e-6)
        for nd in nodes:
            got = nd.learner.get_model().get_parameters()
            for a, b in zip(got, host_state):
                if np.issubdtype(np.asarray(a).dtype, np.floating):  # trainable tensors and running statistics
                    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=0, atol=1e-6)
        # the generic path ends in set_model: it takes the host aggregate, the 0-d batch counter included
        nodes[0].learner.set_model(host)
        for a, b in zip(nodes[0].learner.get_model().get_parameters(), host_state):
            assert np.shape(a) == np.shape(b)
            np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=0, atol=1e-6)
    finally:
        _stop(nodes)


def test_device_path_vote_counts_trainers_across_ranks():
    """More than 16 trainers in the round, or a peer without flat parameters on any rank, sends
    every rank to the generic path: decided from the gathered votes, not the local ones."""
    from types import SimpleNamespace

    from myfyp_amd.stages.collective.wait_agg_models_stage import _VOTED_KINDS, _agree_device_path

    assert "geometric_median" in _VOTED_KINDS and "geometric_median" in weights_plane.DEVICE_KINDS
    flat = SimpleNamespace(learner=SimpleNamespace(flat_params=lambda: None))
    plain = SimpleNamespace(learner=SimpleNamespace())

    def fed(local, others):
        return SimpleNamespace(local_nodes=local, all_gather_object=lambda mine: [mine, *others])

    arrived = {f"a{i}": (1 if i else 0, None) for i in range(9)}  # 8 trainers, one non-trainer
    local = {a: flat for a in arrived}
    kind = "geometric_median"
    assert _agree_device_path(fed(local, [(True, 8)]), kind, arrived)  # 16 in all
    assert not _agree_device_path(fed(local, [(True, 9)]), kind, arrived)  # 17: the other rank's count decides
    assert not _agree_device_path(fed(local, [(False, 1)]), kind, arrived)
    assert not _agree_device_path(fed({**local, "a3": plain}, [(True, 1)]), kind, arrived)


def test_seventeen_trainers_take_the_generic_path():
    """17 trainers: the vote ``join_aggregation``'s leader takes sends the round to the generic
    path, where every peer gets the host aggregate of the wire models."""
    from myfyp_amd.stages.collective import wait_agg_models_stage as stage

    k = 17
    fed, nodes = _start("cpu", [4], k=k)
    try:
        n = nodes[0].learner.flat_params().numel()
        g = torch.Generator().manual_seed(3)
        base = torch.randn(n, generator=g)
        samples = [1 + i % 3 for i in range(k)]
        for nd in nodes:
            with torch.no_grad():
                nd.learner.flat_params().copy_(base + 1e-3 * torch.randn(n, generator=g))
        wire = _wire(nodes, range(k), samples)
        want = GeometricMedian(iters=3).aggregate(wire)
        want_flat = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in want.get_parameters()])
        arrived = {nd.addr: (float(s), None) for nd, s in zip(nodes, samples)}
        assert not stage._agree_device_path(fed, "geometric_median", arrived)
        assert stage._agree_device_path(fed, "geometric_median", dict(list(arrived.items())[:16]))
        weights_plane.aggregate_generic(fed, {nd.addr: (float(s), m) for nd, s, m in zip(nodes, samples, wire)}, nodes[0].aggregator)
        for nd in nodes:
            np.testing.assert_allclose(_flat64(nd.learner.flat_params()), want_flat[:n], rtol=0, atol=1e-6)
    finally:
        _stop(nodes)


@pytest.mark.gpu
def test_geomed_device_plane_gpu(monkeypatch):
    _case("cuda", None, monkeypatch)  # default MLP: rows of the fused engine's stacked buffer


def _two_ranks(env=None):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "workers", "geomed_agg_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("OK") == 2


@pytest.mark.slow
def test_geomed_two_ranks_gloo():
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cpu"))  # CPU tensors also on a GPU host


@pytest.mark.gpu
def test_geomed_two_ranks_gpu():
    """2 ranks x 3 peers on the fused engine (one MI355X: gloo carries the cross-rank collectives,
    RCCL refuses two ranks per device)."""
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cuda", HSA_ENABLE_IPC_MODE_LEGACY="0"))
