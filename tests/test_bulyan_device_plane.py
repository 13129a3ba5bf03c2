"""Bulyan on the collective plane (``weights_plane.aggregate_bulyan``) against the host aggregator on
wire copies of the same models and against the definition (``bulyan_numpy``).

The device path never builds wire models: the trainers' flat rows are measured and picked by the
kernels behind ``ops.bulyan_into`` and the per-coordinate result is written into every local peer.
CPU (in-process, and a 2-device host mesh) here, the same checks on ``cuda:0`` under the gpu marker
(fused MLP engine rows), and a 2-rank gloo run through ``tests/workers``.

Tolerance: device and oracle take the same window per coordinate and each is within
``β·2^-24·max|x|`` of its float64 mean (``tests/test_bulyan_kernels_gpu.py``), so they are within
twice that of each other; off the GPU both are the same fp32 operations and agree bit for bit.
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
from myfyp_amd.learning.aggregators import Bulyan
from myfyp_amd.learning.aggregators.bulyan import bulyan_numpy
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP
from myfyp_amd.node import Node
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [4.0, 0.0, 2.0, 1.0, 3.0, 1.0, 2.0, 5.0, 1.0]  # peer 1 is a non-trainer: K = 8
FLIPPED = 3  # a trainer
F = 1
U = 2.0**-24


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


def _nodes(k, hidden, module=None, f=F):
    data = synthetic_mnist(200, 50)
    tag = time.time_ns()
    if module is None:
        module = (lambda i: MLP(seed=i)) if hidden is None else (lambda i: MLP(hidden_sizes=hidden, seed=i))
    return [Node(TorchModel(module(i)), data, address=f"bl{tag}-{i}", aggregator=Bulyan(num_byzantine=f), protocol=CollectiveCommunicationProtocol)
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
        rows.append(r.numpy())
    return rows


def _wire(nodes, idx, weights):
    return [nodes[i].learner.get_model().build_copy(params=[p.copy() for p in nodes[i].learner.get_model().get_parameters()], num_samples=int(weights[i]),
                                                    contributors=[nodes[i].addr]) for i in idx]


def _start(device, hidden, module=None, devices=None, k=len(WEIGHTS), f=F):
    Settings.DEVICE = device
    Federation.reset()
    fed = Federation.init(devices=devices) if devices else Federation.init()
    nodes = _nodes(k, hidden, module, f)
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
        weights_plane.aggregate_bulyan(fed, {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}, nodes[0].aggregator)
        # row order: the trainers in local order (on a mesh: device by device). The order matters:
        # the last picks score by one nearest row, so the two closest rows left tie exactly and
        # the lower row wins. Every rank and device reduces the same order.
        order = [[nd.addr for nd in nodes].index(a) for a in nodes[0].aggregator.last_selection[0]]
        assert sorted(order) == tr and (devices or order == tr)
        x = np.stack([rows[i] for i in order])
        exp, coef, pick, _, _ = bulyan_numpy(list(x), F)
        assert coef[order.index(FLIPPED)] == 0 and int((coef != 0).sum()) == len(tr) - 2 * F  # the definition rejects the flipped trainer
        atol = 2 * (len(tr) - 4 * F) * U * float(np.abs(x).max())
        for nd in nodes:  # the non-trainer (weight 0) receives the aggregate too
            np.testing.assert_allclose(_flat64(nd.learner.flat_params()), exp, rtol=0, atol=atol)
        for nd in nodes:
            addrs, c = nd.aggregator.last_selection
            assert addrs == [nodes[i].addr for i in order]
            assert c.device.type == nd.learner.flat_params().device.type  # stayed on the device
            assert np.array_equal(c.cpu().numpy(), coef)
            assert getattr(nd.aggregator, "last_weights", None) is None
        _close_rows(nodes, seed=9)  # the same models again, for the host aggregator on wire copies in that order
        host = Bulyan(num_byzantine=F).aggregate(_wire(nodes, order, WEIGHTS))
        host_flat = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in host.get_parameters()])
        np.testing.assert_allclose(host_flat[: exp.size], exp, rtol=0, atol=atol)
    finally:
        _stop(nodes)


def test_bulyan_device_plane_cpu(monkeypatch):
    _case("cpu", [8, 8], monkeypatch)


def test_bulyan_device_plane_cpu_mesh(monkeypatch):
    """Two host-mesh devices: ``_mesh_robust`` (one mesh all-gather, the op per device)."""
    _case("cpu", [8, 8], monkeypatch, devices=["cpu", "cpu"])


def test_bulyan_batchnorm_buffers_cpu(monkeypatch):
    """``get_parameters()`` is the whole ``state_dict``: the host ``Bulyan`` also measures BatchNorm's
    running statistics and its integer batch counter, so the device rows carry them too (the packed
    path). One trainer's counter is far from the others': both must reject it, where the flat
    parameters alone would pick it."""
    fed, nodes = _start("cpu", None, module=lambda i: _BNNet(seed=i))
    try:
        _no_generic(monkeypatch)
        _close_rows(nodes, seed=13, flipped=None)
        g = torch.Generator().manual_seed(17)
        tr = [i for i, w in enumerate(WEIGHTS) if w > 0]
        flats = [_flat64(nodes[i].learner.flat_params()).astype(np.float32) for i in tr]
        _, coef_flat, pick_flat, _, _ = bulyan_numpy(flats, F)
        odd = tr[int(np.argmin(np.where(pick_flat >= 0, pick_flat, 99)))]  # the first row the parameters alone pick
        for i, nd in enumerate(nodes):
            bn = nd.learner.model.get_model().bn
            with torch.no_grad():
                bn.running_mean.copy_(0.01 * torch.randn(8, generator=g))
                bn.running_var.copy_(1 + 0.01 * torch.randn(8, generator=g))
                bn.num_batches_tracked.fill_(40 if i == odd else 3)
        full = [np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in nodes[i].learner.get_model().get_parameters()]) for i in tr]
        _, coef, _, _, _ = bulyan_numpy(full, F)
        o = tr.index(odd)
        assert coef_flat[o] != 0 and coef[o] == 0  # the buffers decide
        host = Bulyan(num_byzantine=F).aggregate(_wire(nodes, tr, WEIGHTS))
        host_state = host.get_parameters()
        weights_plane.aggregate_bulyan(fed, {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}, nodes[0].aggregator)
        c = nodes[1].aggregator.last_selection[1].numpy()
        assert np.array_equal(c, coef)
        for nd in nodes:
            got = nd.learner.get_model().get_parameters()
            for a, b in zip(got, host_state):
                if np.issubdtype(np.asarray(a).dtype, np.floating):  # trainable tensors and running statistics
                    assert np.array_equal(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32))
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

    assert "bulyan" in _VOTED_KINDS and "bulyan" in weights_plane.DEVICE_KINDS
    flat = SimpleNamespace(learner=SimpleNamespace(flat_params=lambda: None))
    plain = SimpleNamespace(learner=SimpleNamespace())

    def fed(local, others):
        return SimpleNamespace(local_nodes=local, all_gather_object=lambda mine: [mine, *others])

    arrived = {f"a{i}": (1 if i else 0, None) for i in range(9)}  # 8 trainers, one non-trainer
    local = {a: flat for a in arrived}
    kind = "bulyan"
    assert _agree_device_path(fed(local, [(True, 8)]), kind, arrived)  # 16 in all
    assert not _agree_device_path(fed(local, [(True, 9)]), kind, arrived)  # 17: the other rank's count decides
    assert not _agree_device_path(fed(local, [(False, 1)]), kind, arrived)
    assert not _agree_device_path(fed({**local, "a3": plain}, [(True, 1)]), kind, arrived)


def test_seventeen_trainers_take_the_generic_path():
    """17 trainers: the vote ``join_aggregation``'s leader takes sends the round to the generic
    path, where every peer gets the host aggregate of the wire models: ``bulyan_numpy``'s."""
    from myfyp_amd.stages.collective import wait_agg_models_stage as stage

    k, f = 17, 3
    fed, nodes = _start("cpu", [4], k=k, f=f)
    try:
        n = nodes[0].learner.flat_params().numel()
        g = torch.Generator().manual_seed(3)
        base = torch.randn(n, generator=g)
        samples = [1 + i % 3 for i in range(k)]
        for i, nd in enumerate(nodes):
            with torch.no_grad():
                nd.learner.flat_params().copy_((-1 if i == 11 else 1) * (base + 1e-3 * torch.randn(n, generator=g)))
        order = sorted(range(k), key=lambda i: nodes[i].addr)  # the generic path's row order (ties go to the lower row)
        want, coef, _, _, _ = bulyan_numpy([nodes[i].learner.flat_params().detach().numpy().copy() for i in order], f)
        assert coef[order.index(11)] == 0 and int((coef != 0).sum()) == k - 2 * f
        wire = _wire(nodes, range(k), samples)
        arrived = {nd.addr: (float(s), None) for nd, s in zip(nodes, samples)}
        assert not stage._agree_device_path(fed, "bulyan", arrived)
        assert stage._agree_device_path(fed, "bulyan", dict(list(arrived.items())[:16]))
        weights_plane.aggregate_generic(fed, {nd.addr: (float(s), m) for nd, s, m in zip(nodes, samples, wire)}, nodes[0].aggregator)
        for nd in nodes:
            assert np.array_equal(nd.learner.flat_params().detach().numpy(), want)
        addrs, c = nodes[0].aggregator.last_selection
        assert addrs == [nodes[i].addr for i in order]
        assert np.array_equal(np.asarray(c), coef)
    finally:
        _stop(nodes)


@pytest.mark.parametrize("devices", [None, ["cpu", "cpu"]])
def test_too_few_trainers_raise_before_any_collective(monkeypatch, devices):
    """K < 4f + 3 for the round's trainers: the host aggregator's ``ValueError`` from the gathered K,
    before a tensor collective and before any row is written (every rank holds the same K, so all
    raise or none does: two ranks in ``tests/workers/bulyan_agg_worker.py``)."""
    fed, nodes = _start("cpu", [8, 8], devices=devices)
    try:
        rows = _close_rows(nodes, seed=21)
        weights = [1.0] * 6 + [0.0] * 3  # K = 6 < 7

        def no_collective(*a, **k):
            raise AssertionError("a tensor collective ran")

        monkeypatch.setattr(fed, "all_gather_into_tensor_", no_collective, raising=False)
        if fed.mesh is not None:
            monkeypatch.setattr(fed.mesh, "all_gather_", no_collective, raising=False)
        with pytest.raises(ValueError, match=r"4f \+ 3.*K = 6.*f = 1"):
            weights_plane.aggregate_bulyan(fed, {nd.addr: (w, None) for nd, w in zip(nodes, weights)}, nodes[0].aggregator)
        for nd, r in zip(nodes, rows):
            assert np.array_equal(nd.learner.flat_params().detach().numpy(), r)
            assert nd.aggregator.last_selection is None
    finally:
        _stop(nodes)


@pytest.mark.gpu
def test_bulyan_device_plane_gpu(monkeypatch):
    _case("cuda", None, monkeypatch)  # default MLP: rows of the fused engine's stacked buffer


def _two_ranks(env=None):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "workers", "bulyan_agg_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("OK") == 2


@pytest.mark.slow
def test_bulyan_two_ranks_gloo():
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cpu"))  # CPU tensors also on a GPU host


@pytest.mark.gpu
def test_bulyan_two_ranks_gpu():
    """2 ranks x 4 peers on the fused engine (one MI355X: gloo carries the cross-rank collectives,
    RCCL refuses two ranks per device)."""
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cuda", HSA_ENABLE_IPC_MODE_LEGACY="0"))
