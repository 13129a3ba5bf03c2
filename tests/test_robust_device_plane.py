"""Krum and TrimmedMean on the collective plane (``weights_plane.aggregate_krum`` /
``aggregate_trimmed_mean``) against the host aggregators on wire copies of the same models and
against the closed forms in float64 numpy.

The device path never builds wire models: the trainers' flat rows are measured, selected and
averaged by the kernels behind ``ops.krum_into`` / ``ops.trimmed_mean_into`` and written into every
local peer. CPU (in-process, and a 2-device host mesh) here, the same checks on ``cuda:0`` under the
gpu marker (fused MLP engine rows), and a 2-rank gloo run through ``tests/workers``.
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
from myfyp_amd.learning.aggregators import Krum, TrimmedMean
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP
from myfyp_amd.node import Node
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1.0, 0.0, 2.0, 3.0, 4.0]
FLIPPED = 3  # a trainer


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


def _nodes(make_agg, k, hidden, module=None):
    data = synthetic_mnist(200, 50)
    tag = time.time_ns()
    if module is None:
        module = (lambda i: MLP(seed=i)) if hidden is None else (lambda i: MLP(hidden_sizes=hidden, seed=i))
    return [Node(TorchModel(module(i)), data, address=f"rob{tag}-{i}", aggregator=make_agg(), protocol=CollectiveCommunicationProtocol) for i in range(k)]


def _flat64(t):
    return t.detach().double().cpu().numpy().ravel()


def _close_rows(nodes, seed):
    """Every peer one shared model plus ~1e-3 of noise; the trainer FLIPPED sends its negation."""
    g = torch.Generator().manual_seed(seed)
    n = nodes[0].learner.flat_params().numel()
    base = torch.randn(n, generator=g)
    rows = []
    for i, nd in enumerate(nodes):
        r = base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g)
        if i == FLIPPED:
            r = -r
        with torch.no_grad():
            nd.learner.flat_params().copy_(r)
        rows.append(r.double().numpy())
    return rows


def _wire(nodes, idx, weights):
    return [nodes[i].learner.get_model().build_copy(params=[p.copy() for p in nodes[i].learner.get_model().get_parameters()], num_samples=int(weights[i]),
                                                    contributors=[nodes[i].addr]) for i in idx]


def _krum_closed_form(x, w, f, m):
    """``Krum.aggregate`` in float64 over the vectors ``x`` (distances from differences)."""
    k = len(x)
    d = np.array([[((x[i] - x[j]) ** 2).sum() for j in range(k)] for i in range(k)])
    cnt = max(1, k - f - 2)
    scores = np.array([np.sort(np.delete(d[i], i))[:cnt].sum() for i in range(k)])
    chosen = sorted(np.argsort(scores, kind="stable")[: max(1, min(m, k))])
    tot = sum(w[i] for i in chosen)
    return chosen, [w[i] / tot if i in chosen else 0.0 for i in range(k)]


def _start(device, make_agg, hidden, module=None, devices=None, k=len(WEIGHTS)):
    Settings.DEVICE = device
    Federation.reset()
    fed = Federation.init(devices=devices) if devices else Federation.init()
    nodes = _nodes(make_agg, k, hidden, module)
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


def _krum_case(device, hidden, monkeypatch, devices=None):
    fed, nodes = _start(device, lambda: Krum(num_byzantine=1, multi=3), hidden, devices=devices)
    try:
        _no_generic(monkeypatch)
        rows = _close_rows(nodes, seed=9)
        tr = [i for i, w in enumerate(WEIGHTS) if w > 0]
        chosen, coef = _krum_closed_form([rows[i] for i in tr], [WEIGHTS[i] for i in tr], 1, 3)
        exp = sum(c * rows[i] for c, i in zip(coef, tr))
        assert tr.index(FLIPPED) not in chosen
        host = Krum(num_byzantine=1, multi=3).aggregate(_wire(nodes, tr, WEIGHTS))
        host_flat = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in host.get_parameters()])
        np.testing.assert_allclose(host_flat[: exp.size], exp, rtol=0, atol=1e-6)
        weights_plane.aggregate_krum(fed, {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}, nodes[0].aggregator)
        for nd in nodes:  # the non-trainer (weight 0) receives the aggregate too
            np.testing.assert_allclose(_flat64(nd.learner.flat_params()), exp, rtol=0, atol=1e-6)
        for nd in nodes:
            addrs, c = nd.aggregator.last_selection
            # row order: the trainers in local order (on a mesh: device by device)
            assert sorted(addrs) == sorted(nodes[i].addr for i in tr) and (devices or addrs == [nodes[i].addr for i in tr])
            assert c.device.type == nd.learner.flat_params().device.type  # stayed on the device
            by_addr = dict(zip(addrs, c.cpu().numpy()))
            assert by_addr[nodes[FLIPPED].addr] == 0
            np.testing.assert_allclose([by_addr[nodes[i].addr] for i in tr], coef, rtol=1e-6, atol=0)
    finally:
        _stop(nodes)


def _trimmed_case(device, hidden, k, monkeypatch, devices=None):
    fed, nodes = _start(device, lambda: TrimmedMean(beta=0.34), hidden, devices=devices, k=k)
    try:
        _no_generic(monkeypatch)
        weights = WEIGHTS[:k]
        rows = _close_rows(nodes, seed=11)
        tr = [i for i, w in enumerate(weights) if w > 0]
        trim = int(np.floor(0.34 * len(tr)))
        assert trim == 1
        exp = np.sort(np.stack([rows[i] for i in tr]), axis=0)[trim : len(tr) - trim].mean(axis=0)
        host = TrimmedMean(beta=0.34).aggregate(_wire(nodes, tr, [1.0] * k))
        host_flat = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in host.get_parameters()])
        np.testing.assert_allclose(host_flat[: exp.size], exp, rtol=0, atol=1e-6)
        arrived = {nd.addr: (w, None) for nd, w in zip(nodes, weights)}
        weights_plane.aggregate_trimmed_mean(fed, arrived, nodes[0].aggregator)
        for nd in nodes:
            np.testing.assert_allclose(_flat64(nd.learner.flat_params()), exp, rtol=0, atol=1e-6)
        # 2·trim >= K: the host aggregator's error, before anything is written
        with pytest.raises(ValueError, match="beta too large"):
            weights_plane.aggregate_trimmed_mean(fed, arrived, TrimmedMean(beta=0.7))
        for nd in nodes:
            np.testing.assert_allclose(_flat64(nd.learner.flat_params()), exp, rtol=0, atol=1e-6)
    finally:
        _stop(nodes)


def test_krum_device_plane_cpu(monkeypatch):
    _krum_case("cpu", [8, 8], monkeypatch)


@pytest.mark.parametrize("k", [4, 5])
def test_trimmed_device_plane_cpu(k, monkeypatch):
    _trimmed_case("cpu", [8, 8], k, monkeypatch)


def test_krum_device_plane_cpu_mesh(monkeypatch):
    """Two host-mesh devices: ``_mesh_robust`` (one mesh all-gather, the op per device)."""
    _krum_case("cpu", [8, 8], monkeypatch, devices=["cpu", "cpu"])


def test_trimmed_device_plane_cpu_mesh(monkeypatch):
    _trimmed_case("cpu", [8, 8], 5, monkeypatch, devices=["cpu", "cpu"])


def test_krum_batchnorm_buffers_cpu(monkeypatch):
    """``get_parameters()`` is the whole ``state_dict``: the host ``Krum`` also measures BatchNorm's
    running statistics and its integer batch counter. One trainer's counter is far from the others'
    while its weights are the closest of all: the host rejects it, and so must the device."""
    fed, nodes = _start("cpu", lambda: Krum(num_byzantine=1, multi=2), None, module=lambda i: _BNNet(seed=i))
    try:
        _no_generic(monkeypatch)
        _close_rows(nodes, seed=13)
        odd = 0  # the least noisy row: chosen first when only the weights are measured
        g = torch.Generator().manual_seed(17)
        for i, nd in enumerate(nodes):
            bn = nd.learner.model.get_model().bn
            with torch.no_grad():
                bn.running_mean.copy_(0.01 * torch.randn(8, generator=g))
                bn.running_var.copy_(1 + 0.01 * torch.randn(8, generator=g))
                bn.num_batches_tracked.fill_(40 if i == odd else 3)
        tr = [i for i, w in enumerate(WEIGHTS) if w > 0]
        full = [np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in nodes[i].learner.get_model().get_parameters()]) for i in tr]
        chosen, coef = _krum_closed_form(full, [WEIGHTS[i] for i in tr], 1, 2)
        assert tr.index(odd) not in chosen and tr.index(FLIPPED) not in chosen
        flats = [_flat64(nodes[i].learner.flat_params()) for i in tr]
        assert tr.index(odd) in _krum_closed_form(flats, [WEIGHTS[i] for i in tr], 1, 2)[0]  # the buffers decide
        host = Krum(num_byzantine=1, multi=2).aggregate(_wire(nodes, tr, WEIGHTS))
        host_state = host.get_parameters()
        weights_plane.aggregate_krum(fed, {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}, nodes[0].aggregator)
        c = nodes[1].aggregator.last_selection[1].numpy()
        np.testing.assert_array_equal(c != 0, np.array(coef) != 0)
        for nd in nodes:
            got = nd.learner.get_model().get_parameters()
            for a, b in zip(got, host_state):
                if np.issubdtype(np.asarray(a).dtype, np.floating):  # trainable tensors and running statistics
                    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=0, atol=1e-6)
        # the generic path (more than 16 trainers, a peer without flat parameters) ends in set_model:
        # it takes the host aggregate of such a model, the 0-d batch counter included
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

    from myfyp_amd.stages.collective.wait_agg_models_stage import _agree_device_path

    flat = SimpleNamespace(learner=SimpleNamespace(flat_params=lambda: None))
    plain = SimpleNamespace(learner=SimpleNamespace())

    def fed(local, others):
        return SimpleNamespace(local_nodes=local, all_gather_object=lambda mine: [mine, *others])

    arrived = {f"a{i}": (1 if i else 0, None) for i in range(9)}  # 8 trainers, one non-trainer
    local = {a: flat for a in arrived}
    for kind in ("krum", "trimmed_mean"):
        assert _agree_device_path(fed(local, [(True, 8)]), kind, arrived)  # 16 in all
        assert not _agree_device_path(fed(local, [(True, 9)]), kind, arrived)  # 17: the other rank's count decides
        assert not _agree_device_path(fed(local, [(False, 1)]), kind, arrived)
        assert not _agree_device_path(fed({**local, "a3": plain}, [(True, 1)]), kind, arrived)
    assert _agree_device_path(fed(local, [True]), "median", arrived)  # the other kinds vote as before


@pytest.mark.gpu
def test_krum_device_plane_gpu(monkeypatch):
    _krum_case("cuda", None, monkeypatch)  # default MLP: rows of the fused engine's stacked buffer


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 5])
def test_trimmed_device_plane_gpu(k, monkeypatch):
    _trimmed_case("cuda", None, k, monkeypatch)


def _two_ranks(env=None):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "workers", "robust_agg_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("OK") == 2


@pytest.mark.slow
def test_krum_trimmed_two_ranks_gloo():
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cpu"))  # CPU tensors also on a GPU host


@pytest.mark.gpu
def test_krum_trimmed_two_ranks_gpu():
    """2 ranks x 3 peers on the fused engine (one MI355X: gloo carries the cross-rank collectives,
    RCCL refuses two ranks per device)."""
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cuda", HSA_ENABLE_IPC_MODE_LEGACY="0"))
