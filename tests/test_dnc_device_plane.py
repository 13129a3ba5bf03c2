"""DnC on the collective plane (``weights_plane.aggregate_dnc``) against the host aggregator on wire
copies of the same models and against the definition (``dnc_numpy``).

The device path never builds wire models: the trainers' flat rows are measured and filtered by the
kernels behind ``ops.dnc_into`` and the weighted mean of the rows kept is written into every local
peer. CPU (in-process, and a 2-device host mesh) here, the same checks on ``cuda:0`` under the gpu
marker (fused MLP engine rows), and a 2-rank gloo run through ``tests/workers``.

Rows: honest peers one shared model plus 1e-3 of noise, two colluding trainers at μ − 3γσ of the
honest rows (γ min-max's): the oracle's removed scores are several times the kept ones, so device
and oracle remove the same peers. Tolerance: each side is within ``kept·2^-24·max|x|`` of the
float64 ``Σ coef_k·x_k`` (``tests/test_dnc_kernels_gpu.py``), so they are within twice that of each
other.
"""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

from _ports import free_port
import torch

import _collude_ref as cref
import _dnc_ref as ref
from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol
from myfyp_amd.learning.aggregators import DnC
from myfyp_amd.learning.aggregators.dnc import dnc_numpy
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP
from myfyp_amd.node import Node
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [4.0, 0.0, 2.0, 1.0, 3.0, 1.0, 2.0, 5.0, 1.0]  # peer 1 is a non-trainer: K = 8
BAD = [3, 6]  # colluding trainers
F = 2
PARAMS = dict(num_byzantine=F, filter_frac=1.0, iters=2, subsample_dims=2000, seed=3)
U = 2.0**-24


def _nodes(k, hidden, params=PARAMS):
    data = synthetic_mnist(200, 50)
    tag = time.time_ns()
    module = (lambda i: MLP(seed=i)) if hidden is None else (lambda i: MLP(hidden_sizes=hidden, seed=i))
    return [Node(TorchModel(module(i)), data, address=f"dn{tag}-{i}", aggregator=DnC(**params), protocol=CollectiveCommunicationProtocol)
            for i in range(k)]


def _flat64(t):
    return t.detach().double().cpu().numpy().ravel()


def _attacked_rows(nodes, seed, bad=BAD, gs=3.0, weights=WEIGHTS):
    """Every peer one shared model plus 1e-3 of noise; the peers ``bad`` all hold μ − gs·γ·σ of the others' rows."""
    rng = np.random.default_rng(seed)
    n = nodes[0].learner.flat_params().numel()
    base = rng.standard_normal(n)
    rows = [(base + 1e-3 * rng.standard_normal(n)).astype(np.float32) for _ in nodes]
    honest = np.stack([r for i, r in enumerate(rows) if i not in bad and weights[i] > 0]).astype(np.float64)
    _, g, st = cref.oracle(honest, "min_max")
    for i in bad:
        rows[i] = (st["mu"] - gs * g * st["sigma"]).astype(np.float32)
    for nd, r in zip(nodes, rows):
        with torch.no_grad():
            nd.learner.flat_params().copy_(torch.from_numpy(r))
    return rows


def _wire(nodes, idx, weights):
    return [nodes[i].learner.get_model().build_copy(params=[p.copy() for p in nodes[i].learner.get_model().get_parameters()], num_samples=int(weights[i]),
                                                    contributors=[nodes[i].addr]) for i in idx]


def _start(device, hidden, devices=None, k=len(WEIGHTS), params=PARAMS):
    Settings.DEVICE = device
    Federation.reset()
    fed = Federation.init(devices=devices) if devices else Federation.init()
    nodes = _nodes(k, hidden, params)
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


def _definition(x, ws, rnd):
    p = PARAMS
    return dnc_numpy(list(x), ws, p["num_byzantine"], p["filter_frac"], p["iters"], p["subsample_dims"], p["seed"], rnd)


def _case(device, hidden, monkeypatch, devices=None):
    fed, nodes = _start(device, hidden, devices=devices)
    try:
        _no_generic(monkeypatch)
        rows = _attacked_rows(nodes, seed=9)
        assert rows[0].size > PARAMS["subsample_dims"]  # a real subsample
        tr = [i for i, w in enumerate(WEIGHTS) if w > 0]
        rnd = 4
        weights_plane.aggregate_dnc(fed, {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}, nodes[0].aggregator, rnd)
        order = [[nd.addr for nd in nodes].index(a) for a in nodes[0].aggregator.last_selection[0]]
        assert sorted(order) == tr and (devices or order == tr)
        x = np.stack([rows[i] for i in order])
        ws = [WEIGHTS[i] for i in order]
        exp, coef, removed, dist, score, _ = _definition(x, ws, rnd)
        assert sorted(order[i] for i in np.flatnonzero(removed >= 0)) == BAD  # the definition removes the colluders
        for t in range(PARAMS["iters"]):
            assert ref.margin(score[t], F) >= 2.0 and ref.eig_ratio(ref.gram(dist[t])) <= 0.9  # and not by a coin toss
        atol = 2 * int((coef != 0).sum()) * U * float(np.abs(x).max())
        for nd in nodes:  # the non-trainer (weight 0) receives the aggregate too
            np.testing.assert_allclose(_flat64(nd.learner.flat_params()), exp, rtol=0, atol=atol)
        for nd in nodes:
            assert nd.aggregator.round == rnd
            addrs, c = nd.aggregator.last_selection
            assert addrs == [nodes[i].addr for i in order]
            assert c.device.type == nd.learner.flat_params().device.type  # stayed on the device
            assert np.array_equal(c.cpu().numpy(), coef)
        _attacked_rows(nodes, seed=9)  # the same models again, for the host aggregator on wire copies in that order
        host_agg = DnC(**PARAMS)
        host_agg.round = rnd
        host = host_agg.aggregate(_wire(nodes, order, WEIGHTS))
        host_flat = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in host.get_parameters()])
        np.testing.assert_allclose(host_flat[: exp.size], exp, rtol=0, atol=atol)
        assert np.array_equal(np.asarray(host_agg.last_selection[1]), coef)
    finally:
        _stop(nodes)


def test_dnc_device_plane_cpu(monkeypatch):
    _case("cpu", [8, 8], monkeypatch)


def test_dnc_device_plane_cpu_mesh(monkeypatch):
    """Two host-mesh devices: ``_mesh_robust`` (one mesh all-gather, the op per device)."""
    _case("cpu", [8, 8], monkeypatch, devices=["cpu", "cpu"])


def test_the_subsample_changes_with_the_round(monkeypatch):
    fed, nodes = _start("cpu", [8, 8])
    try:
        _no_generic(monkeypatch)
        seen = []
        real = weights_plane.ops.dnc_into

        def spy(rows, outs, ws, *a, **k):
            res = real(rows, outs, ws, *a, **k)
            seen.append((a[-1], res[0].clone()))  # (round, dist)
            return res

        monkeypatch.setattr(weights_plane.ops, "dnc_into", spy)
        arrived = {nd.addr: (w, None) for nd, w in zip(nodes, WEIGHTS)}
        for rnd in (0, 1, 1):
            _attacked_rows(nodes, seed=9)
            weights_plane.aggregate_dnc(fed, arrived, nodes[0].aggregator, rnd)
            assert all(nd.aggregator.round == rnd for nd in nodes)
        assert [r for r, _ in seen] == [0, 1, 1]
        assert not torch.equal(seen[0][1], seen[1][1]) and torch.equal(seen[1][1], seen[2][1])
    finally:
        _stop(nodes)


def test_device_path_vote_counts_trainers_across_ranks():
    """More than 16 trainers in the round, or a peer without flat parameters on any rank, sends
    every rank to the generic path: decided from the gathered votes, not the local ones."""
    from types import SimpleNamespace

    from myfyp_amd.stages.collective.wait_agg_models_stage import _VOTED_KINDS, _agree_device_path

    assert "dnc" in _VOTED_KINDS and "dnc" in weights_plane.DEVICE_KINDS
    flat = SimpleNamespace(learner=SimpleNamespace(flat_params=lambda: None))
    plain = SimpleNamespace(learner=SimpleNamespace())

    def fed(local, others):
        return SimpleNamespace(local_nodes=local, all_gather_object=lambda mine: [mine, *others])

    arrived = {f"a{i}": (1 if i else 0, None) for i in range(9)}  # 8 trainers, one non-trainer
    local = {a: flat for a in arrived}
    kind = "dnc"
    assert _agree_device_path(fed(local, [(True, 8)]), kind, arrived)  # 16 in all
    assert not _agree_device_path(fed(local, [(True, 9)]), kind, arrived)  # 17: the other rank's count decides
    assert not _agree_device_path(fed(local, [(False, 1)]), kind, arrived)
    assert not _agree_device_path(fed({**local, "a3": plain}, [(True, 1)]), kind, arrived)


def test_seventeen_trainers_take_the_generic_path():
    """17 trainers: the vote ``join_aggregation``'s leader takes sends the round to the generic
    path, where every peer gets the host aggregate of the wire models: ``dnc_numpy``'s."""
    from myfyp_amd.stages.collective import wait_agg_models_stage as stage

    k = 17
    params = dict(num_byzantine=3, subsample_dims=None)
    fed, nodes = _start("cpu", [4], k=k, params=params)
    try:
        samples = [1 + i % 3 for i in range(k)]
        rows = _attacked_rows(nodes, seed=3, bad=[2, 7, 11], weights=samples)
        order = sorted(range(k), key=lambda i: nodes[i].addr)  # the generic path's row order
        want, coef, removed, _, _, _ = dnc_numpy([rows[i] for i in order], [float(samples[i]) for i in order], 3, subsample_dims=None)
        assert sorted(order[i] for i in np.flatnonzero(removed >= 0)) == [2, 7, 11]
        wire = _wire(nodes, range(k), samples)
        arrived = {nd.addr: (float(s), None) for nd, s in zip(nodes, samples)}
        assert not stage._agree_device_path(fed, "dnc", arrived)
        assert stage._agree_device_path(fed, "dnc", dict(list(arrived.items())[:16]))
        weights_plane.aggregate_generic(fed, {nd.addr: (float(s), m) for nd, s, m in zip(nodes, samples, wire)}, nodes[0].aggregator)
        for nd in nodes:
            assert np.array_equal(nd.learner.flat_params().detach().numpy(), want)
        addrs, c = nodes[0].aggregator.last_selection
        assert addrs == [nodes[i].addr for i in order]
        assert np.array_equal(np.asarray(c), coef)
    finally:
        _stop(nodes)


@pytest.mark.parametrize("devices", [None, ["cpu", "cpu"]])
def test_bad_parameters_raise_before_any_collective(monkeypatch, devices):
    """iters · m >= K for the round's trainers: ``ValueError`` from the gathered K, before a tensor
    collective and before any row is written (every rank holds the same K, so all raise or none
    does: two ranks in ``tests/workers/dnc_agg_worker.py``)."""
    fed, nodes = _start("cpu", [8, 8], devices=devices)
    try:
        rows = _attacked_rows(nodes, seed=21)
        weights = [1.0] * 4 + [0.0] * 5  # K = 4 = iters · m

        def no_collective(*a, **k):
            raise AssertionError("a tensor collective ran")

        monkeypatch.setattr(fed, "all_gather_into_tensor_", no_collective, raising=False)
        if fed.mesh is not None:
            monkeypatch.setattr(fed.mesh, "all_gather_", no_collective, raising=False)
        with pytest.raises(ValueError, match=r"K = 4, iters = 2"):
            weights_plane.aggregate_dnc(fed, {nd.addr: (w, None) for nd, w in zip(nodes, weights)}, nodes[0].aggregator, 0)
        for nd, r in zip(nodes, rows):
            assert np.array_equal(nd.learner.flat_params().detach().numpy(), r)
            assert nd.aggregator.last_selection is None
    finally:
        _stop(nodes)


@pytest.mark.gpu
def test_dnc_device_plane_gpu(monkeypatch):
    _case("cuda", None, monkeypatch)  # default MLP: rows of the fused engine's stacked buffer


def _two_ranks(env=None):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "workers", "dnc_agg_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("OK") == 2


@pytest.mark.slow
def test_dnc_two_ranks_gloo():
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cpu"))  # CPU tensors also on a GPU host


@pytest.mark.gpu
def test_dnc_two_ranks_gpu():
    """2 ranks x 4 peers on the fused engine (one MI355X: gloo carries the cross-rank collectives,
    RCCL refuses two ranks per device)."""
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cuda", HSA_ENABLE_IPC_MODE_LEGACY="0"))
