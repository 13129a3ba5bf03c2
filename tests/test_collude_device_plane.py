"""Colluding attacks on the collective plane (``weights_plane.collude``, installed by
``fault_injection.ColludingAttack``) against the float64 oracle (``tests/_collude_ref.py``).

The attackers' rows are rewritten in place from the honest trainers' rows: live flat rows where a
model is its flat vector, a packed copy (unpacked into the attackers) where it has buffers. CPU
(in-process, and a 2-device host mesh) here, the same checks on ``cuda:0`` under the gpu marker
(fused MLP engine rows), and a 2-rank gloo run through ``tests/workers``.

Tolerance: off the GPU the op is the float64 definition rounded once to fp32 (``2^-23·max|m|``
covers that rounding and the oracle's own float64 error); on the GPU the per-coordinate bound of
``tests/test_collude_kernels_gpu.py``.
"""

import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import _collude_ref as cr
from _ports import free_port
from myfyp_amd import fault_injection
from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol
from myfyp_amd.learning.aggregators import Krum
from myfyp_amd.learning.aggregators.neighbor_avg import NeighborAvg
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP
from myfyp_amd.node import Node
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [4.0, 0.0, 2.0, 1.0, 3.0, 1.0, 2.0, 5.0, 0.0]  # peers 1 and 8 are non-trainers
ATTACKERS = [2, 6, 8]  # 8 did not train: it is left alone; H = 5 honest trainers, 2 attackers


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


def _start(device, hidden, module=None, devices=None, k=len(WEIGHTS), aggregator=lambda: Krum(num_byzantine=2)):
    Settings.DEVICE = device
    Federation.reset()
    fed = Federation.init(devices=devices) if devices else Federation.init()
    data = synthetic_mnist(200, 50)
    tag = time.time_ns()
    if module is None:
        module = (lambda i: MLP(seed=i)) if hidden is None else (lambda i: MLP(hidden_sizes=hidden, seed=i))
    nodes = [Node(TorchModel(module(i)), data, address=f"co{tag}-{i}", aggregator=aggregator(), protocol=CollectiveCommunicationProtocol) for i in range(k)]
    for nd in nodes:
        nd.start()
    fed.finalize()
    return fed, nodes


def _stop(nodes):
    for nd in nodes:
        nd.stop()
    Federation.reset()
    Settings.DEVICE = "auto"


def _close_rows(nodes, seed):
    """Every peer one shared model plus ~1e-3 of noise."""
    g = torch.Generator().manual_seed(seed)
    n = nodes[0].learner.flat_params().numel()
    base = torch.randn(n, generator=g)
    rows = []
    for i, nd in enumerate(nodes):
        r = base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g)
        with torch.no_grad():
            nd.learner.flat_params().copy_(r)
        rows.append(r.numpy())
    return rows


def _flat(nd):
    return nd.learner.flat_params().detach().cpu().numpy()


def _case(device, hidden, kind, devices=None):
    fed, nodes = _start(device, hidden, devices=devices)
    attack = None
    try:
        addrs = [nd.addr for nd in nodes]
        attack = fault_injection.ColludingAttack(fed, [nodes[i] for i in ATTACKERS], kind, z=1.0)
        rows = _close_rows(nodes, seed=9)
        ref = None
        if kind == "ipm":  # the round-start model: every peer holds one model then
            start = rows[0] + np.float32(2e-3)
            for nd in nodes:
                with torch.no_grad():
                    nd.learner.flat_params().copy_(torch.from_numpy(start))
            for hook in list(fed.round_start_hooks):
                hook(0, fed)
            rows = _close_rows(nodes, seed=9)
            ref = start.astype(np.float64)
        weights = {a: w for a, w in zip(addrs, WEIGHTS)}
        assert len(fed.pre_aggregation_hooks) == 1
        fed.pre_aggregation_hooks[0](0, fed, weights)
        honest, attacking, gamma, stat = attack.last
        order = [addrs.index(a) for a in honest]
        want_honest = [i for i, w in enumerate(WEIGHTS) if w > 0 and i not in ATTACKERS]
        assert sorted(order) == want_honest and (devices or order == want_honest)  # a mesh orders device by device
        assert sorted(attacking) == sorted(addrs[i] for i in ATTACKERS if WEIGHTS[i] > 0)
        assert gamma.device.type == nodes[0].learner.flat_params().device.type  # stayed on the device
        x64 = np.stack([rows[i] for i in order]).astype(np.float64)
        m, g, st = cr.oracle(x64, kind, n_out=2, z=1.0, ref=ref)
        if device == "cpu":
            atol = np.full_like(m, 2.0**-23 * np.abs(m).max())
            gtol = 2.0**-23 * abs(g)
        else:
            n = x64.shape[1]
            solved = kind in ("min_max", "min_sum")
            gtol = cr.gamma_bound(x64, st, n, kind) if solved else 0.0
            ca, cb, c_r = (1.0, -g, 0.0) if solved else {"alie": (1.0, -1.0, 0.0), "ipm": (-0.5, 0.0, 1.5)}[kind]
            atol = cr.out_bound(x64, st, ca, cb, c_r, ref, gtol)
        assert abs(float(gamma.cpu()[0]) - g) <= gtol
        for i, nd in enumerate(nodes):
            if i in ATTACKERS and WEIGHTS[i] > 0:
                assert (np.abs(_flat(nd).astype(np.float64) - m) <= atol).all()
                assert np.array_equal(_flat(nd), _flat(nodes[ATTACKERS[0]]))  # one row for all attackers
            else:  # honest rows, non-trainers and the attacker that did not train are untouched
                assert np.array_equal(_flat(nd), rows[i])
        if kind in ("min_max", "min_sum"):
            lhs, rhs = cr.constraint(x64, _flat(nodes[ATTACKERS[0]]).astype(np.float64), kind)
            assert lhs <= rhs * (1 + 1e-4)
        # no honest trainer, or no attacker among the trainers: nothing happens
        attack.last = None
        before = [_flat(nd).copy() for nd in nodes]
        fed.pre_aggregation_hooks[0](1, fed, {a: (w if i in ATTACKERS else 0.0) for i, (a, w) in enumerate(zip(addrs, WEIGHTS))})
        fed.pre_aggregation_hooks[0](1, fed, {a: (0.0 if i in ATTACKERS else w) for i, (a, w) in enumerate(zip(addrs, WEIGHTS))})
        assert attack.last is None and attack.rounds == 3
        for nd, b in zip(nodes, before):
            assert np.array_equal(_flat(nd), b)
        attack.remove()
        assert not fed.pre_aggregation_hooks and not fed.round_start_hooks
    finally:
        if attack is not None:
            attack.remove()
        _stop(nodes)


@pytest.mark.parametrize("kind", cr.KINDS)
def test_collude_device_plane_cpu(kind):
    _case("cpu", [8, 8], kind)


@pytest.mark.parametrize("kind", ["min_max", "ipm"])
def test_collude_device_plane_cpu_mesh(kind):
    """Two host-mesh devices: ``_mesh_collude`` (one mesh all-gather, the op per device)."""
    _case("cpu", [8, 8], kind, devices=["cpu", "cpu"])


def test_collude_batchnorm_buffers_cpu():
    """A model with BatchNorm buffers goes through the packed path: the crafted row covers the
    running statistics too (the integer batch counter rides behind them, as in Krum's rows, and is
    not written back)."""
    fed, nodes = _start("cpu", None, module=lambda i: _BNNet(seed=i))
    attack = None
    try:
        _close_rows(nodes, seed=13)
        g = torch.Generator().manual_seed(17)
        for i, nd in enumerate(nodes):
            bn = nd.learner.model.get_model().bn
            with torch.no_grad():
                bn.running_mean.copy_(0.01 * torch.randn(8, generator=g))
                bn.running_var.copy_(1 + 0.01 * torch.randn(8, generator=g))
                bn.num_batches_tracked.fill_(3 + i)
        live, row_of = weights_plane._row_fns([nd.learner for nd in nodes], "krum")
        assert not live
        packed = [row_of(nd.learner).clone().numpy() for nd in nodes]
        attack = fault_injection.ColludingAttack(fed, [nodes[i].addr for i in ATTACKERS], "min_max")
        fed.pre_aggregation_hooks[0](0, fed, {nd.addr: w for nd, w in zip(nodes, WEIGHTS)})
        honest = [i for i, w in enumerate(WEIGHTS) if w > 0 and i not in ATTACKERS]
        assert attack.last[0] == [nodes[i].addr for i in honest]
        m, gam, _ = cr.oracle(np.stack([packed[i] for i in honest]).astype(np.float64), "min_max")
        assert abs(float(attack.last[2][0]) - gam) <= 2.0**-23 * gam
        n_state = sum(t.numel() for t in weights_plane.state_tensors(nodes[0].learner))
        assert n_state == packed[0].size - 1  # the batch counter is the row's last entry
        for i, nd in enumerate(nodes):
            got = weights_plane._pack(nd.learner).numpy()
            if i in ATTACKERS and WEIGHTS[i] > 0:
                np.testing.assert_allclose(got.astype(np.float64), m[:n_state], rtol=0, atol=2.0**-23 * np.abs(m).max())
                assert int(nd.learner.model.get_model().bn.num_batches_tracked) == 3 + i
            else:
                assert np.array_equal(got, packed[i][:n_state])
    finally:
        if attack is not None:
            attack.remove()
        _stop(nodes)


def test_ipm_refuses_neighbor_mixing_and_unknown_kinds():
    fed, nodes = _start("cpu", [4], k=3, aggregator=lambda: NeighborAvg())
    try:
        with pytest.raises(ValueError, match="NeighborAvg"):
            fault_injection.ColludingAttack(fed, [nodes[1]], "ipm")
        with pytest.raises(ValueError, match="unknown colluding attack"):
            fault_injection.ColludingAttack(fed, [nodes[1]], "sign_flip")
        assert not fed.pre_aggregation_hooks and not fed.round_start_hooks
        assert fault_injection.COLLUDING == ("alie", "ipm", "min_max", "min_sum")
        assert fault_injection.ATTACKS == ("sign_flip", "gaussian_noise", "scale")
    finally:
        _stop(nodes)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", cr.KINDS)
def test_collude_device_plane_gpu(kind):
    _case("cuda", None, kind)  # default MLP: rows of the fused engine's stacked buffer


def _two_ranks(env=None):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "workers", "collude_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("OK") == 2


@pytest.mark.slow
def test_collude_two_ranks_gloo():
    _two_ranks(dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cpu"))  # CPU tensors also on a GPU host
