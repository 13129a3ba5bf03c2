"""ClippedGossip on the collective plane (``weights_plane.aggregate_neighbors`` with a
``ClippedGossip``) against the float64 oracle (``tests/_clip_ref.py``) on copies of the same rows.

A ring of 6 peers whose rows are one model plus 1e-3 of noise; one peer holds −10 times the model.
CPU (in-process: the packed rows, and a 2-device host mesh) here, the same checks on ``cuda:0``
under the gpu marker (the default MLP: rows of the fused engine's stacked buffer, mixed in place), and a 2-rank
gloo run through ``tests/workers/clipped_gossip_worker.py``.

Tolerances. The rows: the per-element bound of the fp32 mix derived in ``tests/_clip_ref.py``,
against the oracle fed the plane's own ``w_eff`` (off the GPU the result is the float64 value
rounded once to fp32: inside the bound's first term). ``w_eff`` against the oracle's: rtol 2e-5,
the kernel test's bound. How far a row moves: no farther than ``Σ_q W_pq·min(d_pq, τ_p)``, the
definition's bound, where the plain mix moves it by ``|Σ_q W_pq (x_q − x_p)|``: both are asserted.
"""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

from _ports import free_port
import torch

import _clip_ref as ref
from myfyp_amd import ops
from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol
from myfyp_amd.learning.aggregators import ClippedGossip, NeighborAvg
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP
from myfyp_amd.node import Node
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 6
BAD = 2  # index in peer order
# the rows compared with the oracle's plan: from −10·base every honest row is equally far (to 1e-5),
# so which neighbour the attacker itself sets aside is a coin toss; what it does to its own row is
# still checked against the oracle fed the plane's own w_eff
HONEST = [i for i in range(K) if i != BAD]


def _start(device, devices=None, **agg):
    Settings.DEVICE = device
    Federation.reset()
    fed = Federation.init(devices=devices) if devices else Federation.init()
    data = synthetic_mnist(200, 50)
    tag = time.time_ns()
    # on the GPU the default MLP: the shape the fused engine takes, so the peers are rows of one stacked buffer
    module = (lambda i: MLP(seed=i)) if device == "cuda" else (lambda i: MLP(hidden_sizes=[8, 8], seed=i))
    nodes = [Node(TorchModel(module(i)), data, address=f"cg{tag}-{i}", aggregator=ClippedGossip(topology="ring", **agg),
                  protocol=CollectiveCommunicationProtocol) for i in range(K)]
    for nd in nodes:
        nd.start()
    fed.finalize()
    peers = fed.all_peers()
    return fed, sorted(nodes, key=lambda nd: peers.index(nd.addr))  # nodes in peer (row) order


def _stop(nodes):
    for nd in nodes:
        nd.stop()
    Federation.reset()
    Settings.DEVICE = "auto"


def _set_rows(nodes, seed=3):
    """Honest rows base + 1e-3 noise, row BAD = −10·base; float32 [K][n] in peer order."""
    rng = np.random.default_rng(seed)
    n = nodes[0].learner.flat_params().numel()
    base = rng.standard_normal(n)
    x32 = np.stack([base + 1e-3 * rng.standard_normal(n) for _ in nodes]).astype(np.float32)
    x32[BAD] = (-10.0 * base).astype(np.float32)
    for nd, r in zip(nodes, x32):
        with torch.no_grad():
            nd.learner.flat_params().copy_(torch.from_numpy(r.copy()))
    return x32


def _rows(nodes):
    return np.stack([nd.learner.flat_params().detach().cpu().numpy() for nd in nodes])


def _shares(w, present):
    """W of the clipped mix over the present peers, as ``_neighbors`` folds an absent source's share
    back: row i's weights over its present sources (itself included) renormalised, the diagonal dropped."""
    k = len(present)
    out = np.zeros((k, k))
    for r, i in enumerate(present):
        total = sum(w[i, j] for j in present if w[i, j] != 0)
        for c, j in enumerate(present):
            if j != i and w[i, j] != 0:
                out[r, c] = w[i, j] / total
    return out.astype(np.float32)


def _check_rows(got, x32, w_eff, what, rows=None):
    rows = list(range(len(x32))) if rows is None else rows
    err = np.abs(got.astype(np.float64) - ref.mix(x32, w_eff)[rows])
    assert np.all(err <= ref.mix_bound(x32, w_eff)[rows]), (what, float(err.max()))


def _case(device, monkeypatch, devices=None):
    fed, nodes = _start(device, devices=devices)
    try:
        agg = nodes[0].aggregator
        arrived = {nd.addr: None for nd in nodes}
        x32 = _set_rows(nodes)
        w = agg.mixing_matrix(K)
        shares = _shares(w, list(range(K)))
        _, d, tau_ref, _, w_ref = ref.clipped_gossip(x32, shares, b=1)
        assert ref.selection_gap(d, shares, 1, rows=HONEST) > 1e-3
        if device == "cuda":  # the stacked rows are mixed in place: nothing is packed or unpacked
            assert weights_plane._stacked_group([nd.learner for nd in nodes]) is not None

            def boom(*a, **k):
                raise AssertionError("the live rows of the stacked group were packed")

            monkeypatch.setattr(weights_plane, "_pack", boom)
        assert weights_plane.aggregate_neighbors(fed, arrived, agg) == [nd.addr for nd in nodes]
        got = _rows(nodes)
        if devices is None:
            # one call over the six rows: last_clipping names them in row order, on every aggregator
            for nd in nodes:
                addrs, tau, w_eff = nd.aggregator.last_clipping
                assert addrs == [m.addr for m in nodes]
                assert tau.device.type == w_eff.device.type == nd.learner.flat_params().device.type  # stayed on the device
            addrs, tau, w_eff = agg.last_clipping
            tau, w_eff = tau.cpu().numpy(), w_eff.cpu().numpy()
            np.testing.assert_allclose(tau[HONEST], tau_ref[HONEST], rtol=2e-5, atol=0)
            assert np.array_equal(w_eff != 0, w_ref != 0)
            np.testing.assert_allclose(w_eff[HONEST], w_ref[HONEST], rtol=2e-5, atol=0)
            _check_rows(got, x32, w_eff, device)
            # the attacker's column holds the smallest scales
            with np.errstate(all="ignore"):
                scale = np.where(shares > 0, w_eff / shares, np.inf)
            for p in ((BAD - 1) % K, (BAD + 1) % K):
                assert scale[p, BAD] < 0.01 and scale[p, BAD] == scale[p].min() and np.sort(scale[p])[1] > 0.99
        else:
            # one call per device over its rows and the rows it received: sub-matrices of the same plan
            for nd in [nodes[i] for i in HONEST]:
                addrs, tau, w_eff = nd.aggregator.last_clipping
                assert nd.addr in addrs and len(set(addrs)) == len(addrs) <= K
                rows = [[m.addr for m in nodes].index(a) for a in addrs]
                assert rows == sorted(rows)
                p = addrs.index(nd.addr)
                np.testing.assert_allclose(w_eff.numpy()[p], w_ref[rows[p]][rows], rtol=2e-5, atol=0)
                np.testing.assert_allclose(float(tau[p]), tau_ref[rows[p]], rtol=2e-5, atol=0)
            _check_rows(got[HONEST], x32, w_ref, "mesh", rows=HONEST)
        # an honest neighbour of the attacker moves by at most its radius; the plain mix drags it by W·d
        _set_rows(nodes)
        plain = NeighborAvg(topology="ring")
        weights_plane.aggregate_neighbors(fed, arrived, plain)
        dragged = _rows(nodes)
        full = w.copy()
        want_plain = full @ x32.astype(np.float64)
        for p in ((BAD - 1) % K, (BAD + 1) % K):
            moved = np.linalg.norm(got[p].astype(np.float64) - x32[p])
            reach = sum(float(shares[p, q]) * min(np.sqrt(d[p, q]), tau_ref[p]) for q in ref.neighbours(shares, p))
            moved_plain = np.linalg.norm(dragged[p].astype(np.float64) - x32[p])
            want_moved = np.linalg.norm(want_plain[p] - x32[p])
            print(f"{device} row {p}: clipped move {moved:.4e} (reach {reach:.4e}), plain move {moved_plain:.4e} (W·d {want_moved:.4e})")
            assert moved <= reach * (1 + 1e-4)
            np.testing.assert_allclose(moved_plain, want_moved, rtol=1e-4)
            assert abs(want_moved - float(w[p, BAD]) * np.sqrt(d[p, BAD])) < 1e-3 * want_moved  # W·d: the attacker's share of its distance
            assert moved_plain > 1000 * moved
    finally:
        _stop(nodes)


def test_clipped_gossip_device_plane_cpu(monkeypatch):
    _case("cpu", monkeypatch)


def test_clipped_gossip_device_plane_cpu_mesh(monkeypatch):
    """Two host-mesh devices: ``_mesh_neighbors`` (one exchange, one clipped mix per receiving device)."""
    _case("cpu", monkeypatch, devices=["cpu", "cpu"])


@pytest.mark.gpu
def test_clipped_gossip_device_plane_gpu(monkeypatch):
    _case("cuda", monkeypatch)


def _absent_case(device, tau):
    """Peer 4 did not arrive (a dead or non-training neighbour): its share folds back onto the
    present sources of rows 3 and 5 as in the plain mix, and its own row is not touched."""
    fed, nodes = _start(device, tau=tau)
    try:
        agg = nodes[0].aggregator
        present = [0, 1, 2, 3, 5]
        arrived = {nodes[i].addr: None for i in present}
        x32 = _set_rows(nodes, seed=5)
        shares = _shares(agg.mixing_matrix(K), present)
        assert shares[3].sum() == pytest.approx(0.5) and shares[4].sum() == pytest.approx(0.5)  # 1/3 of the remaining 2/3
        _, _, tau_ref, _, w_ref = ref.clipped_gossip(x32[present], shares, tau=tau)
        assert weights_plane.aggregate_neighbors(fed, arrived, agg) == [nodes[i].addr for i in present]
        got = _rows(nodes)
        addrs, taus, w_eff = agg.last_clipping
        assert addrs == [nodes[i].addr for i in present]
        assert nodes[4].aggregator.last_clipping is None
        w_eff = w_eff.cpu().numpy()
        assert np.array_equal(w_eff != 0, w_ref != 0)
        np.testing.assert_allclose(w_eff, w_ref, rtol=2e-5, atol=0)
        assert np.array_equal(got[4], x32[4])
        _check_rows(got[present], x32[present], w_eff, ("absent", device))
        return fed, nodes, arrived, present, x32, got
    except BaseException:
        _stop(nodes)
        raise


def _absent_against_plain(device):
    # a radius nothing reaches: the clipped mix is the plain mix in difference form, so the fold of
    # the absent peer's share must be the plain mix's own
    fed, nodes, arrived, present, x32, got = _absent_case(device, tau=1e30)
    try:
        for nd, r in zip(nodes, x32):
            with torch.no_grad():
                nd.learner.flat_params().copy_(torch.from_numpy(r.copy()))
        weights_plane.aggregate_neighbors(fed, arrived, NeighborAvg(topology="ring"))
        plain = _rows(nodes)
        # both are within a few fp32 roundings of the same float64 value; −10·base dominates the magnitude
        np.testing.assert_allclose(got, plain, rtol=0, atol=8 * 2.0**-24 * float(np.abs(x32).max()))
        assert not np.array_equal(plain[3], x32[3])
    finally:
        _stop(nodes)


def test_absent_neighbour_folds_back_cpu():
    _absent_against_plain("cpu")
    fed, nodes, *_ = _absent_case("cpu", tau=0.05)
    _stop(nodes)


@pytest.mark.gpu
def test_absent_neighbour_folds_back_gpu():
    _absent_against_plain("cuda")


def _plain_case(device):
    """``NeighborAvg`` on the same federation: bit-identical to the plain path's own arithmetic (the
    packed rows through ``ops.weighted_average``; on the GPU the stacked group through one
    ``myfyp_neighbor_mix_stacked`` launch), and no ``ClippedGossip`` state is touched."""
    fed, nodes = _start(device)
    try:
        x32 = _set_rows(nodes, seed=7)
        plain = NeighborAvg(topology="ring")
        w = plain.mixing_matrix(K)
        if device == "cuda":
            group = nodes[0].learner._engine.group
            copy = group.params.clone()
            mix = np.zeros((group.capacity, group.capacity), dtype=np.float32)
            slots = [nd.learner._engine.slot for nd in nodes]
            for i in range(K):
                nz = list(np.nonzero(w[i])[0])
                ws = np.array([w[i, j] for j in nz], dtype=np.float64)
                ws = ws / ws.sum()
                for j, v in zip(nz, ws):
                    mix[slots[i], slots[j]] += v
            ops.check(ops.fast_lib().myfyp_neighbor_mix_stacked(copy.data_ptr(), group.capacity, group.numel, group.S, mix.ctypes.data,
                                                                torch.cuda.current_stream().cuda_stream), "neighbor_mix")
            want = np.stack([copy[s, : group.numel].cpu().numpy() for s in slots])
        else:
            src = [torch.from_numpy(r.copy()) for r in x32]
            want = []
            for i in range(K):
                nz = list(np.nonzero(w[i])[0])
                ws = np.array([w[i, j] for j in nz], dtype=np.float64)
                ws = ws / ws.sum()
                want.append(ops.weighted_average([[src[j]] for j in nz], [float(v) for v in ws])[0].numpy())
            want = np.stack(want)
        weights_plane.aggregate_neighbors(fed, {nd.addr: None for nd in nodes}, plain)
        assert np.array_equal(_rows(nodes).view(np.uint32), want.view(np.uint32))
        assert all(nd.aggregator.last_clipping is None for nd in nodes) and not hasattr(plain, "last_clipping")
    finally:
        _stop(nodes)


def test_plain_neighbor_avg_untouched_cpu():
    _plain_case("cpu")


@pytest.mark.gpu
def test_plain_neighbor_avg_untouched_gpu():
    _plain_case("cuda")


@pytest.mark.slow
def test_clipped_gossip_two_ranks_gloo():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "workers", "clipped_gossip_worker.py")]
    env = dict(os.environ, MYFYP_DIST_BACKEND="gloo", AGG_DEVICE="cpu")  # CPU tensors also on a GPU host
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("OK") == 2
