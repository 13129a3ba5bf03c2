"""``examples/configs/mnist_ring_attack_clippedgossip.yaml`` through ``runner.run_experiment``: a ring
of 6 MLP peers on the collective workflow, synthetic MNIST, peer 2 replacing every model it
contributes by −10 times it, ClippedGossip (b = 1) on the collective plane (CPU tensors here: the
same plumbing, the float64 torch path), 3 rounds.

Every honest peer ends above the 0.5 accuracy that ``test_neighbor_avg_workflow_learns`` asks of an
unattacked ring, everyone trains every round, and every round's plan clips the attacker hardest."""

import os

import numpy as np
import pytest

from myfyp_amd import runner
from myfyp_amd.learning.aggregators import ClippedGossip
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

CFG = os.path.join(os.path.dirname(__file__), "..", "myfyp_amd", "examples", "configs", "mnist_ring_attack_clippedgossip.yaml")


@pytest.fixture
def cpu_settings():
    keep = {k: getattr(Settings, k) for k in ("DEVICE", "FUSED_ROUND", "BATCH_SIZE", "TRAIN_SET_SIZE")}
    Settings.DEVICE = "cpu"
    Federation.reset()
    yield
    Federation.reset()
    for k, v in keep.items():
        setattr(Settings, k, v)


def test_ring_scale_attack_clipped_gossip_learns(monkeypatch, cpu_settings):
    made, rounds = [], []
    build = runner.build_aggregator
    plane = weights_plane.aggregate_neighbors

    def recording(spec):
        made.append(build(spec))
        return made[-1]

    def watched(fed, arrived, aggregator):
        out = plane(fed, arrived, aggregator)
        addrs, tau, w_eff = aggregator.last_clipping
        rounds.append((list(addrs), np.asarray(tau), np.asarray(w_eff)))
        return out

    def generic(*a, **k):
        raise AssertionError("ClippedGossip left the neighbour path of the collective plane")

    monkeypatch.setattr(runner, "build_aggregator", recording)
    monkeypatch.setattr(weights_plane, "aggregate_neighbors", watched)
    monkeypatch.setattr(weights_plane, "aggregate_generic", generic)
    res = runner.run_experiment(CFG, verbose=False)
    assert len(res["nodes"]) == 6 and len(made) == 6 and all(isinstance(a, ClippedGossip) for a in made)
    for h in res["histories"].values():
        assert h.count("TrainStage") == 3  # everyone trains every round
    attacked = "ring-scale-clippedgossip-node-2"
    assert attacked in res["nodes"]
    assert len(rounds) == 3  # one clipped mix per round
    shares = made[0].mixing_matrix(6)
    for addrs, tau, w_eff in rounds:
        assert sorted(addrs) == sorted(res["nodes"])
        bad = addrs.index(attacked)
        for p in ((bad - 1) % 6, (bad + 1) % 6):
            scale = {q: w_eff[p, q] / shares[p, q] for q in ((p - 1) % 6, (p + 1) % 6)}
            assert scale[bad] < 0.2 and scale[bad] == min(scale.values()), (p, scale)  # the attacker is clipped, and hardest
        assert np.all(tau > 0) and np.all(np.isfinite(tau))
    for addr, logs in res["global_logs"].items():
        acc = dict(logs["test_metric"])
        print(f"{addr}: test accuracy {acc[max(acc)]:.3f}")
        if addr != attacked:
            assert acc[max(acc)] > 0.5, (addr, acc)
