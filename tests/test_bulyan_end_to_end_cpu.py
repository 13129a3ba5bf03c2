"""``examples/configs/mnist_attack_signflip_bulyan.yaml`` through ``runner.run_experiment``: 8 peers
on the collective workflow, one sign-flipping every model it contributes, Bulyan (f = 1) on the
collective plane's device path (CPU tensors here: the same plumbing, the torch oracle).

A sign-flipped model is the farthest from every other, so iterated Krum leaves it among the two
rows it never picks: its coefficient is 0 in every round, and the honest peers' test loss falls."""

import os

import numpy as np

from myfyp_amd import runner
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation

CFG = os.path.join(os.path.dirname(__file__), "..", "myfyp_amd", "examples", "configs", "mnist_attack_signflip_bulyan.yaml")


def test_signflip_bulyan_collective_rejects_the_attacker(monkeypatch):
    made, rounds = [], []
    build = runner.build_aggregator
    device_path = weights_plane.aggregate_bulyan

    def recording(spec):
        made.append(build(spec))
        return made[-1]

    def generic(*a, **k):
        raise AssertionError("Bulyan left the device path of the collective plane")

    def watched(fed, arrived, aggregator):
        device_path(fed, arrived, aggregator)
        addrs, coef = aggregator.last_selection
        rounds.append(dict(zip(addrs, coef.tolist())))

    monkeypatch.setattr(runner, "build_aggregator", recording)
    monkeypatch.setattr(weights_plane, "aggregate_generic", generic)
    monkeypatch.setattr(weights_plane, "aggregate_bulyan", watched)
    Federation.reset()
    try:
        res = runner.run_experiment(CFG, verbose=False)
    finally:
        Federation.reset()
    assert len(res["nodes"]) == 8 and len(made) == 8
    for h in res["histories"].values():
        assert h.count("RoundFinishedStage") == 2
    attacked = "fyp-sign-flip-bulyan-node-1"
    assert attacked in res["nodes"]
    assert len(rounds) == 2  # one device aggregation per round
    for coef in rounds:
        assert sorted(coef) == sorted(res["nodes"])  # every peer trained
        assert coef[attacked] == 0, coef
        assert sorted(coef.values()) == [0.0] * 2 + [float(np.float32(1) / np.float32(6))] * 6  # θ = 6 picked, 1/6 each
    for agg in made:
        assert agg.collective_kind == "bulyan" and agg.last_selection is not None
        assert dict(zip(agg.last_selection[0], agg.last_selection[1].tolist())) == rounds[-1]
    # the honest peers learn: the loss on their test split after two rounds is below the start's
    for addr, logs in res["global_logs"].items():
        loss = dict(logs["test_loss"])
        print(f"{addr}: test loss {loss[0]:.3f} -> {loss[max(loss)]:.3f}")
        if addr != attacked:
            assert loss[max(loss)] < loss[0], (addr, loss)
