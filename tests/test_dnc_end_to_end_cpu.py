"""``examples/configs/mnist_attack_minmax_dnc.yaml`` through ``runner.run_experiment``: 8 peers on
the collective workflow, peers 3 and 6 collude with the min-max attack, DnC (f = 2) on the collective
plane's device path (CPU tensors here: the same plumbing, the torch oracle).

The crafted row stays inside the honest rows' distance envelope, but both colluders hold it: their
common shift is the top singular direction of the centred models, their projections on it are the
largest, and their coefficients are 0 in every round, while the honest peers' test loss falls."""

import os

from myfyp_amd import runner
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation

CFG = os.path.join(os.path.dirname(__file__), "..", "myfyp_amd", "examples", "configs", "mnist_attack_minmax_dnc.yaml")


def test_minmax_dnc_collective_removes_the_colluders(monkeypatch):
    made, rounds = [], []
    build = runner.build_aggregator
    device_path = weights_plane.aggregate_dnc

    def recording(spec):
        made.append(build(spec))
        return made[-1]

    def generic(*a, **k):
        raise AssertionError("DnC left the device path of the collective plane")

    def watched(fed, arrived, aggregator, round_):
        device_path(fed, arrived, aggregator, round_)
        addrs, coef = aggregator.last_selection
        rounds.append((round_, dict(zip(addrs, coef.tolist()))))

    monkeypatch.setattr(runner, "build_aggregator", recording)
    monkeypatch.setattr(weights_plane, "aggregate_generic", generic)
    monkeypatch.setattr(weights_plane, "aggregate_dnc", watched)
    Federation.reset()
    try:
        res = runner.run_experiment(CFG, verbose=False)
    finally:
        Federation.reset()
    assert len(res["nodes"]) == 8 and len(made) == 8
    for h in res["histories"].values():
        assert h.count("RoundFinishedStage") == 2
    attackers = ["fyp-min-max-dnc-node-3", "fyp-min-max-dnc-node-6"]
    assert all(a in res["nodes"] for a in attackers)
    assert [r for r, _ in rounds] == [0, 1]  # one device aggregation per round, told its round
    for _, coef in rounds:
        assert sorted(coef) == sorted(res["nodes"])  # every peer trained
        assert sorted(a for a, c in coef.items() if c == 0) == attackers, coef
        assert abs(sum(coef.values()) - 1.0) < 1e-6
    for agg in made:
        assert agg.collective_kind == "dnc" and agg.last_selection is not None
        assert dict(zip(agg.last_selection[0], agg.last_selection[1].tolist())) == rounds[-1][1]
    # the honest peers learn: the loss on their test split after two rounds is below the start's
    for addr, logs in res["global_logs"].items():
        loss = dict(logs["test_loss"])
        print(f"{addr}: test loss {loss[0]:.3f} -> {loss[max(loss)]:.3f}")
        if addr not in attackers:
            assert loss[max(loss)] < loss[0], (addr, loss)
