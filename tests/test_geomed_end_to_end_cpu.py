"""``examples/configs/mnist_attack_signflip_geomed.yaml`` through ``runner.run_experiment``: 5 peers
on the collective workflow, one sign-flipping every model it contributes, the geometric median on
the collective plane's device path (CPU tensors here: the same plumbing, the float64 oracle).

Five equal peers, one flipped: the oracle's three steps from the mean leave the attacker's
coefficient at 1.3e-2 against honest ones of 0.24 .. 0.25 (measured on this path, the oracle's),
below the tenth of the smallest honest coefficient asserted here."""

import os

from myfyp_amd import runner
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation

CFG = os.path.join(os.path.dirname(__file__), "..", "myfyp_amd", "examples", "configs", "mnist_attack_signflip_geomed.yaml")


def test_signflip_geomed_collective_down_weights_the_attacker(monkeypatch):
    made = []
    build = runner.build_aggregator

    def recording(spec):
        made.append(build(spec))
        return made[-1]

    def generic(*a, **k):
        raise AssertionError("GeometricMedian left the device path of the collective plane")

    monkeypatch.setattr(runner, "build_aggregator", recording)
    monkeypatch.setattr(weights_plane, "aggregate_generic", generic)
    Federation.reset()
    try:
        res = runner.run_experiment(CFG, verbose=False)
    finally:
        Federation.reset()
    assert len(res["nodes"]) == 5 and len(made) == 5
    for h in res["histories"].values():
        assert h.count("RoundFinishedStage") == 2
    attacked = "fyp-sign-flip-geomed-node-1"
    assert attacked in res["nodes"]
    for agg in made:
        assert agg.collective_kind == "geometric_median" and agg.last_weights is not None
        addrs, coef = agg.last_weights
        assert sorted(addrs) == sorted(res["nodes"])  # every peer trained
        coef = dict(zip(addrs, coef.tolist()))
        honest = [c for a, c in coef.items() if a != attacked]
        print(f"attacked {coef[attacked]:.3e}, honest {min(honest):.3e} .. {max(honest):.3e}")
        assert abs(sum(coef.values()) - 1) < 1e-6
        assert 0 <= coef[attacked] < 0.1 * min(honest), coef
