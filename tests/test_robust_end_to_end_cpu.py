"""``examples/configs/mnist_attack_signflip_krum.yaml`` through ``runner.run_experiment``: 5 peers on
the collective workflow, one sign-flipping every model it contributes, Multi-Krum on the collective
plane's device path (CPU tensors here: the same plumbing, the torch reference math)."""

import os

from myfyp_amd import runner
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation

CFG = os.path.join(os.path.dirname(__file__), "..", "myfyp_amd", "examples", "configs", "mnist_attack_signflip_krum.yaml")


def test_signflip_krum_collective_rejects_the_attacker(monkeypatch):
    made = []
    build = runner.build_aggregator

    def recording(spec):
        made.append(build(spec))
        return made[-1]

    def generic(*a, **k):
        raise AssertionError("Krum left the device path of the collective plane")

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
    attacked = "fyp-sign-flip-krum-node-1"
    assert attacked in res["nodes"]
    for agg in made:
        assert agg.collective_kind == "krum" and agg.last_selection is not None
        addrs, coef = agg.last_selection
        assert sorted(addrs) == sorted(res["nodes"])  # every peer trained
        coef = dict(zip(addrs, coef.tolist()))
        assert coef[attacked] == 0, coef
        assert sum(1 for c in coef.values() if c != 0) == 3
