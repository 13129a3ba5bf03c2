"""``examples/configs/mnist_attack_minmax_krum.yaml`` through ``runner.run_experiment``: 8 peers on
the collective workflow, two of them colluding (min-max), Krum (f = 2) on the collective plane's
device path; then the same attack under FedAvg on the three round paths (round driver, fused round,
per-stage gangs), the unchanged single-peer attack form, and the attack matrix example.

The attackers' rows are captured right before the aggregation (the hook has run by then): they are
one row, and no farther from any honest row than the honest rows are from each other."""

import math
import os

import numpy as np
import pytest
import torch

import _collude_ref as cr
from myfyp_amd import fault_injection, runner
from myfyp_amd.parallel import weights_plane
from myfyp_amd.parallel.federation import Federation
from myfyp_amd.settings import Settings

CFG = os.path.join(os.path.dirname(__file__), "..", "myfyp_amd", "examples", "configs", "mnist_attack_minmax_krum.yaml")
ATTACKERS = ["fyp-min-max-krum-node-1", "fyp-min-max-krum-node-5"]


def _run(cfg):
    Federation.reset()
    try:
        return runner.run_experiment(cfg, verbose=False)
    finally:
        Federation.reset()


def test_minmax_krum_collective(monkeypatch):
    made, seen, lasts = [], [], []
    build = runner.build_aggregator
    device_path = weights_plane.aggregate_krum
    hook = fault_injection.ColludingAttack._hook

    def recording(spec):
        made.append(build(spec))
        return made[-1]

    def generic(*a, **k):
        raise AssertionError("Krum left the device path of the collective plane")

    def watched(fed, arrived, aggregator):
        rows = {a: fed.local_nodes[a].learner.flat_params().detach().double().cpu().numpy().copy() for a in arrived}
        seen.append((rows, {a: float(arrived[a][0]) for a in arrived}))
        device_path(fed, arrived, aggregator)
        addrs, coef = aggregator.last_selection
        seen[-1] += (dict(zip(addrs, coef.tolist())),)

    def hooked(self, round_, fed, weights):
        self.last = None
        hook(self, round_, fed, weights)
        lasts.append((round_, self.last))

    monkeypatch.setattr(runner, "build_aggregator", recording)
    monkeypatch.setattr(weights_plane, "aggregate_generic", generic)
    monkeypatch.setattr(weights_plane, "aggregate_krum", watched)
    monkeypatch.setattr(fault_injection.ColludingAttack, "_hook", hooked)
    res = _run(CFG)
    assert len(res["nodes"]) == 8 and len(made) == 8
    for h in res["histories"].values():  # stage histories are complete
        assert h.count("RoundFinishedStage") == 2 and h.count("VoteTrainSetStage") == 2 and h.count("GossipModelStage") == 2
        assert h.count("TrainStage") + h.count("WaitAggregatedModelsStage") >= 2
    assert res["attack"].rounds == 2 and [r for r, _ in lasts] == [0, 1]  # the hook: once per round
    assert len(seen) == 2  # one device aggregation per round
    for (rows, weights, coef), (_, last) in zip(seen, lasts):
        assert last is not None
        honest, attacking, gamma, stat = last
        # every peer trained; the row order is the gang's arrival order, as for the aggregators
        assert sorted(attacking) == ATTACKERS and sorted(honest + attacking) == sorted(res["nodes"])
        assert float(gamma[0]) > 0
        m = rows[ATTACKERS[0]]
        assert np.array_equal(m, rows[ATTACKERS[1]])
        x = np.stack([rows[a] for a in honest])
        lhs, rhs = cr.constraint(x, m, "min_max")
        print(f"gamma {float(gamma[0]):.4f}: max_i |m - x_i|^2 = {lhs:.6e}, D = {rhs:.6e}; Krum chose {[a for a, c in coef.items() if c]}"
              f" ({'an attacker' if any(coef[a] for a in ATTACKERS) else 'an honest peer'})")
        assert lhs <= rhs * (1 + 1e-4)
        assert lhs >= rhs * (1 - 1e-3)  # the largest such γ: the constraint binds
        assert abs(float(stat[2 * len(honest) + 1]) - rhs) <= 1e-4 * rhs


def _fedavg_cfg(name, attack, nodes=4, rounds=2):
    return {
        "experiment": {"name": name, "rounds": rounds, "epochs": 1, "trainset_size": nodes, "seed": 666, "same_init": True,
                       "dataset": {"source": "synthetic", "name": "mnist", "n_train": 800, "n_test": 160, "batch_size": 16},
                       "model": {"name": "MLP"}, "aggregator": {"name": "FedAvg"}, "attack": attack},
        "network": {"protocol": "collective", "nodes": nodes},
    }


@pytest.mark.parametrize("mode", ["driver", "fused", "threaded"])
def test_every_round_path_calls_the_hook_once_per_round(monkeypatch, mode):
    """ROUND_DRIVER on; ROUND_DRIVER off with FUSED_ROUND on; both off. (Without a GPU no peer has a
    fused engine and all three take the per-stage gangs; with one, each takes its own path.)"""
    from myfyp_amd.stages.collective import driver, fused_round

    calls, paths = [], []
    hook = fault_injection.ColludingAttack._hook
    drive, join = driver.RoundDriver._drive, fused_round.join

    def hooked(self, round_, fed, weights):
        hook(self, round_, fed, weights)
        calls.append((round_, self.last is not None, sorted(weights)))

    monkeypatch.setattr(fault_injection.ColludingAttack, "_hook", hooked)
    monkeypatch.setattr(driver.RoundDriver, "_drive", lambda self, members: (paths.append("driver"), drive(self, members))[1])
    monkeypatch.setattr(fused_round, "join", lambda *a, **k: (paths.append("fused"), join(*a, **k))[1])
    Settings.FUSED_ROUND = mode != "threaded"
    Settings.ROUND_DRIVER = mode == "driver"
    res = _run(_fedavg_cfg(f"collude-paths-{mode}", {"kind": "alie", "nodes": [1, 2], "z": 1.0}))
    assert [c[0] for c in calls] == [0, 1] and all(c[1] for c in calls)
    assert all(c[2] == sorted(res["nodes"]) for c in calls)
    for h in res["histories"].values():
        assert h.count("RoundFinishedStage") == 2
    if torch.cuda.is_available():
        assert set(paths) == {"driver": {"driver"}, "fused": {"fused"}, "threaded": set()}[mode], paths


def test_colluding_attack_needs_the_collective_protocol():
    cfg = _fedavg_cfg("collude-memory", {"kind": "min_max", "nodes": [1]})
    cfg["network"]["protocol"] = "memory"
    with pytest.raises(ValueError, match="collective protocol"):
        _run(cfg)
    with pytest.raises(ValueError, match="colluding kind"):
        _run(_fedavg_cfg("collude-kind", {"kind": "sign_flip", "nodes": [1]}))


def test_single_peer_attack_form_is_unchanged(monkeypatch):
    """``attack: {node, kind}`` still poisons that peer's initial weights with ``apply_attack`` and
    nothing else. Recorded in this process from the parent's code path: a run without the ``attack``
    key in which ``apply_attack`` is called on the same peer right before learning starts. When
    learning starts every peer holds the same bits in both runs, and after the round (one epoch,
    FedAvg) the same final parameters: up to the order of FedAvg's three-term fp32 sum, which
    follows the peers' arrival (3 roundings of 2^-24 of the largest parameter)."""
    from myfyp_amd.node import Node
    from myfyp_amd.utils import utils

    starts, finals, tag = {}, {}, []
    wait = utils.wait_to_finish
    start = Node.set_start_learning

    def flats():
        f = Federation.get()
        return [f.local_nodes[a].learner.flat_params().detach().cpu().clone() for a in f.local_order]

    def waited(nodes, **kw):
        wait(nodes, **kw)
        finals[tag[-1]] = [nd.learner.flat_params().detach().cpu().clone() for nd in nodes]

    def recording_start(self, *a, **kw):
        if tag[-1] == "recorded":
            fault_injection.apply_attack(self, "sign_flip", 0.1, -1.0, 0)
        starts[tag[-1]] = flats()
        return start(self, *a, **kw)

    monkeypatch.setattr(utils, "wait_to_finish", waited)
    monkeypatch.setattr(Node, "set_start_learning", recording_start)
    plain = _fedavg_cfg("old-form", None, nodes=3, rounds=1)
    del plain["experiment"]["attack"]
    for name, cfg in (("form", _fedavg_cfg("old-form", {"node": 0, "kind": "sign_flip"}, nodes=3, rounds=1)), ("recorded", plain), ("clean", plain)):
        tag.append(name)
        res = _run(cfg)
        assert "attack" not in res
    assert len(starts["form"]) == 3 and len(finals["form"]) == 3
    for i, (a, b, c) in enumerate(zip(starts["form"], starts["recorded"], starts["clean"])):
        assert torch.equal(a, b)
        assert torch.equal(a, -c if i == 0 else c) and bool(a.abs().sum() > 0)  # peer 0 flipped, the others intact
    for a, b, c in zip(finals["form"], finals["recorded"], finals["clean"]):
        tol = 4 * 2.0**-24 * float(a.abs().max())
        print(f"final parameters: form vs recorded {float((a - b).abs().max()):.3e} (tolerance {tol:.3e}), vs the unattacked run {float((a - c).abs().max()):.3e}")
        assert float((a - b).abs().max()) <= tol
        assert float((a - c).abs().max()) > 100 * tol  # the attack is visible in the result


def test_attack_matrix_smoke(capsys):
    from myfyp_amd.examples import attack_matrix

    table = attack_matrix.main(attacks=["sign_flip", "min_max"], aggregators=["FedAvg", "Krum"], nodes=4, attackers=1, rounds=2, n_train=800, n_test=160,
                               verbose=False)
    assert sorted(table) == sorted((a, g) for a in ("sign_flip", "min_max") for g in ("FedAvg", "Krum"))
    assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in table.values())
    out = capsys.readouterr().out
    assert "min_max" in out and "Krum" in out and out.count("\n") >= 4
