"""Attacks x aggregators on the collective protocol: one table of the honest peers' final test accuracy."""

# Rows: no attack is not run; the three single-peer attacks of the FYP harness (sign flip, Gaussian
# noise, scaling: one peer poisons every model it contributes, the first of the attackers) and the
# four colluding attacks (ALIE, IPM, min-max, min-sum: every attacker sends one row crafted from the
# honest peers' models of the round, fault_injection.ColludingAttack). Columns: FedAvg and the five
# defences that aggregate on the device, DnC (the spectral defence min-max and min-sum were designed
# against) last. Bulyan needs K >= 4f + 3 models, so with 8 peers it faces
# one attacker where the others face two.

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from myfyp_amd.runner import run_experiment  # noqa: E402
from myfyp_amd.utils.utils import set_test_settings  # noqa: E402

SINGLE = ("sign_flip", "gaussian_noise", "scale")
COLLUDING = ("alie", "ipm", "min_max", "min_sum")
ATTACKS = SINGLE + COLLUDING
AGGREGATORS = ("FedAvg", "Krum", "TrimmedMean", "GeometricMedian", "Bulyan", "DnC")


def attackers_for(aggregator: str, nodes: int, attackers: int) -> int:
    """Bulyan tolerates f attackers only among K >= 4f + 3 models."""
    return min(attackers, max(0, (nodes - 3) // 4)) if aggregator == "Bulyan" else attackers


def aggregator_spec(name: str, nodes: int, f: int) -> dict:
    params = {"Krum": {"num_byzantine": f}, "Bulyan": {"num_byzantine": f}, "DnC": {"num_byzantine": f},
              "TrimmedMean": {"beta": f / nodes}}.get(name, {})
    return {"name": name, "params": params}


def config(attack: str, aggregator: str, nodes: int, attackers: int, rounds: int, seed: int, n_train: int, n_test: int):
    """(experiment description, the attackers' peer indices)."""
    f = attackers_for(aggregator, nodes, attackers)
    bad = [1 + i * ((nodes - 1) // max(1, f)) for i in range(f)]  # spread over the peers, never peer 0 (it starts the round)
    if attack in COLLUDING:
        att = {"kind": attack, "nodes": bad}
    elif f > 0:
        # ModelPoisoning wraps learner.fit: the fused round of the GPU engines never calls it, so
        # under FedAvg on a GPU these three rows show the unattacked run
        att = {"kind": attack, "node": bad[0], "persistent": True, "factor": 10.0}
    exp = {
        "name": f"matrix-{attack}-{aggregator.lower()}-{seed}",
        "rounds": rounds,
        "epochs": 1,
        "seed": seed,
        "same_init": True,
        "trainset_size": nodes,
        "wait_timeout": 600,
        "dataset": {"source": "synthetic", "name": "mnist", "n_train": n_train, "n_test": n_test, "batch_size": 16,
                    "partitioning": {"strategy": "RandomIIDPartitionStrategy"}},
        "model": {"name": "MLP"},
        "aggregator": aggregator_spec(aggregator, nodes, f),
    }
    if f > 0:
        exp["attack"] = att
    return {"experiment": exp, "network": {"protocol": "collective", "nodes": nodes}}, bad


def honest_accuracy(res: dict, bad_addrs) -> float:
    """Mean over the honest peers of the last test accuracy they logged."""
    vals = []
    for addr, logs in res["global_logs"].items():
        if addr in bad_addrs or not logs.get("test_metric"):
            continue
        vals.append(float(logs["test_metric"][-1][1]))
    return sum(vals) / len(vals) if vals else float("nan")


def format_table(table: dict, attacks, aggregators) -> str:
    lines = [f"{'attack':<16}" + "".join(f"{a:>17}" for a in aggregators)]
    for at in attacks:
        lines.append(f"{at:<16}" + "".join(f"{table[at, ag]:>17.4f}" for ag in aggregators))
    return "\n".join(lines)


def main(attacks=ATTACKS, aggregators=AGGREGATORS, nodes: int = 8, attackers: int = 2, rounds: int = 3, seed: int = 666, n_train: int = 8000,
         n_test: int = 1600, verbose: bool = True) -> dict:
    from myfyp_amd.parallel.federation import Federation

    set_test_settings()
    table = {}
    for at in attacks:
        for ag in aggregators:
            cfg, bad = config(at, ag, nodes, attackers, rounds, seed, n_train, n_test)
            Federation.reset()
            try:
                res = run_experiment(cfg, verbose=False)
            finally:
                Federation.reset()
            table[at, ag] = honest_accuracy(res, {f"{cfg['experiment']['name']}-node-{i}" for i in bad})
            if verbose:
                print(f"{at} x {ag}: {table[at, ag]:.4f}", flush=True)
    print(f"final test accuracy of the honest peers ({nodes} peers, {attackers} attackers, 1 under Bulyan; {rounds} rounds)")
    print(format_table(table, attacks, aggregators))
    return table


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Attacks x aggregators on the collective protocol.")
    ap.add_argument("--attacks", nargs="+", default=list(ATTACKS), choices=list(ATTACKS))
    ap.add_argument("--aggregators", nargs="+", default=list(AGGREGATORS), choices=list(AGGREGATORS))
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--attackers", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=666)
    a = ap.parse_args()
    main(a.attacks, a.aggregators, a.nodes, a.attackers, a.rounds, a.seed)
