"""Krum / TrimmedMean / GeometricMedian / Bulyan / DnC aggregation on the collective plane: device path against the generic path.

    python benchmarks/bench_robust_agg.py                      # MLP (n = 235,146) and ResNet-18, 8 peers
    python benchmarks/bench_robust_agg.py --models mlp --repeats 30
    python benchmarks/bench_robust_agg.py --aggregators geometric_median,krum
    python benchmarks/bench_robust_agg.py --aggregators bulyan
    python benchmarks/bench_robust_agg.py --aggregators dnc,krum   # DnC's sqdist/select pair beside Krum's, all tiles and subsample_dims = 10000
    python benchmarks/bench_robust_agg.py --attack               # ops.collude_into (ALIE, IPM, min-max, min-sum) beside Krum, K = 8 / 16

For each model and aggregator the same 8 co-located peers are aggregated two ways, alternating in
one process on identical inputs (the rows are restored, untimed, before every call):

* device : ``weights_plane.aggregate_krum`` / ``aggregate_trimmed_mean`` / ``aggregate_geometric_median`` / ``aggregate_bulyan`` (the kernels of
  ``csrc/kernels/fl_ops.hip`` on the live rows), host clock around the call plus a device
  synchronise;
* generic: what ``join_aggregation`` does for an aggregator without a device path — a wire model
  per trainer (``get_parameters()``: a device-to-host copy), ``weights_plane.aggregate_generic``
  (the host aggregator over the gathered wire models, ``set_model`` into every peer), synchronise.

The two row-reading kernels are then timed alone with device events over a window of back-to-back
calls, and their achieved GB/s computed from the bytes the algorithm needs (K rows read; the mean
reads the chosen rows and writes P rows). The geometric median's distance/reweight pair is the
difference of a 5-step and a 1-step call, divided by 4: allocation and call overhead cancel; the
whole 1-step call (screen + one step: two pairs) is reported next to Krum's distance/select pair,
which is timed in the same process for that. Bulyan's ``k_bulyan_mean<K, f>`` is timed alone from a
selection made before the window, next to ``k_trimmed_mean<K>`` on the same rows in the same
process. DnC's ``k_dnc_sqdist<K>`` / ``k_dnc_select`` pair is timed with every tile taken and at
``subsample_dims = 10000`` (it then reads about 10000 / n of the bytes), next to Krum's pair in the
same process. One JSON line per (model, aggregator). Needs a GPU:
``--device cpu`` only rehearses the plumbing and its timings mean nothing.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEERS = 8
FLIPPED = 5


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mlp,resnet18")
    ap.add_argument("--aggregators", default="krum,trimmed_mean,geometric_median,bulyan")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--repeats", type=int, default=20, help="timed device calls per case (generic: --generic-repeats)")
    ap.add_argument("--generic-repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=50, help="back-to-back op calls inside one device-event window")
    ap.add_argument("--attack", nargs="?", const="all", default=None,
                    help="time ops.collude_into instead (all, or a comma list of alie,ipm,min_max,min_sum) at K = 8 and 16 honest rows, beside Krum")
    return ap.parse_args()


def build_nodes(model_name: str, make_agg):
    from myfyp_amd.communication.protocols.collective.collective_protocol import CollectiveCommunicationProtocol
    from myfyp_amd.learning.dataset.synthetic import synthetic_cifar10, synthetic_mnist
    from myfyp_amd.learning.frameworks.torch import TorchModel
    from myfyp_amd.models import MLP, ResNet18
    from myfyp_amd.node import Node

    data = synthetic_mnist(256, 64) if model_name == "mlp" else synthetic_cifar10(n_train=256, n_test=64)
    cls = MLP if model_name == "mlp" else ResNet18
    tag = time.time_ns()
    return [Node(TorchModel(cls(seed=0)), data, address=f"bench{tag}-{i}", aggregator=make_agg(), protocol=CollectiveCommunicationProtocol) for i in range(PEERS)]


def sync(dev) -> None:
    import torch

    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def spread(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 4), "min_ms": round(1e3 * min(xs), 4), "max_ms": round(1e3 * max(xs), 4), "n": len(xs)}


def event_ms(dev, fn, iters: int, warmup: int) -> float:
    """Per-call device time of ``fn`` over a window of ``iters`` back-to-back calls."""
    import torch

    for _ in range(warmup):
        fn()
    sync(dev)
    if dev.type != "cuda":
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return 1e3 * (time.perf_counter() - t0) / iters
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def run_case(model_name: str, agg_name: str, args) -> dict:
    import torch

    from myfyp_amd import ops
    from myfyp_amd.learning.aggregators import Bulyan, DnC, GeometricMedian, Krum, TrimmedMean
    from myfyp_amd.parallel import weights_plane
    from myfyp_amd.parallel.federation import Federation

    make = {"krum": lambda: Krum(num_byzantine=1, multi=3), "trimmed_mean": lambda: TrimmedMean(beta=0.125),
            "geometric_median": lambda: GeometricMedian(iters=3), "bulyan": lambda: Bulyan(num_byzantine=1),
            "dnc": lambda: DnC(num_byzantine=1)}[agg_name]
    Federation.reset()
    fed = Federation.init()
    nodes = build_nodes(model_name, make)
    try:
        for nd in nodes:
            nd.start()
        fed.finalize()
        learners = [nd.learner for nd in nodes]
        dev = learners[0].flat_params().device
        n = learners[0].flat_params().numel()
        g = torch.Generator().manual_seed(1)
        base = torch.randn(n, generator=g) * 0.05
        rows0 = torch.stack([(-base if i == FLIPPED else base + 1e-3 * (1 + 0.15 * i) * 0.05 * torch.randn(n, generator=g)) for i in range(PEERS)]).to(dev)
        agg = nodes[0].aggregator
        device_fn = {"krum": weights_plane.aggregate_krum, "trimmed_mean": weights_plane.aggregate_trimmed_mean,
                     "geometric_median": weights_plane.aggregate_geometric_median, "bulyan": weights_plane.aggregate_bulyan,
                     "dnc": lambda f_, arrived, a: weights_plane.aggregate_dnc(f_, arrived, a, 0)}[agg_name]

        def restore() -> None:
            with torch.no_grad():
                for i, lr in enumerate(learners):
                    lr.flat_params().copy_(rows0[i])
            sync(dev)

        def device_call() -> None:
            device_fn(fed, {nd.addr: (float(1 + i), None) for i, nd in enumerate(nodes)}, agg)
            sync(dev)

        def generic_call() -> None:
            arrived = {}
            for i, nd in enumerate(nodes):
                model = nd.learner.get_model()
                wire = model.build_copy(params=model.get_parameters(), num_samples=1 + i, contributors=[nd.addr], additional_info=dict(model.additional_info))
                arrived[nd.addr] = (float(1 + i), wire)
            weights_plane.aggregate_generic(fed, arrived, agg)
            sync(dev)

        def timed(fn) -> float:
            restore()
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

        for _ in range(args.warmup):
            timed(device_call)
        timed(generic_call)
        t_dev, t_gen = [], []
        per_generic = max(1, args.repeats // max(1, args.generic_repeats))
        for r in range(args.repeats):  # alternating: both see the same machine state
            t_dev.append(timed(device_call))
            if r % per_generic == 0 and len(t_gen) < args.generic_repeats:
                t_gen.append(timed(generic_call))
        # both paths compute the same aggregate from the same rows
        restore()
        device_call()
        after_dev = learners[0].flat_params().detach().clone()
        restore()
        generic_call()
        diff = float((learners[0].flat_params() - after_dev).abs().max())

        # the row-reading kernels alone, on the live rows (outputs alias them, as on the round's path)
        restore()
        flats = [lr.flat_params() for lr in learners]
        w = [float(1 + i) for i in range(PEERS)]
        it, wu = args.kernel_iters, args.warmup
        kernels = {}
        if agg_name == "krum":
            scratch = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(PEERS)]  # P outputs that leave the rows intact
            ms_sel = event_ms(dev, lambda: ops.krum_into(flats, [], w, 1, 3), it, wu)
            ms_all = event_ms(dev, lambda: ops.krum_into(flats, scratch, w, 1, 3), it, wu)
            ms_mean = max(ms_all - ms_sel, 1e-6)
            kernels["pairwise_sqdist+select"] = {"ms": round(ms_sel, 4), "GBps": round(PEERS * n * 4 / ms_sel / 1e6, 1), "bytes": "K rows read"}
            kernels["coef_mean"] = {"ms": round(ms_mean, 4), "GBps": round((3 + PEERS) * n * 4 / ms_mean / 1e6, 1), "bytes": "3 chosen rows read, P rows written",
                                    "note": "difference of the two windows"}
        elif agg_name == "geometric_median":
            scratch = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(PEERS)]
            ms_1 = event_ms(dev, lambda: ops.geometric_median_into(flats, [], w, 1), it, wu)
            ms_5 = event_ms(dev, lambda: ops.geometric_median_into(flats, [], w, 5), it, wu)
            ms_3 = event_ms(dev, lambda: ops.geometric_median_into(flats, [], w, 3), it, wu)
            ms_all = event_ms(dev, lambda: ops.geometric_median_into(flats, scratch, w, 3), it, wu)
            ms_krum = event_ms(dev, lambda: ops.krum_into(flats, [], w, 1, 3), it, wu)
            ms_pair = max((ms_5 - ms_1) / 4, 1e-6)
            ms_mean = max(ms_all - ms_3, 1e-6)
            kernels["gm_dist+reweight"] = {"ms": round(ms_pair, 4), "GBps": round(PEERS * n * 4 / ms_pair / 1e6, 1), "bytes": "K rows read",
                                           "note": "(5-step call - 1-step call) / 4"}
            kernels["screen+1 step (2 pairs, whole call)"] = {"ms": round(ms_1, 4), "GBps": round(2 * PEERS * n * 4 / ms_1 / 1e6, 1), "bytes": "K rows read twice"}
            kernels["screen+3 steps (4 pairs, whole call)"] = {"ms": round(ms_3, 4), "GBps": round(4 * PEERS * n * 4 / ms_3 / 1e6, 1), "bytes": "K rows read 4 times"}
            kernels["krum pairwise_sqdist+select (whole call, same process)"] = {"ms": round(ms_krum, 4), "GBps": round(PEERS * n * 4 / ms_krum / 1e6, 1),
                                                                               "bytes": "K rows read"}
            kernels["coef_mean"] = {"ms": round(ms_mean, 4), "GBps": round(2 * PEERS * n * 4 / ms_mean / 1e6, 1), "bytes": "K rows read, P rows written",
                                    "note": "difference of the two windows"}
        elif agg_name == "bulyan":
            scratch = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(PEERS)]
            coef = ops.bulyan_into(flats, [], 1)[2]
            ms_sel = event_ms(dev, lambda: ops.bulyan_into(flats, [], 1), it, wu)
            ms_mean = event_ms(dev, lambda: ops.bulyan_mean_into(flats, scratch, coef, 1), it, wu)
            ms_trim = event_ms(dev, lambda: ops.trimmed_mean_into(flats, scratch, 1), it, wu)
            ms_all = event_ms(dev, lambda: ops.bulyan_into(flats, scratch, 1), it, wu)
            picked = PEERS - 2
            kernels["pairwise_sqdist+bulyan_select"] = {"ms": round(ms_sel, 4), "GBps": round(PEERS * n * 4 / ms_sel / 1e6, 1), "bytes": "K rows read"}
            kernels["bulyan_mean"] = {"ms": round(ms_mean, 4), "GBps": round((picked + PEERS) * n * 4 / ms_mean / 1e6, 1),
                                      "bytes": "K - 2f picked rows read, P rows written"}
            kernels["trimmed_mean (same rows, same process)"] = {"ms": round(ms_trim, 4), "GBps": round(2 * PEERS * n * 4 / ms_trim / 1e6, 1),
                                                                 "bytes": "K rows read, P rows written"}
            kernels["whole call (3 launches)"] = {"ms": round(ms_all, 4)}
        elif agg_name == "dnc":
            scratch = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(PEERS)]
            ms_all_tiles = event_ms(dev, lambda: ops.dnc_into(flats, [], w, 1, subsample_dims=None), it, wu)
            ms_sub = event_ms(dev, lambda: ops.dnc_into(flats, [], w, 1, subsample_dims=10000), it, wu)
            ms_sub3 = event_ms(dev, lambda: ops.dnc_into(flats, [], w, 1, iters=3, subsample_dims=10000), it, wu)
            ms_krum = event_ms(dev, lambda: ops.krum_into(flats, [], w, 1, 3), it, wu)
            ms_whole = event_ms(dev, lambda: ops.dnc_into(flats, scratch, w, 1, subsample_dims=10000), it, wu)
            taken = float(ops.dnc_tiles(n, 0, 0, 1, 10000)[3].mean())
            kernels["dnc_sqdist+select (all tiles)"] = {"ms": round(ms_all_tiles, 4), "GBps": round(PEERS * n * 4 / ms_all_tiles / 1e6, 1), "bytes": "K rows read"}
            kernels["dnc_sqdist+select (subsample_dims 10000)"] = {"ms": round(ms_sub, 4), "tiles_taken": round(taken, 4),
                                                                   "GBps": round(taken * PEERS * n * 4 / ms_sub / 1e6, 1), "bytes": "the taken tiles of K rows read"}
            kernels["dnc_sqdist+select (subsample_dims 10000, iters 3)"] = {"ms": round(ms_sub3, 4)}
            kernels["krum pairwise_sqdist+select (same rows, same process)"] = {"ms": round(ms_krum, 4), "GBps": round(PEERS * n * 4 / ms_krum / 1e6, 1),
                                                                               "bytes": "K rows read"}
            kernels["whole call (3 launches, subsample_dims 10000)"] = {"ms": round(ms_whole, 4)}
        else:
            scratch = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(PEERS)]
            ms = event_ms(dev, lambda: ops.trimmed_mean_into(flats, scratch, 1), it, wu)
            kernels["trimmed_mean"] = {"ms": round(ms, 4), "GBps": round(2 * PEERS * n * 4 / ms / 1e6, 1), "bytes": "K rows read, P rows written"}
        return {"model": model_name, "aggregator": agg_name, "peers": PEERS, "n": n, "device": str(dev), "device_path": spread(t_dev), "generic_path": spread(t_gen),
                "speedup_median": round(statistics.median(t_gen) / statistics.median(t_dev), 2), "max_abs_diff_device_vs_generic": diff, "kernels": kernels,
                "measured": dev.type == "cuda"}
    finally:
        for nd in nodes:
            nd.stop()
        Federation.reset()


def run_attack_case(model_name: str, k: int, kinds, args) -> dict:
    """``ops.collude_into`` (K honest rows, 2 attackers' rows written) next to ``ops.krum_into`` on
    the same rows in the same process, device events over a window of back-to-back calls. The rows
    are plain device tensors of the model's trainable size: no nodes, no collective."""
    import torch

    from myfyp_amd import ops

    dev = torch.device(args.device)
    if model_name == "mlp":
        n = 235146
    else:
        from myfyp_amd.models import ResNet18

        n = sum(p.numel() for p in ResNet18(seed=0).parameters())
    g = torch.Generator().manual_seed(1)
    base = torch.randn(n, generator=g) * 0.05
    rows = [(base + 1e-3 * (1 + 0.15 * i) * 0.05 * torch.randn(n, generator=g)).to(dev) for i in range(k)]
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
    ref = (base + 2e-3 * 0.05 * torch.randn(n, generator=g)).to(dev)
    w = [1.0] * k
    it, wu = args.kernel_iters, args.warmup
    res = {}
    for kind in kinds:
        ms = event_ms(dev, lambda: ops.collude_into(rows, outs, kind, z=1.0, ref=ref if kind == "ipm" else None), it, wu)
        reads = {"alie": 1, "ipm": 1}.get(kind, 3)  # min-max / min-sum read the K rows three times (distances, statistics, write)
        nbytes = (reads * k + 2 + (1 if kind == "ipm" else 0)) * n * 4
        res[kind] = {"ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "launches": 1 if reads == 1 else 4,
                     "bytes": f"K rows read {reads}x, 2 rows written" + (", ref read" if kind == "ipm" else "")}
    ms_sel = event_ms(dev, lambda: ops.krum_into(rows, [], w, 2, 1), it, wu)
    ms_all = event_ms(dev, lambda: ops.krum_into(rows, outs, w, 2, 1), it, wu)
    res["krum select only (same rows, same process)"] = {"ms": round(ms_sel, 4), "GBps": round(k * n * 4 / ms_sel / 1e6, 1), "launches": 2, "bytes": "K rows read"}
    res["krum whole call (same rows, same process)"] = {"ms": round(ms_all, 4), "launches": 3}
    return {"model": model_name, "op": "collude_into", "honest_rows": k, "outputs": 2, "n": n, "device": str(dev), "kernels": res, "measured": dev.type == "cuda"}


def main() -> None:
    args = parse()
    import torch

    from myfyp_amd.settings import Settings

    if args.device == "cuda" and not torch.cuda.is_available():
        raise SystemExit("bench_robust_agg needs a GPU (use --device cpu only to rehearse the plumbing)")
    Settings.DEVICE = args.device
    Settings.LOG_LEVEL = "WARNING"
    if args.attack:  # the colluding attacks alone, beside Krum on the same rows
        kinds = ["alie", "ipm", "min_max", "min_sum"] if args.attack == "all" else [a for a in args.attack.split(",") if a]
        for model_name in [m for m in args.models.split(",") if m]:
            for k in (8, 16):
                print(json.dumps(run_attack_case(model_name, k, kinds, args)), flush=True)
        return
    for model_name in [m for m in args.models.split(",") if m]:
        for agg_name in [a for a in args.aggregators.split(",") if a]:
            print(json.dumps(run_case(model_name, agg_name, args)), flush=True)


if __name__ == "__main__":
    main()
