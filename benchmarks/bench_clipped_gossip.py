"""ClippedGossip's three launches against the plain neighbour mix on the same stacked buffer.

    python benchmarks/bench_clipped_gossip.py
    python benchmarks/bench_clipped_gossip.py --sizes mlp --rounds 5

For P = 8 and 16 rows of a ``[P, S]`` stacked fp32 buffer (S: n rounded up to 64 floats, as the
engines pad their rows) on a ring, at the MLP's size (n = 235,146), LeNet-5's and one
bandwidth-bound size (4 Mi floats per row: 128 / 256 MiB of rows), two things are timed with device
events over a window of back-to-back calls, alternating in one process for ``--rounds`` rounds:

* clipped: ``myfyp_clipped_gossip`` (``k_pairwise_sqdist<P>``, ``k_clip_plan``, ``k_clipped_mix<P>``;
  adaptive radius, b = 1) with its buffers allocated before the window: the launches alone;
* plain  : ``myfyp_neighbor_mix_stacked`` (``k_neighbor_mix<P>``), one launch.

The rows are restored, untimed, before every window (one row is −10 times the shared model). GB/s
from the bytes the algorithm needs: the clipped mix reads the rows twice and writes them once
(3·P·n·4), the plain mix reads and writes them once (2·P·n·4); from traffic alone the ratio to expect
where bandwidth binds is 1.5, and three launch latencies against one at the small sizes. One JSON
line per (size, P) with the median and the minimum over the rounds. Needs a GPU: there is no CPU mode.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="mlp,lenet5,big")
    ap.add_argument("--peers", default="8,16")
    ap.add_argument("--rounds", type=int, default=7, help="alternating (clipped, plain) windows per case")
    ap.add_argument("--iters", type=int, default=0, help="calls per window (0: sized so that a window moves about 20 GB, 20..400)")
    ap.add_argument("--warmup", type=int, default=5)
    return ap.parse_args()


def size_of(name: str) -> int:
    if name == "mlp":
        return 235146
    if name == "lenet5":
        from myfyp_amd.models import LeNet5

        return sum(p.numel() for p in LeNet5(seed=0).parameters())
    return 1 << 22


def ring(p: int):
    import numpy as np

    w = np.zeros((p, p), dtype=np.float32)
    for i in range(p):
        w[i, (i - 1) % p] = w[i, (i + 1) % p] = 1.0 / 3.0
    return w


def window_ms(fn, iters: int) -> float:
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def run_case(name: str, p: int, args) -> dict:
    import numpy as np
    import torch

    from myfyp_amd import ops

    lib = ops.fast_lib()
    dev = torch.device("cuda")
    n = size_of(name)
    s = (n + 63) // 64 * 64
    g = torch.Generator().manual_seed(1)
    base = torch.randn(n, generator=g) * 0.05
    rows0 = torch.zeros(p, s)
    for i in range(p):
        rows0[i, :n] = -10.0 * base if i == 2 else base + 1e-3 * 0.05 * torch.randn(n, generator=g)
    rows0 = rows0.to(dev)
    buf = rows0.clone()
    shares = ring(p)
    mix = shares.copy()
    np.fill_diagonal(mix, 1.0 / 3.0)
    pairs = p * (p - 1) // 2
    work = torch.empty(max(1, int(lib.myfyp_krum_grid(n, p)) * pairs), dtype=torch.float32, device=dev)
    dist = torch.empty(p * p, dtype=torch.float64, device=dev)
    tau = torch.empty(p, dtype=torch.float64, device=dev)
    w_eff = torch.empty(p * p, dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_uint64 * p)(*[buf[i].data_ptr() for i in range(p)])
    stream = torch.cuda.current_stream().cuda_stream

    def clipped() -> None:
        ops.check(lib.myfyp_clipped_gossip(ctypes.cast(ptrs, ctypes.c_void_p), p, shares.ctypes.data, 1, 0.0, 1, n, work.data_ptr(), dist.data_ptr(),
                                           tau.data_ptr(), w_eff.data_ptr(), stream), "clipped_gossip")

    def plain() -> None:
        ops.check(lib.myfyp_neighbor_mix_stacked(buf.data_ptr(), p, n, s, mix.ctypes.data, stream), "neighbor_mix")

    iters = args.iters or int(min(400, max(20, 20e9 / (3 * p * n * 4))))
    for fn in (clipped, plain):
        buf.copy_(rows0)
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    t_clip, t_plain = [], []
    for _ in range(args.rounds):  # alternating: both see the same machine state
        for fn, out in ((clipped, t_clip), (plain, t_plain)):
            buf.copy_(rows0)
            torch.cuda.synchronize()
            out.append(window_ms(fn, iters))
    # what one clipped call did to the rows, for the record: the attacker's neighbours barely move
    buf.copy_(rows0)
    clipped()
    torch.cuda.synchronize()
    scale = (w_eff.view(p, p).cpu().numpy() / np.where(shares > 0, shares, 1.0))
    med_c, med_p = statistics.median(t_clip), statistics.median(t_plain)
    return {"size": name, "n": n, "peers": p, "rows_MiB": round(p * n * 4 / 2**20, 1), "iters_per_window": iters, "rounds": args.rounds,
            "clipped_ms": {"median": round(med_c, 4), "min": round(min(t_clip), 4), "max": round(max(t_clip), 4)},
            "plain_ms": {"median": round(med_p, 4), "min": round(min(t_plain), 4), "max": round(max(t_plain), 4)},
            "ratio_median": round(med_c / med_p, 3), "ratio_min": round(min(t_clip) / min(t_plain), 3),
            "clipped_GBps": round(3 * p * n * 4 / med_c / 1e6, 1), "plain_GBps": round(2 * p * n * 4 / med_p / 1e6, 1),
            "attacker_scale": [round(float(scale[1, 2]), 5), round(float(scale[3, 2]), 5)], "device": torch.cuda.get_device_name(0), "measured": True}


def main() -> None:
    args = parse()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_clipped_gossip needs a GPU")
    for name in [x for x in args.sizes.split(",") if x]:
        for p in [int(x) for x in args.peers.split(",") if x]:
            print(json.dumps(run_case(name, p, args)), flush=True)


if __name__ == "__main__":
    main()
