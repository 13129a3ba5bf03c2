"""Time DnC's k_dnc_sqdist<11, true> + k_dnc_select alone: the one kernel whose .vgpr_count crosses a
waves-per-SIMD step (README of this folder). K = 11 aligned rows of ResNet-18's size, every tile taken,
iters = 1 and 3 (gridDim.y = iters: with 3 the grid is 1536 blocks, six per CU, so the waves a SIMD can
hold matter). One JSON line in the format of benchmarks/bench_robust_agg.py, for bench_table.py.

    [MYFYP_NATIVE_LIB=<parent>/libmyfyp_hip.so] python bench_dnc_k11.py
"""

import json

import torch

from myfyp_amd import ops
from myfyp_amd.ops import _native

K, N, CALLS, WINDOWS = 11, 11_689_512, 20, 7


def main():
    _native.load(required=True)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    base = torch.randn(N, generator=g)
    rows = [(base + 1e-3 * torch.randn(N, generator=g)).to(dev) for _ in range(K)]
    assert all(r.data_ptr() % 16 == 0 for r in rows)
    w = [1.0] * K
    kernels = {}
    for iters in (1, 3):
        def call():
            ops.dnc_into(rows, [], w, 2, 1.0, iters, None, seed=11, round=2)

        for _ in range(5):
            call()
        best = []
        for _ in range(WINDOWS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                call()
            b.record()
            torch.cuda.synchronize()
            best.append(a.elapsed_time(b) / CALLS)
        best.sort()
        kernels[f"dnc_sqdist+select (all tiles, iters {iters})"] = {"ms": round(best[len(best) // 2], 4), "GBps": round(iters * K * N * 4 / best[len(best) // 2] / 1e6, 1)}
    print(json.dumps({"model": "resnet18-size", "aggregator": "dnc", "peers": K, "kernels": kernels}), flush=True)


if __name__ == "__main__":
    main()
