"""Call every robust op of fl_ops.hip and save every device output as .npy, to compare two builds of
the native library byte for byte (select a build with MYFYP_NATIVE_LIB):

    MYFYP_NATIVE_LIB=<parent>/libmyfyp_hip.so python dump_outputs.py out/parent
    python dump_outputs.py out/child
    for f in out/parent/*.npy; do cmp $f out/child/$(basename $f); done

A second argument names other K (of 1, 2, 8, 14, 15, 16): ``python dump_outputs.py out/child14 14,15``;
diff_outputs.py of this folder says how far two such dumps are apart.

K in {lowest, 8, 16}, n in {5, 1027, 600001} (all odd: row i of a packed [K, n] buffer is 4-byte aligned
only), rows aligned and packed, fixed seeds. n = 600001 reaches the 512-block cap of the slab kernels, so
the slab sum's eight-wide loop and its remainder both run.
"""

import os
import sys

import numpy as np
import torch

from myfyp_amd import ops
from myfyp_amd.ops import _native

NS = [5, 1027, 600001]


def rows_of(k, n, seed, dev, packed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    x = torch.stack([base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g) for i in range(k)])
    if k > 5:
        x[5] = -base
    if packed:
        buf = x.to(dev)
        return [buf[i] for i in range(k)]
    return [x[i].to(dev).clone() for i in range(k)]


def main(out_dir, ks=(1, 2, 8, 16)):
    _native.load(required=True)
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda")
    count = 0

    def save(name, tensors):
        nonlocal count
        for i, t in enumerate(tensors):
            np.save(os.path.join(out_dir, f"{name}_{i}.npy"), t.detach().cpu().numpy())
            count += 1

    for n in NS:
        for packed in (False, True):
            def out():
                return torch.empty(2, n, device=dev)[1] if packed else torch.empty(n, device=dev)

            for k in ks:
                tag = f"K{k}_n{n}_{'packed' if packed else 'aligned'}"
                w = [float(1 + (3 * i) % 7) for i in range(k)]
                f = {1: 0, 2: 0, 8: 1, 14: 2, 15: 3, 16: 3}[k]

                def rows(seed):
                    return rows_of(k, n, seed, dev, packed)

                if k != 2:  # the families whose lowest K is 1
                    o = out()
                    ops.median_into(rows(1), [o])
                    save(f"median_{tag}", [o])
                    for trim in sorted({0, (k - 1) // 2}):
                        o = out()
                        ops.trimmed_mean_into(rows(2), [o], trim)
                        save(f"trimmed{trim}_{tag}", [o])
                    o = out()
                    save(f"krum_{tag}", [*ops.krum_into(rows(3), [o], w, f, 3), o])
                    o = out()
                    save(f"bulyan_{tag}", [*ops.bulyan_into(rows(4), [o], f), o])
                    o = out()
                    save(f"geomed_{tag}", [*ops.geometric_median_into(rows(5), [o], w, iters=2, nu=1e-6), o])
                    for iters, b in ((1, None), (2, 300 if n < 100000 else 10000)):
                        if iters * f >= k and f > 0:
                            continue
                        o = out()
                        save(f"dnc{iters}_{tag}", [*ops.dnc_into(rows(6), [o], w, f, 1.0, iters, b, seed=11, round=2), o])
                    g = torch.Generator().manual_seed(7)
                    ref = (rows(8)[0] + 2e-3 * torch.randn(n, generator=g).to(dev)).contiguous()
                    for kind in ("alie", "ipm", "min_max", "min_sum"):
                        o = out()
                        save(f"collude_{kind}_{tag}", [*ops.collude_into(rows(8), [o], kind, z=1.5, eps=0.5, ref=ref if kind == "ipm" else None), o])
                if k != 1:  # ClippedGossip's lowest K is 2
                    wm = np.zeros((k, k))
                    for p in range(k):
                        for q in {(p - 1) % k, (p + 1) % k} - {p}:
                            wm[p, q] = 0.25
                    for kw in ({"tau": 0.02}, {"num_byzantine": 1}):
                        r = rows(9)
                        res = ops.clipped_gossip_into(r, wm, **kw)
                        save(f"clip_{'fixed' if 'tau' in kw else 'adaptive'}_{tag}", [*res, *r])
    torch.cuda.synchronize()
    print(f"{count} files in {out_dir}")


if __name__ == "__main__":
    main(sys.argv[1], *([tuple(int(k) for k in sys.argv[2].split(","))] if len(sys.argv) > 2 else []))
