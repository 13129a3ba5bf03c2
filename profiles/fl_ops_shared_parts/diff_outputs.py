"""How far two dumps of dump_outputs.py are apart: per op, the files that are not byte-equal and the
largest relative difference of a value in them.

    python diff_outputs.py out/parent14 out/child14
"""

import collections
import os
import sys

import numpy as np


def main(a, b):
    per = collections.defaultdict(lambda: [0, 0, 0.0, []])  # files, differing, max relative difference, names
    for name in sorted(os.listdir(a)):
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        p = per[name.split("_K")[0]]
        p[0] += 1
        if x.tobytes() != y.tobytes():
            p[1] += 1
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.abs(x64 - y64) / np.maximum(np.abs(x64), np.abs(y64))
            p[2] = max(p[2], float(np.nanmax(np.where(x64 == y64, 0.0, rel))))
            p[3].append(name)
    for op, (n, d, rel, names) in per.items():
        print(f"{op:20} {n:4} files, {d:3} differ, max relative difference {rel:.3e}  {' '.join(names[:6])}{' ...' if len(names) > 6 else ''}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
