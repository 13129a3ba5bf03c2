"""Compare two device assembly files (hipcc --cuda-device-only -S) kernel by kernel, whatever order
the kernels were emitted in: the same kernel symbols, and per symbol identical text (instructions,
.amdhsa_* block, resource comments) and identical metadata entry. Local labels carry the function's
ordinal (.LBB12_3, .Lfunc_end12, "Header=BB12_16" in comments); the ordinal is dropped, and with it the
padding in front of a comment, which depends on the label's length. What follows the last kernel (globals,
addrsig) must be identical too, without the __hip_cuid_ lines.

    python compare_kernels.py parent.s child.s
"""

import re
import sys

_ORD = re.compile(r"(\.LBB|=BB|Lfunc_begin|Lfunc_end|Ltmp)\d+")
_PAD = re.compile(r"[ \t]+;")
_TEXT = re.compile(r"^\t\.section\t\.text\.(\S+?),")


def parse(path):
    kernels, tail, meta, cur, where = {}, [], {}, None, "text"
    entry = None
    for line in open(path):
        if "__hip_cuid_" in line:
            continue
        if where == "meta":
            if line.startswith("  - ") or not line.startswith(" "):
                if entry is not None:
                    name = [l.split()[-1] for l in entry if l.startswith("    .name:")]
                    if name:
                        meta[name[0]] = entry
                    else:
                        tail.extend(entry)  # (amdhsa.version's list)
                entry = [line] if line.startswith("  - ") else None
                if entry is None:
                    tail.append(line)
            elif entry is not None:
                entry.append(line)
            continue
        if line.startswith("amdhsa.kernels:"):
            where = "meta"
            continue
        m = _TEXT.match(line)
        if m and m.group(1) != cur:
            cur = m.group(1)
            kernels[cur] = []
        if line.startswith("\t.section\t.AMDGPU.gpr_maximums"):
            cur = None  # the module's own lines and the globals after the last kernel
        (tail if cur is None else kernels[cur]).append(_PAD.sub(" ;", _ORD.sub(r"\1", line)))
    return kernels, tail, meta


def main(a, b):
    ka, ta, ma = parse(a)
    kb, tb, mb = parse(b)
    bad = 0
    if set(ka) != set(kb):
        print("kernel symbols differ:", sorted(set(ka) ^ set(kb)))
        bad += 1
    if set(ma) != set(mb) or set(ma) != set(ka):
        print("metadata entries differ:", sorted(set(ma) ^ set(mb)), sorted(set(ma) ^ set(ka)))
        bad += 1
    for k in sorted(set(ka) & set(kb)):
        if ka[k] != kb[k]:
            print("text differs:", k)
            bad += 1
        if ma.get(k) != mb.get(k):
            print("metadata differs:", k)
            bad += 1
    if ta != tb:
        print("the text outside the kernels differs")
        bad += 1
    epoch = sum("mlp_persistent_f32_epoch" in k for k in ka)
    print(f"{len(ka)} kernels ({epoch} mlp_persistent_f32_epoch), {sum(map(len, ka.values()))} lines of kernel text, same order: {list(ka) == list(kb)}: {'IDENTICAL' if not bad else f'{bad} DIFFERENCES'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
