"""Compare two device assembly files of fl_ops.hip (hipcc --cuda-device-only -S) kernel by kernel.

The parsing follows profiles/f32_host_tables/compare_kernels.py, but a kernel runs from its .protected
line to the next one, so kernels that are no templates (they share the .text section) count too. That
script asks for identical text; this change moves device code into inlined helpers, which the compiler
unrolls before it inlines them and schedules differently, so this one asks for what must hold and
reports the rest:

  must hold   the same kernel symbols; per kernel the same LDS size and kernarg size, no scratch where the
              parent has none, and no .vgpr_count that falls into a lower waves-per-SIMD step
  reported    per kernel family: how many instantiations differ in text, and by how many instructions

    python compare_kernels.py parent.s child.s [-v]      (-v: one line per kernel whose text differs)
"""

import collections
import re
import sys

_ORD = re.compile(r"(\bBB|\.LBB|Lfunc_begin|Lfunc_end|Ltmp)\d+")
_PAD = re.compile(r"[ \t]+;")
_BEGIN = re.compile(r"^\t\.protected\t(\S+)")
_INSN = re.compile(r"^\t[a-z]")
_FAMILY = re.compile(r"k_[a-z_0-9]+")
_MUST = (".group_segment_fixed_size", ".kernarg_segment_size")


def parse(path):
    kernels, meta, cur, where, entry = {}, {}, None, "text", None
    for line in open(path):
        if where == "meta":
            if line.startswith("  - ") or not line.startswith(" "):
                if entry is not None and ".name" in entry:
                    meta[entry[".name"]] = entry
                entry = {} if line.startswith("  - ") else None
            if entry is not None and ":" in line:
                key, _, val = line.strip().lstrip("- ").partition(":")
                entry[key.strip()] = val.strip()
            continue
        if line.startswith("amdhsa.kernels:"):
            where = "meta"
            continue
        m = _BEGIN.match(line)
        if m:
            cur = m.group(1)
            kernels[cur] = []
        if line.startswith("\t.section\t.AMDGPU.gpr_maximums"):
            cur = None
        # (.p2alignl / .fill: the padding behind whichever kernel the module emits last)
        if cur is not None and not line.startswith(("\t.section\t.text", "\t.text", "\t.p2alignl", "\t.fill")):
            kernels[cur].append(_PAD.sub(" ;", _ORD.sub(r"\1", line)))
    return kernels, meta


def waves(vgprs):
    """Waves per SIMD of gfx950 for a wave's VGPR + AGPR count: 512 registers, allocated in eights."""
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))


def insns(text):
    return sum(1 for l in text if _INSN.match(l))


def main(a, b, verbose=False):
    ka, ma = parse(a)
    kb, mb = parse(b)
    bad = 0
    if set(ka) != set(kb) or set(ma) != set(mb) or set(ma) != set(ka):
        print("kernel symbols differ:", sorted(set(ka) ^ set(kb)), sorted(set(ma) ^ set(mb)))
        bad += 1
    fam = collections.defaultdict(lambda: [0, 0, [], 0])  # kernels, differing, instruction deltas, vgpr changes
    for k in sorted(set(ka) & set(kb)):
        f = fam[_FAMILY.search(k).group(0)]
        f[0] += 1
        pa, pb = ma[k], mb[k]
        for key in _MUST:
            if pa[key] != pb[key]:
                print(f"{key} differs: {k}: {pa[key]} -> {pb[key]}")
                bad += 1
        if int(pa[".private_segment_fixed_size"]) == 0 and int(pb[".private_segment_fixed_size"]) != 0:
            print(f"scratch appears: {k}: {pb['.private_segment_fixed_size']} bytes")
            bad += 1
        va, vb = int(pa[".vgpr_count"]), int(pb[".vgpr_count"])
        if waves(vb) < waves(va):
            print(f"fewer waves per SIMD: {k}: {va} VGPRs ({waves(va)}) -> {vb} ({waves(vb)})")
            bad += 1
        f[3] += va != vb
        if ka[k] != kb[k]:
            f[1] += 1
            f[2].append(insns(kb[k]) - insns(ka[k]))
            if verbose:
                print(f"  {k}: instructions {insns(ka[k])} -> {insns(kb[k])}, VGPRs {va} -> {vb}, SGPRs {pa['.sgpr_count']} -> {pb['.sgpr_count']}")
    print(f"{'family':28}{'kernels':>8}{'text differs':>14}{'instructions (min .. max)':>28}{'VGPR count differs':>20}")
    for name, (n, d, deltas, v) in sorted(fam.items()):
        span = f"{min(deltas):+d} .. {max(deltas):+d}" if deltas else "-"
        print(f"{name:28}{n:8}{d:14}{span:>28}{v:20}")
    print(f"{len(ka)} kernels, {sum(f[1] for f in fam.values())} differ in text: {'OK' if not bad else f'{bad} VIOLATIONS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], "-v" in sys.argv[3:]))
