#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files kernel by kernel (no GPU needed).

    hipcc <product flags> --cuda-device-only -S ray_tracer_2_amd/csrc/rt_kernel.hip -o new.s     (and the same at the parent)
    python3 tools/kernel_isa_diff.py parent.s new.s

Each file is split per kernel (`.type NAME,@function` ... `.Lfunc_endN`).  Labels that carry the function's number in
the file (.LBB<n>_, .Lfunc_end<n>, .LJTI<n>_, ...) are renumbered and comments (the `%bb.` ones among them) dropped, so
that moving code between files or reordering functions cannot show up as a difference.  Printed per kernel: identical
or different, instruction counts, and vgpr / sgpr / agpr / scratch / LDS from the metadata, with the waves-per-SIMD tier
floor(512 / roundup(vgpr, 8)).  Instantiations renamed by a new trailing `false` template argument are matched to their old names.  Exit status 1 when the two files do not hold the same set of kernels.
"""
import re
import sys

LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(?=_|\b)")
FIELDS = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("agpr", "agpr_count"), ("scratch", "private_segment_fixed_size"),
          ("lds", "group_segment_fixed_size"))


def metadata(text):
    """{kernel name: {field: int}} from the amdhsa.kernels block."""
    out = {}
    md = text[text.index("amdhsa.kernels:"):]
    for ent in re.split(r"\n  - ", md)[1:]:
        name = re.search(r"\.name:\s+(\S+)", ent)
        if not name:
            continue
        out[name.group(1).strip("'\"")] = {k: int(re.search(rf"\.{f}:\s+(\d+)", ent).group(1)) for k, f in FIELDS}
    return out


def bodies(text, names):
    """{kernel name: normalised lines} for the functions that are kernels."""
    out = {}
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        i += 1
        if not m or m.group(1) not in names:
            continue
        body = []
        while i < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[i]):
            line = lines[i].split(";", 1)[0].rstrip()
            if line.strip():
                body.append(LOCAL_LABEL.sub(lambda l: f".L{l.group(1)}#", line))
            i += 1
        out[m.group(1)] = body
    return out


def instructions(body):
    return sum(1 for l in body if not l.lstrip().startswith(".") and not l.rstrip().endswith(":"))


def tier(vgpr):
    return 512 // max(8, (vgpr + 7) // 8 * 8)


def load(path):
    text = open(path).read()
    md = metadata(text)
    return md, bodies(text, md)


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    (md_a, body_a), (md_b, body_b) = load(argv[1]), load(argv[2])
    # A template that gained a trailing bool argument renames its old instantiations (`...Lb0EEEvNS_` -> `...Lb0ELb0EEEvNS_`):
    # a kernel of the first file that is missing from the second is compared with the second's kernel of that longer name
    # (argument false), under the first file's name.
    for name in sorted(set(md_a) - set(md_b)):
        longer = name.replace("EEEvNS_", "ELb0EEEvNS_", 1)
        if longer != name and longer in md_b and longer not in md_a:
            md_b[name] = md_b.pop(longer)
            body_b[name] = [l.replace(longer, name) for l in body_b.pop(longer)]
            print(f"  compared under its old name: {longer}")
    only_a, only_b = sorted(set(md_a) - set(md_b)), sorted(set(md_b) - set(md_a))
    print(f"kernels: {len(md_a)} in {argv[1]}, {len(md_b)} in {argv[2]}; name sets {'equal' if not only_a and not only_b else 'DIFFER'}")
    for n in only_a:
        print(f"  only in the first : {n}")
    for n in only_b:
        print(f"  only in the second: {n}")
    n_same = 0
    for name in sorted(set(md_a) & set(md_b)):
        same = body_a[name] == body_b[name]
        n_same += same
        a, b = md_a[name], md_b[name]
        res = "  ".join(f"{k} {a[k]}" if a[k] == b[k] else f"{k} {a[k]}->{b[k]}" for k, _ in FIELDS)
        ia, ib = instructions(body_a[name]), instructions(body_b[name])
        ins = f"{ia}" if ia == ib else f"{ia}->{ib}"
        ta, tb = tier(a["vgpr"]), tier(b["vgpr"])
        print(f"{'identical' if same else 'DIFFERENT'}  instr {ins:>14s}  {res}  tier {ta if ta == tb else f'{ta}->{tb}'}  {name}")
    print(f"{n_same} of {len(set(md_a) & set(md_b))} common kernels identical after normalisation")
    return 1 if only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
