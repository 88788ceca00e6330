#!/usr/bin/env python3
"""Compare the device code of two builds of the same translation units, kernel by kernel (DESIGN.md sections 17 and 18).

    hipcc <the flags of build.sh> -Rpass-analysis=kernel-resource-usage --save-temps -c X.hip     (once per tree, each in a directory of its own)
    python3 scratch/asm_compare.py PARENT_DIR RESULT_DIR

Reads every *-gfx950.s of the two directories.  Prints, per kernel, the figures of both sides (SGPRs, VGPRs, AGPRs, scratch bytes per
lane, SGPR and VGPR spill counts, LDS bytes, occupancy) and whether the kernel's normalised assembly is equal; then, per file, whether
the whole normalised file is.  Normalised: without the `.file` / `.ident` lines, the lines that name the compilation unit's id symbol
(`__hip_cuid_*`, a hash of the source text) and comments (the compiler names inlined functions in its basic-block comments).
Exit status: 1 when kernel names or figures differ, 2 on usage errors, else 0 -- differing assembly alone is reported, not an error.
"""
import glob
import os
import re
import sys

FIGS = ["sgpr", "vgpr", "agpr", "scratch", "sgpr_spill", "vgpr_spill", "lds", "occupancy"]
META = {".sgpr_count": "sgpr", ".vgpr_count": "vgpr_total", ".agpr_count": "agpr", ".private_segment_fixed_size": "scratch",
        ".sgpr_spill_count": "sgpr_spill", ".vgpr_spill_count": "vgpr_spill", ".group_segment_fixed_size": "lds"}
INFO = {"NumVgprs": "vgpr", "Occupancy": "occupancy"}


def normalise(lines):
    out = []
    for ln in lines:
        if "__hip_cuid_" in ln or re.match(r"\s*\.(file|ident)\b", ln):
            continue
        if not re.match(r"\s*\.(asciz|ascii|string)\b", ln):
            ln = ln.split(";", 1)[0]
        ln = ln.rstrip()
        if ln:
            out.append(ln)
    return out


def read_unit(path):
    lines = open(path, errors="replace").read().split("\n")
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    figs = {n: {} for n in names}
    body = {}
    # the code of a kernel: from its label to its .Lfunc_end; the "; Kernel info:" comment block behind it
    cur, start, info = None, 0, None
    for i, ln in enumerate(lines):
        m = re.match(r"(\S+):\s*(;.*)?$", ln)
        if m and m.group(1) in figs and cur is None:
            cur, start = m.group(1), i
        elif cur is not None and re.match(r"\.Lfunc_end\d+:", ln):
            body[cur] = normalise(lines[start:i])
            info, cur = cur, None
        elif info is not None:
            m = re.match(r";\s*(\w+)\s*:\s*(\d+)", ln)
            if m and m.group(1) in INFO:
                figs[info][INFO[m.group(1)]] = int(m.group(2))
            if m and m.group(1) == "Occupancy":
                info = None
    # the metadata: one entry per kernel
    entry = {}
    for ln in lines[lines.index("amdhsa.kernels:") if "amdhsa.kernels:" in lines else len(lines):]:
        m = re.match(r"(?:  - |    )(\.\w+):\s+(\S+)\s*$", ln)      # (the entry's own keys, not those of its .args)
        if ln.startswith("  - ") or not ln.startswith(" "):
            if entry.get(".name") in figs:
                figs[entry[".name"]].update({v: int(entry[k]) for k, v in META.items() if k in entry})
            entry = {}
        if m:
            entry[m.group(1)] = m.group(2)
    return names, figs, body, normalise(lines)


def main():
    if len(sys.argv) != 3 or not all(os.path.isdir(d) for d in sys.argv[1:]):
        print(__doc__)
        return 2
    units = [{os.path.basename(p): p for p in glob.glob(os.path.join(d, "*-gfx950.s"))} for d in sys.argv[1:]]
    bad = False
    if set(units[0]) != set(units[1]) or not units[0]:
        print("assembly files differ:", sorted(units[0]), sorted(units[1]))
        return 1
    for u in sorted(units[0]):
        (na, fa, ba, wa), (nb, fb, bb, wb) = read_unit(units[0][u]), read_unit(units[1][u])
        print(f"== {u}: {len(na)} / {len(nb)} kernels")
        for n in sorted(set(na) ^ set(nb)):
            print(f"NAME only in {'parent' if n in na else 'result'}: {n}")
            bad = True
        n_fig = n_asm = 0
        for n in na:
            if n not in fb:
                continue
            va, vb = [fa[n].get(k) for k in FIGS], [fb[n].get(k) for k in FIGS]
            same_f, same_a = va == vb and None not in va, ba.get(n) == bb.get(n) and n in ba
            n_fig += not same_f
            n_asm += not same_a
            txt = " ".join(f"{k} {x}" if x == y else f"{k} {x}->{y}" for k, x, y in zip(FIGS, va, vb))
            print(f"{'same figures' if same_f else 'FIGURES DIFFER'} | {'same assembly' if same_a else 'ASSEMBLY DIFFERS'} "
                  f"({len(ba.get(n, []))} / {len(bb.get(n, []))} lines) | {txt} | {n}")
        bad = bad or n_fig > 0
        print(f"== {u}: {n_fig} kernels with other figures, {n_asm} with other assembly; whole normalised file "
              f"{'equal' if wa == wb else 'DIFFERENT'} ({len(wa)} / {len(wb)} lines)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
