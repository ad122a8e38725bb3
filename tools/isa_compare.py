#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assemblies of the same source file, before and after a refactor.

    hipcc <the flags of build.py> --cuda-device-only -S csrc/kernels.hip -o old.s     (parent commit)
    hipcc <the flags of build.py> --cuda-device-only -S csrc/kernels.hip -o new.s     (this tree)
    python tools/isa_compare.py old.s new.s > profiles/<name>_isa_compare.txt

Used on both kernel files, kernels.hip and kernels64.hip, each plain and with -DBCE_PHASE_PROF (the phase marks are device
code too): profiles/lat_variant_isa_compare.txt, profiles/wd_variant_isa_compare.txt.

A kernel's body is the text from its label to .Lfunc_end without comments, directives and blank lines, with the
function number taken out of the local labels (.LBB<n>_ -> .LBB_).  Kernels are paired by the hash of the body, not by
name, so renamed instantiations pair up; the table has old name, new name, hash, and VGPRs / SGPRs / spilled VGPRs /
scratch bytes of both sides.  Exit status 1 if the two multisets of hashes differ, a body refers to a kernel by name
(the names would then enter the hash; a device variable's name does, rightly), or a pair differs in one of the four numbers.

    python tools/isa_compare.py --by-name old.s new.s

pairs the kernels by NAME instead, for a change that touches the bodies: same / CHANGED with the four numbers of both sides, and
whether the body's hash is the same.  Exit status 1 if the two sets of names differ, or a kernel uses more VGPRs, spills more or has
more scratch than before (SGPRs may move: they do not limit occupancy on gfx950 below 106).
"""
import collections
import hashlib
import re
import subprocess
import sys

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")


def kernels(path):
    """{name: (hash, (the four numbers))} of every .amdhsa_kernel of an assembly file"""
    text = open(path).read()
    lines = text.split("\n")
    start = {m.group(1): i for i, m in enumerate(re.match(r"(\w+):", ln) for ln in lines) if m}
    meta = {}
    for blk in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        meta[name] = tuple(int(re.search(r"^\s+%s:\s+(\d+)" % re.escape(k), blk, re.M).group(1)) for k in META)
    out = {}
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    for name in names:
        body = []
        for ln in lines[start[name] + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = ln.split(";")[0].strip()
            if ln and not (ln.startswith(".") and not ln.endswith(":")):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        body = "\n".join(body)
        if any(n in body for n in names):
            sys.exit("%s: the body of %s refers to a kernel by name" % (path, name))
        out[name] = (hashlib.sha256(body.encode()).hexdigest()[:16], meta[name])
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    got = res.stdout.split("\n") if res.returncode == 0 else names
    # without the return type and the argument list (the last top-level parenthesis; "(bce::Fwd)3" inside <> stays)
    return {n: re.sub(r"^void |\((?:[^()]|\([^()]*\))*\)$", "", d) for n, d in zip(names, got)}


def by_name(old, new, old_path, new_path):
    pretty = demangle(sorted(set(old) | set(new)))
    bad = changed = 0
    print("# %d kernels in %s, %d in %s, paired by name; columns: vgpr / sgpr / spilled vgpr / scratch bytes (old -> new), body, name"
          % (len(old), old_path.split("/")[-1], len(new), new_path.split("/")[-1]))
    for name in sorted(set(old) | set(new), key=lambda n: pretty[n]):
        if name not in old or name not in new:
            bad += 1
            print("%-8s  %-44s  %-9s  %s" % ("ADDED" if name in new else "MISSING", "/".join(map(str, (new.get(name) or old[name])[1])), "", pretty[name]))
            continue
        (ho, mo), (hn, mn) = old[name], new[name]
        worse = mn[0] > mo[0] or mn[2] > mo[2] or mn[3] > mo[3]
        bad += worse
        changed += mo != mn
        print("%-8s  %-44s  %-9s  %s" % ("MORE" if worse else "same" if mo == mn else "CHANGED", "/".join(map(str, mo)) + ("" if mo == mn else " -> " + "/".join(map(str, mn))),
                                          "same body" if ho == hn else "new body", pretty[name]))
    print("# %s" % ("%d kernels, none with more VGPRs, spills or scratch; %d with other SGPR counts" % (len(old), changed) if not bad else "%d with MORE VGPRs, spills or scratch, or unpaired" % bad))
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--by-name":
        return by_name(kernels(sys.argv[2]), kernels(sys.argv[3]), sys.argv[2], sys.argv[3])
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    by_hash = collections.defaultdict(list)
    for name, (h, _) in new.items():
        by_hash[h].append(name)
    pretty = demangle(sorted(set(old) | set(new)))
    bad = 0
    print("# %d kernels in %s, %d in %s; columns: hash, vgpr / sgpr / spilled vgpr / scratch bytes (old -> new), old name -> new name"
          % (len(old), sys.argv[1].split("/")[-1], len(new), sys.argv[2].split("/")[-1]))
    for name in sorted(old, key=lambda n: pretty[n]):
        h, m = old[name]
        if not by_hash[h]:
            bad += 1
            print("%s  %-24s  MISSING   %s" % (h, "/".join(map(str, m)), pretty[name]))
            continue
        # several kernels with one body: keep the same name if it is there
        other = name if name in by_hash[h] else by_hash[h][0]
        by_hash[h].remove(other)
        same = new[other][1] == m
        bad += not same
        print("%s  %-24s  %-8s  %s -> %s" % (h, "/".join(map(str, m)) + ("" if same else " -> " + "/".join(map(str, new[other][1]))),
                                              "same" if same else "DIFFERS", pretty[name], pretty[other] if other != name else "="))
    for h, names in sorted(by_hash.items()):
        for name in names:
            bad += 1
            print("%s  %-24s  ADDED     %s" % (h, "/".join(map(str, new[name][1])), pretty[name]))
    print("# %s" % ("identical: %d kernels, every body and register count" % len(old) if not bad else "%d MISMATCHES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
