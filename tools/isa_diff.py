#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds of the library, kernel by kernel ("Where the set-up helpers live"):

    isa_diff.py OLD.so NEW.so      exit status 1 when a kernel is `changed` or exists on one side only

    identical   same instruction text
    permuted    same multiset of instruction lines (operands included, branch targets normalised) AND the same code-object
                metadata: VGPR / AGPR / SGPR counts, LDS bytes, private segment, occupancy
    changed     anything else

A refactor of the kernels' shared set-up code must leave every kernel `identical` or `permuted`.  The tool only compares the
two builds with each other; it looks for no particular instruction.  Disassembly: tools/isa_pk_scan.py, metadata:
tools/scratch_scan.py."""
import collections
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
BRANCH = re.compile(r"^(s_c?branch\w*)\s+\S+$")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def occupancy(meta):
    """waves per SIMD the unified register file (512 per lane, granules of 8) allows, at most 8"""
    regs = (meta.get("vgpr_count", 0) + 7) // 8 * 8
    return min(8, 512 // regs) if regs else 8


def functions(path):
    """{symbol: [instruction text, ...]} of every gfx950 code object in the file (addresses and encodings dropped)"""
    pk, out, cur = _tool("isa_pk_scan"), {}, None
    for blob in pk.code_objects(path):
        for ln in pk.disassemble(blob).splitlines():
            m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", ln.strip())
            if m:
                cur = out.setdefault(m.group(1), [])
            elif cur is not None and ln.startswith("\t"):
                cur.append(" ".join(ln.split("//")[0].split()))
    return out


def classify(old_fn, new_fn, old_meta, new_meta):
    if old_fn == new_fn:
        return "identical"
    norm = lambda ins: collections.Counter(BRANCH.sub(r"\1 L", i) for i in ins)
    same_meta = all(old_meta.get(k, 0) == new_meta.get(k, 0) for k in META) and occupancy(old_meta) == occupancy(new_meta)
    return "permuted" if same_meta and norm(old_fn) == norm(new_fn) else "changed"


def main(old, new):
    scratch = _tool("scratch_scan")
    meta = [scratch.kernels(old), scratch.kernels(new)]
    code = [functions(old), functions(new)]
    only = [sorted(set(meta[0]) - set(meta[1])), sorted(set(meta[1]) - set(meta[0]))]
    count = collections.Counter()
    rows = []
    for k in sorted(set(meta[0]) & set(meta[1])):
        c = classify(code[0].get(k), code[1].get(k), meta[0][k], meta[1][k])
        count[c] += 1
        if c != "identical":
            m = meta[1][k]
            rows.append(f"{c:9s} {len(code[1].get(k) or [])} instructions, " +
                        ", ".join(f"{key.split('_')[0]} {meta[0][k].get(key, 0)} -> {m.get(key, 0)}" for key in META) +
                        f", occupancy {occupancy(meta[0][k])} -> {occupancy(m)}  {k}")
    print(f"old: {len(meta[0])} kernels, new: {len(meta[1])} kernels; identical {count['identical']}, "
          f"permuted {count['permuted']}, changed {count['changed']}, only old {len(only[0])}, only new {len(only[1])}")
    for r in rows:
        print(r)
    for side, names in zip(("old", "new"), only):
        for k in names:
            print(f"only {side}  {k}")
    return 1 if count["changed"] or only[0] or only[1] else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
