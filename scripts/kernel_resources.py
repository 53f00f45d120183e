#!/usr/bin/env python3
"""Per kernel of a device assembly file: registers, LDS, scratch, occupancy and a hash of the instructions (host only, no GPU).

    python scripts/kernel_resources.py fadmm_dense.s                    # one line per kernel
    python scripts/kernel_resources.py before.s after.s                 # the kernels that differ, and a summary
    python scripts/kernel_resources.py --compile                        # compile admm_amd/csrc/fadmm_dense.hip first

The assembly is what scripts/prologue_waits.py's compile_asm writes (hipcc, the library's flags, --cuda-device-only -S); the kernels
and their instruction lines are that file's kernels().  The hash is over the instruction lines with comments stripped, white space
collapsed and the numbers of local labels (.LBB12_3) replaced by the order of their first appearance in the kernel, so that a kernel
that moved within the file keeps its hash.  profiles/lad_loss_table.md was written from this; tests/test_lad_kernels_asm.py reads the
scratch column.
"""
import argparse
import hashlib
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prologue_waits as pw  # noqa: E402

FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def instruction_hash(lines):
    seen = {}
    h = hashlib.sha256()
    for line in lines:
        text = re.sub(r"\s+", " ", line.split(";")[0]).strip()
        if text:
            h.update(LOCAL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), text).encode() + b"\n")
    return h.hexdigest()[:16]


def resources(asm_text):
    """{mangled name: {vgpr, sgpr, lds, scratch, occupancy, hash}} for every kernel of the file."""
    out = {}
    for name, lines in pw.kernels(asm_text).items():
        desc = re.search(r"^\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$(.*?)^\s*\.end_amdhsa_kernel", asm_text, flags=re.M | re.S).group(1)
        vals = [int(re.search(r"\.amdhsa_" + f + r"\s+(\d+)", desc).group(1)) for f in FIELDS]
        # the resource comments follow the kernel's code: the first "; Occupancy:" behind its label
        label = re.search(r"^" + re.escape(name) + r":", asm_text, flags=re.M)
        occ = re.search(r"^; Occupancy:\s*(\d+)", asm_text[label.end():], flags=re.M)
        out[name] = dict(zip(("vgpr", "sgpr", "lds", "scratch"), vals), occupancy=int(occ.group(1)), hash=instruction_hash(lines))
    return out


def _row(name, r):
    return f"{name}  vgpr {r['vgpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['scratch']} occ {r['occupancy']} {r['hash']}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", nargs="*", help="one assembly file to list, or two (before, after) to compare")
    ap.add_argument("--compile", action="store_true", help="compile admm_amd/csrc/fadmm_dense.hip (hipcc, the build's flags) and list it")
    a = ap.parse_args()
    if a.compile:
        with tempfile.TemporaryDirectory() as d:
            with open(pw.compile_asm(os.path.join(d, "fadmm_dense.s"), src=os.path.join(pw.ROOT, "admm_amd", "csrc", "fadmm_dense.hip"))) as fh:
                tables = [resources(fh.read())]
    else:
        if len(a.asm) not in (1, 2):
            ap.error("give one or two assembly files, or --compile")
        tables = []
        for path in a.asm:
            with open(path) as fh:
                tables.append(resources(fh.read()))
    if len(tables) == 1:
        for name in sorted(tables[0]):
            print(_row(name, tables[0][name]))
        return
    before, after = tables
    print(f"kernels: {len(before)} before, {len(after)} after; names identical: {sorted(before) == sorted(after)}")
    same = [n for n in sorted(before) if n in after and before[n] == after[n]]
    print(f"identical (resources and instruction hash): {len(same)}")
    for name in sorted(set(before) | set(after)):
        if name in same:
            continue
        print(name)
        for tag, t in (("  before", before), ("  after ", after)):
            print(tag, _row("", t[name]) if name in t else " absent")


if __name__ == "__main__":
    main()
