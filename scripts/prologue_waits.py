#!/usr/bin/env python3
"""Memory requests and waits at the head of a kernel, read from device assembly (host only, no GPU).

    hipcc <admm_amd/build.py's CXXFLAGS> --cuda-device-only -S admm_amd/csrc/lasso_tall.hip -o lasso_tall.s
    python scripts/prologue_waits.py lasso_tall.s --kernel 'symv1_packed_kernel.*TallGate.*Lb0ELi8' --stop buffer_load_dwordx4
    python scripts/prologue_waits.py --compile --kernel 'tall_tail_kernelILi4E' --loads 24

For the kernel whose (mangled) name matches --kernel it prints, in the order of the assembly text, every memory request
(scalar, vector, buffer and LDS loads, stores, atomics), every s_waitcnt and every s_barrier from the kernel's entry up to the
first line that matches --stop (the stop line included), or up to the --loads'th vector load.  The order of the text is the order
of execution where the prologue is straight-line code or its branches only skip forward, which is what the tall kernels' heads are.

tests/test_tall_prologue_asm.py imports this file: the x-update's tiles must have every prologue request out before their first
vector wait, and the Lasso tail its partial and element requests before any.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUEST = re.compile(r"^\s*((?:s_load|s_buffer_load|global_load|global_store|global_atomic|buffer_load|buffer_store|buffer_atomic|"
                     r"flat_load|flat_store|flat_atomic|scratch_load|scratch_store|ds_read|ds_write|ds_bpermute|ds_permute)\w*)\b")
WAIT = re.compile(r"^\s*(s_waitcnt\b.*|s_barrier\b)")
VECTOR_LOAD = re.compile(r"^\s*(?:global_load|buffer_load|flat_load)\w*")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def compile_asm(out_path, src=None, extra_flags=()):
    """Device assembly of one translation unit with the flags of the library's build."""
    sys.path.insert(0, ROOT)
    from admm_amd import build as b
    src = src or os.path.join(b.CSRC, "lasso_tall.hip")
    cmd = [b.HIPCC] + list(b.CXXFLAGS) + list(extra_flags) + ["--cuda-device-only", "-S", src, "-o", out_path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed:\n{r.stderr[-4000:]}")
    return out_path


def kernels(asm_text):
    """{mangled name: list of its instruction lines}, for every .amdhsa kernel of the file."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, flags=re.M))
    out, cur = {}, None
    for line in asm_text.splitlines():
        m = LABEL.match(line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end") or line.lstrip().startswith(".section") or line.lstrip().startswith(".amdhsa_kernel"):
            cur = None
            continue
        cur.append(line)
    return out


def find_kernel(asm_text, pattern):
    ks = kernels(asm_text)
    hits = [k for k in ks if re.search(pattern, k)]
    if len(hits) != 1:
        raise LookupError(f"{len(hits)} kernels match {pattern!r}: {hits[:8]}")
    return hits[0], ks[hits[0]]


def _clean(line):
    return re.sub(r"\s+", " ", line.split(";")[0]).strip()


def prologue(lines, stop=None, loads=None):
    """Ordered [(kind, text)] with kind in {'request', 'wait'} from the kernel's entry up to and including the first line matching
    `stop`, or the `loads`'th vector load.  Raises if the end is not reached."""
    stop_re = re.compile(stop) if stop else None
    events, nload = [], 0
    for line in lines:
        text = _clean(line)
        if not text:
            continue
        is_stop = bool(stop_re and stop_re.search(text))
        if REQUEST.match(text):
            events.append(("request", text))
            if VECTOR_LOAD.match(text):
                nload += 1
                if loads is not None and nload >= loads:
                    return events
        elif WAIT.match(text):
            events.append(("wait", text))
        if is_stop:
            return events
    raise LookupError(f"the kernel ends before {'the stop pattern ' + repr(stop) if stop else str(loads) + ' vector loads'}")


def vector_waits(events):
    return [t for k, t in events if k == "wait" and "vmcnt" in t]


def scalar_waits(events):
    return [t for k, t in events if k == "wait" and re.search(r"lgkmcnt\(0\)", t)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", nargs="?", help="device assembly of lasso_tall.hip (omit with --compile)")
    ap.add_argument("--compile", action="store_true", help="compile admm_amd/csrc/lasso_tall.hip first (hipcc, the build's flags)")
    ap.add_argument("--kernel", required=True, help="regular expression on the mangled kernel name; must match exactly one")
    ap.add_argument("--stop", default=None, help="regular expression: the listing ends with the first line that matches")
    ap.add_argument("--loads", type=int, default=None, help="... or with this many vector loads")
    a = ap.parse_args()
    if a.stop is None and a.loads is None:
        ap.error("give --stop or --loads")
    if a.compile:
        with tempfile.TemporaryDirectory() as d:
            with open(compile_asm(os.path.join(d, "lasso_tall.s"))) as fh:
                text = fh.read()
    else:
        with open(a.asm) as fh:
            text = fh.read()
    name, lines = find_kernel(text, a.kernel)
    ev = prologue(lines, a.stop, a.loads)
    print(name)
    for kind, t in ev:
        print(f"  {'WAIT   ' if kind == 'wait' else 'request'}  {t}")
    print(f"vector waits: {len(vector_waits(ev))}   lgkmcnt(0) waits: {len(scalar_waits(ev))}")


if __name__ == "__main__":
    main()
