"""CPU: the order of memory requests and waits at the head of the tall loop's two kernels, read from the device assembly that hipcc
produces for admm_amd/csrc/lasso_tall.hip with the library's own flags (scripts/prologue_waits.py; no GPU, skipped without hipcc).

The sources say that a tile of the x-update issues everything it needs from memory before its first matrix request in ONE batch
behind the kernel arguments, and that the Lasso tail is one memory round trip.  Both were true once and then silently stopped being
true: a guard on both sides of a load let the compiler put the load's wait directly behind it, scalar loads were sunk below a branch,
a register pair half of which was a pending load's destination fed an address.  Nothing computes differently when that happens, so
no other test can see it; this one reads the compiled order.
  * the four default x-update instantiations (symv1_packed_kernel and symv1_lower_kernel with TallGate and TallDecideExtra, plain and
    non-temporal): no vector-memory wait and at most two lgkmcnt(0) waits (the kernel arguments; the batch) before the first matrix
    request (buffer_load_dwordx4 of the packed stream, global_load_dwordx4 of the fp32 matrix);
  * tall_tail_kernel<TAIL_SYMV1>: no vector-memory wait between its first and its twenty-fourth vector load (sixteen partials, eight
    element loads of the owner lanes)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("prologue_waits", os.path.join(ROOT, "scripts", "prologue_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _hipcc():
    from admm_amd import build as b
    return b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("hipcc not found")
    pw = _tool()
    out = tmp_path_factory.mktemp("tall_asm") / "lasso_tall.s"
    pw.compile_asm(str(out))
    return pw, out.read_text()


XUPDATE = [("symv1_packed_kernelINS_8TallGateENS_15TallDecideExtraELb0ELi8E", r"buffer_load_dwordx4"),
           ("symv1_packed_kernelINS_8TallGateENS_15TallDecideExtraELb1ELi8E", r"buffer_load_dwordx4"),
           ("symv1_lower_kernelINS_8TallGateENS_15TallDecideExtraELb0ELi8E", r"global_load_dwordx4"),
           ("symv1_lower_kernelINS_8TallGateENS_15TallDecideExtraELb1ELi8E", r"global_load_dwordx4")]


@pytest.mark.parametrize("kernel,stop", XUPDATE, ids=["packed", "packed-nt", "fp32", "fp32-nt"])
def test_a_tile_waits_for_nothing_but_its_arguments_and_one_batch_before_the_matrix(asm, kernel, stop):
    pw, text = asm
    name, lines = pw.find_kernel(text, kernel)
    ev = pw.prologue(lines, stop=stop)
    listing = "\n".join(f"{k:8s}{t}" for k, t in ev)
    assert ev[-1][0] == "request" and stop in ev[-1][1]
    assert pw.vector_waits(ev) == [], f"{name}: a vector-memory wait before the first matrix request\n{listing}"
    assert len(pw.scalar_waits(ev)) <= 2, f"{name}: more than two lgkmcnt(0) waits before the first matrix request\n{listing}"
    # the batch is in there: the six norm partials of the gate (two rows of three columns) are requested ahead of the matrix
    assert sum(1 for k, t in ev if k == "request" and t.startswith("global_load_dwordx2")) == 6, listing


def test_the_lasso_tail_requests_partials_and_elements_without_a_wait_between(asm):
    pw, text = asm
    name, lines = pw.find_kernel(text, r"tall_tail_kernelILi4E")
    ev = pw.prologue(lines, loads=24)
    first = next(i for i, (k, t) in enumerate(ev) if k == "request" and pw.VECTOR_LOAD.match(t))
    listing = "\n".join(f"{k:8s}{t}" for k, t in ev[first:])
    assert sum(1 for k, t in ev[first:] if k == "request" and pw.VECTOR_LOAD.match(t)) == 24
    assert pw.vector_waits(ev[first:]) == [], f"{name}: a vector-memory wait inside the tail's one batch\n{listing}"


def test_the_tool_finds_waits_where_there_are_some():
    """The reader itself: a hand-written head with the defect this file guards against."""
    pw = _tool()
    text = "\n".join(["\t.amdhsa_kernel k1", "k1:", "\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\ts_waitcnt lgkmcnt(0)",
                      "\tglobal_load_dwordx2 v[0:1], v[2:3], off", "\ts_waitcnt vmcnt(0)", "\tv_add_f64 v[0:1], v[0:1], 0",
                      "\ts_load_dword s2, s[0:1], 0x0", "\ts_waitcnt lgkmcnt(0)", "\ts_load_dword s3, s[0:1], 0x4", "\ts_waitcnt lgkmcnt(0)",
                      "\tbuffer_load_dwordx4 v[4:7], v8, s[8:11], 0 offen", "\ts_endpgm", ".Lfunc_end0:"])
    name, lines = pw.find_kernel(text, "k1")
    ev = pw.prologue(lines, stop="buffer_load_dwordx4")
    assert [k for k, _ in ev] == ["request", "wait", "request", "wait", "request", "wait", "request", "wait", "request"]
    assert pw.vector_waits(ev) == ["s_waitcnt vmcnt(0)"] and len(pw.scalar_waits(ev)) == 3
    with pytest.raises(LookupError):
        pw.prologue(lines, loads=5)
    with pytest.raises(LookupError):
        pw.find_kernel(text, "nothing")
