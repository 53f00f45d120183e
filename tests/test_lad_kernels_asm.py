"""CPU: the kernel table of the LAD loop, read from the device assembly that hipcc produces for admm_amd/csrc/fadmm_dense.hip with the
library's own flags (scripts/kernel_resources.py on scripts/prologue_waits.py; no GPU, skipped without hipcc).

kProxKinds' max_slots rows are "the instantiations without scratch": a slot more and the registers of quant_rows_kernel spill.  The
dispatch instantiates what the table admits, so the two cannot disagree -- but nothing else says that the table is still right under
the compiler at hand.  This does:
  * exactly 42 lad_rows_kernel (7 kinds x 6 layouts), 61 quant_rows_kernel (the table's sum of max_slots - 1) and 7 dense_tail_kernel;
  * every one of them with a private segment of 0 bytes."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"lad_rows_kernel": 42, "quant_rows_kernel": 61, "dense_tail_kernel": 7}


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _hipcc():
    from admm_amd import build as b
    return b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("hipcc not found")
    kr = _tool()
    out = tmp_path_factory.mktemp("lad_asm") / "fadmm_dense.s"
    kr.pw.compile_asm(str(out), src=os.path.join(ROOT, "admm_amd", "csrc", "fadmm_dense.hip"))
    return kr.resources(out.read_text())


@pytest.mark.parametrize("kernel", list(COUNTS))
def test_the_table_s_instantiations_and_no_others_none_with_scratch(table, kernel):
    mine = {k: r for k, r in table.items() if f"admm{len(kernel)}{kernel}I" in k}
    assert len(mine) == COUNTS[kernel], sorted(mine)
    spills = {k: r["scratch"] for k, r in mine.items() if r["scratch"] != 0}
    assert not spills, spills


def test_the_reader_on_a_hand_written_kernel():
    kr = _tool()
    text = "\n".join(["k1:", "\ts_load_dword s2, s[0:1], 0x0 ; comment", ".LBB7_2:", "\ts_cbranch_scc1 .LBB7_2", "\ts_endpgm", ".Lfunc_end0:",
                      "\t.section .rodata", "\t.amdhsa_kernel k1", "\t\t.amdhsa_group_segment_fixed_size 64", "\t\t.amdhsa_private_segment_fixed_size 16",
                      "\t\t.amdhsa_next_free_vgpr 9", "\t\t.amdhsa_next_free_sgpr 12", "\t.end_amdhsa_kernel", "; Occupancy: 8"])
    r = kr.resources(text)["k1"]
    assert (r["vgpr"], r["sgpr"], r["lds"], r["scratch"], r["occupancy"]) == (9, 12, 64, 16, 8)
    assert r["hash"] == kr.resources(text.replace("LBB7_2", "LBB9_5").replace("; comment", ""))["k1"]["hash"]
    assert r["hash"] != kr.resources(text.replace("s_endpgm", "s_nop 0\n\ts_endpgm"))["k1"]["hash"]
