"""No inline asm in the kernels' sources issues a scalar memory load.  The registers such a load writes have no
interlock while it is in flight, and an asm statement that hands them back as an ordinary output lets the compiler copy
them before the wait: p2 KStream once did, hash_rows_multi_kernel at width 24 then read stale constants whenever a
second proof contended for memory, and uni-stark proofs changed from run to run.  Scalar loads are the compiler's to
issue (plain loads from the constant address space), so that its own wait-count tracking covers every copy and spill.
The run-time side is tests/test_gpu_p2_kept_cells.py::test_two_proofs_in_flight_repeat_under_the_width_24_set."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = sorted(p for ext in ("hip", "hpp", "h", "cpp") for p in glob.glob(os.path.join(ROOT, "raiko_amd", "csrc", "*." + ext)))
ASM = re.compile(r"\basm\s*(?:volatile\s*)?\((.*?)\)\s*;", re.S)
SMEM_LOAD = re.compile(r"\bs_(?:buffer_)?load_", re.I)


def asm_statements(text):
    return [m.group(1) for m in ASM.finditer(text)]


def test_the_scan_sees_asm_statements():
    core = open(os.path.join(ROOT, "raiko_amd", "csrc", "poseidon2_core.hpp")).read()
    got = asm_statements(core)
    assert any("v_mad_u64_u32" in a for a in got) and len(got) >= 5
    bad = 'asm volatile("s_load_dwordx16 %0, %1, 0x40"\n : "=s"(nxt) : "s"(p));'
    assert [bool(SMEM_LOAD.search(a)) for a in asm_statements(bad)] == [True]


def test_no_inline_asm_issues_a_scalar_load():
    assert len(SOURCES) > 20
    found = [(os.path.basename(p), a.split("\n")[0][:60]) for p in SOURCES for a in asm_statements(open(p).read()) if SMEM_LOAD.search(a)]
    assert found == []
