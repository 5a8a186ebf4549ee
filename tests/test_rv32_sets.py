"""What a verifier pins for each rv32 chip set (raiko_amd.executor.rv32_verifier_tables) and the registry constants,
against literals: the heights below are written out, not computed from the module that holds the chip sets."""
import numpy as np
import pytest

from raiko_amd import executor as X, p3, rv32, rv32cf

CPU_LOG, PROGRAM_LOG = 6, 9
ROOT = np.arange(1, 9, dtype=np.uint32)                   # any eight words: rv32_verifier_tables only asks whether there is a root
# set -> (keyed, the pinned heights, how many heights the proof carries: muldiv, then memop and memory)
SETS = {"rv32i": (False, [6, 0, 5, 18, 16], 0),
        "rv32i-cf": (False, [6, 0, 5, 18, 16, 12], 0),
        "rv32im": (False, [6, 0, 5, 18, 16, 12], 1),
        "rv32im-elf": (True, [6, 9, 5, 18, 16, 12], 1),
        "rv32im-mem": (True, [6, 9, 5, 18, 16, 12], 3)}
_airs = {}


def tables_of(chips, n=None):
    """trace-less tables over the set's AIRs (the first n, cycled when n is larger), the cpu table at 2^6 rows"""
    if chips not in _airs:
        _airs[chips] = X._rv32_airs_of(chips)
    airs = _airs[chips]
    out = []
    for i in range(len(airs) if n is None else n):
        a = airs[i % len(airs)]
        t = p3.Table(a, None, np.zeros(a.n_public, dtype=np.uint32))
        t.log_height = CPU_LOG if i == 0 else 1
        out.append(t)
    return out


def header(logs, words=16):
    """a proof's first words as far as rv32_verifier_tables reads them: word 1 + i is table i's log height"""
    pf = np.zeros(words, dtype=np.uint32)
    stated = list(logs)[:words - 1]
    pf[1:1 + len(stated)] = stated
    return pf


def vk(chips):
    return dict(prep_root=ROOT, program_log_height=PROGRAM_LOG) if SETS[chips][0] else {}


def heights(chips, carried, **kw):
    pinned = SETS[chips][1]
    # the header states other heights for the pinned tables than the verifier pins: they must not be taken from it
    vt = X.rv32_verifier_tables(tables_of(chips), header([3] * len(pinned) + list(carried), **kw), **vk(chips))
    return None if vt is None else [t.log_height for t in vt]


def test_the_literals_are_the_modules_constants():
    assert rv32.BYTE_LOG_ROWS == 18 and rv32cf.SHIFT_LOG_ROWS == 12


@pytest.mark.parametrize("chips", list(SETS))
def test_pinned_and_carried_heights(chips):
    _keyed, pinned, n_carried = SETS[chips]
    carried = [4, 7, 3][:n_carried]                       # muldiv below the cpu's 6; memop one above it, which is allowed
    tables = tables_of(chips)
    assert len(tables) == len(pinned) + n_carried
    vt = X.rv32_verifier_tables(tables, header([3] * len(pinned) + carried), **vk(chips))
    assert [t.log_height for t in vt] == pinned + carried
    assert all(v.trace is None and v.air is t.air and np.array_equal(v.public_values, t.public_values) for v, t in zip(vt, tables))
    if n_carried:
        assert heights(chips, [6, 1, 1][:n_carried]) == pinned + [6, 1, 1][:n_carried]     # the muldiv table as tall as the cpu's


@pytest.mark.parametrize("chips", ["rv32im", "rv32im-elf", "rv32im-mem"])
def test_a_muldiv_height_out_of_range_is_refused(chips):
    rest = [2, 2][:SETS[chips][2] - 1]
    assert heights(chips, [0] + rest) is None
    assert heights(chips, [7] + rest) is None
    assert heights(chips, [6] + rest) is not None


def test_a_memory_height_out_of_range_is_refused():
    for memop, memory in ((8, 2), (2, 8), (0, 2), (2, 0)):
        assert heights("rv32im-mem", [4, memop, memory]) is None
    assert heights("rv32im-mem", [4, 7, 7]) == [6, 9, 5, 18, 16, 12, 4, 7, 7]


@pytest.mark.parametrize("chips", ["rv32im", "rv32im-elf", "rv32im-mem"])
def test_a_proof_too_short_for_its_heights_is_refused(chips):
    n = len(SETS[chips][1]) + SETS[chips][2]
    assert heights(chips, [4, 4, 4][:SETS[chips][2]], words=1 + n) is not None
    assert heights(chips, [4, 4, 4][:SETS[chips][2]], words=n) is None          # the last table's height is past the end
    assert heights(chips, [4, 4, 4][:SETS[chips][2]], words=1) is None


def test_a_table_count_no_set_has_is_an_error():
    for n in (4, 8):
        with pytest.raises(ValueError):
            X.rv32_verifier_tables(tables_of("rv32im-mem", n), header([4] * n))
        with pytest.raises(ValueError):
            X.rv32_verifier_tables(tables_of("rv32im-mem", n), header([4] * n), prep_root=ROOT, program_log_height=PROGRAM_LOG)
    # the count is looked up among the sets of the same keyed-ness only
    with pytest.raises(ValueError):
        X.rv32_verifier_tables(tables_of("rv32im-mem"), header([4] * 9))
    with pytest.raises(ValueError):
        X.rv32_verifier_tables(tables_of("rv32i"), header([4] * 5), prep_root=ROOT, program_log_height=PROGRAM_LOG)


@pytest.mark.parametrize("chips", ["rv32im-elf", "rv32im-mem"])
def test_a_root_without_the_program_height_is_an_error(chips):
    with pytest.raises(ValueError):
        X.rv32_verifier_tables(tables_of(chips), header([4] * 9), prep_root=ROOT, program_log_height=None)


def test_registry_constants():
    assert X.CHIPS == ("trace", "rv32i", "rv32i-cf", "rv32im", "rv32im-elf", "rv32im-mem")
    assert X.RV32_CHIPS == ("rv32i", "rv32i-cf", "rv32im", "rv32im-elf", "rv32im-mem")
    assert X.KEYED_CHIPS == ("rv32im-elf", "rv32im-mem")
