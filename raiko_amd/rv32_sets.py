"""The rv32 chip sets (raiko_amd/rv32.py, rv32cf.py, rv32im.py, rv32elf.py, rv32mem.py) between the executor and the
uni-stark prover: what each set's shard looks like (SETS: one record per set, everything else here is derived from
it), its tables in numpy (`shards`) and written on the GPU (rv32_shard_device, execute_rv32_device), the key of the two
sets proven from one (setup_rv32_elf) and what a verifier pins (rv32_verifier_tables, verify_rv32_*)."""
import ctypes as C
from dataclasses import dataclass
from types import ModuleType
from typing import Sequence, Tuple

import numpy as np

from . import _lib, p3, rv32, rv32cf, rv32commit, rv32elf, rv32im, rv32io, rv32link, rv32mem
from .executor import Execution, Stepper, _rv32_side


@dataclass(frozen=True)
class ChipSet:
    """one shard of a chip set is the tables cpu, program, then one per entry of `fixed`, then muldiv, then the memory
    tables.  A verifier pins the cpu table to the height the statement gives, the program table to the key's (keyed; else
    the proof's) and the fixed ones to `fixed`; the others' heights are the proof's, within the bounds named below"""
    name: str
    module: ModuleType          # its AIRs (airs), numpy tables (shard_tables) and -- keyed -- preprocessed matrices (preps_of)
    entry: str                  # the C entry point that writes a shard's tables on the GPU
    fixed: Tuple[int, ...]      # log heights: register, byte, range[, shift]
    muldiv: bool = False        # a muldiv table of the height the segment needs: 0 < log height <= the cpu table's
    n_mem: int = 0              # memory tables (memop, memory) of the height the segment needs: ... <= the cpu table's + mem_slack
    mem_slack: int = 0
    prep: str = None            # keyed, proven under the key of setup_rv32_elf: the C entry point that writes its matrices
    extra: Tuple[str, ...] = ()  # what shard_tables takes after (seg, data, start, end, ecalls)

    @property
    def keyed(self):
        return self.prep is not None

    @property
    def n_tables(self):
        return 2 + len(self.fixed) + self.muldiv + self.n_mem


_RV32I = (5, rv32.BYTE_LOG_ROWS, rv32elf.RANGE_LOG_ROWS)
_RV32I_CF = _RV32I + (rv32cf.SHIFT_LOG_ROWS,)
SETS = (ChipSet("rv32i", rv32, "rk_exec_rv32_shard_device", _RV32I),
        ChipSet("rv32i-cf", rv32cf, "rk_exec_rv32cf_shard_device", _RV32I_CF),
        ChipSet("rv32im", rv32im, "rk_exec_rv32im_shard_device", _RV32I_CF, muldiv=True),
        ChipSet("rv32im-elf", rv32elf, "rk_exec_rv32elf_shard_device", _RV32I_CF, muldiv=True,
                prep="rk_rv32elf_prep_device", extra=("image",)),
        ChipSet("rv32im-mem", rv32mem, "rk_exec_rv32mem_shard_device", _RV32I_CF, muldiv=True, n_mem=2, mem_slack=1,
                prep="rk_rv32mem_prep_device", extra=("image", "mem")))
_BY_NAME = {cs.name: cs for cs in SETS}
RV32_CHIPS = tuple(_BY_NAME)
CHIPS = ("trace",) + RV32_CHIPS
KEYED_CHIPS = tuple(cs.name for cs in SETS if cs.keyed)
# a proof does not say which set made it: a verifier tells by whether there is a key and by the number of tables
_BY_COUNT = {}
for _cs in SETS:
    assert (_cs.keyed, _cs.n_tables) not in _BY_COUNT, "two chip sets a verifier could not tell apart"
    _BY_COUNT[_cs.keyed, _cs.n_tables] = _cs
# the io form of rv32im-mem (raiko_amd/rv32io.py; io=True, no chip-set name of its own): a key of its own and a tenth
# table, `io`, sized like the memory tables
_IO = ChipSet("rv32im-mem", rv32io, "rk_exec_rv32io_shard_device", _RV32I_CF, muldiv=True, n_mem=3, mem_slack=1,
              prep="rk_rv32io_prep_device", extra=("image", "mem", "io"))
assert (_IO.keyed, _IO.n_tables) not in _BY_COUNT
_BY_COUNT[_IO.keyed, _IO.n_tables] = _IO
# the commit form of the io form (raiko_amd/rv32commit.py; commit=True with io=True): the io form's key and table shapes, a
# wider memop and io table; a verifier tells it from the io form by the io table's 24 public values, not by a count
_COMMIT = ChipSet("rv32im-mem", rv32commit, "rk_exec_rv32commit_shard_device", _RV32I_CF, muldiv=True, n_mem=3, mem_slack=1,
                  prep="rk_rv32io_prep_device", extra=("image", "mem", "io", "commit"))


def _io_set(commit):
    return _COMMIT if commit else _IO


def _rv32_set(chips):
    """-> (the chip set's module, its ChipSet record)"""
    if chips not in _BY_NAME:
        raise ValueError("chips must be one of %s" % (RV32_CHIPS,))
    return _BY_NAME[chips].module, _BY_NAME[chips]


def _rv32_airs_of(chips, ext_w=None, link=False, io=False, commit=False):
    """the AIRs of one shard of chip set `chips`, in table order.  link: the rv32im-mem set with its shard memories
    linked (raiko_amd/rv32link.py: the memory AIR sends the journal and carries its digest).  io: the rv32im-mem set
    with its ecalls bound to the input (raiko_amd/rv32io.py: ten AIRs); composes with link.  commit (with io): the COMMIT
    journal bound as well (raiko_amd/rv32commit.py: the memop and io AIRs differ)"""
    _link_ok(chips, link, io, commit)
    if io:
        return (rv32commit if commit else rv32io).airs(ext_w, link)
    return (rv32link if link else _rv32_set(chips)[0]).airs(ext_w)


def _link_ok(chips, link, io=False, commit=False):
    if link and chips != "rv32im-mem":
        raise ValueError("link=True needs chips=\"rv32im-mem\"")
    if io and chips != "rv32im-mem":
        raise ValueError("io=True needs chips=\"rv32im-mem\"")
    if commit and not (io and chips == "rv32im-mem"):
        raise ValueError("commit=True needs chips=\"rv32im-mem\" and io=True")


def p3_rv32_airs(ext_w=None):
    """(cpu, program, register, byte, range): the AIRs of one rv32i shard, in table order (raiko_amd/rv32.py)"""
    return _rv32_airs_of("rv32i", ext_w)


def p3_rv32cf_airs(ext_w=None):
    """(cpu, program, register, byte, range, shift): the AIRs of one rv32i-cf shard, in table order
    (raiko_amd/rv32cf.py)"""
    return _rv32_airs_of("rv32i-cf", ext_w)


def p3_rv32im_airs(ext_w=None):
    """(cpu, program, register, byte, range, shift, muldiv): the AIRs of one rv32im shard, in table order
    (raiko_amd/rv32im.py)"""
    return _rv32_airs_of("rv32im", ext_w)


def _publics(seg, start, end, n_tables):
    """the public values of a shard's tables: the cpu table's pcs, the register table's registers before and after"""
    return [seg.pc_publics(), (), p3.to_mont(rv32.register_publics(start, end))] + [()] * (n_tables - 3)


def _host_preps(cs, image, n_tables):
    if not cs.keyed:
        return [None] * n_tables
    return [None if m is None else p3.to_mont(m) for m in cs.module.preps_of(image)]


def shards(chips, ex: Execution, image=None, ext_w=None, airs=None, link=False, params=None, io=False, input_words=None, commit=False):
    """one shard of chip set `chips` per executed segment, every table built in numpy (the set's shard_tables) from
    ex.witness, ex.rv32 and what else the set takes (image: rv32elf.program_image(elf); ex.mem) -> [(tables, init
    words)], init = the state digests as in p3_shards.  A keyed set's lookup tables carry their preprocessed matrix in
    Table.prep (p3.setup commits them).  link (rv32im-mem): rv32link's AIRs, the memory table's public values the digest
    of the shard's journal under `params` (None: the SP1 preset) -> [(tables, init words, journal)].  io (rv32im-mem,
    with input_words, the run's input): rv32io's ten tables from ex.ecall_args, the io table's public values the stream
    positions, N_INPUT, the exit and the digest of the shard's slice of the input; the result's shape is link's.  commit
    (with io): rv32commit's ten tables from ex.commit_reads as well; the shard's commit log (k, 3) uint32 is the last
    element of every entry."""
    module, cs = _rv32_set(chips)
    _link_ok(chips, link, io, commit)
    if io:
        return _io_shards(ex, image, ext_w, airs, link, params, input_words, commit)
    if link:
        module = rv32link
    if ex.witness is None or ex.rv32 is None or ("mem" in cs.extra and ex.mem is None):
        raise ValueError("execute(..., record_trace=True) first")
    airs = airs or module.airs(ext_w)
    preps = _host_preps(cs, image, len(airs))
    extra = {"image": lambda k: image, "mem": lambda k: ex.mem[k]}
    out = []
    for k, (s, (_code, data), (start, end, ecalls)) in enumerate(zip(ex.segments, ex.witness, ex.rv32)):
        canon, _pc, _regs, *digest = module.shard_tables(s, data, start, end, ecalls, *(extra[name](k) for name in cs.extra),
                                                          **(dict(params=params) if link else {}))
        pubs = _publics(s, start, end, len(canon))
        if link:
            pubs[rv32link.MEMORY_TABLE] = digest[0]
        tables = [p3.Table(a, p3.to_mont(t), pv, prep=pm) for a, t, pv, pm in zip(airs, canon, pubs, preps)]
        out.append((tables, s.init_words()) + ((rv32link.journal_of_table(canon[rv32link.MEMORY_TABLE]),) if link else ()))
    return out


def _io_shards(ex, image, ext_w, airs, link, params, input_words, commit=False):
    """`shards` in io form, or in commit form"""
    if ex.witness is None or ex.rv32 is None or ex.mem is None or ex.ecall_args is None or input_words is None or \
            (commit and ex.commit_reads is None):
        raise ValueError("execute(..., record_trace=True) first, and pass the run's input_words")
    airs = airs or (rv32commit if commit else rv32io).airs(ext_w, link)
    preps = _host_preps(_IO, image, len(airs))
    out = []
    for k, (s, (_code, data), (start, end, ecalls), mem, (args, pos)) in enumerate(zip(ex.segments, ex.witness, ex.rv32, ex.mem, ex.ecall_args)):
        if commit:
            reads, jpos = ex.commit_reads[k]
            canon, _pc, _regs, digest, io_pubs = rv32commit.shard_tables(s, data, start, end, ecalls, image, mem, args, reads,
                                                                         len(input_words), pos, jpos, params=params, link=link)
        else:
            canon, _pc, _regs, digest, io_pubs = rv32io.shard_tables(s, data, start, end, ecalls, image, mem, args, len(input_words), pos,
                                                                     params=params, link=link)
        pubs = _publics(s, start, end, len(canon))
        pubs[rv32io.IO_TABLE] = io_pubs
        if link:
            pubs[rv32link.MEMORY_TABLE] = digest
        tables = [p3.Table(a, p3.to_mont(t), pv, prep=pm) for a, t, pv, pm in zip(airs, canon, pubs, preps)]
        out.append((tables, s.init_words()) + ((rv32link.journal_of_table(canon[rv32link.MEMORY_TABLE]),) if link else ()) +
                   ((rv32commit.log_of_table(canon[rv32io.IO_TABLE]),) if commit else ()))
    return out


def p3_rv32_shards(ex: Execution, ext_w=None, airs=None):
    """rv32i shards in numpy: tables = cpu, program, register, byte, range (p3_rv32_airs).  The yardstick for the tables
    rk_exec_rv32_shard_device writes on the GPU."""
    return shards("rv32i", ex, None, ext_w, airs)


def p3_rv32cf_shards(ex: Execution, ext_w=None, airs=None):
    """rv32i-cf shards in numpy: tables = cpu, program, register, byte, range, shift (p3_rv32cf_airs).  The yardstick for
    the tables rk_exec_rv32cf_shard_device writes on the GPU."""
    return shards("rv32i-cf", ex, None, ext_w, airs)


def p3_rv32im_shards(ex: Execution, ext_w=None, airs=None):
    """rv32im shards in numpy: tables = cpu, program, register, byte, range, shift, muldiv (p3_rv32im_airs).  The
    yardstick for the tables rk_exec_rv32im_shard_device writes on the GPU."""
    return shards("rv32im", ex, None, ext_w, airs)


def p3_rv32elf_shards(ex: Execution, image, ext_w=None, airs=None):
    """rv32im-elf shards in numpy: tables = cpu, program, register, byte, range, shift, muldiv (rv32elf.airs), the four
    lookup tables with their preprocessed matrix in Table.prep (p3.setup commits them; rv32elf.prep_tables(image)).
    image: rv32elf.program_image(elf).  The yardstick for rk_rv32elf_prep_device / rk_exec_rv32elf_shard_device."""
    return shards("rv32im-elf", ex, image, ext_w, airs)


def p3_rv32mem_shards(ex: Execution, image, ext_w=None, airs=None):
    """rv32im-mem shards in numpy: rv32elf's seven tables, then memop and memory (rv32mem.airs), the four lookup tables
    with their preprocessed matrix in Table.prep (rv32mem.prep_tables(image)).  The yardstick for rk_rv32mem_prep_device
    / rk_exec_rv32mem_shard_device."""
    return shards("rv32im-mem", ex, image, ext_w, airs)


def rv32_shard_device(hal, handle, index, seg, airs, chips="rv32i", key=None, link=False, io=False, commit=False):
    """rk_exec_rv32_shard_device (chips="rv32i") / rk_exec_rv32cf_shard_device ("rv32i-cf") /
    rk_exec_rv32im_shard_device ("rv32im") / rk_exec_rv32elf_shard_device ("rv32im-elf", key: the program's Rv32Key) /
    rk_exec_rv32mem_shard_device ("rv32im-mem", key likewise): segment `index` of an open executor as the tables of a
    shard of that chip set, written on hal's GPU -> (tables without host traces, [(device buffer, log_height)] per
    table, init words).  link (rv32im-mem, airs rv32link's): after the tables are written rk_rv32mem_journal_device reads
    the memory table, its digest (under the parameter set of hal's context, which must be the prover's) becomes that
    table's public values and the journal (k, 3) uint32 is handed back as a fourth element.  io (rv32im-mem, airs
    rv32io's, key from setup_rv32_elf(io=True)): rk_exec_rv32io_shard_device writes the ten tables of the io form and
    hands back the io table's public values, the digest of the shard's slice of the input among them (committed under
    the parameter set of hal's context, which must be the prover's).  commit (with io, airs rv32commit's, the io key):
    rk_exec_rv32commit_shard_device writes the commit form's tables, the io table's public values are its 24 and the
    shard's commit log (k, 3) uint32 is handed back as the last element"""
    _module, cs = _rv32_set(chips)
    _link_ok(chips, link, io, commit)
    if io:
        cs = _io_set(commit)
    lib = _lib.load()
    start, end, _ec = _rv32_side(lib, handle, index)
    rows = C.c_size_t(0)
    if cs.keyed:
        if key is None or key.chips != chips or key.io != io:
            raise ValueError("chips=\"%s\" needs the Rv32Key of setup_rv32_elf(chips=\"%s\"%s)" % (chips, chips, ", io=True" if io else ""))
        rows.value = 1 << key.program_log_height
    else:
        _lib.check(None, lib.rk_exec_rv32_sizes(handle, index, C.byref(rows)))
    # per table in order: its log height, and its row count where the entry point takes one after the table's pointer
    logs, counts = [seg.po2, rows.value.bit_length() - 1, *cs.fixed], [None, rows.value] + [None] * len(cs.fixed)
    sized = [C.c_size_t(0) for _ in range(cs.muldiv + cs.n_mem)]
    if cs.muldiv:
        _lib.check(None, lib.rk_exec_rv32im_sizes(handle, index, C.byref(sized[0])))
    if cs.n_mem:    # a segment with more accesses than twice its cycles is refused here (RK_ERR_CAPACITY)
        _lib.check(None, getattr(lib, "rk_exec_rv32commit_sizes" if commit else "rk_exec_rv32io_sizes" if io else "rk_exec_rv32mem_sizes")(handle, index, *[C.byref(r) for r in sized[cs.muldiv:]]))
    logs += [r.value.bit_length() - 1 for r in sized]
    counts += [r.value for r in sized]
    if len(airs) != len(logs):
        raise ValueError("%d AIRs for the %d tables of %s" % (len(airs), len(logs), chips))
    bufs = [hal.alloc_elem(a.width << lg) for a, lg in zip(airs, logs)]
    args = []
    if cs.keyed:
        args += [key.seg_vaddr.ctypes.data_as(_lib.u32p), key.seg_words.ctypes.data_as(_lib.u32p), key.seg_vaddr.size,
                 C.c_void_p(key.d_words.ptr)]
    for b, n in zip(bufs, counts):
        args += [C.c_void_p(b.ptr)] + ([] if n is None else [n])
    io_pubs = np.zeros(rv32commit.N_PUBLIC_IO if commit else rv32io.N_PUBLIC_IO, dtype=np.uint32)
    if io:
        args.append(io_pubs.ctypes.data_as(_lib.u32p))
    d_log, n_log, commit_log = None, C.c_size_t(0), ()
    try:
        if commit:
            d_log = hal.alloc_elem(3 << logs[rv32io.IO_TABLE])
            args += [C.c_void_p(d_log.ptr), C.byref(n_log)]
        _lib.check(hal._ctx, getattr(lib, cs.entry)(hal._ctx, handle, index, *args))
        if commit:
            commit_log = (d_log.to_host().reshape(-1, 3)[: n_log.value].copy(),)
    except Exception:
        for b in bufs:
            b.free()
        raise
    finally:
        if d_log is not None:
            d_log.free()
    pubs = _publics(seg, start, end, len(logs))
    if io:
        pubs[rv32io.IO_TABLE] = io_pubs
    journal = ()
    if link:
        try:
            root, j = journal_device(hal, bufs[rv32link.MEMORY_TABLE], logs[rv32link.MEMORY_TABLE])
        except Exception:
            for b in bufs:
                b.free()
            raise
        pubs[rv32link.MEMORY_TABLE], journal = root, (j,)
    tables = [p3.Table.pinned(a, lg, pv) for a, lg, pv in zip(airs, logs, pubs)]
    return (tables, list(zip(bufs, logs)), seg.init_words()) + journal + commit_log


def journal_device(hal, d_memory, log_rows, keep=False):
    """rk_rv32mem_journal_device over a finished device memory table of 2^log_rows rows -> (root: 8 Montgomery words,
    journal (k, 3) uint32); keep: also the link matrix (rows, 6) and the count of real rows as the device reports it"""
    lib = _lib.load()
    rows = 1 << log_rows
    work = [hal.alloc_elem(3 * rows), hal.alloc_elem(rv32link.N_DIGEST * 2 * rows), hal.alloc_elem(len(rv32link.LINK_TUPLE) * rows)]
    try:
        root, n_real = np.zeros(rv32link.N_DIGEST, dtype=np.uint32), C.c_size_t(0)
        d_journal, d_nodes, d_link = (C.c_void_p(b.ptr) for b in work)
        _lib.check(hal._ctx, lib.rk_rv32mem_journal_device(hal._ctx, C.c_void_p(d_memory.ptr), rows, d_journal, d_link, d_nodes,
                                                           C.byref(n_real), root.ctypes.data_as(_lib.u32p)))
        journal = work[0].to_host().reshape(rows, 3)[: n_real.value].copy()
        if keep:
            return root, journal, work[2].to_host().reshape(rows, len(rv32link.LINK_TUPLE)).copy(), int(n_real.value)
        return root, journal
    finally:
        for b in work:
            b.free()


def next_rv32_shard(stepper: Stepper, hal, airs, chips="rv32i", key=None, link=False, io=False, commit=False):
    """the next executed segment as the tables of an rv32i (five), rv32i-cf (six), rv32im or rv32im-elf (seven) or
    rv32im-mem (nine) shard written on hal's GPU (rv32_shard_device; key: the Rv32Key of chips="rv32im-elf" /
    "rv32im-mem") -> (ExecSegment, tables without host traces, [(device buffer, log_height)] per table, init words),
    or None after the last.  link: as rv32_shard_device, the journal a fifth element.  io: as rv32_shard_device.  commit:
    as rv32_shard_device, the commit log the last element"""
    seg = stepper.step()
    return None if seg is None else (seg, *rv32_shard_device(hal, stepper._h, seg.index, seg, airs, chips, key, link, io, commit))


def _free(bufs):
    """the device buffers of a shard: [(device buffer, log_height), or None for a table on the host]"""
    for d in bufs:
        if d is not None:
            d[0].free()


def execute_rv32_device(hal, elf: bytes, input_words: Sequence[int] = (), shard_po2: int = 16, airs=None, ext_w=None,
                        chips="rv32i", key=None, link=False, io=False, commit=False):
    """ELF -> rv32i (rv32i-cf, rv32im, rv32im-elf) shards whose tables are written on hal's GPU, one segment at a time
    (the executor's trace of a segment is dropped with the executor; the tables stay in HBM) -> (Execution, [(tables,
    init)], [device traces], [[(device buffer, log_height)]] to free).  key: the Rv32Key of chips="rv32im-elf" (its AIRs
    are the shards').  link (rv32im-mem; key from setup_rv32_elf(link=True)): the shards' memories linked, the journals
    a fifth element of the result.  io (rv32im-mem; key from setup_rv32_elf(io=True)): the io form's ten tables.  commit
    (with io; key from setup_rv32_elf(io=True, commit=True)): the commit form's, the shards' commit logs the last element
    of the result"""
    from .hal import _ptr
    _link_ok(chips, link, io, commit)
    airs = airs or (key.airs if key is not None else _rv32_airs_of(chips, ext_w, link, io, commit))
    st = Stepper(elf, input_words, shard_po2)
    out, dev, metas, journals, logs = [], [], [], [], []
    try:
        while True:
            item = next_rv32_shard(st, hal, airs, chips, key, link, io, commit)
            if item is None:
                break
            seg, tables, bufs, init = item[:4]
            if commit:
                logs.append(item[-1])
                item = item[:-1]
            journals += item[4:]
            out.append((tables, init))
            dev.append(bufs)
            metas.append(seg)
        ex = st.finish()
        ex.segments = metas
    except Exception:
        for d in dev:
            _free(d)
        raise
    finally:
        st.close()
    return (ex, out, [[(_ptr(b), lg) for b, lg in d] for d in dev], dev) + ((journals,) if link else ()) + ((logs,) if commit else ())


def check_rv32_chain(publics, entry_pc=None):
    """the chaining of an rv32i run over its shards' public values: publics = [(cpu public values, register public
    values)] canonical per shard.  Every value a 16-bit limb, the first shard starting from all-zero registers (at
    entry_pc when given), shard k ending in the pc and registers shard k + 1 starts from.  Raises ValueError naming the
    shard."""
    prev_end = None
    for k, (pc, regs) in enumerate(publics):
        pc, regs = np.asarray(pc, dtype=np.int64), np.asarray(regs, dtype=np.int64)
        if pc.shape != (4,) or regs.shape != (128,) or (pc >= 1 << 16).any() or (regs >= 1 << 16).any():
            raise ValueError("shard %d: the public values are not 4 + 128 16-bit limbs" % k)
        start_pc, end_pc = int(pc[0] | pc[1] << 16), int(pc[2] | pc[3] << 16)
        if k == 0:
            if regs[:64].any():
                raise ValueError("shard 0: the registers do not start at zero")
            if entry_pc is not None and start_pc != entry_pc:
                raise ValueError("shard 0: does not start at the entry point")
        elif (start_pc, tuple(regs[:64])) != prev_end:
            raise ValueError("shard %d: does not start where shard %d ended" % (k, k - 1))
        prev_end = (end_pc, tuple(regs[64:]))
    return True


def rv32_publics(shards):
    """[(cpu public values, register public values)] canonical, per shard of [(tables, init)]"""
    return [(p3.from_mont(sh[0][0].public_values), p3.from_mont(sh[0][2].public_values)) for sh in shards]


def verify_rv32_execution(shards, proofs, params=None, entry_pc=None, prep_root=None, program_log_height=None, journals=None,
                          image=None, input_words=None, commit_logs=None, expected_journal=None):
    """Checks a run proven with the rv32i, rv32i-cf, rv32im, rv32im-elf or rv32im-mem chip set: every shard's proof
    (verify_rv32_shard), then check_rv32_chain over the public values.  shards: [(tables, init)] as p3_rv32_shards /
    p3_rv32cf_shards / p3_rv32im_shards / execute_rv32_device give them.  prep_root, program_log_height: the verifying
    key of an rv32im-elf or rv32im-mem run (Execution.prep_root / .program_log_height): every shard must answer to that
    one root.  Under rv32im-mem WITHOUT journals the shards' memories are not chained: every shard's INIT values are
    free.  journals (one per shard) with image (rv32link.memory_image(elf)): the run was proven with link=True; every
    proof is checked with its journal (verify_rv32_shard), and after check_rv32_chain the journals are replayed from the
    ELF's memory image (rv32link.check_memory_chain): INIT of every touched word is what the shards before left there.
    input_words (the run's input; the run was proven with io=True, raiko_amd/rv32io.py): every proof is checked against
    its slice of the input (verify_rv32_shard), and rv32io.check_io_chain binds the shards' stream positions to each other
    and to the input's length; the result is then (exit code -- None for a run that has not halted --, input words read)
    in place of True.  commit_logs (one commit log per shard, with input_words; the run was proven with commit=True,
    raiko_amd/rv32commit.py): every proof is checked with its log (verify_rv32_shard), rv32commit.check_commit_chain binds
    the shards' journal positions to each other, and the result is (exit code, input words read, the PROVEN journal: the
    bytes cut from the logs); expected_journal: a run whose proven journal differs from it is refused (ValueError).
    Raises ValueError naming the shard; returns True."""
    if len(proofs) != len(shards):
        raise ValueError("%d proofs for %d shards" % (len(proofs), len(shards)))
    if commit_logs is not None and (len(commit_logs) != len(shards) or input_words is None):
        raise ValueError("commit_logs: one per shard, with the run's input_words")
    if expected_journal is not None and commit_logs is None:
        raise ValueError("expected_journal goes with commit_logs: no other form proves the journal")
    if journals is not None and (len(journals) != len(shards) or image is None):
        raise ValueError("journals: one per shard, with the ELF's memory image")
    for k, ((tables, init, *_j), pf) in enumerate(zip(shards, proofs)):
        rc = verify_rv32_shard(tables, pf, init, params, prep_root, program_log_height,
                               journal=None if journals is None else journals[k], input_words=input_words,
                               commit_log=None if commit_logs is None else commit_logs[k])
        if rc != 0:
            raise ValueError("shard %d: the proof does not verify (reason %d)" % (k, rc))
    check_rv32_chain(rv32_publics(shards), entry_pc)
    if journals is not None:
        rv32link.check_memory_chain(journals, image)
    if commit_logs is not None:
        pubs = [rv32commit.publics_of(sh[0][rv32io.IO_TABLE].public_values) for sh in shards]
        rv32commit.check_commit_chain(pubs)
        proven = b"".join(rv32commit.log_bytes(pub, log) for pub, log in zip(pubs, commit_logs))
        if expected_journal is not None and proven != bytes(expected_journal):
            raise ValueError("the proven journal (%d bytes) is not the expected one (%d bytes)" % (len(proven), len(expected_journal)))
        return rv32io.check_io_chain(pubs, input_words) + (proven,)
    if input_words is not None:
        return rv32io.check_io_chain([rv32io.publics_of(sh[0][rv32io.IO_TABLE].public_values) for sh in shards], input_words)
    return True


def verify_rv32_shard(tables, proof, init, params=None, prep_root=None, program_log_height=None, journal=None, input_words=None,
                      commit_log=None) -> int:
    """rk_p3_verify of one rv32i (five tables), rv32i-cf (six) or rv32im (seven) shard with the register / byte / range
    / shift tables pinned to 32 / 2^18 / 2^16 / 2^12 rows and the cpu table to the height the statement gives; the
    muldiv table's height is the proof's, refused (reason 2) unless 0 < log height <= the cpu table's -> 0 or the
    verifier's reason.  prep_root (8 Montgomery words) with program_log_height: the statement is the rv32im-elf set's
    seven tables (or the rv32im-mem set's nine) under that verifying key (rk_p3_verify_key) -- the program table's
    height is then pinned by the verifier, no longer the proof's.  The memop and memory tables' heights are the proof's,
    refused (reason 2) unless 0 < log height <= the cpu table's + 1.  journal: the shard was proven with link=True
    (rv32link's AIRs): the digest of the journal at the proof's memory-table height is recomputed and must be that
    table's public values (reason 2 otherwise, also for a journal that is malformed or taller than the table); the proof
    is then verified with the journal's tuples as receive claims (rk_p3_verify_claims).  input_words: the shard was
    proven with io=True (rv32io's ten AIRs, under the io key): the io table's public values must fit the input (N_INPUT
    its length, POS_START <= POS_END <= N_INPUT), the digest of input_words[POS_START:POS_END] at the proof's io-table
    height is recomputed and must be the table's (reason 2 otherwise), and the slice's stream tuples are added as receive
    claims on BUS_INPUT, next to the journal's when there is one.  commit_log (with input_words): the shard was proven with
    commit=True (rv32commit's AIRs; the io table carries 24 public values): the log must be well formed against JPOS_START
    and JPOS_END (rv32commit.log_bytes), its digest at the proof's io-table height is recomputed and must be the table's
    (reason 2 otherwise, before the proof is read), and its tuples are added as receive claims on BUS_COMMIT"""
    vt = rv32_verifier_tables(tables, proof, prep_root, program_log_height)
    if vt is None:
        return 2
    claims = []
    if commit_log is not None and input_words is None:
        raise ValueError("a commit log goes with input_words: commit=True needs io=True")
    if input_words is not None:
        io = vt[rv32io.IO_TABLE] if len(vt) > rv32io.IO_TABLE else None
        n_pub = rv32io.N_PUBLIC_IO if commit_log is None else rv32commit.N_PUBLIC_IO
        if io is None or io.public_values.size != n_pub:
            raise ValueError("input_words go with the ten tables of an rv32im-mem shard proven with io=True: 14 public values "
                             "on the io table, or 24 and a commit log for commit=True")
        pub = rv32io.publics_of(io.public_values) if commit_log is None else rv32commit.publics_of(io.public_values)
        words = rv32io.slice_of(pub, input_words)
        if words is None:
            return 2
        try:
            digest = rv32io.stream_root(pub["pos_start"], words, io.log_height, params)
        except _lib.RkError:
            return 2
        if not np.array_equal(digest, pub["digest"]):
            return 2
        claims += rv32io.claims_of(pub["pos_start"], words)
        if commit_log is not None:
            if rv32commit.log_bytes(pub, commit_log) is None:
                return 2
            try:
                digest = rv32commit.log_root(commit_log, io.log_height, params)
            except _lib.RkError:
                return 2
            if not np.array_equal(digest, pub["commit_digest"]):
                return 2
            claims += rv32commit.claims_of(commit_log)
    elif len(vt) > rv32io.IO_TABLE:
        raise ValueError("the ten tables of an io shard are verified with input_words")
    if journal is not None:
        bd = vt[rv32link.MEMORY_TABLE] if len(vt) > rv32link.MEMORY_TABLE else None
        if bd is None or bd.public_values.size != rv32link.N_DIGEST:
            raise ValueError("a journal goes with the nine tables of a linked rv32im-mem shard")
        try:
            digest = rv32link.journal_root(journal, bd.log_height, params)
        except _lib.RkError:
            return 2
        if not np.array_equal(digest, bd.public_values):
            return 2
        claims += rv32link.claims_of(journal)
    if journal is None and input_words is None:
        return p3.verify(vt, proof, init, params, prep_root=prep_root)
    return p3.verify(vt, proof, init, params, prep_root=prep_root, claims=claims)


def rv32_verifier_tables(tables, proof, prep_root=None, program_log_height=None):
    """the tables verify_rv32_shard hands the verifier -- no traces, the heights pinned as described there; None where the
    proof's muldiv height is out of range (reason 2).  Also what the FRI statements about a shard proof take
    (raiko_amd.fri_transcript.statement(..., prep_root=...))"""
    cs = _BY_COUNT.get((prep_root is not None, len(tables)))
    if cs is None:
        raise ValueError("%d tables are no rv32 chip set's shard" % len(tables))
    if cs.keyed and not program_log_height:
        raise ValueError("a verifying key is the root and the program table's log height")
    cpu_log = tables[0].log_height
    logs = [cpu_log, int(program_log_height) if cs.keyed else 0, *cs.fixed]     # a program table at 0: the proof's height
    for most in [cpu_log] * cs.muldiv + [cpu_log + cs.mem_slack] * cs.n_mem:    # the heights the proof carries
        lg = int(proof[1 + len(logs)]) if len(proof) > 1 + len(logs) else 0
        if not 0 < lg <= most:
            return None
        logs.append(lg)
    return [p3.Table.pinned(t.air, lg, t.public_values) for t, lg in zip(tables, logs)]


def program_image_c(elf: bytes):
    """rk_exec_program_image -> (segment vaddrs, segment word counts, the image's words): uint32 arrays"""
    lib = _lib.load()
    n_segs, n_words = C.c_size_t(0), C.c_size_t(0)
    st = lib.rk_exec_program_image(bytes(elf), len(elf), None, None, 0, C.byref(n_segs), None, 0, C.byref(n_words))
    if st != _lib.RK_ERR_CAPACITY or n_segs.value > 16:
        _lib.check(None, st)
    vaddr, count = np.zeros(max(n_segs.value, 1), dtype=np.uint32), np.zeros(max(n_segs.value, 1), dtype=np.uint32)
    words = np.zeros(max(n_words.value, 1), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_program_image(bytes(elf), len(elf), vaddr.ctypes.data_as(_lib.u32p), count.ctypes.data_as(_lib.u32p),
                                               vaddr.size, C.byref(n_segs), words.ctypes.data_as(_lib.u32p), words.size, C.byref(n_words)))
    return vaddr[: n_segs.value], count[: n_segs.value], words[: n_words.value]


class Rv32Key:
    """setup_rv32_elf's result, the proving key of one ELF under the rv32im-elf chip set: .image [(vaddr, words)], .key
    the p3.Key over the program image and the byte / range / shift tuples, .root its 8 Montgomery words and
    .program_log_height (together the verifying key), .d_words the image's words in device memory (what
    rk_exec_rv32elf_shard_device compares the executed words with), .airs the seven AIRs.  close() frees the device
    memory."""

    def __init__(self, image, seg_vaddr, seg_words, key, d_words, program_log_height, airs, chips="rv32im-elf", io=False):
        self.image, self.seg_vaddr, self.seg_words, self.key, self.d_words = image, seg_vaddr, seg_words, key, d_words
        self.root, self.program_log_height, self.airs, self.chips, self.io = key.root, program_log_height, airs, chips, io
        self._preps = None

    @property
    def bytes(self):
        return self.key.bytes + 4 * self.d_words.size()

    def host_preps(self):
        """the preprocessed matrices as the chip set's prep_tables gives them (Montgomery words), in table order"""
        if self._preps is None:
            self._preps = _host_preps(_IO if self.io else _rv32_set(self.chips)[1], self.image, len(self.airs))
        return self._preps

    def close(self):
        if self.key is not None:
            self.key.close()
            self.d_words.free()
        self.key = self.d_words = None


def setup_rv32_elf(hal, elf: bytes, params=None, ext_w=None, airs=None, chips="rv32im-elf", link=False, io=False, commit=False) -> Rv32Key:
    """The setup of `client.setup(ELF)` for the rv32im-elf chip set: the ELF's program image (rk_exec_program_image), the
    four preprocessed matrices written on hal's GPU (rk_rv32elf_prep_device) and committed (rk_p3_setup) -> Rv32Key.
    params: the parameter set to put hal's context under first (None: the context's current one); ext_w: the AIRs'
    extension (default params' / the context's).  chips="rv32im-mem": that chip set's key (rk_rv32mem_prep_device: the
    program matrix has 48 columns) and nine AIRs.  link (rv32im-mem): the nine AIRs are rv32link's; the key itself --
    the preprocessed matrices, their heights, the root -- is the same either way.  io (rv32im-mem): the key of the io
    form (rk_rv32io_prep_device: the ecall word's tuple reads a0 and a1; another root than rv32im-mem's) and rv32io's ten
    AIRs.  commit (with io): the io form's key -- the decode does not differ -- and rv32commit's ten AIRs."""
    if chips not in KEYED_CHIPS:
        raise ValueError("chips must be one of %s" % (KEYED_CHIPS,))
    _link_ok(chips, link, io, commit)
    cs = _IO if io else _rv32_set(chips)[1]
    lib = _lib.load()
    if params is not None:
        _lib.check(hal._ctx, lib.rk_set_params(hal._ctx, C.byref(params)))
    if airs is None:
        airs = _rv32_airs_of(chips, int(hal.get_params().ext_w) if ext_w is None else ext_w, link, io, commit)
    vaddr, count, words = program_image_c(elf)
    rows = 2
    while rows < words.size:
        rows <<= 1
    # the tables with preprocessed columns, the program table first: table index -> log height
    logs = {i: lg for i, lg in enumerate([None, rows.bit_length() - 1, *cs.fixed]) if airs[i].prep_width}
    bufs = {i: hal.alloc_elem(airs[i].prep_width << lg) for i, lg in logs.items()}
    d_words = None
    try:
        program, *fixed = [C.c_void_p(b.ptr) for b in bufs.values()]
        _lib.check(hal._ctx, getattr(lib, cs.prep)(
            hal._ctx, vaddr.ctypes.data_as(_lib.u32p), count.ctypes.data_as(_lib.u32p), vaddr.size, words.ctypes.data_as(_lib.u32p),
            words.size, program, rows, *fixed))
        tables = [p3.Table.pinned(a, logs.get(i, 1), np.zeros(a.n_public, dtype=np.uint32)) for i, a in enumerate(airs)]
        key = p3.setup(hal, tables, device_preps=[bufs[i].ptr if i in bufs else None for i in range(len(airs))])
        try:
            d_words = hal.copy_from_elem(words if words.size else np.zeros(1, dtype=np.uint32))
            hal.sync()
        except Exception:
            key.close()
            if d_words is not None:
                d_words.free()
            raise
    finally:
        for b in bufs.values():
            b.free()
    image = [(int(v), words[at - int(c):at].astype(np.int64)) for v, c, at in zip(vaddr, count, np.cumsum(count))]
    return Rv32Key(image, vaddr, count, key, d_words, logs[1], airs, chips, io)
