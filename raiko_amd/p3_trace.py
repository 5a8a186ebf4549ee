"""The stand-in trace circuit the way SP1 proves an execution: shards of a uni-stark proof system (rk_p3_*).  The AIRs over
rk_exec_witness's 16 data columns, the program and range tables their lookups go to, and `p3_shards`, which turns an
executor.Execution into [(tables, init words)].  The range table is also the rv32 chip sets' (raiko_amd/rv32.py)."""
import ctypes as C

import numpy as np

from . import _lib, p3

BUS_PROGRAM, BUS_RANGE16 = 1, 2
RANGE_LIMB_COLS = (0, 1, 2, 3, 8, 9, 10, 11, 12, 13)     # pc, next pc, rs1, rs2, rd value: lo / hi limbs


def p3_trace_air(lookups=False, ext_w=None):
    """The stand-in trace circuit as an AIR over rk_exec_witness's 16 data columns (raiko_amd/p3.py; the risc0-shaped form
    is circuit_program.trace_program): flags are bits, a `seq` row advances pc by 4 with the stated carry, the next row
    starts where this one went, padding is final and does nothing, the first / last pc are the public ones
    (public values: start lo / hi, end lo / hi).  Degree 2: one quotient chunk.  NOT a zkVM: the pc chain only.
    lookups: every active row also sends (PROGRAM: pc lo, pc hi, instruction lo, instruction hi) and one (RANGE16: limb)
    per 16-bit limb column -- the way SP1's cpu chip is tied to its program and range chips (p3_program_air,
    p3_range_air receive them): 11 interactions, degree 3."""
    b = p3.AirBuilder(16, 4, p3.EXT_W if ext_w is None else ext_w)
    if lookups:
        b.send(BUS_PROGRAM, [0, 1, 4, 5], mult=15, mult_is_const=False)
        for c in RANGE_LIMB_COLS:
            b.send(BUS_RANGE16, [c], mult=15, mult_is_const=False)
    pc_lo, pc_hi, nx_lo, nx_hi = (b.local(c) for c in range(4))
    seq, carry, wr, active = b.local(6), b.local(7), b.local(14), b.local(15)
    for v in (seq, carry, wr, active):
        b.assert_zero(v * (v - 1))
    b.assert_zero(seq * (nx_lo - pc_lo - 4 + carry * 65536))
    b.assert_zero(seq * (nx_hi - pc_hi - carry))
    t = b.when_transition()
    t.assert_eq(b.next(0), nx_lo)
    t.assert_eq(b.next(1), nx_hi)
    t.assert_zero((1 - active) * b.next(15))               # once padding, always padding
    b.assert_zero((1 - active) * seq)
    b.assert_zero((1 - active) * wr)
    f = b.when_first_row()
    f.assert_eq(pc_lo, b.public(0))
    f.assert_eq(pc_hi, b.public(1))
    last = b.when_last_row()
    last.assert_eq(nx_lo, b.public(2))
    last.assert_eq(nx_hi, b.public(3))
    return b.build()


def p3_program_air(ext_w=None):
    """(pc lo, pc hi, instruction lo, instruction hi, multiplicity): receives the cpu table's PROGRAM tuples -- SP1's
    ProgramChip, whose first four columns SP1 commits once per ELF (preprocessed); here they travel in the main trace"""
    b = p3.AirBuilder(5, 0, p3.EXT_W if ext_w is None else ext_w)
    b.receive(BUS_PROGRAM, [0, 1, 2, 3], mult=4, mult_is_const=False)
    return b.build()


def p3_range_air(ext_w=None):
    """(v, multiplicity), v counting up from 0 one per row: at 2^16 rows the table of all 16-bit values; receives the
    RANGE16 tuples (a verifier pins its log_height to 16 -- the proof carries the heights)"""
    b = p3.AirBuilder(2, 0, p3.EXT_W if ext_w is None else ext_w)
    b.when_first_row().assert_zero(b.local(0))
    b.when_transition().assert_eq(b.next(0), b.local(0) + 1)
    b.receive(BUS_RANGE16, [0], mult=1, mult_is_const=False)
    return b.build()


def p3_shards(ex, air=None, lookups=False, ext_w=None):
    """one shard per executed segment: table = the segment's 16 witness columns as a row-major trace, public values = its
    first and last pc, transcript seed = the machine-state digests before and after it -> [(tables, init words)].
    lookups: three tables per shard -- cpu (p3_trace_air(lookups=True)), program (the distinct (pc, instruction) pairs the
    shard executed with how often), range (2^16 rows with how often each 16-bit value occurs among the cpu limbs)."""
    if ex.witness is None:
        raise ValueError("execute(..., record_trace=True) first")
    air = air or p3_trace_air(lookups, ext_w)
    prog_air, range_air = (p3_program_air(ext_w), p3_range_air(ext_w)) if lookups else (None, None)
    out = []
    for s, (_code, data) in zip(ex.segments, ex.witness):
        tables = [p3.Table(air, np.ascontiguousarray(data.T), s.pc_publics())]
        native = getattr(ex, "lookup_tables", None)
        if lookups and native is not None:       # the native generator's tables (rk_exec_lookup_tables)
            prog, rng = native[len(out)]
            tables += [p3.Table(prog_air, prog), p3.Table(range_air, rng)]
        elif lookups:                            # the same tables from the witness columns in numpy
            rows = p3.from_mont(data).astype(np.uint64)                                # canonical, column-major
            rows = rows[:, rows[15] == 1]                                              # the active rows
            key = (rows[1] << 16 | rows[0]) << 32 | (rows[5] << 16 | rows[4])          # pc, instruction
            uniq, cnt = np.unique(key, return_counts=True)
            n_prog = max(2, 1 << int(len(uniq) - 1).bit_length())
            prog = np.zeros((n_prog, 5), dtype=np.uint64)
            prog[: len(uniq), 0] = (uniq >> 32) & 0xFFFF
            prog[: len(uniq), 1] = uniq >> 48
            prog[: len(uniq), 2] = uniq & 0xFFFF
            prog[: len(uniq), 3] = (uniq >> 16) & 0xFFFF
            prog[: len(uniq), 4] = cnt
            limbs = rows[list(RANGE_LIMB_COLS)].reshape(-1)
            if limbs.size and int(limbs.max()) >= 1 << 16:
                raise ValueError("a limb outside 16 bits: the range argument cannot balance")
            rng = np.stack([np.arange(1 << 16, dtype=np.uint64), np.bincount(limbs.astype(np.int64), minlength=1 << 16).astype(np.uint64)], axis=1)
            tables += [p3.Table.from_canonical(prog_air, prog), p3.Table.from_canonical(range_air, rng)]
        out.append((tables, s.init_words()))
    return out


def next_trace_shard(stepper, hal, airs, lookups=True):
    """the next executed segment of an executor.Stepper as the tables of a uni-stark shard (airs: cpu, program, range):
    the 16 data columns written on the GPU as one row-major matrix (rk_exec_witness_device_rows) and -- lookups -- the
    program / range tables (rk_exec_lookup_tables, host) -> (ExecSegment, tables of which the cpu table has no host
    trace, [(device rows buffer, log_height), then None per host table], init words), or None after the last"""
    seg = stepper.step()
    if seg is None:
        return None
    cpu_air, prog_air, range_air = airs
    rows = hal.alloc_elem(cpu_air.width << seg.po2)
    _lib.check(hal._ctx, _lib.load().rk_exec_witness_device_rows(hal._ctx, stepper._h, seg.index, C.c_void_p(rows.ptr)))
    tables = [p3.Table.pinned(cpu_air, seg.po2, seg.pc_publics())]
    if lookups:
        prog, rng = stepper.lookup_tables(seg.index)
        tables += [p3.Table(prog_air, prog), p3.Table(range_air, rng)]
    hal.sync()       # the rows are complete before another context's stream reads them
    return seg, tables, [(rows, seg.po2)] + [None] * (len(tables) - 1), seg.init_words()
