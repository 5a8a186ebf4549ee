"""The executor + segmenter in front of the proving path: binding of rk_exec_* (raiko_amd/csrc/
executor.cpp the host executor, rv32_shards.hip the witness written on the GPU) and `execute_and_prove`, the shape of `prove_locally` (reference
provers/risc0/driver/src/bonsai.rs:230-272): run the guest ELF, cut the run into segments of at
most 2^po2 cycles, prove every segment, return the receipt.

What the library restates is the public part (RV32IM, ELF32, power-of-two segments); the cycle
model, the ecall table and the state digest are stand-ins and the rv32im circuit's witness layout
is not available (risc0-circuit-rv32im is outside the reference tree), so the segments handed to
the prover carry SYNTHETIC trace columns of the executed segment's size -- seeded by the
segment's state digests, so a different run gives different seals.  See include/raiko_hip.h."""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .segment import P, Segment, synthetic_segment


RkExecOpts, RkExecSummary, RkExecSegment = _lib.RkExecOpts, _lib.RkExecSummary, _lib.RkExecSegment


@dataclass
class ExecSegment:
    index: int
    po2: int
    cycles: int
    start_pc: int
    end_pc: int
    exit: int
    pre_state: Tuple[int, ...]
    post_state: Tuple[int, ...]


@dataclass
class Execution:
    """`risc0_zkvm::Session` as far as this backend has it: segment list, journal, exit code"""
    segments: List[ExecSegment]
    journal: bytes
    exit_code: int
    total_cycles: int
    input_words_read: int
    # with record_trace: per segment (code (2, 2^po2), data (16, 2^po2)) witness columns of the stand-in trace circuit
    witness: Optional[list] = None
    # with profile: [(pc, cycles)], most expensive first (rk_exec_profile)
    profile: Optional[list] = None
    # with record_trace: per segment (program table (rows, 5), range table (65536, 2)), row-major Montgomery words
    # (rk_exec_lookup_tables): what p3_shards(lookups=True) puts beside the cpu table
    lookup_tables: Optional[list] = None
    # with record_trace: per segment (registers at its start (32,), at its end (32,), ecall rows (k, 2): cycle, a0 after)
    # (rk_exec_registers / rk_exec_ecalls): the side data of the rv32i chip set (p3_rv32_shards)
    rv32: Optional[list] = None
    # chips="rv32im-elf": the verifying key of the run -- the root of the preprocessed commitment of the ELF (8 Montgomery
    # words) and the program table's log height, what verify_rv32_execution(prep_root=, program_log_height=) takes
    prep_root: Optional[np.ndarray] = None
    program_log_height: Optional[int] = None
    # with record_trace: per segment the access list (k, 4): cycle, word address, word before, word after
    # (rk_exec_mem_accesses): the side data of the rv32im-mem chip set (p3_rv32mem_shards)
    mem: Optional[list] = None


class ExecutorError(RuntimeError):
    pass


TRACE_CODE_COLS, TRACE_DATA_COLS, TRACE_ACCUM_COLS = 2, 16, 4


def execute(elf: bytes, input_words: Sequence[int] = (), segment_limit_po2: int = 20, session_limit: int = 0,
            record_trace: bool = False, profile: bool = False) -> Execution:
    """`ExecutorImpl::from_elf(env, elf).run()` (bonsai.rs:246-269).  Raises ExecutorError on a trap
    (illegal instruction, misaligned access, unknown ecall, session limit).  profile: what the reference's
    `profile: true` switches on (`env_builder.enable_profiler(..)`, bonsai.rs:252-255) -- here the cycles spent at
    every program counter, most expensive first, in Execution.profile."""
    lib = _lib.load()
    words = np.ascontiguousarray(input_words, dtype=np.uint32)
    opts = RkExecOpts(struct_size=C.sizeof(RkExecOpts), segment_limit_po2=segment_limit_po2, session_limit=session_limit,
                      input_words=words.ctypes.data_as(_lib.u32p), n_input_words=words.size,
                      record_trace=1 if record_trace else 0, profile=1 if profile else 0)
    handle = C.c_void_p()
    st = lib.rk_exec_elf(bytes(elf), len(elf), C.byref(opts), C.byref(handle))
    try:
        if st != 0:
            detail = lib.rk_exec_error(handle).decode() if handle else ""
            raise ExecutorError("%s%s" % (lib.rk_strerror(st).decode(), ": " + detail if detail else ""))
        summ = RkExecSummary()
        lib.rk_exec_summary_get(handle, C.byref(summ))
        segs = []
        for i in range(summ.n_segments):
            s = RkExecSegment()
            lib.rk_exec_segment_get(handle, i, C.byref(s))
            segs.append(ExecSegment(s.index, s.po2, int(s.cycles), s.start_pc, s.end_pc, s.exit,
                                    tuple(s.pre_state), tuple(s.post_state)))
        buf = C.create_string_buffer(max(int(summ.journal_bytes), 1))
        n = C.c_size_t(0)
        lib.rk_exec_journal(handle, buf, summ.journal_bytes, C.byref(n))
        witness = None
        if record_trace:   # rk_exec_witness: the native witness generator of the stand-in trace circuit
            witness = []
            for sg in segs:
                rows = 1 << sg.po2
                code = np.zeros((TRACE_CODE_COLS, rows), dtype=np.uint32)
                data = np.zeros((TRACE_DATA_COLS, rows), dtype=np.uint32)
                _lib.check(None, lib.rk_exec_witness(handle, sg.index, code.ctypes.data_as(_lib.u32p), data.ctypes.data_as(_lib.u32p)))
                witness.append((code, data))
        ex = Execution(segs, buf.raw[: n.value], summ.exit_code, int(summ.total_cycles), int(summ.input_words_read), witness)
        if record_trace:   # rk_exec_lookup_tables: the program / range tables of the uni-stark form with lookups
            ex.lookup_tables = []
            for sg in segs:
                rng = np.zeros((1 << 16, 2), dtype=np.uint32)
                rows = C.c_size_t(0)
                st2 = lib.rk_exec_lookup_tables(handle, sg.index, rng.ctypes.data_as(_lib.u32p), None, C.byref(rows))
                if st2 != _lib.RK_ERR_CAPACITY:
                    _lib.check(None, st2 or _lib.RK_ERR_INTERNAL)
                prog = np.zeros((rows.value, 5), dtype=np.uint32)
                _lib.check(None, lib.rk_exec_lookup_tables(handle, sg.index, rng.ctypes.data_as(_lib.u32p), prog.ctypes.data_as(_lib.u32p), C.byref(rows)))
                ex.lookup_tables.append((prog, rng))
            ex.rv32 = [_rv32_side(lib, handle, sg.index) for sg in segs]
            ex.mem = [mem_accesses(lib, handle, sg.index) for sg in segs]
        if profile:
            cnt = C.c_size_t(0)
            lib.rk_exec_profile(handle, None, None, 0, C.byref(cnt))
            pcs = np.zeros(max(cnt.value, 1), dtype=np.uint32)
            cyc = np.zeros(max(cnt.value, 1), dtype=np.uint64)
            _lib.check(None, lib.rk_exec_profile(handle, pcs.ctypes.data_as(_lib.u32p), cyc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 pcs.size, C.byref(cnt)))
            ex.profile = [(int(p), int(c)) for p, c in zip(pcs[: cnt.value], cyc[: cnt.value])]
        return ex
    finally:
        if handle:
            lib.rk_exec_free(handle)


def segments_for_proving(ex: Execution, widths: Tuple[int, int, int] = (16, 16, 224)) -> List[Segment]:
    """One prover segment per executed segment, of the executed size (2^po2 rows); the trace columns
    are the synthetic stand-in (no rv32im witness layout here), seeded by the segment's digests and
    carrying them as globals, so the seal binds the state transition the executor saw."""
    out = []
    for s in ex.segments:
        seed = int.from_bytes(np.array(s.pre_state + s.post_state, dtype="<u4").tobytes()[:8], "little")
        seg = synthetic_segment(s.po2, widths, seed=seed % (1 << 62), n_globals=0)
        seg.globals_ = np.array(list(s.pre_state) + list(s.post_state) + [s.start_pc % 2013265921, s.exit], dtype=np.uint32)
        out.append(seg)
    return out


class Stepper:
    """rk_exec_open / rk_exec_next_segment: the executor one segment at a time (risc0's `run_with_callback`
    shape), with the trace circuit's witness of every segment as it completes"""

    def __init__(self, elf: bytes, input_words: Sequence[int] = (), segment_limit_po2: int = 20):
        self._lib = _lib.load()
        words = np.ascontiguousarray(input_words, dtype=np.uint32)
        opts = RkExecOpts(struct_size=C.sizeof(RkExecOpts), segment_limit_po2=segment_limit_po2, session_limit=0,
                          input_words=words.ctypes.data_as(_lib.u32p), n_input_words=words.size, record_trace=1)
        self._h = C.c_void_p()
        st = self._lib.rk_exec_open(bytes(elf), len(elf), C.byref(opts), C.byref(self._h))
        if st != 0:
            detail = self._lib.rk_exec_error(self._h).decode() if self._h else ""
            self.close()
            raise ExecutorError("%s%s" % (self._lib.rk_strerror(st).decode(), ": " + detail if detail else ""))
        self.more = True
        self.n = 0

    def next(self, hal=None):
        """-> (ExecSegment, code, data) of the next executed segment, or None after the last.  With `hal` (a HipHal)
        the witness columns are written on the GPU (rk_exec_witness_device) and code / data are device buffers."""
        if not self.more:
            return None
        more = C.c_int(0)
        st = self._lib.rk_exec_next_segment(self._h, C.byref(more))
        if st != 0:
            raise ExecutorError("%s: %s" % (self._lib.rk_strerror(st).decode(), self._lib.rk_exec_error(self._h).decode()))
        self.more = bool(more.value)
        s = RkExecSegment()
        self._lib.rk_exec_segment_get(self._h, self.n, C.byref(s))
        seg = ExecSegment(s.index, s.po2, int(s.cycles), s.start_pc, s.end_pc, s.exit, tuple(s.pre_state), tuple(s.post_state))
        rows = 1 << seg.po2
        if hal is not None:
            code = hal.alloc_elem(TRACE_CODE_COLS * rows)
            data = hal.alloc_elem(TRACE_DATA_COLS * rows)
            _lib.check(None, self._lib.rk_exec_witness_device(hal._ctx, self._h, self.n, C.c_void_p(code.ptr), C.c_void_p(data.ptr)))
            hal.sync()   # the session's contexts run on other streams
        else:
            code = np.zeros((TRACE_CODE_COLS, rows), dtype=np.uint32)
            data = np.zeros((TRACE_DATA_COLS, rows), dtype=np.uint32)
            _lib.check(None, self._lib.rk_exec_witness(self._h, self.n, code.ctypes.data_as(_lib.u32p), data.ctypes.data_as(_lib.u32p)))
        self.n += 1
        return seg, code, data

    def next_shard(self, hal, lookups=True):
        """the next executed segment as the tables of a uni-stark shard: the 16 data columns written on the GPU as one
        row-major matrix (rk_exec_witness_device_rows) and -- lookups -- the program / range tables (rk_exec_lookup_tables,
        host) -> (ExecSegment, device rows buffer, program table or None, range table or None), or None after the last"""
        if not self.more:
            return None
        more = C.c_int(0)
        st = self._lib.rk_exec_next_segment(self._h, C.byref(more))
        if st != 0:
            raise ExecutorError("%s: %s" % (self._lib.rk_strerror(st).decode(), self._lib.rk_exec_error(self._h).decode()))
        self.more = bool(more.value)
        s = RkExecSegment()
        self._lib.rk_exec_segment_get(self._h, self.n, C.byref(s))
        seg = ExecSegment(s.index, s.po2, int(s.cycles), s.start_pc, s.end_pc, s.exit, tuple(s.pre_state), tuple(s.post_state))
        rows = hal.alloc_elem(TRACE_DATA_COLS << seg.po2)
        _lib.check(hal._ctx, self._lib.rk_exec_witness_device_rows(hal._ctx, self._h, self.n, C.c_void_p(rows.ptr)))
        prog = rng = None
        if lookups:
            rng = np.zeros((1 << 16, 2), dtype=np.uint32)
            n_rows = C.c_size_t(0)
            st2 = self._lib.rk_exec_lookup_tables(self._h, self.n, rng.ctypes.data_as(_lib.u32p), None, C.byref(n_rows))
            if st2 != _lib.RK_ERR_CAPACITY:
                _lib.check(None, st2 or _lib.RK_ERR_INTERNAL)
            prog = np.zeros((n_rows.value, 5), dtype=np.uint32)
            _lib.check(None, self._lib.rk_exec_lookup_tables(self._h, self.n, rng.ctypes.data_as(_lib.u32p), prog.ctypes.data_as(_lib.u32p), C.byref(n_rows)))
        hal.sync()       # the rows are complete before another context's stream reads them
        self.n += 1
        return seg, rows, prog, rng

    def next_rv32_shard(self, hal, airs, chips="rv32i", key=None):
        """the next executed segment as the tables of an rv32i (five), rv32i-cf (six), rv32im or rv32im-elf (seven) or
        rv32im-mem (nine) shard written on hal's GPU (rv32_shard_device; key: the Rv32Key of chips="rv32im-elf" /
        "rv32im-mem") -> (ExecSegment, tables without host traces, [(device buffer, log_height)] per table, init words),
        or None after the last"""
        if not self.more:
            return None
        more = C.c_int(0)
        st = self._lib.rk_exec_next_segment(self._h, C.byref(more))
        if st != 0:
            raise ExecutorError("%s: %s" % (self._lib.rk_strerror(st).decode(), self._lib.rk_exec_error(self._h).decode()))
        self.more = bool(more.value)
        s = RkExecSegment()
        self._lib.rk_exec_segment_get(self._h, self.n, C.byref(s))
        seg = ExecSegment(s.index, s.po2, int(s.cycles), s.start_pc, s.end_pc, s.exit, tuple(s.pre_state), tuple(s.post_state))
        tables, bufs, init = rv32_shard_device(hal, self._h, self.n, seg, airs, chips, key)
        self.n += 1
        return seg, tables, bufs, init

    def finish(self) -> Execution:
        summ = RkExecSummary()
        self._lib.rk_exec_summary_get(self._h, C.byref(summ))
        buf = C.create_string_buffer(max(int(summ.journal_bytes), 1))
        n = C.c_size_t(0)
        self._lib.rk_exec_journal(self._h, buf, summ.journal_bytes, C.byref(n))
        ex = Execution([], buf.raw[: n.value], summ.exit_code, int(summ.total_cycles), int(summ.input_words_read))
        self.close()
        return ex

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rk_exec_free(self._h)
            self._h = None


def trace_segments(ex: Execution, program=None) -> List[Segment]:
    """One prover segment per executed segment with its EXECUTION TRACE as witness (rk_exec_witness) and the
    stand-in trace circuit's constraint list (circuit_program.trace_program) behind eval_check: the seal then says
    that the pc chain of the committed trace is consistent and starts / ends at the public pcs.  Not rv32im."""
    from .circuit_program import Program, trace_program
    from .segment import make_tapset
    if ex.witness is None:
        raise ValueError("execute(..., record_trace=True) first")
    taps = make_tapset([[(0,)] * TRACE_ACCUM_COLS, [(0,)] * TRACE_CODE_COLS,
                        [((0, 1) if c in (2, 3, 15) else (0,)) for c in range(TRACE_DATA_COLS)]])
    if program is None:
        program = Program(*trace_program(taps), taps)
    out = []
    for s, (code, data) in zip(ex.segments, ex.witness):
        accum = np.ascontiguousarray(data[:TRACE_ACCUM_COLS])      # unconstrained in this circuit; no accumulate hook
        out.append(_trace_segment(s, taps, program, [accum, code, data]))
    return out


def _trace_segment(s: ExecSegment, taps, program, groups) -> Segment:
    mont = lambda v: (int(v) << 32) % P
    pcs = [s.start_pc & 0xFFFF, s.start_pc >> 16, s.end_pc & 0xFFFF, s.end_pc >> 16]
    globals_ = np.array([mont(v) for v in pcs] + list(s.pre_state) + list(s.post_state), dtype=np.uint32)
    seg = Segment(po2=s.po2, taps=taps, groups=groups, check=None, globals_=globals_, n_accum_mix=4,
                  circuit_info=b"RV32_TRACE:v1___")
    seg.program = program
    return seg


def execute_and_prove(elf: bytes, input_words: Sequence[int] = (), segment_limit_po2: int = 20,
                      widths: Tuple[int, int, int] = (16, 16, 224), device: int = 0, inflight: int = 3,
                      circuit: str = "synthetic", pipeline: bool = False, device_witness: bool = True):
    """`prove_locally` end to end (bonsai.rs:230-272): execute, segment, prove every segment through
    rk_prove_session, assemble the receipt around the journal the guest committed.
    circuit = "synthetic": stand-in columns of the executed size (the shape of the S20 workload);
    circuit = "trace": the execution trace as witness under the stand-in trace circuit, every seal's
    constraint identity verified inside the session; with `pipeline` the executor steps segment by segment and
    each segment is proven while the next one executes, its witness columns generated on the GPU unless
    device_witness is False.  Returns (Execution, Receipt)."""
    from .hal import prove_session
    from .receipt import Receipt, SegmentReceipt
    if circuit == "trace" and pipeline:
        # segment k is proven (rk_stream_*) while the executor runs segment k + 1; the witness columns are written
        # on the GPU from the executed cycles (rk_exec_witness_device), so the host only runs the machine
        from .circuit_program import Program, trace_program
        from .hal import HipHal, SessionStream
        from .segment import make_tapset
        taps = make_tapset([[(0,)] * TRACE_ACCUM_COLS, [(0,)] * TRACE_CODE_COLS,
                            [((0, 1) if c in (2, 3, 15) else (0,)) for c in range(TRACE_DATA_COLS)]])
        program = Program(*trace_program(taps), taps)
        wit_hal = HipHal(device) if device_witness else None
        stepper = Stepper(elf, input_words, segment_limit_po2)
        stream, segs, metas = None, [], []
        try:
            while True:
                item = stepper.next(wit_hal)
                if item is None:
                    break
                meta, code, data = item
                if stream is None:
                    stream = SessionStream(device=device, inflight=inflight, program=program)
                if device_witness:
                    seg = _trace_segment(meta, taps, program, [None, None, None])
                    stream.submit(seg, device_inputs=([data, code, data], None))   # accum = the first columns of data
                else:
                    seg = _trace_segment(meta, taps, program, [np.ascontiguousarray(data[:TRACE_ACCUM_COLS]), code, data])
                    stream.submit(seg)
                segs.append(seg)
                metas.append(meta)
            ex = stepper.finish()
            ex.segments = metas
            seals = stream.close() if stream is not None else []
        finally:
            stepper.close()
    elif circuit == "trace":
        ex = execute(elf, input_words, segment_limit_po2=segment_limit_po2, record_trace=True)
        segs = trace_segments(ex)
        seals = prove_session(segs, device=device, inflight=inflight, program=segs[0].program if segs else None)
    else:
        ex = execute(elf, input_words, segment_limit_po2=segment_limit_po2)
        segs = segments_for_proving(ex, widths)
        seals = prove_session(segs, device=device, inflight=inflight)
    n = len(seals)
    receipts = [SegmentReceipt(seal=s, index=i, po2=segs[i].po2,
                               exit_code=("Halted", ex.exit_code) if i + 1 == n else ("SystemSplit", None))
                for i, s in enumerate(seals)]
    return ex, Receipt(segments=receipts, journal=ex.journal)


# ---- the same execution proven the way SP1 proves one: shards of a uni-stark proof system (rk_p3_*) ----------------
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
    from . import p3
    b = p3.AirBuilder(TRACE_DATA_COLS, 4, p3.EXT_W if ext_w is None else ext_w)
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
    from . import p3
    b = p3.AirBuilder(5, 0, p3.EXT_W if ext_w is None else ext_w)
    b.receive(BUS_PROGRAM, [0, 1, 2, 3], mult=4, mult_is_const=False)
    return b.build()


def p3_range_air(ext_w=None):
    """(v, multiplicity), v counting up from 0 one per row: at 2^16 rows the table of all 16-bit values; receives the
    RANGE16 tuples (a verifier pins its log_height to 16 -- the proof carries the heights)"""
    from . import p3
    b = p3.AirBuilder(2, 0, p3.EXT_W if ext_w is None else ext_w)
    b.when_first_row().assert_zero(b.local(0))
    b.when_transition().assert_eq(b.next(0), b.local(0) + 1)
    b.receive(BUS_RANGE16, [0], mult=1, mult_is_const=False)
    return b.build()


def p3_shards(ex: Execution, air=None, lookups=False, ext_w=None):
    """one shard per executed segment: table = the segment's 16 witness columns as a row-major trace, public values = its
    first and last pc, transcript seed = the machine-state digests before and after it -> [(tables, init words)].
    lookups: three tables per shard -- cpu (p3_trace_air(lookups=True)), program (the distinct (pc, instruction) pairs the
    shard executed with how often), range (2^16 rows with how often each 16-bit value occurs among the cpu limbs)."""
    from . import p3
    if ex.witness is None:
        raise ValueError("execute(..., record_trace=True) first")
    air = air or p3_trace_air(lookups, ext_w)
    prog_air, range_air = (p3_program_air(ext_w), p3_range_air(ext_w)) if lookups else (None, None)
    mont = lambda v: (int(v) << 32) % P
    out = []
    for s, (_code, data) in zip(ex.segments, ex.witness):
        pub = np.array([mont(v) for v in (s.start_pc & 0xFFFF, s.start_pc >> 16, s.end_pc & 0xFFFF, s.end_pc >> 16)], dtype=np.uint32)
        tables = [p3.Table(air, np.ascontiguousarray(data.T), pub)]
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
        out.append((tables, np.array(list(s.pre_state) + list(s.post_state), dtype=np.uint32)))
    return out


class P3Pipeline:
    """ELF -> verified shard proofs with the three stages overlapped: the calling thread runs the executor one shard at a
    time (rk_exec_next_segment), has the shard's cpu table written on the GPU from the executed cycles
    (rk_exec_witness_device_rows: the trace never exists on the host) and builds its lookup tables; a second thread proves
    the shards as they arrive (rk_p3_prove on its own context, the cpu table an on_device input); a small pool verifies
    the proofs (rk_p3_verify is host code).  The contexts and the (compiled) AIRs live as long as the object: run() any
    number of programs, then close().  chips="rv32i" / "rv32i-cf" / "rv32im": every shard's tables of that chip set are written on
    the GPU (Stepper.next_rv32_shard; `lookups` does not apply), every proof is checked by verify_rv32_shard and the run
    by check_rv32_chain.  chips="rv32im-elf" / "rv32im-mem": run() sets the program's key up first (setup_rv32_elf on the
    proving context), proves every shard under it, checks every proof against its root, and closes it when the run ends."""

    def __init__(self, params=None, device: int = 0, lookups=True, compile_airs=True, chips="trace"):
        from . import p3
        from .hal import HipHal, make_params
        if chips not in CHIPS:
            raise ValueError("chips must be one of %s" % (CHIPS,))
        self.params = params if params is not None else make_params(1)
        self.lookups, self.chips = lookups, chips
        ext_w = int(self.params.ext_w)
        self.rv32_airs = _rv32_airs_of(chips, ext_w) if chips in RV32_CHIPS else None
        self.cpu_air = p3_trace_air(lookups, ext_w)
        self.prog_air, self.range_air = (p3_program_air(ext_w), p3_range_air(ext_w)) if lookups else (None, None)
        self.wit_hal, self.prove_hal = HipHal(device), HipHal(device)
        _lib.check(self.prove_hal._ctx, self.prove_hal._lib.rk_set_params(self.prove_hal._ctx, C.byref(self.params)))
        if compile_airs:
            for a in self.rv32_airs or (self.cpu_air, self.prog_air, self.range_air):
                if a is not None:
                    a.compile(self.prove_hal)

    def close(self):
        for h in (self.wit_hal, self.prove_hal):
            if h is not None:
                h.close()
        self.wit_hal = self.prove_hal = None

    def run(self, elf: bytes, input_words: Sequence[int] = (), shard_po2: int = 20, verify=True, keep_tables=False):
        """-> (Execution, [proof words], [(tables, init)] when keep_tables)"""
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor
        from . import p3
        from .hal import _ptr
        mont = lambda v: (int(v) << 32) % P
        todo = queue.Queue(maxsize=3)           # back-pressure: at most three shards' tables wait for the prover
        done = queue.Queue()                    # cpu tables the prover is through with: freed by the thread that owns their context
        proofs, checks, kept, errors, stmts = [], [], [], [], []
        lookups, params, rv32i = self.lookups, self.params, self.chips in RV32_CHIPS
        key = setup_rv32_elf(self.prove_hal, elf, airs=self.rv32_airs, chips=self.chips) if self.chips in KEYED_CHIPS else None
        vk = dict(prep_root=key.root, program_log_height=key.program_log_height) if key else {}
        try:
            stepper = Stepper(elf, input_words, shard_po2)
        except Exception:
            if key:
                key.close()
            raise
        pool = ThreadPoolExecutor(max_workers=4)

        def prover():
            try:
                while True:
                    item = todo.get()
                    if item is None:
                        return
                    if rv32i:
                        seg, tables, bufs, init = item
                        pf = p3.prove(self.prove_hal, tables, init, device_traces=[(_ptr(b), lg) for b, lg in bufs],
                                      key=key.key if key else None)
                        proofs.append(pf)
                        stmts.append((tables, init))
                        if verify:
                            checks.append(pool.submit(verify_rv32_shard, tables, pf, init, params, **vk))
                        if keep_tables:
                            preps = key.host_preps() if key else [None] * len(tables)
                            kept.append(([p3.Table(t.air, b.to_host().reshape(1 << lg, t.air.width), t.public_values, prep=pm)
                                          for t, (b, lg), pm in zip(tables, bufs, preps)], init))
                        done.put(bufs)
                        continue
                    seg, rows, prog, rng = item
                    pub = np.array([mont(v) for v in (seg.start_pc & 0xFFFF, seg.start_pc >> 16, seg.end_pc & 0xFFFF, seg.end_pc >> 16)], dtype=np.uint32)
                    cpu = p3.Table(self.cpu_air, None, pub)
                    cpu.log_height = seg.po2
                    tables = [cpu] + ([p3.Table(self.prog_air, prog), p3.Table(self.range_air, rng)] if lookups else [])
                    init = np.array(list(seg.pre_state) + list(seg.post_state), dtype=np.uint32)
                    pf = p3.prove(self.prove_hal, tables, init, device_traces=[(_ptr(rows), seg.po2)] + [None] * (len(tables) - 1))
                    proofs.append(pf)
                    if verify:
                        checks.append(pool.submit(p3.verify, tables, pf, init, params))
                    if keep_tables:
                        host = p3.Table(self.cpu_air, rows.to_host().reshape(-1, TRACE_DATA_COLS), pub)
                        kept.append(([host] + tables[1:], init))
                    done.put(rows)
            except Exception as e:  # noqa: BLE001
                errors.append(e)
                while todo.get() is not None:      # drain: the producer must not block on a full queue
                    pass

        th = threading.Thread(target=prover)
        th.start()
        metas, bad = [], []
        try:
            while True:
                while not done.empty():
                    _free(done.get())
                item = (stepper.next_rv32_shard(self.wit_hal, self.rv32_airs, self.chips, key) if rv32i
                        else stepper.next_shard(self.wit_hal, lookups))
                if item is None or errors:
                    break
                metas.append(item[0])
                todo.put(item)
            ex = stepper.finish()
            ex.segments = metas
            if key:
                ex.prep_root, ex.program_log_height = key.root.copy(), key.program_log_height
        finally:
            todo.put(None)
            th.join()
            while not done.empty():
                _free(done.get())
            stepper.close()
            bad = [i for i, c in enumerate(checks) if c.result() != 0]
            pool.shutdown()
            if key:
                key.close()
        if errors:
            raise errors[0]
        if bad:
            raise _lib.RkError(_lib.RK_ERR_VERIFY, "shard %d does not verify" % bad[0])
        if rv32i and verify:
            check_rv32_chain(rv32_publics(stmts), entry_pc=metas[0].start_pc if metas else None)
        return ex, proofs, kept


def _free(bufs):
    """a device buffer, or the [(device buffer, log_height)] of an rv32i shard"""
    for b in bufs if isinstance(bufs, list) else [bufs]:
        (b[0] if isinstance(b, tuple) else b).free()


def execute_and_prove_p3_pipelined(elf: bytes, input_words: Sequence[int] = (), shard_po2: int = 20, params=None, device: int = 0,
                                   lookups=True, compile_airs=True, verify=True, keep_tables=False, chips="trace"):
    """one program through a P3Pipeline of its own"""
    pipe = P3Pipeline(params, device, lookups, compile_airs, chips)
    try:
        return pipe.run(elf, input_words, shard_po2, verify, keep_tables)
    finally:
        pipe.close()


def execute_and_prove_p3(elf: bytes, input_words: Sequence[int] = (), shard_po2: int = 16, params=None, device: int = 0, batch: int = 3,
                         lookups=False, chips="trace"):
    """ELF -> executed shards -> one uni-stark proof per shard through rk_p3_prove_shards (every proof verified inside):
    the shape of `client.prove(&pk, stdin)` on the SP1 side (provers/sp1/driver/src/lib.rs:44-57; SHARD_SIZE / SHARD_BATCH_SIZE,
    docs/README_Sp1.md:19-32) with the stand-in trace AIR in place of SP1's chips.  -> (Execution, shards, proofs)
    chips="rv32i": the rv32i chip set instead (raiko_amd/rv32.py; `lookups` does not apply): every shard's five tables
    written on the GPU (rk_exec_rv32_shard_device), every proof verified inside and the run checked by
    verify_rv32_execution.  chips="rv32i-cf": the same with the rv32i-cf chip set's six tables (raiko_amd/rv32cf.py,
    rk_exec_rv32cf_shard_device); chips="rv32im" with the rv32im chip set's seven (raiko_amd/rv32im.py,
    rk_exec_rv32im_shard_device).  chips="rv32im-elf": rv32im with the program bound to the ELF (raiko_amd/rv32elf.py):
    setup_rv32_elf commits the program image and the fixed tables once, every shard's seven traces are written on the
    GPU (rk_exec_rv32elf_shard_device) and proven under that key (rk_p3_prove_shards_key), and the run is checked against
    the key's root, which the returned Execution carries as ex.prep_root (with ex.program_log_height: together the
    verifying key).  chips="rv32im-mem": rv32im-elf with loads, stores and memory constrained within every shard
    (raiko_amd/rv32mem.py): nine traces per shard (rk_exec_rv32mem_shard_device), the same key protocol."""
    from . import p3
    from .hal import make_params
    params = params if params is not None else make_params(1)
    if chips not in CHIPS:
        raise ValueError("chips must be one of %s" % (CHIPS,))
    if chips in RV32_CHIPS:
        from .hal import HipHal
        hal = HipHal(device)
        key, vk = None, {}
        try:
            if chips in KEYED_CHIPS:
                key = setup_rv32_elf(hal, elf, params, chips=chips)
                vk = dict(prep_root=key.root.copy(), program_log_height=key.program_log_height)
            ex, shards, dev_traces, bufs = execute_rv32_device(hal, elf, input_words, shard_po2, ext_w=int(params.ext_w),
                                                               chips=chips, key=key)
            hal.sync()
            try:
                proofs = p3.prove_shards(shards, params, device=device, batch=batch, verify=True, device_traces=dev_traces,
                                         key=key.key if key else None)
            finally:
                for d in bufs:
                    for b, _lg in d:
                        b.free()
        finally:
            if key:
                key.close()
            hal.close()
        verify_rv32_execution(shards, proofs, params, entry_pc=ex.segments[0].start_pc if ex.segments else None, **vk)
        if vk:
            ex.prep_root, ex.program_log_height = vk["prep_root"], vk["program_log_height"]
        return ex, shards, proofs
    ex = execute(elf, input_words, segment_limit_po2=shard_po2, record_trace=True)
    shards = p3_shards(ex, lookups=lookups, ext_w=int(params.ext_w))
    proofs = p3.prove_shards(shards, params, device=device, batch=batch, verify=True)
    return ex, shards, proofs


# ---- the rv32i chip set (raiko_amd/rv32.py): the register file and the integer ALU constrained ------------------------
CHIPS = ("trace", "rv32i", "rv32i-cf", "rv32im", "rv32im-elf", "rv32im-mem")
RV32_CHIPS = ("rv32i", "rv32i-cf", "rv32im", "rv32im-elf", "rv32im-mem")
KEYED_CHIPS = ("rv32im-elf", "rv32im-mem")           # proven under the key of setup_rv32_elf
# the tables past the muldiv table whose height the proof carries: rv32im-mem's memop and memory, at most twice the cpu's
_RV32_MEM_TABLES = {"rv32im-mem": 2}


# per chip set: the module with its AIRs and numpy tables, the entry point that writes a shard's tables on the GPU, the
# fixed-height tables past rv32i's five as (module, name of its log height), whether a muldiv table (of the height the
# segment needs) comes last
_RV32_SETS = {"rv32i": ("rv32", "rk_exec_rv32_shard_device", (), False),
              "rv32i-cf": ("rv32cf", "rk_exec_rv32cf_shard_device", (("rv32cf", "SHIFT_LOG_ROWS"),), False),
              "rv32im": ("rv32im", "rk_exec_rv32im_shard_device", (("rv32cf", "SHIFT_LOG_ROWS"),), True),
              "rv32im-elf": ("rv32elf", "rk_exec_rv32elf_shard_device", (("rv32cf", "SHIFT_LOG_ROWS"),), True),
              "rv32im-mem": ("rv32mem", "rk_exec_rv32mem_shard_device", (("rv32cf", "SHIFT_LOG_ROWS"),), True)}


def _rv32_set(chips):
    """-> (the chip set's module, its C entry point, the pinned log heights of its tables from the register table on,
    whether a muldiv table follows them)"""
    from importlib import import_module
    if chips not in _RV32_SETS:
        raise ValueError("chips must be one of %s" % (RV32_CHIPS,))
    module, entry, fixed, muldiv = _RV32_SETS[chips]
    mod = lambda name: import_module("." + name, __package__)
    pinned = (5, mod("rv32").BYTE_LOG_ROWS, 16) + tuple(getattr(mod(m), name) for m, name in fixed)
    return mod(module), entry, pinned, muldiv


def _rv32_airs_of(chips, ext_w=None):
    """the AIRs of one shard of chip set `chips`, in table order"""
    return _rv32_set(chips)[0].airs(ext_w)


def _rv32_side(lib, handle, index):
    start, end = np.zeros(32, dtype=np.uint32), np.zeros(32, dtype=np.uint32)
    _lib.check(None, lib.rk_exec_registers(handle, index, start.ctypes.data_as(_lib.u32p), end.ctypes.data_as(_lib.u32p)))
    n = C.c_size_t(0)
    st = lib.rk_exec_ecalls(handle, index, None, 0, C.byref(n))
    if st != _lib.RK_ERR_CAPACITY:
        _lib.check(None, st)
    ec = np.zeros((max(n.value, 1), 2), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_ecalls(handle, index, ec.ctypes.data_as(_lib.u32p), ec.shape[0], C.byref(n)))
    return start, end, ec[: n.value]


def mem_accesses(lib, handle, index):
    """rk_exec_mem_accesses -> (k, 4) uint32: cycle, word address, word before, word after"""
    n = C.c_size_t(0)
    st = lib.rk_exec_mem_accesses(handle, index, None, 0, C.byref(n))
    if st != _lib.RK_ERR_CAPACITY:
        _lib.check(None, st)
    out = np.zeros((max(n.value, 1), 4), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_mem_accesses(handle, index, out.ctypes.data_as(_lib.u32p), out.shape[0], C.byref(n)))
    return out[: n.value]


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


def _rv32_publics(seg, start, end):
    from . import rv32
    from .p3 import to_mont
    pub_cpu = to_mont(np.array([seg.start_pc & 0xFFFF, seg.start_pc >> 16, seg.end_pc & 0xFFFF, seg.end_pc >> 16], dtype=np.uint64))
    return pub_cpu, to_mont(rv32.register_publics(start, end))


def _rv32_shards(chips, ex, ext_w, airs):
    """one shard of chip set `chips` per executed segment, every table built in numpy (the set's shard_tables) from
    ex.witness and ex.rv32 -> [(tables, init words)], init = the state digests as in p3_shards"""
    from . import p3
    if ex.witness is None or ex.rv32 is None:
        raise ValueError("execute(..., record_trace=True) first")
    module = _rv32_set(chips)[0]
    airs = airs or module.airs(ext_w)
    out = []
    for s, (_code, data), (start, end, ecalls) in zip(ex.segments, ex.witness, ex.rv32):
        canon, _pc, _regs = module.shard_tables(s, data, start, end, ecalls)
        pub_cpu, pub_reg = _rv32_publics(s, start, end)
        pubs = [pub_cpu, (), pub_reg] + [()] * (len(canon) - 3)
        tables = [p3.Table(a, p3.to_mont(t), pv) for a, t, pv in zip(airs, canon, pubs)]
        out.append((tables, np.array(list(s.pre_state) + list(s.post_state), dtype=np.uint32)))
    return out


def p3_rv32_shards(ex: Execution, ext_w=None, airs=None):
    """rv32i shards in numpy: tables = cpu, program, register, byte, range (p3_rv32_airs).  The yardstick for the tables
    rk_exec_rv32_shard_device writes on the GPU."""
    return _rv32_shards("rv32i", ex, ext_w, airs)


def p3_rv32cf_shards(ex: Execution, ext_w=None, airs=None):
    """rv32i-cf shards in numpy: tables = cpu, program, register, byte, range, shift (p3_rv32cf_airs).  The yardstick for
    the tables rk_exec_rv32cf_shard_device writes on the GPU."""
    return _rv32_shards("rv32i-cf", ex, ext_w, airs)


def p3_rv32im_shards(ex: Execution, ext_w=None, airs=None):
    """rv32im shards in numpy: tables = cpu, program, register, byte, range, shift, muldiv (p3_rv32im_airs).  The
    yardstick for the tables rk_exec_rv32im_shard_device writes on the GPU."""
    return _rv32_shards("rv32im", ex, ext_w, airs)


def rv32_shard_device(hal, handle, index, seg, airs, chips="rv32i", key=None):
    """rk_exec_rv32_shard_device (chips="rv32i") / rk_exec_rv32cf_shard_device ("rv32i-cf") /
    rk_exec_rv32im_shard_device ("rv32im") / rk_exec_rv32elf_shard_device ("rv32im-elf", key: the program's Rv32Key) /
    rk_exec_rv32mem_shard_device ("rv32im-mem", key likewise): segment `index` of an open executor as the tables of a
    shard of that chip set, written on hal's GPU -> (tables without host traces, [(device buffer, log_height)] per
    table, init words)"""
    from . import p3
    _module, entry, pinned, muldiv = _rv32_set(chips)
    lib = _lib.load()
    start, end, _ec = _rv32_side(lib, handle, index)
    rows = C.c_size_t(0)
    if chips in KEYED_CHIPS:
        if key is None or key.chips != chips:
            raise ValueError("chips=\"%s\" needs the Rv32Key of setup_rv32_elf(chips=\"%s\")" % (chips, chips))
        rows.value = 1 << key.program_log_height
    else:
        _lib.check(None, lib.rk_exec_rv32_sizes(handle, index, C.byref(rows)))
    logs = [seg.po2, rows.value.bit_length() - 1, *pinned]
    md_rows = C.c_size_t(0)
    if muldiv:
        _lib.check(None, lib.rk_exec_rv32im_sizes(handle, index, C.byref(md_rows)))
        logs.append(md_rows.value.bit_length() - 1)
    mem_rows = [C.c_size_t(0), C.c_size_t(0)]
    if chips in _RV32_MEM_TABLES:    # a segment with more accesses than twice its cycles is refused here (RK_ERR_CAPACITY)
        _lib.check(None, lib.rk_exec_rv32mem_sizes(handle, index, C.byref(mem_rows[0]), C.byref(mem_rows[1])))
        logs += [r.value.bit_length() - 1 for r in mem_rows]
    if len(airs) != len(logs):
        raise ValueError("%d AIRs for the %d tables of %s" % (len(airs), len(logs), chips))
    bufs = [hal.alloc_elem(a.width << lg) for a, lg in zip(airs, logs)]
    ptrs = [C.c_void_p(b.ptr) for b in bufs]
    n_fixed = len(logs) - _RV32_MEM_TABLES.get(chips, 0)
    args = ptrs[:2] + [rows.value] + ptrs[2:n_fixed] + ([md_rows.value] if muldiv else [])
    for b, r in zip(ptrs[n_fixed:], mem_rows):
        args += [b, r.value]
    if chips in KEYED_CHIPS:
        args = [key.seg_vaddr.ctypes.data_as(_lib.u32p), key.seg_words.ctypes.data_as(_lib.u32p), key.seg_vaddr.size,
                C.c_void_p(key.d_words.ptr)] + args
    try:
        _lib.check(hal._ctx, getattr(lib, entry)(hal._ctx, handle, index, *args))
    except Exception:
        for b in bufs:
            b.free()
        raise
    pub_cpu, pub_reg = _rv32_publics(seg, start, end)
    tables = []
    for a, lg, pv in zip(airs, logs, [pub_cpu, (), pub_reg] + [()] * (len(logs) - 3)):
        t = p3.Table(a, None, pv)
        t.log_height = lg
        tables.append(t)
    init = np.array(list(seg.pre_state) + list(seg.post_state), dtype=np.uint32)
    return tables, list(zip(bufs, logs)), init


def execute_rv32_device(hal, elf: bytes, input_words: Sequence[int] = (), shard_po2: int = 16, airs=None, ext_w=None,
                        chips="rv32i", key=None):
    """ELF -> rv32i (rv32i-cf, rv32im, rv32im-elf) shards whose tables are written on hal's GPU, one segment at a time
    (the executor's trace of a segment is dropped with the executor; the tables stay in HBM) -> (Execution, [(tables,
    init)], [device traces], [[(device buffer, log_height)]] to free).  key: the Rv32Key of chips="rv32im-elf" (its AIRs
    are the shards')"""
    from .hal import _ptr
    airs = airs or (key.airs if key is not None else _rv32_airs_of(chips, ext_w))
    st = Stepper(elf, input_words, shard_po2)
    shards, dev, metas = [], [], []
    try:
        while True:
            item = st.next_rv32_shard(hal, airs, chips, key)
            if item is None:
                break
            seg, tables, bufs, init = item
            shards.append((tables, init))
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
    return ex, shards, [[(_ptr(b), lg) for b, lg in d] for d in dev], dev


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
    from . import p3
    return [(p3.from_mont(t[0].public_values), p3.from_mont(t[2].public_values)) for t, _init in shards]


def verify_rv32_execution(shards, proofs, params=None, entry_pc=None, prep_root=None, program_log_height=None):
    """Checks a run proven with the rv32i, rv32i-cf, rv32im, rv32im-elf or rv32im-mem chip set: every shard's proof
    (verify_rv32_shard), then check_rv32_chain over the public values.  shards: [(tables, init)] as p3_rv32_shards /
    p3_rv32cf_shards / p3_rv32im_shards / execute_rv32_device give them.  prep_root, program_log_height: the verifying
    key of an rv32im-elf or rv32im-mem run (Execution.prep_root / .program_log_height): every shard must answer to that
    one root.  Under rv32im-mem the shards' memories are NOT chained: every shard's INIT values are free.
    Raises ValueError naming the shard; returns True."""
    if len(proofs) != len(shards):
        raise ValueError("%d proofs for %d shards" % (len(proofs), len(shards)))
    for k, ((tables, init), pf) in enumerate(zip(shards, proofs)):
        rc = verify_rv32_shard(tables, pf, init, params, prep_root, program_log_height)
        if rc != 0:
            raise ValueError("shard %d: the proof does not verify (reason %d)" % (k, rc))
    return check_rv32_chain(rv32_publics(shards), entry_pc)


def verify_rv32_shard(tables, proof, init, params=None, prep_root=None, program_log_height=None) -> int:
    """rk_p3_verify of one rv32i (five tables), rv32i-cf (six) or rv32im (seven) shard with the register / byte / range
    / shift tables pinned to 32 / 2^18 / 2^16 / 2^12 rows and the cpu table to the height the statement gives; the
    muldiv table's height is the proof's, refused (reason 2) unless 0 < log height <= the cpu table's -> 0 or the
    verifier's reason.  prep_root (8 Montgomery words) with program_log_height: the statement is the rv32im-elf set's
    seven tables (or the rv32im-mem set's nine) under that verifying key (rk_p3_verify_key) -- the program table's
    height is then pinned by the verifier, no longer the proof's.  The memop and memory tables' heights are the proof's,
    refused (reason 2) unless 0 < log height <= the cpu table's + 1"""
    from . import p3
    vt = rv32_verifier_tables(tables, proof, prep_root, program_log_height)
    return 2 if vt is None else p3.verify(vt, proof, init, params, prep_root=prep_root)


def rv32_verifier_tables(tables, proof, prep_root=None, program_log_height=None):
    """the tables verify_rv32_shard hands the verifier -- no traces, the heights pinned as described there; None where the
    proof's muldiv height is out of range (reason 2).  Also what the FRI statements about a shard proof take
    (raiko_amd.fri_transcript.statement(..., prep_root=...))"""
    from . import p3
    # the chip set is the one with this many tables; the program table's height (0) is the proof's, as the muldiv table's
    sets = [_rv32_set(c)[2:] + (_RV32_MEM_TABLES.get(c, 0),) for c in RV32_CHIPS if (c in KEYED_CHIPS) == (prep_root is not None)]
    pinned, n_mem = next(((p, m) for p, muldiv, m in sets if 2 + len(p) + muldiv + m == len(tables)), (None, 0))
    if pinned is None:
        raise ValueError("%d tables are no rv32 chip set's shard" % len(tables))
    if prep_root is not None and not program_log_height:
        raise ValueError("a verifying key is the root and the program table's log height")
    pinned = (tables[0].log_height, int(program_log_height) if prep_root is not None else 0, *pinned)
    vt = []
    for i, t in enumerate(tables):
        v = p3.Table(t.air, None, t.public_values)
        if i < len(pinned):
            v.log_height = pinned[i]
        else:
            lg = int(proof[1 + i]) if len(proof) > 1 + i else 0
            if not 0 < lg <= tables[0].log_height + (1 if i >= len(tables) - n_mem else 0):
                return None
            v.log_height = lg
        vt.append(v)
    return vt


# ---- the rv32im-elf chip set (raiko_amd/rv32elf.py): the program and the fixed tables proven from a key ---------------
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


def p3_rv32elf_shards(ex: Execution, image, ext_w=None, airs=None):
    """rv32im-elf shards in numpy: tables = cpu, program, register, byte, range, shift, muldiv (rv32elf.airs), the four
    lookup tables with their preprocessed matrix in Table.prep (p3.setup commits them; rv32elf.prep_tables(image)).
    image: rv32elf.program_image(elf).  The yardstick for rk_rv32elf_prep_device / rk_exec_rv32elf_shard_device."""
    from . import p3, rv32elf
    if ex.witness is None or ex.rv32 is None:
        raise ValueError("execute(..., record_trace=True) first")
    airs = airs or rv32elf.airs(ext_w)
    preps = [None if m is None else p3.to_mont(m) for m in rv32elf.preps_of(image)]
    out = []
    for s, (_code, data), (start, end, ecalls) in zip(ex.segments, ex.witness, ex.rv32):
        canon, _pc, _regs = rv32elf.shard_tables(s, data, start, end, ecalls, image)
        pub_cpu, pub_reg = _rv32_publics(s, start, end)
        pubs = [pub_cpu, (), pub_reg] + [()] * (len(canon) - 3)
        tables = [p3.Table(a, p3.to_mont(t), pv, prep=pm) for a, t, pv, pm in zip(airs, canon, pubs, preps)]
        out.append((tables, np.array(list(s.pre_state) + list(s.post_state), dtype=np.uint32)))
    return out


class Rv32Key:
    """setup_rv32_elf's result, the proving key of one ELF under the rv32im-elf chip set: .image [(vaddr, words)], .key
    the p3.Key over the program image and the byte / range / shift tuples, .root its 8 Montgomery words and
    .program_log_height (together the verifying key), .d_words the image's words in device memory (what
    rk_exec_rv32elf_shard_device compares the executed words with), .airs the seven AIRs.  close() frees the device
    memory."""

    def __init__(self, image, seg_vaddr, seg_words, key, d_words, program_log_height, airs, chips="rv32im-elf"):
        self.image, self.seg_vaddr, self.seg_words, self.key, self.d_words = image, seg_vaddr, seg_words, key, d_words
        self.root, self.program_log_height, self.airs, self.chips = key.root, program_log_height, airs, chips
        self._preps = None

    @property
    def bytes(self):
        return self.key.bytes + 4 * self.d_words.size()

    def host_preps(self):
        """the preprocessed matrices as the chip set's prep_tables gives them (Montgomery words), in table order"""
        from . import p3
        if self._preps is None:
            self._preps = [None if m is None else p3.to_mont(m) for m in _rv32_set(self.chips)[0].preps_of(self.image)]
        return self._preps

    def close(self):
        if self.key is not None:
            self.key.close()
            self.d_words.free()
        self.key = self.d_words = None


def setup_rv32_elf(hal, elf: bytes, params=None, ext_w=None, airs=None, chips="rv32im-elf") -> Rv32Key:
    """The setup of `client.setup(ELF)` for the rv32im-elf chip set: the ELF's program image (rk_exec_program_image), the
    four preprocessed matrices written on hal's GPU (rk_rv32elf_prep_device) and committed (rk_p3_setup) -> Rv32Key.
    params: the parameter set to put hal's context under first (None: the context's current one); ext_w: the AIRs'
    extension (default params' / the context's).  chips="rv32im-mem": that chip set's key (rk_rv32mem_prep_device: the
    program matrix has 48 columns) and nine AIRs."""
    from . import p3, rv32, rv32cf, rv32elf
    if chips not in KEYED_CHIPS:
        raise ValueError("chips must be one of %s" % (KEYED_CHIPS,))
    lib = _lib.load()
    if params is not None:
        _lib.check(hal._ctx, lib.rk_set_params(hal._ctx, C.byref(params)))
    if airs is None:
        airs = _rv32_airs_of(chips, int(hal.get_params().ext_w) if ext_w is None else ext_w)
    vaddr, count, words = program_image_c(elf)
    rows = 2
    while rows < words.size:
        rows <<= 1
    logs = {1: rows.bit_length() - 1, 3: rv32.BYTE_LOG_ROWS, 4: rv32elf.RANGE_LOG_ROWS, 5: rv32cf.SHIFT_LOG_ROWS}
    bufs = {i: hal.alloc_elem(airs[i].prep_width << lg) for i, lg in logs.items()}
    d_words = None
    try:
        prep_device = lib.rk_rv32mem_prep_device if chips == "rv32im-mem" else lib.rk_rv32elf_prep_device
        _lib.check(hal._ctx, prep_device(
            hal._ctx, vaddr.ctypes.data_as(_lib.u32p), count.ctypes.data_as(_lib.u32p), vaddr.size, words.ctypes.data_as(_lib.u32p),
            words.size, C.c_void_p(bufs[1].ptr), rows, C.c_void_p(bufs[3].ptr), C.c_void_p(bufs[4].ptr), C.c_void_p(bufs[5].ptr)))
        tables = []
        for i, a in enumerate(airs):
            t = p3.Table(a, None, np.zeros(a.n_public, dtype=np.uint32))
            t.log_height = logs.get(i, 1)
            tables.append(t)
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
    return Rv32Key(image, vaddr, count, key, d_words, logs[1], airs, chips)


def p3_rv32mem_shards(ex: Execution, image, ext_w=None, airs=None):
    """rv32im-mem shards in numpy: rv32elf's seven tables, then memop and memory (rv32mem.airs), the four lookup tables
    with their preprocessed matrix in Table.prep (rv32mem.prep_tables(image)).  The yardstick for rk_rv32mem_prep_device
    / rk_exec_rv32mem_shard_device."""
    from . import p3, rv32mem
    if ex.witness is None or ex.rv32 is None or ex.mem is None:
        raise ValueError("execute(..., record_trace=True) first")
    airs = airs or rv32mem.airs(ext_w)
    preps = [None if m is None else p3.to_mont(m) for m in rv32mem.preps_of(image)]
    out = []
    for s, (_code, data), (start, end, ecalls), mem in zip(ex.segments, ex.witness, ex.rv32, ex.mem):
        canon, _pc, _regs = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)
        pub_cpu, pub_reg = _rv32_publics(s, start, end)
        pubs = [pub_cpu, (), pub_reg] + [()] * (len(canon) - 3)
        tables = [p3.Table(a, p3.to_mont(t), pv, prep=pm) for a, t, pv, pm in zip(airs, canon, pubs, preps)]
        out.append((tables, np.array(list(s.pre_state) + list(s.post_state), dtype=np.uint32)))
    return out
