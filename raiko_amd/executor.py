"""The executor + segmenter in front of the proving path: binding of rk_exec_* (raiko_amd/csrc/executor.cpp, the host
executor) and `execute_and_prove`, the shape of `prove_locally` (reference provers/risc0/driver/src/bonsai.rs:230-272):
run the guest ELF, cut the run into segments of at most 2^po2 cycles, prove every segment, return the receipt.

What the library restates is the public part (RV32IM, ELF32, power-of-two segments); the cycle
model, the ecall table and the state digest are stand-ins and the rv32im circuit's witness layout
is not available (risc0-circuit-rv32im is outside the reference tree), so the segments handed to
the prover carry SYNTHETIC trace columns of the executed segment's size -- seeded by the
segment's state digests, so a different run gives different seals.  See include/raiko_hip.h.

The same execution as shards of a uni-stark proof system, the way SP1 proves one: p3_trace.py (the stand-in trace circuit),
rv32_sets.py (the rv32 chip sets), p3_exec.py (ELF -> shard proofs); their public names are importable from here too."""
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

    def pc_publics(self):
        """the first and the last pc as 16-bit limbs (start lo / hi, end lo / hi), Montgomery words: the public values of
        the segment's cpu table and the first globals of its trace-circuit segment"""
        return np.array([(v << 32) % P for v in (self.start_pc & 0xFFFF, self.start_pc >> 16, self.end_pc & 0xFFFF, self.end_pc >> 16)],
                        dtype=np.uint32)

    def init_words(self):
        """the machine-state digests before and after the segment: what seeds the transcript of its shard proof"""
        return np.array(self.pre_state + self.post_state, dtype=np.uint32)


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
    # chips="rv32im-mem" with link=True (raiko_amd/rv32link.py): per shard the journal (k, 3) uint32 -- word address, INIT,
    # FINAL of every touched word, ascending -- and the run's final image of the touched words {word address: word}
    journals: Optional[list] = None
    final_memory: Optional[dict] = None
    # with record_trace: per segment (ecall rows (k, 5): cycle, t0, a0 before, a1, input position before; the input
    # position at the segment's start) (rk_exec_ecall_args): the side data of the io form of rv32im-mem (rv32io.py)
    ecall_args: Optional[list] = None
    # with record_trace: per segment (commit reads (k, 3): cycle, word address, word of every word an ecall COMMIT reads;
    # the journal's length at the segment's start) (rk_exec_commit_reads): the side data of the commit form (rv32commit.py)
    commit_reads: Optional[list] = None
    # commit=True: per shard the commit log (k, 3) uint32 -- jpos, word, S | CNT << 16 -- the verifier is handed
    commit_logs: Optional[list] = None


class ExecutorError(RuntimeError):
    pass


TRACE_CODE_COLS, TRACE_DATA_COLS, TRACE_ACCUM_COLS = 2, 16, 4


def _open(entry, elf, input_words, **opts):
    """rk_exec_elf / rk_exec_open -> the executor's handle; ExecutorError with the executor's own message"""
    lib = _lib.load()
    words = np.ascontiguousarray(input_words, dtype=np.uint32)
    opts = RkExecOpts(struct_size=C.sizeof(RkExecOpts), input_words=words.ctypes.data_as(_lib.u32p), n_input_words=words.size, **opts)
    handle = C.c_void_p()
    st = getattr(lib, entry)(bytes(elf), len(elf), C.byref(opts), C.byref(handle))
    if st != 0:
        detail = lib.rk_exec_error(handle).decode() if handle else ""
        if handle:
            lib.rk_exec_free(handle)
        raise ExecutorError("%s%s" % (lib.rk_strerror(st).decode(), ": " + detail if detail else ""))
    return handle


def _summary(lib, handle):
    """-> (RkExecSummary, the journal)"""
    summ = RkExecSummary()
    lib.rk_exec_summary_get(handle, C.byref(summ))
    buf = C.create_string_buffer(max(int(summ.journal_bytes), 1))
    n = C.c_size_t(0)
    lib.rk_exec_journal(handle, buf, summ.journal_bytes, C.byref(n))
    return summ, buf.raw[: n.value]


def _segment_get(lib, handle, index) -> ExecSegment:
    s = RkExecSegment()
    lib.rk_exec_segment_get(handle, index, C.byref(s))
    return ExecSegment(s.index, s.po2, int(s.cycles), s.start_pc, s.end_pc, s.exit, tuple(s.pre_state), tuple(s.post_state))


def _witness(lib, handle, seg):
    """rk_exec_witness, the native witness generator of the stand-in trace circuit -> (code (2, 2^po2), data (16, 2^po2))"""
    code = np.zeros((TRACE_CODE_COLS, 1 << seg.po2), dtype=np.uint32)
    data = np.zeros((TRACE_DATA_COLS, 1 << seg.po2), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_witness(handle, seg.index, code.ctypes.data_as(_lib.u32p), data.ctypes.data_as(_lib.u32p)))
    return code, data


def _lookup_tables(lib, handle, index):
    """rk_exec_lookup_tables -> (program table (rows, 5), range table (65536, 2)), row-major Montgomery words"""
    rng = np.zeros((1 << 16, 2), dtype=np.uint32)
    rows = C.c_size_t(0)
    st = lib.rk_exec_lookup_tables(handle, index, rng.ctypes.data_as(_lib.u32p), None, C.byref(rows))
    if st != _lib.RK_ERR_CAPACITY:
        _lib.check(None, st or _lib.RK_ERR_INTERNAL)
    prog = np.zeros((rows.value, 5), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_lookup_tables(handle, index, rng.ctypes.data_as(_lib.u32p), prog.ctypes.data_as(_lib.u32p), C.byref(rows)))
    return prog, rng


def execute(elf: bytes, input_words: Sequence[int] = (), segment_limit_po2: int = 20, session_limit: int = 0,
            record_trace: bool = False, profile: bool = False) -> Execution:
    """`ExecutorImpl::from_elf(env, elf).run()` (bonsai.rs:246-269).  Raises ExecutorError on a trap
    (illegal instruction, misaligned access, unknown ecall, session limit).  profile: what the reference's
    `profile: true` switches on (`env_builder.enable_profiler(..)`, bonsai.rs:252-255) -- here the cycles spent at
    every program counter, most expensive first, in Execution.profile."""
    lib = _lib.load()
    handle = _open("rk_exec_elf", elf, input_words, segment_limit_po2=segment_limit_po2, session_limit=session_limit,
                   record_trace=1 if record_trace else 0, profile=1 if profile else 0)
    try:
        summ, journal = _summary(lib, handle)
        segs = [_segment_get(lib, handle, i) for i in range(summ.n_segments)]
        witness = [_witness(lib, handle, sg) for sg in segs] if record_trace else None
        ex = Execution(segs, journal, summ.exit_code, int(summ.total_cycles), int(summ.input_words_read), witness)
        if record_trace:   # rk_exec_lookup_tables: the program / range tables of the uni-stark form with lookups
            ex.lookup_tables = [_lookup_tables(lib, handle, sg.index) for sg in segs]
            ex.rv32 = [_rv32_side(lib, handle, sg.index) for sg in segs]
            ex.mem = [mem_accesses(lib, handle, sg.index) for sg in segs]
            ex.ecall_args = [ecall_args(lib, handle, sg.index) for sg in segs]
            ex.commit_reads = [commit_reads(lib, handle, sg.index) for sg in segs]
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
        lib.rk_exec_free(handle)


def segments_for_proving(ex: Execution, widths: Tuple[int, int, int] = (16, 16, 224)) -> List[Segment]:
    """One prover segment per executed segment, of the executed size (2^po2 rows); the trace columns
    are the synthetic stand-in (no rv32im witness layout here), seeded by the segment's digests and
    carrying them as globals, so the seal binds the state transition the executor saw."""
    out = []
    for s in ex.segments:
        seed = int.from_bytes(s.init_words().astype("<u4").tobytes()[:8], "little")
        seg = synthetic_segment(s.po2, widths, seed=seed % (1 << 62), n_globals=0)
        seg.globals_ = np.array(list(s.init_words()) + [s.start_pc % P, s.exit], dtype=np.uint32)
        out.append(seg)
    return out


class Stepper:
    """rk_exec_open / rk_exec_next_segment: the executor one segment at a time (risc0's `run_with_callback`
    shape), with the trace circuit's witness of every segment as it completes"""

    def __init__(self, elf: bytes, input_words: Sequence[int] = (), segment_limit_po2: int = 20):
        self._lib = _lib.load()
        self._h = _open("rk_exec_open", elf, input_words, segment_limit_po2=segment_limit_po2, session_limit=0, record_trace=1)
        self.more = True
        self.n = 0

    def step(self) -> Optional[ExecSegment]:
        """runs the next segment -> its ExecSegment (the rk_exec_* entry points take its .index), or None after the last"""
        if not self.more:
            return None
        more = C.c_int(0)
        st = self._lib.rk_exec_next_segment(self._h, C.byref(more))
        if st != 0:
            raise ExecutorError("%s: %s" % (self._lib.rk_strerror(st).decode(), self._lib.rk_exec_error(self._h).decode()))
        self.more = bool(more.value)
        seg = _segment_get(self._lib, self._h, self.n)
        self.n += 1
        return seg

    def next(self, hal=None):
        """-> (ExecSegment, code, data) of the next executed segment, or None after the last.  With `hal` (a HipHal)
        the witness columns are written on the GPU (rk_exec_witness_device) and code / data are device buffers."""
        seg = self.step()
        if seg is None:
            return None
        if hal is None:
            return (seg, *_witness(self._lib, self._h, seg))
        code = hal.alloc_elem(TRACE_CODE_COLS << seg.po2)
        data = hal.alloc_elem(TRACE_DATA_COLS << seg.po2)
        _lib.check(None, self._lib.rk_exec_witness_device(hal._ctx, self._h, seg.index, C.c_void_p(code.ptr), C.c_void_p(data.ptr)))
        hal.sync()   # the session's contexts run on other streams
        return seg, code, data

    def lookup_tables(self, index):
        """the program / range tables of segment `index` (rk_exec_lookup_tables), as Execution.lookup_tables has them"""
        return _lookup_tables(self._lib, self._h, index)

    def finish(self) -> Execution:
        summ, journal = _summary(self._lib, self._h)
        ex = Execution([], journal, summ.exit_code, int(summ.total_cycles), int(summ.input_words_read))
        self.close()
        return ex

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rk_exec_free(self._h)
            self._h = None


def _trace_tapset():
    """the trace circuit's taps: every column at this row, the data columns next pc lo / hi and `active` at the next too"""
    from .segment import make_tapset
    return make_tapset([[(0,)] * TRACE_ACCUM_COLS, [(0,)] * TRACE_CODE_COLS,
                        [((0, 1) if c in (2, 3, 15) else (0,)) for c in range(TRACE_DATA_COLS)]])


def trace_segments(ex: Execution, program=None) -> List[Segment]:
    """One prover segment per executed segment with its EXECUTION TRACE as witness (rk_exec_witness) and the
    stand-in trace circuit's constraint list (circuit_program.trace_program) behind eval_check: the seal then says
    that the pc chain of the committed trace is consistent and starts / ends at the public pcs.  Not rv32im."""
    from .circuit_program import Program, trace_program
    if ex.witness is None:
        raise ValueError("execute(..., record_trace=True) first")
    taps = _trace_tapset()
    if program is None:
        program = Program(*trace_program(taps), taps)
    out = []
    for s, (code, data) in zip(ex.segments, ex.witness):
        accum = np.ascontiguousarray(data[:TRACE_ACCUM_COLS])      # unconstrained in this circuit; no accumulate hook
        out.append(_trace_segment(s, taps, program, [accum, code, data]))
    return out


def _trace_segment(s: ExecSegment, taps, program, groups) -> Segment:
    seg = Segment(po2=s.po2, taps=taps, groups=groups, check=None, globals_=np.concatenate([s.pc_publics(), s.init_words()]), n_accum_mix=4,
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
        taps = _trace_tapset()
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


def ecall_args(lib, handle, index):
    """rk_exec_ecall_args -> ((k, 5) uint32: cycle, t0, a0 before, a1, input position before; the input position at the
    segment's start)"""
    n, pos = C.c_size_t(0), C.c_uint32(0)
    st = lib.rk_exec_ecall_args(handle, index, None, 0, C.byref(n), C.byref(pos))
    if st != _lib.RK_ERR_CAPACITY:
        _lib.check(None, st)
    out = np.zeros((max(n.value, 1), 5), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_ecall_args(handle, index, out.ctypes.data_as(_lib.u32p), out.shape[0], C.byref(n), C.byref(pos)))
    return out[: n.value], int(pos.value)


def commit_reads(lib, handle, index):
    """rk_exec_commit_reads -> ((k, 3) uint32: cycle, word address, word; the journal's length at the segment's start)"""
    n, pos = C.c_size_t(0), C.c_uint32(0)
    st = lib.rk_exec_commit_reads(handle, index, None, 0, C.byref(n), C.byref(pos))
    if st != _lib.RK_ERR_CAPACITY:
        _lib.check(None, st)
    out = np.zeros((max(n.value, 1), 3), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_commit_reads(handle, index, out.ctypes.data_as(_lib.u32p), out.shape[0], C.byref(n), C.byref(pos)))
    return out[: n.value], int(pos.value)


# the uni-stark side of the same executions.  rv32_sets and p3_exec import this module, so these lines come last: every
# name above exists by now.  (Import raiko_amd.executor, not those two, first.)
from .p3_trace import BUS_PROGRAM, BUS_RANGE16, RANGE_LIMB_COLS, p3_program_air, p3_range_air, p3_shards, p3_trace_air  # noqa: E402,F401
from .rv32_sets import (CHIPS, KEYED_CHIPS, RV32_CHIPS, Rv32Key, _rv32_airs_of, _rv32_set, check_rv32_chain,  # noqa: E402,F401
                        execute_rv32_device, p3_rv32_airs, p3_rv32_shards, p3_rv32cf_airs, p3_rv32cf_shards, p3_rv32elf_shards,
                        p3_rv32im_airs, p3_rv32im_shards, p3_rv32mem_shards, program_image_c, rv32_publics, rv32_shard_device,
                        rv32_verifier_tables, setup_rv32_elf, verify_rv32_execution, verify_rv32_shard)
from .p3_exec import P3Pipeline, execute_and_prove_p3, execute_and_prove_p3_pipelined  # noqa: E402,F401
