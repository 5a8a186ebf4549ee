"""ELF -> verified shard proofs, the way SP1 proves an execution (rk_p3_*): `execute_and_prove_p3` runs the program, then
proves its shards in batches; `P3Pipeline` proves each shard while the next one executes.  Both take the stand-in trace
circuit (raiko_amd/p3_trace.py) or one of the rv32 chip sets (raiko_amd/rv32_sets.py)."""
import ctypes as C
from typing import Sequence

from . import _lib, p3, rv32commit, rv32io, rv32link
from .executor import Stepper, execute
from .p3_trace import next_trace_shard, p3_program_air, p3_range_air, p3_shards, p3_trace_air
from .rv32_sets import (CHIPS, KEYED_CHIPS, RV32_CHIPS, _free, _rv32_airs_of, check_rv32_chain, execute_rv32_device,
                        next_rv32_shard, rv32_publics, setup_rv32_elf, verify_rv32_execution, verify_rv32_shard)


class P3Pipeline:
    """ELF -> verified shard proofs with the three stages overlapped: the calling thread runs the executor one shard at a
    time (rk_exec_next_segment), has the shard's cpu table written on the GPU from the executed cycles
    (rk_exec_witness_device_rows: the trace never exists on the host) and builds its lookup tables; a second thread proves
    the shards as they arrive (rk_p3_prove on its own context, the cpu table an on_device input); a small pool verifies
    the proofs (rk_p3_verify is host code).  The contexts and the (compiled) AIRs live as long as the object: run() any
    number of programs, then close().  chips="rv32i" / "rv32i-cf" / "rv32im": every shard's tables of that chip set are written on
    the GPU (rv32_sets.next_rv32_shard; `lookups` does not apply), every proof is checked by verify_rv32_shard and the run
    by check_rv32_chain.  chips="rv32im-elf" / "rv32im-mem": run() sets the program's key up first (setup_rv32_elf on the
    proving context), proves every shard under it, checks every proof against its root, and closes it when the run ends.
    link=True (chips="rv32im-mem" only; ValueError otherwise): the shards' memories are linked (raiko_amd/rv32link.py) --
    every proof is checked with its journal as claims, the run by rv32link.check_memory_chain from the ELF's memory
    image, and the Execution carries ex.journals and ex.final_memory.  io=True (chips="rv32im-mem" only; composes with
    link): the ecalls are bound to the run's input (raiko_amd/rv32io.py) -- every proof is checked against its slice of
    input_words, the run by rv32io.check_io_chain, and ex.exit_code / ex.input_words_read are the verified ones.
    commit=True (with io=True only; composes with link): the COMMIT journal is bound (raiko_amd/rv32commit.py) -- every
    proof is checked with its commit log, the run by rv32commit.check_commit_chain, ex.commit_logs holds the logs and
    ex.journal is the PROVEN journal, cut from them; a journal that differs from the executor's is an RkError."""

    def __init__(self, params=None, device: int = 0, lookups=True, compile_airs=True, chips="trace", link=False, io=False, commit=False):
        from .hal import HipHal, make_params
        if chips not in CHIPS:
            raise ValueError("chips must be one of %s" % (CHIPS,))
        if link and chips != "rv32im-mem":
            raise ValueError("link=True needs chips=\"rv32im-mem\"")
        if io and chips != "rv32im-mem":
            raise ValueError("io=True needs chips=\"rv32im-mem\"")
        if commit and not (io and chips == "rv32im-mem"):
            raise ValueError("commit=True needs chips=\"rv32im-mem\" and io=True")
        self.params = params if params is not None else make_params(1)
        self.lookups, self.chips, self.link, self.io, self.commit = lookups, chips, link, io, commit
        ext_w = int(self.params.ext_w)
        self.rv32_airs = _rv32_airs_of(chips, ext_w, link, io, commit) if chips in RV32_CHIPS else None
        self.cpu_air = p3_trace_air(lookups, ext_w)
        self.prog_air, self.range_air = (p3_program_air(ext_w), p3_range_air(ext_w)) if lookups else (None, None)
        self.wit_hal, self.prove_hal = HipHal(device), HipHal(device)
        _lib.check(self.prove_hal._ctx, self.prove_hal._lib.rk_set_params(self.prove_hal._ctx, C.byref(self.params)))
        if link or io:    # the digests are committed on the witness context: under the prover's parameter set
            _lib.check(self.wit_hal._ctx, self.wit_hal._lib.rk_set_params(self.wit_hal._ctx, C.byref(self.params)))
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
        from .hal import _ptr
        todo = queue.Queue(maxsize=3)           # back-pressure: at most three shards' tables wait for the prover
        done = queue.Queue()                    # device tables the prover is through with: freed by the thread that owns their context
        proofs, checks, kept, errors, stmts, journals, logs = [], [], [], [], [], [], []
        params, rv32i, link, io, commit = self.params, self.chips in RV32_CHIPS, self.link, self.io, self.commit
        key = setup_rv32_elf(self.prove_hal, elf, airs=self.rv32_airs, chips=self.chips, link=link, io=io, commit=commit) \
            if self.chips in KEYED_CHIPS else None
        vk = dict(prep_root=key.root, program_log_height=key.program_log_height) if key else {}
        try:
            stepper = Stepper(elf, input_words, shard_po2)
        except Exception:
            if key:
                key.close()
            raise
        pool = ThreadPoolExecutor(max_workers=4)
        if rv32i:
            next_shard = lambda: next_rv32_shard(stepper, self.wit_hal, self.rv32_airs, self.chips, key, link, io, commit)
        else:
            next_shard = lambda: next_trace_shard(stepper, self.wit_hal, (self.cpu_air, self.prog_air, self.range_air), self.lookups)
        check = verify_rv32_shard if rv32i else p3.verify
        preps = key.host_preps() if key and keep_tables else None

        def prover():
            try:
                while True:
                    item = todo.get()
                    if item is None:
                        return
                    _seg, tables, bufs, init = item[:4]
                    jk = dict(journal=item[4]) if link else {}
                    if io:
                        jk["input_words"] = list(input_words)
                    if commit:
                        jk["commit_log"] = item[-1]
                        logs.append(item[-1])
                        item = item[:-1]
                    journals.extend(item[4:])
                    pf = p3.prove(self.prove_hal, tables, init, device_traces=[None if d is None else (_ptr(d[0]), d[1]) for d in bufs],
                                  key=key.key if key else None)
                    proofs.append(pf)
                    stmts.append((tables, init))
                    if verify:
                        checks.append(pool.submit(check, tables, pf, init, params, **vk, **jk))
                    if keep_tables:
                        kept.append(([t if d is None else p3.Table(t.air, d[0].to_host().reshape(1 << d[1], t.air.width), t.public_values, prep=pm)
                                      for t, d, pm in zip(tables, bufs, preps or [None] * len(tables))], init))
                    done.put(bufs)
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
                item = next_shard()
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
        if link:
            ex.journals = journals
            ex.final_memory = rv32link.check_memory_chain(journals, rv32link.memory_image(elf))
        if io and verify:
            code, ex.input_words_read = rv32io.check_io_chain([rv32io.publics_of(t[rv32io.IO_TABLE].public_values[:rv32io.N_PUBLIC_IO])
                                                               for t, _i in stmts], list(input_words))
            ex.exit_code = ex.exit_code if code is None else code
        if commit and verify:
            pubs = [rv32commit.publics_of(t[rv32io.IO_TABLE].public_values) for t, _i in stmts]
            rv32commit.check_commit_chain(pubs)
            proven = b"".join(rv32commit.log_bytes(pub, log) for pub, log in zip(pubs, logs))
            if proven != ex.journal:
                raise _lib.RkError(_lib.RK_ERR_VERIFY, "the proven journal is not the executor's")
            ex.journal = proven
        if commit:
            ex.commit_logs = logs
        return ex, proofs, kept


def execute_and_prove_p3_pipelined(elf: bytes, input_words: Sequence[int] = (), shard_po2: int = 20, params=None, device: int = 0,
                                   lookups=True, compile_airs=True, verify=True, keep_tables=False, chips="trace", link=False, io=False,
                                   commit=False):
    """one program through a P3Pipeline of its own"""
    pipe = P3Pipeline(params, device, lookups, compile_airs, chips, link, io, commit)
    try:
        return pipe.run(elf, input_words, shard_po2, verify, keep_tables)
    finally:
        pipe.close()


def execute_and_prove_p3(elf: bytes, input_words: Sequence[int] = (), shard_po2: int = 16, params=None, device: int = 0, batch: int = 3,
                         lookups=False, chips="trace", link=False, io=False, commit=False):
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
    (raiko_amd/rv32mem.py): nine traces per shard (rk_exec_rv32mem_shard_device), the same key protocol.  link=True
    (chips="rv32im-mem" only; ValueError otherwise): the shards' memories are linked (raiko_amd/rv32link.py): every
    shard's journal is read off its memory table on the GPU (rk_rv32mem_journal_device), its digest is the table's public
    values, the pool's verifiers check every proof with the journal as claims (rk_p3_prove_shards_claims), and the run is
    checked by verify_rv32_execution(journals=, image=) from the ELF's memory image.  The Execution then carries
    ex.journals and ex.final_memory (the final words of everything the run touched).  io=True (chips="rv32im-mem" only;
    composes with link): the ecalls are bound to input_words (raiko_amd/rv32io.py): ten traces per shard
    (rk_exec_rv32io_shard_device) under the io key, the pool's verifiers check every proof with its slice of the input as
    claims, and the run is checked by verify_rv32_execution(input_words=); ex.exit_code and ex.input_words_read are then
    what that check returns.  commit=True (with io=True only; composes with link): the COMMIT journal is bound
    (raiko_amd/rv32commit.py): ten traces per shard (rk_exec_rv32commit_shard_device) under the io key, every proof is
    checked with its commit log as claims, the run by verify_rv32_execution(commit_logs=, expected_journal=the
    executor's); ex.journal is then the proven journal and ex.commit_logs the logs."""
    from .hal import make_params
    params = params if params is not None else make_params(1)
    if chips not in CHIPS:
        raise ValueError("chips must be one of %s" % (CHIPS,))
    if link and chips != "rv32im-mem":
        raise ValueError("link=True needs chips=\"rv32im-mem\"")
    if io and chips != "rv32im-mem":
        raise ValueError("io=True needs chips=\"rv32im-mem\"")
    if commit and not (io and chips == "rv32im-mem"):
        raise ValueError("commit=True needs chips=\"rv32im-mem\" and io=True")
    if chips in RV32_CHIPS:
        from .hal import HipHal
        hal = HipHal(device)
        key, vk = None, {}
        try:
            if chips in KEYED_CHIPS:
                key = setup_rv32_elf(hal, elf, params, chips=chips, link=link, io=io, commit=commit)
                vk = dict(prep_root=key.root.copy(), program_log_height=key.program_log_height)
            ex, shards, dev_traces, bufs, *journals = execute_rv32_device(hal, elf, input_words, shard_po2, ext_w=int(params.ext_w),
                                                                          chips=chips, key=key, link=link, io=io, commit=commit)
            logs = journals.pop() if commit else None
            hal.sync()
            claims = [rv32link.claims_of(j) for j in journals[0]] if link else [[] for _ in shards] if io else None
            if io:    # the prover's own statement: the slice its io table's public values name
                words = list(input_words)
                for c, (tables, _init) in zip(claims, shards):
                    pub = rv32io.publics_of(tables[rv32io.IO_TABLE].public_values[:rv32io.N_PUBLIC_IO])
                    c += rv32io.claims_of(pub["pos_start"], words[pub["pos_start"]:pub["pos_end"]])
            if commit:
                for c, log in zip(claims, logs):
                    c += rv32commit.claims_of(log)
            try:
                proofs = p3.prove_shards(shards, params, device=device, batch=batch, verify=True, device_traces=dev_traces,
                                         key=key.key if key else None, claims=claims)
            finally:
                for d in bufs:
                    _free(d)
        finally:
            if key:
                key.close()
            hal.close()
        if link:
            image = rv32link.memory_image(elf)
            vk.update(journals=journals[0], image=image)
        if io:
            vk.update(input_words=list(input_words))
        if commit:
            vk.update(commit_logs=logs, expected_journal=ex.journal)
        checked = verify_rv32_execution(shards, proofs, params, entry_pc=ex.segments[0].start_pc if ex.segments else None, **vk)
        if io:
            ex.exit_code, ex.input_words_read = ex.exit_code if checked[0] is None else checked[0], checked[1]
            del vk["input_words"]
        if commit:
            ex.journal, ex.commit_logs = checked[2], logs
            del vk["commit_logs"], vk["expected_journal"]
        if link:
            ex.journals, ex.final_memory = journals[0], rv32link.check_memory_chain(journals[0], image)
            del vk["journals"], vk["image"]
        if vk:
            ex.prep_root, ex.program_log_height = vk["prep_root"], vk["program_log_height"]
        return ex, shards, proofs
    ex = execute(elf, input_words, segment_limit_po2=shard_po2, record_trace=True)
    shards = p3_shards(ex, lookups=lookups, ext_w=int(params.ext_w))
    proofs = p3.prove_shards(shards, params, device=device, batch=batch, verify=True)
    return ex, shards, proofs
