"""What the FRI statement modules (fri_chip, fri_reduce, fri_open, fri_transcript) do alike.  Before a statement exists:
the capture of what one verifier run over the shard proof read (`capture`: one ctypes call for all four rk_p3_fri_*
functions and their _key twins for proofs under a verifying key).  Once a statement's AIRs and witness are written: p3
tables over rows, tables pinned to the statement's heights, the sizes the library gives, the rows written on
the GPU, the proof over them.  The modules pass what is theirs: AIRs, public values and heights per table, the table
names as the size struct prefixes them, the struct, the names of the two library functions and the arguments both start
with (behind the context), the host arrays the row writer reads."""
import collections
import ctypes as C

import numpy as np

from . import _lib, p3

SP1_ROOT_2_27 = 0x1A427A41

Shape = collections.namedtuple("Shape", "log_max n_rounds blowup_log2 queries root_2_27", defaults=(SP1_ROOT_2_27,))


def capture(name, n_arrays, tables, proof, init, params, prep_root=None):
    """one of the library's rk_p3_fri_* captures of a verifier run over `proof`: `name` is the function, n_arrays the
    arrays it hands back -> (verdict, Shape or None, arrays...): Montgomery words; nothing but the verdict unless it is 0.
    The library says how large the arrays are (RK_ERR_CAPACITY) and the call is made again with room for them.
    prep_root: the verifying key's root (p3.Key.root) of a proof with preprocessed columns: the call goes to the _key
    twin of `name` (a `name` that ends in _key goes there with whatever root is given, None = NULL)."""
    keyed = ()
    if prep_root is not None or name.endswith("_key"):
        name = name if name.endswith("_key") else name + "_key"
        kr = None if prep_root is None else np.ascontiguousarray(prep_root, dtype=np.uint32)
        assert kr is None or kr.size == 8
        keyed = (kr.ctypes.data_as(_lib.u32p) if kr is not None else None,)
    arr, keep = p3._c_tables(tables)
    iw = np.ascontiguousarray(init, dtype=np.uint32)
    pf = np.ascontiguousarray(proof, dtype=np.uint32)
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    shape = np.zeros(4, dtype=np.uint32)
    n = [C.c_size_t(0) for _ in range(n_arrays)]
    out = [np.zeros(0, dtype=np.uint32)] * n_arrays
    while True:
        bufs = [x for a in out for x in (u(a) if a.size else None, a.size)]
        rc = getattr(_lib.load(), name)(C.byref(params) if params is not None else None, arr, len(tables), *keyed, u(iw), iw.size, u(pf), pf.size,
                                        u(shape), *bufs, *[C.byref(v) for v in n])
        if rc != _lib.RK_ERR_CAPACITY:
            break
        out = [np.zeros(v.value, dtype=np.uint32) for v in n]
    del keep
    if rc < 0:
        _lib.check(None, rc)
    if rc != 0:
        return (rc,) + (None,) * (1 + n_arrays)
    s = [int(v) for v in p3.from_mont(shape)]
    root = int(params.root_2_27) if params is not None else SP1_ROOT_2_27
    return (0, Shape(s[0], s[1], s[2], s[3], root)) + tuple(out)


def tables_from_rows(airs, rows, public_values):
    """p3 tables over canonical rows (the witness or a variation of it)"""
    return [p3.Table(air, p3.to_mont(r), pv) for air, r, pv in zip(airs, rows, public_values)]


def pinned_tables(airs, public_values, heights):
    """the tables without traces, every height pinned"""
    out = []
    for air, pv, h in zip(airs, public_values, heights):
        t = p3.Table(air, None, pv)
        t.log_height = h
        out.append(t)
    return out


def sizes(size_info, sizes_fn, lead):
    """the library's size struct for the leading arguments `lead` -> dict"""
    out = size_info()
    _lib.check(None, getattr(_lib.load(), sizes_fn)(*lead, C.byref(out)))
    return {n: int(getattr(out, n)) for n, _ in out._fields_ if n != "reserved"}


def device_tables(hal, names, sz, rows_fn, lead, inputs):
    """the rows of the tables `names` (sz: their sizes) written on the GPU under hal's parameter set ->
    [(DeviceBuffer, log_height)]: the rows stay in HBM, ready as on_device tables"""
    from .hal import _ptr
    ins = [hal.copy_from_elem(a) for a in inputs]
    bufs = [hal.alloc_elem(sz[n + "_width"] << sz[n + "_log_height"]) for n in names]
    args = []
    for b in bufs:
        args += [_ptr(b), b.size()]
    _lib.check(hal._ctx, getattr(_lib.load(), rows_fn)(hal._ctx, *lead, *[_ptr(b) for b in ins], *args))
    hal.sync()
    return [(b, sz[n + "_log_height"]) for b, n in zip(bufs, names)]


def prove(hal, pinned, init, device):
    """the proof by rk_p3_prove over the on_device tables `device` (device_tables' result)"""
    from .hal import _ptr
    return p3.prove(hal, pinned, init, device_traces=[(_ptr(b), h) for b, h in device])
