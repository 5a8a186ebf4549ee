"""What the FRI statement modules (fri_chip, fri_reduce, fri_open) do alike once a statement's AIRs and witness are
written: p3 tables over rows, tables pinned to the statement's heights, the sizes the library gives, the rows written on
the GPU, the proof over them.  The modules pass what is theirs: AIRs, public values and heights per table, the table
names as the size struct prefixes them, the struct, the names of the two library functions and the arguments both start
with (behind the context), the host arrays the row writer reads."""
import ctypes as C

from . import _lib, p3


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
