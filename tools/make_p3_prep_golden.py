#!/usr/bin/env python3
"""Writes the fixtures of tests/test_p3_prep.py (needs the GPU; run once, the results are committed):

    python tools/make_p3_prep_golden.py [out_dir = tests/golden/p3-prep]

  range_prep.npz   the range-prep demo (p3.lookup_demo_tables_prep) at log_cpu 4, log_range 3
  gate_next.npz    p3_prep_cases.gate_table(3, 2, cubic=True): an AIR with a PREP_NEXT constraint and two quotient chunks
each under the SP1 preset with 7 queries and 2 proof-of-work bits: the proof words, the key's root, the init words, and
every table's trace and preprocessed matrix (Montgomery words; the AIRs are rebuilt from code by the test)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OVER = dict(queries=7, pow_bits=2)


def main():
    import p3_prep_cases as K
    from raiko_amd import hal as H, p3
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "p3-prep")
    os.makedirs(out, exist_ok=True)
    hal = H.HipHal(0)
    blob = hal.set_params(1, **OVER)
    init = p3.to_mont([4, 3, 7])
    for name, tables in (("range_prep", p3.lookup_demo_tables_prep(4, 3, seed=5)), ("gate_next", [K.gate_table(3, 2, cubic=True)])):
        key = p3.setup(hal, tables)
        pf = p3.prove(hal, tables, init, key=key)
        assert p3.verify(K.pinned(tables), pf, init, params=blob, prep_root=key.root) == 0
        arrays = {"proof": pf, "root": key.root, "init": init}
        for i, t in enumerate(tables):
            arrays["trace%d" % i] = t.trace
            if t.prep is not None:
                arrays["prep%d" % i] = t.prep
        np.savez_compressed(os.path.join(out, name + ".npz"), **arrays)
        print(name, pf.size, "words")
        key.close()
    hal.close()


if __name__ == "__main__":
    main()
