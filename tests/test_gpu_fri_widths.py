"""fri_reduce_kernel (raiko_amd/csrc/fri_tables.hip) at the widths where its scan changes shape: a workgroup of 256 lanes
takes 256 columns of a matrix at a time, the running sums come from a shuffle scan within a wave of 64, a carry across
waves and a carry across 256-column pieces through LDS, and the running reduced opening is handed from the last column
of a matrix to the next matrix.  The kernel's workgroup runs only on the GPU (tests/emul runs its lane bodies).

Two shards of wide tables (threshold_cases.FRI_SHARDS): A, widths 256, 65 and 513 in one round; B, widths 64 and 255 at
one height and 257 at another.  For each, under each of the three statements that write the reduce table -- the reduce
statement (the kernel's row stride 0: the table's own width), the open and the transcript statement (stride = the width
of the table widened by the sponge columns; sponge chains of about 105 permutations per lane) --: the GPU's shard proof
is the oracle's, and every table of device_tables equals the numpy witness word for word.
tests/test_launch_thresholds.py checks the layouts.

The steps are those of tests/test_gpu_fri_reduce.py, ..._open.py and ..._transcript.py (their step_rows, with the shard
taken from threshold_cases), each in a child process of its own under a time limit of its own (this file run as a
script: `python tests/test_gpu_fri_widths.py STATEMENT SHARD`), once: a step that fails is not started again, and after a
step that ended by a signal or ran into its time limit no further step is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATEMENTS = ["reduce", "open", "transcript"]
_stop = []          # set by a step that faulted or hung: nothing more is started on the GPU


def run_step(statement, shard, limit=300):
    if _stop:
        pytest.fail("not started: the step %s ended abnormally before" % _stop[0])
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), statement, shard], cwd=ROOT, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _stop.append(statement + " " + shard)
        pytest.fail("%s %s ran into its time limit of %d s" % (statement, shard, limit))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stop.append(statement + " " + shard)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("shard", ["A", "B"])
@pytest.mark.parametrize("statement", STATEMENTS)
def test_gpu_rows_equal_the_witness(statement, shard):
    assert "rows ok" in run_step(statement, shard)


# ---------------------------------------------------------------------------------------------- the step (child process)
def main(statement, shard):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as o
    import threshold_cases as T
    from raiko_amd import hal, p3
    mod = __import__("test_gpu_fri_" + statement)

    def shard_of(h, case, **more):
        out = T.fri_setup(case, h.set_params, lambda tables, init: p3.prove(h, tables, init))
        return out + ((1, T.FRI_OVER),) if statement == "transcript" else out

    mod._shard = shard_of            # step_rows as it stands, on a shard that is no case of P3_CASES
    h = hal.HipHal(0)
    try:
        mod.step_rows(h, shard)
    finally:
        o.oracle_set_params()
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
