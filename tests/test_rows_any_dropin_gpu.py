"""Key lists with repeats, and in any order, end to end: KVWorker -> slicer ->
KVServerRowHandle / KVServerRowOptHandle built with any_order (ps/row_handle.h,
ps/row_opt_handle.h: psg_table_handle_any / psg_table_update_any on a psg_table
in HBM) -> pull merge, on the MI355X.

tests/harness/kv_rows_any_device.cpp replays every request on a host map, one
occurrence after the other, and CHECKs every pulled value bit for bit (a failed
CHECK aborts the job: non-zero exit).
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_any_device")


def run(path, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("ns,nw,procs", [(1, 1, False), (2, 2, False), (2, 1, True)])
@pytest.mark.parametrize("mode", [0, 1], ids=["accumulate", "sgd"])
def test_lists_with_repeats_through_the_kv_api(mode, ns, nw, procs):
    assert os.path.exists(EXE), f"{EXE} not built"
    width = 20 if mode == 0 else 4
    args = ["-ns", ns, "-nw", nw] + (["-procs"] if procs else []) + [width, 3000, mode]
    r = run(EXE, *args)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows any ok") == nw, r.stdout
