"""Rows of W values per key end to end: KVWorker -> slicer -> KVServerRowHandle
(ps/row_handle.h, a psg_table in HBM) -> pull merge, on the MI355X.

tests/harness/kv_rows_device.cpp replays every request on a host map with the
reference's loop and CHECKs every pulled value bit for bit (a failed CHECK
aborts the job: non-zero exit).
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_device")


def run(path, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("ns,nw,procs", [(1, 1, False), (2, 2, False), (2, 1, True)])
@pytest.mark.parametrize("width", [4, 20])
def test_rows_through_the_kv_api(width, ns, nw, procs):
    assert os.path.exists(EXE), f"{EXE} not built"
    args = ["-ns", ns, "-nw", nw] + (["-procs"] if procs else []) + [width, 3000]
    r = run(EXE, *args)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows ok") == nw, r.stdout
