"""Rows trained on the servers in sync-mode rounds, end to end: KVWorker ->
slicer -> KVServerRowSyncHandle (ps/row_sync_handle.h: one
psg_table_update_merged per round on a psg_table in HBM) -> answers, on the
MI355X.

tests/harness/kv_rows_sync_device.cpp seeds rows with an accumulate Push, runs
three rounds in which every worker Pushes gradients on an overlapping ascending
list (worker 0's with cmd = 1 end an iteration on every server) between
barriers, replays merge and update on a host map in plain C++ and CHECKs every
pulled value bit for bit; a wrapper on each server CHECKs iteration() after
every gradient Push (a failed CHECK aborts the job: non-zero exit).
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_sync_device")


def run(path, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)


CASES = [(ns, nw, width, 1) for ns, nw in ((1, 1), (1, 2), (2, 2), (1, 3)) for width in (4, 20)]
CASES.append((2, 2, 3, 0))  # SGD on the element path: a handle without Adam state


@pytest.mark.parametrize("ns,nw,width,adam", CASES)
def test_rows_trained_in_rounds_through_the_kv_api(ns, nw, width, adam):
    assert os.path.exists(EXE), f"{EXE} not built"
    r = run(EXE, "-ns", ns, "-nw", nw, "-procs", width, 2000, adam)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows sync ok") == nw, r.stdout
