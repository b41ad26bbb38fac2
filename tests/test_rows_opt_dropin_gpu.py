"""Rows trained on the servers end to end: KVWorker -> slicer ->
KVServerRowOptHandle (ps/row_opt_handle.h: psg_table_update on a psg_table in
HBM) -> pull merge, on the MI355X.

tests/harness/kv_rows_opt_device.cpp seeds rows with accumulate Pushes, runs
three iterations of gradient Pushes (worker 0's with cmd = 1 end an iteration
on every server) between barriers, replays every request on a host map with the
update's arithmetic in plain C++ and CHECKs every pulled value bit for bit (a
failed CHECK aborts the job: non-zero exit).
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_opt_device")


def run(path, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)


CASES = [(ns, nw, procs, width, 1) for ns, nw, procs in ((1, 1, False), (2, 2, False), (2, 1, True))
         for width in (4, 20)]
CASES.append((2, 2, False, 4, 0))  # SGD: a handle without Adam state


@pytest.mark.parametrize("ns,nw,procs,width,adam", CASES)
def test_rows_trained_through_the_kv_api(ns, nw, procs, width, adam):
    assert os.path.exists(EXE), f"{EXE} not built"
    args = ["-ns", ns, "-nw", nw] + (["-procs"] if procs else []) + [width, 3000, adam]
    r = run(EXE, *args)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows opt ok") == nw, r.stdout
