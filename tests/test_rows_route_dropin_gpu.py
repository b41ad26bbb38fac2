"""Key lists in any order and with repeats on a table sharded over several
servers, end to end: KVWorker's Any calls -> psg_route / psg_rows_gather (or the
host route) -> one message per server on the route's bounds -> the row handles
built with any_order / KVServerRowSyncHandle -> psg_rows_scatter, on the MI355X.

tests/harness/kv_rows_route_device.cpp replays every request on a host map, one
occurrence after the other, and CHECKs every pulled value bit for bit (a failed
CHECK aborts the job: non-zero exit).
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_route_device")


def run(path, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)


def check(r, ns, nw):
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows route ok") == nw, r.stdout
    # every worker's lists reached every server
    assert re.findall(r"servers addressed (\d+)", r.stdout) == [str(ns)] * nw, r.stdout


@pytest.mark.parametrize("procs", [False, True], ids=["threads", "procs"])
@pytest.mark.parametrize("ns,nw", [(1, 1), (2, 1), (2, 2), (4, 2)])
@pytest.mark.parametrize("mode", [0, 1], ids=["accumulate", "sgd"])
def test_routed_lists_through_the_kv_api(mode, ns, nw, procs):
    assert os.path.exists(EXE), f"{EXE} not built"
    width = 20 if mode == 0 else 4
    args = ["-ns", ns, "-nw", nw] + (["-procs"] if procs else []) + [width, 3000, mode]
    check(run(EXE, *args), ns, nw)


@pytest.mark.parametrize("procs", [False, True], ids=["threads", "procs"])
def test_a_sync_round_of_routed_lists(procs):
    assert os.path.exists(EXE), f"{EXE} not built"
    args = ["-ns", 2, "-nw", 2] + (["-procs"] if procs else []) + [4, 3000, 2]
    check(run(EXE, *args), 2, 2)


def test_an_any_call_refuses_a_custom_slicer():
    assert os.path.exists(EXE), f"{EXE} not built"
    r = run(EXE, "-ns", 2, "-nw", 1, 4, 100, 0, "slicer")
    assert r.returncode != 0, r.stdout
    assert "cannot be combined with a custom slicer" in r.stdout + r.stderr
    assert "passed a custom slicer" not in r.stdout
