"""Rows read without inserting them and rows erased, end to end: KVWorker ->
slicer / router -> a row handle's kRowLookup Pull and kRowErase Push
(ps/row_handle.h: psg_table_lookup / psg_table_erase on a psg_table in HBM), on
the MI355X, every node a process.

tests/harness/kv_rows_lifecycle_device.cpp compares every pulled value with its
host replay bit for bit (a failed CHECK aborts the job: non-zero exit).  Here
the servers' size() lines are summed over the shards: a lookup leaves the sum as
it was, the same list as a plain Pull grows it by exactly the unseen ids, and
the erases lower it by exactly the present keys they named.
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_lifecycle_device")
KEYS = 1200


def run(ns, nw, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    assert os.path.exists(EXE), f"{EXE} not built"
    return subprocess.run([EXE, "-ns", str(ns), "-nw", str(nw), "-procs", *map(str, args)], capture_output=True,
                          text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("ns,nw", [(1, 1), (2, 2), (2, 1)])
@pytest.mark.parametrize("kind,width", [("opt", 4), ("opt", 3), ("acc", 20)])
def test_lookup_and_erase_through_the_kv_api(kind, width, ns, nw):
    r = run(ns, nw, kind, width, KEYS)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    ok = re.findall(r"rows lifecycle ok: worker \d+, \w+, width \d+, keys (\d+), unseen (\d+), erased (\d+)", r.stdout)
    assert len(ok) == nw, r.stdout
    keys, unseen, erased = (sum(int(x[i]) for x in ok) for i in range(3))
    assert keys == KEYS and unseen > 0 and erased > 0
    size = {}
    for point, rank, rows in re.findall(r"rows lifecycle size (\w+) server (\d+): (\d+)", r.stdout):
        size.setdefault(point, {})[int(rank)] = int(rows)
    assert all(len(size[p]) == ns for p in ("trained", "looked", "pulled", "erased")), r.stdout
    total = {p: sum(v.values()) for p, v in size.items()}
    assert total["trained"] == KEYS
    assert total["looked"] == total["trained"], "a lookup inserted rows"
    assert total["pulled"] == total["trained"] + unseen, "a plain Pull inserts exactly the unseen ids"
    assert total["erased"] == total["pulled"] - erased, "an erase removes exactly the present keys it names"
    if ns > 1:
        assert all(v > 0 for v in size["trained"].values()), "every server holds rows"


@pytest.mark.parametrize("kind", ["opt", "acc"])
def test_a_pushpull_with_the_erase_cmd_fails_its_check(kind):
    r = run(1, 1, kind, 4, 100, "badcmd", timeout=60)
    assert r.returncode != 0, r.stdout
    assert "a PushPull cannot carry cmd 4" in r.stdout + r.stderr
    assert "a PushPull passed" not in r.stdout
