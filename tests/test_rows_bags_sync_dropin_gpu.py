"""Sync-mode rounds of pooled gradient frames, end to end: KVWorker::ZPushPooledAll
-> psg_route / psg_route_bags -> one message to EVERY server (its keys stretch,
possibly empty, its nb + 1 offsets, the gradient frame) -> KVServerRowSyncHandle
holds the frames of the round -> ONE psg_table_update_pooled_merged call per
round and server, on the MI355X.

tests/harness/kv_rows_bags_sync_device.cpp sends three rounds from all workers
at once (all pooled; one worker's list on server 0 alone; one plain PushPull
among pooled Pushes), replays every round on a host map — merge per id, one
Adam step with the server's iteration — and CHECKs the plain reply, a pooled
Pull after every round and a final Pull of all rows bit for bit (a failed CHECK
aborts the job: non-zero exit).
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_bags_sync_device")
ROUNDS = 3


def run(path, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a frame read before its
    # copy or kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("procs", [False, True], ids=["threads", "procs"])
@pytest.mark.parametrize("ns,nw", [(1, 1), (2, 1), (1, 2), (2, 3), (4, 3)])
@pytest.mark.parametrize("width", [4, 20])
def test_pooled_rounds_through_the_kv_api(width, ns, nw, procs):
    assert os.path.exists(EXE), f"{EXE} not built"
    args = ["-ns", ns, "-nw", nw] + (["-procs"] if procs else []) + [width, 2000]
    r = run(EXE, *args)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows bags sync ok") == nw, r.stdout
    # every round closed on every server and ended worker 0's iteration there:
    # also round 1, where worker 0's list names ids of server 0 alone
    assert re.findall(r"iterations((?: \d+)+)$", r.stdout, re.M) == [f" {ROUNDS}" * ns] * nw, r.stdout
