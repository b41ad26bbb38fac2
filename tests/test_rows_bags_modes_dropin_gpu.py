"""Weighted and mean bags on a table sharded over several servers, end to end:
KVWorker::ZPullPooledWeighted / ZPushPooledWeighted / ZPullPooledMean /
ZPushPooledMean / ZPushPooledMeanAll -> psg_route / psg_route_bags (and the
weights routed by psg_rows_gather, the gradient rows divided by
psg_pool_scale_mean) -> one message per server (with its weights frame) -> the
row handles' cmds 5-8 -> psg_table_lookup_pooled_weighted / _update_pooled_weighted
-> psg_pool_reduce / psg_pool_reduce_mean of the servers' partial frames, on the
MI355X.

tests/harness/kv_rows_bags_modes_device.cpp replays every request on a host map
by the definitions of include/psg.h ("Weighted and mean bags across servers")
and CHECKs every reply and a final ZPullAny of all rows bit for bit (a failed
CHECK aborts the job: non-zero exit).
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_bags_modes_device")


def run(path, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a frame read before its
    # kernel wrote it fails the harness's comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    return subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("procs", [False, True], ids=["threads", "procs"])
@pytest.mark.parametrize("ns,nw", [(1, 1), (2, 1), (2, 2), (4, 2)])
@pytest.mark.parametrize("width", [4, 20])
def test_weighted_and_mean_calls_through_the_kv_api(width, ns, nw, procs):
    assert os.path.exists(EXE), f"{EXE} not built"
    args = ["-ns", ns, "-nw", nw] + (["-procs"] if procs else []) + [width, 2000, 0]
    r = run(EXE, *args)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows bags modes ok") == nw, r.stdout
    # every worker's lists reached every server
    assert re.findall(r"servers addressed (\d+)", r.stdout) == [str(ns)] * nw, r.stdout
    # three rounds of nw turns, every other turn with step on BOTH its Pushes: only
    # worker 0's count, and every server counted each of them
    steps = 2 * sum(1 for turn in range(3 * nw) if turn % 2 == 0 and turn % nw == 0)
    assert re.findall(r"iterations((?: \d+)+),", r.stdout) == [f" {steps}" * ns] * nw, r.stdout


def test_mean_pushes_in_sync_rounds_and_lookups_on_the_sync_handle():
    assert os.path.exists(EXE), f"{EXE} not built"
    r = run(EXE, "-ns", 2, "-nw", 2, 4, 2000, 1)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows bags modes sync ok") == 2, r.stdout
    # two rounds, each ended by worker 0's step on every server
    assert re.findall(r"iterations((?: \d+)+)$", r.stdout, re.M) == [" 2 2"] * 2, r.stdout


def test_the_sync_handle_refuses_a_weighted_update():
    assert os.path.exists(EXE), f"{EXE} not built"
    r = run(EXE, "-ns", 2, "-nw", 1, 4, 200, 2)
    assert r.returncode != 0, r.stdout
    assert "a round's frames carry no weights" in r.stdout + r.stderr
    assert "took a weighted update" not in r.stdout


def test_the_accumulate_handle_answers_the_lookups_and_refuses_a_weighted_update():
    assert os.path.exists(EXE), f"{EXE} not built"
    r = run(EXE, "-ns", 2, "-nw", 1, 4, 200, 3)
    assert "answered the weighted and the mean lookup" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.returncode != 0, r.stdout
    assert "is served by KVServerRowOptHandle only" in r.stdout + r.stderr
    assert "took a weighted update" not in r.stdout
