"""A trained row table saved by one job and resumed by another, on another number
of servers, end to end: KVWorker -> slicer -> the three row handles' SaveModel /
LoadModel (ps/row_checkpoint.h: psg_table_export / psg_table_assign on a
psg_table in HBM), on the MI355X, every node a process.

tests/harness/kv_rows_ckpt_device.cpp is run twice.  The first job trains
iterations 0-1, every server saves its shard, the worker pulls every row into
dir/mid, trains iterations 2-3 and pulls into dir/final.  The second job starts
from nothing, every server loads the keys of its own range from every saved
shard and checks its iteration (2); its Pulls must equal dir/mid and, after
iterations 2-3, dir/final byte for byte (a failed CHECK aborts the job:
non-zero exit).
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_ckpt_device")
KEYS = 400


def run(ns, nw, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    assert os.path.exists(EXE), f"{EXE} not built"
    r = subprocess.run([EXE, "-ns", str(ns), "-nw", str(nw), "-procs", *map(str, args)], capture_output=True, text=True,
                       timeout=timeout, env=e)
    return r


def ok(r, phase, nw):
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count(f"rows ckpt {phase} ok") == nw, r.stdout


def saved(tmp_path_factory, kind, width, ns, nw):
    d = tmp_path_factory.mktemp(f"{kind}-w{width}")
    ok(run(ns, nw, kind, width, KEYS, d, "save", ns), "save", nw)
    for f in [f"shard-{r}" for r in range(ns)] + ["mid", "final"]:
        assert os.path.getsize(d / f) > 0, f
    return d


@pytest.fixture(scope="module", params=[4, 3])
def opt_saved(request, tmp_path_factory):
    return request.param, saved(tmp_path_factory, "opt", request.param, 2, 1)


@pytest.mark.parametrize("ns", [1, 2, 3])
def test_opt_handle_resumes_on_any_number_of_servers(opt_saved, ns):
    width, d = opt_saved
    ok(run(ns, 1, "opt", width, KEYS, d, "resume", 2), "resume", 1)


@pytest.mark.parametrize("width", [4, 3])
def test_sync_handle_resumes_on_three_servers(tmp_path_factory, width):
    d = saved(tmp_path_factory, "sync", width, 2, 2)
    ok(run(3, 2, "sync", width, KEYS, d, "resume", 2), "resume", 2)


@pytest.mark.parametrize("width", [4, 3])
def test_accumulate_handle_resumes_on_two_servers(tmp_path_factory, width):
    d = saved(tmp_path_factory, "acc", width, 1, 1)
    ok(run(2, 1, "acc", width, KEYS, d, "resume", 1), "resume", 1)


def test_a_file_of_another_width_is_refused(opt_saved):
    width, d = opt_saved
    r = run(1, 1, "opt", width, KEYS, d, "badwidth", 2)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("rows ckpt badwidth ok") == 1, r.stdout


FILE_EXE = os.path.join(ROOT, "tests", "_bin", "row_ckpt_file")


@pytest.mark.parametrize("width,rows,adam", [(64, 30000, 1), (3, 1000, 0), (4, 1, 1)])
def test_files_come_back_bit_for_bit(tmp_path, width, rows, adam):
    """ps::SaveRowTable / LoadRowTable on one GPU (tests/harness/unit/row_ckpt_file.cpp):
    whole, in two parts of the key range, and with or without moments on either
    side; 30000 rows of W = 64 with moments are three chunks of 16 MiB."""
    assert os.path.exists(FILE_EXE), f"{FILE_EXE} not built"
    r = subprocess.run([FILE_EXE, str(width), str(rows), str(tmp_path / "table"), str(adam)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "row ckpt file ok" in r.stdout
    assert os.path.getsize(tmp_path / "table") == 64 + rows * (8 + width * 4 + (width * 16 if adam else 0))
