"""Seeded initial rows across servers, end to end: KVWorker -> slicer / router ->
the three row handles after SetInit (psg_table_set_init on a psg_table in HBM),
on the MI355X, every node a process.

tests/harness/kv_rows_init_device.cpp restates the generator on the host.  Its
save phase checks that ids nobody has sent come back as the generator's rows
through kRowLookup and as its pooled sums through ZPullPooled, ZPullPooledWeighted
and ZPullPooledMean, that training starts every id from its initial row, and
leaves every row before and after two more iterations in dir/mid and dir/final;
these files must be the same at every server count.  The resume phase starts
from nothing on another number of servers, with the same SetInit, loads the
saved shards and must reproduce both files byte for byte, although iterations
2-3 name ids the files do not hold (a failed CHECK aborts the job: non-zero
exit).
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_init_device")


def run(ns, *args, timeout=120):
    # recycled HBM blocks start as NaN (device::Alloc): a reply read before its
    # kernel wrote it fails the comparison
    e = dict(os.environ, PS_POOL_POISON="1")
    assert os.path.exists(EXE), f"{EXE} not built"
    return subprocess.run([EXE, "-ns", str(ns), "-nw", "1", "-procs", *map(str, args)], capture_output=True, text=True,
                          timeout=timeout, env=e)


def ok(r, phase):
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count(f"rows init {phase} ok") == 1, r.stdout


def read(d, name):
    with open(d / name, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """(kind, width) -> the directory of the save phase on ONE server, run once"""
    made = {}

    def get(kind, width):
        if (kind, width) not in made:
            d = tmp_path_factory.mktemp(f"{kind}-w{width}-ns1")
            ok(run(1, kind, width, d, "save", 1), "save")
            made[kind, width] = d
        return made[kind, width]

    return get


@pytest.mark.parametrize("ns", [2, 3, 4])
@pytest.mark.parametrize("kind,width", [("opt", 4), ("opt", 3), ("sync", 4), ("acc", 3)])
def test_every_server_count_gives_the_rows_of_one_server(saved, tmp_path, kind, width, ns):
    one = saved(kind, width)
    ok(run(ns, kind, width, tmp_path, "save", ns), "save")
    for name in ("mid", "final"):
        assert len(read(one, name)) == 300 * width * 4
        assert read(tmp_path, name) == read(one, name), f"{name} at {ns} servers differs from one server's"
    assert read(one, "mid") != read(one, "final")
    # the job resumed on ONE server from these ns shards
    ok(run(1, kind, width, tmp_path, "resume", ns), "resume")


@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("kind,width", [("opt", 4), ("sync", 3), ("acc", 4)])
def test_resume_on_more_servers(saved, kind, width, ns):
    ok(run(ns, kind, width, saved(kind, width), "resume", 1), "resume")
