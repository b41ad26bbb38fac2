"""Lines that the nodes of an in-process cluster print to std::cout come out
whole (RunLocalCluster's per-thread line buffer, src/post_office.cc).

tests/_bin/lines_host: every worker prints its lines in several `<<` pieces,
all workers at once, then a last line without a newline.  No GPU needed.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "lines_host")


def test_lines_of_concurrent_workers_stay_whole():
    assert os.path.exists(EXE), f"{EXE} not built (make -C parameter-server_amd all)"
    nw, lines = 4, 2000
    args = [EXE, "-ns", "1", "-nw", str(nw), str(lines)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    tail = re.compile(r"(?:worker \d+ left without a newline)+")
    seen = {w: [] for w in range(nw)}
    left = 0
    for line in r.stdout.split("\n"):
        m = re.fullmatch(r"worker (\d+), line (\d+): 0, 0", line)
        if m:
            seen[int(m.group(1))].append(int(m.group(2)))
            continue
        # the unfinished lines go out when their threads end: whole, in any order
        assert line == "" or tail.fullmatch(line), repr(line)
        left += line.count("left without a newline")
    assert left == nw
    for w in range(nw):
        assert seen[w] == list(range(lines)), w  # every line once, a worker's lines in order
