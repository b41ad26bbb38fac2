"""Row-wise Adagrad end to end: KVWorker::ZPushAny -> psg_route -> two servers'
KVServerRowSyncHandle with SetAdagrad -> psg_table_update_merged on an Adagrad
table, three rounds from two workers (threads of one process), then a ZPullAny.

tests/harness/kv_rows_adagrad_device.cpp prints the pulled rows as hex words; the
rounds are replayed here on ONE whole-range RowAdagradModel (a row's bits do not
depend on the number of servers) and compared bit for bit.  Keys and gradients
are the harness's formulas, restated."""
import os
import subprocess

import numpy as np
import pytest

from row_adagrad_model import RowAdagradModel
from row_model import F32, PUSH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_bin", "kv_rows_adagrad_device")
NS, NW, WIDTH, ROUNDS, IDS, OCCURRENCES = 2, 2, 8, 3, 50, 80
LR, EPS, INIT = float(np.float32(0.05)), 1e-8, 0.125
KMAX = (1 << 64) - 1
STRIDE = KMAX // 64


def test_rounds_through_the_kv_api_match_one_model():
    assert os.path.exists(EXE), f"{EXE} not built"
    env = dict(os.environ, PS_POOL_POISON="1")
    r = subprocess.run([EXE, "-ns", str(NS), "-nw", str(NW), str(WIDTH)], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got = {int(f[1]): np.array([int(x, 16) for x in f[2:]], dtype=np.uint32)
           for f in (line.split() for line in r.stdout.splitlines()) if f and f[0] == "row"}
    assert len(got) == IDS

    m = RowAdagradModel(F32, WIDTH, key_end=KMAX)
    assert m.set_adagrad(LR, EPS, INIT) == {}
    i, c = np.arange(OCCURRENCES), np.arange(WIDTH)
    for rnd in range(ROUNDS):
        keys = [((i * 7 + rank * 3 + rnd * 11) % IDS).astype(np.uint64) * np.uint64(STRIDE) + np.uint64(1)
                for rank in range(NW)]
        grads = [((i[:, None] + 2 * c[None, :] + rank + rnd) % 7 - 3).astype(np.float32) for rank in range(NW)]
        m.update_merged(PUSH, keys, grads, LR, rnd)
    assert m.size == IDS and len(np.unique(m.acc)) > 1
    for key, row in zip(m.keys, m.rows):
        np.testing.assert_array_equal(got[int(key)], row.view(np.uint32))
