"""Row-wise Adagrad on the row table (psg_table_set_adagrad, k_rows_walk_rowwise in
csrc/psg_rows.hip) against RowAdagradModel: rows, accumulators and PSG_PULL
replies bit for bit, through every update call.

Widths: below one 16-B unit (1, 3), one unit (4), padding to the tree's power of
two (5, 12, 100, 252, 260, 1020, 4095), one full group (64 elements; 256 = 64
units), the group at its cap with several units a lane (260 .. 4096), and, for
widths of whole units, gradients 4 B off a 16-B boundary (the element path)."""
import numpy as np
import pytest

import psg
from row_adagrad_model import RowAdagradModel
from row_model import F32, POOL_MEAN, POOL_SUM, PULL, PUSH, SAME_LIST, SORTED

pytestmark = pytest.mark.gpu

KEND = 1 << 40
LR, ALR, EPS = 0.05, 0.1, 1e-8
WIDTHS = (1, 3, 4, 5, 12, 64, 100, 252, 256, 260, 1020, 1024, 4095, 4096)
CASES = [(w, 0) for w in WIDTHS] + [(w, 4) for w in WIDTHS if w % 4 == 0]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def dev(a, off=0):
    """the array on the device, starting `off` bytes behind a 16-B boundary"""
    a = np.ascontiguousarray(a)
    b = psg.DeviceBuffer(a.nbytes + 16)
    b.upload(a, offset=off)
    return b, b.ptr + off


def pair(width, eps=EPS, init=0.0):
    t, m = psg.Table(psg.F32, width, 0, KEND, 0), RowAdagradModel(F32, width, key_end=KEND)
    t.set_adagrad(ALR, eps, init)
    assert m.set_adagrad(ALR, eps, init) == {} and t.adagrad() == (ALR, eps, init)
    return t, m


def same(got, exp):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    assert got.dtype == exp.dtype
    np.testing.assert_array_equal(got.view(u).ravel(), exp.view(u).ravel())


def check(t, m):
    keys, rows = t.dump()
    np.testing.assert_array_equal(keys, m.keys)
    same(rows, m.rows)
    same(t.dump_accum(), m.acc)


def update(t, m, q, g, any_order=False, off=0, it=0):
    """PUSH|PULL through update / update_any on table and model; the replies compared"""
    n, w = len(q), t.width
    (kb, kp), (gb, gp) = dev(q), dev(g, off)
    out = psg.DeviceBuffer(n * w * 4)
    (t.update_any if any_order else t.update)(PUSH | PULL, kp, gp, out, n, LR, it)
    exp = (m.update_any if any_order else m.update)(PUSH | PULL, q, g, LR, it)
    same(out.download(np.float32, n * w), exp["out"])
    check(t, m)


def merged(t, m, lists, grads, path, off=0):
    k, w = len(lists), t.width
    kd, gd = [dev(q) for q in lists], [dev(g, off) for g in grads]
    outs = [psg.DeviceBuffer(len(q) * w * 4) for q in lists]
    got = t.update_merged(PUSH | PULL, [p for _, p in kd], [p for _, p in gd], outs, [len(q) for q in lists], LR, 1)
    exp = m.update_merged(PUSH | PULL, lists, grads, LR, 1)
    assert got == exp["path"] == path
    for j in range(k):
        same(outs[j].download(np.float32, len(lists[j]) * w), exp["outs"][j])
    check(t, m)


def grads_for(rng, n, w):
    return rng.uniform(-1, 1, (n, w)).astype(np.float32)


@pytest.mark.parametrize("width,off", CASES, ids=[f"w{w}-off{o}" for w, o in CASES])
def test_update_calls_match_the_model(width, off):
    rng = np.random.default_rng(width + off)
    keys = np.sort(rng.choice(1 << 20, 60, replace=False).astype(np.uint64))
    known, fresh = keys[:40], keys[40:]
    t, m = pair(width)
    for _ in range(2):  # the second step starts from the first one's accumulators
        update(t, m, known, grads_for(rng, 40, width), off=off)
    # any order: one id named 9 times, ids the table does not hold among the rest
    q = np.concatenate([known[:24], np.repeat(known[3], 8), fresh[:8]])
    rng.shuffle(q)
    assert (q == known[3]).sum() == 9
    update(t, m, q, grads_for(rng, len(q), width), any_order=True, off=off)
    merged(t, m, [known] * 3, [grads_for(rng, 40, width) for _ in range(3)], SAME_LIST, off)
    lists = [known[5:30], rng.permutation(keys[20:]), np.concatenate([known[:7], known[:7]])]
    merged(t, m, lists, [grads_for(rng, len(x), width) for x in lists], SORTED, off)
    t.close()


@pytest.mark.parametrize("order", ("ascending", "shuffled"))
@pytest.mark.parametrize("width", (4, 100, 256))
def test_pooled_updates_match_the_model(width, order):
    rng = np.random.default_rng(7 * width + len(order))
    keys = np.sort(rng.choice(1 << 20, 60, replace=False).astype(np.uint64))
    t, m = pair(width)
    update(t, m, keys[:40], grads_for(rng, 40, width))
    q = keys[5:55].copy() if order == "ascending" else rng.choice(keys, 120).astype(np.uint64)
    sizes = [0, 1, 7] + [3] * ((len(q) - 8) // 3)
    sizes += [len(q) - sum(sizes), 0]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n, nb = len(q), len(sizes)
    path = SAME_LIST if order == "ascending" else SORTED
    for weights, mode in ((None, POOL_SUM), (rng.uniform(-2, 2, n).astype(np.float32), POOL_SUM), (None, POOL_MEAN)):
        g = grads_for(rng, nb, width)
        (_, kp), (_, op), (_, gp) = kd, od, gd = dev(q), dev(offsets), dev(g)
        wd = dev(weights) if weights is not None else (None, None)
        if weights is None and mode == POOL_SUM:
            t.update_pooled(kp, op, gp, n, nb, LR, 0)
        else:
            t.update_pooled_weighted(kp, op, wd[1], mode, gp, n, nb, LR, 0)
        assert m.update_pooled_weighted(q, offsets, g, LR, 0, weights, mode) == {"path": path}
        check(t, m)
    # a round of one pooled and one plain frame
    plain = rng.permutation(keys[:30])
    g0, g1 = grads_for(rng, nb, width), grads_for(rng, len(plain), width)
    held = [dev(q), dev(offsets), dev(g0), dev(plain), dev(g1)]
    frames = [(held[0][1], held[1][1], held[2][1]), (held[3][1], None, held[4][1])]
    assert t.update_pooled_merged(frames, [n, len(plain)], [nb, 0], LR, 2) == SORTED
    assert m.update_pooled_merged([(q, offsets, g0), (plain, None, g1)], LR, 2) == {"path": SORTED}
    check(t, m)
    t.close()


def test_accumulators_follow_their_rows_through_insert_growth_erase_and_clear():
    rng = np.random.default_rng(11)
    width, init = 4, 0.125
    t, m = pair(width, init=init)
    keys = np.sort(rng.choice(1 << 20, 1500, replace=False).astype(np.uint64))
    first, between = keys[::3], np.sort(np.concatenate([keys[1::3], keys[2::3]]))
    update(t, m, first, grads_for(rng, len(first), width))
    assert int(t.info().capacity) == 1024 and not (t.dump_accum() == init).any()
    update(t, m, between, grads_for(rng, len(between), width))  # inserted between the present rows, past 1024
    assert int(t.info().size) == 1500 and int(t.info().capacity) > 1024
    gone = rng.permutation(keys)[:500]
    (_, gp) = held = dev(gone)
    assert t.erase(gp, len(gone)) == m.erase(gone)["erased"] == 500
    check(t, m)
    update(t, m, keys[::2], grads_for(rng, len(keys[::2]), width))  # survivors step on, erased ids start afresh
    t.clear()
    m.clear()
    assert t.adagrad() == (ALR, EPS, init)
    update(t, m, keys[:5], np.zeros((5, width), np.float32))
    same(t.dump_accum(), np.full(5, init))
    t.close()


def test_tiny_and_huge_gradients_in_one_request_and_a_zero_row():
    rng = np.random.default_rng(12)
    width = 12
    t, m = pair(width)
    keys = np.arange(10, 50, dtype=np.uint64)
    update(t, m, keys, grads_for(rng, 40, width))
    before = t.dump()[1].view(np.uint32).copy()
    g = grads_for(rng, 40, width)
    g[::3] *= np.float32(1e-30)
    g[1::3] *= np.float32(1e18)
    g[5] = 0.0
    update(t, m, keys, g)
    assert np.isfinite(m.rows).all() and np.isfinite(m.acc).all()
    np.testing.assert_array_equal(t.dump()[1].view(np.uint32)[5], before[5])
    t.close()
