"""Row-wise Adagrad on F16 / BF16 rows (psg_table_set_adagrad_half,
k_rows_walk_rowwise_half in csrc/psg_rows.hip) against RowAdagradHalfModel: rows,
accumulators and PSG_PULL replies byte for byte, through every update call.

Widths: the element path and a short tail (1, 7), one 16-B unit (8), groups with
spare lanes (24, 72), a full group with spare units (520), eight units a lane (4096)."""
import numpy as np
import pytest

import psg
from row_adagrad_half_model import NEAREST, STOCHASTIC, RowAdagradHalfModel
from row_adagrad_model import RowAdagradModel
from row_model import BF16, F16, F32, POOL_MEAN, POOL_SUM, PULL, PUSH, SAME_LIST, SORTED, to_acc
from test_rows_adagrad_gpu import ALR, EPS, KEND, LR, dev, device, grads_for  # noqa: F401 (device: the fixture)

pytestmark = pytest.mark.gpu

SEED = (0xC0FFEE << 32) | 0x1234567
both = pytest.mark.parametrize("dtype", (F16, BF16), ids=("f16", "bf16"))
modes = pytest.mark.parametrize("rounding", (NEAREST, STOCHASTIC), ids=("nearest", "stochastic"))


def pair(dtype, rounding, width, alr=ALR, init_acc=0.0, init=None):
    t, m = psg.Table(dtype, width, 0, KEND, 0), RowAdagradHalfModel(dtype, width, key_end=KEND)
    if init:
        t.set_init(*init)
        assert m.set_init(*init) == {}
    t.set_adagrad_half(alr, EPS, init_acc, rounding, SEED)
    assert m.set_adagrad_half(alr, EPS, init_acc, rounding, SEED) == {}
    assert t.adagrad() == (alr, EPS, init_acc) and t.rounding() == (rounding, SEED)
    return t, m


def same(got, exp):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.itemsize == exp.itemsize
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.itemsize]
    np.testing.assert_array_equal(got.view(u).ravel(), exp.view(u).ravel())


def check(t, m):
    keys, rows = t.dump()
    np.testing.assert_array_equal(keys, m.keys)
    same(rows, m.rows)
    same(t.dump_accum(), m.acc)


def update(t, m, q, g, flags=PUSH | PULL, any_order=False, off=0):
    n, w = len(q), t.width
    (_, kp), (_, gp) = held = dev(q), dev(g, off)
    out = psg.DeviceBuffer(n * w * 4)
    (t.update_any if any_order else t.update)(flags, kp, gp, out if flags & PULL else None, n, LR, 0)
    exp = (m.update_any if any_order else m.update)(flags, q, g, LR, 0)
    if flags & PULL:
        same(out.download(np.float32, n * w), exp["out"])
    check(t, m)


def merged(t, m, lists, grads, path, off=0):
    kd, gd = [dev(q) for q in lists], [dev(g, off) for g in grads]
    outs = [psg.DeviceBuffer(len(q) * t.width * 4) for q in lists]
    got = t.update_merged(PUSH | PULL, [p for _, p in kd], [p for _, p in gd], outs, [len(q) for q in lists], LR, 1)
    exp = m.update_merged(PUSH | PULL, lists, grads, LR, 1)
    assert got == exp["path"] == path
    for out, q, e in zip(outs, lists, exp["outs"]):
        same(out.download(np.float32, len(q) * t.width), e)
    check(t, m)


@pytest.mark.parametrize("width", (1, 7, 8, 24, 72, 520, 4096))
@modes
@both
def test_every_update_call_matches_the_model(dtype, rounding, width):
    rng = np.random.default_rng(width)
    keys = np.sort(rng.choice(1 << 20, 330, replace=False).astype(np.uint64))
    known, n = keys[:300], 300
    t, m = pair(dtype, rounding, width)
    update(t, m, known, grads_for(rng, n, width), PUSH)
    update(t, m, known, grads_for(rng, n, width))  # its words come from the first step's accumulators
    # any order: one id named 9 times, ids the table does not hold among the rest
    q = rng.permutation(np.concatenate([known[:262], np.repeat(known[3], 8), keys[300:]]))
    update(t, m, q, grads_for(rng, n, width), any_order=True)
    merged(t, m, [known] * 3, [grads_for(rng, n, width) for _ in range(3)], SAME_LIST)
    lists = [known[5:130], rng.permutation(keys[120:]), np.concatenate([known[:7], known[:7]])]
    merged(t, m, lists, [grads_for(rng, len(x), width) for x in lists], SORTED)
    # bags: an ascending list (the strict path), then lists with repeats under weights and as means
    sizes = [0, 1, 7] + [3] * 97 + [1, 0]
    offsets, nb = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), len(sizes)
    some = [rng.choice(keys, n).astype(np.uint64) for _ in range(2)]
    for q, weights, mode in ((known, None, POOL_SUM), (some[0], rng.uniform(-2, 2, n).astype(np.float32), POOL_SUM),
                             (some[1], None, POOL_MEAN)):
        g = grads_for(rng, nb, width)
        held = dev(q), dev(offsets), dev(g), dev(np.zeros(1) if weights is None else weights)
        (_, kp), (_, op), (_, gp), (_, wp) = held
        if weights is None and mode == POOL_SUM:
            t.update_pooled(kp, op, gp, n, nb, LR, 0)
        else:
            t.update_pooled_weighted(kp, op, None if weights is None else wp, mode, gp, n, nb, LR, 0)
        path = SAME_LIST if q is known else SORTED
        assert m.update_pooled_weighted(q, offsets, g, LR, 0, weights, mode) == {"path": path}
        check(t, m)
    plain = rng.permutation(keys[:200])
    g0, g1 = grads_for(rng, nb, width), grads_for(rng, len(plain), width)
    held = [dev(q), dev(offsets), dev(g0), dev(plain), dev(g1)]
    frames = [(held[0][1], held[1][1], held[2][1]), (held[3][1], None, held[4][1])]
    assert t.update_pooled_merged(frames, [n, len(plain)], [nb, 0], LR, 2) == SORTED
    assert m.update_pooled_merged([(q, offsets, g0), (plain, None, g1)], LR, 2) == {"path": SORTED}
    check(t, m)
    t.close()


@pytest.mark.parametrize("width", (72, 520, 4096))
@both
def test_unaligned_gradients_and_initial_rows(dtype, width):
    """widths of whole units with the gradients 4 B off a 16-B boundary: the element path with 4, 16 and 64
    elements a lane, on a table with an initializer"""
    rng = np.random.default_rng(5)
    keys = np.sort(rng.choice(1 << 20, 300, replace=False).astype(np.uint64))
    t, m = pair(dtype, STOCHASTIC, width, init=(77, -0.5, 0.5))
    update(t, m, keys, grads_for(rng, 300, width), off=4)
    assert (m.rows != 0).all()
    merged(t, m, [keys] * 2, [grads_for(rng, 300, width) for _ in range(2)], SAME_LIST, off=4)
    lists = [keys[5:130], rng.permutation(keys[100:])]
    merged(t, m, lists, [grads_for(rng, len(x), width) for x in lists], SORTED, off=4)
    t.close()


@modes
@both
def test_special_rows(dtype, rounding):
    """a NaN gradient; a step past F16's range (learning_rate 1e5 on a one-hot row: step * g = 1e5 * sqrt(24));
    a step far below half an ulp of rows in [1, 2]; a -0.0 element under a zero gradient"""
    w, keys = 24, np.arange(10, 14, dtype=np.uint64)
    t, m = pair(dtype, rounding, w, alr=1e5, init_acc=1.0, init=(3, 1.0, 2.0))
    g = np.zeros((4, w), np.float32)
    g[0, 5], g[1, 2], g[2, :] = np.nan, 1e30, 1e-10
    update(t, m, keys, g)
    rows = to_acc(dtype, m.rows)
    assert np.isnan(rows[0]).all() and np.isinf(rows[1, 2]) == (dtype == F16) and np.isfinite(rows[2:]).all()
    z = np.zeros((1, w), np.uint16)
    z[0, 3] = 0x8000
    (_, kp), (_, zp) = held = dev(keys[3:]), dev(z)
    t.assign(kp, zp, 1)
    m.assign(keys[3:], z)
    g[3, 4] = 1.0
    update(t, m, keys[2:], g[2:])
    assert m.rows[3, 3] == 0x8000 and m.rows[3, 4] != 0
    t.close()


def test_accumulators_equal_an_f32_tables_and_stochastic_rows_move_where_nearest_rows_stay():
    rng = np.random.default_rng(9)
    w, keys = 24, np.sort(rng.choice(1 << 20, 300, replace=False).astype(np.uint64))
    ts, ms = pair(BF16, STOCHASTIC, w, init_acc=1.0, init=(11, 1.0, 2.0))
    tn, mn = pair(BF16, NEAREST, w, init_acc=1.0, init=(11, 1.0, 2.0))
    tf, mf = psg.Table(psg.F32, w, 0, KEND, 0), RowAdagradModel(F32, w, key_end=KEND)
    tf.set_adagrad(ALR, EPS, 1.0)
    assert mf.set_adagrad(ALR, EPS, 1.0) == {}
    # steps of 1.5e-3 at most: below half an ulp of a row in [1, 2] (2^-8) and of the binade beneath it (2^-9)
    g = grads_for(rng, 300, w) * np.float32(0.3)
    (_, kp), (_, gp) = held = dev(keys), dev(g)
    for _ in range(64):
        for t, m in ((ts, ms), (tn, mn), (tf, mf)):
            t.update(PUSH, kp, gp, None, 300, LR, 0)
            m.update(PUSH, keys, g, LR, 0)
    start = mn.initial(keys)
    for t, m in ((ts, ms), (tn, mn)):
        check(t, m)
        same(t.dump_accum(), tf.dump_accum())
    same(tf.dump_accum(), mf.acc)
    assert (mn.rows == start).all() and (ms.rows != start).any(axis=1).all()
    for t in (ts, tn, tf):
        t.close()
