"""psg_table_lookup_pooled_batch (k_batch_front, k_batch_pool) against a numpy
model of the per-table definition in its acc_t and arrival order, bit for bit; the
same expected bytes must also be what psg_table_lookup_pooled_weighted returns for
the entry on its own.  Tables hold 48 rows (test_qrows_gpu.py's) plus absent ids.

The T = 6 call: widths 1 / 17 / 260 / 4096 (halves 3 / 8 / 264 / 4096), a table
of size 0 under 7 ids directly in front of 2300 ids in 40 bags (entries of 1 and 3
resolve tiles), a table with an initializer, one table in two entries (its second
the entry with nb = 0; two entries with different lists AND modes on one table are
in the T = 5 refusal call), a reply 8 B off a 16-B boundary (element units on a
16-B row)."""
import ctypes as C
import functools

import numpy as np
import pytest

import psg
import row_init_model as im
import row_model as rm

pytestmark = pytest.mark.gpu

KEND = 1 << 40
OK, INVALID, RANGE = 0, 1, 4
SUM, MEAN = psg.POOL_SUM, psg.POOL_MEAN
DTYPES = {"f32": psg.F32, "f64": psg.F64, "f16": psg.F16, "bf16": psg.BF16}
dtypes = pytest.mark.parametrize("dtype", list(DTYPES))
PRESENT = np.arange(1000, 1048, dtype=np.uint64) * 7
ABSENT = np.arange(5, 13, dtype=np.uint64) * 1001
SIZES = [0, 0, 150, 3, 0, 40, 1, 4, 2, 0, 61, 5, 0, 35, 0]  # bag 7: absent ids only
INIT = (77, -0.5, 1.5)
SENTINEL = 0xA5
dev = psg.DeviceBuffer.from_numpy


def widths(dtype):
    return (3, 8, 264, 4096) if dtype in ("f16", "bf16") else (1, 17, 260, 4096)


@functools.lru_cache(maxsize=None)
def table(dtype, width, kind="rows"):
    """(Table, its 48 stored rows or None for the table of size 0, its initializer or None)"""
    psg.set_device(0)
    dt = DTYPES[dtype]
    t = psg.Table(dt, width, 0, KEND, 0)
    if kind == "init":
        t.set_init(*INIT)
    if kind == "empty":
        return t, None, None
    x = np.random.default_rng(width).normal(0, 2, (len(PRESENT), width))
    stored = np.ascontiguousarray(rm.from_acc(dt, x.astype(np.float64 if dt == psg.F64 else np.float32)))
    t.assign(dev(PRESENT), dev(stored), len(PRESENT))
    return t, stored, INIT if kind == "init" else None


def bag_list(seed, sizes, weighted):
    """ids (present, absent and repeated ones; bag 7 of SIZES absent only), offsets, weights or None"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ids = rng.choice(np.concatenate([PRESENT, ABSENT[:4]]), int(offsets[-1]))
    if len(sizes) == len(SIZES):
        ids[int(offsets[7]):int(offsets[8])] = ABSENT[4:]
    assert len(ids) < 8 or (0 < np.isin(ids, ABSENT).sum() < len(ids) and len(np.unique(ids)) < len(ids))
    return ids, offsets, rng.uniform(-2, 2, len(ids)).astype(np.float32) if weighted else None


def expected(dtype, stored, init, width, ids, offsets, weights, mode):
    """the definition: acc_t, arrival order, one multiply then one add, one division, one rounding"""
    dt = DTYPES[dtype]
    acc_t = np.float64 if dt == psg.F64 else np.float32
    rows, found = np.zeros((len(ids), width), acc_t), np.zeros(len(ids), bool)
    if stored is not None:
        at = np.minimum(np.searchsorted(PRESENT, ids), len(PRESENT) - 1)
        found = PRESENT[at] == ids
        rows[found] = rm.to_acc(dt, stored)[at[found]]
    if init is not None:
        rows[~found] = rm.to_acc(dt, im.init_rows(ids[~found], dt, width, *init))
        found[:] = True
    if weights is not None:
        rows = weights.astype(acc_t)[:, None] * rows
    out = np.zeros((len(offsets) - 1, width), acc_t)
    for b in range(len(out)):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        for p in range(lo, hi):
            if found[p]:
                out[b] = out[b] + rows[p]
        if mode == MEAN and hi > lo:
            out[b] = out[b] / acc_t(hi - lo)
    assert out.dtype == acc_t
    return np.ascontiguousarray(rm.from_acc(dt, out))


class Entry:
    """one request: its device arrays, a reply filled with the sentinel (16 B more behind it), the expected bytes"""

    def __init__(self, dtype, tab, ids, offsets, weights, mode, off=0):
        self.t, stored, init = tab
        self.n, self.nb, self.mode, width = len(ids), len(offsets) - 1, mode, self.t.width
        self.keys, self.offsets = dev(ids), dev(offsets)
        self.weights = None if weights is None else dev(weights)
        self.exp = expected(dtype, stored, init, width, ids, offsets, weights, mode).tobytes() if self.nb else b""
        self.off = off
        self.fresh()

    def fresh(self):
        self.out = dev(np.full(self.off + len(self.exp) + 16, SENTINEL, np.uint8))
        return self.out.ptr + self.off

    def reply(self):
        got = self.out.download(np.uint8, self.off + len(self.exp) + 16).tobytes()
        assert set(got[:self.off] + got[self.off + len(self.exp):]) == {SENTINEL}, "wrote outside out"
        return got[self.off:self.off + len(self.exp)]

    def untouched(self):
        return set(self.reply()) <= {SENTINEL}

    def alone(self):
        """the per-table call on this entry"""
        self.t.lookup_pooled_weighted(self.keys, self.offsets, self.weights, self.mode, self.fresh(), self.n, self.nb)
        return self.reply()


def batch(entries):
    """the C call: (return code, statuses)"""
    T = len(entries)
    ptrs = lambda xs: (C.c_void_p * T)(*xs)
    status = (C.c_int * T)(*[9] * T)
    rc = psg.lib().psg_table_lookup_pooled_batch(
        T, ptrs([e.t.h.value for e in entries]), ptrs([e.keys.ptr for e in entries]),
        ptrs([e.offsets.ptr for e in entries]), ptrs([None if e.weights is None else e.weights.ptr for e in entries]),
        (C.c_int * T)(*[e.mode for e in entries]), ptrs([e.fresh() for e in entries]),
        (C.c_uint64 * T)(*[e.n for e in entries]), (C.c_uint64 * T)(*[e.nb for e in entries]), None, status)
    return rc, list(status)


def state(tables):
    return [(bytes(t.info()), [a.tobytes() for a in t.dump()]) for t in tables]


@dtypes
@pytest.mark.parametrize("weighted,mode", [(False, SUM), (True, SUM), (False, MEAN)], ids=["sum", "weighted", "mean"])
def test_one_entry_is_the_per_table_call(dtype, weighted, mode):
    e = Entry(dtype, table(dtype, widths(dtype)[1]), *bag_list(11, SIZES, weighted), mode)
    status = psg.lookup_pooled_batch([e.t], [e.keys], [e.offsets], [e.weights] if weighted else None, [mode],
                                     [e.fresh()], [e.n], [e.nb])
    got = e.reply()
    assert status == [OK] and got == e.exp and e.alone() == e.exp
    rb = len(got) // e.nb
    zero = [b for b in range(e.nb) if not any(got[b * rb:(b + 1) * rb])]
    assert zero == [0, 1, 4, 7, 9, 12, 14], "only the empty bags and the bag of absent ids are +0"


@dtypes
def test_six_entries_in_one_call(dtype):
    w0, w1, w2, w3 = widths(dtype)
    small, forty = [3, 0, 4], list(np.random.default_rng(5).multinomial(2300, [1 / 40] * 40))
    assert sum(small) == 7 and sum(forty) == 2300 and len(forty) == 40
    entries = [
        Entry(dtype, table(dtype, w1, "empty"), *bag_list(1, small, False), SUM),  # 7 ids, all absent: +0
        Entry(dtype, table(dtype, w2), *bag_list(2, forty, True), SUM, off=8),  # tiles 1 | 3; element units
        Entry(dtype, table(dtype, w0), *bag_list(3, SIZES, False), MEAN),
        Entry(dtype, table(dtype, w3), *bag_list(4, SIZES, False), SUM),  # two bags a pooling tile
        Entry(dtype, table(dtype, w1, "init"), *bag_list(6, SIZES, True), SUM),
        Entry(dtype, table(dtype, w0), np.zeros(0, np.uint64), np.zeros(1, np.uint64), None, SUM),  # nb = 0
    ]
    tables = [e.t for e in entries]
    before = state(tables)
    rc, status = batch(entries)
    assert (rc, status) == (OK, [OK] * 6)
    for i, e in enumerate(entries):
        assert e.reply() == e.exp, "entry %d differs from the definition" % i
        assert any(e.exp) == (i not in (0, 5)), "entry %d: only the empty table's reply is all +0" % i
    assert state(tables) == before, "a table, or a device pointer of its info, moved"
    for i, e in enumerate(entries[:5]):
        assert e.alone() == e.exp, "entry %d: the per-table call differs from the definition" % i


@dtypes
def test_refused_entries_are_left_out_and_the_rest_served(dtype):
    w0, w1, _, _ = widths(dtype)
    ids, offsets, weights = bag_list(8, SIZES, True)
    short = offsets.copy()
    short[-1] -= 1  # offsets[nb] != n
    outside = ids.copy()
    outside[200] = KEND
    entries = [
        Entry(dtype, table(dtype, w0), ids, offsets, weights, SUM),
        Entry(dtype, table(dtype, w1), ids, short, None, SUM),
        Entry(dtype, table(dtype, w0), *bag_list(9, SIZES, False), MEAN),  # entry 0's table, another list and mode
        Entry(dtype, table(dtype, w1), outside, offsets, None, SUM),
        Entry(dtype, table(dtype, w1, "init"), outside, short, None, MEAN),
    ]
    rc, status = batch(entries)
    assert (rc, status) == (INVALID, [OK, INVALID, OK, RANGE, INVALID])
    assert all(entries[i].untouched() for i in (1, 3, 4)), "a refused entry's out was written"
    assert all(entries[i].reply() == entries[i].exp and any(entries[i].exp) for i in (0, 2))
