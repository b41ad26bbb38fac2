"""psg_table_freeze_q8 and the psg_qtable_* calls (k_qrows_freeze, k_qrows_pool)
against the numpy model of their definition (row_q8_model), bit for bit.  48 rows
per table, among them a constant row, an all -0.0 row and, f32, a subnormal range,
a scale that underflows to 0 and +-1e38; the bag list is the 301 positions of
test_rows_pooled_wgrad_gpu.py."""
import functools

import numpy as np
import pytest

import psg
import row_model as rm
import row_q8_model as qm

pytestmark = pytest.mark.gpu

KEND = 1 << 40
INVALID, RANGE, UNSUPPORTED = 1, 4, 6
DTYPES = {"f32": psg.F32, "f16": psg.F16, "bf16": psg.BF16}
GRID = [("f32", w) for w in (1, 3, 4, 15, 16, 17, 260, 4095, 4096)] + \
       [(d, w) for d in ("f16", "bf16") for w in (3, 8, 264, 4096)]
grid = pytest.mark.parametrize("dtype,width", GRID, ids=[f"{d}-w{w}" for d, w in GRID])
PRESENT = np.arange(1000, 1048, dtype=np.uint64) * 7
ABSENT = np.arange(5, 13, dtype=np.uint64) * 1001
SIZES = [0, 0, 150, 3, 0, 40, 1, 4, 2, 0, 61, 5, 0, 35, 0]  # bag 7: absent ids only
dev = psg.DeviceBuffer.from_numpy


def source(dtype, width):
    """48 rows as the table stores them, and the same widened to f32"""
    x = np.random.default_rng(width).normal(0, 2, (len(PRESENT), width)).astype(np.float32)
    x[0], x[1] = 1.5, -0.0
    if dtype == psg.F32:
        for r, pat in ((2, [0, 3e-40, 1e-40]), (3, [0, 1e-44]), (4, [1e38, -1e38])):
            x[r] = np.resize(np.array(pat, np.float32), width)
    stored = rm.from_acc(dtype, x)
    return stored, rm.to_acc(dtype, stored)


@functools.lru_cache(maxsize=None)
def frozen(dtype, width):
    """table, its snapshot, and the model's codes, scale, bias and read-back rows"""
    psg.set_device(0)
    stored, x = source(DTYPES[dtype], width)
    t = psg.Table(DTYPES[dtype], width, 0, KEND, 0)
    t.assign(dev(PRESENT), dev(stored), len(PRESENT))
    before = [a.tobytes() for a in t.dump()]
    q = t.freeze_q8()
    assert [a.tobytes() for a in t.dump()] == before, "the freeze changed its source"
    c, s, b = qm.quantise(x)
    return t, q, (c, s, b), qm.dequantise(c, s, b)


def exported(q, width, count):
    k, r = psg.DeviceBuffer(8 * count), psg.DeviceBuffer(count * (width + 8))
    q.export(0, count, k, r)
    psg.device_sync()
    return k.download(np.uint64, count), r.download(np.uint8, count * (width + 8)).reshape(count, width + 8)


def looked_up(q, width, ids):
    n = len(ids)
    out, found = dev(np.full(n * width + 4, -7.0, np.float32)), dev(np.full(n + 4, 9, np.uint8))
    q.lookup(dev(ids), out, found, n)
    assert (out.download(np.float32, 4, offset=4 * n * width) == -7.0).all(), "wrote behind out"
    assert (found.download(np.uint8, 4, offset=n) == 9).all(), "wrote behind found"
    return out.download(np.float32, n * width).reshape(n, width), found.download(np.uint8, n)


def shuffled_ids():
    ids = np.random.default_rng(4).choice(np.concatenate([PRESENT, ABSENT]), 133)
    assert 0 < np.isin(ids, ABSENT).sum() < 133 and len(np.unique(ids)) < 133
    return ids


def same(got, exp):
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))


@grid
def test_freeze_then_export_is_the_model(dtype, width):
    _, q, (c, s, b), _ = frozen(dtype, width)
    keys, rows = exported(q, width, len(PRESENT))
    np.testing.assert_array_equal(keys, PRESENT)
    np.testing.assert_array_equal(rows, qm.packed(c, s, b))
    if dtype == "f32" and width > 1:
        assert s[1] == 0 and s[3] == 0 and 0 < s[2] < 1e-38 and np.isfinite(s[4]), "the special rows are what they claim"
    i = q.info()
    assert (i.width, i.row_bytes, i.size, i.key_begin, i.key_end) == (width, width + 8, len(PRESENT), 0, KEND)
    assert i.device_bytes >= len(PRESENT) * (8 + width + 8)


@grid
def test_lookup_is_the_model(dtype, width):
    _, q, _, xhat = frozen(dtype, width)
    ids = shuffled_ids()
    rows, found = looked_up(q, width, ids)
    exp_rows, exp_found = qm.lookup(PRESENT, xhat, ids)
    same(rows, exp_rows)
    np.testing.assert_array_equal(found, exp_found)


@pytest.mark.parametrize("off", [0, 4], ids=["aligned", "off4"])
@grid
def test_pooled_lookup_is_an_f32_table_of_the_read_back_rows(dtype, width, off):
    _, q, _, xhat = frozen(dtype, width)
    rng = np.random.default_rng(11)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
    # row 4 (+-1e38) stays out of the bags: its sums overflow, and which NaN inf - inf gives is the machine's
    ids = rng.choice(np.concatenate([np.delete(PRESENT, 4), ABSENT[:4]]), int(offsets[-1]))
    ids[int(offsets[7]):int(offsets[8])] = ABSENT[4:]
    weights = rng.uniform(-2, 2, len(ids)).astype(np.float32)
    nb = len(SIZES)
    for w, mode in ((None, psg.POOL_SUM), (weights, psg.POOL_SUM), (None, psg.POOL_MEAN)):
        out = dev(np.full(nb * width + 8, -7.0, np.float32))  # out starts `off` bytes behind a 16-B boundary
        q.lookup_pooled(dev(ids), dev(offsets), None if w is None else dev(w), mode, out.ptr + off, len(ids), nb)
        assert (out.download(np.float32, 3, offset=off + 4 * nb * width) == -7.0).all(), "wrote behind out"
        got = out.download(np.float32, nb * width, offset=off).reshape(nb, width)
        same(got, qm.pooled(PRESENT, xhat, ids, offsets, w, mode))
        assert (got[[0, 7, 14]].view(np.uint32) == 0).all(), "an empty bag and a bag of absent ids are +0.0"


@grid
def test_from_rows_of_the_export_answers_alike(dtype, width):
    _, q, _, _ = frozen(dtype, width)
    keys, rows = exported(q, width, len(PRESENT))
    q2 = psg.QTable.from_rows(width, 0, KEND, dev(keys), dev(rows), len(keys))
    ids = shuffled_ids()
    for a, b in zip(looked_up(q2, width, ids), looked_up(q, width, ids)):
        assert a.tobytes() == b.tobytes()
    k2, r2 = exported(q2, width, len(keys))
    assert k2.tobytes() == keys.tobytes() and r2.tobytes() == rows.tobytes()
    for bad, code in ((keys[::-1].copy(), INVALID), (np.append(keys[:-1], np.uint64(KEND)), RANGE)):
        with pytest.raises(psg.PsgError) as e:
            psg.QTable.from_rows(width, 0, KEND, dev(bad), dev(rows), len(keys))
        assert e.value.code == code


@pytest.mark.parametrize("dtype,width", [("f32", 17), ("f32", 260), ("bf16", 264)])
@pytest.mark.parametrize("bad", [[np.nan], [np.inf], [-3e38, 3e38]], ids=["nan", "inf", "range"])
def test_a_row_the_definition_refuses_fails_the_freeze(dtype, width, bad):
    if dtype != "f32" and len(bad) == 2:
        bad = [-3.38e38, 3.38e38]  # finite in bf16, their difference not in f32
    stored, _ = source(DTYPES[dtype], width)
    t = psg.Table(DTYPES[dtype], width, 0, KEND, 0)
    t.assign(dev(PRESENT), dev(stored), len(PRESENT))
    row = rm.to_acc(DTYPES[dtype], stored[40]).copy()
    row[-len(bad):] = bad
    t.assign(dev(PRESENT[40:41]), dev(rm.from_acc(DTYPES[dtype], row)), 1)
    with pytest.raises(psg.PsgError) as e:
        t.freeze_q8()
    assert e.value.code == INVALID
    t.assign(dev(PRESENT[40:41]), dev(stored[40]), 1)  # the row overwritten: the same table freezes
    assert exported(t.freeze_q8(), width, 48)[1].tobytes() == exported(frozen(dtype, width)[1], width, 48)[1].tobytes()


def test_edges():
    psg.set_device(0)
    q = psg.Table(psg.F32, 5, 0, KEND, 0).freeze_q8()  # an empty table: size 0, every id absent
    assert q.info().size == 0
    rows, found = looked_up(q, 5, PRESENT[:3].copy())
    assert (rows.view(np.uint32) == 0).all() and (found == 0).all()
    with pytest.raises(psg.PsgError) as e:
        psg.Table(psg.F64, 5, 0, KEND, 0).freeze_q8()
    assert e.value.code == UNSUPPORTED
    _, q, _, _ = frozen("f32", 16)
    ids, offsets = PRESENT[:6].copy(), np.array([0, 2, 6], np.uint64)
    out_of_range, bad_offsets = np.append(ids[:5], np.uint64(KEND)), np.array([0, 4, 3], np.uint64)
    for kk, oo, code in ((ids, bad_offsets, INVALID), (out_of_range, offsets, RANGE), (out_of_range, bad_offsets, INVALID)):
        out = dev(np.full(2 * 16, -7.0, np.float32))
        with pytest.raises(psg.PsgError) as e:
            q.lookup_pooled(dev(kk), dev(oo), None, psg.POOL_SUM, out, 6, 2)
        assert e.value.code == code and (out.download(np.float32, 32) == -7.0).all()
    out = dev(np.full(6 * 16, -7.0, np.float32))
    with pytest.raises(psg.PsgError) as e:
        q.lookup(dev(out_of_range), out, None, 6)
    assert e.value.code == RANGE and (out.download(np.float32, 96) == -7.0).all()
