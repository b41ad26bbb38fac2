"""The numpy restatement of the initial rows (tests/row_init_model.py) against
what it must agree with: the Random123 known answers of Philox4x32-10, the
definition in include/psg.h, and the properties the feature is built for (a row
depends on seed, key and column alone).  No GPU is used: these cases pin the
mirror, not the device code, which test_rows_init_gpu.py checks against it.
"""
import numpy as np
import pytest

import row_init_model as rim
import row_model as rm
from row_init_model import F32, F64, F16, BF16, RowInitModel, init_rows
from row_model import PUSH, PULL, Refused

KEND = 1 << 40
SEED = 0x1234_5678_9ABC_DEF0

# counter words, key words, output words (Random123's kat_vectors, philox4x32 10)
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("ctr,key,out", KNOWN, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, out):
    got = rim.philox4x32_10(np.array(ctr, np.uint64), key)
    assert [int(x) for x in got] == list(out)
    # the same through a batch, beside other counters
    batch = np.array([KNOWN[0][0], ctr, KNOWN[2][0]], np.uint64)
    assert [int(x) for x in rim.philox4x32_10(batch, key)[1]] == list(out)


def test_known_answers_through_init_words():
    """key 0 and seed 0, width 4: block 0 is the first known answer; the third one
    through its key, seed and block as the definition lays them into the counter"""
    assert [int(x) for x in rim.init_words([0], 4, 0)[0]] == list(KNOWN[0][2])
    ctr, key, _ = KNOWN[2]
    k, seed = ctr[0] | (ctr[1] << 32), key[0] | (key[1] << 32)
    x = rim.init_words([k], 4, seed)[0]
    assert [int(v) for v in x] == [int(v) for v in rim.philox4x32_10(np.array([ctr[0], ctr[1], 0, 0], np.uint64), key)]


def test_unit_interval():
    x = np.array([0, 0xFF, 0x100, 0xFFFFFFFF, 0x80000000], np.uint32)
    u = rim.unit_interval(x)
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]
    rng = np.random.default_rng(0)
    u = rim.unit_interval(rim.init_words(rng.integers(0, 1 << 63, 4000, dtype=np.uint64), 7, SEED))
    assert u.min() >= 0.0 and u.max() < 1.0
    assert 0.45 < u.mean() < 0.55 and u.min() < 0.01 and u.max() > 0.99


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16])
def test_range_and_constant_rows(dtype):
    keys = np.arange(0, 3000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    r = rm.to_acc(dtype, init_rows(keys, dtype, 6, SEED, -0.05, 0.05)).astype(np.float64)
    assert r.min() >= -0.05 - 1e-3 and r.max() <= 0.05 + 1e-3 and r.std() > 0.02
    if dtype in (F32, F64):  # in [lo, hi] of the f32 bounds, hi included
        assert r.min() >= float(np.float32(-0.05)) and r.max() <= float(np.float32(0.05))
    c = init_rows(keys, dtype, 6, SEED, 0.25, 0.25)  # lo == hi
    assert np.all(rm.to_acc(dtype, c) == 0.25)
    z = init_rows(keys[:5], dtype, 6, SEED, 0.0, 0.0)
    assert not bits(z).any()


def test_width_five_uses_block_one_word_zero():
    keys = rm.u64([0, 7, (1 << 32) + 7, (1 << 64) - 1])
    x = rim.init_words(keys, 5, SEED)
    for i, k in enumerate(int(v) for v in keys):
        lo, hi = k & 0xFFFFFFFF, k >> 32
        key = (SEED & 0xFFFFFFFF, SEED >> 32)
        b0 = rim.philox4x32_10(np.array([lo, hi, 0, 0], np.uint64), key)
        b1 = rim.philox4x32_10(np.array([lo, hi, 1, 0], np.uint64), key)
        assert x[i].tolist() == b0.tolist() + [int(b1[0])]
    # a row's width beyond the column does not matter
    same(init_rows(keys, F32, 5, SEED, -1, 1), init_rows(keys, F32, 12, SEED, -1, 1)[:, :5])


def test_high_words_of_key_and_seed_matter():
    k = rm.u64([5, 5 + (1 << 32)])
    r = init_rows(k, F32, 8, SEED, -1, 1)
    assert not np.any(r[0] == r[1])
    a = init_rows(k[:1], F32, 8, 7, -1, 1)
    b = init_rows(k[:1], F32, 8, 7 + (1 << 32), -1, 1)
    assert not np.any(a == b)


def test_halves_round_to_nearest_even_once():
    keys = np.arange(500, dtype=np.uint64)
    v = init_rows(keys, F32, 4, SEED, -0.5, 0.5)
    same(init_rows(keys, F16, 4, SEED, -0.5, 0.5), v.astype(np.float16))
    bf = init_rows(keys, BF16, 4, SEED, -0.5, 0.5)
    back = (bf.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert np.all(np.abs(back - v) <= np.abs(v) * 2.0 ** -8)
    same(init_rows(keys, F64, 4, SEED, -0.5, 0.5), v.astype(np.float64))


def test_set_init_refusals():
    m = RowInitModel(F32, 4, 0, KEND)
    for bad in ((2, 1, 0.0, 1.0), (1, 1, np.nan, 1.0), (1, 1, 0.0, np.inf), (1, 1, 1.0, 0.5),
                (1, 1, -3e38, 3e38)):
        r = m.set_init(bad[1], bad[2], bad[3], kind=bad[0])
        assert isinstance(r, Refused) and r.code == rm.INVALID, bad
    assert m.set_init(1, 0.5, 0.5) == {}
    assert isinstance(m.set_init(1, 0.0, 1.0), Refused)  # a second call


def random_keys(rng, n):
    return np.unique(rng.integers(0, KEND, 2 * n, dtype=np.uint64))[:n]


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_dump_is_independent_of_insertion_order_and_grouping(adam):
    rng = np.random.default_rng(3)
    keys = random_keys(rng, 900)

    def fresh():
        m = RowInitModel(F32, 5, 0, KEND)
        m.set_init(SEED, -0.1, 0.1)
        if adam:
            m.set_adam(*rm.ADAM)
        return m

    a, b, c = fresh(), fresh(), fresh()
    a.handle(PULL, keys)
    for part in np.array_split(rng.permutation(keys), 30):
        b.handle_any(PULL, np.concatenate([part, part[:3]]))
    c.assign(keys[::2])
    c.handle_any(PULL, rng.permutation(keys))
    for x in (b, c):
        np.testing.assert_array_equal(a.keys, x.keys)
        same(a.rows, x.rows)
    same(a.rows, init_rows(keys, F32, 5, SEED, -0.1, 0.1))
    assert not a.m.any() and not a.v.any()  # the moments of a new row stay zero
    # an update starts from the initial row
    g = rm.grads(rng, 10 * 5)
    a.update(PUSH, keys[:10], g, rm.LR, 0)
    d = fresh()
    d.update(PUSH, keys[:10], g, rm.LR, 0)
    same(a.rows[:10], d.rows)
    # an erased key that is named again is its initial row again
    a.erase(keys[:10])
    a.handle(PULL, keys[:10])
    same(a.rows, b.rows)


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16])
def test_lookup_is_the_pull_that_follows(dtype):
    rng = np.random.default_rng(4)
    keys = random_keys(rng, 400)
    m = RowInitModel(dtype, 3, 0, KEND)
    m.set_init(SEED, -1.0, 1.0)
    m.handle(PUSH, keys[:200], rm.values(rng, dtype, 200 * 3))
    q = rng.choice(keys, 300)
    size = m.size
    r = m.lookup(q)
    assert m.size == size
    present = np.isin(q, keys[:200])
    np.testing.assert_array_equal(r["found"], present.astype(np.uint8))
    assert (~present).sum() > 50
    same(r["out"], m.handle_any(PULL, q)["out"])
    assert m.size > size


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16])
@pytest.mark.parametrize("L", [1, 2, 4, 8])
def test_mean_of_an_absent_bag_is_the_weighted_sum_with_one_over_L(dtype, L):
    """1 / L is a power of two: w * x and x / L round alike, and the sums that
    follow see the same addends in another order of operations only where the
    scaling is exact, which it is short of underflow"""
    rng = np.random.default_rng(5)
    m = RowInitModel(dtype, 5, 0, KEND)
    m.set_init(SEED, -1.0, 1.0)
    nb = 40
    q = random_keys(rng, nb * L)
    offsets = np.arange(nb + 1, dtype=np.uint64) * np.uint64(L)
    assert m.size == 0
    mean = m.lookup_pooled_weighted(q, offsets, None, rm.POOL_MEAN)["out"]
    if L == 1:
        same(mean, init_rows(q, dtype, 5, SEED, -1.0, 1.0))
    weighted = m.lookup_pooled_weighted(q, offsets, np.full(nb * L, 1.0 / L, np.float32))["out"]
    same(mean, weighted)
    assert m.size == 0  # nothing was inserted
    assert bits(mean).any()
    # without an initializer the same bags are rows of +0
    z = rm.RowModel(dtype, 5, 0, KEND).lookup_pooled_weighted(q, offsets, None, rm.POOL_MEAN)["out"]
    assert not bits(z).any()


def test_pooled_lookup_mixes_present_and_absent_ids():
    rng = np.random.default_rng(6)
    keys = random_keys(rng, 300)
    m = RowInitModel(F32, 4, 0, KEND)
    m.set_init(SEED, -1.0, 1.0)
    m.handle(PUSH, keys[:150], rm.values(rng, F32, 150 * 4))
    q = rng.choice(keys, 500)
    offsets = np.concatenate([[0, 0], np.sort(rng.integers(0, 501, 98)), [500, 500]]).astype(np.uint64)
    w = rng.uniform(-2, 2, 500).astype(np.float32)
    got = m.lookup_pooled_weighted(q, offsets, w)["out"]
    assert m.size == 150
    rows = m.lookup(q)["out"]  # present rows and initial rows, as bytes
    exp = np.zeros((len(offsets) - 1, 4), np.float32)
    for b in range(len(offsets) - 1):
        for p in range(int(offsets[b]), int(offsets[b + 1])):
            exp[b] = exp[b] + w[p] * rows[p]
    same(got, exp)
