"""The row-valued HBM table (psg_table_*, csrc/psg_rows.hip) against the oracle.

The checker is the existing scalar oracle.Store fed expanded keys: the distinct
keys of a test are mapped to ranks (np.unique) and a row request on keys k_i is
replayed as the scalar request on keys rank(k_i) * W + j, row-major — exactly
the reference loop (KVApp.h:446-454) per element, in arrival order.  Every
comparison is bit for bit.
"""
import numpy as np
import pytest

import oracle
import psg

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1
NPT = {psg.F32: np.float32, psg.F64: np.float64, psg.F16: np.uint16, psg.BF16: np.uint16}
ES = {psg.F32: 4, psg.F64: 8, psg.F16: 2, psg.BF16: 2}
BITS = {4: np.uint32, 8: np.uint64, 2: np.uint16}


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def dev(a):
    return psg.DeviceBuffer.from_numpy(a)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype.itemsize])


def same(got, exp):
    np.testing.assert_array_equal(bits(got), bits(exp))


def synth(n, dtype, seed):
    """real-valued data for F32 / F64, integer-valued for the halves (as test_gpu_parity)."""
    if dtype in (psg.F32, psg.F64):
        return oracle.synth(n, dtype, seed, 1, -1.0, 1.0)
    return oracle.synth(n, dtype, seed, 0, 0.0, 1000.0)


def random_keys(rng, n, lo=0, hi=1 << 63):
    u = np.unique(rng.integers(lo, hi, 2 * n + 16, dtype=np.uint64))
    return np.sort(rng.choice(u, n, replace=False))


class RowOracle:
    """oracle.Store on expanded scalar keys rank * W + j."""

    def __init__(self, dtype, width, all_keys):
        self.w = width
        self.u = np.unique(np.asarray(all_keys, dtype=np.uint64))
        self.st = oracle.Store(dtype)
        oracle.lib().oracle_store_reserve(self.st.h, len(self.u) * width)

    def handle(self, flags, keys, vals=None):
        keys = np.asarray(keys, dtype=np.uint64)
        ranks = np.searchsorted(self.u, keys)
        assert np.array_equal(self.u[ranks], keys)
        ek = (ranks[:, None].astype(np.uint64) * np.uint64(self.w) + np.arange(self.w, dtype=np.uint64)).ravel()
        return self.st.handle(flags, ek, vals, len(ek))

    def dump(self):
        k, v = self.st.dump()
        return self.u[(k[::self.w] // np.uint64(self.w)).astype(np.int64)], v.reshape(-1, self.w)


class Rig:
    """A table and its oracle, fed the same requests."""

    def __init__(self, dtype, width, all_keys, key_begin=0, key_end=KMAX, capacity=0):
        self.dtype, self.w = dtype, width
        self.t = psg.Table(dtype, width, key_begin, key_end, capacity)
        self.o = RowOracle(dtype, width, all_keys)

    def request(self, flags, keys, vals=None):
        """the request on both; compares the Pull's reply; returns it"""
        n = len(keys)
        dk = dev(np.asarray(keys, dtype=np.uint64))
        dv = dev(vals) if flags & psg.PUSH else None
        out = psg.DeviceBuffer(max(n * self.w * ES[self.dtype], 1)) if flags & psg.PULL else None
        self.t.handle(flags, dk, dv, out, n)
        exp = self.o.handle(flags, keys, vals)
        if not flags & psg.PULL:
            return None
        got = out.download(NPT[self.dtype], n * self.w)
        same(got, exp)
        return got

    def check_dump(self):
        k, rows = self.t.dump()
        ok, orows = self.o.dump()
        np.testing.assert_array_equal(k, ok)
        same(rows, orows)
        assert self.t.info().size == len(ok)


GRID = [(psg.F32, w, n) for w in (1, 3, 4, 20, 64, 260) for n in (1, 65, 4097, 20011)]
GRID += [(dt, w, 4097) for dt in (psg.F64, psg.F16, psg.BF16) for w in (3, 20)]


@pytest.mark.parametrize("dtype,width,n", GRID)
def test_push_pushpull_pull_vs_oracle(dtype, width, n):
    """W = 3: element-wise rows; 4: one vector; 20: 16-B rows, no power of two;
    260: a row longer than one wave's pass; n up to several blocks and tiles."""
    rng = np.random.default_rng(width * 100003 + n)
    keys = random_keys(rng, n)
    rig = Rig(dtype, width, keys)
    v1, v2 = synth(n * width, dtype, 11), synth(n * width, dtype, 12)
    rig.request(psg.PUSH, keys, v1)
    got = rig.request(psg.PUSH | psg.PULL, keys, v2)
    pulled = rig.request(psg.PULL, keys)
    same(pulled, got)
    rig.check_dump()
    if width == 1:
        # the same requests on a scalar SORTED store
        st = psg.Store(psg.SORTED, dtype, 0, KMAX, 0)
        dk, out = dev(keys), psg.DeviceBuffer(n * ES[dtype])
        st.handle(psg.PUSH, dk, dev(v1), None, n)
        st.handle(psg.PUSH | psg.PULL, dk, dev(v2), out, n)
        same(out.download(NPT[dtype], n), got)
        st.handle(psg.PULL, dk, None, out, n)
        same(out.download(NPT[dtype], n), pulled)


@pytest.mark.parametrize("width", [3, 20])
def test_insert_moves_rows(width):
    rng = np.random.default_rng(width)
    n = 1500
    a = random_keys(rng, n, 1 << 20, 1 << 40)
    # b: every other key of a, and new keys before, between and after a's
    new = np.concatenate([random_keys(rng, 200, 0, 1 << 20), random_keys(rng, n, 1 << 20, 1 << 40),
                          random_keys(rng, 200, 1 << 40, 1 << 41)])
    new = np.setdiff1d(new, a)
    b = np.union1d(a[::2], new)
    absent = np.setdiff1d(random_keys(rng, 300, 0, 1 << 41), np.union1d(a, b))
    c = np.union1d(absent, a[1::3])  # a Pull holding absent keys among present ones
    rig = Rig(psg.F32, width, np.concatenate([a, b, c]))
    rig.request(psg.PUSH, a, synth(len(a) * width, psg.F32, 1))
    cap_a = rig.t.info().capacity
    assert rig.t.info().size == len(a)
    rig.request(psg.PUSH, b, synth(len(b) * width, psg.F32, 2))
    assert rig.t.info().size == len(np.union1d(a, b)) and rig.t.info().capacity > cap_a  # merged and grown
    rig.request(psg.PULL, np.union1d(a, b))
    before = rig.t.info().size
    got = rig.request(psg.PULL, c).reshape(len(c), width)
    assert not np.any(bits(got[np.isin(c, absent)])), "absent keys answer zero rows"
    assert rig.t.info().size == before + len(absent)
    rig.check_dump()


@pytest.mark.parametrize("width", [3, 4])
def test_sparse_subsets_leave_other_rows_alone(width):
    rng = np.random.default_rng(50 + width)
    n = 50000
    keys = random_keys(rng, n)
    rig = Rig(psg.F32, width, keys)
    rig.request(psg.PUSH, keys, synth(n * width, psg.F32, 3))
    _, base = rig.t.dump()
    touched = np.zeros(n, bool)
    for seed, idx in ((4, np.arange(0, n, 7)), (5, np.sort(rng.choice(n, n // 10, replace=False)))):
        sub = keys[idx]
        rig.request(psg.PUSH | psg.PULL, sub, synth(len(sub) * width, psg.F32, seed))
        rig.request(psg.PULL, sub)
        touched[idx] = True
    _, rows = rig.t.dump()
    same(rows[~touched], base[~touched])
    rig.check_dump()


def test_key_extremes():
    keys = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 2], dtype=np.uint64)
    rig = Rig(psg.F32, 4, keys, 0, KMAX)
    rig.request(psg.PUSH, keys, synth(len(keys) * 4, psg.F32, 6))
    rig.request(psg.PUSH | psg.PULL, keys, synth(len(keys) * 4, psg.F32, 7))
    rig.request(psg.PULL, keys[[0, 2, 4]])
    rig.check_dump()


def test_table_over_a_narrow_range():
    keys = np.array([1000, 1001, 1500, 1999], dtype=np.uint64)
    rig = Rig(psg.F32, 3, keys, 1000, 2000)
    rig.request(psg.PUSH | psg.PULL, keys, synth(len(keys) * 3, psg.F32, 8))
    rig.request(psg.PULL, keys[[0, 3]])
    for bad in ([999, 1000], [1999, 2000]):
        with pytest.raises(psg.PsgError) as ei:
            rig.t.handle(psg.PULL, dev(np.array(bad, dtype=np.uint64)), None, psg.DeviceBuffer(64), 2)
        assert ei.value.code == 4
    rig.check_dump()


@pytest.mark.parametrize("flags", [psg.PUSH, psg.PUSH | psg.PULL, psg.PULL])
def test_rejected_requests_leave_the_table_unchanged(flags):
    width, end = 20, 1 << 30
    rng = np.random.default_rng(9)
    keys = random_keys(rng, 3000, 0, end - 1)
    fresh = np.setdiff1d(random_keys(rng, 500, 0, end - 1), keys)  # absent keys a bad list also holds
    rig = Rig(psg.F32, width, np.concatenate([keys, fresh]), 0, end)
    rig.request(psg.PUSH, keys, synth(len(keys) * width, psg.F32, 1))
    k0, r0 = rig.t.dump()
    cap0 = rig.t.info().capacity
    base = np.union1d(keys[::2], fresh)
    swapped = base.copy()
    swapped[[700, 701]] = swapped[[701, 700]]
    repeated = base.copy()
    repeated[1200] = repeated[1199]
    at_end = np.append(base, np.uint64(end))
    for lst, code in ((swapped, 1), (repeated, 1), (at_end, 4)):
        n = len(lst)
        vals = dev(synth(n * width, psg.F32, 2))
        out = psg.DeviceBuffer(n * width * 4)
        with pytest.raises(psg.PsgError) as ei:
            rig.t.handle(flags, dev(lst), vals if flags & psg.PUSH else None, out if flags & psg.PULL else None, n)
        assert ei.value.code == code, str(ei.value)
        k1, r1 = rig.t.dump()
        np.testing.assert_array_equal(k1, k0)
        same(r1, r0)
        assert rig.t.info().capacity == cap0
    rig.request(psg.PUSH | psg.PULL, base, synth(len(base) * width, psg.F32, 3))
    rig.check_dump()


def test_clear_and_reuse():
    width = 20
    rng = np.random.default_rng(10)
    keys = random_keys(rng, 2000)
    rig = Rig(psg.F32, width, keys)
    rig.request(psg.PUSH, keys, synth(len(keys) * width, psg.F32, 1))
    rig.t.clear()
    assert rig.t.info().size == 0
    k, rows = rig.t.dump()
    assert len(k) == 0 and rows.shape == (0, width)
    # a fresh oracle: the Push after the clear starts from zero rows
    rig.o = RowOracle(psg.F32, width, keys)
    sub = keys[::3]
    v = synth(len(sub) * width, psg.F32, 2)
    got = rig.request(psg.PUSH | psg.PULL, sub, v)
    same(got, v)
    rig.check_dump()


def test_empty_request_is_a_noop():
    t = psg.Table(psg.F32, 4, 0, KMAX, 0)
    for flags in (psg.PUSH, psg.PULL, psg.PUSH | psg.PULL):
        t.handle(flags, None, None, None, 0)
    assert t.info().size == 0
    keys = np.array([5, 9], dtype=np.uint64)
    t.handle(psg.PUSH, dev(keys), dev(np.ones(8, np.float32)), None, 2)
    t.handle(psg.PUSH | psg.PULL, dev(keys), dev(np.ones(8, np.float32)), psg.DeviceBuffer(32), 0)
    k, rows = t.dump()
    np.testing.assert_array_equal(k, keys)
    same(rows, np.ones((2, 4), np.float32))
