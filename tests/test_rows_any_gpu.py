"""The row table's order-preserving requests (psg_table_handle_any /
psg_table_update_any, csrc/psg_rows.hip) against the oracle.

Accumulate: the scalar oracle.Store fed the expanded keys rank * W + j,
row-major, in the request's own order — the reference loop (KVApp.h:446-454)
per element, which applies repeats in arrival order.  Update: a host mirror of
rows and moments replayed in rounds — round r holds the r-th occurrence of
every key, so its keys are distinct and one oracle.lr_apply serves it; the
rounds run in order, which is arrival order inside every key.  Every comparison
is bit for bit.
"""
import numpy as np
import pytest

import oracle
import psg

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1
LR = 0.05
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
NPT = {psg.F32: np.float32, psg.F64: np.float64, psg.F16: np.uint16, psg.BF16: np.uint16}
ES = {psg.F32: 4, psg.F64: 8, psg.F16: 2, psg.BF16: 2}
BITS = {4: np.uint32, 8: np.uint64, 2: np.uint16}
WIDTHS = [1, 3, 4, 20, 64, 260]


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
    """real-valued data for F32 / F64, integer-valued for the halves (as test_rows_gpu)."""
    if dtype in (psg.F32, psg.F64):
        return oracle.synth(n, dtype, seed, 1, -1.0, 1.0)
    return oracle.synth(n, dtype, seed, 0, 0.0, 1000.0)


def random_keys(rng, n, lo=0, hi=1 << 63):
    u = np.unique(rng.integers(lo, hi, 2 * n + 16, dtype=np.uint64))
    return np.sort(rng.choice(u, n, replace=False))


# ---- the lists ------------------------------------------------------------------
def straddle_list(rng):
    """2049 occurrences; in sorted order one key holds positions 1020..1027, across
    the edge (1023 / 1024) of the head scan's 1024-position tile."""
    d = random_keys(rng, 2042)
    s = np.concatenate([d[:1020], np.repeat(d[1020], 8), d[1021:]])
    assert len(s) == 2049 and s[1019] < s[1020] == s[1027] < s[1028]
    return rng.permutation(s)


LISTS = {
    "shuffled65": lambda rng: rng.permutation(random_keys(rng, 65)),
    "shuffled4097": lambda rng: rng.permutation(random_keys(rng, 4097)),
    "descending": lambda rng: random_keys(rng, 1500)[::-1].copy(),
    "repeats": lambda rng: rng.choice(random_keys(rng, 500), 4097),
    "nondescending": lambda rng: np.sort(rng.choice(random_keys(rng, 400), 3000)),
    "hot300": lambda rng: np.repeat(random_keys(rng, 1), 300),
    "straddle": straddle_list,
    "n1": lambda rng: random_keys(rng, 1),
    "n2same": lambda rng: np.repeat(random_keys(rng, 1), 2),
}


# ---- accumulate -----------------------------------------------------------------
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
    """A table and its oracle, fed the same requests through handle_any."""

    def __init__(self, dtype, width, all_keys, key_begin=0, key_end=KMAX, capacity=0):
        self.dtype, self.w = dtype, width
        self.t = psg.Table(dtype, width, key_begin, key_end, capacity)
        self.o = RowOracle(dtype, width, all_keys)

    def request(self, flags, keys, vals=None, offset=0):
        """the request on both; compares the Pull's reply; returns it.  offset:
        bytes by which the request arrays are shifted inside their buffers."""
        n = len(keys)
        nb = n * self.w * ES[self.dtype]
        dk = dev(np.asarray(keys, dtype=np.uint64))
        dv = out = None
        if flags & psg.PUSH:
            dv = psg.DeviceBuffer(nb + 16)
            dv.upload(vals, offset=offset)
        if flags & psg.PULL:
            out = psg.DeviceBuffer(nb + 16)
        self.t.handle_any(flags, dk, dv.ptr + offset if dv else None, out.ptr + offset if out else None, n)
        np.testing.assert_array_equal(dk.download(np.uint64, n), keys)  # the caller's keys are never written
        exp = self.o.handle(flags, keys, vals)
        if not flags & psg.PULL:
            return None
        got = out.download(NPT[self.dtype], n * self.w, offset=offset)
        same(got, exp)
        return got

    def check_dump(self):
        k, rows = self.t.dump()
        ok, orows = self.o.dump()
        np.testing.assert_array_equal(k, ok)
        same(rows, orows)
        assert self.t.info().size == len(ok)


def three_requests(rig, keys, seed, offset=0):
    n, w, dt = len(keys), rig.w, rig.dtype
    rig.request(psg.PUSH, keys, synth(n * w, dt, seed), offset)
    rig.request(psg.PUSH | psg.PULL, keys, synth(n * w, dt, seed + 1), offset)
    pulled = rig.request(psg.PULL, keys, None, offset).reshape(n, w)
    # every occurrence of a key is answered with the row
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    same(pulled, pulled[first][inv])
    rig.check_dump()


@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("width", WIDTHS)
def test_push_pushpull_pull_in_arrival_order(width, name):
    """W = 1, 3: element path; 4, 20, 64: 16-B rows; 260: a row longer than one
    pass of a wave.  The Push inserts every key once; the PushPull and the Pull
    find them present."""
    rng = np.random.default_rng(width * 1009 + sorted(LISTS).index(name))
    keys = LISTS[name](rng)
    rig = Rig(psg.F32, width, keys)
    three_requests(rig, keys, 11)
    assert rig.t.info().size == len(np.unique(keys))


@pytest.mark.parametrize("width", [3, 20])
@pytest.mark.parametrize("dtype", [psg.F64, psg.F16, psg.BF16], ids=["f64", "f16", "bf16"])
def test_other_dtypes_on_the_repeats_list(dtype, width):
    rng = np.random.default_rng(dtype * 31 + width)
    keys = LISTS["repeats"](rng)
    three_requests(Rig(dtype, width, keys), keys, 21)


def test_inserts_of_keys_named_several_times_on_a_table_that_grows():
    width = 20
    rng = np.random.default_rng(3)
    a = random_keys(rng, 1000, 1 << 20, 1 << 40)
    fresh = np.setdiff1d(np.concatenate([random_keys(rng, 100, 0, 1 << 20), random_keys(rng, 1200, 1 << 20, 1 << 40),
                                         random_keys(rng, 100, 1 << 40, 1 << 41)]), a)
    rig = Rig(psg.F32, width, np.concatenate([a, fresh]))
    rig.request(psg.PUSH, rng.permutation(a), synth(len(a) * width, psg.F32, 1))
    cap0 = rig.t.info().capacity
    assert rig.t.info().size == len(a) and cap0 < len(a) + len(fresh)
    # present keys among absent ones, each absent key named three times
    lst = rng.permutation(np.concatenate([a[::2], np.repeat(fresh, 3)]))
    got = rig.request(psg.PUSH | psg.PULL, lst, synth(len(lst) * width, psg.F32, 2))
    assert got is not None
    assert rig.t.info().size == len(a) + len(fresh) and rig.t.info().capacity > cap0
    rig.check_dump()
    # a Pull that names absent keys several times: zero rows, inserted once each
    more = random_keys(rng, 300, 0, 1 << 41)
    rig2 = Rig(psg.F32, width, more)
    pulled = rig2.request(psg.PULL, rng.permutation(np.repeat(more, 2)))
    assert not np.any(bits(pulled)) and rig2.t.info().size == len(more)


def test_unaligned_request_arrays():
    """vals and out 4 B into their buffers: the element path on 16-B rows."""
    rng = np.random.default_rng(4)
    keys = LISTS["repeats"](rng)
    rig = Rig(psg.F32, 20, keys)
    three_requests(rig, keys, 31, offset=4)
    three_requests(rig, keys, 41)  # and aligned arrays on the same table


def state(t, adam):
    k, rows = t.dump()
    return (k, rows) + (t.dump_moments() if adam else ())


def assert_state(t, before, adam):
    for got, exp in zip(state(t, adam), before):
        assert got.shape == exp.shape
        same(got, exp)


def test_a_key_out_of_range_fails_the_request_and_writes_nothing():
    width, end = 20, 1 << 30
    rng = np.random.default_rng(5)
    keys = random_keys(rng, 2000, 0, end - 1)
    fresh = np.setdiff1d(random_keys(rng, 300, 0, end - 1), keys)
    t = psg.Table(psg.F32, width, 0, end, 0)
    t.set_adam(*ADAM)
    t.update(psg.PUSH, dev(keys), dev(synth(len(keys) * width, psg.F32, 1)), None, len(keys), LR, 0)
    before, cap0, size0 = state(t, True), t.info().capacity, t.info().size
    lst = rng.permutation(np.concatenate([np.repeat(keys[::3], 2), fresh, [np.uint64(end)]]).astype(np.uint64))
    n = len(lst)
    vals, out = dev(synth(n * width, psg.F32, 2)), psg.DeviceBuffer(n * width * 4)
    for flags in (psg.PUSH, psg.PUSH | psg.PULL, psg.PULL):
        with pytest.raises(psg.PsgError) as ei:
            t.handle_any(flags, dev(lst), vals, out, n)
        assert ei.value.code == 4, str(ei.value)
    for flags in (psg.PUSH, psg.PUSH | psg.PULL):
        with pytest.raises(psg.PsgError) as ei:
            t.update_any(flags, dev(lst), vals, out, n, LR, 1)
        assert ei.value.code == 4, str(ei.value)
    assert_state(t, before, True)
    assert t.info().capacity == cap0 and t.info().size == size0
    # the argument checks of the strict calls
    for bad_flags in (0, 4):
        with pytest.raises(psg.PsgError) as ei:
            t.handle_any(bad_flags, dev(lst), vals, out, n)
        assert ei.value.code == 1
    for call in (lambda: t.update_any(psg.PULL, dev(lst), vals, out, n, LR, 1),
                 lambda: t.update_any(psg.PUSH, dev(lst), vals, None, n, LR, -1),
                 lambda: t.update_any(psg.PUSH, dev(lst), None, None, n, LR, 1),
                 lambda: t.handle_any(psg.PUSH, dev(lst), None, None, n),
                 lambda: t.handle_any(psg.PULL, dev(lst), None, None, n),
                 lambda: t.handle_any(psg.PULL, None, None, out, n)):
        with pytest.raises(psg.PsgError) as ei:
            call()
        assert ei.value.code == 1
    h = psg.Table(psg.F16, 4, 0, KMAX, 0)
    with pytest.raises(psg.PsgError) as ei:
        h.update_any(psg.PUSH, dev(np.array([3, 3], np.uint64)), dev(np.ones(8, np.float32)), None, 2, LR, 0)
    assert ei.value.code == 6
    # n == 0 is a no-op
    t.handle_any(psg.PUSH | psg.PULL, None, None, None, 0)
    t.update_any(psg.PUSH, None, None, None, 0, LR, 0)
    assert_state(t, before, True)


def test_the_strict_calls_still_reject_such_lists():
    width = 4
    rng = np.random.default_rng(6)
    keys = random_keys(rng, 1000)
    t = psg.Table(psg.F32, width, 0, KMAX, 0)
    t.handle(psg.PUSH, dev(keys), dev(synth(len(keys) * width, psg.F32, 1)), None, len(keys))
    before = state(t, False)
    for lst in (rng.permutation(keys), np.sort(rng.choice(keys, 1000))):
        n = len(lst)
        with pytest.raises(psg.PsgError) as ei:
            t.handle(psg.PUSH | psg.PULL, dev(lst), dev(synth(n * width, psg.F32, 2)), psg.DeviceBuffer(n * width * 4), n)
        assert ei.value.code == 1, str(ei.value)
        with pytest.raises(psg.PsgError) as ei:
            t.update(psg.PUSH, dev(lst), dev(synth(n * width, psg.F32, 2)), None, n, LR, 0)
        assert ei.value.code == 1, str(ei.value)
        assert_state(t, before, False)


@pytest.mark.parametrize("width", [3, 20])
def test_a_strictly_ascending_list_equals_the_strict_call(width):
    rng = np.random.default_rng(7 + width)
    keys = random_keys(rng, 4097)
    n = len(keys)
    a, b = psg.Table(psg.F32, width, 0, KMAX, 0), psg.Table(psg.F32, width, 0, KMAX, 0)
    for t in (a, b):
        t.set_adam(*ADAM)
    dk = dev(keys)
    for seed, flags in ((1, psg.PUSH), (2, psg.PUSH | psg.PULL), (3, psg.PULL)):
        v = dev(synth(n * width, psg.F32, seed))
        oa, ob = psg.DeviceBuffer(n * width * 4), psg.DeviceBuffer(n * width * 4)
        a.handle_any(flags, dk, v, oa, n)
        b.handle(flags, dk, v, ob, n)
        if flags & psg.PULL:
            same(oa.download(np.float32, n * width), ob.download(np.float32, n * width))
    for seed, flags in ((4, psg.PUSH), (5, psg.PUSH | psg.PULL)):
        g = dev(synth(n * width, psg.F32, seed))
        oa, ob = psg.DeviceBuffer(n * width * 4), psg.DeviceBuffer(n * width * 4)
        a.update_any(flags, dk, g, oa, n, LR, seed)
        b.update(flags, dk, g, ob, n, LR, seed)
        if flags & psg.PULL:
            same(oa.download(np.float32, n * width), ob.download(np.float32, n * width))
    assert_state(a, state(b, True), True)


# ---- the optimizer update ---------------------------------------------------------
class Mirror:
    """rows and moments of every key a test uses, in key order, on the host."""

    def __init__(self, width, all_keys, adam):
        self.w, self.adam = width, adam
        self.u = np.unique(np.asarray(all_keys, dtype=np.uint64))
        s = len(self.u)
        self.present = np.zeros(s, bool)
        self.rows = np.zeros((s, width), np.float32)
        self.m = np.zeros((s, width), np.float64)
        self.v = np.zeros((s, width), np.float64)

    def ranks(self, keys):
        r = np.searchsorted(self.u, keys)
        assert np.array_equal(self.u[r], keys)
        self.present[r] = True
        return r

    def accumulate(self, keys, vals):
        """distinct keys"""
        r = self.ranks(keys)
        self.rows[r] = self.rows[r] + vals.reshape(len(keys), self.w)  # f32 adds

    def update_distinct(self, r, grads, lr, iteration):
        w = np.ascontiguousarray(self.rows[r]).ravel()
        grads = np.ascontiguousarray(grads).ravel()
        if self.adam:
            m = np.ascontiguousarray(self.m[r]).ravel()
            v = np.ascontiguousarray(self.v[r]).ravel()
            oracle.lr_apply(w, grads, lr, m, v, *self.adam, iteration)
            self.m[r] = m.reshape(len(r), self.w)
            self.v[r] = v.reshape(len(r), self.w)
        else:
            oracle.lr_apply(w, grads, lr, None, None, iteration=iteration)
        self.rows[r] = w.reshape(len(r), self.w)
        return self.rows[r]

    def update(self, keys, grads, lr, iteration):
        """any list, in rounds: round k holds the k-th occurrence of every key.
        Returns the reply: the row after each occurrence."""
        n = len(keys)
        r = self.ranks(keys)
        g = grads.reshape(n, self.w)
        order = np.argsort(keys, kind="stable")
        sk = keys[order]
        start = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
        occ = np.empty(n, np.int64)
        occ[order] = np.arange(n) - np.repeat(start, np.diff(np.append(start, n)))
        out = np.empty((n, self.w), np.float32)
        for k in range(int(occ.max()) + 1):
            idx = np.flatnonzero(occ == k)
            out[idx] = self.update_distinct(r[idx], g[idx], lr, iteration)
        return out.ravel()


class OptRig:
    def __init__(self, width, all_keys, adam, key_begin=0, key_end=KMAX):
        self.w = width
        self.t = psg.Table(psg.F32, width, key_begin, key_end, 0)
        if adam:
            self.t.set_adam(*ADAM)
        self.o = Mirror(width, all_keys, ADAM if adam else None)

    def accumulate(self, keys, vals):
        self.t.handle(psg.PUSH, dev(keys), dev(vals), None, len(keys))
        self.o.accumulate(keys, vals)

    def update(self, flags, keys, grads, iteration, lr=LR):
        n = len(keys)
        out = psg.DeviceBuffer(n * self.w * 4) if flags & psg.PULL else None
        self.t.update_any(flags, dev(keys), dev(grads), out, n, lr, iteration)
        exp = self.o.update(keys, grads, lr, iteration)
        if out is not None:
            same(out.download(np.float32, n * self.w), exp)

    def check(self):
        p = self.o.present
        k, rows = self.t.dump()
        np.testing.assert_array_equal(k, self.o.u[p])
        same(rows, self.o.rows[p])
        assert self.t.info().size == int(p.sum())
        if self.o.adam:
            m, v = self.t.dump_moments()
            same(m, self.o.m[p])
            same(v, self.o.v[p])


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("width", WIDTHS)
def test_update_in_arrival_order(width, adam):
    rng = np.random.default_rng(width * 7919 + adam)
    lists = [LISTS[name](rng) for name in ("repeats", "shuffled4097", "hot300")]
    rig = OptRig(width, np.concatenate(lists), adam)
    seed = np.unique(lists[0])[::2]  # half of the first list's keys are present, the rest are inserted
    rig.accumulate(seed, synth(len(seed) * width, psg.F32, 1))
    step = 0
    for keys in lists:
        for iteration, flags in ((0, psg.PUSH), (7, psg.PUSH | psg.PULL)):
            rig.update(flags, keys, synth(len(keys) * width, psg.F32, 100 + step), iteration)
            step += 1
    rig.check()


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_update_of_an_absent_key_named_three_times(adam):
    width = 20
    present = np.array([10, 30], dtype=np.uint64)
    rig = OptRig(width, np.array([10, 20, 30], dtype=np.uint64), adam)
    rig.accumulate(present, synth(2 * width, psg.F32, 1))
    keys = np.array([20, 30, 20, 10, 20], dtype=np.uint64)
    rig.update(psg.PUSH | psg.PULL, keys, synth(len(keys) * width, psg.F32, 2), 3)
    assert rig.t.info().size == 3
    rig.check()


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("width", [3, 20])
def test_the_definition_n_one_key_requests(width, adam):
    """65 occurrences of 20 keys: a twin table fed the 65 one-key strict calls
    ends identical in rows, moments and reply, for accumulate and for update."""
    rng = np.random.default_rng(8 + width)
    keys = rng.choice(random_keys(rng, 20), 65)
    n = len(keys)
    a, b = psg.Table(psg.F32, width, 0, KMAX, 0), psg.Table(psg.F32, width, 0, KMAX, 0)
    if adam:
        for t in (a, b):
            t.set_adam(*ADAM)
    dk = dev(keys)
    for seed, update, flags in ((1, False, psg.PUSH | psg.PULL), (2, True, psg.PUSH | psg.PULL), (3, True, psg.PUSH),
                                (4, False, psg.PULL)):
        v = dev(synth(n * width, psg.F32, seed))
        oa, ob = psg.DeviceBuffer(n * width * 4), psg.DeviceBuffer(n * width * 4)
        rb = width * 4
        if update:
            a.update_any(flags, dk, v, oa, n, LR, 5)
            for i in range(n):
                b.update(flags, dk.ptr + 8 * i, v.ptr + rb * i, ob.ptr + rb * i, 1, LR, 5)
        else:
            a.handle_any(flags, dk, v, oa, n)
            for i in range(n):
                b.handle(flags, dk.ptr + 8 * i, v.ptr + rb * i, ob.ptr + rb * i, 1)
        if flags & psg.PULL:
            same(oa.download(np.float32, n * width), ob.download(np.float32, n * width))
    assert_state(a, state(b, adam), adam)
