"""The row table's optimizer update (psg_table_update / psg_table_set_adam,
csrc/psg_rows.hip) against the oracle.

The checker is a host mirror: the sorted distinct keys of a test with
rows f32[S, W] and m, v f64[S, W].  An update is replayed by gathering the
request's ranks, flattening, one oracle.lr_apply (the reference's LRServer /
Adam arithmetic; m = v = None for SGD) and scattering back.  Every comparison
is bit for bit.
"""
import numpy as np
import pytest

import oracle
import psg

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1
LR = 0.05                          # the request's f32 learning rate
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)   # an f32 rate widened, as the KV handle passes it
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


def synth(n, seed):
    return oracle.synth(n, oracle.F32, seed, 1, -1.0, 1.0)


def random_keys(rng, n, lo=0, hi=1 << 63):
    u = np.unique(rng.integers(lo, hi, 2 * n + 16, dtype=np.uint64))
    return np.sort(rng.choice(u, n, replace=False))


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
        r = self.ranks(keys)
        self.rows[r] = self.rows[r] + vals.reshape(len(keys), self.w)  # f32 adds

    def update(self, keys, grads, lr, iteration):
        r = self.ranks(keys)                                   # gather
        w = np.ascontiguousarray(self.rows[r]).ravel()         # flatten
        if self.adam:
            m = np.ascontiguousarray(self.m[r]).ravel()
            v = np.ascontiguousarray(self.v[r]).ravel()
            oracle.lr_apply(w, grads, lr, m, v, *self.adam, iteration)
            self.m[r] = m.reshape(len(keys), self.w)           # scatter
            self.v[r] = v.reshape(len(keys), self.w)
        else:
            oracle.lr_apply(w, grads, lr, None, None, iteration=iteration)
        self.rows[r] = w.reshape(len(keys), self.w)
        return w

    def clear(self):
        self.present[:] = False
        self.rows[:] = 0
        self.m[:] = 0
        self.v[:] = 0


class Rig:
    """A table and its mirror, fed the same requests."""

    def __init__(self, width, all_keys, adam, key_begin=0, key_end=KMAX, capacity=0):
        self.w = width
        self.t = psg.Table(psg.F32, width, key_begin, key_end, capacity)
        if adam:
            self.t.set_adam(*ADAM)
        self.o = Mirror(width, all_keys, ADAM if adam else None)

    def accumulate(self, keys, vals):
        self.t.handle(psg.PUSH, dev(keys), dev(vals), None, len(keys))
        self.o.accumulate(keys, vals)

    def update(self, flags, keys, grads, iteration, lr=LR):
        """the update on both; compares a PushPull's reply"""
        n = len(keys)
        out = psg.DeviceBuffer(n * self.w * 4) if flags & psg.PULL else None
        self.t.update(flags, dev(keys), dev(grads), out, n, lr, iteration)
        exp = self.o.update(keys, grads, lr, iteration)
        if out is not None:
            same(out.download(np.float32, n * self.w), exp)

    def check(self):
        p = self.o.present
        k, rows = self.t.dump()
        np.testing.assert_array_equal(k, self.o.u[p])
        same(rows, self.o.rows[p])
        if self.o.adam:
            m, v = self.t.dump_moments()
            assert m.shape == v.shape == (int(p.sum()), self.w)
            same(m, self.o.m[p])
            same(v, self.o.v[p])


def state(t, adam=True):
    k, rows = t.dump()
    return (k, rows) + (t.dump_moments() if adam else ())


def assert_state(t, before, adam=True):
    for got, exp in zip(state(t, adam), before):
        assert got.shape == exp.shape
        same(got, exp)


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("width", [1, 3, 4, 20, 64, 260])
def test_update_parity(width, adam):
    """W = 1, 3: element path; 4: one vector a row, many rows a tile; 20, 64:
    16-B rows; 260: a row longer than one pass of the block.  4097 keys are 3
    tiles at W = 4."""
    rng = np.random.default_rng(width * 7919 + adam)
    n = 4097
    keys = random_keys(rng, n)
    rig = Rig(width, keys, adam)
    rig.accumulate(keys, synth(n * width, 1))
    step = 0
    for iteration in (0, 1, 7, 999):
        for count in (1, 65, 2000, 4097):
            sub = keys if count == n else keys[np.sort(rng.choice(n, count, replace=False))]
            flags = psg.PUSH if step % 2 == 0 else psg.PUSH | psg.PULL
            rig.update(flags, sub, synth(count * width, 100 + step), iteration)
            step += 1
    rig.check()


def test_moments_follow_their_rows():
    width = 20
    rng = np.random.default_rng(5)
    b = random_keys(rng, 4097)
    a = b[::64]  # 65 keys, each with 63 new keys between it and the next
    assert len(a) == 65
    rig = Rig(width, b, True, capacity=0)
    rig.update(psg.PUSH, a, synth(len(a) * width, 1), 0)
    assert rig.t.info().size == 65 and rig.t.info().capacity == 1024
    rig.update(psg.PUSH | psg.PULL, b, synth(len(b) * width, 2), 1)
    assert rig.t.info().size == 4097 and rig.t.info().capacity > 1024  # rows moved, the table grew
    rig.update(psg.PUSH | psg.PULL, a, synth(len(a) * width, 3), 2)
    rig.check()


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_unaligned_request_arrays(adam):
    """grads and out 4 B into their buffers: the element path on 16-B rows."""
    width, n = 4, 4097
    rng = np.random.default_rng(6)
    keys = random_keys(rng, n)
    rig = Rig(width, keys, adam)
    rig.accumulate(keys, synth(n * width, 1))
    for it, flags in ((0, psg.PUSH), (3, psg.PUSH | psg.PULL)):
        g = synth(n * width, 10 + it)
        gb, ob = psg.DeviceBuffer(n * width * 4 + 16), psg.DeviceBuffer(n * width * 4 + 16)
        gb.upload(g, offset=4)
        rig.t.update(flags, dev(keys), gb.ptr + 4, ob.ptr + 4 if flags & psg.PULL else None, n, LR, it)
        exp = rig.o.update(keys, g, LR, it)
        if flags & psg.PULL:
            same(ob.download(np.float32, n * width, offset=4), exp)
    # and an aligned request on the same table: both paths share one moment layout
    rig.update(psg.PUSH | psg.PULL, keys, synth(n * width, 20), 4)
    rig.check()


def test_rejections_leave_everything_unchanged():
    width, end = 20, 1 << 30
    rng = np.random.default_rng(9)
    keys = random_keys(rng, 3000, 0, end - 1)
    fresh = np.setdiff1d(random_keys(rng, 500, 0, end - 1), keys)  # absent keys a bad list also holds
    rig = Rig(width, np.concatenate([keys, fresh]), True, 0, end)
    rig.accumulate(keys, synth(len(keys) * width, 1))
    rig.update(psg.PUSH, keys[::3], synth(len(keys[::3]) * width, 2), 0)  # moments that are not zero
    before = state(rig.t)
    cap0 = rig.t.info().capacity
    base = np.union1d(keys[::2], fresh)
    swapped = base.copy()
    swapped[[700, 701]] = swapped[[701, 700]]
    repeated = base.copy()
    repeated[1200] = repeated[1199]
    at_end = np.append(base, np.uint64(end))
    for lst, flags, code in ((swapped, psg.PUSH, 1), (repeated, psg.PUSH | psg.PULL, 1), (at_end, psg.PUSH, 4),
                             (base, psg.PULL, 1), (base, 0, 1)):
        n = len(lst)
        with pytest.raises(psg.PsgError) as ei:
            rig.t.update(flags, dev(lst), dev(synth(n * width, 3)), psg.DeviceBuffer(n * width * 4), n, LR, 1)
        assert ei.value.code == code, str(ei.value)
        assert_state(rig.t, before)
        assert rig.t.info().capacity == cap0
    with pytest.raises(psg.PsgError) as ei:
        rig.t.update(psg.PUSH, dev(base), dev(synth(len(base) * width, 3)), None, len(base), LR, -1)
    assert ei.value.code == 1
    with pytest.raises(psg.PsgError) as ei:
        rig.t.set_adam(*ADAM)  # a second call
    assert ei.value.code == 1
    assert_state(rig.t, before)
    for bad in ((0.01, 1.0, 0.999, 1e-8), (0.01, 0.9, -0.1, 1e-8), (0.01, 0.9, 0.999, -1e-8)):
        with pytest.raises(psg.PsgError) as ei:
            psg.Table(psg.F32, width, 0, end, 0).set_adam(*bad)
        assert ei.value.code == 1, bad
    # an F16 table takes neither Adam state nor an update, and keeps its rows
    h = psg.Table(psg.F16, 4, 0, KMAX, 0)
    hk = np.array([3, 8], dtype=np.uint64)
    h.handle(psg.PUSH, dev(hk), dev(np.arange(8, dtype=np.float16)), None, 2)
    h0 = state(h, adam=False)
    with pytest.raises(psg.PsgError) as ei:
        h.set_adam(*ADAM)
    assert ei.value.code == 6
    with pytest.raises(psg.PsgError) as ei:
        h.update(psg.PUSH, dev(hk), dev(np.ones(8, np.float32)), None, 2, LR, 0)
    assert ei.value.code == 6
    assert_state(h, h0, adam=False)
    # the table still serves a good request
    rig.update(psg.PUSH | psg.PULL, base, synth(len(base) * width, 4), 1)
    rig.check()


def test_interplay_with_accumulate_clear_and_plain_tables():
    width = 20
    rng = np.random.default_rng(10)
    keys = random_keys(rng, 2000)
    rig = Rig(width, keys, True)
    rig.update(psg.PUSH, keys, synth(len(keys) * width, 1), 0)
    # an accumulate Push (with keys the update never saw in between): rows only
    _, _, m0, v0 = state(rig.t)
    sub = keys[::3]
    rig.accumulate(sub, synth(len(sub) * width, 2))
    _, _, m1, v1 = state(rig.t)
    same(m1, m0)
    same(v1, v0)
    rig.check()
    # clear: the next update starts from zero rows and zero moments
    rig.t.clear()
    rig.o.clear()
    assert rig.t.info().size == 0
    m, v = rig.t.dump_moments()
    assert m.shape == v.shape == (0, width)
    rig.update(psg.PUSH | psg.PULL, sub, synth(len(sub) * width, 3), 5)
    rig.check()
    # a table without set_adam updates as SGD and has no moments to dump
    plain = Rig(width, keys, False)
    plain.update(psg.PUSH | psg.PULL, keys, synth(len(keys) * width, 4), 0)
    plain.update(psg.PUSH, sub, synth(len(sub) * width, 5), 1)
    plain.check()
    with pytest.raises(psg.PsgError) as ei:
        plain.t.dump_moments()
    assert ei.value.code == 1
    # an empty request is a no-op
    rig.t.update(psg.PUSH, None, None, None, 0, LR, 0)
    rig.check()
