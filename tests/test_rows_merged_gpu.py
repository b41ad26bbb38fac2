"""The row table's merged update (psg_table_update_merged, csrc/psg_rows.hip):
the sync-mode round of LRServer.h:151-178 on rows.

The expected state comes from a host mirror of rows and moments.  For each
unique key the gradients of its occurrences are added in numpy f32 from
np.float32(0) in arrival order (frame, then position); then ONE oracle.lr_apply
runs over the touched elements with the request's iteration.  Every comparison
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
WIDTHS = [1, 3, 4, 20, 64, 260]
SAME, SORTED = psg.MERGED_SAME_LIST, psg.MERGED_SORTED


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def dev(a):
    return psg.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, exp):
    np.testing.assert_array_equal(bits(got), bits(exp))


def synth(n, seed):
    return oracle.synth(n, psg.F32, seed, 1, -1.0, 1.0)


def random_keys(rng, n, lo=0, hi=1 << 63):
    u = np.unique(rng.integers(lo, hi, 2 * n + 16, dtype=np.uint64))
    return np.sort(rng.choice(u, n, replace=False))


# ---- the host mirror ----------------------------------------------------------
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
        self.rows[r] = self.rows[r] + vals.reshape(len(keys), self.w)

    def merged(self, keys_list, grads_list, lr, iteration):
        """The round: per unique key f32 adds from 0 in arrival order, one
        lr_apply over the touched rows.  Returns each frame's reply."""
        keys = np.concatenate([np.asarray(k, np.uint64) for k in keys_list])
        g = np.concatenate([np.asarray(x, np.float32).reshape(-1, self.w) for x in grads_list])
        n = len(keys)
        r = self.ranks(keys)
        touched, inv = np.unique(r, return_inverse=True)
        order = np.argsort(r, kind="stable")
        sr = r[order]
        start = np.flatnonzero(np.concatenate([[True], sr[1:] != sr[:-1]]))
        occ = np.empty(n, np.int64)
        occ[order] = np.arange(n) - np.repeat(start, np.diff(np.append(start, n)))
        s = np.zeros((len(touched), self.w), np.float32)  # the merge buffer, from +0
        for k in range(int(occ.max()) + 1):  # round k: the k-th occurrence of every key, distinct rows
            idx = np.flatnonzero(occ == k)
            s[inv[idx]] = s[inv[idx]] + g[idx]
        w = np.ascontiguousarray(self.rows[touched]).ravel()
        if self.adam:
            m = np.ascontiguousarray(self.m[touched]).ravel()
            v = np.ascontiguousarray(self.v[touched]).ravel()
            oracle.lr_apply(w, s.ravel(), lr, m, v, *self.adam, iteration)
            self.m[touched] = m.reshape(-1, self.w)
            self.v[touched] = v.reshape(-1, self.w)
        else:
            oracle.lr_apply(w, s.ravel(), lr, None, None, iteration=iteration)
        self.rows[touched] = w.reshape(-1, self.w)
        out = self.rows[r]
        cuts = np.cumsum([len(k) for k in keys_list])[:-1]
        return [x.ravel() for x in np.split(out, cuts)], (self.u[touched], s)


class Rig:
    def __init__(self, width, all_keys, adam, key_begin=0, key_end=KMAX):
        self.w = width
        self.t = psg.Table(psg.F32, width, key_begin, key_end, 0)
        if adam:
            self.t.set_adam(*ADAM)
        self.o = Mirror(width, all_keys, ADAM if adam else None)

    def accumulate(self, keys, vals):
        self.t.handle(psg.PUSH, dev(keys), dev(vals), None, len(keys))
        self.o.accumulate(keys, vals)

    def merged(self, flags, keys_list, seed, iteration, lr=LR, grad_off=(), out_off=(), share_keys=False):
        """The round on the table and on the mirror; compares every frame's
        reply; returns the path.  grad_off / out_off: frames whose gradient /
        reply array starts 4 B into its buffer.  share_keys: an even frame that
        carries frame 0's list passes frame 0's device array itself."""
        k, w = len(keys_list), self.w
        ns = [len(x) for x in keys_list]
        grads = [synth(n * w, seed + 31 * j) for j, n in enumerate(ns)]
        dk, dg, do, pk, pg, po = [], [], [], [], [], []
        for j, n in enumerate(ns):
            if n == 0:  # an empty frame: null pointers
                pk.append(None), pg.append(None), po.append(None), do.append(None)
                continue
            if share_keys and j and j % 2 == 0 and keys_list[j] is keys_list[0]:
                pk.append(pk[0])
            else:
                dk.append(dev(keys_list[j]))
                pk.append(dk[-1].ptr)
            go = 4 if j in grad_off else 0
            b = psg.DeviceBuffer(n * w * 4 + 16)
            b.upload(grads[j], offset=go)
            dg.append(b)
            pg.append(b.ptr + go)
            oo = 4 if j in out_off else 0
            ob = psg.DeviceBuffer(n * w * 4 + 16) if flags & psg.PULL else None
            do.append((ob, oo))
            po.append(ob.ptr + oo if ob else None)
        path = self.t.update_merged(flags, pk, pg, po if flags & psg.PULL else None, ns, lr, iteration)
        exp, _ = self.o.merged(keys_list, grads, lr, iteration)
        if flags & psg.PULL:
            for j, n in enumerate(ns):
                if n:
                    ob, oo = do[j]
                    same(ob.download(np.float32, n * w, offset=oo), exp[j])
        return path

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


# ---- the rounds -----------------------------------------------------------------
def same_list(n, k):
    return lambda rng: [random_keys(rng, n)] * k


def changed(n, k):
    """the same lists, one key of frame 1 changed (to its neighbour: a repeat)"""
    def make(rng):
        a = random_keys(rng, n)
        b = a.copy()
        b[n // 2] = b[n // 2 + 1]
        return [a, b] + [a] * (k - 2)
    return make


def straddle(rng):
    """2049 occurrences in 3 frames; in sorted order one key holds positions
    1020..1027, across the edge (1023 / 1024) of the head scan's tile."""
    d = random_keys(rng, 2042)
    s = np.concatenate([d[:1020], np.repeat(d[1020], 8), d[1021:]])
    assert len(s) == 2049 and s[1019] < s[1020] == s[1027] < s[1028]
    s = rng.permutation(s)
    return [s[:700], s[700:1400], s[1400:]]


def disjoint(rng):
    d = random_keys(rng, 3000)
    return [d[0::3], d[1::3][:700], d[2::3][:999]]


def overlap(rng):
    pool = random_keys(rng, 500)
    return [rng.choice(pool, 1000) for _ in range(4)]


def ragged(rng):
    pool = random_keys(rng, 900)
    return [rng.choice(pool, 700), pool[:0], rng.choice(pool, 1), rng.permutation(pool)[:650], rng.choice(pool, 1300)]


def hot300(rng):
    key = random_keys(rng, 1)
    return [np.repeat(key, 19 if j < 12 else 18) for j in range(16)]  # 12 * 19 + 4 * 18 = 300


ROUNDS = {f"same{n}_k{k}": (same_list(n, k), SAME) for n in (65, 4097) for k in (1, 2, 3, 16)}
ROUNDS.update({
    "changed65_k2": (changed(65, 2), SORTED),
    "changed65_k16": (changed(65, 16), SORTED),
    "changed4097_k3": (changed(4097, 3), SORTED),
    "disjoint_k3": (disjoint, SORTED),
    "overlap_k4": (overlap, SORTED),
    "ragged_k5": (ragged, SORTED),
    "straddle_k3": (straddle, SORTED),
    "hot300_k16": (hot300, SORTED),
    "n1": (same_list(1, 1), SAME),
    "shuffled_k1": (lambda rng: [rng.permutation(random_keys(rng, 1500))], SORTED),
})


@pytest.mark.parametrize("name", list(ROUNDS))
@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("width", WIDTHS)
def test_parity_with_the_host_mirror(width, adam, name):
    """W = 1, 3: element path; 4, 20, 64: 16-B units; 260: a row longer than one
    pass of a wave.  A Push at iteration 0 (half the keys present, the rest
    inserted), then a PushPull at iteration 7."""
    make, path = ROUNDS[name]
    rng = np.random.default_rng(width * 1009 + 2 * sorted(ROUNDS).index(name) + adam)
    keys_list = make(rng)
    rig = Rig(width, np.concatenate(keys_list), adam)
    seed = rig.o.u[::2]
    rig.accumulate(seed, synth(len(seed) * width, 1))
    assert rig.merged(psg.PUSH, keys_list, 100, 0, share_keys=True) == path
    assert rig.merged(psg.PUSH | psg.PULL, keys_list, 200, 7) == path
    assert rig.t.info().size == len(rig.o.u)
    rig.check()


def state(t, adam):
    k, rows = t.dump()
    return (k, rows) + (t.dump_moments() if adam else ())


def assert_state(t, before, adam):
    for got, exp in zip(state(t, adam), before):
        assert got.shape == exp.shape
        same(got, exp)


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("width", [3, 20])
def test_the_definition_on_a_twin_table(width, adam):
    """Rows, moments and replies equal those of psg_table_update on the unique
    ascending list with the host-summed gradients."""
    rng = np.random.default_rng(40 + width)
    pool = random_keys(rng, 300)
    keys_list = [rng.choice(pool, 400), rng.permutation(pool)[:250], rng.choice(pool, 7)]
    a, b = psg.Table(psg.F32, width, 0, KMAX, 0), psg.Table(psg.F32, width, 0, KMAX, 0)
    seedv = dev(synth(150 * width, 1))
    for t in (a, b):
        if adam:
            t.set_adam(*ADAM)
        t.handle(psg.PUSH, dev(pool[::2]), seedv, None, 150)
    for it, seed in ((0, 10), (5, 20)):
        grads = [synth(len(x) * width, seed + j) for j, x in enumerate(keys_list)]
        outs = [psg.DeviceBuffer(len(x) * width * 4) for x in keys_list]
        path = a.update_merged(psg.PUSH | psg.PULL, [dev(x) for x in keys_list], [dev(g) for g in grads], outs,
                               [len(x) for x in keys_list], LR, it)
        assert path == SORTED
        _, (uk, s) = Mirror(width, pool, None).merged(keys_list, grads, LR, it)  # the host-summed gradients
        ob = psg.DeviceBuffer(len(uk) * width * 4)
        b.update(psg.PUSH | psg.PULL, dev(uk), dev(s), ob, len(uk), LR, it)
        twin = ob.download(np.float32, len(uk) * width).reshape(len(uk), width)
        for x, o in zip(keys_list, outs):
            same(o.download(np.float32, len(x) * width).reshape(len(x), width), twin[np.searchsorted(uk, x)])
        assert_state(a, state(b, adam), adam)


def test_one_adam_step_on_the_sum_not_one_per_occurrence():
    """One key named 5 times: the moments are those of one step on the sum, and
    differ from a twin fed psg_table_update_any (five steps)."""
    width = 4
    key = np.array([77], np.uint64)
    keys = np.repeat(key, 5)
    g = synth(5 * width, 3)
    rig = Rig(width, key, True)
    twin = psg.Table(psg.F32, width, 0, KMAX, 0)
    twin.set_adam(*ADAM)
    rig.accumulate(key, synth(width, 1))
    twin.handle(psg.PUSH, dev(key), dev(synth(width, 1)), None, 1)
    dg = dev(g)
    assert rig.t.update_merged(psg.PUSH, [dev(keys)], [dg], None, [5], LR, 2) == SORTED
    rig.o.merged([keys], [g], LR, 2)
    rig.check()
    twin.update_any(psg.PUSH, dev(keys), dg, None, 5, LR, 2)
    m, v = rig.t.dump_moments()
    tm, tv = twin.dump_moments()
    assert not np.array_equal(bits(m), bits(tm)) and not np.array_equal(bits(v), bits(tv))
    # one step on the sum, by the strict call on a third table
    s = np.zeros(width, np.float32)
    for i in range(5):
        s = s + g[i * width:(i + 1) * width]
    one = psg.Table(psg.F32, width, 0, KMAX, 0)
    one.set_adam(*ADAM)
    one.handle(psg.PUSH, dev(key), dev(synth(width, 1)), None, 1)
    one.update(psg.PUSH, dev(key), dev(s), None, 1, LR, 2)
    assert_state(rig.t, state(one, True), True)


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_inserts_of_absent_keys_named_in_several_frames_on_a_table_that_grows(adam):
    width = 20
    rng = np.random.default_rng(3)
    a = random_keys(rng, 1000, 1 << 20, 1 << 40)
    fresh = np.setdiff1d(np.concatenate([random_keys(rng, 100, 0, 1 << 20), random_keys(rng, 1200, 1 << 20, 1 << 40),
                                         random_keys(rng, 100, 1 << 40, 1 << 41)]), a)
    rig = Rig(width, np.concatenate([a, fresh]), adam)
    assert rig.merged(psg.PUSH, [a, a], 1, 0) == SAME  # every key inserted by the same-list path
    cap0 = rig.t.info().capacity
    assert rig.t.info().size == len(a) and cap0 < len(a) + len(fresh)
    frames = [rng.permutation(np.concatenate([a[::2], fresh])), rng.permutation(fresh), np.repeat(fresh[:50], 2)]
    assert rig.merged(psg.PUSH | psg.PULL, frames, 2, 1) == SORTED
    assert rig.t.info().size == len(a) + len(fresh) and rig.t.info().capacity > cap0
    rig.check()


@pytest.mark.parametrize("general", [False, True], ids=["same_list", "sorted"])
def test_a_frame_4_bytes_off_takes_the_element_path(general):
    """grads of frame 1, then out of frame 2, 4 B into their buffers (16-B rows)."""
    rng = np.random.default_rng(4)
    base = random_keys(rng, 700)
    frames = [rng.choice(base, 900) for _ in range(3)] if general else [base] * 3
    rig = Rig(20, base, True)
    path = SORTED if general else SAME
    assert rig.merged(psg.PUSH | psg.PULL, frames, 1, 0, grad_off=(1,)) == path
    assert rig.merged(psg.PUSH | psg.PULL, frames, 2, 1, out_off=(2,)) == path
    assert rig.merged(psg.PUSH, frames, 3, 2, grad_off=(0, 2)) == path
    assert rig.merged(psg.PUSH | psg.PULL, frames, 4, 3) == path  # and aligned arrays on the same table
    rig.check()


def test_rejections_write_nothing():
    width, end = 20, 1 << 30
    rng = np.random.default_rng(5)
    keys = random_keys(rng, 2000, 0, end - 1)
    fresh = np.setdiff1d(random_keys(rng, 300, 0, end - 1), keys)
    t = psg.Table(psg.F32, width, 0, end, 0)
    t.set_adam(*ADAM)
    t.update(psg.PUSH, dev(keys), dev(synth(len(keys) * width, 1)), None, len(keys), LR, 0)
    before, cap0, size0 = state(t, True), t.info().capacity, t.info().size

    def call(flags, frames, iteration=1, k=None):
        ns = [len(x) for x in frames]
        g = [dev(synth(max(n, 1) * width, 2)) for n in ns]
        o = [psg.DeviceBuffer(max(n, 1) * width * 4) for n in ns]
        if k is not None:
            return psg.lib().psg_table_update_merged(t.h, flags, k, None, None, None, None, LR, iteration, None, None)
        return t.update_merged(flags, [dev(x) for x in frames], g, o, ns, LR, iteration)

    bad = np.uint64(end)
    # a key out of range in the last frame: general lists, and same-list candidates
    mixed = [rng.permutation(np.concatenate([keys[::3], fresh])), rng.permutation(keys),
             rng.permutation(np.concatenate([fresh, [bad]]).astype(np.uint64))]
    asc = np.sort(np.concatenate([keys[::5], fresh]))
    last = asc.copy()
    last[-1] = bad
    for frames in (mixed, [asc, asc, last], [last], [last, last]):
        for flags in (psg.PUSH, psg.PUSH | psg.PULL):
            with pytest.raises(psg.PsgError) as ei:
                call(flags, frames)
            assert ei.value.code == 4, str(ei.value)
    assert_state(t, before, True)
    assert t.info().capacity == cap0 and t.info().size == size0
    # arguments
    for bad_call in (lambda: call(psg.PULL, [asc]), lambda: call(0, [asc]), lambda: call(psg.PUSH, [asc], -1),
                     lambda: t.update_merged(psg.PUSH | psg.PULL, [dev(asc)], [dev(synth(len(asc) * width, 2))], None,
                                             [len(asc)], LR, 0),
                     lambda: t.update_merged(psg.PUSH, [dev(asc)], [None], None, [len(asc)], LR, 0),
                     lambda: t.update_merged(psg.PUSH, [None], [dev(synth(len(asc) * width, 2))], None, [len(asc)],
                                             LR, 0)):
        with pytest.raises(psg.PsgError) as ei:
            bad_call()
        assert ei.value.code == 1, str(ei.value)
    assert call(psg.PUSH, [], k=0) == 1 and call(psg.PUSH, [], k=17) == 1
    h = psg.Table(psg.F16, 4, 0, KMAX, 0)
    with pytest.raises(psg.PsgError) as ei:
        h.update_merged(psg.PUSH, [dev(np.array([3, 3], np.uint64))], [dev(np.ones(8, np.float32))], None, [2], LR, 0)
    assert ei.value.code == 6
    # sum(ns) == 0 is a no-op
    assert t.update_merged(psg.PUSH | psg.PULL, [None, None], [None, None], [None, None], [0, 0], LR, 0) == 0
    assert_state(t, before, True)


@pytest.mark.parametrize("width", [3, 4])
@pytest.mark.parametrize("frames,path", [([[5, 9]], SAME), ([[5, 9], [5, 9]], SAME), ([[9, 5]], SORTED),
                                         ([[9], [5, 5]], SORTED)],
                         ids=["same_k1", "same_k2", "sorted_k1", "sorted_k2"])
def test_the_sum_starts_from_plus_zero_and_the_first_add_is_kept(frames, path, width):
    """Key 5 gets only -0.0f gradients: its sum is 0.0f + -0.0f = +0.0f, so an SGD
    row of -0.0f stays -0.0f ((double)-0.0 - (double)(lr * +0.0f)).  A sum seeded
    with the first occurrence would be -0.0f and turn the row into +0.0f.  The
    table has no call that leaves -0.0f in a row, so the test writes the rows."""
    keys = np.array([5, 9], np.uint64)
    rig = Rig(width, keys, False)
    rig.accumulate(keys, np.zeros(2 * width, np.float32))  # inserts both keys
    minus = np.full(2 * width, -0.0, np.float32)
    dminus = dev(minus)
    psg.memcpy_d2d(rig.t.info().rows, dminus, minus.nbytes)
    psg.device_sync()
    rig.o.rows[:] = -0.0
    kl = [np.array(x, np.uint64) for x in frames]
    ns = [len(x) for x in kl]
    # key 5: -0.0f everywhere; key 9: a real gradient
    grads = [np.where(np.repeat(x == 5, width), np.float32(-0.0), np.float32(0.25)).astype(np.float32) for x in kl]
    outs = [psg.DeviceBuffer(n * width * 4) for n in ns]
    assert rig.t.update_merged(psg.PUSH | psg.PULL, [dev(x) for x in kl], [dev(g) for g in grads], outs, ns, LR,
                               0) == path
    exp, _ = rig.o.merged(kl, grads, LR, 0)
    for o, e, n in zip(outs, exp, ns):
        same(o.download(np.float32, n * width), e)
    rig.check()
    _, rows = rig.t.dump()
    assert np.all(bits(rows[0]) == 0x80000000), rows[0]  # key 5's row is still -0.0f
    assert not np.any(bits(rows[1]) == 0x80000000)


def test_every_occurrence_of_a_pushpull_is_answered_with_the_final_row():
    width = 20
    rng = np.random.default_rng(6)
    pool = random_keys(rng, 200)
    frames = [rng.choice(pool, 500) for _ in range(3)]
    t = psg.Table(psg.F32, width, 0, KMAX, 0)
    outs = [psg.DeviceBuffer(500 * width * 4) for _ in frames]
    t.update_merged(psg.PUSH | psg.PULL, [dev(x) for x in frames], [dev(synth(500 * width, 9 + j)) for j in range(3)],
                    outs, [500] * 3, LR, 0)
    k, rows = t.dump()
    for x, o in zip(frames, outs):
        same(o.download(np.float32, 500 * width).reshape(500, width), rows[np.searchsorted(k, x)])
