"""Bags across servers (psg_route_bags, psg_pool_reduce, csrc/psg_route.hip)
against numpy, and the definition they serve (include/psg.h): a pooled lookup
and a pooled update on range-sharded tables against one table over the whole
range.

References.  psg_route_bags: np.searchsorted on each server's stretch of perm.
psg_pool_reduce: the fold `acc = +0; for s in rank order: acc += P_s; round once`
written in numpy in the accumulator type (f32; f64 for F64).  Every comparison is
bit for bit, through unsigned views, except where the expected value is a NaN
(payloads differ between host and device: only the class is asserted, and where
it occurs).
"""
import numpy as np
import pytest

import psg
import row_specials as rs

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1
SENTINEL = 0xAB
INVALID = 1
DTYPES = {"f32": psg.F32, "f64": psg.F64, "f16": psg.F16, "bf16": psg.BF16}
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
LR = 0.05


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def dev(a):
    return psg.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def ubits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, exp):
    np.testing.assert_array_equal(ubits(got).ravel(), ubits(exp).ravel())


# ---- lists and bags ------------------------------------------------------------------
def ids_of(rng, b, e, servers, per):
    """`per` distinct ids inside each named server's range"""
    out = []
    for s in servers:
        out.append(np.unique(u64(b[s]) + rng.integers(0, int(e[s]) - int(b[s]), per, dtype=np.uint64)))
    return np.concatenate(out)


def skewed(rng, ids, n):
    """n occurrences of ids, a few hot ones named again and again, shuffled"""
    hot = ids[rng.integers(0, len(ids), max(1, len(ids) // 16))]
    pick = np.where(rng.random(n) < 0.4, hot[rng.integers(0, len(hot), n)], ids[rng.integers(0, len(ids), n)])
    return u64(pick)


def bag_offsets(rng, nb):
    """nb bags of 0-40 ids: runs of empty bags, an empty first and last bag"""
    lens = rng.integers(0, 41, nb)
    lens[rng.random(nb) < 0.15] = 0
    if nb >= 8:
        at = int(rng.integers(1, nb - 6))
        lens[at:at + 5] = 0
    if nb >= 3:
        lens[0] = lens[-1] = 0
    if lens.sum() == 0:
        lens[nb // 2] = 17
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def np_route(keys, e):
    owner = np.searchsorted(e, keys, "right")
    perm = np.argsort(owner, kind="stable").astype(np.uint32)
    pos = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=len(e)))]).astype(np.uint64)
    return owner, perm, pos


def np_route_bags(offsets, perm, pos):
    return np.stack([np.searchsorted(perm[int(pos[s]):int(pos[s + 1])], offsets, "left")
                     for s in range(len(pos) - 1)]).astype(np.uint64)


def gpu_route(keys, b, e):
    """(device keys as sent, device perm or None, key_pos)"""
    n = len(keys)
    dk, dr, dp = dev(keys), dev(np.zeros(n, np.uint64)), dev(np.zeros(n, np.uint32))
    kp, ident = psg.route(dk, n, b, e, dr, dp)
    return (dk, None, kp) if ident else (dr, dp, kp)


# ---- psg_route_bags ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["shuffled", "sorted", "gap"])
@pytest.mark.parametrize("nb", [1, 257, 1025])
@pytest.mark.parametrize("ns", [1, 2, 3, 64])
def test_route_bags_is_the_lower_bound_on_every_stretch(ns, nb, kind):
    rng = np.random.default_rng(100 * ns + nb + len(kind))
    b, e = psg.server_ranges(ns)
    owners = [s for s in range(ns) if not (kind == "gap" and s == 1)]  # gap: server 1 owns no id
    offsets = bag_offsets(rng, nb)
    n = int(offsets[-1])
    keys = skewed(rng, ids_of(rng, b, e, owners, max(2, 300 // len(owners))), n)
    if kind == "sorted":
        keys = np.sort(keys)
    owner, perm, pos = np_route(keys, e)
    if kind == "gap" and ns > 1:
        assert pos[1] == pos[2]
    exp = np_route_bags(offsets, perm, pos)
    _, dp, kp = gpu_route(keys, b, e)
    np.testing.assert_array_equal(kp, pos)
    assert (dp is None) == bool(np.all(np.diff(owner) >= 0))
    if kind == "sorted":
        assert dp is None
        clamp = np.stack([np.clip(offsets, pos[s], pos[s + 1]) - pos[s] for s in range(ns)])
        np.testing.assert_array_equal(exp, clamp)  # the identity route's closed form
    do = dev(offsets)
    dso = dev(np.full(ns * (nb + 1), SENTINEL, dtype=np.uint64))
    psg.route_bags(do, nb, dp, n, kp, dso)
    got = dso.download(np.uint64, ns * (nb + 1)).reshape(ns, nb + 1)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(got[:, -1], np.diff(pos))  # every stretch ends at its length
    np.testing.assert_array_equal(do.download(np.uint64, nb + 1), offsets)  # never written


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("rule", ["first", "order", "last"])
def test_route_bags_refuses_a_broken_offsets_rule_and_writes_nothing(rule, identity):
    rng = np.random.default_rng(5)
    ns, nb = 3, 257
    b, e = psg.server_ranges(ns)
    offsets = bag_offsets(rng, nb)
    n = int(offsets[-1])
    keys = skewed(rng, ids_of(rng, b, e, range(ns), 50), n)
    if identity:
        keys = np.sort(keys)
    _, dp, kp = gpu_route(keys, b, e)
    assert (dp is None) == identity
    bad = offsets.copy()
    if rule == "first":  # starts at 1, still ascends to n
        bad = np.maximum(offsets, np.uint64(1))
    elif rule == "order":  # one offset above its successor, deep inside the array
        mid = int(np.flatnonzero(np.diff(offsets) > 1)[3]) + 1
        bad[mid] = offsets[mid + 1] + np.uint64(1)
    else:  # ascends from 0, ends one past n
        bad[-1] = n + 1
    dso = dev(np.full(ns * (nb + 1), SENTINEL, dtype=np.uint64))
    with pytest.raises(psg.PsgError) as ei:
        psg.route_bags(dev(bad), nb, dp, n, kp, dso)
    assert ei.value.code == INVALID and "offsets must start at 0" in str(ei.value)
    assert np.all(dso.download(np.uint64, ns * (nb + 1)) == SENTINEL)
    # the next call on this thread is served: the flag does not stick
    psg.route_bags(dev(offsets), nb, dp, n, kp, dso)
    np.testing.assert_array_equal(dso.download(np.uint64, ns * (nb + 1)).reshape(ns, nb + 1),
                                  np_route_bags(offsets, np_route(keys, e)[1], kp))


# ---- psg_pool_reduce -----------------------------------------------------------------
def to_acc(dtype, stored):
    if dtype == psg.F64:
        return np.asarray(stored, dtype=np.float64)
    if dtype == psg.BF16:
        return (ubits(stored).astype(np.uint32) << np.uint32(16)).view(np.float32)
    return np.asarray(stored).astype(np.float32)


def from_acc(dtype, acc):
    if dtype in (psg.F32, psg.F64):
        return ubits(acc)
    if dtype == psg.F16:
        with np.errstate(over="ignore"):
            return acc.astype(np.float16).view(np.uint16)
    u = acc.view(np.uint32).astype(np.uint64)  # BF16: the rounding on the f32 bits (finite sums)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def np_fold(dtype, partials):
    acc = np.zeros(len(partials[0]), dtype=np.float64 if dtype == psg.F64 else np.float32)
    with np.errstate(all="ignore"):
        for p in partials:
            acc = acc + to_acc(dtype, p)
    return from_acc(dtype, acc)


def real_values(rng, dtype, count):
    x = (rng.uniform(-4, 4, count) * rng.choice([1.0, 1.0, 0.001, 8.0], count)).astype(np.float32)
    if dtype == psg.F32:
        return x
    if dtype == psg.F64:
        return rng.uniform(-4, 4, count) * rng.choice([1.0, 1e-9, 1e6], count)
    if dtype == psg.F16:
        return x.astype(np.float16)
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def reduce_on_gpu(dtype, partials, shift=0):
    """partials: arrays as stored; shift: elements every pointer sits off its allocation"""
    count = len(partials[0])
    es = partials[0].dtype.itemsize
    pad = np.zeros(shift, dtype=partials[0].dtype)
    bufs = [dev(np.concatenate([pad, p])) for p in partials]
    out = dev(np.full((count + shift + 1) * es, SENTINEL, dtype=np.uint8))
    psg.pool_reduce(out.ptr + shift * es, [x.ptr + shift * es for x in bufs], count, dtype)
    psg.device_sync()
    raw = out.download(np.uint8, (count + shift + 1) * es)
    assert np.all(raw[:shift * es] == SENTINEL) and np.all(raw[(shift + count) * es:] == SENTINEL), "wrote outside out"
    for x, p in zip(bufs, partials):
        same(x.download(p.dtype, count, offset=shift * es), p)  # the partials are only read
    return raw[shift * es:(shift + count) * es].view(ubits(partials[0]).dtype)


@pytest.mark.parametrize("count", [1, 3, 4099, 4112])
@pytest.mark.parametrize("k", [1, 2, 3, 64])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_pool_reduce_is_the_fold_in_list_order(name, k, count):
    dtype = DTYPES[name]
    rng = np.random.default_rng(1000 * k + count + dtype)
    partials = [real_values(rng, dtype, count) for _ in range(k)]
    exp = np_fold(dtype, partials)
    for shift in (0, 1):  # 16-B aligned (vectors when count allows), and one element off
        np.testing.assert_array_equal(reduce_on_gpu(dtype, partials, shift), exp, err_msg=f"shift={shift}")


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_pool_reduce_on_signs_and_infinities(name):
    dtype = DTYPES[name]
    a, b = rs.pairs(dtype)
    zero = np.zeros_like(a)
    exp = rs.np_add(dtype, rs.np_add(dtype, zero, a), b)  # (+0 + a) + b; the halves' inner sum is exact
    nan = rs.inf_pairs_mask(dtype, a, b)
    assert nan.sum() == rs.N_NAN
    np.testing.assert_array_equal(rs.nan_mask(dtype, exp), nan)
    pa, pb = rs.storage(dtype, a), rs.storage(dtype, b)
    for shift in (0, 1):
        got = reduce_on_gpu(dtype, [pa, pb], shift)
        np.testing.assert_array_equal(rs.nan_mask(dtype, got), nan)  # (+inf, -inf): NaN, by class
        np.testing.assert_array_equal(got[~nan], exp[~nan])
    # -0 alone, and any number of them, give +0: the sum starts from +0
    neg0 = rs.storage(dtype, np.full(19, rs.specials(dtype)["-0"], dtype=rs.UINT[dtype]))
    for k in (1, 3):
        assert np.all(reduce_on_gpu(dtype, [neg0] * k) == 0)


def test_pool_reduce_of_halves_overflows_only_at_the_final_rounding():
    f16 = lambda *v: np.array(v, dtype=np.float16)
    #          stays finite in f32   == max      the tie: inf   -max      -inf     back inside
    p0 = f16(60000, 60000, 60000, -60000, -60000, 60000, -60000)
    p1 = f16(60000, 5504, 5520, -5504, -5520, 60000, -60000)
    p2 = f16(-60000, 0, 0, 0, 0, -60000 - 32, 60000 + 32)
    exp = np_fold(psg.F16, [p0, p1, p2])
    np.testing.assert_array_equal(exp.view(np.float16), f16(60000, 65504, np.inf, -65504, -np.inf, 59968, -59968))
    np.testing.assert_array_equal(reduce_on_gpu(psg.F16, [p0, p1, p2]), exp)
    np.testing.assert_array_equal(reduce_on_gpu(psg.F16, [np.tile(p, 8) for p in (p0, p1, p2)]), np.tile(exp, 8))


# ---- sharded against whole -------------------------------------------------------------
class Sharded:
    """ns tables over psg.server_ranges(ns) and one over the whole range, a
    shuffled skewed list in bags, routed on the GPU."""

    def __init__(self, ns, width, integer_rows, adam=False, seed=0):
        rng = np.random.default_rng(seed)
        self.ns, self.w, self.rng = ns, width, rng
        self.b, self.e = psg.server_ranges(ns)
        self.shards = [psg.Table(psg.F32, width, int(self.b[s]), int(self.e[s]), 0) for s in range(ns)]
        self.whole = psg.Table(psg.F32, width, int(self.b[0]), int(self.e[-1]), 0)
        for t in self.shards + [self.whole]:
            if adam:
                t.set_adam(*ADAM)
        ids = np.sort(ids_of(rng, self.b, self.e, range(ns), 30))
        present = ids[rng.random(len(ids)) < 0.8]  # the rest are absent: a lookup skips them, an update inserts them
        if integer_rows:
            rows = rng.integers(-64, 65, (len(present), width)).astype(np.float32)
        else:
            rows = real_values(rng, psg.F32, len(present) * width).reshape(len(present), width)
        self.rows = {int(k): rows[j] for j, k in enumerate(present)}
        owner = np.searchsorted(self.e, present, "right")
        for s, t in enumerate(self.shards):
            m = owner == s
            t.assign(dev(present[m]), dev(rows[m]), int(m.sum()))
        self.whole.assign(dev(present), dev(rows), len(present))
        self.nb = 97
        self.offsets = bag_offsets(rng, self.nb)
        self.n = int(self.offsets[-1])
        self.keys = skewed(rng, ids, self.n)
        self.dkeys, self.dperm, self.kp = gpu_route(self.keys, self.b, self.e)
        assert self.dperm is not None
        self.dso = dev(np.zeros(ns * (self.nb + 1), np.uint64))
        psg.route_bags(dev(self.offsets), self.nb, self.dperm, self.n, self.kp, self.dso)

    def stretch(self, s):
        """(device keys, device offsets, n) of server s"""
        return self.dkeys.ptr + int(self.kp[s]) * 8, self.dso.ptr + s * (self.nb + 1) * 8, int(self.kp[s + 1] - self.kp[s])

    def forward(self):
        count = self.nb * self.w
        frames = []
        for s, t in enumerate(self.shards):
            k, o, n = self.stretch(s)
            if n == 0:
                continue  # owns none of the list's ids: skipped, as the definition allows
            frames.append(psg.DeviceBuffer(count * 4))
            t.lookup_pooled(k, o, frames[-1], n, self.nb)
        out = psg.DeviceBuffer(count * 4)
        psg.pool_reduce(out, frames, count, psg.F32)
        psg.device_sync()
        return out.download(np.float32, count).reshape(self.nb, self.w)

    def forward_ref(self):
        """the definition in numpy: per server the bag's present rows in arrival order from +0, then the servers in rank order"""
        owner = np.searchsorted(self.e, self.keys, "right")
        out = np.zeros((self.nb, self.w), np.float32)
        for bag in range(self.nb):
            lo, hi = int(self.offsets[bag]), int(self.offsets[bag + 1])
            acc = np.zeros(self.w, np.float32)
            for s in range(self.ns):
                part = np.zeros(self.w, np.float32)
                for p in range(lo, hi):
                    if owner[p] == s and int(self.keys[p]) in self.rows:
                        part = part + self.rows[int(self.keys[p])]
                acc = acc + part
            out[bag] = acc
        return out


@pytest.mark.parametrize("width", [3, 4, 64])
@pytest.mark.parametrize("ns", [2, 3])
def test_sharded_forward_is_the_definition(ns, width):
    sh = Sharded(ns, width, integer_rows=False, seed=10 * ns + width)
    same(sh.forward(), sh.forward_ref())


@pytest.mark.parametrize("width", [3, 4, 64])
@pytest.mark.parametrize("ns", [2, 3])
def test_sharded_forward_on_integer_rows_is_the_whole_table(ns, width):
    sh = Sharded(ns, width, integer_rows=True, seed=20 * ns + width)
    got = sh.forward()
    same(got, sh.forward_ref())
    out = psg.DeviceBuffer(sh.nb * width * 4)
    sh.whole.lookup_pooled(dev(sh.keys), dev(sh.offsets), out, sh.n, sh.nb)
    same(got, out.download(np.float32, sh.nb * width))  # every order of adds is exact


@pytest.mark.parametrize("opt", ["sgd", "adam0", "adam7"])
@pytest.mark.parametrize("width", [3, 4, 64])
@pytest.mark.parametrize("ns", [2, 3])
def test_sharded_backward_is_the_whole_table(ns, width, opt):
    adam, it = opt != "sgd", 7 if opt == "adam7" else 0
    sh = Sharded(ns, width, integer_rows=False, adam=adam, seed=30 * ns + width + it)
    grads = dev(real_values(sh.rng, psg.F32, sh.nb * width))
    before = sum(t.info().size for t in sh.shards)
    for s, t in enumerate(sh.shards):
        k, o, n = sh.stretch(s)
        t.update_pooled(k, o, grads, n, sh.nb, LR, it)
    sh.whole.update_pooled(dev(sh.keys), dev(sh.offsets), grads, sh.n, sh.nb, LR, it)
    dumps = [t.dump() for t in sh.shards]
    wk, wr = sh.whole.dump()
    assert len(wk) > before, "the update inserted no id"
    np.testing.assert_array_equal(np.concatenate([d[0] for d in dumps]), wk)
    same(np.concatenate([d[1] for d in dumps]), wr)
    if adam:
        moms = [t.dump_moments() for t in sh.shards if t.info().size]
        for j, whole in enumerate(sh.whole.dump_moments()):
            same(np.concatenate([m[j] for m in moms]), whole)
