"""The worker's routing pass and its row copies (psg_route, psg_rows_gather,
psg_rows_scatter, csrc/psg_route.hip) against numpy, and the definition they
serve: a list routed to two half-range tables gives, bit for bit, what one
table over the whole range gives for the list as it is.

Route reference: owner = searchsorted(ends, keys, 'right'),
perm_ref = argsort(owner, kind='stable').  Row copies: numpy fancy indexing,
byte for byte.
"""
import numpy as np
import pytest

import psg

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 20011, 300001]
SERVERS = [1, 2, 3, 8, psg.ROUTE_MAX_SERVERS]
SENTINEL = 0xAB


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def dev(a):
    return psg.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def in_range(rng, lo, hi, n):
    """n keys in [lo, hi) (uint64 bounds)."""
    return u64(lo) + rng.integers(0, int(hi) - int(lo), n, dtype=np.uint64)


# ---- the lists --------------------------------------------------------------------
def shuffled(rng, n, b, e):
    return rng.integers(0, KMAX, n, dtype=np.uint64)


def first_server(rng, n, b, e):
    return in_range(rng, b[0], e[0], n)


def last_server(rng, n, b, e):
    return in_range(rng, b[-1], e[-1], n)


def one_key(rng, n, b, e):
    return np.repeat(rng.integers(0, KMAX, 1, dtype=np.uint64), n)


def alternating(rng, n, b, e):
    o = np.arange(n) % len(b)
    return b[o] + rng.integers(0, int(e[0] - b[0]), n, dtype=np.uint64)


def edges(rng, n, b, e):
    pool = np.unique(np.concatenate([b, e - np.uint64(1), u64([0, KMAX - 1])]))
    return rng.permutation(pool[np.arange(n) % len(pool)])


LISTS = {"shuffled": shuffled, "first_server": first_server, "last_server": last_server, "one_key": one_key,
         "alternating": alternating, "edges": edges}


def route(keys, b, e):
    """(routed, perm, key_pos, identity); routed / perm start sentinel-filled."""
    n = len(keys)
    dk = dev(keys)
    dr = dev(np.full(n, SENTINEL, dtype=np.uint64))
    dp = dev(np.full(n, SENTINEL, dtype=np.uint32))
    kp, ident = psg.route(dk, n, b, e, dr, dp)
    np.testing.assert_array_equal(dk.download(np.uint64, n), keys)  # the caller's keys are never written
    return dr, dr.download(np.uint64, n), dp.download(np.uint32, n), kp, ident


@pytest.mark.parametrize("kind", sorted(LISTS))
@pytest.mark.parametrize("ns", SERVERS)
def test_route_is_the_stable_partition_by_owner(ns, kind):
    b, e = psg.server_ranges(ns)
    rng = np.random.default_rng(1000 * ns + len(kind))
    for n in SIZES:
        keys = LISTS[kind](rng, n, b, e)
        owner = np.searchsorted(e, keys, "right")
        perm_ref = np.argsort(owner, kind="stable")
        pos_ref = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=ns))]).astype(np.uint64)
        dr, routed, perm, kp, ident = route(keys, b, e)
        np.testing.assert_array_equal(kp, pos_ref, err_msg=f"n={n}")
        assert ident == bool(np.all(np.diff(owner) >= 0)), n
        if ident:
            assert np.all(routed == SENTINEL) and np.all(perm == SENTINEL), n
            dr = dev(keys)  # the caller sends its own array
        else:
            np.testing.assert_array_equal(perm, perm_ref, err_msg=f"n={n}")
            np.testing.assert_array_equal(routed, keys[perm_ref], err_msg=f"n={n}")
        sp, _ = psg.slice_keys(dr, n, b, e)
        np.testing.assert_array_equal(sp, pos_ref, err_msg=f"psg_slice on the routed list, n={n}")


@pytest.mark.parametrize("kind", ["sorted", "nondescending", "partitioned"])
def test_a_partitioned_list_is_left_where_it_is(kind):
    rng = np.random.default_rng(7)
    b, e = psg.server_ranges(3)
    for n in (65, 4097, 20011):
        if kind == "sorted":
            keys = np.unique(rng.integers(0, KMAX, n, dtype=np.uint64))
        elif kind == "nondescending":
            keys = np.sort(rng.choice(rng.integers(0, KMAX, n // 8 + 1, dtype=np.uint64), n))
        else:  # by owner, shuffled inside every stretch
            keys = np.concatenate([rng.permutation(in_range(rng, b[s], e[s], n // 3 + s)) for s in range(3)])
            assert np.any(np.diff(keys.astype(np.float64)) < 0)
        _, routed, perm, kp, ident = route(keys, b, e)
        assert ident
        assert np.all(routed == SENTINEL) and np.all(perm == SENTINEL)
        np.testing.assert_array_equal(kp, np.searchsorted(np.searchsorted(e, keys, "right"), np.arange(4)))


def test_a_key_outside_the_ranges_fails_the_call():
    rng = np.random.default_rng(8)
    b, e = psg.server_ranges(4)
    keys = rng.integers(0, KMAX, 5000, dtype=np.uint64)
    keys[3333] = e[-1]  # at the last range's end
    with pytest.raises(psg.PsgError) as ei:
        route(keys, b, e)
    assert ei.value.code == 4
    pb, pe = b[1:3].copy(), e[1:3].copy()  # a partial range set
    inside = in_range(rng, pb[0], pe[1], 5000)
    kp = route(inside, pb, pe)[3]
    assert kp[2] == 5000
    inside[77] = pb[0] - np.uint64(1)  # just below the first range
    with pytest.raises(psg.PsgError) as ei:
        route(inside, pb, pe)
    assert ei.value.code == 4


# ---- gather and scatter -------------------------------------------------------------
ROW_BYTES = [2, 4, 6, 12, 16, 48, 80, 1040, 16384, 32768]
ROWS = [1, 65, 4097]
CANARY = 2  # rows past n


@pytest.fixture(scope="module")
def byte_pool():
    return np.random.default_rng(11).integers(0, 256, (max(ROWS) + CANARY) * max(ROW_BYTES), dtype=np.uint8)


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "offset4"])
@pytest.mark.parametrize("rb", ROW_BYTES)
def test_gather_and_scatter_match_fancy_indexing(byte_pool, rb, offset):
    rng = np.random.default_rng(rb + offset)
    for n in ROWS:
        total = (n + CANARY) * rb
        x = byte_pool[:total].reshape(n + CANARY, rb)
        perm = rng.permutation(n).astype(np.uint32)
        dperm = dev(perm)
        src = psg.DeviceBuffer(total + 16)
        src.upload(x.ravel(), offset=offset)

        def run(fn, source_ptr):
            dst = psg.DeviceBuffer(total + 16)
            dst.upload(np.full(total + 16, SENTINEL, dtype=np.uint8))
            fn(dst.ptr + offset, source_ptr, dperm, n, rb)
            psg.device_sync()
            whole = dst.download(np.uint8, total + 16)
            assert np.all(whole[:offset] == SENTINEL) and np.all(whole[offset + n * rb:] == SENTINEL), (n, rb)
            return dst, whole[offset:offset + n * rb].reshape(n, rb)

        gathered_dev, gathered = run(psg.rows_gather, src.ptr + offset)
        np.testing.assert_array_equal(gathered, x[:n][perm], err_msg=f"gather n={n}")
        _, scattered = run(psg.rows_scatter, src.ptr + offset)
        exp = np.empty((n, rb), dtype=np.uint8)
        exp[perm] = x[:n]
        np.testing.assert_array_equal(scattered, exp, err_msg=f"scatter n={n}")
        _, back = run(psg.rows_scatter, gathered_dev.ptr + offset)
        np.testing.assert_array_equal(back, x[:n], err_msg=f"scatter(gather(x)) n={n}")


# ---- the definition -----------------------------------------------------------------
HALF = KMAX // 2
LR = float(np.float32(0.05))
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)


@pytest.fixture(scope="module")
def minibatch():
    """4097 occurrences of 500 keys over the whole key space, shuffled."""
    rng = np.random.default_rng(21)
    distinct = np.unique(rng.integers(0, KMAX, 500, dtype=np.uint64))
    keys = rng.choice(distinct, 4097)
    assert (keys < HALF).any() and (keys >= HALF).any()
    return keys


class Routed:
    """A list routed over the two half ranges, its values gathered."""

    def __init__(self, keys, vals, w):
        self.n, self.w = len(keys), w
        b, e = psg.server_ranges(2)
        assert e[0] == HALF
        self.keys = dev(keys)
        self.rkeys = psg.DeviceBuffer(self.n * 8)
        self.perm = psg.DeviceBuffer(self.n * 4)
        self.pos, ident = psg.route(self.keys, self.n, b, e, self.rkeys, self.perm)
        assert not ident
        self.vals = dev(vals)
        self.rvals = psg.DeviceBuffer(self.n * w * 4)
        psg.rows_gather(self.rvals, self.vals, self.perm, self.n, w * 4)
        self.rout = psg.DeviceBuffer(self.n * w * 4)

    def stretch(self, s):
        """(keys, vals, out, count) of server s"""
        lo, cnt = int(self.pos[s]), int(self.pos[s + 1] - self.pos[s])
        return self.rkeys.ptr + lo * 8, self.rvals.ptr + lo * self.w * 4, self.rout.ptr + lo * self.w * 4, cnt

    def reply(self):
        out = psg.DeviceBuffer(self.n * self.w * 4)
        psg.rows_scatter(out, self.rout, self.perm, self.n, self.w * 4)
        psg.device_sync()
        return out.download(np.float32, self.n * self.w)


@pytest.mark.parametrize("op", ["handle_any", "update_any", "update_merged"])
@pytest.mark.parametrize("w", [3, 4, 64])
def test_two_half_range_tables_give_what_one_table_gives(minibatch, w, op):
    keys = minibatch
    n = len(keys)
    rng = np.random.default_rng(w)
    vals = rng.uniform(-1, 1, n * w).astype(np.float32)
    seed = rng.uniform(-1, 1, n * w).astype(np.float32)
    pair = [psg.Table(psg.F32, w, 0, HALF, 0), psg.Table(psg.F32, w, HALF, KMAX, 0)]
    whole = psg.Table(psg.F32, w, 0, KMAX, 0)
    flags = psg.PUSH | psg.PULL
    if op != "handle_any":
        for t in pair + [whole]:
            t.set_adam(*ADAM)
    # rows to start from: an accumulate Push of the list, routed as well
    r0 = Routed(keys, seed, w)
    for s, t in enumerate(pair):
        k, v, _, cnt = r0.stretch(s)
        t.handle_any(psg.PUSH, k, v, None, cnt)
    whole.handle_any(psg.PUSH, r0.keys, r0.vals, None, n)

    out = psg.DeviceBuffer(n * w * 4)
    if op == "update_merged":
        cut = 2000
        frames = [Routed(keys[:cut], vals[:cut * w], w), Routed(keys[cut:], vals[cut * w:], w)]
        for s, t in enumerate(pair):
            st = [f.stretch(s) for f in frames]
            t.update_merged(flags, [x[0] for x in st], [x[1] for x in st], [x[2] for x in st], [x[3] for x in st],
                            LR, 7)
        got = np.concatenate([f.reply() for f in frames])
        whole.update_merged(flags, [f.keys for f in frames], [f.vals for f in frames],
                            [out.ptr, out.ptr + cut * w * 4], [cut, n - cut], LR, 7)
    else:
        r = Routed(keys, vals, w)
        for s, t in enumerate(pair):
            k, v, o, cnt = r.stretch(s)
            if op == "handle_any":
                t.handle_any(flags, k, v, o, cnt)
            else:
                t.update_any(flags, k, v, o, cnt, LR, 7)
        got = r.reply()
        if op == "handle_any":
            whole.handle_any(flags, r.keys, r.vals, out, n)
        else:
            whole.update_any(flags, r.keys, r.vals, out, n, LR, 7)
    psg.device_sync()
    exp = out.download(np.float32, n * w)
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg="replies")
    dumps = [t.dump() for t in pair]
    wk, wr = whole.dump()
    np.testing.assert_array_equal(np.concatenate([d[0] for d in dumps]), wk)
    np.testing.assert_array_equal(np.concatenate([d[1] for d in dumps]).view(np.uint32), wr.view(np.uint32),
                                  err_msg="rows")
    if op != "handle_any":
        moms = [t.dump_moments() for t in pair]
        wm, wv = whole.dump_moments()
        np.testing.assert_array_equal(np.concatenate([m[0] for m in moms]).view(np.uint64), wm.view(np.uint64))
        np.testing.assert_array_equal(np.concatenate([m[1] for m in moms]).view(np.uint64), wv.view(np.uint64))
    for t in pair + [whole]:
        t.close()
