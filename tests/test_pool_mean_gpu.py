"""A mean over a sharded bag (psg_pool_reduce_mean, psg_pool_scale_mean,
csrc/psg_route.hip) against a numpy mirror, and the two equivalences with the
one-table calls that the worker's mean calls rest on (include/psg.h).

The mirror.  psg_pool_reduce_mean: `acc = +0; for s in list order: acc += P_s;
out = acc / L_b` in the accumulator type (f32; f64 for F64), an empty bag +0.
f32 and f64 adds and divisions are correctly rounded on both sides, so the
mirror is exact; halves are widened, computed in f32 and rounded once
(row_model.to_acc / from_acc).  psg_pool_scale_mean: one f32 division.  Every
comparison is bit for bit through unsigned views, except where the expected
value is a NaN (payloads differ between host and device: the class is asserted,
and where it occurs).
"""
import numpy as np
import pytest

import psg
import row_model as rm
import row_specials as rs

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1
SENTINEL = 0xAB
DTYPES = {"f32": psg.F32, "f64": psg.F64, "f16": psg.F16, "bf16": psg.BF16}
ESIZE = {psg.F32: 4, psg.F64: 8, psg.F16: 2, psg.BF16: 2}
# per dtype: widths whose rows are whole 16-B vectors (a vector inside one bag),
# and widths where a vector would straddle two bags (the element path)
WIDTHS = {"f32": (4, 20, 1, 3), "f64": (2, 1), "f16": (8, 4, 5), "bf16": (8, 4, 5)}
CASES = [(name, w) for name in sorted(WIDTHS) for w in WIDTHS[name]]
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
LR = 0.05


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def dev(a):
    return psg.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def stored(dtype, f):
    """f32 / f64 values -> the elements as memory holds them (halves: uint16 bits)"""
    if dtype == psg.F64:
        return np.asarray(f, dtype=np.float64)
    f = np.asarray(f, dtype=np.float32)
    if dtype == psg.F32:
        return f
    if dtype == psg.F16:
        with np.errstate(over="ignore"):
            return f.astype(np.float16).view(np.uint16)
    return (f.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def ubits(dtype, a):
    return np.ascontiguousarray(a).view(rs.UINT[dtype])


def bag_lengths(nb):
    """lengths 0 (first, last and in the middle), 1, 3 and 7; neighbours differ"""
    if nb == 1:
        return np.array([3], dtype=np.uint64)
    lens = np.array([(0, 7, 1, 0, 3)[b % 5] for b in range(nb)], dtype=np.uint64)
    lens[0] = lens[-1] = 0
    return lens


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def real_values(rng, dtype, count):
    x = rng.uniform(-4, 4, count) * rng.choice([1.0, 1.0, 0.001, 8.0], count)
    if dtype == psg.F64:
        x = rng.uniform(-4, 4, count) * rng.choice([1.0, 1e-9, 1e6], count)
    return stored(dtype, x)


def np_reduce_mean(dtype, partials, lens, width):
    """bit patterns of the definition"""
    acc_t = np.float64 if dtype == psg.F64 else np.float32
    acc = np.zeros(len(partials[0]), dtype=acc_t)
    L = np.repeat(lens.astype(np.uint32), width)  # read as 32 bits, then converted round-to-nearest
    with np.errstate(all="ignore"):
        for p in partials:
            acc = acc + rm.to_acc(dtype, p)
        q = np.where(L > 0, acc / np.where(L > 0, L, 1).astype(acc_t), acc_t(0.0)).astype(acc_t)
        return ubits(dtype, rm.from_acc(dtype, q))


def reduce_mean_on_gpu(dtype, partials, lens, width, shift_out=0, shift_part=None):
    """partials: arrays as stored; shift_out: elements out sits off its allocation;
    shift_part: the one partial that sits one element off its own"""
    nb, es, count = len(lens), ESIZE[dtype], len(partials[0])
    assert count == nb * width
    pad = np.zeros(1, dtype=partials[0].dtype)
    sh = [1 if j == shift_part else 0 for j in range(len(partials))]
    bufs = [dev(np.concatenate([pad[:s], p])) for s, p in zip(sh, partials)]
    out = dev(np.full((count + shift_out + 1) * es, SENTINEL, dtype=np.uint8))
    psg.pool_reduce_mean(out.ptr + shift_out * es, [x.ptr + s * es for x, s in zip(bufs, sh)], dev(offsets_of(lens)), nb,
                         width, dtype)
    psg.device_sync()
    raw = out.download(np.uint8, (count + shift_out + 1) * es)
    assert np.all(raw[:shift_out * es] == SENTINEL) and np.all(raw[(shift_out + count) * es:] == SENTINEL), "wrote outside out"
    for x, s, p in zip(bufs, sh, partials):  # the partials are only read
        np.testing.assert_array_equal(ubits(dtype, x.download(p.dtype, count, offset=s * es)), ubits(dtype, p))
    return raw[shift_out * es:(shift_out + count) * es].view(rs.UINT[dtype])


def check_reduce_mean(dtype, partials, lens, width, **kw):
    exp = np_reduce_mean(dtype, partials, lens, width)
    got = reduce_mean_on_gpu(dtype, partials, lens, width, **kw)
    nan = rs.nan_mask(dtype, exp)
    np.testing.assert_array_equal(rs.nan_mask(dtype, got), nan, err_msg=str(kw))
    np.testing.assert_array_equal(got[~nan], exp[~nan], err_msg=str(kw))
    return got, nan


# ---- psg_pool_reduce_mean --------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 64])
@pytest.mark.parametrize("name,width", CASES)
def test_reduce_mean_is_the_fold_divided_once(name, width, k):
    dtype = DTYPES[name]
    for nb in (1, 5, 257):
        rng = np.random.default_rng(1000 * k + 10 * nb + width + dtype)
        lens = bag_lengths(nb)
        partials = [real_values(rng, dtype, nb * width) for _ in range(k)]
        # aligned (vectors when a row is whole vectors); out, then one partial, one element off
        for kw in ({}, {"shift_out": 1}, {"shift_part": k - 1}):
            got, nan = check_reduce_mean(dtype, partials, lens, width, **kw)
            assert not nan.any()
            empty = np.repeat(lens == 0, width)
            assert np.all(got[empty] == 0), "an empty bag is +0"


@pytest.mark.parametrize("name,width", CASES)
def test_reduce_mean_of_one_empty_bag_is_plus_zero_whatever_the_partials_hold(name, width):
    dtype = DTYPES[name]
    nan_row = np.full(width, rs.specials(dtype)["+inf"] | 1, dtype=rs.UINT[dtype]).view(rs.STORAGE[dtype])
    got = reduce_mean_on_gpu(dtype, [nan_row, nan_row], np.zeros(1, np.uint64), width)
    assert np.all(got == 0)


@pytest.mark.parametrize("name,width", CASES)
def test_reduce_mean_on_infinities_a_nan_minus_zero_and_subnormal_quotients(name, width):
    dtype = DTYPES[name]
    pats = rs.specials(dtype)
    lens = np.array([0, 7, 3, 1, 0, 7, 3, 0], dtype=np.uint64)
    nb = len(lens)
    row = lambda pat: np.full(width, pats[pat], dtype=rs.UINT[dtype])
    #          empty    +inf       -inf + +inf  -0 alone  empty    minsub/7     minnorm/3     empty
    p0 = [row("+0"), row("+inf"), row("-inf"), row("-0"), row("one"), row("+minsub"), row("-minnorm"), row("-0")]
    p1 = [row("+0"), row("one"), row("+inf"), row("-0"), row("+inf"), row("+0"), row("+0"), row("+0")]
    p0 = np.concatenate(p0).view(rs.STORAGE[dtype])
    p1 = np.concatenate(p1).view(rs.STORAGE[dtype])
    for kw in ({}, {"shift_out": 1}):
        got, nan = check_reduce_mean(dtype, [p0, p1], lens, width, **kw)
        g = got.reshape(nb, width)
        assert np.all(nan.reshape(nb, width)[2]) and nan.sum() == width  # (-inf) + (+inf): the one NaN row
        assert np.all(g[1] == pats["+inf"])
        assert np.all(g[3] == 0)  # -0 rows fold to +0: the sum starts from +0
        assert np.all(g[0] == 0) and np.all(g[4] == 0) and np.all(g[7] == 0)  # empty: +0, also over an inf partial
    # a NaN in one partial reaches exactly its own elements
    p2 = p1.copy()
    ubits(dtype, p2)[width:2 * width] = pats["+inf"] | 1
    got, nan = check_reduce_mean(dtype, [p0, p2], lens, width)
    assert np.all(nan.reshape(nb, width)[1]) and nan.sum() == 2 * width
    # more quotients in and just above the subnormals, each rounded once
    tiny = np.array([pats[n] for n in ("+minsub", "maxsub", "+minnorm", "s", "-minnorm")], dtype=rs.UINT[dtype])
    lens5 = np.array([7, 3, 7, 3, 7], dtype=np.uint64)
    check_reduce_mean(dtype, [np.repeat(tiny, width).view(rs.STORAGE[dtype])], lens5, width)


def test_reduce_mean_converts_a_length_of_2_24_plus_1_to_nearest():
    # only the offsets hold the length; 2^24 + 1 is a tie in f32 and rounds to the even 2^24
    lens = np.array([(1 << 24) + 1, 3], dtype=np.uint64)
    assert np.float32(np.uint32(lens[0])) == np.float32(1 << 24)
    for name, width in (("f32", 4), ("f32", 3), ("f16", 8), ("f64", 2)):
        dtype = DTYPES[name]
        x = stored(dtype, np.tile([float(3 << 24), 1.0, float((1 << 24) + 2), 5.0], 2 * width)[:2 * width])
        got, _ = check_reduce_mean(dtype, [x], lens, width)
        if name == "f32":
            assert got.view(np.float32)[0] == np.float32(3.0)


# ---- psg_pool_scale_mean ---------------------------------------------------------------
def scale_mean_on_gpu(grads, lens, width, shift_dst=0, shift_grads=0):
    nb, count = len(lens), len(grads)
    g = dev(np.concatenate([np.zeros(shift_grads, np.float32), grads]))
    dst = dev(np.full((count + shift_dst + 1) * 4, SENTINEL, dtype=np.uint8))
    psg.pool_scale_mean(dst.ptr + shift_dst * 4, g.ptr + shift_grads * 4, dev(offsets_of(lens)), nb, width)
    psg.device_sync()
    raw = dst.download(np.uint8, (count + shift_dst + 1) * 4)
    assert np.all(raw[:shift_dst * 4] == SENTINEL) and np.all(raw[(shift_dst + count) * 4:] == SENTINEL), "wrote outside dst"
    # grads is unchanged afterwards
    np.testing.assert_array_equal(g.download(np.uint32, count, offset=shift_grads * 4), grads.view(np.uint32))
    return raw[shift_dst * 4:(shift_dst + count) * 4].view(np.uint32)


def np_scale_mean(grads, lens, width):
    L = np.repeat(lens.astype(np.uint32), width)
    with np.errstate(all="ignore"):
        q = np.where(L > 0, grads / np.where(L > 0, L, 1).astype(np.float32), np.float32(0.0))
    return q.astype(np.float32).view(np.uint32)


@pytest.mark.parametrize("nb", [1, 5, 257])
@pytest.mark.parametrize("width", WIDTHS["f32"])
def test_scale_mean_is_one_division_per_element(width, nb):
    rng = np.random.default_rng(77 * nb + width)
    lens = bag_lengths(nb)
    grads = real_values(rng, psg.F32, nb * width)
    f = rs.specials(psg.F32)
    spec = np.array([f[n] for n in ("+minsub", "maxsub", "-minnorm", "s", "+inf", "-inf", "-0", "+max")], np.uint32)
    grads.view(np.uint32)[:min(len(spec), len(grads))] = spec[:len(grads)]  # (an empty first bag: not read)
    if nb > 1:
        grads.view(np.uint32)[width:width + min(len(spec), width)] = spec[:width]
    empty = np.repeat(lens == 0, width)
    grads.view(np.uint32)[empty] = f["+inf"] | 1  # an empty bag's gradient row is NaN and is not read
    exp = np_scale_mean(grads, lens, width)
    assert not rs.nan_mask(psg.F32, exp).any()
    for kw in ({}, {"shift_dst": 1}, {"shift_grads": 1}):
        got = scale_mean_on_gpu(grads, lens, width, **kw)
        np.testing.assert_array_equal(got, exp, err_msg=str(kw))
        assert np.all(got[empty] == 0)


def test_scale_mean_converts_a_length_of_2_24_plus_1_to_nearest():
    lens = np.array([(1 << 24) + 1, 3], dtype=np.uint64)
    for width in (4, 3):
        grads = np.tile(np.float32([3 << 24, 1.0, (1 << 24) + 2, 5.0]), 2 * width)[:2 * width]
        got = scale_mean_on_gpu(grads, lens, width)
        np.testing.assert_array_equal(got, np_scale_mean(grads, lens, width))
        assert got.view(np.float32)[0] == np.float32(3.0)


# ---- the equivalences on one table -----------------------------------------------------
class OneTable:
    """about 300 ids, 2000 occurrences in bags of 0-12 (the first and the last
    empty), four ids in five present"""

    def __init__(self, dtype, width, sorted_list, seed):
        rng = np.random.default_rng(seed)
        self.dtype, self.w = dtype, width
        self.ids = np.unique(rng.integers(0, 1 << 62, 300, dtype=np.uint64))
        self.present = self.ids[rng.random(len(self.ids)) < 0.8]
        self.rows = real_values(rng, dtype, len(self.present) * width)
        n = 2000
        lens = [0]
        while sum(lens) < n:
            lens.append(min(int(rng.integers(0, 13)), n - sum(lens)))
        lens.append(0)
        self.lens = np.array(lens, dtype=np.uint64)
        self.nb, self.n = len(lens), n
        hot = self.ids[rng.integers(0, len(self.ids), 8)]
        keys = np.where(rng.random(n) < 0.3, hot[rng.integers(0, 8, n)], self.ids[rng.integers(0, len(self.ids), n)])
        self.keys = np.sort(keys) if sorted_list else keys
        self.dkeys, self.doff = dev(self.keys.astype(np.uint64)), dev(offsets_of(self.lens))
        self.grads = real_values(rng, psg.F32, self.nb * width)

    def table(self, adam):
        t = psg.Table(self.dtype, self.w, 0, KMAX, 0)
        if adam:
            t.set_adam(*ADAM)
        t.assign(dev(self.present), dev(self.rows), len(self.present))
        return t


@pytest.mark.parametrize("sorted_list", [False, True], ids=["shuffled", "sorted"])
@pytest.mark.parametrize("width", [4, 20])
def test_a_plain_pooled_update_on_the_scaled_rows_is_the_one_table_mean_update(width, sorted_list):
    c = OneTable(psg.F32, width, sorted_list, seed=5 + width)
    a, b = c.table(True), c.table(True)
    dg = dev(c.grads)
    for it in range(2):
        scaled = psg.DeviceBuffer(c.nb * width * 4)
        psg.pool_scale_mean(scaled, dg, c.doff, c.nb, width)
        a.update_pooled(c.dkeys, c.doff, scaled, c.n, c.nb, LR, it)
        b.update_pooled_weighted(c.dkeys, c.doff, None, psg.POOL_MEAN, dg, c.n, c.nb, LR, it)
    psg.device_sync()
    (ka, ra), (kb, rb) = a.dump(), b.dump()
    np.testing.assert_array_equal(ka, kb)
    assert len(ka) == len(np.unique(np.concatenate([c.present, c.keys])))
    np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32))
    for x, y in zip(a.dump_moments(), b.dump_moments()):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("sorted_list", [False, True], ids=["shuffled", "sorted"])
@pytest.mark.parametrize("width", [4, 20])
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_reduce_mean_of_one_sum_partial_is_the_one_table_mean_lookup(name, width, sorted_list):
    dtype = DTYPES[name]
    c = OneTable(dtype, width, sorted_list, seed=9 + width + dtype)
    t = c.table(False)
    es, count = ESIZE[dtype], c.nb * width
    part, out, exp = (psg.DeviceBuffer(count * es) for _ in range(3))
    t.lookup_pooled(c.dkeys, c.doff, part, c.n, c.nb)
    psg.pool_reduce_mean(out, [part], c.doff, c.nb, width, dtype)
    t.lookup_pooled_weighted(c.dkeys, c.doff, None, psg.POOL_MEAN, exp, c.n, c.nb)
    psg.device_sync()
    np.testing.assert_array_equal(out.download(rs.UINT[dtype], count), exp.download(rs.UINT[dtype], count))
