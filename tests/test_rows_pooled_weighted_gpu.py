"""The row table's weighted and mean pooled calls (psg_table_lookup_pooled_weighted /
psg_table_update_pooled_weighted, csrc/psg_rows.hip): a bag's rows summed with a
weight per id, or averaged over the bag's length, and the round in which every id
receives its bag's gradient row times its weight, or over the length.

The mirrors are numpy.  The forward's is a Python loop in the accumulator type
(f32; f64 for F64 tables): per present id ONE multiply and ONE add, in arrival
order from +0, then for a mean ONE division by the length, then one rounding.  The
backward's definition is the twin test: a table that took update_pooled_weighted
equals a table that took psg_table_update_merged on the host-built gradient rows
E (one numpy f32 multiply or division each).  Every comparison is bit for bit,
through unsigned views.  The inputs keep every expected value finite, and the
mirror asserts it.

Shapes: about 2,000 ids in about 600 bags (k_bag_of crosses a block), the widths
at which a row goes as 16-B units and as elements for each dtype.
"""
import numpy as np
import pytest

import psg

pytestmark = pytest.mark.gpu

KEND = 1 << 40
LR = 0.05
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
BITS = {4: np.uint32, 8: np.uint64, 2: np.uint16}
INVALID, RANGE, UNSUPPORTED = 1, 4, 6
DTYPES = {"f32": psg.F32, "f64": psg.F64, "f16": psg.F16, "bf16": psg.BF16}
FILL = 0xA5
SUM, MEAN = psg.POOL_SUM, psg.POOL_MEAN
# 16-B units and elements of each dtype: F32 rows of 4 and 8 are 16-B units, 1 and 3
# are not; F64 2 / 3; halves 8 / 5
GRID = [("f32", 1), ("f32", 3), ("f32", 4), ("f32", 8), ("f64", 2), ("f64", 3), ("f16", 5), ("f16", 8),
        ("bf16", 5), ("bf16", 8)]
GRID_IDS = [f"{d}-w{w}" for d, w in GRID]
ORDERS = ("ascending", "shuffled")


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
    np.testing.assert_array_equal(bits(got).ravel(), bits(exp).ravel())


def random_keys(rng, n, lo=0, hi=KEND):
    u = np.unique(rng.integers(lo, hi, 2 * n + 16, dtype=np.uint64))
    return np.sort(rng.choice(u, n, replace=False))


def absent_keys(rng, present, n, hi=KEND):
    u = np.setdiff1d(np.unique(rng.integers(0, hi, 2 * n + 16, dtype=np.uint64)), present)
    return rng.choice(u, n, replace=False)


def snapshot(t, adam):
    """everything a call that must not change the table could change"""
    i = t.info()
    k, rows = t.dump()
    mom = t.dump_moments() if adam else ()
    return (int(i.size), int(i.capacity), i.rows, i.keys, k.copy(), bits(rows).copy()) + tuple(bits(x).copy() for x in mom)


def assert_unchanged(t, snap, adam):
    now = snapshot(t, adam)
    assert now[:4] == snap[:4], "size, capacity or a device pointer changed"
    for a, b in zip(now[4:], snap[4:]):
        np.testing.assert_array_equal(a, b)


def assert_twins(a, b, adam):
    """two tables hold the same keys, rows and moments, bit for bit"""
    ka, ra = a.dump()
    kb, rb = b.dump()
    np.testing.assert_array_equal(ka, kb)
    same(ra, rb)
    if adam:
        for x, y in zip(a.dump_moments(), b.dump_moments()):
            same(x, y)


# ---- values per dtype: finite rows, the accumulator's view of them, the one rounding -------
def finite_rows(rng, dtype, count):
    """count finite elements as the table stores them (psg_table_assign takes bytes);
    halves: at most 32, so a bag of 300 with weights in [-2, 2] stays below 19,200"""
    scales = [1.0, 1.0, 0.001, 100.0] if dtype in (psg.F32, psg.F64) else [1.0, 1.0, 0.001, 8.0]
    x = (rng.uniform(-4, 4, count) * rng.choice(scales, count)).astype(np.float32)
    if dtype == psg.F32:
        return x
    if dtype == psg.F64:
        return rng.uniform(-4, 4, count) * rng.choice([1.0, 1e-9, 1e6], count)
    if dtype == psg.F16:
        return x.astype(np.float16)
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)  # BF16: the upper half of an f32


def to_acc(dtype, stored):
    """stored elements -> the accumulator type (exact for every dtype)"""
    if dtype == psg.F64:
        return np.asarray(stored, dtype=np.float64)
    if dtype == psg.BF16:
        return (bits(stored).astype(np.uint32) << np.uint32(16)).view(np.float32)
    return np.asarray(stored).astype(np.float32)


def from_acc(dtype, acc):
    """the accumulator -> the table's element bits: halves round once, to nearest even"""
    if dtype in (psg.F32, psg.F64):
        return bits(acc)
    if dtype == psg.F16:
        return acc.astype(np.float16).view(np.uint16)
    u = acc.view(np.uint32).astype(np.uint64)  # BF16: the rounding on the f32 bits (finite inputs)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def value_table(dtype, width, keys, rng, adam=False):
    t = psg.Table(dtype, width, 0, KEND, 0)
    if adam:
        t.set_adam(*ADAM)
    t.assign(dev(keys), dev(finite_rows(rng, dtype, len(keys) * width)), len(keys))
    return t


def acc_rows(t):
    """{key: the row in the accumulator type} from the dump"""
    k, rows = t.dump()
    a = to_acc(t.dtype, rows).reshape(len(k), t.width)
    return {int(k[j]): a[j] for j in range(len(k))}


# ---- the request ---------------------------------------------------------------------------------
def offsets_of_sizes(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def request(rng, present, absent, order, n=2000):
    """About n ids in about 600 bags, about a tenth of them absent: empty bags first,
    in the middle and last, a bag of one id, one bag of 300, bags of 3, 5 and 7 (a
    mean by a reciprocal would show), short random bags with empty ones among them.
    shuffled: ids in any order with repeats, and two bags more: one id five times
    (five weights), absent ids only.  ascending: strictly, every id once."""
    pool = np.concatenate([present, absent[:len(present) // 9]])
    if order == "ascending":
        q = np.sort(rng.choice(pool, n, replace=False))
        sizes = [0, 1, 0]
    else:
        head = np.concatenate([[present[0]], [present[1]] * 5, absent[-6:]]).astype(np.uint64)
        q = np.concatenate([head, rng.choice(pool, n - len(head), replace=True)])
        sizes = [0, 1, 5, 6, 0]
    sizes += [300, 3, 5, 7]
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(0, 7)), n - sum(sizes)))
    sizes.append(0)
    offsets = offsets_of_sizes(sizes)
    assert offsets[-1] == n == len(q) and 256 < len(sizes) < 900
    return np.ascontiguousarray(q, dtype=np.uint64), offsets


def weights_for(rng, n):
    return rng.uniform(-2, 2, n).astype(np.float32)


def forward_case(dtype, width, order, seed, adam=False):
    rng = np.random.default_rng(seed + width + 7 * DTYPES[dtype] + (13 if order == "shuffled" else 0))
    keys = random_keys(rng, 2700)
    absent = absent_keys(rng, keys, 400)
    t = value_table(DTYPES[dtype], width, keys, rng, adam)
    q, offsets = request(rng, keys, absent, order)
    share = 1 - np.isin(q, keys).mean()
    assert 0.05 < share < 0.2, share
    return rng, t, q, offsets


# ---- forward: the mirror and the call ------------------------------------------------------------
def weighted_ref(t, mir, q, offsets, weights, mode):
    """the definition: per bag +0, then per present id ONE multiply (weights given) and
    ONE add in the accumulator type, in arrival order; a mean then divides ONCE by the
    bag's length, absent ids counted; an empty bag divides nothing"""
    nb = len(offsets) - 1
    acc_t = np.float64 if t.dtype == psg.F64 else np.float32
    out = np.zeros((nb, t.width), dtype=acc_t)
    for b in range(nb):
        p0, p1 = int(offsets[b]), int(offsets[b + 1])
        acc = np.zeros(t.width, dtype=acc_t)
        for p in range(p0, p1):
            row = mir.get(int(q[p]))
            if row is None:
                continue
            if weights is not None:
                prod = acc_t(weights[p]) * row
                assert prod.dtype == acc_t
                acc = acc + prod
            else:
                acc = acc + row
        if mode == MEAN and p1 > p0:
            acc = acc / acc_t(np.uint32(p1 - p0))
        assert acc.dtype == acc_t
        out[b] = acc
    assert np.isfinite(out).all(), "the inputs are chosen so that every expected value is finite"
    return out


def filled(nbytes):
    out = psg.DeviceBuffer(nbytes)
    out.upload(np.full(nbytes, FILL, dtype=np.uint8))
    return out


def pooled_weighted(t, q, offsets, weights, mode, out_off=0, w_off=0):
    """psg_table_lookup_pooled_weighted of the host lists -> element bits [nb, W]; out
    starts as FILL bytes; out_off / w_off: bytes by which out / weights start late"""
    nb, w, u = len(offsets) - 1, t.width, BITS[t.esize]
    nbytes = nb * w * t.esize + 16
    out = filled(nbytes)
    wd = None
    if weights is not None:
        wd = psg.DeviceBuffer(len(weights) * 4 + 16)
        wd.upload(np.concatenate([np.zeros(w_off, np.uint8), weights.view(np.uint8), np.zeros(16 - w_off, np.uint8)]))
    t.lookup_pooled_weighted(dev(q) if len(q) else None, dev(offsets), wd.ptr + w_off if wd is not None else None, mode,
                             out.ptr + out_off, len(q), nb)
    got = out.download(u, nb * w, offset=out_off).reshape(nb, w)
    edge = out.download(np.uint8, nbytes)
    assert (edge[:out_off] == FILL).all() and (edge[out_off + nb * w * t.esize:] == FILL).all(), "wrote outside out"
    return got


def pooled_plain(t, q, offsets):
    """psg_table_lookup_pooled, the unweighted call -> element bits [nb, W]"""
    nb, w = len(offsets) - 1, t.width
    out = filled(nb * w * t.esize)
    t.lookup_pooled(dev(q), dev(offsets), out, len(q), nb)
    return out.download(BITS[t.esize], nb * w).reshape(nb, w)


def check_forward(t, mir, q, offsets, weights, mode, **kw):
    got = pooled_weighted(t, q, offsets, weights, mode, **kw)
    np.testing.assert_array_equal(got, from_acc(t.dtype, weighted_ref(t, mir, q, offsets, weights, mode)))
    return got


# ---- forward -------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype,width", GRID, ids=GRID_IDS)
def test_forward_weighted_sum_is_the_mirror(dtype, width, order):
    rng, t, q, offsets = forward_case(dtype, width, order, 5000)
    snap = snapshot(t, False)
    weights = weights_for(rng, len(q))
    if order == "shuffled":
        assert len(set(weights[1:6].tolist())) == 5 and len(set(q[1:6].tolist())) == 1, "one id, five weights"
    check_forward(t, acc_rows(t), q, offsets, weights, SUM)
    assert_unchanged(t, snap, False)
    t.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype,width", GRID, ids=GRID_IDS)
def test_forward_mean_is_the_mirror(dtype, width, order):
    """bags of 3, 5, 7 and 300 ids among them: x / 3 is not x * (1 / 3) rounded"""
    rng, t, q, offsets = forward_case(dtype, width, order, 6000)
    snap = snapshot(t, False)
    lengths = np.diff(offsets.astype(np.int64))
    assert {3, 5, 7, 300} <= set(lengths.tolist()) and lengths[0] == 0 and lengths[-1] == 0
    got = check_forward(t, acc_rows(t), q, offsets, None, MEAN)
    assert not got[lengths == 0].any(), "an empty bag's mean is a row of +0"
    assert_unchanged(t, snap, False)
    t.close()


@pytest.mark.parametrize("dtype,width", GRID, ids=GRID_IDS)
def test_forward_weights_of_one_and_no_weights_are_the_unweighted_call(dtype, width):
    rng, t, q, offsets = forward_case(dtype, width, "shuffled", 7000)
    snap = snapshot(t, False)
    plain = pooled_plain(t, q, offsets)
    np.testing.assert_array_equal(pooled_weighted(t, q, offsets, np.ones(len(q), dtype=np.float32), SUM), plain)
    np.testing.assert_array_equal(pooled_weighted(t, q, offsets, None, SUM), plain)
    assert_unchanged(t, snap, False)
    t.close()


def test_forward_out_one_element_off_takes_the_element_path():
    """W = 8 F32 rows are 32 B and would go as 16-B units; an out that is not on 16 B cannot"""
    rng, t, q, offsets = forward_case("f32", 8, "shuffled", 8000)
    mir = acc_rows(t)
    check_forward(t, mir, q, offsets, weights_for(rng, len(q)), SUM, out_off=4)
    check_forward(t, mir, q, offsets, None, MEAN, out_off=4)
    t.close()


def test_forward_weights_one_element_off_16_bytes():
    """weights are read as words, wherever they start; the rows still go as 16-B units"""
    rng, t, q, offsets = forward_case("f32", 8, "shuffled", 9000)
    check_forward(t, acc_rows(t), q, offsets, weights_for(rng, len(q)), SUM, w_off=4)
    t.close()


def test_forward_leaves_an_adam_table_alone():
    rng, t, q, offsets = forward_case("f32", 4, "shuffled", 10000, adam=True)
    keys = t.dump()[0]
    for it in range(2):
        g = rng.uniform(-1, 1, len(keys) * 4).astype(np.float32)
        t.update(psg.PUSH, dev(keys), dev(g), None, len(keys), LR, it)
    snap = snapshot(t, True)
    mir = acc_rows(t)
    check_forward(t, mir, q, offsets, weights_for(rng, len(q)), SUM)
    assert_unchanged(t, snap, True)
    check_forward(t, mir, q, offsets, None, MEAN)
    assert_unchanged(t, snap, True)
    t.close()


def test_forward_a_zero_weight_on_an_inf_row_is_a_nan_and_a_nan_weight_on_an_absent_id_is_nothing():
    rng = np.random.default_rng(21)
    width = 4
    keys = random_keys(rng, 50)
    absent = absent_keys(rng, keys, 4)
    t = value_table(psg.F32, width, keys, rng)
    inf_key = np.array([keys[-1] + np.uint64(3)], dtype=np.uint64)
    t.assign(dev(inf_key), dev(np.full(width, np.inf, dtype=np.float32)), 1)
    q = np.array([keys[0], inf_key[0], keys[1], keys[2], absent[0], keys[3]], dtype=np.uint64)
    offsets = np.array([0, 3, 6], dtype=np.uint64)
    weights = np.array([1.5, 0.0, -0.5, 0.25, np.nan, 2.0], dtype=np.float32)
    got = pooled_weighted(t, q, offsets, weights, SUM).view(np.float32)
    assert np.isnan(got[0]).all(), "0 * inf is a NaN, and it reaches the bag"
    mir = acc_rows(t)
    exp = (np.float32(0.25) * mir[int(keys[2])]) + np.float32(2.0) * mir[int(keys[3])]
    assert np.isfinite(got[1]).all()
    same(got[1], exp)
    t.close()


# ---- refusals found on the device ----------------------------------------------------------------
def refused(call, code):
    with pytest.raises(psg.PsgError) as ei:
        call()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def bad_requests(keys):
    """(name, q, offsets, code): small lists that break one rule, or two"""
    q = np.ascontiguousarray(keys[:6])
    out_of_range = q.copy()
    out_of_range[4] = KEND
    good = np.array([0, 2, 2, 6], dtype=np.uint64)
    return [("offsets[0] != 0", q, np.array([1, 2, 2, 6], dtype=np.uint64), INVALID),
            ("a decreasing pair", q, np.array([0, 3, 2, 6], dtype=np.uint64), INVALID),
            ("offsets[nb] above n", q, np.array([0, 2, 2, 7], dtype=np.uint64), INVALID),
            ("offsets[nb] below n", q, np.array([0, 2, 2, 5], dtype=np.uint64), INVALID),
            ("a key out of range", out_of_range, good, RANGE),
            ("both", out_of_range, np.array([0, 3, 2, 6], dtype=np.uint64), INVALID)]


POOLINGS = ("weighted", "mean")


def pooling_args(pooling, n):
    """(weights on the device or None, mode)"""
    if pooling == "mean":
        return None, MEAN
    return dev(np.linspace(-2, 2, n).astype(np.float32)), SUM


@pytest.mark.parametrize("pooling", POOLINGS)
def test_forward_refusals_write_nothing(pooling):
    rng = np.random.default_rng(22)
    keys = random_keys(rng, 300)
    for width in (4, 3):
        t = value_table(psg.F32, width, keys, rng, adam=True)
        snap = snapshot(t, True)
        for name, q, offsets, code in bad_requests(keys):
            nb = len(offsets) - 1
            out = filled(nb * width * 4)
            wd, mode = pooling_args(pooling, len(q))
            msg = refused(lambda: t.lookup_pooled_weighted(dev(q), dev(offsets), wd, mode, out, len(q), nb), code)
            assert "psg_table_lookup_pooled_weighted" in msg or code == RANGE, (name, msg)
            assert (out.download(np.uint8, nb * width * 4) == FILL).all(), name + ": out was written"
            assert_unchanged(t, snap, True)
        t.close()


# ---- backward ------------------------------------------------------------------------------------
def bag_index(offsets):
    """bag(i) for every position i"""
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))


def expanded(grads, offsets, width, weights, mode):
    """E, which update_pooled_weighted never builds: row i is the gradient row of bag(i)
    times weights[i] (one f32 multiply), or over (float)L_bag(i) (one f32 division), or
    as it is.  An empty bag's row is not read."""
    b = bag_index(offsets)
    rows = grads.reshape(-1, width)[b]
    if mode == MEAN:
        rows = rows / np.diff(offsets.astype(np.int64)).astype(np.float32)[b][:, None]
    elif weights is not None:
        rows = weights[:, None] * rows
    assert rows.dtype == np.float32 and np.isfinite(rows).all()
    return np.ascontiguousarray(rows).ravel()


def update_weighted(t, q, offsets, weights, mode, grads, it):
    t.update_pooled_weighted(dev(q), dev(offsets), None if weights is None else dev(weights), mode, dev(grads), len(q),
                             len(offsets) - 1, LR, it)


def twin_tables(width, known, adam):
    a = value_table(psg.F32, width, known, np.random.default_rng(1), adam)
    b = value_table(psg.F32, width, known, np.random.default_rng(1), adam)
    assert_twins(a, b, adam)
    return a, b


def backward_request(rng, known, order, width):
    """the request of one iteration: about a tenth of its ids are not in the table yet
    (shuffled: some of them named several times); the gradient rows of its empty
    bags are NaN"""
    new = absent_keys(rng, known, 400)
    q, offsets = request(rng, known, new, order)
    nb = len(offsets) - 1
    grads = rng.uniform(-1, 1, (nb, width)).astype(np.float32)
    empty = np.diff(offsets.astype(np.int64)) == 0
    assert empty[0] and empty[-1] and empty[1:-1].any()
    grads[empty] = np.nan
    return q, offsets, grads.ravel()


@pytest.mark.parametrize("width", (4, 3))
@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("opt", ("sgd", "adam"))
def test_backward_twin(opt, order, pooling, width):
    """two consecutive iterations; an id of several bags steps once, an absent id is
    inserted once, the NaN gradient row of an empty bag reaches nothing"""
    rng = np.random.default_rng(700 + width + (7 if opt == "adam" else 0) + (13 if order == "shuffled" else 0) +
                                (29 if pooling == "mean" else 0))
    adam = opt == "adam"
    known = random_keys(rng, 2700)
    a, b = twin_tables(width, known, adam)
    for it in range(2):
        q, offsets, grads = backward_request(rng, known, order, width)
        weights, mode = (None, MEAN) if pooling == "mean" else (weights_for(rng, len(q)), SUM)
        if order == "shuffled":
            assert len(np.unique(q)) < len(q)
        update_weighted(a, q, offsets, weights, mode, grads, it)
        path = b.update_merged(psg.PUSH, [dev(q)], [dev(expanded(grads, offsets, width, weights, mode))], None, [len(q)],
                               LR, it)
        assert path == (psg.MERGED_SAME_LIST if order == "ascending" else psg.MERGED_SORTED)
        known = np.union1d(known, q)
        assert int(a.info().size) == len(known), "absent ids are inserted once"
        assert_twins(a, b, adam)
    assert not np.isnan(a.dump()[1]).any()
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_backward_without_weights_is_update_pooled(order):
    rng = np.random.default_rng(23)
    for width, adam in ((4, True), (3, False)):
        known = random_keys(rng, 2700)
        a, b = twin_tables(width, known, adam)
        for it in range(2):
            q, offsets, grads = backward_request(rng, known, order, width)
            update_weighted(a, q, offsets, None, SUM, grads, it)
            b.update_pooled(dev(q), dev(offsets), dev(grads), len(q), len(offsets) - 1, LR, it)
            known = np.union1d(known, q)
            assert_twins(a, b, adam)
        a.close()
        b.close()


@pytest.mark.parametrize("width", (4, 3))
def test_backward_an_id_of_three_bags_steps_once_in_arrival_order(width):
    """s summed in f32 in arrival order from +0.0f, row = f32(f64(row) - f64(f32(lr) * s)).
    One id sits in three bags with weights 2, 0.5, -1 and gradients 5e7, 2.0, 1e8: its E
    rows are 1e8, 1.0, -1e8, whose f32 sum is 0 in that order (the 1.0 is lost next to
    1e8) and 1 in any other."""
    rng = np.random.default_rng(24)
    keys = random_keys(rng, 600)
    new = absent_keys(rng, keys, 40)
    x = keys[7]
    t = value_table(psg.F32, width, keys, np.random.default_rng(2))
    k0, r0 = t.dump()
    rows = {int(k): r0[j].copy() for j, k in enumerate(k0)}
    others = np.setdiff1d(np.concatenate([keys, new]), [x])
    bags = [[x, keys[1]], [keys[2], x, keys[3]], [x]]
    bags += [rng.choice(others, rng.integers(0, 7), replace=True) for _ in range(300)] + [new]
    q = np.concatenate([np.asarray(b, dtype=np.uint64) for b in bags]).astype(np.uint64)
    offsets = offsets_of_sizes([len(b) for b in bags])
    nb = len(offsets) - 1
    grads = rng.uniform(-1, 1, (nb, width)).astype(np.float32)
    weights = weights_for(rng, len(q))
    grads[0], grads[1], grads[2] = 5e7, 2.0, 1e8
    weights[0], weights[3], weights[5] = 2.0, 0.5, -1.0
    update_weighted(t, q, offsets, weights, SUM, grads.ravel(), 0)
    s = {}
    for i, b in enumerate(bag_index(offsets)):
        e = weights[i] * grads[b]  # one f32 multiply
        s[int(q[i])] = s.get(int(q[i]), np.zeros(width, dtype=np.float32)) + e  # one f32 add
    assert (s[int(x)] == 0).all(), "the order of the adds is the arrival order"
    for key, sk in s.items():
        row = rows.get(key, np.zeros(width, dtype=np.float32))
        rows[key] = (row.astype(np.float64) - (np.float32(LR) * sk).astype(np.float64)).astype(np.float32)
    k1, r1 = t.dump()
    np.testing.assert_array_equal(k1, np.array(sorted(rows), dtype=np.uint64))
    same(r1, np.stack([rows[int(k)] for k in k1]))
    t.close()


@pytest.mark.parametrize("pooling", POOLINGS)
def test_backward_refusals_change_nothing(pooling):
    rng = np.random.default_rng(25)
    keys = random_keys(rng, 300)
    for dtype in (psg.F64, psg.F16, psg.BF16):
        t = value_table(dtype, 4, keys, rng)
        snap = snapshot(t, False)
        wd, mode = pooling_args(pooling, 6)
        msg = refused(lambda: t.update_pooled_weighted(dev(keys[:6]), dev(np.array([0, 2, 6], dtype=np.uint64)), wd, mode,
                                                       dev(np.zeros(8, dtype=np.float32)), 6, 2, LR, 0), UNSUPPORTED)
        assert "F32" in msg
        assert_unchanged(t, snap, False)
        t.close()
    for width, adam in ((4, True), (3, False)):
        t = value_table(psg.F32, width, keys, rng, adam)
        if adam:
            t.update(psg.PUSH, dev(keys), dev(rng.uniform(-1, 1, len(keys) * width).astype(np.float32)), None, len(keys),
                     LR, 0)
        snap = snapshot(t, adam)
        for name, q, offsets, code in bad_requests(keys):
            nb = len(offsets) - 1
            for lst in (q, q[::-1].copy()):  # ascending (the path without a sort) and not
                wd, mode = pooling_args(pooling, len(lst))
                refused(lambda: t.update_pooled_weighted(dev(lst), dev(offsets), wd, mode,
                                                         dev(np.ones(nb * width, dtype=np.float32)), len(lst), nb, LR, 1),
                        code)
                assert_unchanged(t, snap, adam)  # the Adam moments among it
        t.close()
