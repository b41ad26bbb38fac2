"""The row table's pooled calls (psg_table_lookup_pooled / psg_table_update_pooled,
csrc/psg_rows.hip): the rows of a bag of ids summed, and the round in which every
id of a bag receives the bag's one gradient row.

The mirrors are numpy.  The forward's is a Python loop that adds a bag's rows in
arrival order in the accumulator type (f32; f64 for F64 tables) from +0 and
rounds once; the backward's definition is the twin test: a table that took
update_pooled equals a table that took psg_table_update_merged on the
host-expanded gradient rows.  Every comparison is bit for bit, through unsigned
views, except where the expected value is a NaN (payloads differ between host
and device: only NaN-ness is asserted).
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
    """count finite elements as the table stores them (psg_table_assign takes bytes)"""
    # halves: small enough that a bag of 2500 stays finite in F16
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
        with np.errstate(over="ignore"):
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


def pooled_ref(t, mir, q, offsets):
    """the definition: per bag, +0, then one add per present id in arrival order"""
    nb = len(offsets) - 1
    acc_t = np.float64 if t.dtype == psg.F64 else np.float32
    out = np.zeros((nb, t.width), dtype=acc_t)
    with np.errstate(all="ignore"):
        for b in range(nb):
            acc = np.zeros(t.width, dtype=acc_t)
            for p in range(int(offsets[b]), int(offsets[b + 1])):
                row = mir.get(int(q[p]))
                if row is not None:
                    acc = acc + row
            out[b] = acc
    return out


def pooled(t, q, offsets, out_off=0):
    """psg_table_lookup_pooled of the host lists -> element bits [nb, W]; out starts as FILL bytes"""
    nb, w, u = len(offsets) - 1, t.width, BITS[t.esize]
    nbytes = nb * w * t.esize + 16
    out = psg.DeviceBuffer(nbytes)
    out.upload(np.full(nbytes, FILL, dtype=np.uint8))
    t.lookup_pooled(dev(q) if len(q) else None, dev(offsets), out.ptr + out_off, len(q), nb)
    got = out.download(u, nb * w, offset=out_off).reshape(nb, w)
    edge = out.download(np.uint8, nbytes)
    assert (edge[:out_off] == FILL).all() and (edge[out_off + nb * w * t.esize:] == FILL).all(), "wrote outside out"
    return got


def check_pooled(t, mir, q, offsets, **kw):
    got = pooled(t, q, offsets, **kw)
    np.testing.assert_array_equal(got, from_acc(t.dtype, pooled_ref(t, mir, q, offsets)))


def offsets_of(bags):
    return np.concatenate([[0], np.cumsum([len(b) for b in bags])]).astype(np.uint64)


def flat(bags):
    return np.concatenate([np.asarray(b, dtype=np.uint64) for b in bags]).astype(np.uint64)


def bag_request(rng, present, absent, small=False):
    """One request with every bag shape: empty bags at the start, in the middle
    and at the end, a bag of 1, a bag of 2500 ids (it crosses the resolve's
    1024-key tile; half of them absent), a bag of absent ids only, one id five
    times inside a bag, one id in many bags, ids descending.  small: nb = 8 and
    n = 44, for rows of 4096 elements."""
    both = np.concatenate([present, absent])
    hot, five = present[0], present[1]
    desc = np.sort(rng.choice(both, 30, replace=False))[::-1]
    if small:
        bags = [[], [hot], [five, present[2], five, five, absent[0], five, five], absent[1:4], [], desc,
                [hot, present[3], hot], []]
    else:
        bags = [[], [hot], rng.choice(both, 2500, replace=True), absent[:7], [],
                [five, present[2], five, five, absent[0], five, five]]
        bags += [[present[10 + j], hot] for j in range(12)]  # one id in many bags
        bags += [desc]
        bags += [rng.choice(both, rng.integers(0, 10), replace=True) for _ in range(20)]  # about half absent
        bags += [[]]
    return flat(bags), offsets_of(bags)


def random_bags(rng, pool, nb, longest=4):
    bags = [rng.choice(pool, rng.integers(0, longest + 1), replace=True) for _ in range(nb)]
    return flat(bags), offsets_of(bags)


# ---- forward: the grid ---------------------------------------------------------------------------
WIDTHS = (1, 3, 4, 8, 33, 128, 4096)
GRID = [(d, w) for d in DTYPES for w in WIDTHS]


@pytest.mark.parametrize("dtype,width", GRID, ids=[f"{d}-w{w}" for d, w in GRID])
def test_forward_grid(dtype, width):
    rng = np.random.default_rng(2000 + width + 7 * DTYPES[dtype])
    small = width == 4096
    keys = random_keys(rng, 40 if small else 3000)
    absent = absent_keys(rng, keys, 40 if small else 3000)
    t = value_table(DTYPES[dtype], width, keys, rng)
    snap = snapshot(t, False)
    q, offsets = bag_request(rng, keys, absent, small)
    if small:
        assert len(offsets) - 1 <= 8 and len(q) <= 64
    check_pooled(t, acc_rows(t), q, offsets)
    assert_unchanged(t, snap, False)
    t.close()


def test_forward_out_4_bytes_off_takes_the_element_path():
    """W = 8 F32 rows are 32 B and would go as 16-B units; an out that is not on 16 B cannot"""
    rng = np.random.default_rng(11)
    keys = random_keys(rng, 3000)
    t = value_table(psg.F32, 8, keys, rng)
    q, offsets = bag_request(rng, keys, absent_keys(rng, keys, 3000))
    check_pooled(t, acc_rows(t), q, offsets, out_off=4)
    t.close()


# rows_per_tile = 2048 units: at W = 128 (32 units a row) a tile is 64 bags, at W = 33
# (elements) 62, at W = 4 (one unit) 2048: 257 and 1000 bags end in a partial tile of a
# grid of several blocks at the first two, 4100 bags at the third
@pytest.mark.parametrize("width,nb", [(w, nb) for w in (4, 33, 128) for nb in (1, 2, 257, 1000)] + [(4, 4100)])
def test_forward_bag_counts(width, nb):
    rng = np.random.default_rng(300 + width + nb)
    keys = random_keys(rng, 500)
    t = value_table(psg.F32, width, keys, rng)
    q, offsets = random_bags(rng, np.concatenate([keys, absent_keys(rng, keys, 500)]), nb)
    assert len(offsets) == nb + 1
    check_pooled(t, acc_rows(t), q, offsets)
    t.close()


def test_forward_no_ids_in_three_bags_gives_three_rows_of_plus_zero():
    rng = np.random.default_rng(12)
    for dtype in DTYPES.values():
        t = value_table(dtype, 4, random_keys(rng, 100), rng)
        got = pooled(t, np.zeros(0, np.uint64), np.zeros(4, np.uint64))
        assert got.shape == (3, 4) and not got.any()
        t.close()


def test_forward_leaves_an_adam_table_alone():
    """about half of the ids absent: nothing is inserted, no row and no moment changes"""
    rng = np.random.default_rng(13)
    keys = random_keys(rng, 3000)
    for width in (4, 3):
        t = value_table(psg.F32, width, keys, rng, adam=True)
        for it in range(2):
            g = rng.uniform(-1, 1, len(keys) * width).astype(np.float32)
            t.update(psg.PUSH, dev(keys), dev(g), None, len(keys), LR, it)
        snap = snapshot(t, True)
        q, offsets = bag_request(rng, keys, absent_keys(rng, keys, 3000))
        absent_share = 1 - np.isin(q, keys).mean()
        assert 0.3 < absent_share < 0.7, absent_share
        check_pooled(t, acc_rows(t), q, offsets)
        assert_unchanged(t, snap, True)
        t.close()


# ---- forward: special values ---------------------------------------------------------------------
def test_forward_specials_f32():
    """-0.0, +-inf and subnormals are pooled exactly; all -0.0 gives +0.0; inf - inf is a NaN"""
    pats = {"+0": 0x00000000, "-0": 0x80000000, "+inf": 0x7F800000, "-inf": 0xFF800000, "+minsub": 0x00000001,
            "-minsub": 0x80000001, "maxsub": 0x007FFFFF, "+minnorm": 0x00800000, "-minnorm": 0x80800000,
            "+max": 0x7F7FFFFF, "-max": 0xFF7FFFFF, "one": 0x3F800000}
    names = list(pats)
    width = 4
    keys = np.arange(1, len(names) + 1, dtype=np.uint64) * np.uint64(1000)
    key_of = dict(zip(names, keys))
    rows = np.repeat(np.array([pats[x] for x in names], dtype=np.uint32), width)
    t = psg.Table(psg.F32, width, 0, KEND, 0)
    t.assign(dev(keys), dev(rows), len(keys))  # as bytes: the patterns arrive as they are
    same(t.dump()[1], rows)
    bags = [[key_of[a], key_of[b]] for a in names for b in names]  # every ordered pair
    bags += [[key_of["-0"]] * 3, [key_of["-0"]], [key_of["+minsub"]] * 5, [key_of["maxsub"], key_of["+minsub"]],
             [key_of["+max"], key_of["+max"]], [key_of["+inf"], key_of["one"], key_of["-inf"]]]
    q, offsets = flat(bags), offsets_of(bags)
    got = pooled(t, q, offsets)
    exp = pooled_ref(t, acc_rows(t), q, offsets)
    nan = np.isnan(exp)
    assert nan.any() and not nan.all()
    assert np.isnan(got.view(np.float32)[nan]).all(), "a sum that is a NaN on the host is not one on the device"
    np.testing.assert_array_equal(got[~nan], bits(exp)[~nan])
    first = len(names) ** 2
    assert not got[first].any() and not got[first + 1].any(), "bags of -0.0 rows: the sum starts from +0"
    assert (got[first + 2] == 5).all(), "five times the smallest subnormal"
    assert (got[first + 3] == 0x00800000).all(), "maxsub + minsub is the smallest normal"
    assert (got[first + 4] == 0x7F800000).all(), "max + max rounds to +inf"
    assert np.isnan(got[first + 5].view(np.float32)).all(), "(inf + 1) - inf"
    t.close()


def test_forward_bags_of_one_equal_the_lookup_as_numbers():
    """0 + x == x for a finite x, so a bag of length 1 is psg_table_lookup's row AS A
    NUMBER; not as bytes: -0.0 comes back as +0.0 (0 + -0 is +0), and the test says so"""
    rng = np.random.default_rng(14)
    keys = random_keys(rng, 2000)
    width = 8
    t = value_table(psg.F32, width, keys, rng)
    minus_zero = np.array([keys[-1] + np.uint64(5)], dtype=np.uint64)
    t.assign(dev(minus_zero), dev(np.full(width, 0x80000000, dtype=np.uint32)), 1)
    q = np.concatenate([rng.permutation(np.concatenate([keys[:700], absent_keys(rng, keys, 300)])), minus_zero])
    n = len(q)
    out = psg.DeviceBuffer(n * width * 4)
    t.lookup(dev(q), out, None, n)
    looked = out.download(np.float32, n * width).reshape(n, width)
    got = pooled(t, q, np.arange(n + 1, dtype=np.uint64)).view(np.float32)
    np.testing.assert_array_equal(got, looked)  # as numbers: -0.0 == +0.0
    assert (bits(looked[-1]) == 0x80000000).all() and (bits(got[-1]) == 0).all()
    np.testing.assert_array_equal(bits(got[:-1]), bits(looked[:-1]))
    t.close()


# ---- forward: refusals found on the device -------------------------------------------------------
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


def test_forward_refusals_write_nothing():
    rng = np.random.default_rng(15)
    keys = random_keys(rng, 300)
    for width in (4, 3):
        t = value_table(psg.F32, width, keys, rng, adam=True)
        snap = snapshot(t, True)
        for name, q, offsets, code in bad_requests(keys):
            nb = len(offsets) - 1
            out = psg.DeviceBuffer(nb * width * 4)
            out.upload(np.full(nb * width * 4, FILL, dtype=np.uint8))
            msg = refused(lambda: t.lookup_pooled(dev(q), dev(offsets), out, len(q), nb), code)
            assert "psg_table_lookup_pooled" in msg or code == RANGE, (name, msg)
            assert (out.download(np.uint8, nb * width * 4) == FILL).all(), name + ": out was written"
            assert_unchanged(t, snap, True)
        t.close()


# ---- backward ------------------------------------------------------------------------------------
def bag_index(offsets):
    """bag(i) for every position i"""
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))


def expanded(grads, offsets, width):
    """E: the gradient row of bag(i) at row i — what update_pooled never builds"""
    return np.ascontiguousarray(grads.reshape(-1, width)[bag_index(offsets)]).ravel()


def cut_into_bags(rng, q, big=2500):
    """offsets over the list q: an empty bag, a bag of 1, one bag of `big`, random
    short bags with empty ones among them, an empty bag at the end"""
    n = len(q)
    assert n > big + 1
    sizes = [0, 1, big]
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(0, 9)), n - sum(sizes)))
    sizes.append(0)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def step_lists(rng, known, order, it):
    """the ids of iteration `it`: 3000 of the known ones and 200 new ones"""
    new = absent_keys(rng, known, 200)
    if order == "ascending":  # strictly: the path that does not sort
        return np.sort(np.concatenate([rng.choice(known, 3000, replace=False), new])), new
    q = np.concatenate([rng.choice(known, 3000, replace=True), new, new[:50]])  # repeats, also of new ids
    return rng.permutation(q), new


@pytest.mark.parametrize("width", (1, 3, 4, 33, 128))
@pytest.mark.parametrize("order", ("ascending", "shuffled"))
@pytest.mark.parametrize("opt", ("sgd", "adam"))
def test_backward_twin(opt, order, width):
    rng = np.random.default_rng(400 + width + (7 if opt == "adam" else 0) + (13 if order == "shuffled" else 0))
    adam = opt == "adam"
    known = random_keys(rng, 4000)
    seed = np.random.default_rng(1)
    a = value_table(psg.F32, width, known, seed, adam)
    b = value_table(psg.F32, width, known, np.random.default_rng(1), adam)
    assert_twins(a, b, adam)
    for it in range(3):
        q, new = step_lists(rng, known, order, it)
        n = len(q)
        offsets = cut_into_bags(rng, q)
        nb = len(offsets) - 1
        grads = rng.uniform(-1, 1, nb * width).astype(np.float32)
        assert offsets[1] == 0 and offsets[-2] == n
        grads[:width] = grads[-width:] = np.nan  # the first and the last bag are empty: their rows are not read
        a.update_pooled(dev(q), dev(offsets), dev(grads), n, nb, LR, it)
        path = b.update_merged(psg.PUSH, [dev(q)], [dev(expanded(grads, offsets, width))], None, [n], LR, it)
        assert path == (psg.MERGED_SAME_LIST if order == "ascending" else psg.MERGED_SORTED)
        known = np.union1d(known, new)
        assert int(a.info().size) == len(known), "absent ids are inserted once"
        assert_twins(a, b, adam)
    assert not np.isnan(a.dump()[1]).any()
    a.close()
    b.close()


@pytest.mark.parametrize("width", (4, 3))
def test_backward_sgd_against_numpy(width):
    """s summed in f32 in arrival order from +0.0f, row = f32(f64(row) - f64(f32(lr) * s)).
    One id sits in three bags whose gradients are 1e8, 1.0, -1e8: in that order the f32
    sum is 0 (the 1.0 is lost next to 1e8), in any other it is 1."""
    rng = np.random.default_rng(16)
    keys = random_keys(rng, 600)
    new = absent_keys(rng, keys, 40)
    x = keys[7]
    order_bags = [[x, keys[1]], [keys[2], x, keys[3]], [x]]
    for strict in (False, True):
        t = value_table(psg.F32, width, keys, np.random.default_rng(2))
        k0, r0 = t.dump()
        rows = {int(k): r0[j].copy() for j, k in enumerate(k0)}
        if strict:
            q = np.sort(np.concatenate([rng.choice(keys, 300, replace=False), new]))
            sizes = [0, 1] + [5] * ((len(q) - 1) // 5)
            sizes += [len(q) - sum(sizes), 0]
            offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        else:
            others = np.setdiff1d(np.concatenate([keys, new]), [x])
            bags = order_bags + [rng.choice(others, rng.integers(0, 7), replace=True) for _ in range(200)] + [new]
            q, offsets = flat(bags), offsets_of(bags)
        nb = len(offsets) - 1
        grads = rng.uniform(-1, 1, (nb, width)).astype(np.float32)
        if not strict:
            grads[0], grads[1], grads[2] = 1e8, 1.0, -1e8
        t.update_pooled(dev(q), dev(offsets), dev(grads.ravel()), len(q), nb, LR, 0)
        s = {}
        for i, b in enumerate(bag_index(offsets)):
            s[int(q[i])] = s.get(int(q[i]), np.zeros(width, dtype=np.float32)) + grads[b]  # one f32 add each
        if not strict:
            assert (s[int(x)] == 0).all(), "the order of the adds is the arrival order"
        for key, sk in s.items():
            row = rows.get(key, np.zeros(width, dtype=np.float32))
            rows[key] = (row.astype(np.float64) - (np.float32(LR) * sk).astype(np.float64)).astype(np.float32)
        k1, r1 = t.dump()
        np.testing.assert_array_equal(k1, np.array(sorted(rows), dtype=np.uint64))
        same(r1, np.stack([rows[int(k)] for k in k1]))
        t.close()


def test_backward_an_empty_bag_with_a_nan_gradient_row_changes_nothing():
    rng = np.random.default_rng(17)
    keys = random_keys(rng, 200)
    width = 4
    for adam in (False, True):
        a = value_table(psg.F32, width, keys, np.random.default_rng(3), adam)
        b = value_table(psg.F32, width, keys, np.random.default_rng(3), adam)
        q = rng.permutation(keys[:50])
        offsets = np.array([0, 20, 20, 50], dtype=np.uint64)
        grads = rng.uniform(-1, 1, 3 * width).astype(np.float32)
        clean = grads.copy()
        grads[width: 2 * width] = np.nan
        a.update_pooled(dev(q), dev(offsets), dev(grads), 50, 3, LR, 0)
        b.update_pooled(dev(q), dev(np.array([0, 20, 50], dtype=np.uint64)),
                        dev(np.concatenate([clean[:width], clean[2 * width:]])), 50, 2, LR, 0)
        assert_twins(a, b, adam)
        assert not np.isnan(a.dump()[1]).any()
        # a request of empty bags only: nothing is read, nothing changes
        snap = snapshot(a, adam)
        a.update_pooled(None, dev(np.zeros(3, dtype=np.uint64)), dev(np.full(2 * width, np.nan, dtype=np.float32)), 0, 2,
                        LR, 1)
        assert_unchanged(a, snap, adam)
        a.close()
        b.close()


def test_backward_refusals_change_nothing():
    rng = np.random.default_rng(18)
    keys = random_keys(rng, 300)
    for dtype in (psg.F64, psg.F16, psg.BF16):
        t = value_table(dtype, 4, keys, rng)
        snap = snapshot(t, False)
        msg = refused(lambda: t.update_pooled(dev(keys[:6]), dev(np.array([0, 2, 6], dtype=np.uint64)),
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
                refused(lambda: t.update_pooled(dev(lst), dev(offsets), dev(np.ones(nb * width, dtype=np.float32)),
                                                len(lst), nb, LR, 1), code)
                assert_unchanged(t, snap, adam)
        t.close()


def test_round_trip_lookup_pooled_after_update_pooled():
    rng = np.random.default_rng(19)
    keys = random_keys(rng, 3000)
    for width in (8, 33):
        t = value_table(psg.F32, width, keys, rng, adam=True)
        q, offsets = bag_request(rng, keys, absent_keys(rng, keys, 3000))
        nb = len(offsets) - 1
        for it in range(2):
            t.update_pooled(dev(q), dev(offsets), dev(rng.uniform(-1, 1, nb * width).astype(np.float32)), len(q), nb, LR, it)
        assert int(t.info().size) == len(np.union1d(keys, q)), "every id of the request is in the table now"
        check_pooled(t, acc_rows(t), q, offsets)
        t.close()
