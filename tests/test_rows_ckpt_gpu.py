"""The row table's assign and export (psg_table_assign / psg_table_export,
csrc/psg_rows.hip): rows and Adam moments put into a table as bytes and taken
out again in chunks, on the device.

Every comparison is bit for bit, through unsigned views.  The definition is the
resume test: a table exported after three updates and assigned into a fresh
one, which then takes three more, equals the table that took all six.
"""
import numpy as np
import pytest

import oracle
import psg
import row_specials as rs

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1
LR = 0.05
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
BITS = {4: np.uint32, 8: np.uint64, 2: np.uint16}
ESIZE = {psg.F32: 4, psg.F64: 8, psg.F16: 2, psg.BF16: 2}
INVALID, RANGE = 1, 4


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


def synth(n, seed):
    return oracle.synth(n, oracle.F32, seed, 1, -1.0, 1.0)


def random_keys(rng, n, lo=0, hi=1 << 63):
    u = np.unique(rng.integers(lo, hi, 2 * n + 16, dtype=np.uint64))
    return np.sort(rng.choice(u, n, replace=False))


def moments(rng, count):
    return rng.standard_normal(count), rng.random(count) * 1e-3


def table(dtype, width, adam, key_end=KMAX):
    t = psg.Table(dtype, width, 0, key_end, 0)
    if adam:
        t.set_adam(*ADAM)
    return t


def state(t, adam=True):
    k, rows = t.dump()
    return (k, rows) + (t.dump_moments() if adam else ())


def assert_state(t, exp, adam=True):
    got = state(t, adam)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.size == e.size
        same(g, e)


def exported(t, cuts, adam, esize, off_rows=0, off_mom=0):
    """the table through psg_table_export, chunk by chunk: rows [cuts[i], cuts[i+1])
    land at their place in one set of output arrays (off_*: bytes the arrays
    start after a 16-B boundary)"""
    n, w = t.info().size, t.width
    ko = psg.DeviceBuffer(max(n, 1) * 8)
    ro = psg.DeviceBuffer(n * w * esize + 16)
    mo, vo = psg.DeviceBuffer(n * w * 8 + 16), psg.DeviceBuffer(n * w * 8 + 16)
    for a, b in zip(cuts[:-1], cuts[1:]):
        t.export(a, b - a, ko.ptr + a * 8, ro.ptr + off_rows + a * w * esize,
                 mo.ptr + off_mom + a * w * 8 if adam else None, vo.ptr + off_mom + a * w * 8 if adam else None)
    psg.device_sync()
    out = (ko.download(np.uint64, n), ro.download(BITS[esize], n * w, offset=off_rows))
    if adam:
        out += (mo.download(np.float64, n * w, offset=off_mom), vo.download(np.float64, n * w, offset=off_mom))
    return out


def nan_patterns(dtype):
    """a quiet NaN with a payload, a signalling NaN and a negative NaN with a
    payload: for F32 0x7fc00001, 0x7f800001 and 0xffc12345"""
    e, m = rs.FORMAT[dtype]
    inf, quiet, sign = ((1 << e) - 1) << m, 1 << (m - 1), 1 << (e + m)
    return np.array([inf | quiet | 1, inf | 1, sign | inf | quiet | (0x12345 & (quiet - 1))], dtype=rs.UINT[dtype])


def test_nan_patterns_are_the_ones_named():
    assert list(nan_patterns(rs.F32)) == [0x7fc00001, 0x7f800001, 0xffc12345]
    for dt in rs.FORMAT:
        assert rs.nan_mask(dt, nan_patterns(dt)).all()


@pytest.mark.parametrize("width", [3, 8])
@pytest.mark.parametrize("dtype", [psg.F32, psg.F64, psg.F16, psg.BF16], ids=["f32", "f64", "f16", "bf16"])
def test_bytes_are_kept(dtype, width):
    """Specials and NaNs with payloads, into an empty table and over present
    rows; W = 8 is the 16-B path for every dtype, W = 3 the element path."""
    pats = np.concatenate([rs.SPECIALS[dtype], nan_patterns(dtype)])
    n = 50
    rng = np.random.default_rng(dtype * 10 + width)
    keys = random_keys(rng, n)
    first = np.resize(pats, n * width)
    second = np.roll(first, 7)
    t = table(dtype, width, False)
    for vals in (first, second):
        t.assign(dev(keys), dev(vals), n)
        k, rows = t.dump()
        np.testing.assert_array_equal(k, keys)
        same(rows, vals)
        ek, er = exported(t, [0, n], False, ESIZE[dtype])
        np.testing.assert_array_equal(ek, keys)
        same(er, vals)


def test_a_push_from_zero_does_not_keep_the_bytes():
    """Why assign exists: a Push into an empty table is 0 + x."""
    width, n = 4, 30
    pats = np.concatenate([rs.SPECIALS[rs.F32], nan_patterns(rs.F32)])
    vals = np.resize(pats, n * width)
    keys = random_keys(np.random.default_rng(3), n)
    t = table(psg.F32, width, False)
    t.handle(psg.PUSH, dev(keys), dev(vals), None, n)
    got = bits(t.dump()[1]).ravel()
    minus_zero = vals == rs.specials(rs.F32)["-0"]
    assert minus_zero.any() and (got[minus_zero] == 0).all()  # 0 + -0.0 is +0.0
    a = table(psg.F32, width, False)
    a.assign(dev(keys), dev(vals), n)
    same(a.dump()[1], vals)


def cuts_of(n):
    return [0, n // 5, n // 2 + (1 if n > 2 else 0), n]


def check_grid(width, n, off_rows, off_mom):
    rng = np.random.default_rng(width * 7919 + n)
    keys = random_keys(rng, n)
    rows = synth(n * width, width + n)
    m, v = moments(rng, n * width)
    rb = psg.DeviceBuffer(rows.nbytes + 16)
    mb, vb = psg.DeviceBuffer(m.nbytes + 16), psg.DeviceBuffer(v.nbytes + 16)
    rb.upload(rows, offset=off_rows)
    mb.upload(m, offset=off_mom)
    vb.upload(v, offset=off_mom)
    t = table(psg.F32, width, True)
    t.assign(dev(keys), rb.ptr + off_rows, n, mb.ptr + off_mom, vb.ptr + off_mom)
    exp = (keys, rows, m, v)
    assert t.info().size == n
    assert_state(t, exp)
    for cuts in ([0, n], cuts_of(n)):
        for g, e in zip(exported(t, cuts, True, 4, off_rows, off_mom), exp):
            same(g, e)


@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("width", [1, 3, 4, 20, 64, 260])
def test_assign_dump_export_grid(width, n):
    """W = 1, 3: elements; 4, 20, 64, 260: 16-B rows and pairs of moments; 4097
    rows are several tiles at every width and the chunks [0, n/5), [n/5, n/2 + 1),
    [n/2 + 1, n) start inside one."""
    check_grid(width, n, 0, 0)


@pytest.mark.parametrize("width", [1, 3, 4, 20, 64, 260])
def test_unaligned_arrays_take_the_element_paths(width):
    """rows 4 B and moments 8 B after a 16-B boundary, in and out"""
    check_grid(width, 4097, 4, 8)


def test_the_widest_rows():
    """W = 4096: 64-KiB moment rows, one row a tile"""
    check_grid(4096, 3, 0, 0)


def test_inserts_move_rows_and_moments():
    width = 20
    rng = np.random.default_rng(11)
    every = random_keys(rng, 4097)
    present = every[::2]
    n = len(every)
    rows = synth(n * width, 5)
    m, v = moments(rng, n * width)
    # moments given: every row and moment is the assigned one, old or inserted
    t = table(psg.F32, width, True)
    t.update(psg.PUSH, dev(present), dev(synth(len(present) * width, 1)), None, len(present), LR, 0)
    cap0 = t.info().capacity
    t.assign(dev(every), dev(rows), n, dev(m), dev(v))
    assert t.info().size == n and t.info().capacity > cap0
    assert_state(t, (every, rows, m, v))
    # no moments given: present keys keep theirs, inserted keys have zeros
    t = table(psg.F32, width, True)
    t.update(psg.PUSH, dev(present), dev(synth(len(present) * width, 1)), None, len(present), LR, 0)
    _, _, m0, v0 = state(t)
    assert np.count_nonzero(m0) > m0.size // 2
    t.assign(dev(every), dev(rows), n)
    em, ev = np.zeros((n, width)), np.zeros((n, width))
    em[::2], ev[::2] = m0, v0
    assert_state(t, (every, rows, em, ev))


def fill(count, seed):
    b = psg.DeviceBuffer(count * 4)
    b.fill_synth(count, psg.F32, seed, 1, -1.0, 1.0)
    return b


@pytest.mark.parametrize("merged", [False, True], ids=["update", "merged"])
@pytest.mark.parametrize("width", [4, 3])
def test_resume_equals_uninterrupted(width, merged):
    rng = np.random.default_rng(width + 17 * merged)
    universe = random_keys(rng, 1500)
    k = 3 if merged else 1
    lists = [[np.sort(rng.choice(universe, 300 + 40 * j + it, replace=False)) for j in range(k)] for it in range(6)]

    def train(t, its):
        for it in its:
            ks = [dev(l) for l in lists[it]]
            gs = [fill(len(l) * width, 100 * it + j) for j, l in enumerate(lists[it])]
            if merged:
                t.update_merged(psg.PUSH, ks, gs, None, [len(l) for l in lists[it]], LR, it)
            else:
                t.update(psg.PUSH, ks[0], gs[0], None, len(lists[it][0]), LR, it)

    a = table(psg.F32, width, True)
    train(a, range(6))
    b = table(psg.F32, width, True)
    train(b, range(3))
    n = b.info().size
    ko, ro = psg.DeviceBuffer(n * 8), psg.DeviceBuffer(n * width * 4)
    mo, vo = psg.DeviceBuffer(n * width * 8), psg.DeviceBuffer(n * width * 8)
    b.export(0, n, ko, ro, mo, vo)
    psg.device_sync()
    c = table(psg.F32, width, True)
    c.assign(ko, ro, n, mo, vo)  # device to device
    assert_state(c, state(b))
    train(c, range(3, 6))
    assert a.info().size == c.info().size > n
    assert_state(c, state(a))


def test_rejections_write_nothing():
    width, end = 20, 1 << 30
    rng = np.random.default_rng(9)
    keys = random_keys(rng, 3000, 0, end - 1)
    fresh = np.setdiff1d(random_keys(rng, 500, 0, end - 1), keys)
    t = table(psg.F32, width, True, end)
    t.handle(psg.PUSH, dev(keys), dev(synth(len(keys) * width, 1)), None, len(keys))
    t.update(psg.PUSH, dev(keys[::3]), dev(synth(len(keys[::3]) * width, 2)), None, len(keys[::3]), LR, 0)
    before, cap0 = state(t), t.info().capacity
    base = np.union1d(keys[::2], fresh)
    swapped = base.copy()
    swapped[[700, 701]] = swapped[[701, 700]]
    repeated = base.copy()
    repeated[1200] = repeated[1199]
    at_end = np.append(base, np.uint64(end))
    for lst, code in ((swapped, INVALID), (repeated, INVALID), (at_end, RANGE)):
        n = len(lst)
        m, v = moments(rng, n * width)
        for mv in ((dev(m), dev(v)), (None, None)):
            with pytest.raises(psg.PsgError) as ei:
                t.assign(dev(lst), dev(synth(n * width, 3)), n, *mv)
            assert ei.value.code == code, str(ei.value)
            assert_state(t, before)
            assert t.info().size == len(keys) and t.info().capacity == cap0
    # export past the end
    size = t.info().size
    out = psg.DeviceBuffer(4 * width * 8)
    for first, count in ((size - 1, 2), (size + 1, 0), (0, size + 1)):
        with pytest.raises(psg.PsgError) as ei:
            t.export(first, count, None, out if count < 4 else None)
        assert ei.value.code == INVALID, str(ei.value)
    assert_state(t, before)
    # moments and a table without Adam state
    p = table(psg.F32, width, False, end)
    p.handle(psg.PUSH, dev(keys), dev(synth(len(keys) * width, 1)), None, len(keys))
    p0 = state(p, False)
    n = len(base)
    m, v = moments(rng, n * width)
    with pytest.raises(psg.PsgError) as ei:
        p.assign(dev(base), dev(synth(n * width, 3)), n, dev(m), dev(v))
    assert ei.value.code == INVALID and "Adam" in str(ei.value)
    with pytest.raises(psg.PsgError) as ei:
        p.export(0, 2, None, out, out, out)
    assert ei.value.code == INVALID and "Adam" in str(ei.value)
    assert_state(p, p0, False)
    # empty calls are no-ops, and the table still serves a good request
    t.assign(None, None, 0)
    t.export(size, 0, None, None)
    assert_state(t, before)
    t.assign(dev(base), dev(synth(len(base) * width, 4)), len(base))
    assert t.info().size == len(np.union1d(keys, fresh))


def test_strict_neighbours_see_the_assigned_state():
    """a Pull and an update after an assign give what the host mirror
    (oracle.lr_apply) gives from the assigned rows and moments"""
    width, n = 20, 2000
    rng = np.random.default_rng(21)
    keys = random_keys(rng, n)
    rows = synth(n * width, 1).reshape(n, width)
    m, v = (x.reshape(n, width) for x in moments(rng, n * width))
    t = table(psg.F32, width, True)
    t.assign(dev(keys), dev(rows), n, dev(m), dev(v))
    pick = np.sort(rng.choice(n, 700, replace=False))
    sub = keys[pick]
    out = psg.DeviceBuffer(len(sub) * width * 4)
    t.handle(psg.PULL, dev(sub), None, out, len(sub))
    same(out.download(np.float32, len(sub) * width), rows[pick])
    g = synth(len(sub) * width, 2)
    t.update(psg.PUSH | psg.PULL, dev(sub), dev(g), out, len(sub), LR, 2)
    w1, m1, v1 = (np.ascontiguousarray(x[pick]).ravel() for x in (rows, m, v))
    oracle.lr_apply(w1, g, LR, m1, v1, *ADAM, 2)
    same(out.download(np.float32, len(sub) * width), w1)
    rows[pick], m[pick], v[pick] = (x.reshape(len(sub), width) for x in (w1, m1, v1))
    assert_state(t, (keys, rows, m, v))


def test_keys_without_rows_are_inserted_and_nothing_else_is_written():
    """rows = NULL: how a checkpoint of many chunks is merged into the table once"""
    width = 20
    rng = np.random.default_rng(12)
    every = random_keys(rng, 4097)
    present = every[::2]
    t = table(psg.F32, width, True)
    t.update(psg.PUSH, dev(present), dev(synth(len(present) * width, 1)), None, len(present), LR, 0)
    _, r0, m0, v0 = state(t)
    with pytest.raises(psg.PsgError) as ei:
        t.assign(dev(every), None, len(every), dev(np.zeros(4)), dev(np.zeros(4)))
    assert ei.value.code == INVALID and "moments without rows" in str(ei.value)
    t.assign(dev(every), None, len(every))
    er = np.zeros((len(every), width), np.float32)
    em, ev = np.zeros((len(every), width)), np.zeros((len(every), width))
    er[::2], em[::2], ev[::2] = r0, m0, v0
    assert_state(t, (every, er, em, ev))
