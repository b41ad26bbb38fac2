"""The row table's lookup and erase (psg_table_lookup / psg_table_erase,
csrc/psg_rows.hip): rows read without inserting, and keys removed.

The mirror is a Python dict built from psg_table_dump / dump_moments.  Every
comparison is bit for bit, through unsigned views.  The definition of the erase
is the twin test: a table that took updates, an erase and more updates equals a
fresh table that was assigned the survivors and took the same further updates.
"""
import numpy as np
import pytest

import psg

pytestmark = pytest.mark.gpu

KEND = 1 << 40
LR = 0.05
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
BITS = {4: np.uint32, 8: np.uint64, 2: np.uint16}
INVALID, RANGE = 1, 4
DTYPES = {"f32": psg.F32, "f64": psg.F64, "f16": psg.F16, "bf16": psg.BF16}


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


def byte_table(dtype, width, keys, rng, key_begin=0, key_end=KEND):
    """a table whose rows are random BYTES, put there by psg_table_assign"""
    t = psg.Table(dtype, width, key_begin, key_end, 0)
    u = BITS[t.esize]
    rows = rng.integers(0, np.iinfo(u).max, len(keys) * width, dtype=u, endpoint=True)
    t.assign(dev(keys), dev(rows), len(keys))
    return t


def trained_table(width, keys, seed, steps=3):
    """an F32 Adam table after `steps` psg_table_update calls on all its keys"""
    t = psg.Table(psg.F32, width, 0, KEND, 0)
    t.set_adam(*ADAM)
    rng = np.random.default_rng(seed)
    dk = dev(keys)
    for it in range(steps):
        g = rng.uniform(-1, 1, len(keys) * width).astype(np.float32)
        t.update(psg.PUSH, dk, dev(g), None, len(keys), LR, it)
    return t


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


def mirror(t, adam=False):
    """{key: (row bits, m bits, v bits)} from the dumps"""
    k, rows = t.dump()
    r = bits(rows).reshape(len(k), t.width)
    if adam:
        m, v = (bits(x) for x in t.dump_moments())
        return {int(k[j]): (r[j].copy(), m[j].copy(), v[j].copy()) for j in range(len(k))}
    return {int(k[j]): (r[j].copy(),) for j in range(len(k))}


def assert_is(t, mir, adam=False):
    """the table holds exactly the mirror: keys in order, rows and moments"""
    k, rows = t.dump()
    exp = sorted(mir)
    assert int(t.info().size) == len(exp)
    np.testing.assert_array_equal(k, np.array(exp, dtype=np.uint64))
    if not exp:
        return
    np.testing.assert_array_equal(bits(rows).reshape(len(k), t.width), np.stack([mir[x][0] for x in exp]))
    if adam:
        m, v = (bits(x) for x in t.dump_moments())
        np.testing.assert_array_equal(m, np.stack([mir[x][1] for x in exp]))
        np.testing.assert_array_equal(v, np.stack([mir[x][2] for x in exp]))


def looked_up(t, q, out_off=0, want_out=True, want_found=True):
    """psg_table_lookup of the host list q -> (rows as bits [n, W] or None, found or None)"""
    n, w, u = len(q), t.width, BITS[t.esize]
    out = psg.DeviceBuffer(n * w * t.esize + 16) if want_out else None
    fnd = psg.DeviceBuffer(max(n, 1)) if want_found else None
    t.lookup(dev(q), out.ptr + out_off if out else None, fnd, n)
    rows = out.download(u, n * w, offset=out_off).reshape(n, w) if out else None
    return rows, (fnd.download(np.uint8, n) if fnd else None)


def expected(mir, q, width, u):
    rows = np.zeros((len(q), width), dtype=u)
    fnd = np.zeros(len(q), dtype=np.uint8)
    for i, key in enumerate(q):
        hit = mir.get(int(key))
        if hit is not None:
            rows[i], fnd[i] = hit[0], 1
    return rows, fnd


def check_lookup(t, mir, q, **kw):
    rows, fnd = looked_up(t, q, **kw)
    erows, efnd = expected(mir, q, t.width, BITS[t.esize])
    if rows is not None:
        np.testing.assert_array_equal(rows, erows)
    if fnd is not None:
        np.testing.assert_array_equal(fnd, efnd)


# ---- lookup: the grid ----------------------------------------------------------------
def lists(rng, keys, n):
    """ascending, shuffled and with repeats; half of each list's keys are present"""
    pres = rng.choice(keys, (n + 1) // 2, replace=False)
    absn = absent_keys(rng, keys, n // 2)
    asc = np.sort(np.concatenate([pres, absn]))
    shuf = rng.permutation(asc)
    # one absent key 300 times (a third of a list shorter than 900), the rest drawn with repeats
    often = min(300, n // 3)
    pool = np.concatenate([pres, absn])
    rep = np.concatenate([np.full(often, absent_keys(rng, np.concatenate([keys, absn]), 1)[0], dtype=np.uint64),
                          rng.choice(pool, n - often, replace=True)])
    return {"ascending": asc, "shuffled": shuf, "repeats": rng.permutation(rep)}


GRID = [("f32", w) for w in (1, 3, 4, 20, 64, 260)] + [(d, w) for d in ("f64", "f16", "bf16") for w in (3, 8)]


@pytest.mark.parametrize("dtype,width", GRID, ids=[f"{d}-w{w}" for d, w in GRID])
def test_lookup_grid(dtype, width):
    rng = np.random.default_rng(1000 + width + 7 * DTYPES[dtype])
    keys = random_keys(rng, 3000)
    t = byte_table(DTYPES[dtype], width, keys, rng)
    mir = mirror(t)
    snap = snapshot(t, False)
    for n in (1, 65, 4097):
        # 4097 keys, half of them present, of a table of 3000: a list of distinct
        # keys has room for 2049 present ones
        for order, q in lists(rng, keys, n).items():
            assert len(q) == n, (order, n)
            check_lookup(t, mir, q)
    assert_unchanged(t, snap, False)
    t.close()


def test_lookup_leaves_moments_alone():
    rng = np.random.default_rng(5)
    keys = random_keys(rng, 3000)
    for width in (4, 3):
        t = trained_table(width, keys, 50 + width)
        mir = mirror(t, True)
        snap = snapshot(t, True)
        for q in lists(rng, keys, 4097).values():
            check_lookup(t, mir, q)
        assert_unchanged(t, snap, True)
        t.close()


# ---- lookup: the edges ------------------------------------------------------------------
@pytest.fixture(scope="module")
def f32w4():
    rng = np.random.default_rng(77)
    keys = random_keys(rng, 3000)
    t = byte_table(psg.F32, 4, keys, rng)
    yield t, keys, mirror(t)
    t.close()


def test_presence_flips_at_the_tile_edges(f32w4):
    """present | absent | present, flipping exactly at 1023 | 1024 and 2047 | 2048"""
    t, keys, mir = f32w4
    rng = np.random.default_rng(78)
    pres = rng.choice(keys, 2048, replace=False)
    q = np.concatenate([pres[:1024], absent_keys(rng, keys, 1024), pres[1024:]])
    rows, fnd = looked_up(t, q)
    assert fnd[1023] == 1 and fnd[1024] == 0 and fnd[2047] == 0 and fnd[2048] == 1
    check_lookup(t, mir, q)
    check_lookup(t, mir, np.concatenate([q[1024:2048], pres[:1024], q[1024:2048]]))


def test_all_absent_all_present_and_an_empty_table(f32w4):
    t, keys, mir = f32w4
    rng = np.random.default_rng(79)
    check_lookup(t, mir, absent_keys(rng, keys, 1500))
    check_lookup(t, mir, keys)
    check_lookup(t, mir, rng.permutation(keys))
    e = psg.Table(psg.F32, 4, 0, KEND, 0)
    check_lookup(e, {}, keys[:1300])
    assert e.info().size == 0 and e.info().capacity == 0
    e.lookup(None, None, None, 0)
    e.close()


def test_out_or_found_may_be_null(f32w4):
    t, keys, mir = f32w4
    rng = np.random.default_rng(80)
    q = rng.permutation(np.concatenate([keys[::3], absent_keys(rng, keys, 700)]))
    check_lookup(t, mir, q, want_out=False)
    check_lookup(t, mir, q, want_found=False)
    with pytest.raises(psg.PsgError) as e:
        t.lookup(dev(q), None, None, len(q))
    assert e.value.code == INVALID


def test_out_off_16_byte_alignment_takes_the_element_body(f32w4):
    t, keys, mir = f32w4
    rng = np.random.default_rng(81)
    q = rng.permutation(np.concatenate([keys[:900], absent_keys(rng, keys, 400)]))
    check_lookup(t, mir, q, out_off=4)


def test_the_first_and_the_last_key_of_the_range():
    rng = np.random.default_rng(82)
    kb = 100
    keys = np.array([kb, kb + 5, KEND - 1], dtype=np.uint64)
    t = byte_table(psg.F32, 3, keys, rng, key_begin=kb)
    mir = mirror(t)
    check_lookup(t, mir, np.array([KEND - 1, kb, kb + 1, KEND - 2, kb, KEND - 1], dtype=np.uint64))
    t.close()
    t = psg.Table(psg.F32, 3, kb, KEND, 0)  # the same on a table that holds neither
    check_lookup(t, {}, np.array([KEND - 1, kb], dtype=np.uint64))
    t.close()


@pytest.mark.parametrize("width", [4, 3])
def test_special_values_come_back_as_bytes(width):
    pats = np.array([0x80000000, 0x7f800001, 0x7f800000, 0xff800000, 0xffc12345, 0x00000001], dtype=np.uint32)
    n = 40
    rng = np.random.default_rng(83)
    keys = random_keys(rng, n)
    rows = np.resize(pats, n * width)
    t = psg.Table(psg.F32, width, 0, KEND, 0)
    t.assign(dev(keys), dev(rows), n)
    q = rng.permutation(np.concatenate([keys, keys[:7]]))
    got, fnd = looked_up(t, q)
    assert fnd.all()
    pos = np.searchsorted(keys, q)
    np.testing.assert_array_equal(got, rows.reshape(n, width)[pos])
    t.close()


@pytest.mark.parametrize("width", [2049, 4096])
def test_rows_longer_than_a_tile(width):
    rng = np.random.default_rng(84 + width)
    keys = random_keys(rng, 9)
    t = byte_table(psg.F32, width, keys, rng)
    mir = mirror(t)
    q = rng.permutation(np.concatenate([keys, absent_keys(rng, keys, 4), keys[:2]]))
    snap = snapshot(t, False)
    check_lookup(t, mir, q)
    if width % 4 == 0:
        check_lookup(t, mir, q, out_off=4)
    assert_unchanged(t, snap, False)
    t.close()


@pytest.mark.parametrize("n,at", [(1, 0), (3000, 0), (3000, 1500), (3000, 2999)])
def test_a_key_outside_the_range_fails_the_lookup_and_writes_nothing(f32w4, n, at):
    t, keys, mir = f32w4
    snap = snapshot(t, False)
    q = keys[:n].copy()
    q[at] = KEND
    out = dev(np.full(n * 4, 0xA5A5A5A5, dtype=np.uint32))
    fnd = dev(np.full(n, 0x5A, dtype=np.uint8))
    with pytest.raises(psg.PsgError) as e:
        t.lookup(dev(q), out, fnd, n)
    assert e.value.code == RANGE
    assert (out.download(np.uint32, n * 4) == 0xA5A5A5A5).all()
    assert (fnd.download(np.uint8, n) == 0x5A).all()
    assert_unchanged(t, snap, False)
    check_lookup(t, mir, keys[:n])  # the next call is served


# ---- erase ----------------------------------------------------------------------------------
def erase_lists(rng, keys):
    S = len(keys)
    absn = absent_keys(rng, keys, 200)
    mixed = rng.permutation(np.concatenate([keys[5::7], keys[5::14], absn, absn[:50]]))
    return {
        "every third": keys[::3],
        "a stretch": keys[S // 3: S // 3 + S // 4],
        "first and last": keys[[0, S - 1]],
        "shuffled, repeats, absent": mixed,
        "every key": rng.permutation(keys),
        "none present": absn,
    }


def check_erase(t, mir, q, adam):
    """erase q; the table must equal the mirror minus q.  Returns the new mirror."""
    before = t.info()
    named = {int(x) for x in q} & set(mir)
    left = {k: v for k, v in mir.items() if k not in named}
    erased = t.erase(dev(q), len(q))
    assert erased == len(named)
    after = t.info()
    assert int(after.size) == len(left)
    if named:
        assert after.capacity <= max(2 * after.size, 1024)
    else:
        assert (after.capacity, after.rows, after.keys) == (before.capacity, before.rows, before.keys)
    assert_is(t, left, adam)
    return left


@pytest.mark.parametrize("width", [4, 8, 3])
def test_erase_on_adam_tables(width):
    rng = np.random.default_rng(200 + width)
    keys = random_keys(rng, 2500)
    for name, q in erase_lists(rng, keys).items():
        t = trained_table(width, keys, 300 + width)
        mir = mirror(t, True)
        left = check_erase(t, mir, q, True)
        # the erased keys are absent now, the survivors read back
        check_lookup(t, left, rng.permutation(keys)[:1100])
        if name == "every key":
            assert t.info().size == 0
            # an emptied table takes keys again
            t.update(psg.PUSH, dev(keys[:10]), dev(np.ones(10 * width, np.float32)), None, 10, LR, 0)
            assert t.info().size == 10
        t.close()


@pytest.mark.parametrize("dtype,width,adam", [("f16", 3, False), ("bf16", 10, False), ("f16", 8, False),
                                              ("f64", 3, False), ("f32", 4096, True)],
                         ids=["2B", "4B", "16B", "f64-8B-rows", "w4096-adam"])
def test_erase_move_units(dtype, width, adam):
    rng = np.random.default_rng(400 + width)
    S = 12 if width == 4096 else 1500
    keys = random_keys(rng, S)
    if adam:
        t = trained_table(width, keys, 401, steps=1)  # 64-KiB moment rows
    else:
        t = byte_table(DTYPES[dtype], width, keys, rng)
    mir = mirror(t, adam)
    left = check_erase(t, mir, rng.permutation(np.concatenate([keys[1::2], keys[1:4]])), adam)
    check_erase(t, left, keys[1::2], adam)  # none of them is left: a no-op
    t.close()


@pytest.mark.parametrize("S", [1, 1023, 1024, 1025, 4097])
def test_erase_across_the_compaction_tiles(S):
    """dead slots on both sides of every 1024-slot tile edge the table has"""
    rng = np.random.default_rng(500 + S)
    keys = random_keys(rng, S)
    t = trained_table(4, keys, 501, steps=1)
    mir = mirror(t, True)
    slots = [s for s in (0, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, S - 1) if s < S]
    left = check_erase(t, mir, keys[np.unique(slots)][::-1].copy(), True)
    # and the complement pattern: everything but the slots beside the edges
    if S > 1:
        lk = sorted(left)  # the compacted table's slots
        keep = {lk[s] for s in (0, 1023, 1024, 2047, 2048) if s < len(lk)}
        q = np.array([k for k in lk if k not in keep], dtype=np.uint64)
        check_erase(t, left, rng.permutation(q), True)
    t.close()


def further_updates(t, keys_a, keys_b, width, seed, merged):
    rng = np.random.default_rng(seed)
    for it, ks in ((3, keys_a), (4, keys_b)):
        g = [rng.uniform(-1, 1, len(ks) * width).astype(np.float32) for _ in range(2)]
        if merged:
            dk = dev(ks)
            t.update_merged(psg.PUSH, [dk, dk], [dev(g[0]), dev(g[1])], None, [len(ks), len(ks)], LR, it)
        else:
            t.update(psg.PUSH, dev(ks), dev(g[0]), None, len(ks), LR, it)


@pytest.mark.parametrize("merged", [False, True], ids=["update", "update_merged"])
@pytest.mark.parametrize("width", [4, 3])
def test_erase_then_train_equals_a_twin_assigned_the_survivors(width, merged):
    """The defining property.  The further updates name survivors, erased keys
    and keys never seen."""
    rng = np.random.default_rng(600 + width)
    keys = random_keys(rng, 2000)
    t = trained_table(width, keys, 601)
    gone = rng.permutation(np.concatenate([keys[::4], keys[100:300]]))
    k0, r0 = t.dump()
    m0, v0 = t.dump_moments()
    alive = ~np.isin(k0, gone)
    assert t.erase(dev(gone), len(gone)) == int((~alive).sum())
    twin = psg.Table(psg.F32, width, 0, KEND, 0)
    twin.set_adam(*ADAM)
    n = int(alive.sum())
    twin.assign(dev(k0[alive]), dev(r0[alive]), n, dev(m0[alive]), dev(v0[alive]))
    fresh = absent_keys(rng, keys, 150)
    keys_a = np.sort(np.concatenate([keys[::2], fresh[:100]]))  # survivors, erased keys, new keys
    keys_b = np.sort(np.concatenate([keys[1::3], keys[:40:4], fresh[50:]]))
    keys_b = np.unique(keys_b)
    for x in (t, twin):
        further_updates(x, keys_a, keys_b, width, 602, merged)
    assert_is(t, mirror(twin, True), True)
    assert t.info().size == twin.info().size
    t.close()
    twin.close()


@pytest.mark.parametrize("width", [4, 3])
def test_an_erased_key_pushed_again_starts_as_a_key_never_seen(width):
    rng = np.random.default_rng(700 + width)
    keys = random_keys(rng, 600)
    t = trained_table(width, keys, 701)
    back = int(keys[300])
    new = int(absent_keys(rng, keys, 1)[0])
    assert t.erase(dev(np.array([back], dtype=np.uint64)), 1) == 1
    pair = np.array(sorted([back, new]), dtype=np.uint64)
    g = np.tile(rng.uniform(-1, 1, width).astype(np.float32), 2)
    t.update(psg.PUSH, dev(pair), dev(g), None, 2, LR, 3)
    mir = mirror(t, True)
    for a, b in zip(mir[back], mir[new]):
        np.testing.assert_array_equal(a, b)
    assert mir[back][1].any(), "the moments did not move"
    t.close()


def test_an_erase_that_is_rejected_or_empty_changes_nothing():
    rng = np.random.default_rng(800)
    keys = random_keys(rng, 1500)
    t = trained_table(4, keys, 801)
    snap = snapshot(t, True)
    q = keys[:1200].copy()
    q[700] = KEND
    with pytest.raises(psg.PsgError) as e:
        t.erase(dev(q), len(q))
    assert e.value.code == RANGE
    assert_unchanged(t, snap, True)
    assert t.erase(None, 0) == 0
    assert t.erase(dev(absent_keys(rng, keys, 300)), 300) == 0
    assert_unchanged(t, snap, True)
    e = psg.Table(psg.F32, 4, 0, KEND, 0)
    assert e.erase(dev(keys), len(keys)) == 0
    assert e.info().size == 0
    e.close()
    t.close()
