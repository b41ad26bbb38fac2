"""Seeded initial rows on the GPU (psg_table_set_init / psg_init_rows,
csrc/psg_rows.hip) against the numpy restatement (tests/row_init_model.py).
Everything is compared as bytes.

  the generator    psg_init_rows in all four dtypes, the 16-B path and the element
                   path (an odd width, or `out` one element off 16 B), one row, a
                   tile of rows exactly and one more, the keys whose halves matter;
  inserting calls  every call that inserts, each on a fresh table, against
                   RowInitModel: rows, moments, size, capacity and reply;
  insert behaviour the order and grouping of inserts, growth with moments
                   attached, an erased key named again;
  no-insert reads  psg_table_lookup and the three pooled lookups answer an absent
                   id with the bytes an insert would store and insert nothing.
The executor is test_rows_sequences_gpu.py's, on a table and a model that were
both given the same initializer.
"""
import numpy as np
import pytest

import psg
import row_init_model as rim
import row_model as rm
import test_rows_sequences_gpu as seq
from row_init_model import init_rows
from row_model import F32, F64, F16, BF16, PUSH, PULL, Refused, step

pytestmark = pytest.mark.gpu

PP = PUSH | PULL
KEND = seq.KEND
INIT = (0x0123_4567_89AB_CDEF, -0.125, 0.25)  # seed, lo, hi
ESIZE = {F32: 4, F64: 8, F16: 2, BF16: 2}
NAMES = {F32: "f32", F64: "f64", F16: "f16", BF16: "bf16"}
UNITS_PER_TILE = 2048  # kUnitsPerTile, csrc/psg_internal.h
same = seq.same


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def rows_per_tile(upr):  # rows_per_tile, csrc/psg_internal.h
    return 1 if upr >= UNITS_PER_TILE else UNITS_PER_TILE // upr


# ---- psg_init_rows against the mirror ---------------------------------------------------------------
SPECIAL_KEYS = rm.u64([0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, rm.KMAX - 1, 1, (1 << 63) + 5])


def device_init_rows(keys, dtype, width, shift, init=INIT):
    """psg_init_rows into a sentinel-filled buffer, `shift` elements off its 16-B start"""
    n, es = len(keys), ESIZE[dtype]
    st = rm.rs.STORAGE[dtype]
    dk = psg.DeviceBuffer.from_numpy(rm.u64(keys))
    buf = psg.DeviceBuffer(n * width * es + 64)
    buf.upload(np.full(buf.nbytes, seq.FILL, np.uint8))
    psg.init_rows(buf.ptr + shift * es, dk, n, dtype, width, *init)
    raw = buf.download(np.uint8, buf.nbytes)
    lo, hi = shift * es, shift * es + n * width * es
    assert np.all(raw[:lo] == seq.FILL) and np.all(raw[hi:] == seq.FILL), "written outside the rows"
    return raw[lo:hi].view(st).reshape(n, width)


@pytest.mark.parametrize("width", [1, 3, 4, 5, 8, 12, 4096])
@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16], ids=[NAMES[d] for d in (F32, F64, F16, BF16)])
def test_init_rows_against_the_mirror(dtype, width):
    rng = np.random.default_rng(width * 8 + dtype)
    es = ESIZE[dtype]
    pool = np.concatenate([SPECIAL_KEYS, rng.integers(0, 1 << 64, 4000, dtype=np.uint64, endpoint=False)])
    for shift in (0, 1):
        vec = (width * es) % 16 == 0 and shift == 0
        upr = width * es // 16 if vec else (width + 3) // 4  # 16-B units, or blocks of four elements
        rpt = rows_per_tile(upr)
        for n in (1, rpt, rpt + 1):
            q = rm.u64(rng.choice(pool, n))  # shuffled, with repeats
            if n >= len(SPECIAL_KEYS):
                q[rng.choice(n, len(SPECIAL_KEYS), replace=False)] = SPECIAL_KEYS
            else:
                q[0] = SPECIAL_KEYS[(shift + width) % 4]
            got = device_init_rows(q, dtype, width, shift)
            same(got, init_rows(q, dtype, width, *INIT), f"{NAMES[dtype]} w{width} shift {shift} n {n}")


def test_init_rows_seed_range_and_constant():
    q = rm.u64([5, 5 + (1 << 32), 6])
    a = device_init_rows(q, F32, 8, 0, (7, -1.0, 1.0))
    b = device_init_rows(q, F32, 8, 0, (7 + (1 << 32), -1.0, 1.0))
    same(a, init_rows(q, F32, 8, 7, -1.0, 1.0), "seed 7")
    same(b, init_rows(q, F32, 8, 7 + (1 << 32), -1.0, 1.0), "the seed's high word")
    assert not np.any(a == b) and not np.any(a[0] == a[1])
    for dtype in (F32, F64, F16, BF16):
        c = device_init_rows(q, dtype, 5, 0, (7, 0.5, 0.5))
        same(c, init_rows(q, dtype, 5, 7, 0.5, 0.5), "lo == hi")
        assert np.all(rm.to_acc(dtype, c) == 0.5)
    # Philox's first known answer: key 0 under seed 0, u = x >> 8 over 2^24 with lo 0 and hi 1
    x = np.array([0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], np.uint32)
    got = device_init_rows(rm.u64([0]), F32, 4, 0, (0, 0.0, 1.0))[0]
    same(got, (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), "known answer")


# ---- a table and a model with the same initializer -------------------------------------------------------
class InitWalk(seq.Walk):
    def __init__(self, profile, init=INIT):
        super().__init__(profile)
        self.m = rim.new_model(profile, init)
        self.t.set_init(*init)
        assert self.t.init() == (psg.INIT_UNIFORM, init[0], float(np.float32(init[1])), float(np.float32(init[2])))


class InitScript(seq.Script):
    """seq.Script on an InitWalk; any dtype (the optimizer calls need F32).

    do() returns the MODEL's reply, as seq.Script.do does: the device's reply to
    the same step was compared with it byte for byte inside Walk.step, and that
    comparison is the device check.  What a test asserts on a returned reply
    afterwards says in plain terms what both hold.  initial() is the other
    side of such an assertion: the rows psg_init_rows itself wrote on the
    device, checked against the mirror on the way."""

    def __init__(self, width, adam, seed, dtype=F32, init=INIT):
        self.profile = dict(kind="train" if dtype == F32 else "accumulate", dtype=dtype, width=width, adam=adam,
                            key_begin=0, key_end=KEND)
        self.g = rm.Generator(seed, self.profile)
        self.rng, self.w = self.g.rng, width
        self.walk = InitWalk(self.profile, init)
        self.it = 0
        if adam:
            self.walk.step(step("set_adam", adam=rm.ADAM))

    def initial(self, keys):
        keys = rm.u64(keys)
        got = device_init_rows(keys, self.profile["dtype"], self.w, 0)
        same(got, init_rows(keys, self.profile["dtype"], self.w, *INIT), "psg_init_rows against the mirror")
        return got


GRID = seq.GRID
GRID_IDS = seq.GRID_IDS
HALF = [(3, F16), (8, F16), (3, BF16), (8, BF16), (3, F64), (4, F64)]
HALF_IDS = [f"w{w}-{NAMES[d]}" for w, d in HALF]


def bags_of(n, rng):
    """offsets over n positions: an empty bag first, inside and last"""
    cuts = np.sort(rng.integers(0, n + 1, max(1, n // 3)))
    return np.sort(np.concatenate([[0, 0], cuts, [cuts[len(cuts) // 2]], [n, n]])).astype(np.uint64)


# ---- every inserting call, each on a fresh table -----------------------------------------------------------
OPT_CALLS = ["update", "update_any", "update_merged_same", "update_merged_sorted", "update_pooled",
             "update_pooled_weighted", "update_pooled_mean", "update_pooled_merged"]
ACC_CALLS = ["push", "pull", "pushpull", "any_push", "any_pull", "any_pushpull", "assign_no_rows", "assign_rows"]


def first_call(s, name, K):
    """the named call as the FIRST request of a fresh table: every key is inserted by it"""
    rng = s.rng
    shuffled = rm.u64(rng.permutation(np.concatenate([K, K[:40], K[5:6].repeat(9)])))
    if name in ("push", "pull", "pushpull"):
        return s.do("handle", K, flags={"push": PUSH, "pull": PULL, "pushpull": PP}[name])
    if name.startswith("any_"):
        return s.do("handle_any", shuffled, flags={"any_push": PUSH, "any_pull": PULL, "any_pushpull": PP}[name])
    if name == "assign_no_rows":
        return s.walk.step(step("assign", keys=K))
    if name == "assign_rows":
        return s.do("assign", K[::2])
    if name == "update":
        return s.do("update", K)
    if name == "update_any":
        return s.do("update_any", shuffled)
    if name == "update_merged_same":
        r = s.do("update_merged", frames=s.frames([K, K, K]))
        assert r["path"] == rm.SAME_LIST
        return r
    if name == "update_merged_sorted":
        r = s.do("update_merged", frames=s.frames([shuffled[:300], K[:0], shuffled[300:]]))
        assert r["path"] == rm.SORTED
        return r
    if name == "update_pooled":  # the strict path (an ascending list), then the sorted one on a second table
        return s.do("update_pooled", K, offsets=bags_of(len(K), rng))
    if name == "update_pooled_weighted":
        return s.do("update_pooled_weighted", shuffled, offsets=bags_of(len(shuffled), rng),
                    weights=rng.uniform(-2, 2, len(shuffled)).astype(np.float32))
    if name == "update_pooled_mean":
        return s.do("update_pooled_weighted", shuffled, offsets=bags_of(len(shuffled), rng), mode=rm.POOL_MEAN)
    if name == "update_pooled_merged":
        o = bags_of(300, rng)
        return s.do("update_pooled_merged", frames=s.frames([shuffled[:300], K[:200], shuffled[300:]],
                                                            [o, None, bags_of(len(shuffled) - 300, rng)]))
    raise ValueError(name)


def after_first_call(s, K):
    """what the walk has compared bit for bit, said once more in plain terms: the
    table holds the keys, and a key nothing was pushed to is its initial row"""
    t = s.walk.t
    keys, rows = t.dump()
    assert len(keys) and np.all(np.isin(keys, K))
    r = s.do("lookup", K)  # the rows as they are; a key the call did not name is still absent
    np.testing.assert_array_equal(r["found"], np.isin(K, keys).astype(np.uint8))


@pytest.mark.parametrize("width,adam", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("name", OPT_CALLS + ACC_CALLS)
def test_inserting_call_f32(name, width, adam):
    s = InitScript(width, adam, 11)
    K = s.keys(1100)  # more than 1024: the first insert allocates past the minimum capacity
    first_call(s, name, K)
    assert s.walk.t.info().size == (550 if name == "assign_rows" else 1100)
    if name in ("pull", "any_pull", "assign_no_rows"):  # nothing was added: the table IS the initial rows
        same(s.walk.t.dump()[1], s.initial(K), "rows of a table that only inserted")
    if adam and name in ACC_CALLS:
        m, v = s.walk.t.dump_moments()
        assert not m.any() and not v.any()  # the moments of a new row stay zero
    after_first_call(s, K)
    # a second call of the same kind: half the keys present, half new, next to them
    first_call(s, name, np.unique(np.concatenate([K[::2], s.keys(500)])))


@pytest.mark.parametrize("width,dtype", HALF, ids=HALF_IDS)
@pytest.mark.parametrize("name", ACC_CALLS)
def test_inserting_call_other_dtypes(name, width, dtype):
    s = InitScript(width, False, 12, dtype)
    K = s.keys(1100)
    first_call(s, name, K)
    if name in ("pull", "any_pull", "assign_no_rows"):
        same(s.walk.t.dump()[1], s.initial(K), "rows of a table that only inserted")
    first_call(s, name, np.unique(np.concatenate([K[::2], s.keys(500)])))


# ---- insert behaviour ------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [3, 4])
def test_insertion_order_independence(width):
    """the same 3000 keys as one request, as thirty requests in another order, and as bags"""
    a, b, c = (InitScript(width, False, 13) for _ in range(3))
    K = a.keys(3000)
    rng = np.random.default_rng(13)
    a.do("handle", K, flags=PULL)
    for part in np.array_split(rng.permutation(K), 30):
        b.do("handle_any", np.concatenate([part, part[:2]]), flags=PULL)
    q = rm.u64(rng.permutation(np.concatenate([K, K[:100]])))
    offsets = bags_of(len(q), rng)
    c.do("update_pooled", q, offsets=offsets, vals=np.zeros((len(offsets) - 1) * width, np.float32))  # row - 0 is the row
    ka, ra = a.walk.t.dump()
    for other in (b, c):
        ko, ro = other.walk.t.dump()
        np.testing.assert_array_equal(ka, ko)
        same(ra, ro, "dump")
    same(ra, a.initial(K), "the initial rows")


@pytest.mark.parametrize("width", [3, 4])
def test_growth_keeps_rows_and_moments(width):
    """an Adam table from 1000 to 1100 rows across the 1024 boundary"""
    s = InitScript(width, True, 14)
    K, t = s.keys(1100), s.walk.t
    pick = np.sort(s.rng.choice(1100, 1000, replace=False))
    old = K[pick]
    new = np.setdiff1d(K, old)
    s.do("update", old)
    s.do("update", old[::3])
    assert (t.info().size, t.info().capacity) == (1000, 1024)
    rows0, (m0, v0) = t.dump()[1], t.dump_moments()
    assert m0.any() and v0.any()
    s.do("handle_any", rm.u64(s.rng.permutation(np.concatenate([new, old[:50]]))), flags=PULL)
    assert (t.info().size, t.info().capacity) == (1100, 2048)
    keys, rows = t.dump()
    m, v = t.dump_moments()
    was = np.isin(keys, old)
    same(rows[was], rows0, "old rows")
    same(m[was], m0, "old first moments")
    same(v[was], v0, "old second moments")
    same(rows[~was], s.initial(new), "new rows")
    assert not m[~was].any() and not v[~was].any()
    s.do("update_any", rm.u64(s.rng.permutation(K)))  # old and new rows train on


@pytest.mark.parametrize("width,adam", GRID, ids=GRID_IDS)
def test_erased_key_starts_again_from_its_initial_row(width, adam):
    s = InitScript(width, adam, 15)
    K = s.keys(1500)
    s.do("update_any", rm.u64(s.rng.permutation(K)))
    gone = K[100:700:2]
    assert s.do("erase", gone)["erased"] == len(gone)
    r = s.do("lookup", gone)  # absent again: the initial row, nothing inserted
    assert not r["found"].any()
    same(r["out"], s.initial(gone), "lookup of erased keys")
    same(s.do("handle", gone, flags=PULL)["out"], s.initial(gone), "erased keys named again")
    s.do("clear")  # the setting stays
    assert s.walk.t.init()[0] == psg.INIT_UNIFORM
    same(s.do("handle", K[:70], flags=PULL)["out"], s.initial(K[:70]), "after clear")


# ---- the reads that never insert ------------------------------------------------------------------------------
READ_GRID = [(3, F32), (4, F32), (3, F64), (4, F64), (3, F16), (8, F16), (3, BF16), (8, BF16)]
READ_IDS = [f"w{w}-{NAMES[d]}" for w, d in READ_GRID]


@pytest.mark.parametrize("width,dtype", READ_GRID, ids=READ_IDS)
def test_lookup_answers_an_absent_id_with_its_initial_row(width, dtype):
    s = InitScript(width, False, 16, dtype)
    K, t, rng = s.keys(2600), s.walk.t, s.rng
    s.do("handle", K[:1300], flags=PUSH)
    info = t.info()
    before = (info.size, info.capacity, info.rows, info.keys)
    for shift in (0, 1):
        q = rm.u64(rng.permutation(np.concatenate([rng.choice(K, 2100), K[1300:1302].repeat(4)])))
        r = s.do("lookup", q, shift=shift)
        absent = ~np.isin(q, K[:1300])
        assert 500 < absent.sum() < 1800
        np.testing.assert_array_equal(r["found"], (~absent).astype(np.uint8))
        same(r["out"][absent], s.initial(q[absent]), "absent ids")
        info = t.info()
        assert (info.size, info.capacity, info.rows, info.keys) == before  # untouched, nothing reallocated
    pulled = s.do("handle_any", q, flags=PULL, shift=1)  # the Pull that follows inserts and answers the same bytes
    same(pulled["out"], r["out"], "the Pull after the lookup")
    assert t.info().size > before[0]
    bad = q.copy()
    bad[len(bad) - 3] = np.uint64(KEND)
    assert isinstance(s.do("lookup", bad), Refused)  # PSG_ERR_RANGE, and the walk saw nothing written


@pytest.mark.parametrize("width,dtype", READ_GRID, ids=READ_IDS)
def test_pooled_lookups_add_the_initial_row_of_an_absent_id(width, dtype):
    s = InitScript(width, False, 17, dtype)
    K, t, rng = s.keys(900), s.walk.t, s.rng
    present, absent = K[:500], K[500:]
    s.do("handle", present, flags=PUSH)
    # bags: empty, all absent, mixed (with repeats), one absent id, a long mixed bag, empty
    lists = [K[:0], absent[:5], np.concatenate([present[:3], absent[5:8], present[1:2], absent[5:6]]), absent[9:10],
             rng.choice(K, 300), K[:0]]
    q = rm.u64(np.concatenate(lists))
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    weights = rng.uniform(-2, 2, len(q)).astype(np.float32)
    st = rm.rs.STORAGE[dtype]
    acc_t = np.float64 if dtype == F64 else np.float32
    one = rm.to_acc(dtype, s.initial(absent[9:10]))[0]  # the bag of one absent id: what psg_init_rows wrote for it
    w_one = weights[int(offsets[3])].astype(acc_t)
    for shift in (0, 1):
        size = t.info().size
        r = s.do("lookup_pooled", q, offsets=offsets, shift=shift)["out"].view(st).reshape(-1, width)
        assert not seq.bits(r[0]).any() and not seq.bits(r[5]).any()  # an empty bag is a row of +0
        same(r[3], rm.from_acc(dtype, acc_t(0) + one), "sum over one absent id")
        r = s.do("lookup_pooled_weighted", q, offsets=offsets, weights=weights, shift=shift)["out"]
        same(r.view(st).reshape(-1, width)[3], rm.from_acc(dtype, acc_t(0) + w_one * one), "weight times one absent id")
        r = s.do("lookup_pooled_weighted", q, offsets=offsets, mode=rm.POOL_MEAN, shift=shift)["out"]
        same(r.view(st).reshape(-1, width)[3], rm.from_acc(dtype, (acc_t(0) + one) / acc_t(1)), "mean over one absent id")
        assert t.info().size == size  # nothing was inserted
    bad = q.copy()
    bad[len(bad) - 2] = np.uint64(KEND)
    for kw in (dict(), dict(weights=weights), dict(mode=rm.POOL_MEAN)):
        op = "lookup_pooled_weighted" if kw else "lookup_pooled"
        assert isinstance(s.do(op, bad, offsets=offsets, **kw), Refused)
    # a table of absent ids only: the forward pass of the first training step
    e = InitScript(width, False, 18, dtype)
    e.do("lookup_pooled", q, offsets=offsets)
    e.do("lookup_pooled_weighted", q, offsets=offsets, weights=weights)
    e.do("lookup_pooled_weighted", q, offsets=offsets, mode=rm.POOL_MEAN)
    assert e.walk.t.info().size == 0


SEQ_PROFILES = [
    ("train-adam-w3", 201, dict(kind="train", dtype=F32, width=3, adam=True)),
    ("train-sgd-w4", 202, dict(kind="train", dtype=F32, width=4, adam=False)),
    ("accumulate-bf16-w3", 203, dict(kind="accumulate", dtype=BF16, width=3)),
    ("accumulate-f64-w4", 204, dict(kind="accumulate", dtype=F64, width=4)),
]


@pytest.mark.parametrize("name,seed,profile", SEQ_PROFILES, ids=[p[0] for p in SEQ_PROFILES])
def test_random_sequence_on_a_table_with_an_initializer(name, seed, profile):
    """one walk of row_model.make_sequence, compared after every step; the
    sequence must hold what makes the walk mean something"""
    steps = rm.make_sequence(seed, profile)
    walk = InitWalk(profile)
    looked = absent = 0
    for s in steps:
        if s["op"] in ("lookup", "lookup_pooled", "lookup_pooled_weighted"):
            looked += len(s["keys"])
            absent += int((~walk.m._find(rm.u64(s["keys"]))[1]).sum())
        walk.step(s)
    assert absent > 200 and looked - absent > 200, (looked, absent)
    assert seq.bits(walk.t.dump()[1]).any()
