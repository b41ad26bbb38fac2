"""Long mixed request sequences on ONE row table (psg_table_*, csrc/psg_rows.hip)
against ONE host model (tests/row_model.py): what outlives a call on a table a
server keeps for days.  The cached scratch (slots, the any-order block carved at
offsets that depend on n, the flag words), growth and shrink with moments
attached, the sort width through the table's own plumbing, and a refused
request between served ones.

An executor walks a sequence of step records on a psg.Table and on the model.
After EVERY step it compares the step's reply (out, found, the erased count, the
merged calls' path, an export's arrays), info().size and capacity, dump() and,
on Adam tables, dump_moments().  Keys are compared as integers, everything else
bit for bit through unsigned views; the sequences are free of NaN
(test_row_model.py asserts it), so there is no exemption.  After a refusal: the
error code, the reply buffers still hold their sentinel, the table is unchanged.

The random sequences are row_model.SEQUENCES, the ones test_row_model.py runs dry
and whose contents it asserts.  The scripted ones walk the named edges.
"""
import numpy as np
import pytest

import psg
import row_model as rm
from row_model import F32, PUSH, PULL, Refused, step

pytestmark = pytest.mark.gpu

PP = PUSH | PULL
FILL = 0xA5
BITS = {2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}
assert (psg.F32, psg.F64, psg.F16, psg.BF16) == (rm.F32, rm.F64, rm.F16, rm.BF16)
assert (psg.MERGED_SAME_LIST, psg.MERGED_SORTED, psg.POOL_SUM, psg.POOL_MEAN) == (rm.SAME_LIST, rm.SORTED, rm.POOL_SUM,
                                                                                  rm.POOL_MEAN)


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype.itemsize])


def same(got, exp, what):
    np.testing.assert_array_equal(bits(got).ravel(), bits(exp).ravel(), err_msg=what)


class Arrays:
    """The device arrays of one request.  put: a host array into a buffer,
    shifted by `shift` elements from the buffer's (16-B aligned) start.  reply:
    a buffer of sentinel bytes the call is to write."""

    def __init__(self, shift):
        self.shift, self.keep, self.replies = shift, [], {}

    def put(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        off = self.shift * a.dtype.itemsize
        b = psg.DeviceBuffer(a.nbytes + 32)
        b.upload(a, offset=off)
        self.keep.append(b)
        return b.ptr + off

    def reply(self, name, dtype, count):
        dtype = np.dtype(dtype)
        off = self.shift * dtype.itemsize
        b = psg.DeviceBuffer(count * dtype.itemsize + 32)
        b.upload(np.full(b.nbytes, FILL, np.uint8))
        self.replies[name] = (b, off, dtype, count)
        return b.ptr + off

    def get(self, name):
        b, off, dtype, count = self.replies[name]
        return b.download(dtype, count, offset=off)

    def untouched(self):
        for name, (b, _, _, _) in self.replies.items():
            assert np.all(b.download(np.uint8, b.nbytes) == FILL), f"{name} was written by a refused call"


def call(t, s, a):
    """the step on the table; the reply in the model's terms"""
    op, w = s["op"], t.width
    st = rm.rs.STORAGE[t.dtype]
    keys = None
    if "keys" in s:
        keys, n = a.put(rm.u64(s["keys"])), len(s["keys"])
    if op in ("handle", "handle_any", "update", "update_any"):
        out = a.reply("out", st, n * w) if s["flags"] & PULL and n else None
        vals = a.put(s.get("vals"))
        if op.startswith("handle"):
            getattr(t, op)(s["flags"], keys, vals, out, n)
        else:
            getattr(t, op)(s["flags"], keys, vals, out, n, s["lr"], s["iteration"])
        return {"out": a.get("out") if out else None}
    if op == "update_merged":
        fr = s["frames"]
        ns = [len(f[0]) for f in fr]
        pull = bool(s["flags"] & PULL)
        outs = [a.reply(f"out{j}", np.float32, nj * w) if pull and nj else None for j, nj in enumerate(ns)]
        path = t.update_merged(s["flags"], [a.put(rm.u64(f[0])) if len(f[0]) else None for f in fr],
                               [a.put(f[2]) if len(f[0]) else None for f in fr], outs if pull else None, ns, s["lr"],
                               s["iteration"])
        return {"outs": [a.get(f"out{j}") if o else None for j, o in enumerate(outs)], "path": path}
    if op == "update_pooled_merged":
        fr = s["frames"]
        frames = [(a.put(rm.u64(f[0])) if len(f[0]) else None, a.put(rm.u64(f[1])) if f[1] is not None else None,
                   a.put(f[2]) if len(f[2]) else None) for f in fr]
        path = t.update_pooled_merged(frames, [len(f[0]) for f in fr], [len(f[1]) - 1 if f[1] is not None else 0 for f in fr],
                                      s["lr"], s["iteration"])
        return {"path": path}
    if op == "lookup":
        out, found = a.reply("out", st, n * w), a.reply("found", np.uint8, n)
        t.lookup(keys, out, found, n)
        return {"out": a.get("out"), "found": a.get("found")}
    if op == "erase":
        return {"erased": t.erase(keys, n)}
    if op == "assign":
        t.assign(keys, a.put(s.get("vals")), n, a.put(s.get("m")), a.put(s.get("v")))
        return {}
    if op == "export":
        c, adam = s["count"], t.adam() is not None
        ko, ro = a.reply("keys", np.uint64, c), a.reply("rows", st, c * w)
        mo, vo = (a.reply("m", np.float64, c * w), a.reply("v", np.float64, c * w)) if adam else (None, None)
        t.export(s["first"], c, ko, ro, mo, vo)
        psg.device_sync()
        return {k: a.get(k) for k in a.replies}
    if op == "clear":
        t.clear()
        return {}
    if op == "set_adam":
        t.set_adam(*s["adam"])
        return {}
    offsets, nb = a.put(rm.u64(s["offsets"])), len(s["offsets"]) - 1
    weights = a.put(s["weights"])
    if op in ("lookup_pooled", "lookup_pooled_weighted"):
        out = a.reply("out", st, nb * w)
        if op == "lookup_pooled":
            t.lookup_pooled(keys, offsets, out, n, nb)
        else:
            t.lookup_pooled_weighted(keys, offsets, weights, s["mode"], out, n, nb)
        return {"out": a.get("out")}
    grads = a.put(s["vals"])
    if op == "update_pooled":
        t.update_pooled(keys, offsets, grads, n, nb, s["lr"], s["iteration"])
    else:
        t.update_pooled_weighted(keys, offsets, weights, s["mode"], grads, n, nb, s["lr"], s["iteration"])
    return {}


class Walk:
    """one table and one model, fed the same steps"""

    def __init__(self, profile):
        self.t = psg.Table(profile["dtype"], profile["width"], profile.get("key_begin", 0), profile.get("key_end", rm.KMAX),
                           profile.get("capacity", 0))
        self.m = rm.new_model(profile)
        self.i = 0

    def check_state(self, what):
        t, m = self.t, self.m
        info = t.info()
        assert info.size == m.size, f"{what}: size"
        assert info.capacity == m.capacity, f"{what}: capacity"
        k, rows = t.dump()
        np.testing.assert_array_equal(k, m.keys, err_msg=f"{what}: keys")
        same(rows, m.rows, f"{what}: rows")
        assert (t.adam() is not None) == (m.adam is not None)
        if m.adam:
            mm, vv = t.dump_moments()
            same(mm, m.m, f"{what}: first moments")
            same(vv, m.v, f"{what}: second moments")

    def step(self, s):
        what = f"step {self.i} ({rm.op_name(s)})"
        self.i += 1
        want = rm.apply_step(self.m, s)
        a = Arrays(s["shift"])
        try:
            got = call(self.t, s, a)
        except psg.PsgError as e:
            got = Refused(e.code)
        if isinstance(want, Refused):
            assert isinstance(got, Refused) and got.code == want.code, f"{what}: {got} where {want} was due"
            a.untouched()
        else:
            assert not isinstance(got, Refused), f"{what}: {got}"
            for k, exp in want.items():
                if k == "outs":
                    for j, e in enumerate(exp):
                        if e is not None and len(e):  # an empty frame has no reply
                            same(got["outs"][j], e, f"{what}: reply of frame {j}")
                elif k in ("erased", "path"):
                    if k in got:  # the pooled update calls report no path
                        assert got[k] == exp, f"{what}: {k} {got[k]} where {exp} was due"
                elif k == "keys":
                    np.testing.assert_array_equal(got[k], exp, err_msg=f"{what}: exported keys")
                elif exp is not None:
                    same(got[k], exp, f"{what}: {k}")
        self.check_state(what)
        return want

    def run(self, steps):
        for s in steps:
            self.step(s)


# ---- the random sequences -------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed,profile", rm.SEQUENCES, ids=[s[0] for s in rm.SEQUENCES])
def test_random_sequence(name, seed, profile):
    Walk(profile).run(rm.make_sequence(seed, profile))


# ---- scripted sequences for the named edges ---------------------------------------------------------
GRID = [(3, False), (3, True), (4, False), (4, True)]  # element body / 16-B body, SGD / Adam
GRID_IDS = ["w3-sgd", "w3-adam", "w4-sgd", "w4-adam"]
KEND = 1 << 40


class Script:
    """step records for a scripted walk, values from the generator's streams"""

    def __init__(self, width, adam, seed, key_begin=0, key_end=KEND):
        self.profile = dict(kind="train", dtype=F32, width=width, adam=adam, key_begin=key_begin, key_end=key_end)
        self.g = rm.Generator(seed, self.profile)
        self.rng, self.w = self.g.rng, width
        self.walk = Walk(self.profile)
        self.it = 0
        if adam:
            self.walk.step(step("set_adam", adam=rm.ADAM))

    def keys(self, n):
        return np.sort(self.rng.choice(self.g.universe, n, replace=False))

    def do(self, op, keys=None, **kw):
        n = 0 if keys is None else len(keys)
        if keys is not None:
            kw["keys"] = rm.u64(keys)
        if op in ("handle", "handle_any", "assign") and kw.get("flags", PUSH) & PUSH:
            kw.setdefault("vals", self.g.values(n * self.w))
        if op in ("update", "update_any"):
            kw.setdefault("vals", self.g.grads(n * self.w))
        if op.startswith("handle") or op in ("update", "update_any", "update_merged"):
            kw.setdefault("flags", PP)
        if "offsets" in kw and op.startswith("update"):
            kw.setdefault("vals", self.g.grads((len(kw["offsets"]) - 1) * self.w))
        if op.startswith("update"):
            kw.setdefault("iteration", self.it)
            self.it += 1
        return self.walk.step(step(op, **kw))

    def frames(self, lists, offsets=None):
        offsets = offsets or [None] * len(lists)
        return [(rm.u64(q), None if o is None else rm.u64(o),
                 self.g.grads((len(q) if o is None else len(o) - 1) * self.w)) for q, o in zip(lists, offsets)]


@pytest.mark.parametrize("width,adam", GRID, ids=GRID_IDS)
def test_capacity_walk(width, adam):
    """1023, 1024, 1025, 2049 rows; down to 1025, 1024, 1023, 1; up to 1500; every
    key erased; an any-order update that inserts; clear; a merged round.  Rows and
    moments follow through every reallocation."""
    s = Script(width, adam, 1)
    K, rng, t = s.keys(3000), s.rng, s.walk.t
    s.do("handle", K[:1023], flags=PUSH)
    assert t.info().capacity == 1024
    s.do("update", K[:1024])
    assert (t.info().size, t.info().capacity) == (1024, 1024)
    s.do("handle_any", rng.permutation(K[:1025]))
    assert (t.info().size, t.info().capacity) == (1025, 2048)
    s.do("update_any", rng.permutation(np.concatenate([K[:2049], K[2040:2049]])), shift=1)
    assert (t.info().size, t.info().capacity) == (2049, 4096)
    for lo, hi, left in ((1025, 2049, 1025), (1024, 1025, 1024), (1023, 1024, 1023), (1, 1023, 1)):
        assert s.do("erase", rng.permutation(K[lo:hi]))["erased"] == hi - lo
        assert (t.info().size, t.info().capacity) == (left, max(left, 1024))
        s.do("update", K[:left:7])  # the survivors train on
    s.do("update_any", rng.permutation(np.concatenate([K[:1500], K[:30]])))
    assert (t.info().size, t.info().capacity) == (1500, 2048)
    assert s.do("erase", rng.permutation(K[:1600]))["erased"] == 1500
    assert (t.info().size, t.info().capacity) == (0, 0)
    s.do("update_any", rng.choice(K[100:400], 900), shift=1)
    assert t.info().size <= 300 and t.info().capacity == 1024
    s.do("clear")
    assert (t.info().size, t.info().capacity) == (0, 1024)
    assert s.do("update_merged", frames=s.frames([rng.choice(K[:500], 400), rng.choice(K[:500], 3), K[:500]]))["path"] == rm.SORTED
    assert s.do("update_merged", frames=s.frames([K[200:1700]] * 3))["path"] == rm.SAME_LIST
    assert t.info().capacity == 2048


@pytest.mark.parametrize("width", [3, 4])
@pytest.mark.parametrize("place", ["new", "populated", "after_clear", "after_erase_all"])
def test_set_adam_placement(place, width):
    """set_adam on an empty new table, on a populated one, after clear (capacity
    kept, size 0) and after an erase of every key; then inserts and training.  A
    row inserted after set_adam starts from zero moments, whatever the moment
    allocation held: a trained Adam table of the same shape is freed first, so
    that the allocations that follow find its moments in memory."""
    old = Script(width, True, 2)
    old.do("update_any", old.rng.choice(old.keys(2000), 4000))
    old.walk.t.close()
    s = Script(width, False, 3)
    K, rng, t = s.keys(2600), s.rng, s.walk.t
    if place != "new":
        s.do("handle", K[:1500], flags=PUSH)
        s.do("update", K[:1500:2])
    if place == "after_clear":
        s.do("clear")
        assert (t.info().size, t.info().capacity) == (0, 1500)
    if place == "after_erase_all":
        assert s.do("erase", K[:1500])["erased"] == 1500
    s.do("set_adam", adam=rm.ADAM)
    s.do("handle_any", rng.permutation(K[1200:1900]), flags=PUSH)  # inserts next to rows already there
    s.do("update_any", rng.choice(K[1000:2600], 2500))  # trains old and new rows, inserts more, grows
    s.do("update", K[::3])
    s.do("update_pooled", rng.choice(K, 600), offsets=s.g.bags(600))
    m, v = t.dump_moments()
    assert np.any(m != 0) and np.all(v >= 0)


@pytest.mark.parametrize("width,adam", GRID, ids=GRID_IDS)
def test_scratch_under_a_short_call(width, adam):
    """a large any-order request leaves its slots and its carved scratch under
    the short calls of every other kind that follow on the same table"""
    s = Script(width, adam, 4)
    K, rng = s.keys(3000), s.rng
    s.do("handle_any", rng.choice(K[:900], 5000))
    s.do("handle_any", K[77:78])
    s.do("handle_any", np.repeat(K[901:902], 3))
    s.do("lookup", rng.permutation(np.concatenate([rng.choice(K[:902], 2049), K[950:2998]])))
    s.do("update_pooled", K[[5, 2999]], offsets=[0, 1, 2])
    s.do("lookup_pooled_weighted", K[[3, 950, 3]], offsets=[0, 3], weights=np.float32([0.5, -2.0, 1.25]))
    assert s.do("erase", K[5:6])["erased"] == 1
    hot = [rng.choice(K[10:50], 120) for _ in range(16)]
    assert s.do("update_merged", frames=s.frames(hot))["path"] == rm.SORTED
    assert s.do("lookup", K[5:6])["found"][0] == 0
    s.do("update_any", rng.choice(K[:900], 4097), shift=1)
    s.do("lookup_pooled", K[5:6], offsets=[0, 0, 1, 1])
    s.do("update", K[5:6])
    s.do("handle", K[:3], flags=PULL)


@pytest.mark.parametrize("width,adam", GRID, ids=GRID_IDS)
def test_refusals_in_the_middle(width, adam):
    """every refusal between two served calls of other kinds: rows, moments and
    size stay, the reply keeps its sentinel, the next call is served"""
    kb, ke = 1000, KEND
    s = Script(width, adam, 5, kb, ke)
    K, rng, w = s.keys(3000), s.rng, width
    refused = lambda r, code: isinstance(r, Refused) and r.code == code
    s.do("handle", K[:2000], flags=PUSH)
    s.do("update_any", rng.choice(K[:2200], 3000))
    bad = K[:1500].copy()
    bad[[1400, 1401]] = bad[[1401, 1400]]
    assert refused(s.do("handle", bad), rm.INVALID)
    s.do("lookup", rng.choice(K, 700))
    q = rng.choice(K[:2200], 1300)
    q[1299] = ke
    assert refused(s.do("update_any", q), rm.RANGE)
    s.do("handle", K[100:1200])
    q = rng.choice(K, 1300).astype(np.uint64)
    q[1250] = kb - 1
    assert refused(s.do("lookup", q), rm.RANGE)
    s.do("update", K[500:2500])
    q, o = rng.choice(K, 600), s.g.bags(600)
    o1, o2, o3 = o.copy(), o.copy(), o.copy()
    o1[0] = 1
    o2[len(o) // 2] = o2[len(o) // 2 + 1] + np.uint64(1)
    o3[-1] = 601
    assert refused(s.do("lookup_pooled", q, offsets=o1), rm.INVALID)
    assert s.do("erase", K[2400:2410])["erased"] == 10
    assert refused(s.do("update_pooled", q, offsets=o2), rm.INVALID)
    s.do("handle_any", rng.choice(K, 65))
    assert refused(s.do("lookup_pooled_weighted", q, offsets=o3, weights=rng.uniform(-2, 2, 600).astype(np.float32)),
                   rm.INVALID)
    lists = [rng.choice(K, 900), rng.choice(K, 2500).astype(np.uint64), rng.choice(K, 30)]
    assert s.do("update_merged", frames=s.frames(lists))["path"] == rm.SORTED
    lists[1][2400] = ke  # in the last tile of its frame
    assert refused(s.do("update_merged", frames=s.frames(lists)), rm.RANGE)
    s.do("lookup_pooled", q, offsets=o)
    assert refused(s.do("update_pooled_merged", frames=s.frames(lists, [None, s.g.bags(2500), None])), rm.RANGE)
    s.do("update_pooled", q, offsets=o)
    same3 = [K[:1300].copy() for _ in range(3)]
    same3[2][1299] = ke  # the same-list round's last frame differs in its last key, out of range
    assert refused(s.do("update_merged", frames=s.frames(same3)), rm.RANGE)
    s.do("assign", K[2900:])


# 1 << 41 is the six-pass case
KEY_ENDS = [2, 256, 257, 65536, 65537, (1 << 24) + 1, 1 << 33, 1 << 41, (1 << 48) + 1, 1 << 56, (1 << 64) - 1]
SORT_CASES = [(ke, kb) for ke in KEY_ENDS for kb in ([0] + ([ke // 3] if ke // 3 >= 1 and ke - ke // 3 >= 2 else []))]


@pytest.mark.parametrize("width,adam", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("key_end,key_begin", SORT_CASES, ids=[f"end{ke:#x}-begin{kb:#x}" for ke, kb in SORT_CASES])
def test_sort_widths_through_the_table(key_end, key_begin, width, adam):
    """bit_width(key_end - 1) gives 1 to 8 passes of the any-order sort and last
    passes of 1 and 8 bits: about 2000 occurrences through the accumulate, the
    update, the pooled round and the weighted pooled update, which pick the
    sort's result buffer, cut its runs and read perm each in its own way, in the
    element body (width 3) and the 16-B body (width 4; the last round's arrays
    are shifted, so it takes the element body on 16-B rows), with SGD and Adam"""
    assert [-(-(ke - 1).bit_length() // 8) for ke in KEY_ENDS] == [1, 1, 2, 2, 3, 4, 5, 6, 7, 7, 8]
    s = Script(width, adam, key_end % 1009 + key_begin % 13, key_begin, key_end)
    rng = s.rng
    span = key_end - key_begin
    pool = np.unique(np.concatenate([rng.integers(key_begin, key_end, min(600, 4 * span), dtype=np.uint64),
                                     rm.u64([key_begin, key_end - 1])]))
    assert len(pool) >= 2
    draw = lambda n: rm.u64(rng.choice(pool, n))
    q = draw(2000)
    assert not rm.strictly_ascending(q)
    s.do("handle_any", q)
    s.do("update_any", draw(2000))
    r = s.do("update_pooled_merged", frames=s.frames([draw(1200), draw(800)], [s.g.bags(1200), None]))
    assert r["path"] == rm.SORTED
    s.do("update_pooled_weighted", draw(1999), offsets=s.g.bags(1999), weights=rng.uniform(-2, 2, 1999).astype(np.float32))
    assert s.do("update_merged", frames=s.frames([draw(700), draw(700)]), shift=1)["path"] == rm.SORTED
