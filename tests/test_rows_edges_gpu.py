"""The row table's value side (csrc/psg_rows.hip): the unit bodies, widths and
values the other row tests never reach.

  1  half and F64 rows on every unit size, real-valued (and, for F16,
     overflowing) data, through the strict and the any-order call
  2  inserts that move existing rows, per move unit (2 B, 4 B, 16 B)
  3  rows longer than one block pass and one tile, up to the maximum width
  4  special values (row_specials.py) through the accumulate kernels
  5  the row optimizer against tests/golden/lr_ref.npz, the reference's own rounds
  6  optimizer edges: subnormal and underflowing lr * g, overflowing rows

Accumulate is checked against the scalar oracle.Store on expanded keys
rank * W + j (RowOracle of test_rows_gpu.py); the optimizer against the host
mirror of test_rows_any_gpu.py / test_rows_merged_gpu.py (oracle.lr_apply) or,
in 5, against the fixture alone.  Every comparison is bit for bit.  The one
exception is in 4: a NaN is compared by class and position, not by payload,
and the number of NaNs is asserted exactly.
"""
import os

import numpy as np
import pytest

import oracle
import psg
import row_specials as rs
from test_rows_any_gpu import Mirror as AnyMirror
from test_rows_gpu import BITS, ES, KMAX, NPT, RowOracle, bits, dev, random_keys, same
from test_rows_merged_gpu import Mirror as MergedMirror

pytestmark = pytest.mark.gpu

LR = 0.05
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
SAME, SORTED = psg.MERGED_SAME_LIST, psg.MERGED_SORTED
DT_ID = {psg.F32: "f32", psg.F64: "f64", psg.F16: "f16", psg.BF16: "bf16"}
P, PP, PL = psg.PUSH, psg.PUSH | psg.PULL, psg.PULL


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


def real(n, dtype, seed, scale=1.0):
    """real-valued data in [-scale, scale) for every dtype"""
    return oracle.synth(n, dtype, seed, 1, -scale, scale)


def repeats_list(rng, pool, extra):
    """every key of pool once and `extra` more occurrences, shuffled; never strictly ascending"""
    lst = rng.permutation(np.concatenate([pool, rng.choice(pool, extra)]))
    if len(lst) > 1 and np.all(lst[1:] > lst[:-1]):
        lst = lst[::-1].copy()
    return lst


class Mirror(AnyMirror):
    """rows and moments on the host: update() of test_rows_any_gpu (any list, in
    rounds) and merged() of test_rows_merged_gpu on one state."""
    merged = MergedMirror.merged


# ---- the rigs ---------------------------------------------------------------------
class AccRig:
    """A table and its oracle, fed the same accumulate requests."""

    def __init__(self, dtype, width, all_keys):
        self.dtype, self.w = dtype, width
        self.t = psg.Table(dtype, width, 0, KMAX, 0)
        self.o = RowOracle(dtype, width, all_keys)
        self.nans = 0  # NaNs the next compare has to find (4: special values)

    def compare(self, got, exp):
        g, e = rs.nan_mask(self.dtype, got), rs.nan_mask(self.dtype, exp)
        np.testing.assert_array_equal(g, e)
        assert int(g.sum()) == self.nans
        np.testing.assert_array_equal(bits(got).ravel()[~g.ravel()], bits(exp).ravel()[~e.ravel()])

    def request(self, flags, keys, vals=None, any_order=False, voff=0, ooff=0):
        """the request on both; compares the Pull's reply; returns it.  voff /
        ooff: bytes by which vals / out are shifted inside their buffers."""
        n = len(keys)
        nb = n * self.w * ES[self.dtype]
        dk = dev(np.asarray(keys, dtype=np.uint64))
        dv = out = None
        if flags & psg.PUSH:
            dv = psg.DeviceBuffer(nb + 16)
            dv.upload(vals, offset=voff)
        if flags & psg.PULL:
            out = psg.DeviceBuffer(nb + 16)
        call = self.t.handle_any if any_order else self.t.handle
        call(flags, dk, dv.ptr + voff if dv else None, out.ptr + ooff if out else None, n)
        exp = self.o.handle(flags, keys, vals)
        if not flags & psg.PULL:
            return None
        got = out.download(NPT[self.dtype], n * self.w, offset=ooff)
        self.compare(got, exp)
        return got

    def check_dump(self):
        k, rows = self.t.dump()
        ok, orows = self.o.dump()
        np.testing.assert_array_equal(k, ok)
        self.compare(rows, orows)
        assert self.t.info().size == len(ok)


class OptRig:
    """An F32 table and its mirror, fed the same optimizer requests.  off: bytes
    by which every gradient and reply array is shifted inside its buffer."""

    def __init__(self, width, all_keys, adam, off=0):
        self.w, self.off = width, off
        self.t = psg.Table(psg.F32, width, 0, KMAX, 0)
        if adam:
            self.t.set_adam(*ADAM)
        self.o = Mirror(width, all_keys, ADAM if adam else None)

    def seed(self, keys, vals):
        self.t.handle(psg.PUSH, dev(keys), dev(vals), None, len(keys))
        self.o.accumulate(keys, vals)

    def _grads(self, g):
        b = psg.DeviceBuffer(g.nbytes + 16)
        b.upload(g, offset=self.off)
        return b

    def update(self, flags, keys, grads, iteration, lr=LR, any_order=False):
        n = len(keys)
        g = self._grads(grads)
        out = psg.DeviceBuffer(n * self.w * 4 + 16) if flags & psg.PULL else None
        call = self.t.update_any if any_order else self.t.update
        call(flags, dev(keys), g.ptr + self.off, out.ptr + self.off if out else None, n, lr, iteration)
        exp = self.o.update(keys, grads, lr, iteration)
        if out is not None:
            same(out.download(np.float32, n * self.w, offset=self.off), exp)

    def merged(self, flags, keys_list, grads_list, iteration, lr=LR):
        ns = [len(x) for x in keys_list]
        dk = [dev(x) for x in keys_list]
        dg = [self._grads(g) for g in grads_list]
        do = [psg.DeviceBuffer(n * self.w * 4 + 16) for n in ns] if flags & psg.PULL else None
        path = self.t.update_merged(flags, dk, [b.ptr + self.off for b in dg],
                                    [b.ptr + self.off for b in do] if do else None, ns, lr, iteration)
        exp, _ = self.o.merged(keys_list, grads_list, lr, iteration)
        if do:
            for b, e, n in zip(do, exp, ns):
                same(b.download(np.float32, n * self.w, offset=self.off), e)
        return path

    def check(self):
        p = self.o.present
        k, rows = self.t.dump()
        np.testing.assert_array_equal(k, self.o.u[p])
        same(rows, self.o.rows[p])
        assert self.t.info().size == int(p.sum())
        if self.o.adam:
            m, v = self.t.dump_moments()
            assert m.shape == v.shape == (int(p.sum()), self.w)
            same(m, self.o.m[p])
            same(v, self.o.v[p])


# ---- 1. half and F64 rows on every unit size ---------------------------------------
# halves: 2: 4-B move; 3: 2-B move; 8: one 16-B unit; 10: 20-B rows; 24: 3 units;
# 264: 33 units (no power of two).  F64: 1, 3: element body; 2: one unit; 6: 3 units.
VALUES = [(dt, w, 1.0) for dt in (psg.F16, psg.BF16) for w in (2, 3, 8, 10, 24, 264)]
VALUES += [(psg.F64, w, 1.0) for w in (1, 2, 3, 6)]
# F16 in [-60000, 60000): some sums overflow to inf (max 65504), many round
VALUES += [(psg.F16, w, 60000.0) for w in (2, 3, 8, 10, 24, 264)]
VALUE_IDS = [f"{DT_ID[dt]}-w{w}-x{int(s)}" for dt, w, s in VALUES]


@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("dtype,width,scale", VALUES, ids=VALUE_IDS)
def test_strict_call_on_real_valued_rows(dtype, width, scale, n):
    rng = np.random.default_rng(dtype * 1000003 + width * 101 + n)
    keys = random_keys(rng, n)
    rig = AccRig(dtype, width, keys)
    rig.request(P, keys, real(n * width, dtype, 11, scale))
    got = rig.request(PP, keys, real(n * width, dtype, 12, scale))
    same(rig.request(PL, keys), got)
    rig.check_dump()


@pytest.mark.parametrize("dtype,width,scale", VALUES, ids=VALUE_IDS)
def test_any_order_call_with_hot_keys_on_real_valued_rows(dtype, width, scale):
    """4097 occurrences of 500 keys (the `repeats` list of test_rows_any_gpu):
    the segment walk applies step about eight times to one register."""
    rng = np.random.default_rng(dtype * 31 + width)
    keys = rng.choice(random_keys(rng, 500), 4097)
    n = len(keys)
    rig = AccRig(dtype, width, keys)
    rig.request(P, keys, real(n * width, dtype, 21, scale), any_order=True)
    rig.request(PP, keys, real(n * width, dtype, 22, scale), any_order=True)
    pulled = rig.request(PL, keys, any_order=True).reshape(n, width)
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    same(pulled, pulled[first][inv])  # every occurrence is answered with the row
    rig.check_dump()


@pytest.mark.parametrize("dtype,width,off", [(psg.F16, 8, 2), (psg.BF16, 8, 2), (psg.F64, 2, 8)],
                         ids=["f16", "bf16", "f64"])
def test_vector_and_element_body_agree_on_one_table(dtype, width, off):
    """16-B rows with vals (and out) one element into their buffers: the element
    body.  Then aligned requests, the 16-B body, on the same table."""
    rng = np.random.default_rng(70 + dtype)
    n = 4097
    keys = random_keys(rng, n)
    hot = rng.choice(keys[:300], 2000)
    rig = AccRig(dtype, width, keys)
    rig.request(P, keys, real(n * width, dtype, 31), voff=off)
    rig.request(PP, keys, real(n * width, dtype, 32), voff=off, ooff=off)
    rig.request(PP, hot, real(len(hot) * width, dtype, 33), any_order=True, voff=off, ooff=off)
    rig.request(PL, keys, ooff=off)
    rig.request(PP, keys, real(n * width, dtype, 34))
    rig.request(PP, hot, real(len(hot) * width, dtype, 35), any_order=True)
    rig.request(PP, keys, real(n * width, dtype, 36), voff=off)  # vals off alone: element body again
    rig.request(PL, keys)
    rig.check_dump()


# ---- 2. inserts that move existing rows, per move unit -----------------------------
@pytest.mark.parametrize("dtype,width", [(psg.F16, 3), (psg.BF16, 10), (psg.F16, 8), (psg.F64, 3)],
                         ids=["f16-w3-2B", "bf16-w10-4B", "f16-w8-16B", "f64-w3-4B"])
def test_insert_moves_rows_of_every_unit_size(dtype, width):
    """The scheme of test_rows_gpu.test_insert_moves_rows: push a; push every
    other key of a plus new keys before, between and after (the table grows);
    pull the union."""
    rng = np.random.default_rng(dtype * 97 + width)
    n = 1500
    a = random_keys(rng, n, 1 << 20, 1 << 40)
    new = np.concatenate([random_keys(rng, 200, 0, 1 << 20), random_keys(rng, n, 1 << 20, 1 << 40),
                          random_keys(rng, 200, 1 << 40, 1 << 41)])
    new = np.setdiff1d(new, a)
    b = np.union1d(a[::2], new)
    both = np.union1d(a, b)
    rig = AccRig(dtype, width, both)
    rig.request(P, a, real(len(a) * width, dtype, 1))
    cap_a = rig.t.info().capacity
    assert rig.t.info().size == len(a)
    rig.check_dump()
    rig.request(P, b, real(len(b) * width, dtype, 2))
    assert rig.t.info().size == len(both) and rig.t.info().capacity > cap_a  # merged and grown
    rig.request(PL, both)
    rig.check_dump()


# ---- 3. wide rows --------------------------------------------------------------------
# 257: element body, upr 257 > kBlock (RowWalk's dr == 0), 7 rows a tile;
# 2049: element body, rows_per_tile's 1-row branch; 4096: the 16-B body at upr
# 1024, 2 rows a tile; 4096 with arrays 4 B off: the element body at upr 4096;
# F64 4096: the 16-B body at upr 2048 == the units of a tile.
WIDE = {"w257": (psg.F32, 257, 0), "w2049": (psg.F32, 2049, 0), "w4096": (psg.F32, 4096, 0),
        "w4096_off4": (psg.F32, 4096, 4), "f64_w4096": (psg.F64, 4096, 0)}
WIDE_ACC = [(c, n) for c in WIDE for n in (1, 5, 65)] + [("w257", 4097)]
WIDE_OPT = [(c, n) for c, n in WIDE_ACC if WIDE[c][0] == psg.F32]


@pytest.mark.parametrize("case,n", WIDE_ACC)
def test_wide_rows_accumulate(case, n):
    dtype, width, off = WIDE[case]
    rng = np.random.default_rng(width * 13 + n + off)
    keys = random_keys(rng, n)
    lst = repeats_list(rng, keys, min(n, 64) // 2 + 2)
    rig = AccRig(dtype, width, keys)
    rig.request(P, keys, real(n * width, dtype, 1), voff=off)
    got = rig.request(PP, keys, real(n * width, dtype, 2), voff=off, ooff=off)
    same(rig.request(PL, keys, ooff=off), got)
    rig.request(PP, lst, real(len(lst) * width, dtype, 3), any_order=True, voff=off, ooff=off)
    rig.request(PL, lst, any_order=True, ooff=off)
    rig.check_dump()


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("case,n", WIDE_OPT)
def test_wide_rows_update(case, n, adam):
    """update, update_any and update_merged on both paths; with Adam the moments
    too (mom_col at width 4096 keeps its pairs 2048 doubles apart)."""
    _, width, off = WIDE[case]
    rng = np.random.default_rng(width * 17 + n + off + adam)
    keys = random_keys(rng, n)
    g = lambda rows, seed: real(rows * width, psg.F32, seed)
    rig = OptRig(width, keys, adam, off)
    rig.seed(keys[::2], g(len(keys[::2]), 1))  # every other row present, the rest inserted
    rig.update(P, keys, g(n, 2), 0)
    rig.update(PP, keys, g(n, 3), 1)
    lst = repeats_list(rng, keys, min(n, 64) // 2 + 2)
    rig.update(PP, lst, g(len(lst), 4), 2, any_order=True)
    assert rig.merged(PP, [keys] * 3, [g(n, 5 + j) for j in range(3)], 3) == SAME
    frames = [rng.choice(keys, n + 1), rng.choice(keys, n), rng.permutation(keys)]
    assert rig.merged(PP, frames, [g(len(x), 8 + j) for j, x in enumerate(frames)], 7) == SORTED
    rig.check()


def test_adam_moment_rows_of_the_maximum_width_move():
    """3 rows, then 40 with keys between them: the insert moves 16-KiB value rows
    and 64-KiB moment rows, one row a tile."""
    width = 4096
    rng = np.random.default_rng(40)
    b = random_keys(rng, 40)
    a = b[[5, 20, 35]]
    rig = OptRig(width, b, True)
    rig.update(P, a, real(3 * width, psg.F32, 1), 0)
    assert rig.t.info().size == 3
    rig.update(PP, b, real(40 * width, psg.F32, 2), 1)
    assert rig.t.info().size == 40
    rig.update(PP, a, real(3 * width, psg.F32, 3), 2)
    rig.check()


# ---- 4. special values through the accumulate kernels -----------------------------
# each dtype on its 16-B body and on its element body
SPECIAL_GRID = [(psg.F16, 8), (psg.F16, 3), (psg.BF16, 8), (psg.BF16, 3), (psg.F32, 4), (psg.F32, 3), (psg.F64, 2),
                (psg.F64, 3)]


@pytest.mark.parametrize("any_order", [False, True], ids=["handle", "handle_any"])
@pytest.mark.parametrize("dtype,width", SPECIAL_GRID, ids=[f"{DT_ID[dt]}-w{w}" for dt, w in SPECIAL_GRID])
def test_special_values_through_the_accumulate_kernels(dtype, width, any_order):
    """The cross product of row_specials.SPECIALS, row-major over ceil(pairs / W)
    rows (zero padding): Push a into the empty table, PushPull b, Pull.  Each
    dtype on its 16-B body and on its element body.  The NaNs sit at the two
    (+inf, -inf) pairs, in the reply and in the table, and nowhere else — so
    the mask hides no finite, infinite, zero or subnormal result."""
    a, b = rs.pairs(dtype)
    rows = -(-len(a) // width)
    va, vb = np.zeros(rows * width, rs.UINT[dtype]), np.zeros(rows * width, rs.UINT[dtype])
    va[:len(a)], vb[:len(b)] = a, b
    assert int(rs.inf_pairs_mask(dtype, va, vb).sum()) == rs.N_NAN
    rng = np.random.default_rng(dtype * 7 + width)
    keys = random_keys(rng, rows)
    if any_order:
        keys = rng.permutation(keys)
        assert not np.all(keys[1:] > keys[:-1])
    rig = AccRig(dtype, width, keys)
    rig.request(P, keys, rs.storage(dtype, va), any_order=any_order)
    rig.check_dump()  # 0 + a: no NaN yet
    rig.nans = rs.N_NAN
    got = rig.request(PP, keys, rs.storage(dtype, vb), any_order=any_order)
    np.testing.assert_array_equal(rs.nan_mask(dtype, got), rs.inf_pairs_mask(dtype, va, vb))
    rig.request(PL, keys, any_order=any_order)
    rig.check_dump()


# ---- 5. the row optimizer against the reference's own rounds ------------------------
LRG = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_ref.npz"))
GOLDEN = [(str(c), w, len(LRG[f"{c}_w0"]) // w) for c in LRG["cases"] if len(LRG[f"{c}_w0"]) == 4099
          for w in (1, 4, 64, 4096)]
GOLDEN += [("adam_lr05", 4, 257), ("adam_lr05", 3, 343), ("adam_skips", 3, 259)]


@pytest.mark.parametrize("call", ["update", "update_merged", "update_any"])
@pytest.mark.parametrize("case,width,rows", GOLDEN, ids=[f"{c}-w{w}" for c, w, _ in GOLDEN])
def test_update_against_the_reference_rounds(case, width, rows, call):
    """The first rows * width elements of a fixture case as rows of the table:
    every round's reply and the final rows equal the fixture's, which the
    reference's own Adam.h computed.  OptUnit against the reference, not the oracle."""
    n = rows * width
    assert 0 < n <= len(LRG[f"{case}_w0"])
    lr = float(LRG[f"{case}_lr"][0])
    t = psg.Table(psg.F32, width, 0, KMAX, 0)
    if bool(LRG[f"{case}_adam"][0]):
        t.set_adam(lr, 0.9, 0.999, 1e-8)
    keys = np.arange(rows, dtype=np.uint64) * np.uint64(7) + np.uint64(3)
    dk = dev(keys)
    t.handle(psg.PUSH, dk, dev(LRG[f"{case}_w0"][:n]), None, rows)  # 0 + w is exact
    out = psg.DeviceBuffer(n * 4)
    exp = None
    for r, it in enumerate(LRG[f"{case}_iters"]):
        g = dev(np.ascontiguousarray(LRG[f"{case}_merged"][r][:n]))
        if call == "update":
            t.update(PP, dk, g, out, rows, lr, int(it))
        elif call == "update_any":
            t.update_any(PP, dk, g, out, rows, lr, int(it))
        else:
            assert t.update_merged(PP, [dk], [g], [out], [rows], lr, int(it)) == SAME
        exp = LRG[f"{case}_out"][r][:n]
        np.testing.assert_array_equal(bits(out.download(np.float32, n)), bits(exp), err_msg=f"round {r}")
    k, got = t.dump()
    np.testing.assert_array_equal(k, keys)
    same(got.ravel(), exp)


# ---- 6. optimizer edges ----------------------------------------------------------------
FLT_MAX = np.float32(3.4028234663852886e38)
MIN_NORMAL = np.float32(1.1754943508222875e-38)
# lr = 0.05.  In units of the smallest f32 subnormal (2^-149, about 1.4e-45):
# g = 7 -> lr * g = 0.35: underflows to zero; 9 -> 0.45: to zero; 21 -> 1.05:
# one; 30 -> 1.5 and a little (0.05f is above 0.05): two; 1e-40, 1e-38: subnormal g and
# product; 1e-37, 2e-37: normal g, subnormal product; 2.4e-37: the product is
# just normal; 3e38: lr * g is finite, g + g would not be.
# An f64 subnormal second moment cannot be reached from an f32 gradient: the
# smallest nonzero lr * g is 2^-149, so v >= (1 - beta2) * 2^-298, far above
# 2^-1022; the zero case (sqrt(0 / c2), 0 / (0 + eps)) is what there is.
EDGE_GRADS = np.array([0.0] + [x * 1.401298464324817e-45 for x in (7, 9, 21, 30)] +
                      [1e-40, 1e-38, 1e-37, 2e-37, 2.4e-37, 1.0, 3e38], np.float32)
EDGE_GRADS = np.concatenate([EDGE_GRADS, -EDGE_GRADS])
# rows at +-FLT_MAX overflow on (float)((double)row - g); rows at the smallest
# normal land on subnormals; a subnormal row; 0 and 1
EDGE_ROWS = np.array([FLT_MAX, -FLT_MAX, MIN_NORMAL, -MIN_NORMAL, 3 * 1.401298464324817e-45, 0.0, 1.0], np.float32)


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("width", [4, 3])
def test_optimizer_edges(width, adam):
    """Every edge row against every edge gradient, W = 4 (16-B body) and W = 3
    (element body), three iterations; rows, replies and moments bit for bit."""
    assert np.all(np.isfinite(EDGE_GRADS)) and len(np.unique(bits(EDGE_GRADS))) == len(EDGE_GRADS)
    lrg = np.float32(LR) * EDGE_GRADS
    assert np.all(np.isfinite(lrg)) and np.any((lrg != 0) & (np.abs(lrg) < MIN_NORMAL))
    assert int(np.sum((lrg == 0) & (EDGE_GRADS != 0))) == 4  # the products that underflow
    w0 = np.repeat(EDGE_ROWS, len(EDGE_GRADS))
    g0 = np.tile(EDGE_GRADS, len(EDGE_ROWS))
    rows = -(-len(w0) // width)
    w, g = np.zeros(rows * width, np.float32), np.zeros(rows * width, np.float32)
    w[:len(w0)], g[:len(g0)] = w0, g0
    keys = random_keys(np.random.default_rng(width), rows)
    rig = OptRig(width, keys, adam)
    rig.seed(keys, w)
    for it, sign in ((0, 1), (1, -1), (999, 1)):
        rig.update(PP, keys, (sign * g).astype(np.float32), it)
    rig.check()
    if not adam:
        _, got = rig.t.dump()
        got = got.ravel()[:len(w0)].reshape(len(EDGE_ROWS), len(EDGE_GRADS))
        assert np.isinf(got[0]).any() and np.isinf(got[1]).any()  # the rows at +-FLT_MAX did overflow
        sub = (got != 0) & (np.abs(got) < MIN_NORMAL)
        assert sub[2].any() and sub[3].any()  # the rows at the smallest normal did land on subnormals
