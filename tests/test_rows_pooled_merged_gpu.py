"""The sync-mode round over pooled and plain frames
(psg_table_update_pooled_merged, csrc/psg_rows.hip).

The definition is the twin test: table A takes the new call, table B takes
psg_table_update_merged on the host-expanded gradient rows E_j (a plain frame's
own rows; for a pooled frame the row of bag(i) at row i), and keys, rows and
Adam moments must then be equal.  Every case runs two consecutive rounds, at
iteration 0 and 3, so the moments carry over.  Every comparison is bit for bit,
through unsigned views, except in the one case with NaN gradients, where only
NaN-ness is asserted at the positions B holds a NaN.
"""
import numpy as np
import pytest

import psg
from test_rows_pooled_gpu import (ADAM, INVALID, KEND, LR, RANGE, absent_keys, assert_twins, assert_unchanged, bits, dev,
                                  expanded, offsets_of, flat, random_keys, refused, same, snapshot, value_table)

pytestmark = pytest.mark.gpu

ITERATIONS = (0, 3)


@pytest.fixture(scope="module", autouse=True)
def device():
    assert psg.device_count() >= 1, "no GPU visible"
    psg.set_device(0)
    yield


# ---- frames on the host ---------------------------------------------------------------------------
class Frame:
    """keys q, offsets (None: a plain frame), grads [rows, W]; E is what
    psg_table_update_merged takes in its place"""

    def __init__(self, q, offsets, grads, width):
        self.q = np.ascontiguousarray(q, dtype=np.uint64)
        self.offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        self.grads = np.ascontiguousarray(grads, dtype=np.float32).reshape(-1, width)
        self.n = len(self.q)
        self.nb = 0 if offsets is None else len(offsets) - 1
        assert len(self.grads) == (self.n if offsets is None else self.nb)
        self.E = self.grads.ravel() if offsets is None else expanded(self.grads.ravel(), self.offsets, width)
        assert len(self.E) == self.n * width


def bags_of(rng, ids):
    """cut ids into bags of 0-12, the first and the last bag empty"""
    sizes, n = [0], len(ids)
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(0, 13)), n - sum(sizes)))
    sizes.append(0)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def make_frame(rng, kind, ids, width):
    if kind == "plain":
        return Frame(ids, None, rng.uniform(-1, 1, (len(ids), width)), width)
    if kind == "empty-plain":
        return Frame([], None, np.zeros((0, width)), width)
    if kind == "pooled-no-keys":  # ns = 0, nb = 5: legal, and no gradient row is read
        return Frame([], np.zeros(6, dtype=np.uint64), np.full((5, width), np.nan), width)
    if kind == "pooled-no-bags":  # nb = 0
        return Frame([], np.zeros(1, dtype=np.uint64), np.zeros((0, width)), width)
    assert kind == "pooled"
    offsets = bags_of(rng, ids)
    grads = rng.uniform(-1, 1, (len(offsets) - 1, width)).astype(np.float32)
    grads[np.diff(offsets.astype(np.int64)) == 0] = np.nan  # an empty bag's row is never read
    return Frame(ids, offsets, grads, width)


def make_round(rng, kinds, known, total, width, hot=None):
    """`total` occurrences over the frames that carry keys: about a sixth of the
    distinct ids absent from the table, `hot` named more than 300 times across
    the frames.  Returns the frames and the new ids."""
    new = absent_keys(rng, known, max(1, len(known) // 5))
    pool = np.concatenate([known, new])
    carriers = [j for j, kd in enumerate(kinds) if kd in ("plain", "pooled")]
    share = rng.multinomial(total, np.ones(len(carriers)) / len(carriers))
    frames = []
    for j, kd in enumerate(kinds):
        ids = np.zeros(0, dtype=np.uint64)
        if j in carriers:
            ids = rng.choice(pool, share[carriers.index(j)], replace=True)
            if hot is not None and len(ids):
                at = rng.choice(len(ids), min(len(ids), 330 // len(carriers) + 1), replace=False)
                ids[at] = hot
        frames.append(make_frame(rng, kd, ids, width))
    assert sum(f.n for f in frames) == total
    return frames, new


class Uploaded:
    """the frames in HBM; grads_off: the gradient arrays start that many bytes off 16"""

    def __init__(self, frames, grads_off=0):
        self.keep = []
        self.frames, self.ns, self.nbs = [], [f.n for f in frames], [f.nb for f in frames]
        for f in frames:
            k = dev(f.q) if f.n else None
            o = dev(f.offsets) if f.offsets is not None else None
            g = None
            if f.grads.size:
                buf = psg.DeviceBuffer(f.grads.nbytes + 16)
                buf.upload(f.grads, offset=grads_off)
                self.keep.append(buf)
                g = buf.ptr + grads_off
            self.keep += [k, o]
            self.frames.append((k, o, g))


def push_a(a, frames, it, grads_off=0):
    up = Uploaded(frames, grads_off)
    return a.update_pooled_merged(up.frames, up.ns, up.nbs, LR, it)


def push_b(b, frames, it):
    keys = [dev(f.q) if f.n else None for f in frames]
    grads = [dev(f.E) if f.n else None for f in frames]
    return b.update_merged(psg.PUSH, keys, grads, None, [f.n for f in frames], LR, it)


def twins(width, known, adam, seed=1):
    return (value_table(psg.F32, width, known, np.random.default_rng(seed), adam),
            value_table(psg.F32, width, known, np.random.default_rng(seed), adam))


def assert_no_nan(t, adam):
    assert not np.isnan(t.dump()[1]).any()
    if adam:
        assert not any(np.isnan(x).any() for x in t.dump_moments())


def run_rounds(width, adam, kinds, total, nkeys, hot, seed, grads_off=0):
    rng = np.random.default_rng(seed)
    known = random_keys(rng, nkeys)
    a, b = twins(width, known, adam)
    for it in ITERATIONS:
        frames, new = make_round(rng, kinds, known, total, width, known[0] if hot else None)
        named = np.unique(np.concatenate([f.q for f in frames]))
        if hot:
            assert sum(int((f.q == known[0]).sum()) for f in frames) > 300
        path = push_a(a, frames, it, grads_off)
        push_b(b, frames, it)
        if len(kinds) > 1 and any(f.offsets is not None for f in frames):
            assert path == psg.MERGED_SORTED
        known = np.union1d(known, named)
        assert int(a.info().size) == len(known), "absent ids are inserted once"
        assert_twins(a, b, adam)
    assert_no_nan(b, adam)
    a.close()
    b.close()


K16 = ["pooled", "plain", "empty-plain", "pooled-no-keys", "pooled", "pooled-no-bags", "plain", "pooled",
       "pooled", "plain", "pooled", "empty-plain", "pooled", "plain", "pooled", "pooled"]
# (width, frame kinds, occurrences, table keys, hot id)
CASES = {
    "w4-k3-mixed-5000": (4, ["pooled", "plain", "pooled"], 5000, 1500, True),
    "w20-k2-pooled-5000": (20, ["pooled", "pooled"], 5003, 1500, True),
    "w3-k16-every-kind-5000": (3, K16, 4999, 1500, True),
    "w1-k3-empty-plain-257": (1, ["pooled", "empty-plain", "pooled"], 257, 120, False),
    "w4-k2-no-keys-255": (4, ["pooled-no-keys", "pooled"], 255, 120, False),
    "w20-k3-no-bags-1": (20, ["pooled-no-bags", "pooled", "empty-plain"], 1, 30, False),
    "w1-k2-mixed-5000": (1, ["plain", "pooled"], 5000, 1500, True),
    "w3-k2-pooled-255": (3, ["pooled", "pooled"], 255, 120, False),
    "w20-k16-every-kind-257": (20, K16, 257, 120, False),
    "w4-k16-every-kind-1": (4, K16, 1, 30, False),
    "w4096-k2-mixed-3": (4096, ["pooled", "plain"], 3, 8, False),
}


@pytest.mark.parametrize("opt", ("sgd", "adam"))
@pytest.mark.parametrize("case", list(CASES))
def test_twin(case, opt):
    width, kinds, total, nkeys, hot = CASES[case]
    assert len(K16) == 16
    run_rounds(width, opt == "adam", kinds, total, nkeys, hot, seed=sum(map(ord, case)))


def test_about_a_sixth_of_the_ids_is_absent():
    """what make_round promises (host only, but it pins the other tests' inputs)"""
    rng = np.random.default_rng(5)
    known = random_keys(rng, 1500)
    frames, new = make_round(rng, ["pooled", "plain", "pooled"], known, 5000, 4, known[0])
    named = np.unique(np.concatenate([f.q for f in frames]))
    share = 1 - np.isin(named, known).mean()
    assert 0.1 < share < 0.25, share
    for f in frames:
        if f.offsets is not None:
            sizes = np.diff(f.offsets.astype(np.int64))
            assert sizes[0] == 0 and sizes[-1] == 0 and sizes.max() <= 12


@pytest.mark.parametrize("opt", ("sgd", "adam"))
def test_a_gradient_array_4_bytes_off_takes_the_scalar_form(opt):
    """W = 4 rows would go as 16-B units; a gradient array that is not on 16 B cannot"""
    run_rounds(4, opt == "adam", ["pooled", "plain", "pooled"], 5000, 1500, True, seed=77, grads_off=4)


@pytest.mark.parametrize("opt", ("sgd", "adam"))
def test_all_frames_plain_is_update_merged(opt):
    adam = opt == "adam"
    rng = np.random.default_rng(21)
    width = 4
    known = random_keys(rng, 600)
    a, b = twins(width, known, adam)
    for it in ITERATIONS:
        # one ascending list in every frame, then shuffled lists with repeats
        lst = np.sort(np.concatenate([rng.choice(known, 200, replace=False), absent_keys(rng, known, 40)]))
        same_list = [Frame(lst, None, rng.uniform(-1, 1, (len(lst), width)), width) for _ in range(3)]
        shuffled, _ = make_round(rng, ["plain", "empty-plain", "plain"], known, 700, width)
        for frames, want in ((same_list, psg.MERGED_SAME_LIST), (shuffled, psg.MERGED_SORTED)):
            pa, pb = push_a(a, frames, it), push_b(b, frames, it)
            assert pa == pb == want
            assert_twins(a, b, adam)
    assert_no_nan(b, adam)
    a.close()
    b.close()


@pytest.mark.parametrize("opt", ("sgd", "adam"))
@pytest.mark.parametrize("width", (4, 3))
def test_one_pooled_frame_is_update_pooled(width, opt):
    adam = opt == "adam"
    rng = np.random.default_rng(22 + width)
    known = random_keys(rng, 600)
    a, b = twins(width, known, adam)
    c = value_table(psg.F32, width, known, np.random.default_rng(1), adam)
    for it in ITERATIONS:
        asc = np.sort(np.concatenate([rng.choice(known, 300, replace=False), absent_keys(rng, known, 50)]))
        shuffled = rng.choice(np.concatenate([known, absent_keys(rng, known, 100)]), 700, replace=True)
        for ids, want in ((asc, psg.MERGED_SAME_LIST), (shuffled, psg.MERGED_SORTED)):
            f = make_frame(rng, "pooled", ids, width)
            assert push_a(a, [f], it) == want
            push_b(b, [f], it)
            c.update_pooled(dev(f.q), dev(f.offsets), dev(f.grads), f.n, f.nb, LR, it)
            assert_twins(a, b, adam)
            assert_twins(a, c, adam)
    assert_no_nan(b, adam)
    for t in (a, b, c):
        t.close()


def test_minus_zero_gradients_sum_from_plus_zero():
    """a row of -0.0 that receives only -0.0 gradients stays -0.0 under SGD:
    s = +0 + -0 + -0 = +0, and -0 - (+0) is -0; a sum that started from its
    first term would be -0, and -0 - (-0) is +0"""
    width = 4
    keys = np.array([10, 20, 30], dtype=np.uint64)
    rows = np.full(3 * width, 0x80000000, dtype=np.uint32)
    a, b = psg.Table(psg.F32, width, 0, KEND, 0), psg.Table(psg.F32, width, 0, KEND, 0)
    for t in (a, b):
        t.assign(dev(keys), dev(rows), 3)
    mz = np.float32(-0.0)
    frames = [Frame([20, 10, 20], [0, 0, 2, 3, 3], np.full((4, width), mz), width),
              Frame([10, 30], None, np.full((2, width), mz), width),
              Frame([30, 20], [0, 2], np.full((1, width), mz), width)]
    for it in ITERATIONS:
        assert push_a(a, frames, it) == psg.MERGED_SORTED
        push_b(b, frames, it)
        assert_twins(a, b, False)
        assert (bits(a.dump()[1]) == 0x80000000).all()
    a.close()
    b.close()


@pytest.mark.parametrize("opt", ("sgd", "adam"))
def test_inf_and_nan_gradients(opt):
    """the one case with NaN in its expected arrays: NaN-ness there, bits elsewhere"""
    adam = opt == "adam"
    rng = np.random.default_rng(23)
    width = 4
    known = random_keys(rng, 300)
    a, b = twins(width, known, adam)
    for it in ITERATIONS:
        frames, _ = make_round(rng, ["pooled", "plain", "pooled"], known, 900, width)
        for f in frames:
            g = f.grads
            live = np.flatnonzero(~np.isnan(g[:, 0]))
            pick = rng.choice(live, 12, replace=False)
            g[pick[:4], 0], g[pick[4:8], 1], g[pick[8:], 2] = np.inf, -np.inf, np.nan
        frames = [Frame(f.q, f.offsets, f.grads, width) for f in frames]  # E again, from the new rows
        push_a(a, frames, it)
        push_b(b, frames, it)
        (ka, ra), (kb, rb) = a.dump(), b.dump()
        np.testing.assert_array_equal(ka, kb)
        pairs = [(ra, rb)] + (list(zip(a.dump_moments(), b.dump_moments())) if adam else [])
        for got, exp in pairs:
            nan = np.isnan(exp)
            assert np.isnan(got[nan]).all()
            np.testing.assert_array_equal(bits(got)[~nan], bits(exp)[~nan])
    assert np.isnan(rb).any() and not np.isnan(rb).all()
    a.close()
    b.close()


def test_refusals_found_on_the_device_change_nothing():
    rng = np.random.default_rng(24)
    width = 4
    known = random_keys(rng, 300)
    for adam in (True, False):
        t = value_table(psg.F32, width, known, rng, adam)
        if adam:
            t.update(psg.PUSH, dev(known), dev(rng.uniform(-1, 1, len(known) * width).astype(np.float32)), None,
                     len(known), LR, 0)
        snap = snapshot(t, adam)
        good, _ = make_round(rng, ["pooled", "pooled", "plain"], known, 600, width)

        def with_bad_offsets(frames):
            f = frames[1]
            o = f.offsets.copy()
            o[3], o[4] = o[4] + 1, o[3]  # a decreasing pair
            bad = Frame.__new__(Frame)
            bad.__dict__.update(f.__dict__)
            bad.offsets = o
            return [frames[0], bad, frames[2]]

        def with_key_out_of_range(frames):
            f = frames[2]
            q = f.q.copy()
            q[-1] = KEND
            return [frames[0], frames[1], Frame(q, None, f.grads, width)]

        for frames, code in ((with_bad_offsets(good), INVALID), (with_key_out_of_range(good), RANGE),
                             (with_key_out_of_range(with_bad_offsets(good)), INVALID)):
            msg = refused(lambda: push_a(t, frames, 1), code)
            assert "psg_table_update_pooled_merged" in msg or code == RANGE, msg
            assert_unchanged(t, snap, adam)
        # rounds of no key: valid offsets are a no-op, bad ones are refused
        empty = [make_frame(rng, "pooled-no-keys", None, width), make_frame(rng, "empty-plain", None, width)]
        assert push_a(t, empty, 1) == 0
        assert_unchanged(t, snap, adam)
        empty[0].offsets[2] = 1
        refused(lambda: push_a(t, empty, 1), INVALID)
        assert_unchanged(t, snap, adam)
        t.close()
