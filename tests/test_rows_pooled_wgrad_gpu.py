"""psg_table_pooled_weight_grad (k_rows_pool_wgrad) against the numpy model of its
definition, bit for bit; a NaN is compared as a NaN (which NaN is the machine's).
One list of 301 positions: empty bags first, in the middle and last, a bag of 150
(three chunks), bag boundaries inside chunks, repeats, absent ids, n odd."""
import numpy as np
import pytest

import psg
import row_init_model as im
import row_model as rm
import row_wgrad_model as wm

pytestmark = pytest.mark.gpu

KEND = 1 << 40
INVALID, RANGE = 1, 4
SEED, LO, HI = 77, -1.0, 1.0
DTYPES = {"f32": psg.F32, "f64": psg.F64, "f16": psg.F16, "bf16": psg.BF16}
GRID = [("f32", w) for w in (1, 3, 4, 8, 12, 260, 4095, 4096)] + \
       [(d, w) for d in ("f16", "bf16", "f64") for w in (3, 8, 264, 4096)]
PRESENT = np.arange(1000, 1048, dtype=np.uint64) * 7
ABSENT = np.arange(5, 13, dtype=np.uint64) * 1001
SIZES = [0, 0, 150, 3, 0, 40, 1, 4, 2, 0, 61, 5, 0, 35, 0]  # bag 7: absent ids only
dev = psg.DeviceBuffer.from_numpy


@pytest.fixture(scope="module")
def ids():
    psg.set_device(0)
    rng = np.random.default_rng(11)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
    q = rng.choice(np.concatenate([PRESENT, ABSENT[:4]]), int(offsets[-1]))
    q[int(offsets[7]):int(offsets[8])] = ABSENT[4:]
    assert len(q) == 301 and 10 < np.isin(q, ABSENT).sum() < 60
    return q, offsets


def stored(dtype, x):  # values as the table stores them (halves: bit patterns)
    return x.astype(np.float64) if dtype == psg.F64 else rm.from_acc(dtype, x.astype(np.float32))


def table_of(dtype, width, rows, init=False, opt=None):
    t = psg.Table(dtype, width, 0, KEND, 0)
    if init:
        t.set_init(SEED, LO, HI)
    if opt:
        getattr(t, opt)(0.01)
    t.assign(dev(PRESENT), dev(rows), len(PRESENT))
    return t


def run(t, q, offsets, grads, off=0):
    """the call -> dw; grads and dw start `off` bytes behind a 256-B boundary"""
    n, nb = len(q), len(offsets) - 1
    g = psg.DeviceBuffer(grads.nbytes + 16)
    g.upload(grads, offset=off)
    d = dev(np.full(n + 4, -7.0, np.float32))
    t.pooled_weight_grad(dev(q) if n else None, dev(offsets), g.ptr + off, d.ptr + off, n, nb)
    assert (d.download(np.float32, 3, offset=off + 4 * n) == -7.0).all(), "wrote behind dw"
    return d.download(np.float32, n, offset=off)


def expect(t, rows, q, offsets, grads, init=False):
    present = np.isin(q, PRESENT)
    x = np.zeros((len(q), t.width), rows.dtype)
    x[present] = rows.reshape(len(PRESENT), -1)[np.searchsorted(PRESENT, q[present])]
    if init:
        x[~present] = im.init_rows(q[~present], t.dtype, t.width, SEED, LO, HI)
    return wm.weight_grad(t.dtype, x, present | init, grads.reshape(-1, t.width), offsets)


def same(got, exp):
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], exp.view(np.uint32)[~nan])


@pytest.mark.parametrize("init", [False, True], ids=["zero", "init"])
@pytest.mark.parametrize("dtype,width", GRID, ids=[f"{d}-w{w}" for d, w in GRID])
def test_every_width_and_dtype_is_the_model(ids, dtype, width, init):
    q, offsets = ids
    rng = np.random.default_rng(width)
    rows = stored(DTYPES[dtype], rng.uniform(-4, 4, len(PRESENT) * width))
    grads = rng.uniform(-2, 2, (len(SIZES), width)).astype(np.float32)
    if not init:
        grads[7] = np.inf  # the bag of absent ids: +0.0f, no NaN
    t = table_of(DTYPES[dtype], width, rows, init)
    exp = expect(t, rows, q, offsets, grads, init)
    assert np.isfinite(exp).all() and (init or (exp[~np.isin(q, PRESENT)].view(np.uint32) == 0).all())
    same(run(t, q, offsets, grads), exp)  # 16-B units where the row allows them
    same(run(t, q, offsets, grads, off=4), exp)  # grads and dw 4 B off a 16-B boundary: element units, same bits


@pytest.mark.parametrize("width", [3, 4, 260])
def test_special_values(width):
    """row 0: -0.0 against positive gradients -> -0.0; row 1: a 0 under an infinite
    gradient -> NaN; row 2: a NaN with a payload -> NaN; row 3: cancels to +0.0"""
    rows = np.ones((len(PRESENT), width), np.float32)
    rows[0] = -0.0
    rows[1, 0] = 0.0
    rows[2, -1] = np.uint32(0x7FC12345).view(np.float32)
    rows[3, 1::2] = -1.0
    rows[3, 2 * (width // 2):] = 0.0
    grads = np.ones((4, width), np.float32)
    grads[1, 0] = np.inf
    q, offsets = PRESENT[:4].copy(), np.arange(5, dtype=np.uint64)
    t = table_of(psg.F32, width, rows)
    exp = expect(t, rows, q, offsets, grads)
    assert exp.view(np.uint32)[0] == 0x80000000 and np.isnan(exp[1]) and np.isnan(exp[2]) and exp.view(np.uint32)[3] == 0
    same(run(t, q, offsets, grads), exp)


def test_it_is_the_derivative_of_the_weighted_forward():
    """small integers, so every sum is exact: dw[p] = <grads[b], out(w + e_p)[b] - out(w)[b]>"""
    rng = np.random.default_rng(5)
    width, q, offsets = 8, PRESENT[[3, 9, 3, 20, 1, 9, 7]].copy(), np.array([0, 3, 3, 7], np.uint64)
    rows = rng.integers(-8, 9, (len(PRESENT), width)).astype(np.float32)
    grads = rng.integers(-8, 9, (3, width)).astype(np.float32)
    w = rng.integers(-4, 5, len(q)).astype(np.float32)
    t = table_of(psg.F32, width, rows)
    dw = run(t, q, offsets, grads)

    def forward(weights):
        out = psg.DeviceBuffer(3 * width * 4)
        t.lookup_pooled_weighted(dev(q), dev(offsets), dev(weights), psg.POOL_SUM, out, len(q), 3)
        return out.download(np.float32, 3 * width).reshape(3, width)

    base = forward(w)
    for p in range(len(q)):
        b = int(np.searchsorted(offsets, p, side="right")) - 1
        assert dw[p] == (grads[b] * (forward(w + np.eye(len(q), dtype=np.float32)[p])[b] - base[b])).sum()


def snapshot(t, opt):
    i = t.info()
    extra = {None: tuple, "set_adam": t.dump_moments, "set_adagrad": lambda: (t.dump_accum(),)}[opt]()
    return (int(i.size), int(i.capacity), i.rows, i.keys), [x.tobytes() for x in t.dump() + tuple(extra)]


@pytest.mark.parametrize("opt", [None, "set_adam", "set_adagrad"])
def test_the_table_is_unchanged_and_device_refusals_write_nothing(ids, opt):
    q, offsets = ids
    rng = np.random.default_rng(9)
    rows = rng.uniform(-4, 4, len(PRESENT) * 12).astype(np.float32)
    grads = rng.uniform(-2, 2, (len(SIZES), 12)).astype(np.float32)
    t = table_of(psg.F32, 12, rows, opt=opt)
    before = snapshot(t, opt)
    same(run(t, q, offsets, grads), expect(t, rows, q, offsets, grads))
    bad_q, bad_off = q.copy(), offsets.copy()
    bad_q[200] = KEND
    bad_off[3] = 200  # above its successor, 153
    for qq, oo, code in ((q, bad_off, INVALID), (bad_q, offsets, RANGE), (bad_q, bad_off, INVALID)):
        d = dev(np.full(len(q), -7.0, np.float32))
        with pytest.raises(psg.PsgError) as e:
            t.pooled_weight_grad(dev(qq), dev(oo), dev(grads), d, len(q), len(SIZES))
        assert e.value.code == code and (d.download(np.float32, len(q)) == -7.0).all()
    # edge counts: no ids in three bags writes nothing (run looks behind dw); no bags is a no-op
    run(t, q[:0], np.zeros(4, np.uint64), grads)
    t.pooled_weight_grad(None, None, None, None, 0, 0)
    assert snapshot(t, opt) == before
