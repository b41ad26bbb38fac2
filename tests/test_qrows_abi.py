"""The frozen 8-bit snapshot in the C-ABI: the seven symbols exported, listed and
bound; bad arguments refused before any device call in the header's order (CPU-only:
the addresses are not mapped, table and snapshot are zeroed host memory); and the
numpy model pinned by three hand-worked rows and the error bound of its definition."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import psg
import row_q8_model as qm

NAMES = {"psg_table_freeze_q8": 3, "psg_qtable_create": 8, "psg_qtable_destroy": 1, "psg_qtable_get_info": 2,
         "psg_qtable_export": 6, "psg_qtable_lookup": 6, "psg_qtable_lookup_pooled": 9}
OK, INVALID, RANGE, UNSUPPORTED = 0, 1, 4, 6
PTR, ODD = C.c_void_p(0x1000), C.c_void_p(0x1002)
TOO_MANY = (1 << 32) - 1


@pytest.fixture
def obj():
    """zeroed host memory in a table's or a snapshot's place; as a table its dtype is F64"""
    buf = C.create_string_buffer(512)
    C.cast(buf, C.POINTER(C.c_int))[0] = psg.F64
    yield C.cast(buf, C.c_void_p)
    assert bytes(buf.raw)[4:] == bytes(508), "the object was written"


def test_declared_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in NAMES.items():
        assert re.search(r"\bT %s$" % name, nm, re.M), name
        assert name in psg.EXPORTS and len(getattr(psg.lib(), name).argtypes) == nargs
    assert all(callable(getattr(psg.QTable, m)) for m in ("from_rows", "info", "export", "lookup", "lookup_pooled", "close"))
    assert callable(psg.Table.freeze_q8)


# each call breaks the rule under test AND every later one: the message names the first
@pytest.mark.parametrize("args,code,msg", [
    ((None, None, None, None, 7, ODD, TOO_MANY, 2), INVALID, "null snapshot"),
    (("q", None, None, ODD, 7, ODD, TOO_MANY, 2), INVALID, "null keys"),
    (("q", PTR, None, ODD, 7, ODD, TOO_MANY, 2), INVALID, "null offsets"),
    (("q", PTR, PTR, ODD, 7, None, TOO_MANY, 2), INVALID, "null out"),
    (("q", PTR, None, ODD, 7, None, TOO_MANY, 0), INVALID, "4294967295 keys and no bag"),
    (("q", PTR, PTR, ODD, 7, ODD, TOO_MANY, 2), INVALID, "mode 7 is no pooling mode"),
    (("q", PTR, PTR, ODD, psg.POOL_MEAN, ODD, TOO_MANY, 2), INVALID, "weights with PSG_POOL_MEAN"),
    (("q", PTR, PTR, ODD, psg.POOL_SUM, ODD, TOO_MANY, 2), INVALID, "weights not on a 4-B boundary"),
    (("q", PTR, PTR, PTR, psg.POOL_SUM, ODD, TOO_MANY, 2), INVALID, "out not on a 4-B boundary"),
    (("q", PTR, PTR, PTR, psg.POOL_SUM, PTR, TOO_MANY, TOO_MANY), RANGE, "more than 2^32-2 keys"),
    (("q", PTR, PTR, None, psg.POOL_MEAN, PTR, 5, TOO_MANY), RANGE, "more than 2^32-2 bags"),
    (("q", None, None, None, psg.POOL_SUM, None, 0, 0), OK, None),  # no bags: a no-op
])
def test_pooled_refusals_come_in_the_stated_order(obj, args, code, msg):
    assert psg.lib().psg_qtable_lookup_pooled(obj if args[0] == "q" else None, *args[1:], None) == code
    if msg:
        assert ("psg_qtable_lookup_pooled: %s" % msg).encode() in psg.lib().psg_last_error()


@pytest.mark.parametrize("table,out,code,msg", [
    (False, False, INVALID, "null table"),
    (True, False, INVALID, "null out"),
    (True, True, UNSUPPORTED, "the freeze is built for F32, F16 and BF16 tables"),  # an F64 source
])
def test_freeze_refusals_come_in_the_stated_order(obj, table, out, code, msg):
    h = C.c_void_p(0x55)
    assert psg.lib().psg_table_freeze_q8(obj if table else None, C.byref(h) if out else None, None) == code
    assert ("psg_table_freeze_q8: %s" % msg).encode() in psg.lib().psg_last_error()
    assert h.value == 0x55, "*out was written"


@pytest.mark.parametrize("row,codes,scale,bias_bits,xhat", [
    ([0, 255], [0, 255], 1.0, 0, [0, 255]),
    ([5, 5, 5], [0, 0, 0], 0.0, 0x40A00000, [5, 5, 5]),  # a constant row: scale 0, the bias carries it
    ([-0.0, -0.0], [0, 0], 0.0, 0x00000000, [0, 0]),  # a -0.0 minimum is stored as +0.0
])
def test_model_rows_worked_by_hand(row, codes, scale, bias_bits, xhat):
    c, s, b = qm.quantise(np.array([row], np.float32))
    assert c.tolist() == [codes] and s.view(np.uint32)[0] == np.float32(scale).view(np.uint32)
    assert b.view(np.uint32)[0] == bias_bits
    assert qm.dequantise(c, s, b).view(np.uint32).tolist() == [np.array(xhat, np.float32).view(np.uint32).tolist()]
    p = qm.packed(c, s, b)
    assert p.shape == (1, len(row) + 8) and bytes(p[0, len(row):]) == s.tobytes() + b.tobytes()
    assert all(np.array_equal(u, v) for u, v in zip(qm.unpacked(p, len(row)), (c, s, b)))


def test_read_back_error_is_half_a_step_and_four_ulp():
    """|xhat - x| <= scale / 2 + 4 ulp(max(|lo|, |hi|)): half a step of the grid, and the
    roundings of x - lo, the quotient, code * scale and + bias, each at most one ulp of
    a value no larger than the row's largest magnitude (ulp taken in f64 at f32's spacing)"""
    rng = np.random.default_rng(3)
    mag = 10.0 ** rng.uniform(-30, 30, (6000, 1))
    x = (rng.uniform(-1, 1, (6000, 10)) * mag + rng.uniform(-1, 1, (6000, 1)) * mag).astype(np.float32)
    c, s, b = qm.quantise(x)
    err = np.abs(qm.dequantise(c, s, b).astype(np.float64) - x.astype(np.float64))
    big = np.maximum(np.abs(x.min(1)), np.abs(x.max(1)))
    ulp = np.spacing(big).astype(np.float64)
    assert (err <= (s.astype(np.float64) / 2 + 4 * ulp)[:, None]).all()
