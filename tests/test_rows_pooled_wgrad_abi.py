"""psg_table_pooled_weight_grad in the C-ABI: exported, bound, bad arguments refused
before any device call in the header's order (CPU-only: the addresses are not mapped
and the table is zeroed host memory), and the numpy model pinned on three cases."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import psg
import row_wgrad_model as wm

NAME = "psg_table_pooled_weight_grad"
OK, INVALID, RANGE = 0, 1, 4
PTR, ODD = C.c_void_p(0x1000), C.c_void_p(0x1002)
TOO_MANY = (1 << 32) - 1


def call(table, keys, offsets, grads, dw, n, nb):
    return getattr(psg.lib(), NAME)(table, keys, offsets, grads, dw, n, nb, None)


@pytest.fixture
def table():
    buf = C.create_string_buffer(512)
    C.cast(buf, C.POINTER(C.c_int))[0] = psg.F16
    yield C.cast(buf, C.c_void_p)
    assert bytes(buf.raw)[4:] == bytes(508), "the table was written"


def test_declared_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % NAME, nm, re.M)
    assert NAME in psg.EXPORTS and len(getattr(psg.lib(), NAME).argtypes) == 8
    assert callable(psg.Table.pooled_weight_grad)


# each call breaks the rule under test AND every later one: the message names the first
@pytest.mark.parametrize("args,code,msg", [
    ((None, None, None, ODD, None, TOO_MANY, 2), INVALID, "null table"),
    (("t", None, None, ODD, None, TOO_MANY, 2), INVALID, "null keys"),
    (("t", PTR, None, ODD, None, TOO_MANY, 2), INVALID, "null offsets"),
    (("t", PTR, PTR, None, None, TOO_MANY, 2), INVALID, "null grads"),
    (("t", PTR, None, ODD, None, TOO_MANY, 0), INVALID, "4294967295 keys and no bag"),
    (("t", PTR, PTR, ODD, None, TOO_MANY, 2), INVALID, "null dw"),
    (("t", PTR, PTR, ODD, ODD, TOO_MANY, 2), INVALID, "grads not on a 4-B boundary"),
    (("t", PTR, PTR, PTR, ODD, TOO_MANY, 2), INVALID, "dw not on a 4-B boundary"),
    (("t", PTR, PTR, PTR, PTR, TOO_MANY, TOO_MANY), RANGE, "more than 2^32-2 keys"),
    (("t", PTR, PTR, PTR, PTR, 5, TOO_MANY), RANGE, "more than 2^32-2 bags"),
    (("t", PTR, PTR, PTR, PTR, 0, 0), OK, None),  # no bags: a no-op
    (("t", None, None, None, None, 0, 0), OK, None),
    (("t", None, None, ODD, None, 0, 0), INVALID, "grads not on a 4-B boundary"),  # which hides no refusal
])
def test_refusals_come_in_the_stated_order(table, args, code, msg):
    assert call(table if args[0] == "t" else None, *args[1:]) == code
    if msg:
        assert ("%s: %s" % (NAME, msg)).encode() in psg.lib().psg_last_error()


@pytest.mark.parametrize("dtype,row,grad,bits", [
    (psg.F32, [-0.0, -0.0, -0.0], [1, 2, 3], 0x80000000),  # every term and the padding -0.0: -0.0
    (psg.F32, [1, 2, 3], [4, 5, 6], 0x42000000),  # (4 + 18) + (10 + -0.0) = 32
    # (2^53 + 1) rounds to 2^53 before -2^53 arrives: +0.0, where left to right gives 1
    (psg.F64, [2.0 ** 53, -2.0 ** 53, 1, 0], [1, 1, 1, 1], 0x00000000),
])
def test_model_is_the_stated_tree(dtype, row, grad, bits):
    rows = np.array([row], np.float64 if dtype == psg.F64 else np.float32)
    dw = wm.weight_grad(dtype, rows, np.array([True]), np.array([grad], np.float32), np.array([0, 1], np.uint64))
    assert dw.dtype == np.float32 and dw.view(np.uint32)[0] == bits
