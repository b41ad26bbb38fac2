"""psg_table_set_adagrad_half / psg_table_get_rounding: exported and bound, the
setter's refusal order (each case breaks one rule and every later one), what
stays refused, and the model's round16 over all 65536 words of a value.

CPU-only: the tables are the zeroed stand-ins of test_rows_pooled_abi.py."""
import ctypes as C
import math

import numpy as np
import pytest

import psg
from row_adagrad_half_model import FORMAT, nearest16, round16
from row_model import BF16, F16, to_acc
from test_rows_adagrad_abi import INF, NAN, refused
from test_rows_pooled_abi import INVALID, OK, PTR, UNSUPPORTED, stand_in_table


def get_rounding(table):
    mode, seed = C.c_int(-1), C.c_uint64(9)
    assert psg.lib().psg_table_get_rounding(table, C.byref(mode), C.byref(seed)) == OK
    return mode.value, seed.value


@pytest.mark.parametrize("dtype", (psg.F16, psg.BF16))
def test_setter_refusal_order_and_what_stays_refused(dtype):
    lib = psg.lib()
    fn, name = lib.psg_table_set_adagrad_half, b"psg_table_set_adagrad_half"
    assert {"psg_table_set_adagrad_half", "psg_table_get_rounding"} <= set(psg.EXPORTS)
    assert (psg.ROUND_NEAREST, psg.ROUND_STOCHASTIC) == (0, 1)
    keep, table = stand_in_table(dtype)
    refused(fn(None, NAN, -1.0, NAN, 7, 1), INVALID, name + b": null table")
    for other in (psg.F32, psg.F64):
        refused(fn(stand_in_table(other)[1], NAN, -1.0, NAN, 7, 1), UNSUPPORTED, b"neither F16 nor BF16")
    refused(fn(table, INF, -1.0, NAN, 7, 1), INVALID, b"learning_rate")
    refused(fn(table, 0.1, -1e-9, NAN, 7, 1), INVALID, b"epsilon")
    refused(fn(table, 0.1, 0.0, -0.5, 7, 1), INVALID, b"initial_accumulator")
    for rounding in (-1, 2, 7):
        refused(fn(table, 0.1, 0.0, 0.5, rounding, 1), INVALID, b"rounding")
    assert get_rounding(table) == (0, 0) and bytes(keep.raw)[4:] == bytes(508), "a refused call wrote"
    # the F32 setter still refuses the table, and so does an update while the state is missing
    refused(lib.psg_table_set_adagrad(table, 0.1, 0.0, 0.0), UNSUPPORTED, b"F32 tables")
    refused(lib.psg_table_update(table, psg.PUSH, PTR, PTR, None, 1, 0.1, 0, None), UNSUPPORTED, b"F32 tables")
    assert fn(table, 0.1, 0.0, 0.5, psg.ROUND_STOCHASTIC, (1 << 63) + 5) == OK
    assert get_rounding(table) == (1, (1 << 63) + 5)
    has, p = C.c_int(0), (C.c_double * 3)()
    assert lib.psg_table_get_adagrad(table, C.byref(has), p) == OK and (has.value, tuple(p)) == (1, (0.1, 0.0, 0.5))
    refused(fn(table, NAN, -1.0, NAN, 7, 1), INVALID, name + b": the table already has Adagrad state")
    assert lib.psg_table_update(table, psg.PUSH, PTR, PTR, None, 0, 0.1, 0, None) == OK  # accepted; no key, no device
    refused(lib.psg_table_get_rounding(table, None, None), INVALID, b"null argument")


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)


# f32 patterns: representable in both formats; normals; an F16 subnormal result; an f32 subnormal (a BF16
# subnormal input); the last binade below each format's overflow; zeros, infinities, a NaN
VALUES = (0x3FC00000, 0x3F8ABCDE, 0xC0490FDB, 0x3DCCCCCD, 0x33D6BF95, 0xB3000001, 0x00012345, 0x80400001,
          0x477FE001, 0x477FF000, 0xC77FFFFF, 0x7F7F8001, 0xFF7FFFFF, 0x00000000, 0x80000000, 0x7F800000,
          0xFF800000, 0x7FC00000)


@pytest.mark.parametrize("dtype", (F16, BF16))
@pytest.mark.parametrize("bits", VALUES, ids=[f"{b:08x}" for b in VALUES])
def test_round16_over_every_word(dtype, bits):
    """the result is one of v's two neighbours, away from zero for exactly k of the 65536 words"""
    v = f32(bits)
    got = round16(dtype, np.repeat(v, 65536), np.arange(65536))
    if not np.isfinite(v[0]) or (dtype == F16 and abs(v[0]) >= 65536):  # nothing to choose between
        assert (got == nearest16(dtype, v)[0]).all()
        return
    mbits, emin = FORMAT[dtype]
    a = abs(float(v[0]))
    q = 2.0 ** (max(math.frexp(a)[1] - 1, emin) - mbits)
    n, k = divmod(a / q, 1.0)
    k = int(k * 65536)  # floor: exact, k * 65536 has at most 24 bits
    with np.errstate(over="ignore"):
        down, up = (nearest16(dtype, np.float32(math.copysign(x * q, v[0])))[0] for x in (n, n + 1))
    assert to_acc(dtype, np.array([down]))[0] == np.float32(math.copysign(n * q, v[0])), "n * q is representable"
    assert (np.signbit(to_acc(dtype, got)) == np.signbit(v[0])).all()
    assert set(got) <= {down, up} and int((got != down).sum()) == k
    assert (got[:65536 - k] == down).all(), "up exactly for the k largest words"
    if k == 0:
        assert down == nearest16(dtype, v)[0]
