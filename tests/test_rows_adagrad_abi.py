"""psg_table_set_adagrad, psg_table_get_adagrad, psg_table_dump_accum: exported and
bound, the order in which they refuse bad arguments (each case breaks one rule
and every later one), and the model's summation tree against the exact sum.

CPU-only: the table is the zeroed stand-in of test_rows_pooled_abi.py, whose
capacity is 0, so the served calls are host only, too."""
import ctypes as C
import math

import numpy as np
import pytest

import psg
from row_adagrad_model import pow2_above, tree_sum
from test_rows_pooled_abi import INVALID, OK, last_error, stand_in_table

UNSUPPORTED = 6
NAN, INF = math.nan, math.inf


def refused(rc, code, text):
    assert rc == code, (rc, last_error())
    assert text in last_error(), last_error()


def get_adagrad(table):
    has, p = C.c_int(-1), (C.c_double * 3)(9, 9, 9)
    assert psg.lib().psg_table_get_adagrad(table, C.byref(has), p) == OK
    return has.value, tuple(p)


def test_set_adagrad_refusal_order_and_its_neighbours():
    lib = psg.lib()
    fn, name = lib.psg_table_set_adagrad, b"psg_table_set_adagrad"
    assert {"psg_table_set_adagrad", "psg_table_get_adagrad", "psg_table_dump_accum"} <= set(psg.EXPORTS)
    keep, table = stand_in_table()
    refused(fn(None, NAN, -1.0, NAN), INVALID, name + b": null table")
    for dtype in (psg.F64, psg.F16, psg.BF16):
        refused(fn(stand_in_table(dtype)[1], NAN, -1.0, NAN), UNSUPPORTED, b"F32 tables")
    for lr in (NAN, INF, -INF):
        refused(fn(table, lr, -1.0, NAN), INVALID, b"learning_rate")
    for eps in (-1e-9, NAN, INF):
        refused(fn(table, 0.1, eps, NAN), INVALID, b"epsilon")
    for init in (-0.5, NAN, INF):
        refused(fn(table, 0.1, 0.0, init), INVALID, b"initial_accumulator")
    assert get_adagrad(table) == (0, (0.0, 0.0, 0.0)) and bytes(keep.raw)[4:] == bytes(508), "a refused call wrote"
    refused(lib.psg_table_dump_accum(table, None), INVALID, b"no Adagrad state")
    # served; then a second call and Adam are refused in front of the parameters' own rules
    assert fn(table, -0.5, 0.0, 0.125) == OK and get_adagrad(table) == (1, (-0.5, 0.0, 0.125))
    refused(fn(table, NAN, -1.0, NAN), INVALID, name + b": the table already has Adagrad state")
    refused(lib.psg_table_set_adam(table, 0.1, 0.9, 0.999, 1e-8), INVALID, b"Adagrad state")
    assert lib.psg_table_dump_accum(table, None) == OK, "an empty table has nothing to copy"
    # an Adam table takes no Adagrad state
    _, adam = stand_in_table()
    assert lib.psg_table_set_adam(adam, 0.1, 0.9, 0.999, 1e-8) == OK
    refused(fn(adam, NAN, -1.0, NAN), INVALID, name + b": the table already has Adam state")
    has = C.c_int(0)
    refused(lib.psg_table_get_adagrad(None, C.byref(has), None), INVALID, b"null argument")
    refused(lib.psg_table_get_adagrad(table, None, None), INVALID, b"null argument")


@pytest.mark.parametrize("width", (1, 3, 100, 4096))
def test_the_tree_is_within_its_bound_of_the_exact_sum(width):
    """only the adds round (g * g is exact in f64): log2(P) roundings on any path to the root"""
    rng = np.random.default_rng(width)
    scale = np.array([1, 1e-20, 1e15, 1] * 2)[:, None]
    g = rng.uniform(-1, 1, (8, width)).astype(np.float32).astype(np.float64) * scale
    p = pow2_above(width)
    y = np.zeros((8, p))
    y[:, :width] = g * g
    exact = [math.fsum(row) for row in y]
    got = tree_sum(y.copy())
    # (1 + 2^-53)^log2(P) - 1, which f64 cannot form as written: 1 + 2^-53 rounds to 1
    bound = math.expm1(int(math.log2(p)) * math.log1p(2.0 ** -53))
    for a, b in zip(got, exact):
        assert abs(a - b) <= bound * b
