"""psg_table_set_init, psg_table_get_init and psg_init_rows: declared, exported,
bound, and the order in which they refuse bad arguments — each case breaks one
rule and every later one, and the code and the message are those of the first.

CPU-only: nothing here launches a kernel or touches a GPU.  The table is zeroed
host memory (the stand-in of test_rows_pooled_abi.py) and the addresses given
for device arrays are not mapped: a call that got as far as a device call would
not return the code it is asked for.  The two table calls are host-only by
contract, so on the stand-in they are served, too.
"""
import ctypes as C
import math
import os
import re
import subprocess

import psg
from test_rows_pooled_abi import INVALID, OK, PTR, RANGE, TOO_MANY, last_error, stand_in_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["psg_table_set_init", "psg_table_get_init", "psg_init_rows"]
P = PTR.value
NAN, INF = math.nan, math.inf


def refused(rc, code, text):
    assert rc == code, (rc, last_error())
    assert text in last_error(), last_error()


def test_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "psg.h")).read()
    for s in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % s, text, re.M), s
        assert s in psg.EXPORTS
    assert re.search(r"^#define PSG_INIT_ZERO 0$", text, re.M) and re.search(r"^#define PSG_INIT_UNIFORM 1$", text, re.M)
    assert re.search(r"^#define PSG_ABI_VERSION 1$", text, re.M), "the change is additive"
    assert (psg.INIT_ZERO, psg.INIT_UNIFORM) == (0, 1)
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r"\bT (psg_\w+)", out))


def get_init(table):
    kind, seed, lo, hi = C.c_int(-1), C.c_uint64(99), C.c_float(9), C.c_float(9)
    assert psg.lib().psg_table_get_init(table, C.byref(kind), C.byref(seed), C.byref(lo), C.byref(hi)) == OK
    return kind.value, seed.value, lo.value, hi.value


def test_set_init_refusal_order_and_get_init():
    set_init = psg.lib().psg_table_set_init
    name = b"psg_table_set_init"
    keep, table = stand_in_table()
    # a table never given an initializer
    assert get_init(table) == (psg.INIT_ZERO, 0, 0.0, 0.0)
    # 1. a null table
    refused(set_init(None, 7, 1, NAN, -INF), INVALID, name + b": null table")
    # 2. an unknown kind
    for kind in (7, -1, 2):
        refused(set_init(table, kind, 1, NAN, -INF), INVALID, name + (b": kind %d is no initializer" % kind))
    # 4. lo or hi not finite (3. needs a served call: below)
    for lo, hi in ((NAN, -INF), (0.0, NAN), (INF, 0.0), (1.0, -INF), (0.0, INF)):
        refused(set_init(table, psg.INIT_UNIFORM, 1, lo, hi), INVALID, b"is not finite")
        assert b"hi - lo" not in last_error()
    # 5. lo above hi, with a difference that is not finite either
    refused(set_init(table, psg.INIT_UNIFORM, 1, 3e38, -3e38), INVALID, b"above hi")
    refused(set_init(table, psg.INIT_UNIFORM, 1, 1.0, 0.5), INVALID, b"above hi")
    # 6. hi - lo overflows f32
    refused(set_init(table, psg.INIT_UNIFORM, 1, -3e38, 3e38), INVALID, b"hi - lo is not finite in f32")
    # a refused call sets nothing
    assert get_init(table) == (psg.INIT_ZERO, 0, 0.0, 0.0)
    assert bytes(keep.raw) == bytes(512), "the table was written by a refused call"
    # served: lo == hi is allowed; all 64 bits of the seed are kept
    seed = 0xFEDC_BA98_7654_3210
    assert set_init(table, psg.INIT_UNIFORM, seed, 0.25, 0.25) == OK
    assert get_init(table) == (psg.INIT_UNIFORM, seed, 0.25, 0.25)
    # 3. a second call, in front of the rules about lo and hi; the first setting stays
    refused(set_init(table, psg.INIT_UNIFORM, 5, NAN, -INF), INVALID, name + b": the table already has an initializer")
    refused(set_init(table, psg.INIT_ZERO, 5, 0.0, 1.0), INVALID, name + b": the table already has an initializer")
    refused(set_init(table, 9, 5, 0.0, 1.0), INVALID, b"is no initializer")  # 2. in front of 3.
    assert get_init(table) == (psg.INIT_UNIFORM, seed, 0.25, 0.25)
    # PSG_INIT_ZERO said aloud is a call like any other: it is the one call
    keep2, table2 = stand_in_table()
    assert set_init(table2, psg.INIT_ZERO, 3, -1.0, 1.0) == OK
    assert get_init(table2) == (psg.INIT_ZERO, 3, -1.0, 1.0)
    refused(set_init(table2, psg.INIT_UNIFORM, 3, -1.0, 1.0), INVALID, b"already has an initializer")


def test_get_init_arguments():
    fn = psg.lib().psg_table_get_init
    keep, table = stand_in_table()
    kind = C.c_int(-1)
    refused(fn(None, C.byref(kind), None, None, None), INVALID, b"psg_table_get_init: null argument")
    refused(fn(table, None, None, None, None), INVALID, b"psg_table_get_init: null argument")
    assert fn(table, C.byref(kind), None, None, None) == OK and kind.value == psg.INIT_ZERO


def test_init_rows_refusal_order():
    fn = psg.lib().psg_init_rows
    name = b"psg_init_rows"

    def call(out, keys, n, dtype, width, lo=0.0, hi=1.0):
        return fn(out, keys, n, dtype, width, 1, lo, hi, None)

    # 1. a bad dtype
    for dtype in (4, -1, 99):
        refused(call(None, None, TOO_MANY, dtype, 0, NAN, -INF), INVALID, name + (b": bad dtype %d" % dtype))
    # 2. the width
    for width in (0, 4097):
        refused(call(None, None, TOO_MANY, psg.F32, width, NAN, -INF), INVALID,
                name + (b": width %d outside [1, 4096]" % width))
    # 3. null out, 4. null keys
    refused(call(None, None, TOO_MANY, psg.F32, 4, NAN, -INF), INVALID, name + b": null out")
    refused(call(P, None, TOO_MANY, psg.F16, 4096, NAN, -INF), INVALID, name + b": null keys")
    # 5. out between two elements
    refused(call(P + 2, P, TOO_MANY, psg.F32, 4, NAN, -INF), INVALID, name + b": out not on an element boundary")
    refused(call(P + 4, P, TOO_MANY, psg.F64, 4, NAN, -INF), INVALID, name + b": out not on an element boundary")
    # 6. lo and hi, as psg_table_set_init refuses them
    refused(call(P, P, TOO_MANY, psg.F32, 4, NAN, -INF), INVALID, name + b": lo nan or hi -inf is not finite")
    refused(call(P, P, TOO_MANY, psg.F32, 4, 2.0, 1.0), INVALID, name + b": lo 2 above hi 1")
    refused(call(P + 2, P, TOO_MANY, psg.BF16, 1, -3e38, 3e38), INVALID, name + b": hi - lo is not finite in f32")
    # 7. the count
    refused(call(P, P, TOO_MANY, psg.F32, 4), RANGE, name + b": more than 2^32-2 keys in one request")
    # no keys: a no-op behind the rules about dtype, width and the range
    assert call(None, None, 0, psg.F32, 4) == OK
    assert call(None, None, 0, psg.F64, 4096, 0.5, 0.5) == OK
    refused(call(None, None, 0, psg.F32, 0), INVALID, b"outside [1, 4096]")
    refused(call(None, None, 0, psg.F32, 4, 1.0, 0.0), INVALID, b"above hi")
