"""The row table's pooled calls in the C-ABI (psg_table_lookup_pooled /
psg_table_update_pooled): declared, exported, bound, and bad arguments refused
before any device call, in the order include/psg.h states.

CPU-only: nothing here launches a kernel or touches a GPU.  The addresses given
for device arrays are not mapped and the table is zeroed host memory: a call
that got as far as a device call would not return the code it is asked for.
"""
import ctypes as C
import os
import re
import subprocess

import psg

SYMBOLS = ("psg_table_lookup_pooled", "psg_table_update_pooled")
OK, INVALID, RANGE, UNSUPPORTED = 0, 1, 4, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = C.c_void_p(0x1000)
TOO_MANY = (1 << 32) - 1


def stand_in_table(dtype=psg.F32):
    """zeroed host memory in a table's place (there is no device to create one
    on), its first word the dtype: a call that refuses its arguments reads
    nothing else of it"""
    buf = C.create_string_buffer(512)
    C.cast(buf, C.POINTER(C.c_int))[0] = dtype
    return buf, C.cast(buf, C.c_void_p)


def lookup(table, keys, offsets, out, n, nb):
    return psg.lib().psg_table_lookup_pooled(table, keys, offsets, out, n, nb, None)


def update(table, keys, offsets, grads, n, nb, iteration=0):
    return psg.lib().psg_table_update_pooled(table, keys, offsets, grads, n, nb, 0.1, iteration, None)


def last_error():
    return psg.lib().psg_last_error()


def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "psg.h")).read()
    for s in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % s, text, re.M), s
    assert re.search(r"^#define PSG_ABI_VERSION 1$", text, re.M), "the change is additive"


def test_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r"\bT (psg_\w+)", out))


def test_binding_binds_the_symbols():
    for s in SYMBOLS:
        assert s in psg.EXPORTS
        assert getattr(psg.lib(), s).argtypes is not None
    assert callable(psg.Table.lookup_pooled) and callable(psg.Table.update_pooled)


def test_refusals_come_in_the_stated_order():
    """each call breaks the rule under test AND every later one: the message
    names the first"""
    keep, table = stand_in_table()
    for call, name, rows in ((lookup, b"psg_table_lookup_pooled", b"out"), (update, b"psg_table_update_pooled", b"grads")):
        # 1. a null table (with null keys, null offsets, null rows as well)
        assert call(None, None, None, None, 5, 2) == INVALID
        assert name + b": null table" in last_error()
        # 2. null keys with n > 0 (with null offsets and null rows as well)
        assert call(table, None, None, None, 5, 2) == INVALID
        assert name + b": null keys" in last_error()
        # 3. null offsets, or null out / grads, with nb > 0 (with too many keys as well)
        assert call(table, PTR, None, PTR, TOO_MANY, 2) == INVALID
        assert name + b": null offsets" in last_error()
        assert call(table, PTR, PTR, None, TOO_MANY, 2) == INVALID
        assert name + b": null " + rows in last_error()
        # 4. keys and no bag (with too many keys as well)
        assert call(table, PTR, None, None, TOO_MANY, 0) == INVALID
        assert name + b": 4294967295 keys and no bag" in last_error()
        # then the count
        assert call(table, PTR, PTR, PTR, TOO_MANY, 2) == RANGE
        assert name + b": more than 2^32-2 keys" in last_error()
        assert call(table, PTR, PTR, PTR, 5, TOO_MANY) == RANGE
        assert name + b": more than 2^32-2 bags" in last_error()
    assert bytes(keep.raw) == bytes(512), "the table was written"


def test_null_keys_are_fine_without_keys():
    """n == 0 with nb == 0 needs no array at all"""
    keep, table = stand_in_table()
    assert lookup(table, None, None, None, 0, 0) == OK
    assert update(table, None, None, None, 0, 0) == OK
    del keep


def test_no_bags_is_a_no_op_before_any_device_call():
    keep, table = stand_in_table()
    assert lookup(table, PTR, PTR, PTR, 0, 0) == OK
    assert update(table, PTR, PTR, PTR, 0, 0) == OK
    assert bytes(keep.raw) == bytes(512), "the table was written"


def test_update_refuses_a_negative_iteration_before_any_device_call():
    keep, table = stand_in_table()
    assert update(table, PTR, PTR, PTR, 5, 2, iteration=-1) == INVALID
    assert b"psg_table_update_pooled: iteration -1 below 0" in last_error()
    # the argument refusals come first
    assert update(table, None, PTR, PTR, 5, 2, iteration=-1) == INVALID
    assert b"null keys" in last_error()
    del keep


def test_update_refuses_a_table_that_is_not_f32_before_any_device_call():
    for dtype in (psg.F64, psg.F16, psg.BF16):
        keep, table = stand_in_table(dtype)
        assert update(table, PTR, PTR, PTR, 5, 2) == UNSUPPORTED
        assert b"psg_table_update_pooled: the update is built for F32 tables" in last_error()
        assert update(table, PTR, PTR, PTR, 0, 0) == UNSUPPORTED, "also without bags, as psg_table_update without keys"
        del keep
