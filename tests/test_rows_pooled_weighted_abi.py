"""The row table's weighted and mean pooled calls in the C-ABI
(psg_table_lookup_pooled_weighted / psg_table_update_pooled_weighted): declared,
exported, bound, and bad arguments refused before any device call, in the order
include/psg.h states.

CPU-only: nothing here launches a kernel or touches a GPU.  The addresses given
for device arrays are not mapped and the table is zeroed host memory: a call
that got as far as a device call would not return the code it is asked for.
"""
import ctypes as C
import os
import re
import subprocess

import psg

SYMBOLS = ("psg_table_lookup_pooled_weighted", "psg_table_update_pooled_weighted")
OK, INVALID, RANGE, UNSUPPORTED = 0, 1, 4, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = C.c_void_p(0x1000)
ODD = C.c_void_p(0x1002)  # not on a 4-B boundary
TOO_MANY = (1 << 32) - 1
SUM, MEAN, NO_MODE = 0, 1, 2


def stand_in_table(dtype=psg.F32):
    """zeroed host memory in a table's place (there is no device to create one
    on), its first word the dtype: a call that refuses its arguments reads
    nothing else of it"""
    buf = C.create_string_buffer(512)
    C.cast(buf, C.POINTER(C.c_int))[0] = dtype
    return buf, C.cast(buf, C.c_void_p)


def lookup(table, keys, offsets, weights, mode, out, n, nb, iteration=0):
    return psg.lib().psg_table_lookup_pooled_weighted(table, keys, offsets, weights, mode, out, n, nb, None)


def update(table, keys, offsets, weights, mode, grads, n, nb, iteration=0):
    return psg.lib().psg_table_update_pooled_weighted(table, keys, offsets, weights, mode, grads, n, nb, 0.1,
                                                      iteration, None)


def last_error():
    return psg.lib().psg_last_error()


def test_header_declares_the_symbols_and_the_modes():
    text = open(os.path.join(ROOT, "include", "psg.h")).read()
    for s in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % s, text, re.M), s
    assert re.search(r"^#define PSG_POOL_SUM\s+0$", text, re.M)
    assert re.search(r"^#define PSG_POOL_MEAN\s+1$", text, re.M)
    assert re.search(r"^#define PSG_ABI_VERSION 1$", text, re.M), "the change is additive"
    assert text.index("psg_table_update_pooled(") < text.index("psg_table_lookup_pooled_weighted("), \
        "behind psg_table_update_pooled"


def test_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r"\bT (psg_\w+)", out))


def test_binding_binds_the_symbols():
    for s in SYMBOLS:
        assert s in psg.EXPORTS
        assert getattr(psg.lib(), s).argtypes is not None
    assert callable(psg.Table.lookup_pooled_weighted) and callable(psg.Table.update_pooled_weighted)
    assert (psg.POOL_SUM, psg.POOL_MEAN) == (SUM, MEAN)


def test_refusals_come_in_the_stated_order():
    """each call breaks the rule under test AND every later one: the message
    names the first.  The later ones of a lookup: no such mode (which hides MEAN
    with weights, so that rule has a probe of its own), weights off a 4-B
    boundary, too many keys; an update adds a negative iteration in front of the
    count and, behind it, a table that is not F32."""
    keep16, f16 = stand_in_table(psg.F16)
    for call, name, rows in ((lookup, b"psg_table_lookup_pooled_weighted", b"out"),
                             (update, b"psg_table_update_pooled_weighted", b"grads")):
        # 1. the unweighted call's own refusals
        assert call(None, None, None, ODD, NO_MODE, None, TOO_MANY, 2, -1) == INVALID
        assert name + b": null table" in last_error()
        assert call(f16, None, None, ODD, NO_MODE, None, TOO_MANY, 2, -1) == INVALID
        assert name + b": null keys" in last_error()
        assert call(f16, PTR, None, ODD, NO_MODE, PTR, TOO_MANY, 2, -1) == INVALID
        assert name + b": null offsets" in last_error()
        assert call(f16, PTR, PTR, ODD, NO_MODE, None, TOO_MANY, 2, -1) == INVALID
        assert name + b": null " + rows in last_error()
        assert call(f16, PTR, None, ODD, NO_MODE, None, TOO_MANY, 0, -1) == INVALID
        assert name + b": 4294967295 keys and no bag" in last_error()
        # 2. a mode that is none
        for mode in (NO_MODE, -1):
            assert call(f16, PTR, PTR, ODD, mode, PTR, TOO_MANY, 2, -1) == INVALID
            assert name + b": mode %d is no pooling mode" % mode in last_error()
        # 3. MEAN with weights
        assert call(f16, PTR, PTR, ODD, MEAN, PTR, TOO_MANY, 2, -1) == INVALID
        assert name + b": weights with PSG_POOL_MEAN" in last_error()
        # 4. weights off a 4-B boundary
        assert call(f16, PTR, PTR, ODD, SUM, PTR, TOO_MANY, 2, -1) == INVALID
        assert name + b": weights not on a 4-B boundary" in last_error()
        # 5. update only: a negative iteration
        if call is update:
            assert call(f16, PTR, PTR, PTR, SUM, PTR, TOO_MANY, 2, -1) == INVALID
            assert name + b": iteration -1 below 0" in last_error()
        # 6. the counts
        assert call(f16, PTR, PTR, PTR, SUM, PTR, TOO_MANY, 2, 0) == RANGE
        assert name + b": more than 2^32-2 keys" in last_error()
        assert call(f16, PTR, PTR, None, MEAN, PTR, 5, TOO_MANY, 0) == RANGE
        assert name + b": more than 2^32-2 bags" in last_error()
        # 7. update only: a table that is not F32
        if call is update:
            for weights, mode in ((PTR, SUM), (None, SUM), (None, MEAN)):
                assert call(f16, PTR, PTR, weights, mode, PTR, 5, 2, 0) == UNSUPPORTED
                assert name + b": the update is built for F32 tables" in last_error()
    assert bytes(keep16.raw)[4:] == bytes(508), "the table was written"


def test_no_bags_is_a_no_op_before_any_device_call():
    keep, table = stand_in_table()
    for weights, mode in ((PTR, SUM), (None, SUM), (None, MEAN)):
        assert lookup(table, PTR, PTR, weights, mode, PTR, 0, 0) == OK
        assert update(table, PTR, PTR, weights, mode, PTR, 0, 0) == OK
        assert lookup(table, None, None, weights, mode, None, 0, 0) == OK
        assert update(table, None, None, weights, mode, None, 0, 0) == OK
    assert bytes(keep.raw) == bytes(512), "the table was written"


def test_no_bags_does_not_hide_a_refusal():
    """nb == 0 is a no-op only for a call that passed every check in front of it"""
    keep, table = stand_in_table()
    assert lookup(table, None, None, None, NO_MODE, None, 0, 0) == INVALID
    assert update(table, None, None, PTR, MEAN, None, 0, 0) == INVALID
    assert update(table, None, None, None, SUM, None, 0, 0, -1) == INVALID
    del keep
