"""The row table's lookup and erase in the C-ABI (psg_table_lookup /
psg_table_erase): exported, bound, and bad arguments refused before any device
call.

CPU-only: nothing here launches a kernel or touches a GPU.
"""
import ctypes as C
import re
import subprocess

import psg

SYMBOLS = ("psg_table_lookup", "psg_table_erase")
INVALID = 1


def stand_in_table():
    """zeroed host memory in a table's place (there is no device to create one
    on): a call that refuses its arguments never reads past it"""
    buf = C.create_string_buffer(512)
    return buf, C.cast(buf, C.c_void_p)


def test_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r"\bT (psg_\w+)", out))


def test_binding_binds_the_symbols():
    for s in SYMBOLS:
        assert s in psg.EXPORTS
        assert getattr(psg.lib(), s).argtypes is not None
    assert callable(psg.Table.lookup) and callable(psg.Table.erase)


def test_a_null_table_is_refused_before_any_device_call():
    lib = psg.lib()
    assert lib.psg_table_lookup(None, None, None, None, 0, None) == INVALID
    assert b"psg_table_lookup: null table" in lib.psg_last_error()
    assert lib.psg_table_erase(None, None, 0, None, None) == INVALID
    assert b"psg_table_erase: null table" in lib.psg_last_error()


def test_null_keys_are_refused_before_any_device_call():
    """The addresses given for out, found and the count are not mapped: a call
    that got as far as a device call (or wrote the count) would not return 1."""
    lib = psg.lib()
    keep, table = stand_in_table()
    ptr = C.c_void_p(0x1000)
    assert lib.psg_table_lookup(table, None, ptr, ptr, 5, None) == INVALID
    assert b"psg_table_lookup: null keys" in lib.psg_last_error()
    assert lib.psg_table_erase(table, None, 5, None, None) == INVALID
    assert b"psg_table_erase: null keys" in lib.psg_last_error()
    del keep


def test_a_lookup_without_out_and_found_is_refused_before_any_device_call():
    lib = psg.lib()
    keep, table = stand_in_table()
    assert lib.psg_table_lookup(table, C.c_void_p(0x1000), None, None, 5, None) == INVALID
    assert b"psg_table_lookup: out and found are both null" in lib.psg_last_error()
    del keep


def test_an_empty_list_is_a_no_op_before_any_device_call():
    lib = psg.lib()
    keep, table = stand_in_table()
    erased = C.c_uint64(77)
    assert lib.psg_table_lookup(table, None, None, None, 0, None) == 0
    assert lib.psg_table_erase(table, None, 0, C.byref(erased), None) == 0
    assert erased.value == 0
    assert bytes(keep.raw) == bytes(512), "the table was written"
