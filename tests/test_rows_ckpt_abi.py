"""The row table's assign and export in the C-ABI (psg_table_assign /
psg_table_export): exported, bound, and bad arguments refused before any device
call.

CPU-only: nothing here launches a kernel or touches a GPU.
"""
import ctypes as C
import re
import subprocess

import pytest

import psg

SYMBOLS = ("psg_table_assign", "psg_table_export")


def test_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r"\bT (psg_\w+)", out))


def test_binding_binds_the_symbols():
    for s in SYMBOLS:
        assert s in psg.EXPORTS
        assert getattr(psg.lib(), s).argtypes is not None
    assert callable(psg.Table.assign) and callable(psg.Table.export)


def test_a_null_table_is_refused_before_any_device_call():
    lib = psg.lib()
    assert lib.psg_table_assign(None, None, None, None, None, 0, None) == 1
    assert b"psg_table_assign: null table" in lib.psg_last_error()
    assert lib.psg_table_export(None, 0, 0, None, None, None, None, None) == 1
    assert b"psg_table_export: null table" in lib.psg_last_error()


@pytest.mark.parametrize("given,missing", [("m", "v"), ("v", "m")])
def test_one_moment_array_without_the_other_is_refused(given, missing):
    """The pairing is checked before the table is looked at: the stand-in table
    (zeroed host memory, there is no device to create one on) is never read, and
    neither is the array (an address that is not mapped)."""
    lib = psg.lib()
    stand_in = C.create_string_buffer(512)
    table = C.cast(stand_in, C.c_void_p)
    ptr = C.c_void_p(0x1000)
    m, v = (ptr, None) if given == "m" else (None, ptr)
    assert lib.psg_table_assign(table, None, None, m, v, 5, None) == 1
    msg = lib.psg_last_error()
    assert b"psg_table_assign: m and v come as a pair" in msg and f"{missing} is null".encode() in msg, msg
    assert lib.psg_table_export(table, 0, 5, None, None, m, v, None) == 1
    msg = lib.psg_last_error()
    assert b"psg_table_export: m_out and v_out come as a pair" in msg and f"{missing}_out is null".encode() in msg, msg
