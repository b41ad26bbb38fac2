"""The row table's merged update in the C-ABI (psg_table_update_merged):
exported, bound, and bad arguments refused before any device call.

CPU-only: nothing here launches a kernel or touches a GPU.
"""
import ctypes as C
import re
import subprocess

import psg

SYMBOL = "psg_table_update_merged"


def test_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert SYMBOL in set(re.findall(r"\bT (psg_\w+)", out))


def test_binding_binds_the_symbol():
    assert SYMBOL in psg.EXPORTS
    assert getattr(psg.lib(), SYMBOL).argtypes is not None
    assert callable(psg.Table.update_merged)
    assert (psg.MERGED_SAME_LIST, psg.MERGED_SORTED) == (1, 2)


def test_a_null_table_is_refused_before_any_device_call():
    lib = psg.lib()
    assert lib.psg_table_update_merged(None, psg.PUSH, 1, None, None, None, None, 0.01, 0, None, None) == 1
    assert b"null table" in lib.psg_last_error()


def test_a_frame_count_outside_1_to_16_is_refused_before_any_device_call():
    """The count is checked before the table is looked at: the stand-in table
    (zeroed host memory, there is no device to create one on) is never read."""
    lib = psg.lib()
    stand_in = C.create_string_buffer(512)
    table = C.cast(stand_in, C.c_void_p)
    for k in (0, 17, -1):
        assert lib.psg_table_update_merged(table, psg.PUSH, k, None, None, None, None, 0.01, 0, None, None) == 1
        msg = lib.psg_last_error()
        assert b"frames outside [1, 16]" in msg and str(k).encode() in msg, msg
