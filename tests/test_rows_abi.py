"""The row-valued table's C-ABI (psg_table_*): exported, bound, and its
arguments validated before any device call.

CPU-only: nothing here launches a kernel or touches a GPU.
"""
import re
import subprocess

import pytest

import psg

TABLE_SYMBOLS = ["psg_table_create", "psg_table_destroy", "psg_table_get_info", "psg_table_clear",
                 "psg_table_handle", "psg_table_dump"]


def test_library_exports_the_table_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (psg_\w+)", out))
    missing = [s for s in TABLE_SYMBOLS if s not in exported]
    assert not missing, missing


def test_binding_binds_the_table_symbols():
    missing = [s for s in TABLE_SYMBOLS if s not in psg.EXPORTS]
    assert not missing, missing
    lib = psg.lib()
    for s in TABLE_SYMBOLS:
        assert getattr(lib, s).argtypes is not None, s


@pytest.mark.parametrize("args,what", [
    ((psg.F32, 0, 0, 10, 0), "width"),        # width 0
    ((psg.F32, 4097, 0, 10, 0), "width"),     # width above 4096
    ((99, 4, 0, 10, 0), "dtype"),             # bad dtype
    ((psg.F32, 4, 11, 10, 0), "key range"),   # key_begin > key_end
])
def test_invalid_table_arguments_fail_before_any_device_call(args, what):
    with pytest.raises(psg.PsgError) as ei:
        psg.Table(*args)
    assert ei.value.code == 1 and what in str(ei.value), str(ei.value)
