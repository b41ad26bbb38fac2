"""The row table's order-preserving C-ABI (psg_table_handle_any / _update_any):
exported, bound, and a null table refused before any device call.

CPU-only: nothing here launches a kernel or touches a GPU.
"""
import re
import subprocess

import psg

ANY_SYMBOLS = ["psg_table_handle_any", "psg_table_update_any"]


def test_library_exports_the_any_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (psg_\w+)", out))
    missing = [s for s in ANY_SYMBOLS if s not in exported]
    assert not missing, missing


def test_binding_binds_the_any_symbols():
    missing = [s for s in ANY_SYMBOLS if s not in psg.EXPORTS]
    assert not missing, missing
    lib = psg.lib()
    for s in ANY_SYMBOLS:
        assert getattr(lib, s).argtypes is not None, s
    for method in ("handle_any", "update_any"):
        assert callable(getattr(psg.Table, method)), method


def test_a_null_table_is_refused_before_any_device_call():
    lib = psg.lib()
    assert lib.psg_table_handle_any(None, psg.PUSH, None, None, None, 4, None) == 1
    assert b"null table" in lib.psg_last_error()
    assert lib.psg_table_update_any(None, psg.PUSH, None, None, None, 4, 0.01, 0, None) == 1
    assert b"null table" in lib.psg_last_error()
