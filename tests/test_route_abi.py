"""The worker's routing calls in the C-ABI (psg_route, psg_rows_gather,
psg_rows_scatter): exported, bound, and bad arguments refused before any device
call.

CPU-only: nothing here launches a kernel or touches a GPU.  The stand-in
pointers are never dereferenced by a call that is refused.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import psg

SYMBOLS = ("psg_route", "psg_rows_gather", "psg_rows_scatter")
FAKE = 0x1000  # a non-null stand-in for a device pointer


def route(keys, n, begins, ends, routed=FAKE, perm=FAKE, key_pos=True, identity=True, ns=None):
    ns = len(begins) if ns is None else ns
    kp = np.full(len(begins) + 1, 77, dtype=np.uint64)
    ident = C.c_int(-1)
    rc = psg.lib().psg_route(keys, n, ns, begins.ctypes.data_as(C.c_void_p), ends.ctypes.data_as(C.c_void_p),
                             routed, perm, kp.ctypes.data_as(C.c_void_p) if key_pos else None,
                             C.byref(ident) if identity else None, None)
    return rc, kp, ident.value


def test_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (psg_\w+)", out))
    assert set(SYMBOLS) <= exported


def test_binding_binds_the_symbols():
    for s in SYMBOLS:
        assert s in psg.EXPORTS
        assert getattr(psg.lib(), s).argtypes is not None
    assert callable(psg.route) and callable(psg.rows_gather) and callable(psg.rows_scatter)
    assert psg.ROUTE_MAX_SERVERS == 64


def test_route_refuses_null_keys():
    b, e = psg.server_ranges(2)
    rc, _, _ = route(None, 4, b, e)
    assert rc == 1 and b"null keys" in psg.lib().psg_last_error()


def test_route_refuses_null_outputs():
    b, e = psg.server_ranges(2)
    assert route(FAKE, 4, b, e, routed=None)[0] == 1
    assert route(FAKE, 4, b, e, perm=None)[0] == 1
    assert b"null routed_keys or perm" in psg.lib().psg_last_error()
    assert route(FAKE, 4, b, e, key_pos=False)[0] == 1
    assert route(FAKE, 4, b, e, identity=False)[0] == 1
    assert b"null ranges or outputs" in psg.lib().psg_last_error()


@pytest.mark.parametrize("ns", [0, -1, psg.ROUTE_MAX_SERVERS + 1])
def test_route_refuses_a_server_count_outside_the_limit(ns):
    b, e = psg.server_ranges(psg.ROUTE_MAX_SERVERS + 1)
    rc, _, _ = route(FAKE, 4, b, e, ns=ns)
    assert rc == 1 and b"servers outside [1, 64]" in psg.lib().psg_last_error()


def test_route_refuses_ranges_that_are_not_contiguous():
    b, e = psg.server_ranges(3)
    e[1] -= 1
    rc, _, _ = route(FAKE, 4, b, e)
    assert rc == 1 and b"not adjacent" in psg.lib().psg_last_error()


def test_route_refuses_more_than_2_32_minus_2_keys():
    b, e = psg.server_ranges(2)
    rc, _, _ = route(FAKE, 2**32 - 1, b, e)
    assert rc == 1 and b"more than 2^32-2" in psg.lib().psg_last_error()


def test_an_empty_list_is_routed_without_a_device():
    b, e = psg.server_ranges(3)
    rc, kp, ident = route(None, 0, b, e, routed=None, perm=None)
    assert rc == 0 and kp.tolist() == [0, 0, 0, 0] and ident == 1
    kp, ident = psg.route(None, 0, b, e, None, None)
    assert kp.tolist() == [0, 0, 0, 0] and ident is True


@pytest.mark.parametrize("name", ["psg_rows_gather", "psg_rows_scatter"])
def test_row_copies_refuse_bad_arguments(name):
    fn = getattr(psg.lib(), name)
    for row_bytes in (0, 4096 * 8 + 1):
        assert fn(FAKE, FAKE, FAKE, 4, row_bytes, None) == 1
        assert b"row_bytes" in psg.lib().psg_last_error()
    assert fn(FAKE, FAKE, None, 4, 16, None) == 1
    assert b"null perm" in psg.lib().psg_last_error()
    assert fn(None, FAKE, FAKE, 4, 16, None) == 1
    assert fn(FAKE, None, FAKE, 4, 16, None) == 1
    assert b"null rows" in psg.lib().psg_last_error()
    assert fn(FAKE, FAKE, FAKE, 2**32 - 1, 16, None) == 1
    assert fn(None, None, None, 0, 16, None) == 0  # an empty list is a no-op
