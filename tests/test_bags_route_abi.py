"""Bags across servers in the C-ABI (psg_route_bags, psg_pool_reduce): exported,
bound, and bad arguments refused with their code before any device call.

CPU-only: nothing here launches a kernel or touches a GPU.  The stand-in
pointers are never dereferenced by a call that is refused.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import psg

SYMBOLS = ("psg_route_bags", "psg_pool_reduce")
FAKE = 0x1000  # a non-null stand-in for a device pointer
INVALID, RANGE = 1, 4


def route_bags(offsets=FAKE, nb=3, perm=FAKE, n=4, key_pos=(0, 2, 4), so=FAKE, ns=None):
    kp = None if key_pos is None else np.asarray(key_pos, dtype=np.uint64)
    ns = len(kp) - 1 if ns is None else ns
    return psg.lib().psg_route_bags(offsets, nb, perm, n, ns, None if kp is None else kp.ctypes.data_as(C.c_void_p),
                                    so, None)


def pool_reduce(out=FAKE, partials=(0x2000, 0x3000), k=None, count=4, dtype=psg.F32, null_list=False):
    k = len(partials) if k is None else k
    arr = (C.c_void_p * max(len(partials), 1))(*partials)
    return psg.lib().psg_pool_reduce(out, None if null_list else arr, k, count, dtype, None)


def err():
    return psg.lib().psg_last_error()


def test_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (psg_\w+)", out))
    assert set(SYMBOLS) <= exported


def test_binding_binds_the_symbols():
    for s in SYMBOLS:
        assert s in psg.EXPORTS
        assert getattr(psg.lib(), s).argtypes is not None
    assert callable(psg.route_bags) and callable(psg.pool_reduce)


def test_route_bags_refuses_nulls():
    assert route_bags(offsets=None) == INVALID and b"null offsets" in err()
    assert route_bags(so=None) == INVALID and b"null server_offsets" in err()
    assert route_bags(key_pos=None, ns=2) == INVALID and b"null key_pos" in err()


@pytest.mark.parametrize("ns", [0, -1, psg.ROUTE_MAX_SERVERS + 1])
def test_route_bags_refuses_a_server_count_outside_the_limit(ns):
    kp = np.zeros(psg.ROUTE_MAX_SERVERS + 2, dtype=np.uint64)
    assert route_bags(key_pos=kp, n=0, ns=ns) == INVALID and b"servers outside [1, 64]" in err()


@pytest.mark.parametrize("key_pos", [(1, 2, 4), (0, 2, 3), (0, 2, 5), (0, 5, 4), (0, 3, 2, 4)])
def test_route_bags_refuses_bounds_that_do_not_ascend_from_0_to_n(key_pos):
    assert route_bags(key_pos=key_pos) == INVALID and b"key_pos" in err()


def test_route_bags_refuses_more_than_2_32_minus_2_keys_or_bags():
    big = 2**32 - 1
    assert route_bags(n=big, key_pos=(0, 2, big)) == RANGE and b"more than 2^32-2" in err()
    assert route_bags(nb=big) == RANGE and b"more than 2^32-2" in err()
    # the argument checks come first: a bad count with a null array is INVALID
    assert route_bags(nb=big, offsets=None) == INVALID


def test_route_bags_without_bags_is_a_no_op():
    assert route_bags(offsets=None, nb=0, so=None) == 0
    psg.route_bags(None, 0, None, 4, np.array([0, 1, 4], dtype=np.uint64), None)


@pytest.mark.parametrize("k", [0, -1, psg.ROUTE_MAX_SERVERS + 1])
def test_pool_reduce_refuses_a_frame_count_outside_the_limit(k):
    assert pool_reduce(k=k) == INVALID and b"partials outside [1, 64]" in err()


def test_pool_reduce_refuses_bad_arguments():
    assert pool_reduce(dtype=9) == INVALID and b"unknown dtype" in err()
    assert pool_reduce(out=None) == INVALID and b"null out or partials" in err()
    assert pool_reduce(null_list=True) == INVALID and b"null out or partials" in err()
    assert pool_reduce(partials=(0x2000, 0)) == INVALID and b"partial 1 is null" in err()
    assert pool_reduce(partials=(0x2000, 0x3002)) == INVALID and b"not aligned" in err()
    # out inside a partial's bytes, either way round
    assert pool_reduce(out=0x2000, partials=(0x3000, 0x2000)) == INVALID and b"overlaps partial 1" in err()
    assert pool_reduce(out=0x2008, partials=(0x2000,), count=4) == INVALID and b"overlaps partial 0" in err()
    assert pool_reduce(out=0x2000, partials=(0x2008,), count=4) == INVALID and b"overlaps partial 0" in err()


def test_pool_reduce_of_nothing_is_a_no_op():
    assert pool_reduce(out=None, partials=(0,), count=0) == 0
