"""A mean over a sharded bag in the C-ABI (psg_pool_reduce_mean,
psg_pool_scale_mean): declared, exported, bound, and bad arguments refused with
their code, in the documented order, before any device call.

CPU-only: nothing here launches a kernel or touches a GPU.  The stand-in
pointers are never dereferenced by a call that is refused.  Each refusal is
shown with ONE argument broken, and its place in the order by breaking it
together with every check that comes after it.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

import psg

SYMBOLS = ("psg_pool_reduce_mean", "psg_pool_scale_mean")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "psg.h")
INVALID, RANGE = 1, 4
BIG = 2 ** 32 - 1  # one above the 2^32 - 2 bags a call takes


def reduce_mean(out=0x1000, partials=(0x2000, 0x3000), k=None, offsets=0x8000, nb=2, width=4, dtype=psg.F32,
                null_list=False):
    k = len(partials) if k is None else k
    arr = (C.c_void_p * max(len(partials), 1))(*partials)
    return psg.lib().psg_pool_reduce_mean(out, None if null_list else arr, k, offsets, nb, width, dtype, None)


def scale_mean(dst=0x1000, grads=0x2000, offsets=0x8000, nb=2, width=4):
    return psg.lib().psg_pool_scale_mean(dst, grads, offsets, nb, width, None)


def err():
    return psg.lib().psg_last_error()


def test_header_library_and_binding_agree_on_the_symbols():
    header = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (psg_\w+)", out))
    for s in SYMBOLS:
        assert re.search(r"^int %s\(" % s, header, re.M), s
        assert s in exported
        assert s in psg.EXPORTS
        assert getattr(psg.lib(), s).argtypes is not None
    assert callable(psg.pool_reduce_mean) and callable(psg.pool_scale_mean)
    assert len(psg.lib().psg_pool_reduce_mean.argtypes) == 8
    assert len(psg.lib().psg_pool_scale_mean.argtypes) == 6


# ---- psg_pool_reduce_mean: every check, one argument broken ---------------------------
@pytest.mark.parametrize("k", [0, -1, 65])
def test_reduce_mean_refuses_a_frame_count_outside_the_limit(k):
    assert reduce_mean(k=k) == INVALID and b"partials outside [1, 64]" in err()


def test_reduce_mean_refuses_an_unknown_dtype():
    assert reduce_mean(dtype=9) == INVALID and b"unknown dtype 9" in err()


@pytest.mark.parametrize("width", [0, 4097])
def test_reduce_mean_refuses_a_width_outside_the_limit(width):
    assert reduce_mean(width=width) == INVALID and b"outside [1, 4096]" in err()


def test_reduce_mean_refuses_nulls():
    assert reduce_mean(out=None) == INVALID and b"null out or partials" in err()
    assert reduce_mean(null_list=True) == INVALID and b"null out or partials" in err()
    assert reduce_mean(offsets=None) == INVALID and b"null offsets" in err()
    assert reduce_mean(partials=(0x2000, 0)) == INVALID and b"partial 1 is null" in err()


def test_reduce_mean_refuses_a_pointer_off_its_element():
    assert reduce_mean(out=0x1002) == INVALID and b"not aligned to its 4-byte" in err()
    assert reduce_mean(partials=(0x2000, 0x3002)) == INVALID and b"not aligned to its 4-byte" in err()
    assert reduce_mean(partials=(0x2004, 0x3000), dtype=psg.F64) == INVALID and b"not aligned to its 8-byte" in err()
    assert reduce_mean(out=0x1001, dtype=psg.F16) == INVALID and b"not aligned to its 2-byte" in err()
    assert reduce_mean(offsets=0x8004) == INVALID and b"offsets are not aligned to 8" in err()


def test_reduce_mean_refuses_an_out_that_overlaps_a_partial():
    # nb * width * 4 = 32 bytes
    assert reduce_mean(out=0x2000, partials=(0x3000, 0x2000)) == INVALID and b"overlaps partial 1" in err()
    assert reduce_mean(out=0x201c, partials=(0x2000,)) == INVALID and b"overlaps partial 0" in err()
    assert reduce_mean(out=0x2000, partials=(0x201c,)) == INVALID and b"overlaps partial 0" in err()
    # frames of 2 * BIG bytes: one byte short of apart is refused; exactly apart is
    # no overlap, and the next refusal (the bag count) is reached
    assert reduce_mean(out=0x2000 + 2 * BIG - 2, partials=(0x2000,), nb=BIG, width=1, dtype=psg.F16) == INVALID
    assert b"overlaps partial 0" in err()
    assert reduce_mean(out=0x2000 + 2 * BIG, partials=(0x2000,), nb=BIG, width=1, dtype=psg.F16) == RANGE


def test_reduce_mean_refuses_more_than_2_32_minus_2_bags():
    assert reduce_mean(out=0x1000, partials=(1 << 50, 1 << 51), nb=BIG) == RANGE and b"more than 2^32-2" in err()


def test_reduce_mean_of_no_bags_is_a_no_op():
    assert reduce_mean(out=None, partials=(0,), offsets=None, nb=0) == 0
    assert reduce_mean(out=None, null_list=True, offsets=None, nb=0) == 0
    psg.pool_reduce_mean(None, [None], None, 0, 4, psg.F32)


def test_reduce_mean_refuses_in_the_documented_order():
    far = (1 << 50, 1 << 51)
    # everything broken: k is named first
    assert reduce_mean(out=None, partials=(0, 0), k=0, offsets=None, nb=BIG, width=0, dtype=9) == INVALID
    assert b"partials outside" in err()
    assert reduce_mean(out=None, partials=(0, 0), offsets=None, nb=BIG, width=0, dtype=9) == INVALID
    assert b"unknown dtype" in err()
    assert reduce_mean(out=None, partials=(0, 0), offsets=None, nb=BIG, width=0) == INVALID
    assert b"width 0 outside" in err()
    assert reduce_mean(out=None, partials=(0x2002, 0), offsets=0x8004, nb=BIG) == INVALID
    assert b"null out or partials" in err()
    assert reduce_mean(out=0x2002, partials=(0x2002, 0), offsets=None, nb=BIG) == INVALID
    assert b"null offsets" in err()
    assert reduce_mean(out=0x2002, partials=(0x2002, 0), offsets=0x8004, nb=BIG) == INVALID
    assert b"partial 1 is null" in err()
    assert reduce_mean(out=0x2002, partials=(0x2002, 0x3000), offsets=0x8004, nb=BIG) == INVALID
    assert b"not aligned to its 4-byte" in err()
    assert reduce_mean(out=0x2000, partials=(0x2000, 0x3000), offsets=0x8004, nb=BIG) == INVALID
    assert b"offsets are not aligned" in err()
    assert reduce_mean(out=0x2000, partials=(0x2000, 0x3000), nb=BIG) == INVALID
    assert b"overlaps partial 0" in err()
    assert reduce_mean(out=0x1000, partials=far, nb=BIG) == RANGE
    # with no bags the pointers are not looked at, the first three checks are
    assert reduce_mean(out=None, partials=(0,), offsets=None, nb=0, width=0) == INVALID
    assert reduce_mean(out=None, partials=(0,), offsets=None, nb=0, dtype=9) == INVALID
    assert reduce_mean(out=None, partials=(0,), k=65, offsets=None, nb=0) == INVALID


# ---- psg_pool_scale_mean ---------------------------------------------------------------
@pytest.mark.parametrize("width", [0, 4097])
def test_scale_mean_refuses_a_width_outside_the_limit(width):
    assert scale_mean(width=width) == INVALID and b"outside [1, 4096]" in err()


def test_scale_mean_refuses_nulls():
    assert scale_mean(dst=None) == INVALID and b"null dst or grads" in err()
    assert scale_mean(grads=None) == INVALID and b"null dst or grads" in err()
    assert scale_mean(offsets=None) == INVALID and b"null offsets" in err()


def test_scale_mean_refuses_a_pointer_off_its_element():
    assert scale_mean(dst=0x1002) == INVALID and b"not aligned to its 4-byte" in err()
    assert scale_mean(grads=0x2001) == INVALID and b"not aligned to its 4-byte" in err()
    assert scale_mean(offsets=0x8004) == INVALID and b"offsets are not aligned to 8" in err()


def test_scale_mean_refuses_overlapping_frames():
    assert scale_mean(dst=0x2000, grads=0x2000) == INVALID and b"dst overlaps grads" in err()
    assert scale_mean(dst=0x201c, grads=0x2000) == INVALID and b"dst overlaps grads" in err()
    assert scale_mean(dst=0x2000, grads=0x201c) == INVALID and b"dst overlaps grads" in err()


def test_scale_mean_refuses_more_than_2_32_minus_2_bags():
    assert scale_mean(dst=0x1000, grads=1 << 50, nb=BIG) == RANGE and b"more than 2^32-2" in err()


def test_scale_mean_of_no_bags_is_a_no_op():
    assert scale_mean(dst=None, grads=None, offsets=None, nb=0) == 0
    psg.pool_scale_mean(None, None, None, 0, 4)


def test_scale_mean_refuses_in_the_documented_order():
    assert scale_mean(dst=None, grads=None, offsets=None, nb=BIG, width=0) == INVALID and b"width 0" in err()
    assert scale_mean(dst=None, grads=0x2002, offsets=None, nb=BIG) == INVALID and b"null dst or grads" in err()
    assert scale_mean(dst=0x2002, grads=0x2002, offsets=None, nb=BIG) == INVALID and b"null offsets" in err()
    assert scale_mean(dst=0x2002, grads=0x2002, offsets=0x8004, nb=BIG) == INVALID and b"4-byte" in err()
    assert scale_mean(dst=0x2000, grads=0x2000, offsets=0x8004, nb=BIG) == INVALID and b"offsets are not" in err()
    assert scale_mean(dst=0x2000, grads=0x2000, nb=BIG) == INVALID and b"dst overlaps grads" in err()
    assert scale_mean(dst=0x1000, grads=1 << 50, nb=BIG) == RANGE
