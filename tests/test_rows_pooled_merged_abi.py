"""The sync-mode round over pooled and plain frames in the C-ABI
(psg_table_update_pooled_merged): declared, exported, bound, and bad arguments
refused before any device call, in the order include/psg.h states.

CPU-only: nothing here launches a kernel or touches a GPU.  The addresses given
for device arrays are not mapped and the table is zeroed host memory (the
stand-in of test_rows_pooled_abi.py): a call that got as far as a device call
would not return the code it is asked for.
"""
import ctypes as C
import os
import re
import subprocess

import psg
from test_rows_pooled_abi import INVALID, OK, PTR, RANGE, ROOT, TOO_MANY, UNSUPPORTED, last_error, stand_in_table

SYMBOL = "psg_table_update_pooled_merged"
NAME = SYMBOL.encode()
P = PTR.value


def ptrs(xs):
    return (C.c_void_p * len(xs))(*xs)


def words(xs):
    return (C.c_uint64 * len(xs))(*xs)


def call(table, frames, iteration=0, k=None, path=None, drop=()):
    """frames: (keys, n, offsets, nb, grads) per frame, addresses as ints or
    None; drop: names of the host arrays passed as NULL"""
    cols = list(zip(*frames)) if frames else [(), (), (), (), ()]
    arrays = {"keys": ptrs(cols[0]), "ns": words(cols[1]), "offsets": ptrs(cols[2]), "nbs": words(cols[3]),
              "grads": ptrs(cols[4])}
    a = {name: (None if name in drop else arr) for name, arr in arrays.items()}
    return psg.lib().psg_table_update_pooled_merged(table, len(frames) if k is None else k, a["keys"], a["ns"],
                                                    a["offsets"], a["nbs"], a["grads"], 0.1, iteration, None, path)


POOLED = (P, 5, P, 2, P)
PLAIN = (P, 5, None, 0, P)


def test_header_declares_the_symbol():
    text = open(os.path.join(ROOT, "include", "psg.h")).read()
    assert re.search(r"^int\s+%s\s*\(" % SYMBOL, text, re.M)
    assert re.search(r"^#define PSG_ABI_VERSION 1$", text, re.M), "the change is additive"


def test_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", psg.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert SYMBOL in set(re.findall(r"\bT (psg_\w+)", out))
    assert psg.lib().psg_abi_version() == 1


def test_binding_binds_the_symbol():
    assert SYMBOL in psg.EXPORTS
    assert getattr(psg.lib(), SYMBOL).argtypes is not None
    assert callable(psg.Table.update_pooled_merged)


def test_refusals_come_in_the_stated_order():
    """each call breaks the rule under test AND every later one: the message
    names the first"""
    keep, table = stand_in_table()
    keep64, table64 = stand_in_table(psg.F64)
    bad_frame = (None, TOO_MANY, P, 0, None)  # breaks every per-frame rule, and the count
    # 1. a null table
    assert call(None, [bad_frame], iteration=-1, k=17, drop=("keys",)) == INVALID
    assert NAME + b": null table" in last_error()
    # 2. k outside [1, 16]
    for k in (0, 17, -1):
        assert call(table64, [bad_frame], iteration=-1, k=k, drop=("keys",)) == INVALID
        assert NAME + (b": %d frames outside [1, 16]" % k) in last_error()
    # 3. iteration < 0
    assert call(table64, [bad_frame], iteration=-1, drop=("keys",)) == INVALID
    assert NAME + b": iteration -1 below 0" in last_error()
    # 4. any of the five host arrays null
    for name in ("keys", "ns", "offsets", "nbs", "grads"):
        assert call(table64, [bad_frame], drop=(name,)) == INVALID
        assert NAME + b": null keys, ns, offsets, nbs or grads array" in last_error()
    # 5. per frame in order (frame 0 is fine, the count is not, the table is F64)
    fine = (P, 5, P, 2, P)
    assert call(table64, [fine, (None, TOO_MANY, P, 0, None)]) == INVALID
    assert NAME + b": null keys of frame 1" in last_error()
    assert call(table64, [fine, (P, TOO_MANY, P, 2, None)]) == INVALID
    assert NAME + b": null grads of pooled frame 1" in last_error()
    assert call(table64, [fine, (P, TOO_MANY, P, 0, None)]) == INVALID
    assert NAME + b": 4294967295 keys of frame 1 and no bag" in last_error()
    assert call(table64, [fine, (P, TOO_MANY, None, 0, None)]) == INVALID
    assert NAME + b": null grads of frame 1" in last_error()
    # an earlier frame's fault is named before a later frame's
    assert call(table64, [(P, 5, None, 0, None), (None, 5, P, 2, P)]) == INVALID
    assert NAME + b": null grads of frame 0" in last_error()
    # 6. the counts: keys, then gradient rows (the table is F64)
    assert call(table64, [fine, (P, TOO_MANY - 5, None, 0, P)]) == RANGE
    assert NAME + b": more than 2^32-2 keys" in last_error()
    assert call(table64, [(P, TOO_MANY, P, 2, P)]) == RANGE
    assert NAME + b": more than 2^32-2 keys" in last_error()
    assert call(table64, [fine, (P, 5, P, TOO_MANY - 2, P)]) == RANGE
    assert NAME + b": more than 2^32-2 gradient rows" in last_error()
    assert call(table64, [PLAIN, (P, 5, P, TOO_MANY - 5, P)]) == RANGE, "a plain frame's rows are its keys"
    assert NAME + b": more than 2^32-2 gradient rows" in last_error()
    # 7. a table that is not F32
    for dtype in (psg.F64, psg.F16, psg.BF16):
        k2, t2 = stand_in_table(dtype)
        for frames in ([POOLED], [PLAIN], [POOLED, PLAIN], [(None, 0, None, 0, None)]):
            assert call(t2, frames) == UNSUPPORTED
            assert NAME + b": the update is built for F32 tables" in last_error()
        del k2
    assert bytes(keep.raw) == bytes(512) and bytes(keep64.raw)[4:] == bytes(508), "a table was written"


def test_sixteen_frames_are_the_most():
    keep, table = stand_in_table()
    empty = (None, 0, None, 0, None)
    assert call(table, [empty] * 16) == OK
    assert call(table, [empty] * 17) == INVALID
    del keep


def test_rounds_without_keys_or_bags_are_no_ops_before_any_device_call():
    """nothing to merge and no offsets to check: PSG_OK, *path_host 0, and no
    array is read (the addresses are not mapped, the table is host memory)"""
    keep, table = stand_in_table()
    rounds = (
        [(None, 0, None, 0, None)],                          # one empty plain frame, no array at all
        [(P, 0, None, 7, P)] * 3,                            # plain frames ignore nbs
        [(None, 0, P, 0, None)],                             # one pooled frame without bags
        [(P, 0, P, 0, P), (None, 0, None, 0, None)],         # pooled without bags beside an empty plain frame
        [(P, 0, P, 0, P)] * 16,
    )
    for frames in rounds:
        path = C.c_int(-1)
        assert call(table, frames, path=C.byref(path)) == OK, frames
        assert path.value == 0
        assert call(table, frames) == OK, "path_host may be NULL"
    assert bytes(keep.raw) == bytes(512), "the table was written"
