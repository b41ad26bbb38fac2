"""The order in which the row table's request calls refuse bad arguments
(psg_table_handle, _handle_any, _update, _update_any, _update_merged, _assign,
_export, _lookup, _erase): each case breaks one rule and every later one, and
the code and the message are those of the first.

CPU-only: nothing here launches a kernel or touches a GPU.  The addresses given
for device arrays are not mapped and the table is zeroed host memory (the
stand-in of test_rows_pooled_abi.py, no Adam state, no rows): a call that got as
far as a device call would not return the code it is asked for.  Two rules need
a table the stand-in cannot be (psg_table_assign's "moments without rows" needs
Adam state, psg_table_export's "null rows_out" needs rows) and are not reached.
"""
import ctypes as C

import psg
from test_rows_pooled_abi import INVALID, OK, PTR, RANGE, TOO_MANY, UNSUPPORTED, last_error, stand_in_table

P = PTR.value
PUSH, PULL = psg.PUSH, psg.PULL
NOT_F32 = (psg.F64, psg.F16, psg.BF16)


def refused(rc, code, text):
    assert rc == code, (rc, last_error())
    assert text in last_error(), last_error()


def ptrs(xs):
    return (C.c_void_p * len(xs))(*xs)


def words(xs):
    return (C.c_uint64 * len(xs))(*xs)


def test_handle_and_handle_any():
    keep, table = stand_in_table()
    for symbol in ("psg_table_handle", "psg_table_handle_any"):
        fn, name = getattr(psg.lib(), symbol), symbol.encode()

        def call(t, flags, keys, vals, out, n):
            return fn(t, flags, keys, vals, out, n, None)

        # 1. a null table
        refused(call(None, 7, None, None, None, TOO_MANY), INVALID, name + b": null table")
        # 2. flags outside [1, 3], also without keys
        for flags in (7, 0, -1, 4):
            refused(call(table, flags, None, None, None, TOO_MANY), INVALID, name + (b": bad flags %d" % flags))
            refused(call(table, flags, None, None, None, 0), INVALID, name + (b": bad flags %d" % flags))
        # no keys: a no-op in front of every rule about the arrays
        for flags in (PUSH, PULL, PUSH | PULL):
            assert call(table, flags, None, None, None, 0) == OK
        # 3. null keys
        refused(call(table, PUSH | PULL, None, None, None, TOO_MANY), INVALID, name + b": null keys")
        # 4. a Push without vals
        refused(call(table, PUSH | PULL, P, None, None, TOO_MANY), INVALID, b"push without vals")
        refused(call(table, PUSH, P, None, None, TOO_MANY), INVALID, b"push without vals")
        # 5. a Pull without out
        refused(call(table, PUSH | PULL, P, P, None, TOO_MANY), INVALID, b"pull without out buffer")
        refused(call(table, PULL, P, None, None, TOO_MANY), INVALID, b"pull without out buffer")
        # 6. the count
        for flags, vals, out in ((PUSH | PULL, P, P), (PUSH, P, None), (PULL, None, P)):
            refused(call(table, flags, P, vals, out, TOO_MANY), RANGE,
                    name + b": more than 2^32-2 keys in one request")
    assert bytes(keep.raw) == bytes(512), "the table was written"


def test_update_and_update_any():
    keep, table = stand_in_table()
    keep64, table64 = stand_in_table(psg.F64)
    for symbol in ("psg_table_update", "psg_table_update_any"):
        fn, name = getattr(psg.lib(), symbol), symbol.encode()

        def call(t, flags, keys, grads, out, n, iteration=0):
            return fn(t, flags, keys, grads, out, n, 0.1, iteration, None)

        # 1. a null table
        refused(call(None, PULL, None, None, None, TOO_MANY, -1), INVALID, name + b": null table")
        # 2. flags that are neither PUSH nor PUSH|PULL
        for flags in (PULL, 0, 4, 7, -1):
            refused(call(table64, flags, None, None, None, TOO_MANY, -1), INVALID,
                    name + (b": flags %d are neither PUSH nor PUSH|PULL" % flags))
        # 3. iteration < 0
        for flags in (PUSH, PUSH | PULL):
            refused(call(table64, flags, None, None, None, TOO_MANY, -1), INVALID, name + b": iteration -1 below 0")
            refused(call(table64, flags, None, None, None, 0, -7), INVALID, name + b": iteration -7 below 0")
        # 4. a table that is not F32, also without keys
        for dtype in NOT_F32:
            k2, t2 = stand_in_table(dtype)
            for n in (TOO_MANY, 0):
                refused(call(t2, PUSH | PULL, None, None, None, n), UNSUPPORTED,
                        name + b": the update is built for F32 tables")
            del k2
        # no keys: a no-op in front of every rule about the arrays
        for flags in (PUSH, PUSH | PULL):
            assert call(table, flags, None, None, None, 0) == OK
        # 5. null keys
        refused(call(table, PUSH | PULL, None, None, None, TOO_MANY), INVALID, name + b": null keys")
        # 6. null grads
        refused(call(table, PUSH | PULL, P, None, None, TOO_MANY), INVALID, name + b": null grads")
        refused(call(table, PUSH, P, None, None, TOO_MANY), INVALID, name + b": null grads")
        # 7. a Pull without out
        refused(call(table, PUSH | PULL, P, P, None, TOO_MANY), INVALID, b"pull without out buffer")
        # 8. the count
        refused(call(table, PUSH | PULL, P, P, P, TOO_MANY), RANGE, name + b": more than 2^32-2 keys in one request")
        refused(call(table, PUSH, P, P, None, TOO_MANY), RANGE, name + b": more than 2^32-2 keys in one request")
    assert bytes(keep.raw) == bytes(512) and bytes(keep64.raw)[4:] == bytes(508), "a table was written"


def merged(table, flags, frames, iteration=0, k=None, path=None, drop=()):
    """frames: (keys, n, grads, out) per frame, addresses as ints or None; drop:
    names of the host arrays passed as NULL"""
    cols = list(zip(*frames))
    arrays = {"keys": ptrs(cols[0]), "ns": words(cols[1]), "grads": ptrs(cols[2]), "outs": ptrs(cols[3])}
    a = {name: (None if name in drop else arr) for name, arr in arrays.items()}
    return psg.lib().psg_table_update_merged(table, flags, len(frames) if k is None else k, a["keys"], a["ns"],
                                             a["grads"], a["outs"], 0.1, iteration, None, path)


def test_update_merged():
    name = b"psg_table_update_merged"
    keep, table = stand_in_table()
    keep64, table64 = stand_in_table(psg.F64)
    bad = (None, TOO_MANY, None, None)  # breaks every per-frame rule
    fine = (P, 5, P, P)
    every = ("keys", "ns", "grads", "outs")
    # 1. a null table
    refused(merged(None, PULL, [bad], -1, k=17, drop=every), INVALID, name + b": null table")
    # 2. k outside [1, 16]
    for k in (0, 17, -1):
        refused(merged(table64, PULL, [bad], -1, k=k, drop=every), INVALID,
                name + (b": %d frames outside [1, 16]" % k))
    # 3. flags that are neither PUSH nor PUSH|PULL
    for flags in (PULL, 0, 4, -1):
        refused(merged(table64, flags, [bad], -1, drop=every), INVALID,
                name + (b": flags %d are neither PUSH nor PUSH|PULL" % flags))
    # 4. iteration < 0
    refused(merged(table64, PUSH | PULL, [bad], -1, drop=every), INVALID, name + b": iteration -1 below 0")
    # 5. keys, ns or grads null
    for missing in ("keys", "ns", "grads"):
        refused(merged(table64, PUSH | PULL, [bad], drop=(missing, "outs")), INVALID,
                name + b": null keys, ns or grads array")
    # 6. a Pull without the outs array; a Push needs none
    refused(merged(table64, PUSH | PULL, [bad], drop=("outs",)), INVALID, name + b": pull without outs array")
    refused(merged(table64, PUSH, [bad], drop=("outs",)), RANGE, name + b": more than 2^32-2 keys in one round")
    # 7. per frame in order: the count, null keys or grads, a Pull without out (the table is F64)
    refused(merged(table64, PUSH | PULL, [fine, bad]), RANGE, name + b": more than 2^32-2 keys in one round")
    refused(merged(table64, PUSH | PULL, [fine, (None, TOO_MANY - 5, None, None)]), RANGE,
            name + b": more than 2^32-2 keys in one round")
    refused(merged(table64, PUSH | PULL, [fine, (None, 5, None, None)]), INVALID,
            name + b": null keys or grads of frame 1")
    refused(merged(table64, PUSH | PULL, [fine, (P, 5, None, None)]), INVALID,
            name + b": null keys or grads of frame 1")
    refused(merged(table64, PUSH | PULL, [fine, (P, 5, P, None)]), INVALID,
            name + b": pull without out buffer of frame 1")
    # an earlier frame's fault is named before a later frame's
    refused(merged(table64, PUSH | PULL, [(P, 5, P, None), (None, TOO_MANY, None, None)]), INVALID,
            name + b": pull without out buffer of frame 0")
    # 8. a table that is not F32, also a round without keys
    for dtype in NOT_F32:
        k2, t2 = stand_in_table(dtype)
        for frames in ([fine], [fine, (P, 5, P, P)], [(None, 0, None, None)]):
            refused(merged(t2, PUSH | PULL, frames), UNSUPPORTED, name + b": the update is built for F32 tables")
        del k2
    # a round without keys: PSG_OK and *path_host 0
    path = C.c_int(-1)
    assert merged(table, PUSH | PULL, [(None, 0, None, None)] * 16, path=C.byref(path)) == OK
    assert path.value == 0
    assert bytes(keep.raw) == bytes(512) and bytes(keep64.raw)[4:] == bytes(508), "a table was written"


def test_assign():
    name = b"psg_table_assign"
    keep, table = stand_in_table()

    def call(t, keys, rows, m, v, n):
        return psg.lib().psg_table_assign(t, keys, rows, m, v, n, None)

    # 1. a null table
    refused(call(None, None, None, P, None, TOO_MANY), INVALID, name + b": null table")
    # 2. one of m and v alone, also without keys
    for n in (TOO_MANY, 0):
        refused(call(table, None, None, P, None, n), INVALID, name + b": m and v come as a pair, v is null")
        refused(call(table, None, None, None, P, n), INVALID, name + b": m and v come as a pair, m is null")
    # 3. moments for a table without Adam state, also without keys
    for n in (TOO_MANY, 0):
        refused(call(table, None, None, P, P, n), INVALID, name + b": moments for a table without Adam state")
    # no keys: a no-op in front of every rule about the arrays
    assert call(table, None, None, None, None, 0) == OK
    # 4. null keys
    refused(call(table, None, None, None, None, TOO_MANY), INVALID, name + b": null keys")
    # 5. the count, with rows and without
    refused(call(table, P, P, None, None, TOO_MANY), RANGE, name + b": more than 2^32-2 keys in one request")
    refused(call(table, P, None, None, None, TOO_MANY), RANGE, name + b": more than 2^32-2 keys in one request")
    assert bytes(keep.raw) == bytes(512), "the table was written"


def test_export():
    name = b"psg_table_export"
    keep, table = stand_in_table()

    def call(t, first, count, keys_out, rows_out, m_out, v_out):
        return psg.lib().psg_table_export(t, first, count, keys_out, rows_out, m_out, v_out, None)

    # 1. a null table
    refused(call(None, 1, 1, None, None, P, None), INVALID, name + b": null table")
    # 2. one of m_out and v_out alone
    refused(call(table, 1, 1, None, None, P, None), INVALID, name + b": m_out and v_out come as a pair, v_out is null")
    refused(call(table, 1, 1, None, None, None, P), INVALID, name + b": m_out and v_out come as a pair, m_out is null")
    # 3. moments of a table without Adam state, also without rows
    for first, count in ((1, 1), (0, 0)):
        refused(call(table, first, count, None, None, P, P), INVALID,
                name + b": moments of a table without Adam state")
    # 4. rows the table does not hold (it holds none)
    refused(call(table, 1, 1, None, None, None, None), INVALID, name + b": rows [1, 1 + 1) of a table of 0")
    refused(call(table, 0, 3, None, None, None, None), INVALID, name + b": rows [0, 0 + 3) of a table of 0")
    refused(call(table, 2, 0, None, None, None, None), INVALID, name + b": rows [2, 2 + 0) of a table of 0")
    # no rows: a no-op in front of the rule about rows_out
    assert call(table, 0, 0, None, None, None, None) == OK
    assert bytes(keep.raw) == bytes(512), "the table was written"


def test_lookup():
    name = b"psg_table_lookup"
    keep, table = stand_in_table()

    def call(t, keys, out, found, n):
        return psg.lib().psg_table_lookup(t, keys, out, found, n, None)

    # 1. a null table, also without keys
    for n in (TOO_MANY, 0):
        refused(call(None, None, None, None, n), INVALID, name + b": null table")
    # no keys: a no-op in front of every rule about the arrays
    assert call(table, None, None, None, 0) == OK
    # 2. null keys
    refused(call(table, None, None, None, TOO_MANY), INVALID, name + b": null keys")
    # 3. out and found both null
    refused(call(table, P, None, None, TOO_MANY), INVALID, name + b": out and found are both null")
    # 4. the count
    for out, found in ((P, P), (P, None), (None, P)):
        refused(call(table, P, out, found, TOO_MANY), RANGE, name + b": more than 2^32-2 keys in one request")
    assert bytes(keep.raw) == bytes(512), "the table was written"


def test_erase():
    name = b"psg_table_erase"
    keep, table = stand_in_table()

    def call(t, keys, n, erased=None):
        return psg.lib().psg_table_erase(t, keys, n, erased, None)

    # 1. a null table, also without keys; the count is not written
    erased = C.c_uint64(77)
    for n in (TOO_MANY, 0):
        refused(call(None, None, n, C.byref(erased)), INVALID, name + b": null table")
    assert erased.value == 77
    # no keys: a no-op in front of every rule about the arrays
    assert call(table, None, 0, C.byref(erased)) == OK
    assert erased.value == 0
    # 2. null keys; the count is zeroed before any refusal behind the table's
    erased = C.c_uint64(77)
    refused(call(table, None, TOO_MANY, C.byref(erased)), INVALID, name + b": null keys")
    assert erased.value == 0
    # 3. the count
    refused(call(table, P, TOO_MANY), RANGE, name + b": more than 2^32-2 keys in one request")
    assert bytes(keep.raw) == bytes(512), "the table was written"
