"""psg_table_lookup_pooled_batch in the C-ABI: exported, bound, and a bad call
refused as a whole before any device call, in the order include/psg.h states.

CPU-only: the addresses given for device arrays are not mapped and the tables are
zeroed host memory (test_rows_pooled_abi.py's stand-in): a call that got as far as
a device call would not return the code it is asked for.  Each case breaks the
rule under test and, where it can, every later one: the message names the first.
"""
import ctypes as C

import pytest

import psg
from test_rows_pooled_abi import INVALID, OK, PTR, RANGE, TOO_MANY, UNSUPPORTED, last_error, stand_in_table

NAME = "psg_table_lookup_pooled_batch"
P, ODD = PTR.value, 0x1002
SUM, MEAN = psg.POOL_SUM, psg.POOL_MEAN
ARRAYS = ("tables", "keys", "offsets", "weights", "modes", "outs", "ns", "nbs")
# an entry is (table, keys, offsets, weights, mode, out, n, nb); "t" / "h": an F32 / F16 stand-in
FINE = ("t", P, P, None, SUM, P, 5, 2)
WORST = (None, None, None, ODD, 7, None, TOO_MANY, 0)  # breaks every rule about an entry
NOOP = ("t", None, None, None, SUM, None, 0, 0)


def call(entries, tables, T=None, drop=(), status=None):
    cols = list(zip(*entries))
    kinds = (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64)
    cols[0] = [tables[t].value if t else None for t in cols[0]]
    a = [None if name in drop else (kind * len(entries))(*col) for name, kind, col in zip(ARRAYS, kinds, cols)]
    return psg.lib().psg_table_lookup_pooled_batch(len(entries) if T is None else T, *a, None, status)


def test_exported_and_bound():
    assert NAME in psg.EXPORTS and len(getattr(psg.lib(), NAME).argtypes) == 11
    assert psg.BATCH_MAX == 1024 and callable(psg.lookup_pooled_batch)


@pytest.mark.parametrize("entries,kw,code,msg", [
    ([WORST], dict(T=0, drop=ARRAYS), INVALID, "0 entries outside [1, 1024]"),
    ([WORST], dict(T=psg.BATCH_MAX + 1, drop=ARRAYS), INVALID, "1025 entries outside [1, 1024]"),
    *[([WORST], dict(drop=(a, "weights")), INVALID, "null %s array" % a) for a in ARRAYS if a != "weights"],
    ([("t", P, P, None, 7, P, TOO_MANY, 2)], dict(drop=("weights",)), INVALID, "mode 7 of entry 0"),  # no weights array: fine
    ([FINE, WORST], {}, INVALID, "null table of entry 1"),
    ([FINE, ("t", None, None, ODD, 7, None, TOO_MANY, 2)], {}, INVALID, "null keys of entry 1"),
    ([FINE, ("t", P, None, ODD, 7, None, TOO_MANY, 2)], {}, INVALID, "null offsets of entry 1"),
    ([FINE, ("t", P, P, ODD, 7, None, TOO_MANY, 2)], {}, INVALID, "null out of entry 1"),
    ([FINE, ("t", P, None, ODD, 7, None, TOO_MANY, 0)], {}, INVALID, "4294967295 keys and no bag to hold them in entry 1"),
    ([FINE, ("t", P, P, ODD, 7, P, TOO_MANY, 2)], {}, INVALID, "mode 7 of entry 1"),
    ([FINE, ("t", P, P, ODD, MEAN, P, TOO_MANY, 2)], {}, INVALID, "weights with PSG_POOL_MEAN in entry 1"),
    ([FINE, ("t", P, P, ODD, SUM, P, TOO_MANY, 2)], {}, INVALID, "weights of entry 1 not on a 4-B boundary"),
    ([("t", P, P, P, 7, P, 5, 2), WORST], {}, INVALID, "mode 7 of entry 0"),  # entries in index order
    ([("h", P, P, P, SUM, P, TOO_MANY, 2), WORST], {}, INVALID, "null table of entry 1"),  # every INVALID before a RANGE
    ([FINE, ("h", P, P, P, SUM, P, TOO_MANY, 2)], {}, RANGE, "more than 2^32-2 keys or bags in entry 1"),
    ([FINE, ("h", P, P, P, SUM, P, 5, TOO_MANY)], {}, RANGE, "more than 2^32-2 keys or bags in entry 1"),
    ([FINE, NOOP, ("h", P, P, P, SUM, P, 5, 2)], {}, UNSUPPORTED, "entry 2's table has dtype"),
    ([NOOP, ("h", None, None, None, MEAN, None, 0, 0)], {}, UNSUPPORTED, "entry 1's table has dtype"),  # also of no-ops
])
def test_refusals_come_in_the_stated_order(entries, kw, code, msg):
    (keep, t), (keep_h, h) = stand_in_table(), stand_in_table(psg.F16)
    status = (C.c_int * 4)(9, 9, 9, 9)
    assert call(entries, {"t": t, "h": h}, status=status, **kw) == code
    assert ("%s: %s" % (NAME, msg)).encode() in last_error(), last_error()
    assert list(status) == [9] * 4, "a refused call wrote statuses"
    assert bytes(keep.raw) == bytes(512) and bytes(keep_h.raw)[4:] == bytes(508), "a table was written"


def test_entries_without_bags_are_noops():
    keep, t = stand_in_table()
    status = (C.c_int * 3)(9, 9, 9)
    assert call([NOOP, ("t", P, P, None, MEAN, P, 0, 0), NOOP], {"t": t}, status=status) == OK
    assert list(status) == [OK] * 3 and bytes(keep.raw) == bytes(512)
