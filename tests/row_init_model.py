"""The initial rows of a row table (psg_table_set_init / psg_init_rows,
include/psg.h) restated in numpy, and the host model of a table that has an
initializer, for test_row_init_model.py (CPU), test_rows_init_gpu.py and the
tools that measure the feature.

philox4x32_10 is the standard Philox (Salmon et al., Random123) on arrays of
counters; init_rows is the header's definition, one numpy operation per stated
operation (the f32 multiply and the f32 add are two array operations, so
nothing is fused).  RowInitModel is RowModel with the three places changed
where the header says "or the table's initial row": the insert, the lookup and
the pooled lookups.  The module never imports psg.
"""
import numpy as np

import row_model as rm
from row_model import F32, F64, F16, BF16, POOL_MEAN, POOL_SUM, Refused, RowModel  # noqa: F401

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the round's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the key's Weyl constants
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
INIT_ZERO, INIT_UNIFORM = 0, 1


def philox4x32_10(counter, key):
    """counter: (..., 4) words, key: (2,) words -> (..., 4) uint32"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def init_words(keys, width, seed):
    """x of the definition: (n, width) uint32, column j from block j // 4, word j % 4"""
    keys = rm.u64(keys)
    n, nblocks = len(keys), (width + 3) // 4
    ctr = np.zeros((n, nblocks, 4), np.uint64)
    ctr[:, :, 0] = (keys & MASK)[:, None]
    ctr[:, :, 1] = (keys >> S32)[:, None]
    ctr[:, :, 2] = np.arange(nblocks, dtype=np.uint64)[None, :]
    seed = int(seed)
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return np.ascontiguousarray(x.reshape(n, nblocks * 4)[:, :width])


def unit_interval(x):
    """u of the definition: the upper 24 bits over 2^24, exact in f32"""
    u = (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    return u


def init_rows(keys, dtype, width, seed, lo, hi):
    """(n, width) initial rows in the table's storage type (halves as bit patterns)"""
    lo, hi = np.float32(lo), np.float32(hi)
    span = np.float32(hi - lo)  # one f32 subtraction
    prod = unit_interval(init_words(keys, width, seed)) * span  # one f32 multiply
    v = lo + prod  # one f32 add
    assert prod.dtype == np.float32 and v.dtype == np.float32
    if dtype == F64:
        return v.astype(np.float64)  # exact
    return np.ascontiguousarray(rm.from_acc(dtype, v))  # F32 as is; halves: one round-to-nearest-even


class RowInitModel(RowModel):
    """RowModel whose new rows are initial rows: set_init before the first request."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.init = None  # (seed, lo, hi)

    def set_init(self, seed, lo, hi, kind=INIT_UNIFORM):
        lo, hi = np.float32(lo), np.float32(hi)
        with np.errstate(all="ignore"):
            bad = (kind not in (INIT_ZERO, INIT_UNIFORM) or self.init is not None or not np.isfinite(lo)
                   or not np.isfinite(hi) or lo > hi or not np.isfinite(np.float32(hi - lo)))
        if bad:
            return Refused(rm.INVALID)
        self.init = (int(seed), lo, hi, kind)
        return {}

    def initial(self, keys):
        if self.init is None or self.init[3] == INIT_ZERO:
            return np.zeros((len(keys), self.w), self.st)
        return init_rows(keys, self.dtype, self.w, *self.init[:3])

    def _insert(self, keys):
        """RowModel._insert with the new rows from the generator; moments stay zero"""
        u = np.unique(keys)
        new = u[~self._find(u)[1]]
        idx = super()._insert(keys)
        if len(new):
            self.rows[np.searchsorted(self.keys, new)] = self.initial(new)
        return idx

    def lookup(self, keys):
        r = super().lookup(keys)
        if isinstance(r, Refused) or r["out"] is None:
            return r
        absent = r["found"] == 0
        r["out"][absent] = self.initial(rm.u64(keys)[absent])  # found stays 0
        return r

    def lookup_pooled_weighted(self, keys, offsets, weights=None, mode=POOL_SUM):
        """Every position adds: a present id its row, an absent one its initial
        row.  Served by the parent on a copy that holds the list's absent ids."""
        r = super().lookup_pooled_weighted(keys, offsets, weights, mode)
        if isinstance(r, Refused) or r["out"] is None:
            return r
        full = RowInitModel(self.dtype, self.w, self.kb, self.ke)
        full.init = self.init
        full.keys, full.rows = self.keys.copy(), self.rows.copy()
        full.m, full.v = self.m.copy(), self.v.copy()
        full._insert(rm.u64(keys))
        return RowModel.lookup_pooled_weighted(full, keys, offsets, weights, mode)

    def lookup_pooled(self, keys, offsets):
        return self.lookup_pooled_weighted(keys, offsets)


def new_model(profile, init):
    m = RowInitModel(profile["dtype"], profile["width"], profile.get("key_begin", 0), profile.get("key_end", rm.KMAX),
                     profile.get("capacity", 0))
    assert not isinstance(m.set_init(*init), Refused)
    return m
