"""Row-wise Adagrad on 16-bit rows (psg_table_set_adagrad_half, include/psg.h) in
numpy: round16 in the header's arithmetic form, the step's words from the Philox
of row_init_model, and RowAdagradModel (with RowInitModel's initial rows) whose
_step ends in round16.  Rows are bit patterns (uint16); replies are f32."""
import numpy as np

from row_adagrad_model import RowAdagradModel, pow2_above, tree_sum
from row_init_model import INIT_ZERO, MASK, S32, RowInitModel, init_rows, philox4x32_10
from row_model import BF16, F16, F32, INVALID, UNSUPPORTED, Refused, from_acc, to_acc

NEAREST, STOCHASTIC = 0, 1
FORMAT = {F16: (10, -14), BF16: (7, -126)}  # explicit mantissa bits, the smallest normal exponent
QNAN = {F16: 0x7E00, BF16: 0x7FC0}


def nearest16(dtype, v):
    """f32 -> bit patterns, to nearest even (numpy's float16; from_acc's integer RNE); a NaN the format's quiet NaN"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = from_acc(dtype, v)
    return np.where(np.isnan(v), np.uint16(QNAN[dtype]), h).astype(np.uint16)


def round16(dtype, v, r):
    """PSG_ROUND_STOCHASTIC: v f32, r its 16-bit words; every operation below is exact in f64"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    mbits, emin = FORMAT[dtype]
    fin = np.isfinite(v)
    a = np.where(fin, np.abs(v), 0).astype(np.float64)
    q = np.ldexp(1.0, np.maximum(np.frexp(a)[1] - 1, emin) - mbits)  # frexp: a = f * 2^e with f in [0.5, 1)
    t = a / q
    n = np.floor(t)
    k = np.floor((t - n) * 65536.0).astype(np.int64)
    up = (k + np.asarray(r).astype(np.int64)) >> 16
    with np.errstate(over="ignore"):
        mag = np.copysign((n + up) * q, v).astype(np.float32)  # representable, or 2^(emax + 1): inf at the latest below
    return np.where(fin, nearest16(dtype, mag), nearest16(dtype, v))


class RowAdagradHalfModel(RowAdagradModel, RowInitModel):
    """The parents refuse to train a table that is not F32 by looking at self.dtype:
    while a request of a table with the state is served, dtype reads F32 (lifted);
    the arithmetic below takes the stored type from self.half."""
    dtype = property(lambda self: F32 if self.lifted else self.half, lambda self, value: None)

    def __init__(self, dtype, width, **kw):
        self.half, self.lifted, self.rounding, self.seed = dtype, False, NEAREST, 0
        super().__init__(dtype, width, **kw)

    def _lifted(self, method, *args):
        self.lifted = True
        try:
            return method(*args)
        finally:
            self.lifted = False

    def set_adagrad_half(self, lr, eps=1e-8, initial_accumulator=0.0, rounding=STOCHASTIC, seed=0):
        if self.half not in (F16, BF16):
            return Refused(UNSUPPORTED)
        r = self._lifted(self.set_adagrad, lr, eps, initial_accumulator)
        if not isinstance(r, Refused) and rounding not in (NEAREST, STOCHASTIC):
            self.adagrad, r = None, Refused(INVALID)
        if not isinstance(r, Refused):
            self.rounding, self.seed = rounding, int(seed)
        return r

    def initial(self, keys):
        if self.init is None or self.init[3] == INIT_ZERO:
            return np.zeros((len(keys), self.w), self.st)
        return init_rows(keys, self.half, self.w, *self.init[:3])

    def words(self, keys, acc):
        """(n, width) 16-bit words: half c % 8 of the block (key, A lo ^ A hi, c / 8) under the seed"""
        n, nb = len(keys), (self.w + 7) // 8
        a = np.ascontiguousarray(acc).view(np.uint64)
        ctr = np.zeros((n, nb, 4), np.uint64)
        ctr[:, :, 0], ctr[:, :, 1] = (keys & MASK)[:, None], (keys >> S32)[:, None]
        ctr[:, :, 2], ctr[:, :, 3] = ((a ^ (a >> S32)) & MASK)[:, None], np.arange(nb, dtype=np.uint64)[None, :]
        x = philox4x32_10(ctr, (self.seed & 0xFFFFFFFF, self.seed >> 32))
        return np.stack([x & np.uint32(0xFFFF), x >> np.uint32(16)], axis=-1).reshape(n, nb * 8)[:, :self.w]

    def _step(self, ri, g, lr, iteration):
        alr, eps, _ = self.adagrad
        g = (np.float32(lr) * np.ascontiguousarray(g, dtype=np.float32).reshape(len(ri), self.w)).astype(np.float64)
        y = np.zeros((len(ri), pow2_above(self.w)), np.float64)
        y[:, :self.w] = g * g
        before = self.acc[ri].copy()
        acc = before + tree_sum(y) / np.float64(self.w)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            step = np.float64(alr) / (np.sqrt(acc) + np.float64(eps))
            v = (to_acc(self.half, self.rows[ri]).astype(np.float64) - step[:, None] * g).astype(np.float32)
        if self.rounding == STOCHASTIC:
            h = round16(self.half, v, self.words(self.keys[ri], before))
        else:
            h = nearest16(self.half, v)
        self.acc[ri], self.rows[ri] = acc, h
        return to_acc(self.half, h)  # a reply is the stored row widened

    def _merge(self, keys, E, lr, iteration):
        return to_acc(self.half, super()._merge(keys, E, lr, iteration))


for _name in ("_update", "update_merged", "update_pooled_weighted", "update_pooled_merged"):
    def _served(self, *args, _parent=getattr(RowAdagradModel, _name), **kw):
        if self.adagrad is None:
            return _parent(self, *args, **kw)
        return self._lifted(lambda: _parent(self, *args, **kw))
    setattr(RowAdagradHalfModel, _name, _served)
