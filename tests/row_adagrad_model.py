"""RowModel with row-wise Adagrad (psg_table_set_adagrad, include/psg.h): one f64
accumulator per row, and _step restated in numpy f64 with the tree of the header.
Every update call of RowModel then serves an Adagrad table as it stands."""
import numpy as np

from row_model import F32, INVALID, UNSUPPORTED, Refused, RowModel


def tree_sum(y):
    """y[:, :P] (P a power of two) summed per row by the header's tree; y is overwritten"""
    h = y.shape[1] // 2
    while h >= 1:
        y[:, :h] += y[:, h:2 * h]
        h //= 2
    return y[:, 0]


def pow2_above(w):
    return 1 << (w - 1).bit_length()


class RowAdagradModel(RowModel):
    def __init__(self, dtype, width, **kw):
        self.adagrad = None
        super().__init__(dtype, width, **kw)

    def clear(self):
        super().clear()
        self.acc = np.zeros(0, np.float64)

    def set_adagrad(self, lr, eps=1e-8, initial_accumulator=0.0):
        if self.dtype != F32:
            return Refused(UNSUPPORTED)
        ok = np.isfinite(lr) and np.isfinite(eps) and eps >= 0 and np.isfinite(initial_accumulator) and \
            initial_accumulator >= 0
        if self.adam is not None or self.adagrad is not None or not ok:
            return Refused(INVALID)
        self.adagrad = (float(lr), float(eps), float(initial_accumulator))
        self.acc = np.full(self.size, initial_accumulator, np.float64)
        return {}

    def _follow(self, old_keys, old_acc):
        """acc by key: a key that stayed keeps its accumulator, a new one starts afresh"""
        acc = np.full(self.size, self.adagrad[2] if self.adagrad else 0.0, np.float64)
        p, found = self._find(old_keys)
        acc[p[found]] = old_acc[found]
        self.acc = acc

    def _insert(self, keys):
        old = self.keys, self.acc
        idx = super()._insert(keys)
        self._follow(*old)
        return idx

    def erase(self, keys):
        old = self.keys, self.acc
        r = super().erase(keys)
        self._follow(*old)
        return r

    def _step(self, ri, g, lr, iteration):
        if not self.adagrad:
            return super()._step(ri, g, lr, iteration)
        alr, eps, _ = self.adagrad
        g = (np.float32(lr) * np.ascontiguousarray(g, dtype=np.float32).reshape(len(ri), self.w)).astype(np.float64)
        y = np.zeros((len(ri), pow2_above(self.w)), np.float64)
        y[:, :self.w] = g * g
        acc = self.acc[ri] + tree_sum(y) / np.float64(self.w)
        with np.errstate(invalid="ignore", divide="ignore"):
            step = np.float64(alr) / (np.sqrt(acc) + np.float64(eps))
            w = (self.rows[ri].astype(np.float64) - step[:, None] * g).astype(np.float32)
        self.acc[ri] = acc
        self.rows[ri] = w
        return w
