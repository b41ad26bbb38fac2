"""psg_table_pooled_weight_grad (include/psg.h) restated in numpy: f64 products, the
tree over them padded with -0.0 to a power of two, one rounding to f32.  Every
add is one numpy f64 add of two arrays, so the order is the definition's."""
import numpy as np

import row_model as rm


def tree(y):
    """(..., W) f64 -> (...): y[c] += y[c + h] for c < h, h = P/2 .. 1"""
    w = y.shape[-1]
    p = 1 << (w - 1).bit_length()
    y = np.concatenate([y, np.full(y.shape[:-1] + (p - w,), -0.0)], axis=-1)
    while p > 1:
        p //= 2
        y = y[..., :p] + y[..., p:2 * p]
    return y[..., 0]


def weight_grad(dtype, rows, present, grads, offsets):
    """rows: (n, W) stored elements per position; present: False where the call gives +0.0f -> dw (n,) f32"""
    bag = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets).astype(np.int64))
    x = rm.to_acc(dtype, rows).astype(np.float64).reshape(len(bag), -1)
    with np.errstate(all="ignore"):
        dw = tree(np.asarray(grads, np.float32)[bag].astype(np.float64) * x).astype(np.float32)
    return np.where(present, dw, np.float32(0.0))
