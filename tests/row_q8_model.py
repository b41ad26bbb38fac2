"""The frozen 8-bit row (include/psg.h, "THE FROZEN ROW") restated in numpy: every
operation one f32 numpy operation on arrays, so each is rounded once and nothing
is fused.  The pooled expectation is the f32 pooling arithmetic of the row table
(row_model.RowModel.lookup_pooled_weighted) applied to the read-back rows."""
import numpy as np

import row_model as rm

f = np.float32


def quantise(x):
    """x: (n, W) f32, finite -> codes (n, W) u8, scale (n,), bias (n,); raises on a row the freeze refuses"""
    x = np.asarray(x, f)
    zero = x == 0
    lo, hi = x.min(1), x.max(1)
    # -0.0 ranks below +0.0: a zero extreme takes the sign the ranking gives it
    lo = np.where(lo == 0, np.where((zero & np.signbit(x)).any(1), f(-0.0), f(0.0)), lo)
    hi = np.where(hi == 0, np.where((zero & ~np.signbit(x)).any(1), f(0.0), f(-0.0)), hi)
    with np.errstate(all="ignore"):
        rng = hi - lo
        if not (np.isfinite(x).all() and np.isfinite(rng).all()):
            raise ValueError("a row holds a NaN or an infinity, or its range is not finite")
        bias = lo + f(0)
        scale = rng / f(255)
        q = (x - lo[:, None]) / scale[:, None]
        code = np.where(scale[:, None] == 0, f(0), np.minimum(np.rint(q), f(255)))
    assert rng.dtype == scale.dtype == q.dtype == bias.dtype == f
    return code.astype(np.uint8), scale, bias


def dequantise(code, scale, bias):
    """xhat = (float)code * scale + bias: one multiply, then one add"""
    xhat = code.astype(f) * scale[:, None]
    return xhat + bias[:, None]


def packed(code, scale, bias):
    """the external format: per row W codes, scale, bias (little-endian f32) -> (n, W + 8) u8"""
    head = np.stack([scale, bias], 1).astype("<f4").view(np.uint8).reshape(len(code), 8)
    return np.concatenate([code, head], 1)


def unpacked(rows, width):
    rows = np.asarray(rows, np.uint8).reshape(-1, width + 8)
    head = np.ascontiguousarray(rows[:, width:]).view("<f4")
    return rows[:, :width], head[:, 0].copy(), head[:, 1].copy()


def lookup(keys, xhat, q):
    """q: ids in any order -> (rows (n, W) f32, found (n,) u8): +0.0 rows for ids not held"""
    p = np.searchsorted(keys, q)
    found = (p < len(keys)) & (keys[np.minimum(p, len(keys) - 1)] == q) if len(keys) else np.zeros(len(q), bool)
    out = np.zeros((len(q), xhat.shape[1]), f)
    out[found] = xhat[p[found]]
    return out, found.astype(np.uint8)


def pooled(keys, xhat, q, offsets, weights=None, mode=rm.POOL_SUM):
    """the row table's own pooled arithmetic on an F32 table that holds xhat"""
    m = rm.RowModel(rm.F32, xhat.shape[1])
    m.assign(keys, xhat)
    return m.lookup_pooled_weighted(q, offsets, weights, mode)["out"]
