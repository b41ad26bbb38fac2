"""Special floating-point operands shared by test_oracle_specials.py (CPU) and
test_rows_edges_gpu.py: per dtype a list of bit patterns, their cross product
as two operand arrays, the sums restated in numpy, and NaN masks on bits.

Everything is derived from the format's (exponent bits, explicit mantissa
bits), not from a conversion routine: the lists pin the oracle's conversions,
so they must not depend on them.  No pattern is a NaN.
"""
import numpy as np

F32, F64, F16, BF16 = 0, 1, 2, 3  # oracle.F32 ..., psg.F32 ...
FORMAT = {F16: (5, 10), BF16: (8, 7), F32: (8, 23), F64: (11, 52)}  # exponent bits, mantissa bits
UINT = {F16: np.uint16, BF16: np.uint16, F32: np.uint32, F64: np.uint64}
STORAGE = {F16: np.uint16, BF16: np.uint16, F32: np.float32, F64: np.float64}  # oracle.NP / the table's dumps


def specials(dtype):
    e, m = FORMAT[dtype]
    bias = (1 << (e - 1)) - 1
    sign = 1 << (e + m)
    inf = ((1 << e) - 1) << m
    one = bias << m
    p = (bias + m + 1) << m  # 2^(m+1): the first integer whose ulp is 2
    pats = {
        "+0": 0, "-0": sign,
        "+inf": inf, "-inf": sign | inf,
        "+minsub": 1, "-minsub": sign | 1,
        "maxsub": (1 << m) - 1,
        "+minnorm": 1 << m, "-minnorm": sign | (1 << m),
        "+max": inf - 1, "-max": sign | (inf - 1),
        "one": one,
        "p": p, "p+2": p + 1,
        # 2^(emax - m - 1), half an ulp of the largest finite: max + it is the tie
        # between max (odd mantissa) and 2^(emax + 1), which rounds to inf
        "halfulp_max": (2 * bias - m - 1) << m,
        # 1.5 * minnorm: plus maxsub it is (2.5 - 2^-m) * minnorm, a normal result
        # and the tie between two neighbours of the binade above
        "s": (1 << m) | (1 << (m - 1)),
    }
    return pats


SPECIALS = {dt: np.array(list(specials(dt).values()), dtype=UINT[dt]) for dt in FORMAT}
NAMES = list(specials(F32))
N_NAN = 2  # of a cross product's sums: (+inf) + (-inf) and (-inf) + (+inf), nothing else


def pairs(dtype):
    """The full cross product (a, b) of SPECIALS[dtype] as two arrays of bit
    patterns, a varying slowest."""
    s = SPECIALS[dtype]
    return np.repeat(s, len(s)), np.tile(s, len(s))


def storage(dtype, bit_patterns):
    """bit patterns -> the array type the oracle and the table take for dtype"""
    return np.ascontiguousarray(bit_patterns, dtype=UINT[dtype]).view(STORAGE[dtype])


def bits(dtype, a):
    return np.ascontiguousarray(a).view(UINT[dtype])


def nan_mask(dtype, a):
    """NaN by class, on the bits: exponent all ones and a mantissa that is not zero."""
    e, m = FORMAT[dtype]
    b = bits(dtype, a).astype(np.uint64)
    return (((b >> np.uint64(m)) & np.uint64((1 << e) - 1)) == (1 << e) - 1) & ((b & np.uint64((1 << m) - 1)) != 0)


def inf_pairs_mask(dtype, a_bits, b_bits):
    """where a cross product holds (+inf, -inf) or (-inf, +inf)"""
    pats = specials(dtype)
    pi, ni = pats["+inf"], pats["-inf"]
    return ((a_bits == pi) & (b_bits == ni)) | ((a_bits == ni) & (b_bits == pi))


def np_add(dtype, a_bits, b_bits):
    """a + b in numpy, on and to bit patterns: native for F32 / F64; for the
    halves the f32 sum of the widened operands rounded once to nearest even
    (F16: numpy's own float16 conversion; BF16: the shift and the integer
    round-to-nearest-even of test_oracle.py).  NaN results keep whatever
    pattern numpy gives: compare them by nan_mask only."""
    a_bits = np.asarray(a_bits, dtype=UINT[dtype])
    b_bits = np.asarray(b_bits, dtype=UINT[dtype])
    with np.errstate(all="ignore"):
        if dtype in (F32, F64):
            return bits(dtype, a_bits.view(STORAGE[dtype]) + b_bits.view(STORAGE[dtype]))
        if dtype == F16:
            s = a_bits.view(np.float16).astype(np.float32) + b_bits.view(np.float16).astype(np.float32)
            return s.astype(np.float16).view(np.uint16)
        fa = (a_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
        fb = (b_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
        u = (fa + fb).view(np.uint32).astype(np.uint64)
        rne = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
        nan = ((u & np.uint64(0x7F800000)) == 0x7F800000) & ((u & np.uint64(0x7FFFFF)) != 0)
        return np.where(nan, np.uint16(0x7FC0), rne).astype(np.uint16)
