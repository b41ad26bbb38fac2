"""The CPU oracle on special values, pinned against numpy.

test_rows_edges_gpu.py feeds the cross product of row_specials.SPECIALS through
the row kernels and compares with oracle.Store.  A disagreement there has to
point at the kernel, so the oracle's own sums (and, for the halves, its own
conversions) are first checked here against arithmetic that shares no code with
it.  No GPU needed.
"""
import numpy as np
import pytest

import oracle
import row_specials as rs

DTYPES = [oracle.F32, oracle.F64, oracle.F16, oracle.BF16]
IDS = ["f32", "f64", "f16", "bf16"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_lists_hold_what_they_claim(dtype):
    e, m = rs.FORMAT[dtype]
    s = rs.SPECIALS[dtype]
    assert len(s) >= 14 and len(np.unique(s)) == len(s)
    assert not rs.nan_mask(dtype, s).any()
    if dtype == oracle.BF16:
        f = (s.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    else:
        f = s.view({oracle.F16: np.float16, oracle.F32: np.float32, oracle.F64: np.float64}[dtype]).astype(np.float64)
    v = dict(zip(rs.NAMES, f.tolist()))
    emin, emax = 2 - (1 << (e - 1)), (1 << (e - 1)) - 1
    assert v["+0"] == 0 and v["-0"] == 0 and np.signbit(f[rs.NAMES.index("-0")])
    assert v["+inf"] == np.inf and v["-inf"] == -np.inf
    assert v["+minsub"] == 2.0 ** (emin - m) == -v["-minsub"]
    assert v["maxsub"] == 2.0 ** emin - 2.0 ** (emin - m)
    assert v["+minnorm"] == 2.0 ** emin == -v["-minnorm"]
    assert v["+max"] == (2 - 2.0 ** -m) * 2.0 ** emax == -v["-max"]
    assert v["one"] == 1.0
    assert v["p"] == {oracle.F16: 2048.0, oracle.BF16: 256.0, oracle.F32: 2.0 ** 24, oracle.F64: 2.0 ** 53}[dtype]
    assert v["p+2"] == v["p"] + 2
    assert v["halfulp_max"] == 2.0 ** (emax - m - 1)
    assert v["s"] == 1.5 * 2.0 ** emin


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_store_sums_of_the_cross_product_equal_numpy(dtype):
    """Push a, PushPull b on distinct keys: the store holds 0 + a (which turns
    -0 into +0), then (0 + a) + b.  The non-NaN sums equal numpy's bit for bit;
    the NaN sums are exactly the two (+inf, -inf) / (-inf, +inf) pairs."""
    a, b = rs.pairs(dtype)
    n = len(a)
    assert n == len(rs.SPECIALS[dtype]) ** 2
    keys = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(5)
    st = oracle.Store(dtype)
    st.handle(oracle.PUSH, keys, rs.storage(dtype, a), n)
    first = rs.np_add(dtype, np.zeros(n, rs.UINT[dtype]), a)
    k, held = st.dump()
    np.testing.assert_array_equal(k, keys)
    np.testing.assert_array_equal(rs.bits(dtype, held), first)  # no NaN yet
    minus0 = a == rs.specials(dtype)["-0"]
    np.testing.assert_array_equal(first[~minus0], a[~minus0])
    assert not first[minus0].any()

    reply = st.handle(oracle.PUSH | oracle.PULL, keys, rs.storage(dtype, b), n)
    exp = rs.np_add(dtype, first, b)
    _, held = st.dump()
    where_nan = rs.inf_pairs_mask(dtype, a, b)
    assert int(where_nan.sum()) == rs.N_NAN == 2
    for got in (reply, held):
        nan = rs.nan_mask(dtype, got)
        np.testing.assert_array_equal(nan, where_nan)
        assert int(nan.sum()) == 2
        np.testing.assert_array_equal(rs.bits(dtype, got)[~nan], exp[~nan])
    np.testing.assert_array_equal(rs.nan_mask(dtype, exp), where_nan)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_cross_product_reaches_every_edge(dtype):
    """The sums hold an overflow to inf, the tie that rounds to inf, a tie to
    even at ulp 2, subnormal results, a normal result of a subnormal operand and
    exact cancellation: the classes the GPU test relies on being present."""
    pats = rs.specials(dtype)
    a, b = rs.pairs(dtype)
    r = rs.np_add(dtype, a, b)

    def at(x, y):
        return int(r[(a == pats[x]) & (b == pats[y])][0])

    assert at("+max", "+max") == pats["+inf"] and at("-max", "-max") == pats["-inf"]
    assert at("+max", "halfulp_max") == pats["+inf"]
    assert at("p", "one") == pats["p"]            # 2^(m+1) + 1: tie, down to even
    assert at("p+2", "one") == pats["p+2"] + 1    # 2^(m+1) + 3: tie, up to even
    assert at("+minnorm", "-minsub") == pats["maxsub"]
    assert at("+minsub", "+minsub") == 2
    assert at("maxsub", "+minsub") == pats["+minnorm"]
    m = rs.FORMAT[dtype][1]
    assert at("s", "maxsub") == (2 << m) | (1 << (m - 2))  # 1.25 * 2 minnorm: the tie went to even
    for x, y in (("+max", "-max"), ("+minsub", "-minsub"), ("-minnorm", "+minnorm"), ("-0", "+0")):
        assert at(x, y) == 0
    assert at("-0", "-0") == pats["-0"]
