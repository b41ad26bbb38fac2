"""The host model of the row table (tests/row_model.py) and the sequences
test_rows_sequences_gpu.py walks: the model against the definitions it must
agree with (include/psg.h), its optimizer step against the reference's own
rounds (tests/golden/lr_ref.npz), and a dry run of every sequence that asserts
what the sequence must contain, so that a pass on the GPU cannot be a vacuous one.
No GPU is used.
"""
import os

import numpy as np
import pytest

import row_model as rm
from row_model import F32, F64, F16, BF16, PUSH, PULL, Refused, RowModel

PP = PUSH | PULL
KEND = 1 << 40


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def same_state(a, b):
    np.testing.assert_array_equal(a.keys, b.keys)
    same(a.rows, b.rows)
    same(a.m, b.m)
    same(a.v, b.v)
    assert a.capacity == b.capacity


def random_keys(rng, n, hi=KEND):
    return np.sort(rng.choice(np.unique(rng.integers(0, hi, 2 * n + 16, dtype=np.uint64)), n, replace=False))


def trained(rng, width, adam, nkeys=600, dtype=F32):
    """a populated model whose rows (and moments) are not zero"""
    m = RowModel(dtype, width, 0, KEND)
    keys = random_keys(rng, nkeys)
    m.assign(keys, rm.values(rng, dtype, nkeys * width))
    if adam:
        m.set_adam(*rm.ADAM)
        m.update(PUSH, keys, rm.grads(rng, nkeys * width), rm.LR, 0)
    return m, keys


def twin(m):
    t = RowModel(m.dtype, m.w, m.kb, m.ke)
    t.keys, t.rows, t.m, t.v, t.adam, t.capacity = m.keys.copy(), m.rows.copy(), m.m.copy(), m.v.copy(), m.adam, m.capacity
    return t


def bagged(rng, keys, n, nb):
    """n ids (a fifth absent, repeats) in nb bags"""
    q = np.concatenate([rng.choice(keys, n - n // 5), random_keys(rng, n // 5)])
    q = rng.permutation(q).astype(np.uint64)
    cuts = np.sort(rng.integers(0, n + 1, nb - 1))
    return q, np.concatenate([[0], cuts, [n]]).astype(np.uint64)


# ---- the model against the definitions ------------------------------------------------------
@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("variant", ["sum", "weights", "mean"])
def test_update_pooled_is_update_merged_on_the_expanded_rows(variant, adam):
    rng = np.random.default_rng(1)
    a, keys = trained(rng, 5, adam)
    b = twin(a)
    q, offsets = bagged(rng, keys, 700, 200)
    grads = rng.uniform(-1, 1, 200 * 5).astype(np.float32)
    weights = rng.uniform(-2, 2, 700).astype(np.float32) if variant == "weights" else None
    mode = rm.POOL_MEAN if variant == "mean" else rm.POOL_SUM
    lens = np.diff(offsets).astype(np.int64)
    bag_of = np.repeat(np.arange(200), lens)
    E = grads.reshape(200, 5)[bag_of]
    if variant == "weights":
        E = weights[:, None] * E
    if variant == "mean":
        E = E / lens[bag_of].astype(np.float32)[:, None]
    assert E.dtype == np.float32
    if variant == "sum":
        r = a.update_pooled(q, offsets, grads, rm.LR, 3)
    else:
        r = a.update_pooled_weighted(q, offsets, grads, rm.LR, 3, weights, mode)
    assert r["path"] == rm.SORTED
    b.update_merged(PUSH, [q], [E], rm.LR, 3)
    same_state(a, b)
    assert a.size > len(keys)  # absent ids were inserted


def test_update_pooled_merged_is_update_merged_on_the_expanded_rows():
    rng = np.random.default_rng(2)
    a, keys = trained(rng, 4, True)
    b = twin(a)
    q0, o0 = bagged(rng, keys, 300, 90)
    q1 = rng.choice(keys, 200).astype(np.uint64)
    q2, o2 = bagged(rng, keys, 100, 7)
    g0, g1, g2 = (rng.uniform(-1, 1, n * 4).astype(np.float32) for n in (90, 200, 7))
    r = a.update_pooled_merged([(q0, o0, g0), (q1, None, g1), (q2, o2, g2)], rm.LR, 2)
    assert r["path"] == rm.SORTED
    b.update_merged(PUSH, [q0, q1, q2], [a.expand(o0, g0), g1, a.expand(o2, g2)], rm.LR, 2)
    same_state(a, b)


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_update_merged_of_one_frame_of_distinct_keys_is_update(adam):
    rng = np.random.default_rng(3)
    a, keys = trained(rng, 3, adam)
    b = twin(a)
    q = np.sort(np.concatenate([keys[::3], np.setdiff1d(random_keys(rng, 50), keys)]))
    g = rng.uniform(-1, 1, len(q) * 3).astype(np.float32)
    ra = a.update_merged(PP, [q], [g], rm.LR, 1)
    rb = b.update(PP, q, g, rm.LR, 1)
    assert ra["path"] == rm.SAME_LIST
    same(ra["outs"][0], rb["out"])
    same_state(a, b)
    # and update_any on the same list
    c = twin(b)
    same(b.update(PP, q, g, rm.LR, 2)["out"], c.update_any(PP, q, g, rm.LR, 2)["out"])
    same_state(b, c)


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16], ids=["f32", "f64", "f16", "bf16"])
def test_handle_any_on_an_ascending_list_is_handle(dtype):
    rng = np.random.default_rng(4)
    a, keys = trained(rng, 3, False, dtype=dtype)
    b = twin(a)
    q = np.sort(np.concatenate([keys[::2], np.setdiff1d(random_keys(rng, 50), keys)]))
    vals = rm.values(rng, dtype, len(q) * 3)
    for flags in (PUSH, PP, PULL):
        ra, rb = a.handle_any(flags, q, vals), b.handle(flags, q, vals)
        if flags & PULL:
            same(ra["out"], rb["out"])
    same_state(a, b)
    # repeats: the running row, occurrence by occurrence, is that of one-key requests
    hot = np.repeat(q[:2], 5)
    got = a.handle_any(PP, hot, vals[:30])["out"]
    for i in range(10):
        same(got[i], b.handle(PP, hot[i:i + 1], vals[3 * i:3 * i + 3])["out"][0])
    same_state(a, b)


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16], ids=["f32", "f64", "f16", "bf16"])
def test_bags_of_one_id_are_lookup(dtype):
    rng = np.random.default_rng(5)
    a, keys = trained(rng, 5, False, dtype=dtype)
    q, _ = bagged(rng, keys, 300, 2)
    offsets = np.arange(301, dtype=np.uint64)
    want = a.lookup(q)
    assert 0 < want["found"].sum() < 300
    same(a.lookup_pooled(q, offsets)["out"], want["out"])
    same(a.lookup_pooled_weighted(q, offsets, None, rm.POOL_MEAN)["out"], want["out"])
    same(a.lookup_pooled_weighted(q, offsets, np.ones(300, np.float32))["out"], want["out"])


@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16], ids=["f32", "f64", "f16", "bf16"])
def test_mean_is_weighted_by_the_reciprocal_where_the_length_is_a_power_of_two(dtype):
    """x / 2^k and x * 2^-k round alike, and a sum of rows scaled by 2^-k is the
    scaled sum, as long as nothing underflows: the rows are far from it."""
    rng = np.random.default_rng(6)
    a, keys = trained(rng, 3, False, dtype=dtype)
    lens = np.array([1, 2, 4, 8, 16, 64, 2, 4], dtype=np.int64)
    n = int(lens.sum())
    q, _ = bagged(rng, keys, n, 2)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    w = np.repeat(1.0 / lens, lens).astype(np.float32)
    same(a.lookup_pooled_weighted(q, offsets, None, rm.POOL_MEAN)["out"], a.lookup_pooled_weighted(q, offsets, w)["out"])


def test_refusals_change_nothing():
    rng = np.random.default_rng(7)
    a, keys = trained(rng, 3, True)
    a.kb, a.ke = 5, KEND
    b = twin(a)
    g = np.ones(9, np.float32)
    unsorted, high, low = keys[[2, 1, 3]], np.append(keys[:2], np.uint64(KEND)), np.append(keys[:2], np.uint64(4))
    off = np.array([0, 1, 3], np.uint64)
    cases = [a.handle(PP, unsorted, g), a.update(PP, unsorted, g, 0.1, 0), a.assign(unsorted, g),
             a.handle_any(PP, high, g), a.update_any(PP, low, g, 0.1, 0), a.lookup(high), a.erase(low),
             a.update_merged(PP, [keys[:3], high], [g, g], 0.1, 0), a.lookup_pooled(high, off),
             a.lookup_pooled(keys[:3], np.array([1, 2, 3], np.uint64)), a.lookup_pooled(keys[:3], np.array([0, 2, 1, 3], np.uint64)),
             a.update_pooled(keys[:3], np.array([0, 1, 4], np.uint64), g[:6], 0.1, 0),
             a.update_pooled(high, np.array([0, 1, 4], np.uint64), g[:6], 0.1, 0),
             a.update_pooled_merged([(keys[:3], off, g[:6]), (low, None, g)], 0.1, 0), a.export(a.size, 1)]
    codes = [r.code for r in cases]
    assert codes == [1, 1, 1, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1, 4, 1]
    same_state(a, b)
    h = RowModel(F16, 3)
    assert h.update(PP, keys[:3], g, 0.1, 0).code == rm.UNSUPPORTED and h.set_adam(*rm.ADAM).code == rm.UNSUPPORTED


def test_capacity_follows_the_rules_of_growth_and_erase():
    m = RowModel(F32, 3)
    k = np.arange(5000, dtype=np.uint64)
    z = lambda n: np.zeros(n * 3, np.float32)
    m.handle(PUSH, k[:1], z(1))
    assert m.capacity == 1024
    m.handle(PUSH, k[:1025], z(1025))
    assert m.capacity == 2048
    m.handle(PUSH, k[:4600], z(4600))
    assert m.capacity == 4600
    assert m.erase(k[100:])["erased"] == 4500 and m.capacity == 1024 and m.size == 100
    m.clear()
    assert m.capacity == 1024 and m.size == 0
    m.handle(PUSH, k[:10], z(10))
    assert m.erase(k)["erased"] == 10 and m.capacity == 0


# ---- the optimizer step against the reference's own rounds --------------------------------------
LRG = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_ref.npz"))


@pytest.mark.parametrize("call", ["update", "update_any", "update_merged", "update_pooled"])
@pytest.mark.parametrize("case", [str(c) for c in LRG["cases"]])
def test_the_step_against_the_reference_rounds(case, call):
    """The fixture's rounds (the reference's own Adam.h inside LRServer's apply
    loop) replayed on the model as rows of width 1 and, where the length allows,
    7: every round's reply bit for bit."""
    w0 = LRG[f"{case}_w0"]
    lr = float(LRG[f"{case}_lr"][0])
    for width in (1, 7):
        rows = len(w0) // width
        n = rows * width
        m = RowModel(F32, width)
        if bool(LRG[f"{case}_adam"][0]):
            m.set_adam(lr, 0.9, 0.999, 1e-8)
        keys = np.arange(rows, dtype=np.uint64) * np.uint64(7) + np.uint64(3)
        m.assign(keys, w0[:n])
        for r, it in enumerate(LRG[f"{case}_iters"]):
            g = np.ascontiguousarray(LRG[f"{case}_merged"][r][:n])
            if call == "update_merged":
                out = m.update_merged(PP, [keys], [g], lr, int(it))["outs"][0]
            elif call == "update_pooled":  # one bag per id
                m.update_pooled(keys, np.arange(rows + 1, dtype=np.uint64), g, lr, int(it))
                out = m.rows
            else:
                out = getattr(m, call)(PP, keys, g, lr, int(it))["out"]
            np.testing.assert_array_equal(bits(out).ravel(), bits(LRG[f"{case}_out"][r][:n]), err_msg=f"round {r}")


# ---- the sequences of the GPU file, dry ---------------------------------------------------------
def nan_free(dtype, a):
    return a is None or not rm.rs.nan_mask(dtype, np.ascontiguousarray(a)).any()


@pytest.mark.parametrize("name,seed,profile", rm.SEQUENCES, ids=[s[0] for s in rm.SEQUENCES])
def test_sequence_dry_run(name, seed, profile):
    steps = rm.make_sequence(seed, profile)
    again = rm.make_sequence(seed, profile)
    assert len(steps) == len(again)
    for a, b in zip(steps, again):  # the generator is deterministic: every field of every step
        assert a.keys() == b.keys()
        for k in a:
            if k == "frames":
                assert len(a[k]) == len(b[k])
                for fa, fb in zip(a[k], b[k]):
                    assert all((x is None and y is None) or np.array_equal(bits(x), bits(y)) for x, y in zip(fa, fb))
            elif isinstance(a[k], np.ndarray):
                np.testing.assert_array_equal(bits(a[k]), bits(b[k]))
            else:
                assert a[k] == b[k], k
    model, replies, st = rm.replay(profile, steps)
    ev = st["events"]
    at = lambda what: [i for i, e in ev if e == what]
    refused = at("refused")
    share_absent = st["absent"] / st["looked"]
    share_refused = len(refused) / len(steps)
    sizes = [len(s["keys"]) if "keys" in s else sum(len(f[0]) for f in s["frames"]) if "frames" in s else s.get("count", 0)
             for s in steps]
    print(f"{name}: {len(steps)} steps, ops {st['ops']}, absent ids {share_absent:.3f} of {st['looked']}, refusals "
          f"{share_refused:.3f} at {refused}, grow at {at('grow')}, shrink at {at('shrink')}, erase_all at "
          f"{at('erase_all')}, insert into an empty table at {at('insert_into_empty')}, hottest key x{st['hot']}, "
          f"largest request {max(sizes)}, final size {model.size}")
    assert 30 <= len(steps) <= 40
    missing = [op for op in rm.profile_ops(profile) if not st["ops"].get(op)]
    assert not missing, missing
    assert at("grow"), "no step grows a populated table past its capacity"
    assert at("shrink"), "no erase shrinks the table"
    assert at("erase_all") and max(at("insert_into_empty")) > min(at("erase_all")), "no erase of every key with an insert behind it"
    assert 0.10 <= share_absent <= 0.40
    assert st["hot"] >= 8
    assert 0 < share_refused <= 0.15
    for i in refused:  # each refusal is followed by a served step of another operation
        assert i + 1 < len(steps) and i + 1 not in refused and steps[i + 1]["op"] != steps[i]["op"], i
    assert max(sizes) <= 5100
    if profile["kind"] == "wide":  # n <= 300 wherever the cost grows with the width: every call but erase
        assert max(n for n, s in zip(sizes, steps) if s["op"] != "erase") <= 300
    # sizes jump between neighbouring requests
    big = [n for n in sizes if n]
    assert sum(max(a, b) >= 8 * min(a, b) for a, b in zip(big, big[1:])) >= len(big) // 2
    assert any(s["shift"] for s in steps) and not all(s["shift"] for s in steps)
    # free of NaN: the state and every expected reply
    dt = profile["dtype"]
    assert nan_free(dt, model.rows) and not np.isnan(model.m).any() and not np.isnan(model.v).any()
    peak = 0
    m2 = rm.new_model(profile)
    for s, r in zip(steps, replies):
        rm.apply_step(m2, s)
        peak = max(peak, m2.size)
        assert nan_free(dt, m2.rows)
        if isinstance(r, Refused):
            continue
        for k in ("out", "rows"):
            assert nan_free(dt, r.get(k))
        for k in ("m", "v"):  # an export's moments
            assert k not in r or not np.isnan(r[k]).any()
        for o in r.get("outs") or []:
            assert nan_free(F32, o)
    assert peak <= 12000
    same_state(model, m2)  # the replay is deterministic
