"""One host model of a row table (psg_table_*, include/psg.h) and a generator of
long mixed request sequences, for test_row_model.py (CPU) and
test_rows_sequences_gpu.py.

The model holds key -> (row in the stored dtype, m[width] f64, v[width] f64) as
three arrays in key order, the key range, the Adam parameters and the capacity
the header's growth and shrink rules give.  Every operation of the table is
restated in numpy with the arithmetic the header states:
  accumulate   one add per occurrence, rounded to the dtype (halves through
               row_specials.np_add), occurrences in arrival order;
  update       oracle.lr_apply, one step per occurrence (update, update_any) or
               one per key on the f32 sum from +0 of its occurrences in arrival
               order (update_merged and, on the expanded rows, the pooled updates);
  pooled read  per bag from +0 in arrival order, one multiply and one add per
               present id in f32 (f64 for F64 tables), one division for a mean,
               one rounding to a half at the end.
Repeats are served in rounds: round r holds the r-th occurrence of every key, so
its rows are distinct and one vector operation serves it; the rounds run in
order, which is arrival order inside every key.  A refused request returns
Refused(code) and changes nothing.  The module never imports psg.

make_sequence(seed, profile) builds a list of step records from the model alone
and apply_step(model, step) replays one, so a sequence is produced and checked
on the host without a GPU.
"""
import numpy as np

import oracle
import row_specials as rs

F32, F64, F16, BF16 = rs.F32, rs.F64, rs.F16, rs.BF16
PUSH, PULL = 1, 2
INVALID, RANGE, UNSUPPORTED = 1, 4, 6  # PSG_ERR_*
SAME_LIST, SORTED = 1, 2  # PSG_MERGED_*
POOL_SUM, POOL_MEAN = 0, 1
KMAX = (1 << 64) - 1
MAX_FRAMES = 16
MIN_CAPACITY = 1024
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
LR = 0.05


class Refused:
    """what a request that is refused returns: the error code; nothing changed"""

    def __init__(self, code):
        self.code = code

    def __repr__(self):
        return f"Refused({self.code})"


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def strictly_ascending(keys):
    return bool(np.all(keys[1:] > keys[:-1]))


def rounds_of(idx):
    """positions grouped by occurrence number: [positions of every row's first
    occurrence, of its second, ...], each in arrival order"""
    n = len(idx)
    if n == 0:
        return []
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    occ = np.empty(n, np.int64)
    occ[order] = np.arange(n) - np.repeat(start, np.diff(np.append(start, n)))
    by_occ = np.argsort(occ, kind="stable")
    cuts = np.flatnonzero(np.diff(occ[by_occ])) + 1
    return np.split(by_occ, cuts)


def offsets_ok(offsets, n):
    """the three rules: starts at 0, never descends, ends at n"""
    return bool(offsets[0] == 0 and np.all(offsets[1:] >= offsets[:-1]) and offsets[-1] == n)


def to_acc(dtype, stored):
    """stored elements -> the pooled lookup's accumulator type (exact)"""
    if dtype == F64:
        return np.asarray(stored, dtype=np.float64)
    if dtype == BF16:
        return (np.asarray(stored, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    if dtype == F16:
        return np.asarray(stored, np.uint16).view(np.float16).astype(np.float32)
    return np.asarray(stored, dtype=np.float32)


def from_acc(dtype, acc):
    """the accumulator -> stored elements: halves round once, to nearest even (finite values)"""
    if dtype in (F32, F64):
        return acc
    if dtype == F16:
        return acc.astype(np.float16).view(np.uint16)
    u = np.ascontiguousarray(acc).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


class RowModel:
    def __init__(self, dtype, width, key_begin=0, key_end=KMAX, capacity=0):
        self.dtype, self.w = dtype, width
        self.kb, self.ke = int(key_begin), int(key_end)
        self.st = rs.STORAGE[dtype]
        self.capacity = int(capacity)
        self.adam = None
        self.clear()

    # ---- state -------------------------------------------------------------------
    @property
    def size(self):
        return len(self.keys)

    def clear(self):
        """every key dropped, rows and moments with them; the capacity stays"""
        self.keys = np.zeros(0, np.uint64)
        self.rows = np.zeros((0, self.w), self.st)
        self.m = np.zeros((0, self.w), np.float64)
        self.v = np.zeros((0, self.w), np.float64)

    def set_adam(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        if self.dtype != F32:
            return Refused(UNSUPPORTED)
        if self.adam is not None or not (0 <= beta1 < 1 and 0 <= beta2 < 1) or eps < 0:
            return Refused(INVALID)
        self.adam = (lr, beta1, beta2, eps)
        self.m[:] = 0  # zero for every row present and for every row inserted later
        self.v[:] = 0
        return {}

    def dump(self):
        return self.keys.copy(), self.rows.copy()

    def dump_moments(self):
        return self.m.copy(), self.v.copy()

    def _out_of_range(self, keys):
        return bool(np.any((keys < np.uint64(self.kb)) | (keys >= np.uint64(self.ke))))

    def _find(self, keys):
        """(lower bound of every key, whether it is present)"""
        p = np.searchsorted(self.keys, keys)
        if self.size == 0:
            return p, np.zeros(len(keys), bool)
        return p, (p < self.size) & (self.keys[np.minimum(p, self.size - 1)] == keys)

    def _insert(self, keys):
        """The list's absent keys inserted once each with a zero row and zero
        moments; growth by max(size + new, 2 * capacity, 1024).  Returns the row
        of every position of the list."""
        u = np.unique(keys)
        new = u[~self._find(u)[1]]
        if len(new):
            if self.size + len(new) > self.capacity:
                self.capacity = max(self.size + len(new), 2 * self.capacity, MIN_CAPACITY)
            at = np.searchsorted(self.keys, new)
            self.keys = np.insert(self.keys, at, new)
            self.rows = np.insert(self.rows, at, np.zeros((len(new), self.w), self.st), axis=0)
            self.m = np.insert(self.m, at, np.zeros((len(new), self.w)), axis=0)
            self.v = np.insert(self.v, at, np.zeros((len(new), self.w)), axis=0)
        return np.searchsorted(self.keys, keys)

    # ---- accumulate ------------------------------------------------------------------
    def _add(self, a, b):
        if self.dtype in (F32, F64):
            return a + b
        return rs.np_add(self.dtype, a, b)

    def _accumulate(self, flags, keys, vals):
        n = len(keys)
        idx = self._insert(keys)
        if not flags & PUSH:
            return {"out": self.rows[idx].copy()}  # every occurrence is answered with the row
        vals = np.ascontiguousarray(vals, dtype=self.st).reshape(n, self.w)
        out = np.empty((n, self.w), self.st) if flags & PULL else None
        for sel in rounds_of(idx):
            rows = self._add(self.rows[idx[sel]], vals[sel])
            assert rows.dtype == self.st
            self.rows[idx[sel]] = rows
            if out is not None:
                out[sel] = rows  # the running row after this occurrence
        return {"out": out}

    def _handle(self, flags, keys, vals, strict):
        if flags not in (1, 2, 3):
            return Refused(INVALID)
        keys = u64(keys)
        if len(keys) == 0:
            return {"out": None}
        if strict and not strictly_ascending(keys):
            return Refused(INVALID)  # a strict call looks at the order before the range
        if self._out_of_range(keys):
            return Refused(RANGE)
        return self._accumulate(flags, keys, vals)

    def handle(self, flags, keys, vals=None):
        return self._handle(flags, keys, vals, True)

    def handle_any(self, flags, keys, vals=None):
        return self._handle(flags, keys, vals, False)

    # ---- the optimizer -------------------------------------------------------------------
    def _step(self, ri, g, lr, iteration):
        """one optimizer step on the distinct rows ri with the gradient rows g"""
        w = np.ascontiguousarray(self.rows[ri]).ravel()
        g = np.ascontiguousarray(g, dtype=np.float32).ravel()
        if self.adam:
            m = np.ascontiguousarray(self.m[ri]).ravel()
            v = np.ascontiguousarray(self.v[ri]).ravel()
            oracle.lr_apply(w, g, lr, m, v, *self.adam, iteration)
            self.m[ri] = m.reshape(-1, self.w)
            self.v[ri] = v.reshape(-1, self.w)
        else:
            oracle.lr_apply(w, g, lr, None, None, iteration=iteration)
        w = w.reshape(-1, self.w)
        self.rows[ri] = w
        return w

    def _opt_refusal(self, flags, iteration):
        if flags not in (PUSH, PUSH | PULL) or iteration < 0:
            return Refused(INVALID)
        if self.dtype != F32:
            return Refused(UNSUPPORTED)
        return None

    def _update(self, flags, keys, grads, lr, iteration, strict):
        bad = self._opt_refusal(flags, iteration)
        if bad:
            return bad
        keys = u64(keys)
        n = len(keys)
        if n == 0:
            return {"out": None}
        if strict and not strictly_ascending(keys):
            return Refused(INVALID)
        if self._out_of_range(keys):
            return Refused(RANGE)
        grads = np.ascontiguousarray(grads, dtype=np.float32).reshape(n, self.w)
        idx = self._insert(keys)
        out = np.empty((n, self.w), np.float32) if flags & PULL else None
        for sel in rounds_of(idx):  # one step per occurrence, all with the request's iteration
            rows = self._step(idx[sel], grads[sel], lr, iteration)
            if out is not None:
                out[sel] = rows
        return {"out": out}

    def update(self, flags, keys, grads, lr, iteration):
        return self._update(flags, keys, grads, lr, iteration, True)

    def update_any(self, flags, keys, grads, lr, iteration):
        return self._update(flags, keys, grads, lr, iteration, False)

    def _merge(self, keys, E, lr, iteration):
        """The round on the concatenated keys and their gradient rows E: per key
        the f32 sum from +0 in arrival order, one step per key.  Returns the
        final row of every occurrence."""
        idx = self._insert(keys)
        touched, inv = np.unique(idx, return_inverse=True)
        s = np.zeros((len(touched), self.w), np.float32)
        for sel in rounds_of(idx):
            s[inv[sel]] = s[inv[sel]] + E[sel]
        self._step(touched, s, lr, iteration)
        return self.rows[idx].copy()

    def update_merged(self, flags, keys_list, grads_list, lr, iteration):
        k = len(keys_list)
        if not 1 <= k <= MAX_FRAMES:
            return Refused(INVALID)
        bad = self._opt_refusal(flags, iteration)
        if bad:
            return bad
        keys_list = [u64(x) for x in keys_list]
        ns = [len(x) for x in keys_list]
        if sum(ns) == 0:
            return {"outs": [None] * k, "path": 0}
        keys = np.concatenate(keys_list)
        if self._out_of_range(keys):
            return Refused(RANGE)
        same = all(n == ns[0] for n in ns) and strictly_ascending(keys_list[0]) and \
            all(np.array_equal(x, keys_list[0]) for x in keys_list[1:])
        E = np.concatenate([np.ascontiguousarray(g, dtype=np.float32).reshape(n, self.w)
                            for g, n in zip(grads_list, ns)])
        rows = self._merge(keys, E, lr, iteration)
        outs = np.split(rows, np.cumsum(ns)[:-1]) if flags & PULL else [None] * k
        return {"outs": outs, "path": SAME_LIST if same else SORTED}

    # ---- the calls that never insert ---------------------------------------------------------
    def lookup(self, keys):
        keys = u64(keys)
        if len(keys) == 0:
            return {"out": None, "found": None}
        if self._out_of_range(keys):
            return Refused(RANGE)
        p, found = self._find(keys)
        out = np.zeros((len(keys), self.w), self.st)
        out[found] = self.rows[p[found]]
        return {"out": out, "found": found.astype(np.uint8)}

    def erase(self, keys):
        keys = u64(keys)
        if len(keys) == 0:
            return {"erased": 0}
        if self._out_of_range(keys):
            return Refused(RANGE)
        p, found = self._find(keys)
        dead = np.zeros(self.size, bool)
        dead[p[found]] = True
        erased = int(dead.sum())
        if erased:
            keep = ~dead
            self.keys, self.rows, self.m, self.v = self.keys[keep], self.rows[keep], self.m[keep], self.v[keep]
            self.capacity = max(self.size, MIN_CAPACITY) if self.size else 0  # memory follows the rows
        return {"erased": erased}

    def assign(self, keys, rows=None, m=None, v=None):
        if (m is None) != (v is None) or (m is not None and self.adam is None):
            return Refused(INVALID)
        keys = u64(keys)
        n = len(keys)
        if n == 0:
            return {}
        if rows is None and m is not None:
            return Refused(INVALID)
        if not strictly_ascending(keys):
            return Refused(INVALID)
        if self._out_of_range(keys):
            return Refused(RANGE)
        idx = self._insert(keys)
        if rows is not None:
            self.rows[idx] = np.ascontiguousarray(rows, dtype=self.st).reshape(n, self.w)  # as bytes
        if m is not None:
            self.m[idx] = np.asarray(m, np.float64).reshape(n, self.w)
            self.v[idx] = np.asarray(v, np.float64).reshape(n, self.w)
        return {}

    def export(self, first, count):
        if first > self.size or count > self.size - first:
            return Refused(INVALID)
        s = slice(first, first + count)
        r = {"keys": self.keys[s].copy(), "rows": self.rows[s].copy()}
        if self.adam:
            r["m"], r["v"] = self.m[s].copy(), self.v[s].copy()
        return r

    # ---- pooled ----------------------------------------------------------------------
    def _pooled_refusal(self, keys, offsets):
        """bad offsets -> INVALID, a key out of range -> RANGE, both -> INVALID"""
        if not offsets_ok(offsets, len(keys)):
            return Refused(INVALID)
        if self._out_of_range(keys):
            return Refused(RANGE)
        return None

    def lookup_pooled_weighted(self, keys, offsets, weights=None, mode=POOL_SUM):
        if mode not in (POOL_SUM, POOL_MEAN) or (mode == POOL_MEAN and weights is not None):
            return Refused(INVALID)
        keys, offsets = u64(keys), u64(offsets)
        nb = len(offsets) - 1
        if nb == 0:
            return Refused(INVALID) if len(keys) else {"out": None}
        bad = self._pooled_refusal(keys, offsets)
        if bad:
            return bad
        acc_t = np.float64 if self.dtype == F64 else np.float32
        p, found = self._find(keys)
        lens = np.diff(offsets).astype(np.int64)
        start = offsets[:-1].astype(np.int64)
        acc = np.zeros((nb, self.w), acc_t)  # +0
        for j in range(int(lens.max())):  # round j: position j of every bag that has one
            b = np.flatnonzero(lens > j)
            pos = start[b] + j
            b, pos = b[found[pos]], pos[found[pos]]  # an absent id adds nothing
            r = to_acc(self.dtype, self.rows[p[pos]])
            if weights is not None:
                r = np.asarray(weights, np.float32)[pos].astype(acc_t)[:, None] * r  # ONE multiply
                assert r.dtype == acc_t
            acc[b] = acc[b] + r  # ONE add
        if mode == POOL_MEAN:
            nz = lens > 0  # an empty bag divides nothing
            acc[nz] = acc[nz] / lens[nz].astype(np.uint32).astype(acc_t)[:, None]
        assert acc.dtype == acc_t
        return {"out": np.ascontiguousarray(from_acc(self.dtype, acc))}

    def lookup_pooled(self, keys, offsets):
        return self.lookup_pooled_weighted(keys, offsets)

    def expand(self, offsets, grads, weights=None, mode=POOL_SUM):
        """E of include/psg.h: the gradient row every position of the list receives"""
        lens = np.diff(u64(offsets)).astype(np.int64)
        bag_of = np.repeat(np.arange(len(lens)), lens)
        g = np.ascontiguousarray(grads, dtype=np.float32).reshape(len(lens), self.w)[bag_of]
        if weights is not None:
            g = np.asarray(weights, np.float32)[:, None] * g  # one f32 multiply
        elif mode == POOL_MEAN:
            g = g / lens[bag_of].astype(np.float32)[:, None]  # one f32 division
        assert g.dtype == np.float32
        return g

    def update_pooled_weighted(self, keys, offsets, grads, lr, iteration, weights=None, mode=POOL_SUM):
        if mode not in (POOL_SUM, POOL_MEAN) or (mode == POOL_MEAN and weights is not None) or iteration < 0:
            return Refused(INVALID)
        if self.dtype != F32:
            return Refused(UNSUPPORTED)
        keys, offsets = u64(keys), u64(offsets)
        if len(offsets) - 1 == 0:
            return Refused(INVALID) if len(keys) else {"path": 0}
        bad = self._pooled_refusal(keys, offsets)
        if bad:
            return bad
        if len(keys) == 0:
            return {"path": 0}  # every bag is empty: no gradient row is read
        self._merge(keys, self.expand(offsets, grads, weights, mode), lr, iteration)
        return {"path": SAME_LIST if strictly_ascending(keys) else SORTED}

    def update_pooled(self, keys, offsets, grads, lr, iteration):
        return self.update_pooled_weighted(keys, offsets, grads, lr, iteration)

    def update_pooled_merged(self, frames, lr, iteration):
        """frames: (keys, offsets or None, grads); a plain frame has one gradient row per key"""
        k = len(frames)
        if not 1 <= k <= MAX_FRAMES or iteration < 0:
            return Refused(INVALID)
        if self.dtype != F32:
            return Refused(UNSUPPORTED)
        frames = [(u64(q), None if o is None else u64(o), g) for q, o, g in frames]
        for q, o, _ in frames:
            if o is not None and len(o) - 1 == 0 and len(q):
                return Refused(INVALID)
        if all(o is None for _, o, _ in frames):
            r = self.update_merged(PUSH, [q for q, _, _ in frames], [g for _, _, g in frames], lr, iteration)
            return r if isinstance(r, Refused) else {"path": r["path"]}
        if k == 1:
            return self.update_pooled(frames[0][0], frames[0][1], frames[0][2], lr, iteration)
        keys = np.concatenate([q for q, _, _ in frames])
        if any(o is not None and len(o) > 1 and not offsets_ok(o, len(q)) for q, o, _ in frames):
            return Refused(INVALID)
        if self._out_of_range(keys):
            return Refused(RANGE)
        if len(keys) == 0:
            return {"path": 0}
        E = np.concatenate([np.ascontiguousarray(g, dtype=np.float32).reshape(len(q), self.w) if o is None
                            else self.expand(o, g) for q, o, g in frames if len(q)])
        self._merge(keys, E, lr, iteration)
        return {"path": SORTED}


# ---- a step record and its replay -----------------------------------------------------------
INSERTING = ("handle", "handle_any", "update", "update_any", "update_merged", "assign", "update_pooled",
             "update_pooled_weighted", "update_pooled_merged")
READING = ("lookup", "lookup_pooled", "lookup_pooled_weighted", "export")
ANY_ORDER = ("handle_any", "update_any")
POOLED = ("lookup_pooled", "lookup_pooled_weighted", "update_pooled", "update_pooled_weighted", "update_pooled_merged")


def step(op, **kw):
    """One request as data: op and, as the op needs them, keys, vals (values,
    gradients or rows), offsets, weights, mode, flags, lr, iteration, frames (a
    list of (keys, offsets or None, grads)), m, v, first, count, adam.  shift:
    1 puts every request array one element off its buffer's 16-B alignment."""
    s = {"op": op, "shift": 0, "mode": POOL_SUM, "weights": None, "lr": LR, "iteration": 0}
    s.update(kw)
    return s


def op_name(s):
    """the operation with the variant that picks another kernel"""
    if s["op"] in ("lookup_pooled_weighted", "update_pooled_weighted"):
        return s["op"] + (":mean" if s["mode"] == POOL_MEAN else ":weights")
    return s["op"]


def apply_step(model, s):
    op = s["op"]
    if op in ("handle", "handle_any"):
        return getattr(model, op)(s["flags"], s["keys"], s.get("vals"))
    if op in ("update", "update_any"):
        return getattr(model, op)(s["flags"], s["keys"], s["vals"], s["lr"], s["iteration"])
    if op == "update_merged":
        return model.update_merged(s["flags"], [f[0] for f in s["frames"]], [f[2] for f in s["frames"]], s["lr"],
                                   s["iteration"])
    if op == "lookup":
        return model.lookup(s["keys"])
    if op == "erase":
        return model.erase(s["keys"])
    if op == "assign":
        return model.assign(s["keys"], s.get("vals"), s.get("m"), s.get("v"))
    if op == "export":
        return model.export(s["first"], s["count"])
    if op == "clear":
        model.clear()
        return {}
    if op == "set_adam":
        return model.set_adam(*s["adam"])
    if op == "lookup_pooled":
        return model.lookup_pooled(s["keys"], s["offsets"])
    if op == "lookup_pooled_weighted":
        return model.lookup_pooled_weighted(s["keys"], s["offsets"], s["weights"], s["mode"])
    if op == "update_pooled":
        return model.update_pooled(s["keys"], s["offsets"], s["vals"], s["lr"], s["iteration"])
    if op == "update_pooled_weighted":
        return model.update_pooled_weighted(s["keys"], s["offsets"], s["vals"], s["lr"], s["iteration"], s["weights"],
                                            s["mode"])
    if op == "update_pooled_merged":
        return model.update_pooled_merged(s["frames"], s["lr"], s["iteration"])
    raise ValueError(op)


def new_model(profile):
    return RowModel(profile["dtype"], profile["width"], profile.get("key_begin", 0), profile.get("key_end", KMAX),
                    profile.get("capacity", 0))


def replay(profile, steps):
    """The sequence on a fresh model: (model, replies, statistics).  The
    statistics are what a sequence must show for its GPU run to mean something:
    the served steps per operation, the ids looked up or pooled and how many of
    them were absent, the largest count of one key in an any-order step, and the
    events (step, what): refused, grow (a populated table outgrew its capacity),
    shrink (an erase left a smaller capacity), erase_all, insert_into_empty."""
    model = new_model(profile)
    replies, ops, events = [], {}, []
    looked, absent, hot = 0, 0, 0
    for i, s in enumerate(steps):
        cap, size = model.capacity, model.size
        ids = [f[0] for f in s["frames"]] if "frames" in s else [s["keys"]] if "keys" in s else []
        ids = np.concatenate([u64(x) for x in ids]) if ids else np.zeros(0, np.uint64)
        was_absent = int((~model._find(ids)[1]).sum())
        r = apply_step(model, s)
        replies.append(r)
        if isinstance(r, Refused):
            events.append((i, "refused"))
            assert model.capacity == cap and model.size == size
            continue
        ops[op_name(s)] = ops.get(op_name(s), 0) + 1
        if s["op"] == "lookup" or (s["op"] in POOLED and "frames" not in s):
            looked += len(ids)
            absent += was_absent
        if model.capacity > cap and size > 0:
            events.append((i, "grow"))
        if s["op"] == "erase" and model.capacity < cap:
            events.append((i, "shrink"))
        if s["op"] == "erase" and size and model.size == 0:
            events.append((i, "erase_all"))
        if s["op"] in INSERTING and size == 0 and model.size:
            events.append((i, "insert_into_empty"))
        if s["op"] in ANY_ORDER and len(ids):
            hot = max(hot, int(np.unique(ids, return_counts=True)[1].max()))
    return model, replies, {"ops": ops, "events": events, "hot": hot, "looked": looked, "absent": absent}


# ---- the sequence generator -------------------------------------------------------------------
SIZES = (1, 3, 65, 1023, 1024, 1025, 4097, 5003)
WIDE_SIZES = (1, 3, 65, 255, 256, 257, 300)
TRAIN_OPS = ("handle", "handle_any", "update", "update_any", "update_merged", "lookup", "assign", "export",
             "lookup_pooled", "lookup_pooled_weighted:weights", "lookup_pooled_weighted:mean", "update_pooled",
             "update_pooled_weighted:weights", "update_pooled_weighted:mean", "update_pooled_merged")
ACCUMULATE_OPS = ("handle", "handle_any", "lookup", "assign", "export", "lookup_pooled",
                  "lookup_pooled_weighted:weights", "lookup_pooled_weighted:mean")


def profile_ops(profile):
    """every operation a sequence of the profile must serve at least once"""
    core = ACCUMULATE_OPS if profile["kind"] == "accumulate" else TRAIN_OPS
    return core + ("erase", "clear") + (("set_adam",) if profile.get("adam") else ())


def values(rng, dtype, count):
    """finite elements in [-1, 1] as the table stores them: small enough that an F16 row stays finite"""
    x = rng.uniform(-1, 1, count).astype(np.float32)
    if dtype == F32:
        return x
    if dtype == F64:
        return rng.uniform(-1, 1, count)
    if dtype == F16:
        return x.astype(np.float16).view(np.uint16)
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)  # BF16: the upper half of an f32


def grads(rng, count):
    return rng.uniform(-1, 1, count).astype(np.float32)


class Generator:
    """Builds the steps of one sequence against a model that follows it."""

    def __init__(self, seed, profile):
        self.rng = rng = np.random.default_rng(seed)
        self.profile = profile
        self.model = new_model(profile)
        self.w, self.dtype = profile["width"], profile["dtype"]
        kb, ke = self.model.kb, self.model.ke
        wide = profile["kind"] == "wide"
        self.sizes = WIDE_SIZES if wide else SIZES
        nuni = 2400 if wide else 5600
        u = np.unique(np.concatenate([rng.integers(kb, ke, nuni + 1500 + 64, dtype=np.uint64), u64([kb, ke - 1])]))
        u = rng.permutation(u)
        self.never = np.sort(u[:1500])  # ids no step inserts: what the reading calls find absent
        self.universe = np.sort(np.concatenate([u[1500:1500 + nuni - 2], u64([kb, ke - 1])]))
        self.universe = np.unique(self.universe)
        self.never = np.setdiff1d(self.never, self.universe)
        self.iteration = 0
        self.prev_n = 1

    # ---- values ---------------------------------------------------------------------------
    def values(self, count):
        return values(self.rng, self.dtype, count)

    def grads(self, count):
        return grads(self.rng, count)

    # ---- sizes and keys -------------------------------------------------------------------
    def next_n(self):
        """a request size at least 8 times larger or smaller than the one before"""
        ok = [n for n in self.sizes if max(n, self.prev_n) >= 8 * min(n, self.prev_n)]
        if self.prev_n == 0:  # a fill: the largest sizes
            ok = self.sizes[-3:]
        self.prev_n = int(self.rng.choice(ok))
        return self.prev_n

    def draw(self, n, share_absent, distinct, inserting):
        """n ids, about share_absent of them absent: from the universe for a call
        that inserts, from the ids no step inserts for one that does not"""
        rng, present = self.rng, self.model.keys
        pool = np.setdiff1d(self.universe, present) if inserting else self.never
        na = int(rng.binomial(n, share_absent)) if len(present) else n
        if len(pool) == 0:
            na = 0
        if distinct == "prefer":  # a list that may come in any order ascends only where the share allows it
            distinct = na <= len(pool) and n - na <= len(present)
        if distinct:
            na = max(min(na, len(pool)), n - len(present))
            q = np.concatenate([rng.choice(pool, na, replace=False), rng.choice(present, n - na, replace=False)])
            return np.sort(q)
        few = max(1, min(len(pool), na if share_absent >= 1 else na // 2 + 1))  # absent ids repeat too: inserted once each
        q = np.concatenate([rng.choice(rng.choice(pool, few, replace=False), na) if na else u64([]),
                            rng.choice(present, n - na) if n > na else u64([])])
        q = rng.permutation(u64(q))
        if n >= 65:  # one key 8 to 12 times
            q[rng.choice(n, int(rng.integers(8, 13)), replace=False)] = q[0]
        return u64(q)

    def bags(self, n):
        """offsets of about n / 3 bags over n positions: empty bags first, inside and last, one long bag"""
        sizes = [0]
        if n >= 65:
            sizes.append(min(n // 4, 300))
        while sum(sizes) < n:
            sizes.append(min(int(self.rng.integers(0, 7)), n - sum(sizes)))
        sizes.append(0)
        return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)

    def frames_of(self, n, pooled):
        """2 to 4 frames over about n occurrences; one in three rounds carries the
        same ascending list in every frame (plain frames only)"""
        rng = self.rng
        k = int(rng.integers(2, 5)) if n >= 3 else 1
        if not pooled and rng.integers(3) == 0:
            q = self.draw(max(1, n // k), 0.3, True, True)
            return [(q, None, self.grads(len(q) * self.w)) for _ in range(k)]
        q = self.draw(n, 0.3, False, True)
        parts = np.array_split(q, k)
        if k > 2:
            parts[1] = parts[1][:0]  # an empty frame
        out = []
        for j, part in enumerate(parts):
            if pooled and j % 2 == 0 and len(part):
                o = self.bags(len(part))
                out.append((u64(part), o, self.grads((len(o) - 1) * self.w)))
            else:
                out.append((u64(part), None, self.grads(len(part) * self.w)))
        return out

    # ---- one served step ----------------------------------------------------------------------
    def served(self, name, share=0.3):
        """share: the share of absent ids in a request that inserts"""
        rng, w = self.rng, self.w
        op, _, variant = name.partition(":")
        shift = int(rng.integers(3) == 0)
        it = self.iteration
        if op in ("clear",):
            return step(op)
        if op == "set_adam":
            return step(op, adam=ADAM)
        if op == "export":
            first = int(rng.integers(0, self.model.size))
            return step(op, first=first, count=int(rng.integers(1, min(self.model.size - first, self.sizes[-1]) + 1)),
                        shift=shift)
        n = self.next_n()
        if op in ("handle", "handle_any"):
            flags = int(rng.choice([PUSH, PUSH | PULL, PUSH | PULL, PULL]))
            q = self.draw(n, share, op == "handle", True)
            return step(op, flags=flags, keys=q, vals=self.values(len(q) * w) if flags & PUSH else None, shift=shift)
        if op in ("update", "update_any"):
            self.iteration += 1
            q = self.draw(n, share, op == "update", True)
            return step(op, flags=int(rng.choice([PUSH, PUSH | PULL])), keys=q, vals=self.grads(len(q) * w),
                        iteration=it, shift=shift)
        if op == "update_merged":
            self.iteration += 1
            return step(op, flags=int(rng.choice([PUSH, PUSH | PULL])), frames=self.frames_of(n, False), iteration=it,
                        shift=shift)
        if op == "update_pooled_merged":
            self.iteration += 1
            return step(op, frames=self.frames_of(n, True), iteration=it, shift=shift)
        if op == "assign":
            q = self.draw(n, 0.3, True, True)
            s = step(op, keys=q, vals=self.values(len(q) * w), shift=shift)
            if self.model.adam and rng.integers(2):
                s["m"] = rng.uniform(-0.1, 0.1, len(q) * w)
                s["v"] = rng.uniform(0, 0.01, len(q) * w)  # a second moment is never negative
            return s
        if op == "lookup":
            return step(op, keys=self.draw(n, 0.25, False, False), shift=shift)
        if op == "erase":
            raise ValueError("erase steps are built by erase_some / erase_all")
        inserting = op.startswith("update")
        ascending = rng.integers(4) == 0  # the strict path of the pooled update
        q = self.draw(n, 0.25, "prefer" if ascending else False, inserting)
        s = step(op, keys=q, offsets=self.bags(len(q)), shift=shift)
        if variant == "weights":
            s["weights"] = rng.uniform(-2, 2, len(q)).astype(np.float32)
        if variant == "mean":
            s["mode"] = POOL_MEAN
        if inserting:
            self.iteration += 1
            s["vals"], s["iteration"] = self.grads((len(s["offsets"]) - 1) * w), it
        return s

    def erase_some(self):
        """about 60 % of the rows, ids that are absent and repeats among them: the table shrinks"""
        rng, present = self.rng, self.model.keys
        q = np.concatenate([rng.choice(present, int(0.6 * len(present)), replace=False), rng.choice(self.never, 40),
                            rng.choice(present, 25)])
        return step("erase", keys=u64(rng.permutation(q)), shift=int(rng.integers(2)))

    def erase_all(self):
        return step("erase", keys=u64(self.rng.permutation(self.model.keys)))

    # ---- one refused step ---------------------------------------------------------------------
    def refused(self, kind, not_op):
        """A request the table must refuse, of an operation other than not_op;
        its bad element sits near the end of an otherwise good list."""
        rng, w, prof = self.rng, self.w, self.profile
        train = prof["kind"] != "accumulate"
        n = int(rng.choice([65, 1025] if self.sizes is SIZES else [65, 257]))
        strict = [o for o in (["handle", "assign"] + (["update"] if train else [])) if o != not_op]
        loose = [o for o in (["handle_any", "lookup", "erase"] + (["update_any"] if train else [])) if o != not_op]
        pooled = [o for o in (["lookup_pooled", "lookup_pooled_weighted"] + (["update_pooled"] if train else []))
                  if o != not_op]
        if kind == "below_begin" and self.model.kb == 0:
            kind = "key_end"
        if kind == "unsorted":
            op = str(rng.choice(strict))
            q = self.draw(n, 0.3, True, True)
            q[[n - 2, n - 1]] = q[[n - 1, n - 2]]
        else:
            op = str(rng.choice(pooled if kind.startswith("offsets") else loose))
            q = self.draw(n, 0.3, False, op not in ("lookup", "erase", "lookup_pooled", "lookup_pooled_weighted"))
            if kind == "key_end":
                q[n - 1] = np.uint64(self.model.ke)
            elif kind == "below_begin":
                q[n - 2] = np.uint64(self.model.kb - 1)
        s = step(op, keys=u64(q), flags=PUSH | PULL, iteration=self.iteration)
        if op in ("handle", "handle_any", "assign"):
            s["vals"] = self.values(n * w)
        if op in ("update", "update_any"):
            s["vals"] = self.grads(n * w)
        if op in POOLED:
            o = self.bags(n)
            if kind == "offsets_start":
                o[0] = 1
            elif kind == "offsets_descend":
                o[len(o) // 2] = o[len(o) // 2 + 1] + np.uint64(1)
            elif kind == "offsets_end":
                o[-1] = n + 1
            s["offsets"] = o
            if op == "lookup_pooled_weighted":
                s["weights"] = rng.uniform(-2, 2, n).astype(np.float32)
            if op == "update_pooled":
                s["vals"] = self.grads((len(o) - 1) * w)
        return s


REFUSALS = ("unsorted", "key_end", "below_begin", "offsets_start", "offsets_descend", "offsets_end")


def make_sequence(seed, profile):
    """30 to 40 steps for the profile, built from the model alone.

    The plan: every operation of the profile at least once in shuffled order;
    an erase of most rows after a third of the steps (the table shrinks), an
    erase of every key after half of them and a clear near the end, each
    followed by steps that insert again; four refusals spread over the
    sequence, each in front of a served step of another operation.  A reading
    step never meets a table of fewer than 64 rows: an any-order request fills
    the table first.  Sizes jump by a factor of 8 or more between neighbours."""
    g = Generator(seed, profile)
    rng, model = g.rng, g.model
    accumulate = profile["kind"] == "accumulate"
    core = list(ACCUMULATE_OPS if accumulate else TRAIN_OPS)
    body = list(rng.permutation(core)) + list(rng.permutation(core))[:len(core) if accumulate else
                                                                     4 if profile["kind"] == "wide" else 10]
    if accumulate:
        body += list(rng.permutation(core))[:6]
    body = [str(x) for x in body]
    body.insert(len(body) // 3, "erase_some")
    body.insert(len(body) // 2 + 1, "erase_all")
    body.insert(len(body) - 4, "clear")
    if profile.get("adam"):
        body.insert(int(rng.integers(0, 3)), "set_adam")  # on the new table, or on a populated one
    slots = set(int(x) for x in (len(body) * np.array([0.2, 0.45, 0.7, 0.9])).astype(int))
    kinds = list(rng.permutation(REFUSALS))
    fill = "handle_any" if accumulate else "update_any"
    steps = []

    def emit(s):
        r = apply_step(model, s)
        steps.append(s)
        return r

    for i, name in enumerate(body):
        needs_rows = name.partition(":")[0] in READING + POOLED or name in ("erase_some", "erase_all")
        if needs_rows and model.size < 64:
            g.prev_n = 0  # a large request
            s = g.served(fill)
            assert not isinstance(emit(s), Refused)
        while name == "erase_some" and model.capacity <= MIN_CAPACITY:  # a populated table outgrows its capacity first
            g.prev_n = 0
            assert not isinstance(emit(g.served(fill, 1.0)), Refused)
        if name == "erase_all" and model.size > g.sizes[-1]:  # one request names at most about 5000 ids
            emit(g.erase_some())
        if i in slots:
            s = g.refused(str(kinds.pop()), name.partition(":")[0].replace("erase_some", "erase").replace("erase_all", "erase"))
            assert isinstance(emit(s), Refused), (s["op"], i)
        s = g.erase_some() if name == "erase_some" else g.erase_all() if name == "erase_all" else g.served(name)
        r = emit(s)
        assert not isinstance(r, Refused), (name, r)
    return steps


# ---- the sequences both test files use ---------------------------------------------------------
def _profiles():
    out = []
    for adam in (False, True):
        for w in (3, 4, 20):
            out.append((f"train-{'adam' if adam else 'sgd'}-w{w}", dict(kind="train", dtype=F32, width=w, adam=adam)))
    out.append(("train-adam-w4-cap1500", dict(kind="train", dtype=F32, width=4, adam=True, capacity=1500)))
    # 42 significant key bits: six passes of the any-order sort
    out.append(("train-sgd-w3-begin", dict(kind="train", dtype=F32, width=3, adam=False, key_begin=(1 << 40) + 12345,
                                           key_end=(1 << 41) + 7)))
    out.append(("wide-adam-w260", dict(kind="wide", dtype=F32, width=260, adam=True)))
    for name, dt in (("f64", F64), ("f16", F16), ("bf16", BF16)):
        for w in (3, 8):
            out.append((f"accumulate-{name}-w{w}", dict(kind="accumulate", dtype=dt, width=w)))
    return out


SEQUENCES = [(name, 100 + i, prof) for i, (name, prof) in enumerate(_profiles())]
