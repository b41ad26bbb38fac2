#!/usr/bin/env python3
"""The row table's order-preserving requests (psg_table_handle_any /
psg_table_update_any) — a record, not a test.  Needs an MI355X; prints ONE JSON
line and writes it to --out.

F32, W in {8, 32, 128}, a table of 1 GiB of rows (n = 1 GiB / (4 W) keys), every
time event-timed around the whole call, median of --reps.  Per width:

  ascending   the full strictly ascending list: handle_any against
              psg_table_handle in the same process, Push and Pull.
              strict_spread is (max - min) / min over three repeated medians of
              the strict call's Push + Pull; ratio = any / strict (Push + Pull).
  shuffled    the full list of distinct keys in a shuffled order: handle_any
              Push + Pull against psg_store_handle on a SORTED store with the
              expanded keys key * W + j in the same shuffled order (its
              order-preserving path: the only way to serve this request without
              the _any calls), widths of --scalar-widths only.
  skewed      as many occurrences as the table has rows, ids drawn Zipf(1.05)
              over the table's rows (hot rows scattered over the key space):
              accumulate Push and PushPull, SGD and Adam PushPull; times,
              algorithmic bytes, the unique keys and the longest segment.

--skew-only W runs only the skewed accumulate and updates of one width (for a
kernel trace in a run of its own); --stats-csv merges the share of time such a
trace's kernel_stats.csv gives the sort (k_rs_*) into the JSON of --out.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))
import psg  # noqa: E402

KMAX = (1 << 64) - 1
LR = 0.05


def median(xs):
    return float(np.median(np.asarray(xs)))


def timed(fn, stream):
    e0, e1 = psg.Event(timing=True), psg.Event(timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.sync()
    ms = e0.elapsed_ms(e1)
    e0.close()
    e1.close()
    return ms


def med(fn, reps, stream):
    fn()  # warm-up
    return median([timed(fn, stream) for _ in range(reps)])


def row_keys(n_table):
    return np.uint64(1) + np.arange(n_table, dtype=np.uint64) * np.uint64(977)


def filled_table(width, n_table, stream, adam=False):
    t = psg.Table(psg.F32, width, 0, KMAX, n_table)
    if adam:
        t.set_adam(0.01)
    full = psg.DeviceBuffer.from_numpy(row_keys(n_table))
    out = psg.DeviceBuffer(n_table * width * 4)
    t.handle(psg.PULL, full, None, out, n_table, stream)  # inserts every key
    full.free()
    out.free()
    return t


def ascending(width, n_table, reps, stream):
    n, nv = n_table, n_table * width
    t = filled_table(width, n_table, stream)
    dk = psg.DeviceBuffer.from_numpy(row_keys(n_table))
    vals, out = psg.DeviceBuffer(nv * 4), psg.DeviceBuffer(nv * 4)
    vals.fill_synth(nv, psg.F32, 7, 0, 0.0, 16.0)
    strict = lambda f: t.handle(f, dk, vals, out, n, stream)  # noqa: E731
    anyo = lambda f: t.handle_any(f, dk, vals, out, n, stream)  # noqa: E731
    sp, sl, ap, al = [], [], [], []
    for _ in range(3):  # interleaved, so drift hits both alike
        sp.append(med(lambda: strict(psg.PUSH), reps, stream))
        ap.append(med(lambda: anyo(psg.PUSH), reps, stream))
        sl.append(med(lambda: strict(psg.PULL), reps, stream))
        al.append(med(lambda: anyo(psg.PULL), reps, stream))
    tot = [a + b for a, b in zip(sp, sl)]
    res = {"strict_push_ms": median(sp), "strict_pull_ms": median(sl), "any_push_ms": median(ap),
           "any_pull_ms": median(al), "strict_medians_push_plus_pull_ms": tot,
           "strict_spread": (max(tot) - min(tot)) / min(tot)}
    res["ratio"] = (res["any_push_ms"] + res["any_pull_ms"]) / (res["strict_push_ms"] + res["strict_pull_ms"])
    t.close()
    for b in (dk, vals, out):
        b.free()
    return res


def shuffled(width, n_table, reps, stream, rng, scalar):
    n, nv = n_table, n_table * width
    keys = rng.permutation(row_keys(n_table))
    t = filled_table(width, n_table, stream)
    dk = psg.DeviceBuffer.from_numpy(keys)
    vals, out = psg.DeviceBuffer(nv * 4), psg.DeviceBuffer(nv * 4)
    vals.fill_synth(nv, psg.F32, 7, 0, 0.0, 16.0)
    res = {"any_push_ms": med(lambda: t.handle_any(psg.PUSH, dk, vals, None, n, stream), reps, stream),
           "any_pull_ms": med(lambda: t.handle_any(psg.PULL, dk, None, out, n, stream), reps, stream),
           # sorted pairs 8 passes x (12 read + 12 written) + key copy 16 + U, seg, slots ~ 24; rows 12 W / 8 W
           "push_bytes": n * (8 * 24 + 40 + 12 * width), "pull_bytes": n * (8 * 24 + 40 + 8 * width)}
    sum_rows = psg.checksum(out, nv * 4, stream)
    t.close()
    if scalar:
        ek = (keys[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)).ravel()
        store = psg.Store(psg.SORTED, psg.F32, 0, KMAX, nv)
        full = psg.DeviceBuffer.from_numpy(np.sort(ek))
        store.handle(psg.PULL, full, None, out, nv, stream=stream)  # inserts every key
        full.free()
        dek = psg.DeviceBuffer.from_numpy(ek)
        del ek
        # the same sequence of requests as the table saw: warm-up and reps Pushes, then the Pulls
        res["scalar_push_ms"] = med(lambda: store.handle(psg.PUSH, dek, vals, None, nv, stream=stream), reps, stream)
        res["scalar_pull_ms"] = med(lambda: store.handle(psg.PULL, dek, None, out, nv, stream=stream), reps, stream)
        res["pull_matches_scalar"] = psg.checksum(out, nv * 4, stream) == sum_rows
        res["scalar_served"] = store.counters()
        res["ratio"] = (res["any_push_ms"] + res["any_pull_ms"]) / (res["scalar_push_ms"] + res["scalar_pull_ms"])
        store.close()
        dek.free()
    for b in (dk, vals, out):
        b.free()
    return res


def zipf_ids(n_table, count, rng, s=1.05):
    """count draws of a rank in [0, n_table) with P(rank k) ~ (k + 1)^-s"""
    cdf = np.cumsum(np.arange(1, n_table + 1, dtype=np.float64) ** -s)
    cdf /= cdf[-1]
    return np.minimum(np.searchsorted(cdf, rng.random(count)), n_table - 1)


def skewed(width, n_table, reps, stream, rng):
    n, nv = n_table, n_table * width
    ids = zipf_ids(n_table, n, rng)
    place = rng.permutation(n_table)  # rank -> row: the hot rows lie scattered
    keys = row_keys(n_table)[place[ids]]
    counts = np.bincount(ids)
    m = int(np.count_nonzero(counts))
    res = {"occurrences": n, "unique_keys": m, "longest_segment": int(counts.max()),
           "top10_share": float(np.sort(counts)[-10:].sum() / n)}
    dk = psg.DeviceBuffer.from_numpy(keys)
    vals, out = psg.DeviceBuffer(nv * 4), psg.DeviceBuffer(nv * 4)
    vals.fill_synth(nv, psg.F32, 7, 1, -1.0, 1.0)
    sort_bytes = n * (8 * 24 + 16) + m * 24
    t = filled_table(width, n_table, stream)
    res["accumulate_push_ms"] = med(lambda: t.handle_any(psg.PUSH, dk, vals, None, n, stream), reps, stream)
    res["accumulate_pushpull_ms"] = med(lambda: t.handle_any(psg.PUSH | psg.PULL, dk, vals, out, n, stream), reps,
                                        stream)
    # rows read and written once per unique key, values read (and replies written) once per occurrence
    res["accumulate_push_bytes"] = sort_bytes + 4 * n + m * 8 * width + n * 4 * width
    res["accumulate_pushpull_bytes"] = res["accumulate_push_bytes"] + n * 4 * width
    t.close()
    for name, adam in (("sgd", False), ("adam", True)):
        t = filled_table(width, n_table, stream, adam)
        res[name + "_pushpull_ms"] = med(
            lambda: t.update_any(psg.PUSH | psg.PULL, dk, vals, out, n, LR, 3, stream), reps, stream)
        res[name + "_pushpull_bytes"] = res["accumulate_pushpull_bytes"] + (m * 32 * width if adam else 0)
        t.close()
    for b in (dk, vals, out):
        b.free()
    return res


def sort_share(path):
    tot = srt = 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            tot += ns
            if "k_rs_" in row["Name"]:
                srt += ns
    return {"kernel_ns": tot, "sort_ns": srt, "sort_share": srt / tot if tot else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--scalar-widths", default="8,32,128")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skew-only", type=int, default=0, metavar="W")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_any_bench.json"))
    a = ap.parse_args()
    if a.stats_csv:
        with open(a.out) as f:
            line = json.loads(f.read())
        line["skew_w32_kernel_trace"] = sort_share(a.stats_csv)
        text = json.dumps(line)
        print(text)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        return
    if psg.device_count() < 1:
        raise SystemExit("rows_any_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    rng = np.random.default_rng(5)
    if a.skew_only:
        print(json.dumps(skewed(a.skew_only, a.table_bytes // (4 * a.skew_only), a.reps, stream, rng)))
        return
    scalar_w = {int(x) for x in a.scalar_widths.split(",") if x}
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        n_table = a.table_bytes // (4 * w)
        c = {"dtype": "f32", "width": w, "table_keys": n_table, "table_bytes": n_table * w * 4}
        c["ascending"] = ascending(w, n_table, a.reps, stream)
        c["shuffled"] = shuffled(w, n_table, a.reps, stream, rng, w in scalar_w)
        c["skewed"] = skewed(w, n_table, a.reps, stream, rng)
        cases.append(c)
        print("rows_any_bench: case done:", json.dumps(c), file=sys.stderr, flush=True)
    w32 = [c for c in cases if c["width"] == 32]
    line = {"bench": "rows_any", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases}
    if w32:
        asc, shf = w32[0]["ascending"], w32[0]["shuffled"]
        bound = max(1.05, 1.0 + asc["strict_spread"])
        line.update(w32_ascending_ratio=asc["ratio"], w32_ascending_bound=bound,
                    w32_ascending_within_bound=asc["ratio"] <= bound, w32_shuffled_ratio=shf.get("ratio"),
                    w32_shuffled_below_one=(shf["ratio"] < 1.0) if "ratio" in shf else None)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
