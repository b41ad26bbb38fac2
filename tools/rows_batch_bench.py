#!/usr/bin/env python3
"""psg_table_lookup_pooled_batch against the T per-table calls it stands for — a
record, not a test.  Needs an MI355X; prints ONE JSON line and writes it to --out.

F32, T in {1, 8, 26, 64} tables of 1 M rows each, W in {16, 64, 128}; every entry has
2048 bags of L in {4, 32} ids, 80 % of them drawn from all of its table's keys and
20 % from a hot set of 1 % of them, in random order.  One more run, T = 8 with
262144 bags of 4 an entry at W = 64, is the shape where bytes and not launches
dominate.  Each time is event-timed around the whole call(s), one warm-up, then the
median of --reps:

  batch_ms      one psg_table_lookup_pooled_batch of the T entries
  per_table_ms  yardstick: T psg_table_lookup_pooled calls, one after the other, in
                the same process
  ratio         batch_ms / per_table_ms

Conditions:
  a  T = 1:   the largest ratio over the T = 1 cases, to hold against 1.05 (and
              against the spread of three runs of this tool)
  b  T = 26, 2048 bags: every ratio below 1; the figure itself is the record

At T = 8, W = 64, L = 4 the batched replies are compared with the yardstick's, bit
for bit.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))
import psg  # noqa: E402
from rows_pooled_bench import measure  # noqa: E402

KMAX = (1 << 64) - 1
ROWS = 1 << 20


def id_list(keys, count, rng):
    hot = rng.choice(keys, len(keys) // 100, replace=False)
    nhot = count // 5
    ids = np.concatenate([keys[rng.integers(0, len(keys), count - nhot)], hot[rng.integers(0, len(hot), nhot)]])
    return rng.permutation(ids)


def case(tables, keys, width, T, nb, bag, reps, stream, rng, check):
    n = nb * bag
    dq = [psg.DeviceBuffer.from_numpy(id_list(keys, n, rng)) for _ in range(T)]
    doff = psg.DeviceBuffer.from_numpy(np.arange(nb + 1, dtype=np.uint64) * np.uint64(bag))
    outs = [psg.DeviceBuffer(nb * width * 4) for _ in range(T)]
    ts = tables[:T]

    def batch():
        status = psg.lookup_pooled_batch(ts, dq, [doff] * T, None, [psg.POOL_SUM] * T, outs, [n] * T, [nb] * T, stream)
        assert not any(status), status

    def per_table():
        for t, q, o in zip(ts, dq, outs):
            t.lookup_pooled(q, doff, o, n, nb, stream)

    r = {"dtype": "f32", "width": width, "tables": T, "bags": nb, "bag": bag, "ids": n}
    r["per_table_ms"] = measure(per_table, reps, stream)
    if check:
        ref = [o.download(np.uint32, nb * width) for o in outs]
        for o in outs:
            o.upload(np.zeros(nb * width, np.uint32))
    r["batch_ms"] = measure(batch, reps, stream)
    if check:
        r["checked"] = all(np.array_equal(o.download(np.uint32, nb * width), x) for o, x in zip(outs, ref))
    r["ratio"] = r["batch_ms"] / r["per_table_ms"]
    print("rows_batch_bench: case done:", json.dumps(r), file=sys.stderr, flush=True)
    for b in dq + outs + [doff]:
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="16,64,128")
    ap.add_argument("--tables", default="1,8,26,64")
    ap.add_argument("--bags", default="4,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_batch_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_batch_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    Ts = [int(x) for x in a.tables.split(",")]
    keys = np.uint64(1) + np.arange(ROWS, dtype=np.uint64) * np.uint64(977)
    dk = psg.DeviceBuffer.from_numpy(keys)
    rng = np.random.default_rng(26)
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        rows = psg.DeviceBuffer(ROWS * w * 4)
        tables = []
        for i in range(max(Ts + [8])):
            rows.fill_synth(ROWS * w, psg.F32, 7 + i, 1, -1.0, 1.0)
            t = psg.Table(psg.F32, w, 0, KMAX, ROWS)
            t.assign(dk, rows, ROWS, None, None, stream)  # every table holds every key before anything is timed
            stream.sync()
            tables.append(t)
        for T in Ts:
            for bag in (int(x) for x in a.bags.split(",")):
                cases.append(case(tables, keys, w, T, 2048, bag, a.reps, stream, rng, (w, T, bag) == (64, 8, 4)))
        if w == 64:
            cases.append(case(tables, keys, w, 8, 262144, 4, a.reps, stream, rng, False))
        for t in tables:
            t.close()
        rows.free()
    one = [c["ratio"] for c in cases if c["tables"] == 1]
    many = [c["ratio"] for c in cases if c["tables"] == 26 and c["bags"] == 2048]
    line = {"bench": "rows_batch", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases,
            "a_T1_largest_ratio": max(one) if one else None,
            "a_within_1_05": (max(one) <= 1.05) if one else None,
            "b_T26_ratios": many, "b_T26_largest_ratio": max(many) if many else None,
            "b_below_1": (max(many) < 1.0) if many else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text + "\n")


if __name__ == "__main__":
    main()
