#!/usr/bin/env python3
"""The row table's pooled calls (psg_table_lookup_pooled / psg_table_update_pooled)
against the existing calls a caller used in their place — a record, not a test.
Needs an MI355X; prints ONE JSON line and writes it to --out.

F32, W in {8, 32, 128}, n = 1 GiB / (4 W) keys — 1 GiB of rows resident, well past
the 256 MiB Infinity Cache — and two id lists of n occurrences each:

  sorted    the table's keys, ascending
  shuffled  80 % of the occurrences drawn from all keys, 20 % from a hot set of 1 %
            of them, in random order

cut into bags of L in {4, 16, 64} consecutive positions (nb = n / L).  Each time is
event-timed around the whole call, one warm-up call, then the median of --reps:

  lookup_pooled_ms   psg_table_lookup_pooled of the list
  lookup_ms          yardstick psg_table_lookup of the same list (out given, found
                     NULL): the same resolve and the same rows read, 4 W B of reply
                     per id where the pooled call writes 4 W / L
  update_pooled_ms   psg_table_update_pooled on an Adam table, one gradient row per bag
  update_merged_ms   yardstick psg_table_update_merged (k = 1) of the same list on
                     the pre-expanded E[i] = grads[bag(i)]; building E is not timed
  expand_ms          psg_rows_gather of grads by bag_of into E: the expansion the
                     caller no longer pays (a stand-in for however it built E)
  *_over_*           the ratio of the times

Conditions, at W = 32, L = 16:
  F  sorted list:    lookup_pooled_over_lookup        must be <= 1.05
  B  shuffled list:  update_pooled_over_update_merged must be <= 1.05

At that shape the results are also compared: the pooled reply against the f32 sums, in
arrival order, of the yardstick lookup's rows, and the rows of a table that took
update_pooled against those of a twin that took update_merged, bit for bit.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))
import psg  # noqa: E402

KMAX = (1 << 64) - 1
LR = 0.05
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)


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


def measure(fn, reps, stream):
    """one warm-up call, then the median of reps timed ones"""
    fn()
    return median([timed(fn, stream) for _ in range(reps)])


def id_lists(keys, rng):
    n = len(keys)
    hot = rng.choice(keys, max(n // 100, 1), replace=False)
    nhot = n // 5
    shuffled = np.concatenate([keys[rng.integers(0, n, n - nhot)], hot[rng.integers(0, len(hot), nhot)]])
    return {"sorted": keys, "shuffled": rng.permutation(shuffled)}


def new_table(width, n, dk, rows, stream):
    t = psg.Table(psg.F32, width, 0, KMAX, n)
    t.set_adam(*ADAM)
    t.assign(dk, rows, n, None, None, stream)  # the table holds every key before anything is timed
    return t


def check_forward(out_pooled, out_lookup, n, width, bag):
    """the pooled reply == the f32 sums, in arrival order from +0, of the looked-up rows"""
    rows = out_lookup.download(np.float32, n * width).reshape(n // bag, bag, width)
    acc = np.zeros((n // bag, width), dtype=np.float32)
    for j in range(bag):
        acc = acc + rows[:, j, :]
    got = out_pooled.download(np.float32, (n // bag) * width).reshape(n // bag, width)
    return bool(np.array_equal(got.view(np.uint32), acc.view(np.uint32)))


def case(width, n, bags, reps, stream, check_at):
    nvals = n * width
    rng = np.random.default_rng(width)
    keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(977)
    dk = psg.DeviceBuffer.from_numpy(keys)
    rows = psg.DeviceBuffer(nvals * 4)
    rows.fill_synth(nvals, psg.F32, 7, 1, -1.0, 1.0)
    t = new_table(width, n, dk, rows, stream)
    out = psg.DeviceBuffer(nvals * 4)     # the lookup's reply, then E
    pooled = psg.DeviceBuffer(nvals * 4 // min(bags))
    grads = psg.DeviceBuffer(nvals * 4 // min(bags))
    grads.fill_synth(nvals // min(bags), psg.F32, 11, 1, -1.0, 1.0)
    res = []
    for order, q in id_lists(keys, rng).items():
        dq = psg.DeviceBuffer.from_numpy(q)
        lookup_ms = measure(lambda: t.lookup(dq, out, None, n, stream), reps, stream)
        for bag in bags:
            nb = n // bag
            assert nb * bag == n
            r = {"dtype": "f32", "width": width, "keys": n, "table_bytes": nvals * 4, "list": order, "bag": bag,
                 "bags": nb, "lookup_ms": lookup_ms}
            doff = psg.DeviceBuffer.from_numpy(np.arange(nb + 1, dtype=np.uint64) * np.uint64(bag))
            dbag = psg.DeviceBuffer.from_numpy(np.repeat(np.arange(nb, dtype=np.uint32), bag))
            r["lookup_pooled_ms"] = measure(lambda: t.lookup_pooled(dq, doff, pooled, n, nb, stream), reps, stream)
            if (width, bag) == check_at:
                t.lookup(dq, out, None, n, stream)
                r["forward_checked"] = check_forward(pooled, out, n, width, bag)
            # the backward: E into `out`, by the gather that stands in for the caller's expansion
            r["expand_ms"] = measure(lambda: psg.rows_gather(out, grads, dbag, n, width * 4, stream), reps, stream)
            stream.sync()
            it = [0]

            def pooled_step():
                t.update_pooled(dq, doff, grads, n, nb, LR, it[0], stream)
                it[0] += 1

            def merged_step():
                t.update_merged(psg.PUSH, [dq], [out], None, [n], LR, it[0], stream)
                it[0] += 1

            r["update_pooled_ms"] = measure(pooled_step, reps, stream)
            r["update_merged_ms"] = measure(merged_step, reps, stream)
            assert t.info().size == n, "a call inserted rows"
            if (width, bag) == check_at:
                a, b = (new_table(width, n, dk, rows, stream) for _ in range(2))
                a.update_pooled(dq, doff, grads, n, nb, LR, 0, stream)
                b.update_merged(psg.PUSH, [dq], [out], None, [n], LR, 0, stream)
                r["backward_checked"] = bool(np.array_equal(a.dump()[1].view(np.uint32), b.dump()[1].view(np.uint32)))
                a.close()
                b.close()
            r["lookup_pooled_over_lookup"] = r["lookup_pooled_ms"] / r["lookup_ms"]
            r["update_pooled_over_update_merged"] = r["update_pooled_ms"] / r["update_merged_ms"]
            r["expand_over_update_pooled"] = r["expand_ms"] / r["update_pooled_ms"]
            res.append(r)
            print("rows_pooled_bench: case done:", json.dumps(r), file=sys.stderr, flush=True)
            doff.free()
            dbag.free()
        dq.free()
    for b in (dk, rows, out, pooled, grads):
        b.free()
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--bags", default="4,16,64")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_pooled_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_pooled_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    bags = [int(x) for x in a.bags.split(",")]
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        cases += case(w, a.table_bytes // (4 * w), bags, a.reps, stream, (32, 16))

    def at(order):
        hit = [c for c in cases if c["width"] == 32 and c["bag"] == 16 and c["list"] == order]
        return hit[0] if hit else None

    f, b = at("sorted"), at("shuffled")
    line = {"bench": "rows_pooled", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases,
            "F_lookup_pooled_over_lookup": f["lookup_pooled_over_lookup"] if f else None,
            "F_within_1_05": (f["lookup_pooled_over_lookup"] <= 1.05) if f else None,
            "B_update_pooled_over_update_merged": b["update_pooled_over_update_merged"] if b else None,
            "B_within_1_05": (b["update_pooled_over_update_merged"] <= 1.05) if b else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text + "\n")


if __name__ == "__main__":
    main()
