#!/usr/bin/env python3
"""The row table's weighted and mean pooled calls (psg_table_lookup_pooled_weighted /
psg_table_update_pooled_weighted) against the unweighted pooled calls on the same list
in the same process — a record, not a test.  Needs an MI355X; prints ONE JSON line
and writes it to --out.

F32, W in {8, 32, 128}, n = 1 GiB / (4 W) keys — 1 GiB of rows resident, well past
the 256 MiB Infinity Cache — and the two id lists of tools/rows_pooled_bench.py:

  sorted    the table's keys, ascending
  shuffled  80 % of the occurrences drawn from all keys, 20 % from a hot set of 1 %
            of them, in random order

cut into bags of L in {4, 16, 64} consecutive positions (nb = n / L).  Each time is
event-timed around the whole call, one warm-up call, then the median of --reps:

  lookup_pooled_ms    yardstick psg_table_lookup_pooled of the list
  lookup_weighted_ms  psg_table_lookup_pooled_weighted, PSG_POOL_SUM with n weights
  lookup_mean_ms      psg_table_lookup_pooled_weighted, PSG_POOL_MEAN
  update_pooled_ms    yardstick psg_table_update_pooled on an Adam table
  update_weighted_ms  psg_table_update_pooled_weighted, PSG_POOL_SUM with n weights
  update_mean_ms      psg_table_update_pooled_weighted, PSG_POOL_MEAN
  *_over_*            the ratio of the times
  *_model             the ratio of the bytes-per-id models below

The yardsticks are the unweighted calls, whose code the weighted calls do not touch.

Bytes per id (F32, Adam, bag length L, u = unique ids / n, P = the sort's passes):
  forward   16 + 4 W + (4 W + 16) / L; the weights add 4
  backward, a strictly ascending list:
            8/L check + 12 resolve + 8 bag_of + 4 count + 4 slot + 4 W / L gradient
            + 40 W row and moments; the weights add 4 (read beside bag_of)
  backward, any other list:
            8/L check + 12 resolve + 16 copy + 4 bag_of + 32 P sort + 16 run heads
            + 30 u unique list, seg and slots + 4 bags + 4 W gradient + 40 W u row and
            moments; the weights add 20: the gather behind the sort reads perm 4,
            bag_of 4 and weights 4 and writes 8, the walk reads the weight 4, and the
            sort's first pass generates its positions instead of reading 4
  a mean adds nothing to either: the length is two offsets the bag's lanes share.

Conditions, at W = 32, L = 16 (the shapes of conditions F and B of the unweighted
calls), each bound the model's ratio times 1.05:
  FW  sorted list:    lookup_weighted_over_lookup_pooled
  FM  sorted list:    lookup_mean_over_lookup_pooled       (model ratio 1)
  BW  shuffled list:  update_weighted_over_update_pooled
  BM  shuffled list:  update_mean_over_update_pooled       (model ratio 1)

At that shape the results are also compared: the weighted reply against the f32 mirror
(one multiply, one add per id, in arrival order from +0) of the yardstick lookup's rows,
the mean against the mirror's sum over L, and the rows of a table that took
update_pooled_weighted against those of a twin that took update_merged on the
host-built E, bit for bit.
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
SORT_PASSES = 8  # key_end = 2^64 - 1: 64 bits, 8 bits a pass
LR = 0.05
ADAM = (float(np.float32(0.01)), 0.9, 0.999, 1e-8)
SPREAD = 1.05


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


def forward_bytes(width, bag, weighted):
    return 16 + 4 * width + (4 * width + 16) / bag + (4 if weighted else 0)


def backward_bytes(width, bag, strict, unique, weighted):
    if strict:
        return 8 / bag + 12 + 8 + 4 + 4 + 4 * width / bag + 40 * width + (4 if weighted else 0)
    return (8 / bag + 12 + 16 + 4 + 32 * SORT_PASSES + 16 + 30 * unique + 4 + 4 * width + 40 * width * unique +
            (20 if weighted else 0))


def check_forward(out_weighted, out_mean, out_lookup, weights, n, width, bag):
    """the replies == the f32 mirror of the looked-up rows: per id one multiply and one add
    in arrival order from +0; the mean: the plain sum, one division by L"""
    rows = out_lookup.download(np.float32, n * width).reshape(n // bag, bag, width)
    w = weights.reshape(n // bag, bag)
    acc = np.zeros((n // bag, width), dtype=np.float32)
    plain = np.zeros((n // bag, width), dtype=np.float32)
    for j in range(bag):
        acc = acc + w[:, j, None] * rows[:, j, :]
        plain = plain + rows[:, j, :]
    mean = plain / np.float32(bag)
    got_w = out_weighted.download(np.float32, (n // bag) * width).reshape(n // bag, width)
    got_m = out_mean.download(np.float32, (n // bag) * width).reshape(n // bag, width)
    return (bool(np.array_equal(got_w.view(np.uint32), acc.view(np.uint32))),
            bool(np.array_equal(got_m.view(np.uint32), mean.view(np.uint32))))


def check_backward(width, n, dk, rows, stream, dq, doff, dw, mode, grads, weights, bag):
    """a table that took update_pooled_weighted == a twin that took update_merged on E"""
    nb = n // bag
    g = grads.download(np.float32, nb * width).reshape(nb, width)
    e = np.repeat(g, bag, axis=0)
    e = e / np.float32(bag) if mode == psg.POOL_MEAN else weights[:, None] * e
    de = psg.DeviceBuffer.from_numpy(np.ascontiguousarray(e, dtype=np.float32).ravel())
    a, b = (new_table(width, n, dk, rows, stream) for _ in range(2))
    a.update_pooled_weighted(dq, doff, dw, mode, grads, n, nb, LR, 0, stream)
    b.update_merged(psg.PUSH, [dq], [de], None, [n], LR, 0, stream)
    ok = bool(np.array_equal(a.dump()[1].view(np.uint32), b.dump()[1].view(np.uint32)))
    a.close()
    b.close()
    de.free()
    return ok


def case(width, n, bags, reps, stream, check_at):
    nvals = n * width
    rng = np.random.default_rng(width)
    keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(977)
    dk = psg.DeviceBuffer.from_numpy(keys)
    rows = psg.DeviceBuffer(nvals * 4)
    rows.fill_synth(nvals, psg.F32, 7, 1, -1.0, 1.0)
    t = new_table(width, n, dk, rows, stream)
    pooled = psg.DeviceBuffer(nvals * 4 // min(bags))
    pooled_mean = psg.DeviceBuffer(nvals * 4 // min(bags))
    grads = psg.DeviceBuffer(nvals * 4 // min(bags))
    grads.fill_synth(nvals // min(bags), psg.F32, 11, 1, -1.0, 1.0)
    weights = rng.uniform(-2, 2, n).astype(np.float32)
    dw = psg.DeviceBuffer.from_numpy(weights)
    res = []
    for order, q in id_lists(keys, rng).items():
        dq = psg.DeviceBuffer.from_numpy(q)
        unique = len(np.unique(q)) / n
        for bag in bags:
            nb = n // bag
            assert nb * bag == n
            r = {"dtype": "f32", "width": width, "keys": n, "table_bytes": nvals * 4, "list": order, "bag": bag,
                 "bags": nb, "unique_share": unique}
            doff = psg.DeviceBuffer.from_numpy(np.arange(nb + 1, dtype=np.uint64) * np.uint64(bag))
            r["lookup_pooled_ms"] = measure(lambda: t.lookup_pooled(dq, doff, pooled, n, nb, stream), reps, stream)
            r["lookup_mean_ms"] = measure(
                lambda: t.lookup_pooled_weighted(dq, doff, None, psg.POOL_MEAN, pooled_mean, n, nb, stream), reps, stream)
            r["lookup_weighted_ms"] = measure(
                lambda: t.lookup_pooled_weighted(dq, doff, dw, psg.POOL_SUM, pooled, n, nb, stream), reps, stream)
            if (width, bag) == check_at:
                out = psg.DeviceBuffer(nvals * 4)
                t.lookup(dq, out, None, n, stream)
                r["forward_weighted_checked"], r["forward_mean_checked"] = check_forward(pooled, pooled_mean, out, weights,
                                                                                        n, width, bag)
                out.free()
            it = [0]

            def step(pooling):
                def run():
                    if pooling == "plain":
                        t.update_pooled(dq, doff, grads, n, nb, LR, it[0], stream)
                    elif pooling == "weighted":
                        t.update_pooled_weighted(dq, doff, dw, psg.POOL_SUM, grads, n, nb, LR, it[0], stream)
                    else:
                        t.update_pooled_weighted(dq, doff, None, psg.POOL_MEAN, grads, n, nb, LR, it[0], stream)
                    it[0] += 1
                return run

            r["update_pooled_ms"] = measure(step("plain"), reps, stream)
            r["update_weighted_ms"] = measure(step("weighted"), reps, stream)
            r["update_mean_ms"] = measure(step("mean"), reps, stream)
            assert t.info().size == n, "a call inserted rows"
            if (width, bag) == check_at:
                r["backward_weighted_checked"] = check_backward(width, n, dk, rows, stream, dq, doff, dw, psg.POOL_SUM,
                                                                grads, weights, bag)
                r["backward_mean_checked"] = check_backward(width, n, dk, rows, stream, dq, doff, None, psg.POOL_MEAN,
                                                            grads, weights, bag)
            strict = order == "sorted"
            r["lookup_weighted_over_lookup_pooled"] = r["lookup_weighted_ms"] / r["lookup_pooled_ms"]
            r["lookup_mean_over_lookup_pooled"] = r["lookup_mean_ms"] / r["lookup_pooled_ms"]
            r["update_weighted_over_update_pooled"] = r["update_weighted_ms"] / r["update_pooled_ms"]
            r["update_mean_over_update_pooled"] = r["update_mean_ms"] / r["update_pooled_ms"]
            r["lookup_weighted_model"] = forward_bytes(width, bag, True) / forward_bytes(width, bag, False)
            r["update_weighted_model"] = (backward_bytes(width, bag, strict, unique, True) /
                                          backward_bytes(width, bag, strict, unique, False))
            res.append(r)
            print("rows_pooled_weighted_bench: case done:", json.dumps(r), file=sys.stderr, flush=True)
            doff.free()
        dq.free()
    for b in (dk, rows, pooled, pooled_mean, grads, dw):
        b.free()
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--bags", default="4,16,64")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_pooled_weighted_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_pooled_weighted_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    bags = [int(x) for x in a.bags.split(",")]
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        cases += case(w, a.table_bytes // (4 * w), bags, a.reps, stream, (32, 16))

    def at(order):
        hit = [c for c in cases if c["width"] == 32 and c["bag"] == 16 and c["list"] == order]
        return hit[0] if hit else None

    def condition(c, ratio, model):
        if not c:
            return None
        bound = (c[model] if model else 1.0) * SPREAD
        return {"ratio": c[ratio], "model": c[model] if model else 1.0, "bound": bound, "held": c[ratio] <= bound}

    f, b = at("sorted"), at("shuffled")
    line = {"bench": "rows_pooled_weighted", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases,
            "FW": condition(f, "lookup_weighted_over_lookup_pooled", "lookup_weighted_model"),
            "FM": condition(f, "lookup_mean_over_lookup_pooled", None),
            "BW": condition(b, "update_weighted_over_update_pooled", "update_weighted_model"),
            "BM": condition(b, "update_mean_over_update_pooled", None)}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text + "\n")


if __name__ == "__main__":
    main()
