#!/usr/bin/env python3
"""The row table's lookup and erase (psg_table_lookup / psg_table_erase) against
existing calls that move the same rows — a record, not a test.  Needs an MI355X;
prints ONE JSON line and writes it to --out.

For F32 and W in {8, 32, 128}, with n = 1 GiB / (4 W) keys — 1 GiB of rows
resident, well past the 256 MiB Infinity Cache — each case reports, event-timed
around the whole call, median of --reps:

  lookup_ms         psg_table_lookup (rows and found), the full ascending list
  pull_ms           yardstick psg_table_handle(PSG_PULL) of that list: the same
                    bytes, two host synchronisations instead of one
  lookup_shuf_ms    psg_table_lookup of the full list, shuffled
  pull_any_ms       yardstick psg_table_handle_any(PSG_PULL) of that list: it sorts
  lookup_half_ms    psg_table_lookup of n occurrences in random order, half of
                    them present keys and half absent ones (report only)
  pull_half_ms      yardstick psg_table_handle(PSG_PULL) of the present half, ascending
  erase_ms          psg_table_erase of every other key (n / 2 rows survive)
  reinsert_ms       yardstick psg_table_assign(rows = NULL) of those keys into
                    the table the erase left: it moves n / 2 old rows and n / 2
                    zero rows into arrays of n, the erase n / 2 rows into n / 2
  *_over_*          the ratio of the times

At W = 32 the two conditions
  lookup_over_pull           must be <= 1.05
  lookup_shuf_over_pull_any  must be below 1.0
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
    """two warm-up calls, then the median of reps timed ones"""
    fn()
    fn()
    return median([timed(fn, stream) for _ in range(reps)])


def case(width, n, reps, stream):
    nvals = n * width
    rng = np.random.default_rng(width)
    keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(977)  # key + 1 is never a key
    dk = psg.DeviceBuffer.from_numpy(keys)
    rows = psg.DeviceBuffer(nvals * 4)
    rows.fill_synth(nvals, psg.F32, 7, 1, -1.0, 1.0)
    out, fnd = psg.DeviceBuffer(nvals * 4), psg.DeviceBuffer(n)
    res = {"dtype": "f32", "width": width, "keys": n, "table_bytes": nvals * 4}

    t = psg.Table(psg.F32, width, 0, KMAX, n)
    t.assign(dk, rows, n, None, None, stream)  # the table holds every key before anything is timed
    rows.free()
    res["lookup_ms"] = measure(lambda: t.lookup(dk, out, fnd, n, stream), reps, stream)
    res["pull_ms"] = measure(lambda: t.handle(psg.PULL, dk, None, out, n, stream), reps, stream)

    ds = psg.DeviceBuffer.from_numpy(rng.permutation(keys))
    res["lookup_shuf_ms"] = measure(lambda: t.lookup(ds, out, fnd, n, stream), reps, stream)
    res["pull_any_ms"] = measure(lambda: t.handle_any(psg.PULL, ds, None, out, n, stream), reps, stream)
    ds.free()

    h = n // 2
    present = np.sort(rng.choice(keys, h, replace=False))
    mixed = np.concatenate([present, rng.choice(keys, n - h, replace=False) + np.uint64(1)])
    dm, dp = psg.DeviceBuffer.from_numpy(rng.permutation(mixed)), psg.DeviceBuffer.from_numpy(present)
    res["lookup_half_ms"] = measure(lambda: t.lookup(dm, out, fnd, n, stream), reps, stream)
    res["pull_half_ms"] = measure(lambda: t.handle(psg.PULL, dp, None, out, h, stream), reps, stream)
    dm.free()
    dp.free()
    assert t.info().size == n, "a yardstick inserted rows"

    odd = np.ascontiguousarray(keys[1::2])
    do = psg.DeviceBuffer.from_numpy(odd)
    er, ins = [], []
    for i in range(2 + reps):  # each erase is undone by its yardstick: two warm-up rounds, then reps timed ones
        a = timed(lambda: t.erase(do, len(odd), stream), stream)
        assert t.info().size == n - len(odd)
        b = timed(lambda: t.assign(do, None, len(odd), None, None, stream), stream)
        assert t.info().size == n
        if i >= 2:
            er.append(a)
            ins.append(b)
    res["erase_ms"], res["reinsert_ms"] = median(er), median(ins)
    res["erase_rows_moved"], res["reinsert_rows_moved"] = n - len(odd), n
    for b in (do, out, fnd, dk):
        b.free()
    t.close()

    res["lookup_over_pull"] = res["lookup_ms"] / res["pull_ms"]
    res["lookup_shuf_over_pull_any"] = res["lookup_shuf_ms"] / res["pull_any_ms"]
    res["lookup_half_over_pull_half"] = res["lookup_half_ms"] / res["pull_half_ms"]
    res["erase_over_reinsert"] = res["erase_ms"] / res["reinsert_ms"]
    res["lookup_gbs"] = n * (16 + 8 * width + 1) / (res["lookup_ms"] * 1e-3) / 1e9
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_lifecycle_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_lifecycle_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        cases.append(case(w, a.table_bytes // (4 * w), a.reps, stream))
        print("rows_lifecycle_bench: case done:", json.dumps(cases[-1]), file=sys.stderr, flush=True)
    w32 = [c for c in cases if c["width"] == 32]
    line = {"bench": "rows_lifecycle", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases,
            "w32_lookup_over_pull": w32[0]["lookup_over_pull"] if w32 else None,
            "w32_lookup_within_1_05": (w32[0]["lookup_over_pull"] <= 1.05) if w32 else None,
            "w32_lookup_shuf_over_pull_any": w32[0]["lookup_shuf_over_pull_any"] if w32 else None,
            "w32_lookup_shuf_below_1": (w32[0]["lookup_shuf_over_pull_any"] < 1.0) if w32 else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
