#!/usr/bin/env python3
"""The row table's optimizer update (psg_table_update) against the row Push and
the dense LR apply — a record, not a test.  Needs an MI355X; prints ONE JSON
line and writes it to --out.

For F32 and W in {8, 32, 128}, with n = 1 GiB / (4 W) keys — 1 GiB of rows
resident, well past the 256 MiB Infinity Cache — and two key lists, every key
of the table and a random half of them, each case reports, event-timed around
the whole call (both passes and the host between them), median of --reps:

  sgd_ms / adam_ms       psg_table_update(PSG_PUSH) on a table without / with
                         Adam state
  push_ms                the yardstick psg_table_handle(PSG_PUSH) on the same list
  dense_sgd_ms / dense_adam_ms   the yardstick psg_lr_apply_sum, one frame,
                         from_zero = 0, on a DENSE store of n W features
  *_bytes                algorithmic bytes: per key 16 (key, slot write and
                         read) + per element 12 (SGD, and the row Push) or 44
                         (Adam: gradient 4, row 8, moments 32); dense: 12 / 44
                         per feature
  *_frac_8tbs, *_frac_copy   bytes / time over 8 TB/s and over psg_copy's rate
                         in this process (copy_gbs)

and at W = 32 on the full list the two conditions

  sgd_over_push          sgd_ms / push_ms                       must be <= 1.10
  adam_over_bound        adam_ms / (push_ms + 1.15 (dense_adam_ms - dense_sgd_ms))
                                                                must be <= 1
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
PEAK = 8e12
LR = 0.01


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
    """two warm-up calls, then the median of reps timed ones; fn takes the call's number"""
    fn(0)
    fn(1)
    return median([timed(lambda: fn(2 + i), stream) for i in range(reps)])


def copy_rate(dst, src, nbytes, reps, stream):
    psg.copy(dst, src, nbytes, 4, 8, stream)
    ms = median([timed(lambda: psg.copy(dst, src, nbytes, 4, 8, stream), stream) for _ in range(reps)])
    return 2 * nbytes / (ms * 1e-3)


def case(width, n_table, subset, reps, rate, stream, rng):
    row_keys = np.uint64(1) + np.arange(n_table, dtype=np.uint64) * np.uint64(977)
    keys = row_keys[rng.random(n_table) < 0.5] if subset else row_keys
    n = len(keys)
    nvals = n * width
    dk = psg.DeviceBuffer.from_numpy(keys)
    grads = psg.DeviceBuffer(nvals * 4)
    grads.fill_synth(nvals, psg.F32, 7, 1, -1.0, 1.0)
    res = {"dtype": "f32", "width": width, "table_keys": n_table, "table_bytes": n_table * width * 4,
           "list": "random half" if subset else "full", "keys": n}

    def table(adam):
        t = psg.Table(psg.F32, width, 0, KMAX, n_table)
        # the table holds every key before the list is timed
        full = psg.DeviceBuffer.from_numpy(row_keys)
        scratch = psg.DeviceBuffer(n_table * width * 4)
        t.handle(psg.PULL, full, None, scratch, n_table, stream)
        full.free()
        scratch.free()
        if adam:
            t.set_adam(LR)
        return t

    t = table(False)
    push_ms = measure(lambda i: t.handle(psg.PUSH, dk, grads, None, n, stream), reps, stream)
    sgd_ms = measure(lambda i: t.update(psg.PUSH, dk, grads, None, n, LR, i, stream), reps, stream)
    t.close()
    t = table(True)
    adam_ms = measure(lambda i: t.update(psg.PUSH, dk, grads, None, n, LR, i, stream), reps, stream)
    t.close()

    dense = psg.Store(psg.DENSE, psg.F32, 0, nvals, nvals)
    dense_sgd_ms = measure(lambda i: psg.lr_apply_sum(dense, [grads], nvals, LR, None, i, False, stream), reps, stream)
    adam = psg.Adam(nvals, LR)
    dense_adam_ms = measure(lambda i: psg.lr_apply_sum(dense, [grads], nvals, LR, adam, i, False, stream), reps, stream)
    adam.close()
    dense.close()
    dk.free()
    grads.free()

    times = {"push": (push_ms, n * 16 + nvals * 12), "sgd": (sgd_ms, n * 16 + nvals * 12),
             "adam": (adam_ms, n * 16 + nvals * 44), "dense_sgd": (dense_sgd_ms, nvals * 12),
             "dense_adam": (dense_adam_ms, nvals * 44)}
    for name, (ms, nbytes) in times.items():
        res[name + "_ms"] = ms
        res[name + "_bytes"] = nbytes
        res[name + "_frac_8tbs"] = nbytes / (ms * 1e-3) / PEAK
        res[name + "_frac_copy"] = nbytes / (ms * 1e-3) / rate
    res["copy_gbs"] = rate / 1e9
    res["sgd_over_push"] = sgd_ms / push_ms
    res["adam_bound_ms"] = push_ms + 1.15 * (dense_adam_ms - dense_sgd_ms)
    res["adam_over_bound"] = adam_ms / res["adam_bound_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_opt_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_opt_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    rng = np.random.default_rng(5)
    cb = min(a.table_bytes, 1 << 30) // 16 * 16
    src, dst = psg.DeviceBuffer(cb), psg.DeviceBuffer(cb)
    rate = copy_rate(dst, src, cb, a.reps, stream)
    src.free()
    dst.free()
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        for subset in (False, True):
            cases.append(case(w, a.table_bytes // (4 * w), subset, a.reps, rate, stream, rng))
            print("rows_opt_bench: case done:", json.dumps(cases[-1]), file=sys.stderr, flush=True)
    full32 = [c for c in cases if c["width"] == 32 and c["list"] == "full"]
    line = {"bench": "rows_opt", "device": psg.device_pci_bus_id(0), "peak_bytes_per_s": PEAK, "reps": a.reps,
            "cases": cases,
            "w32_full_sgd_over_push": full32[0]["sgd_over_push"] if full32 else None,
            "w32_full_sgd_within_1_10": (full32[0]["sgd_over_push"] <= 1.10) if full32 else None,
            "w32_full_adam_over_bound": full32[0]["adam_over_bound"] if full32 else None,
            "w32_full_adam_within_bound": (full32[0]["adam_over_bound"] <= 1.0) if full32 else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
