#!/usr/bin/env python3
"""Row-valued table (psg_table_*) against the scalar SORTED store on expanded
keys — a record, not a test.  Needs an MI355X; prints ONE JSON line and writes
it to --out.

For F32 and W in {8, 32, 128}, with n = 1 GiB / (4 W) keys — a table of 1 GiB
of rows, well past the 256 MiB Infinity Cache — and two key lists, every key
of the table and a random half of them, each case reports

  push_ms / pull_ms      event-timed psg_table_handle (median of --reps), the
                         call as a whole: both passes and the host between them
  push_bytes / pull_bytes   algorithmic bytes: per key 8 (key) + 8 (slot write
                         and read) + 12 W (Push) or 8 W (Pull)
  push_frac_8tbs / ...   bytes / time over 8 TB/s
  copy_gbs               psg_copy's rate in this process (1 GiB copied: 2 GiB
                         moved), the copy ceiling bench.py also reports, and
                         push_frac_copy / pull_frac_copy against it
  scalar_push_ms / scalar_pull_ms   the same values through psg_store_handle
                         on a SORTED store with keys key * W + j (the only way
                         to keep rows without the table), same process, same
                         sequence of requests; skipped (scalar_skipped) where
                         n W exceeds the store's 2^32-2 keys
  ratio                  (push_ms + pull_ms) / (scalar_push_ms + scalar_pull_ms)
  pull_matches_scalar    the last Pull of both paths has one checksum
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
STORE_MAX_KEYS = (1 << 32) - 2


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


def run_requests(handle, out, out_bytes, reps, stream):
    """The one sequence both paths serve: an inserting Push, a warm-up Push and
    Pull, then reps timed (Push, Pull) pairs.  Returns the medians and the
    checksum of the last Pull."""
    handle(psg.PUSH)
    handle(psg.PUSH)
    handle(psg.PULL)
    push, pull = [], []
    for _ in range(reps):
        push.append(timed(lambda: handle(psg.PUSH), stream))
        pull.append(timed(lambda: handle(psg.PULL), stream))
    return median(push), median(pull), psg.checksum(out, out_bytes, stream)


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
    vals = psg.DeviceBuffer(nvals * 4)
    vals.fill_synth(nvals, psg.F32, 7, 0, 0.0, 16.0)
    out = psg.DeviceBuffer(nvals * 4)
    res = {"dtype": "f32", "width": width, "table_keys": n_table, "table_bytes": n_table * width * 4,
           "list": "random half" if subset else "full", "keys": n}

    table = psg.Table(psg.F32, width, 0, KMAX, n_table)
    # the table holds every key before the list is timed (a subset list hits a full table)
    if subset:
        full = psg.DeviceBuffer.from_numpy(row_keys)
        table.handle(psg.PULL, full, None, psg.DeviceBuffer(n_table * width * 4), n_table, stream)
        full.free()
    push_ms, pull_ms, sum_rows = run_requests(
        lambda f: table.handle(f, dk, vals if f & psg.PUSH else None, out if f & psg.PULL else None, n, stream),
        out, nvals * 4, reps, stream)
    table.close()
    push_bytes = n * (16 + 12 * width)
    pull_bytes = n * (16 + 8 * width)
    res.update(push_ms=push_ms, pull_ms=pull_ms, push_bytes=push_bytes, pull_bytes=pull_bytes,
               push_frac_8tbs=push_bytes / (push_ms * 1e-3) / PEAK, pull_frac_8tbs=pull_bytes / (pull_ms * 1e-3) / PEAK,
               copy_gbs=rate / 1e9, push_frac_copy=push_bytes / (push_ms * 1e-3) / rate,
               pull_frac_copy=pull_bytes / (pull_ms * 1e-3) / rate)

    if n_table * width > STORE_MAX_KEYS:
        res["scalar_skipped"] = "n * W = %d exceeds the scalar store's 2^32-2 keys" % (n_table * width)
        return res
    expand = lambda k: (k[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)).ravel()  # noqa: E731
    store = psg.Store(psg.SORTED, psg.F32, 0, KMAX, n_table * width)
    if subset:
        full = psg.DeviceBuffer.from_numpy(expand(row_keys))
        store.handle(psg.PULL, full, None, psg.DeviceBuffer(n_table * width * 4), n_table * width, stream=stream)
        full.free()
    ek = psg.DeviceBuffer.from_numpy(expand(keys))
    s_push, s_pull, sum_scalar = run_requests(
        lambda f: store.handle(f, ek, vals if f & psg.PUSH else None, out if f & psg.PULL else None, nvals,
                               stream=stream),
        out, nvals * 4, reps, stream)
    res.update(scalar_push_ms=s_push, scalar_pull_ms=s_pull, scalar_push_bytes=nvals * 28, scalar_pull_bytes=nvals * 24,
               ratio=(push_ms + pull_ms) / (s_push + s_pull), pull_matches_scalar=sum_rows == sum_scalar,
               scalar_served=store.counters())
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_bench: no GPU (this is a measurement: it does not fall back)")
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
            print("rows_bench: case done:", json.dumps(cases[-1]), file=sys.stderr, flush=True)
    full32 = [c for c in cases if c["width"] == 32 and c["list"] == "full" and "ratio" in c]
    line = {"bench": "rows", "device": psg.device_pci_bus_id(0), "peak_bytes_per_s": PEAK, "reps": a.reps,
            "cases": cases,
            "w32_full_ratio": full32[0]["ratio"] if full32 else None,
            "w32_full_within_two_thirds": (full32[0]["ratio"] <= 2.0 / 3.0) if full32 else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
