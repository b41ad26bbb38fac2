#!/usr/bin/env python3
"""What a bag costs on a frozen 8-bit snapshot (psg_qtable_lookup_pooled,
k_qrows_pool) beside the same bag on the F32 table it was frozen from
(psg_table_lookup_pooled, unchanged code: the yardstick) — a record, not a test.
Needs an MI355X; prints ONE JSON line and writes it to --out.

1 Mi rows present, W = 16, 64, 256; 128 Ki bags of 32 shuffled ids (4 Mi positions,
every row four times), sum pooling.  Event-timed around the whole call, median of
--reps after two warm-up calls, the two calls alternating inside every repetition
of one process:

  q8_ms, f32_ms    the pooled lookup on the snapshot / on the table
  q8_over_f32      their ratio, beside
  byte_bound       (stride + 4) / (4 W + 4): the row bytes and the slot a position
                   fetches, snapshot over table
  freeze_ms        one psg_table_freeze_q8 of the table (wall clock, its one
                   synchronisation included)
  copy_gbs         psg_copy of 1 GiB in this process (read + written)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))

KMAX = (1 << 64) - 1
N = 1 << 20
REPEAT = 4
BAG = 32
WIDTHS = (16, 64, 256)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qrows_bench.json"))
    a = ap.parse_args()
    import psg

    psg.set_device(0)
    stream = psg.Stream()

    def timed(fn):
        e0, e1 = psg.Event(timing=True), psg.Event(timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.sync()
        ms = e0.elapsed_ms(e1)
        e0.close()
        e1.close()
        return ms

    res = {"bench": "qrows", "reps": a.reps, "rows": N, "positions": REPEAT * N, "bag": BAG}
    x, y = psg.DeviceBuffer(1 << 30), psg.DeviceBuffer(1 << 30)
    xs = [timed(lambda: psg.copy(y, x, 1 << 30, stream=stream)) for _ in range(2 + a.reps)][2:]
    res["copy_gbs"] = 2 * (1 << 30) / (float(np.median(xs)) * 1e-3) / 1e9
    x.free()
    y.free()
    rng = np.random.default_rng(1)
    keys = np.uint64(2) + np.arange(N, dtype=np.uint64) * np.uint64(977)
    n, nb = REPEAT * N, REPEAT * N // BAG
    dk = psg.DeviceBuffer.from_numpy(keys)
    dq = psg.DeviceBuffer.from_numpy(rng.permutation(np.tile(keys, REPEAT)))
    doff = psg.DeviceBuffer.from_numpy(np.arange(nb + 1, dtype=np.uint64) * np.uint64(BAG))
    for w in WIDTHS:
        t = psg.Table(psg.F32, w, 0, KMAX, 0)
        rows = psg.DeviceBuffer(N * w * 4)
        psg.init_rows(rows, dk, N, psg.F32, w, 5, -1.0, 1.0, stream)
        t.assign(dk, rows, N, None, None, stream)
        rows.free()
        t0 = time.perf_counter()
        q = t.freeze_q8(stream)
        freeze_ms = (time.perf_counter() - t0) * 1e3
        out = psg.DeviceBuffer(nb * w * 4)
        calls = {"q8": lambda: q.lookup_pooled(dq, doff, None, psg.POOL_SUM, out, n, nb, stream),
                 "f32": lambda: t.lookup_pooled(dq, doff, out, n, nb, stream)}
        ms = {c: [] for c in calls}
        for i in range(2 + a.reps):
            for c, fn in calls.items():
                v = timed(fn)
                if i >= 2:
                    ms[c].append(v)
        stride = (((w + 3) // 4 * 4 + 8) + 15) // 16 * 16
        r = {c + "_ms": float(np.median(ms[c])) for c in calls}
        r["q8_over_f32"] = r["q8_ms"] / r["f32_ms"]
        r["byte_bound"] = (stride + 4) / (4 * w + 4)
        r["freeze_ms"] = freeze_ms
        r["q8_device_bytes"] = int(q.info().device_bytes)
        res[f"w{w}"] = r
        q.close()
        t.close()
        out.free()
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
