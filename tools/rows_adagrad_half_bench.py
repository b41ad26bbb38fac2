#!/usr/bin/env python3
"""What row-wise Adagrad costs on BF16 rows (psg_table_set_adagrad_half,
k_rows_walk_rowwise_half) beside an F32 Adagrad table of the same build and the
same process — a record, not a test.  Needs an MI355X; prints ONE JSON line and
writes it to --out.

Event-timed around the whole call, median of --reps after two warm-up calls, 1 Mi
rows present, for W = 16, 64, 256 and three tables that alternate inside every
repetition (f32; bf16_nearest; bf16_stochastic):

  strict_w{W}_{table}_ms   psg_table_update (PUSH) of the 1 Mi ascending keys
  same_w{W}_{table}_ms     psg_table_update_merged (PUSH), k = 4 frames on that list
..._frac: algorithmic bytes / time over the psg_copy ceiling taken in the same
process (copy_gbs: 1 GiB read + 1 GiB written), and ..._over_f32: the time over the
F32 table's.  Algorithmic bytes, U unique rows of element size s, n occurrences:
n * (8 key + 4 W gradient) + U * (8 slot + 2 s W row read and written + 16
accumulator) and, stochastic, + U * 8 for the row's key.  Per column that is 8 B
against 12 B: 0.67 is the byte bound of strict_..._over_f32 for a wide row.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))

KMAX = (1 << 64) - 1
N = 1 << 20
K = 4
WIDTHS = (16, 64, 256)
LR = 0.05
TABLES = ("f32", "bf16_nearest", "bf16_stochastic")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_adagrad_half_bench.json"))
    a = ap.parse_args()
    import psg

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

    psg.set_device(0)
    stream = psg.Stream()
    res = {"bench": "rows_adagrad_half", "reps": a.reps, "keys": N}
    x, y = psg.DeviceBuffer(1 << 30), psg.DeviceBuffer(1 << 30)
    xs = [timed(lambda: psg.copy(y, x, 1 << 30, stream=stream), stream) for _ in range(2 + a.reps)][2:]
    res["copy_gbs"] = 2 * (1 << 30) / (float(np.median(xs)) * 1e-3) / 1e9
    x.free()
    y.free()
    keys = np.uint64(2) + np.arange(N, dtype=np.uint64) * np.uint64(977)
    dk = psg.DeviceBuffer.from_numpy(keys)
    for w in WIDTHS:
        g = psg.DeviceBuffer(K * N * w * 4)  # K frames of N rows
        g.fill_synth(K * N * w, psg.F32, 7, 1, -1.0, 1.0)
        frames = [g.ptr + j * N * w * 4 for j in range(K)]
        tables = {}
        for name in TABLES:
            t = tables[name] = psg.Table(psg.F32 if name == "f32" else psg.BF16, w, 0, KMAX, 0)
            if name == "f32":
                t.set_adagrad(0.1)
            else:
                t.set_adagrad_half(0.1, rounding=psg.ROUND_STOCHASTIC if name.endswith("stochastic") else psg.ROUND_NEAREST,
                                   seed=12345)
            t.assign(dk, None, N, None, None, stream)
        calls = {
            "strict": (lambda t: t.update(psg.PUSH, dk, g, None, N, LR, 0, stream), N),
            "same": (lambda t: t.update_merged(psg.PUSH, [dk] * K, frames, None, [N] * K, LR, 0, stream), K * N),
        }
        for call_name, (call, n) in calls.items():
            ms = {name: [] for name in TABLES}
            for i in range(2 + a.reps):  # the tables alternate inside every repetition
                for name in TABLES:
                    v = timed(lambda: call(tables[name]), stream)
                    if i >= 2:
                        ms[name].append(v)
            for name in TABLES:
                s = 4 if name == "f32" else 2
                nbytes = n * (8 + 4 * w) + N * (8 + 2 * s * w + 16 + (8 if name.endswith("stochastic") else 0))
                m = float(np.median(ms[name]))
                res[f"{call_name}_w{w}_{name}_ms"] = m
                res[f"{call_name}_w{w}_{name}_spread_ms"] = [float(min(ms[name])), float(max(ms[name]))]
                res[f"{call_name}_w{w}_{name}_frac"] = nbytes / (m * 1e-3) / 1e9 / res["copy_gbs"]
            for name in TABLES[1:]:
                res[f"{call_name}_w{w}_{name}_over_f32"] = res[f"{call_name}_w{w}_{name}_ms"] / res[f"{call_name}_w{w}_f32_ms"]
        for t in tables.values():
            assert t.info().size == N
            t.close()
        g.free()
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
