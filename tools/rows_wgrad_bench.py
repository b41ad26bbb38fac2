#!/usr/bin/env python3
"""What the weighted bag's weight gradient (psg_table_pooled_weight_grad,
k_rows_pool_wgrad) costs beside the forward it belongs to — a record, not a test.
Needs an MI355X; prints ONE JSON line and writes it to --out.

1 Mi rows present, W = 16, 64, 256, F32 and BF16, a list of 4 Mi shuffled positions
(every row four times) in bags of 32 and, the balance claim, the same list as ONE
bag.  Event-timed around the whole call, median of --reps after two warm-up calls,
the calls alternating inside every repetition:

  wgrad_ms, wgrad_onebag_ms   psg_table_pooled_weight_grad, bags of 32 / one bag
  forward_ms                  psg_table_lookup_pooled_weighted on the bags of 32: the yardstick
  lookup_ms                   psg_table_lookup of the same list (n * W elements written)
  copy_gbs                    psg_copy of 1 GiB in this process (read + written)
and wgrad_over_forward, onebag_over_bags, and ..._frac: algorithmic bytes / time over
the copy ceiling.  Algorithmic bytes of n positions in nb bags, e the element size:
key 8 + slot 8 + W e a position, then the forward 4 n weights + nb W e written, the
gradient nb W 4 read + 4 n written, the lookup n W e written.
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
REPEAT = 4
BAG = 32
WIDTHS = (16, 64, 256)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_wgrad_bench.json"))
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

    res = {"bench": "rows_wgrad", "reps": a.reps, "rows": N, "positions": REPEAT * N, "bag": BAG}
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
    done = psg.DeviceBuffer.from_numpy(np.array([0, n], np.uint64))
    dwt = psg.DeviceBuffer(n * 4)
    dwt.fill_synth(n, psg.F32, 9, 1, -1.0, 1.0)
    ddw = psg.DeviceBuffer(n * 4)
    for name, dtype, e in (("f32", psg.F32, 4), ("bf16", psg.BF16, 2)):
        for w in WIDTHS:
            t = psg.Table(dtype, w, 0, KMAX, 0)
            rows = psg.DeviceBuffer(N * w * e)  # rows that are not zero, on a table without an initializer
            psg.init_rows(rows, dk, N, dtype, w, 5, -1.0, 1.0, stream)
            t.assign(dk, rows, N, None, None, stream)
            rows.free()
            g = psg.DeviceBuffer(nb * w * 4)
            g.fill_synth(nb * w, psg.F32, 7, 1, -1.0, 1.0)
            out = psg.DeviceBuffer(n * w * e)
            calls = {
                "wgrad": lambda: t.pooled_weight_grad(dq, doff, g, ddw, n, nb, stream),
                "wgrad_onebag": lambda: t.pooled_weight_grad(dq, done, g, ddw, n, 1, stream),
                "forward": lambda: t.lookup_pooled_weighted(dq, doff, dwt, psg.POOL_SUM, out, n, nb, stream),
                "lookup": lambda: t.lookup(dq, out, None, n, stream),
            }
            ms = {c: [] for c in calls}
            for i in range(2 + a.reps):
                for c, fn in calls.items():
                    v = timed(fn)
                    if i >= 2:
                        ms[c].append(v)
            per = n * (16 + w * e)
            nbytes = {"wgrad": per + nb * w * 4 + 4 * n, "wgrad_onebag": per + w * 4 + 4 * n,
                      "forward": per + 4 * n + nb * w * e, "lookup": per + n * w * e}
            r = {}
            for c in calls:
                m = float(np.median(ms[c]))
                r[c + "_ms"] = m
                r[c + "_frac"] = nbytes[c] / (m * 1e-3) / 1e9 / res["copy_gbs"]
            r["wgrad_over_forward"] = r["wgrad_ms"] / r["forward_ms"]
            r["onebag_over_bags"] = r["wgrad_onebag_ms"] / r["wgrad_ms"]
            res[f"{name}_w{w}"] = r
            assert t.info().size == N
            t.close()
            g.free()
            out.free()
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
