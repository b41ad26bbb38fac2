#!/usr/bin/env python3
"""The row table's merged update (psg_table_update_merged) against what the
table offered before it — a record, not a test.  Needs an MI355X; prints ONE
JSON line and writes it to --out.

F32, W in {8, 32, 128}, n = 1 GiB / (4 W) keys — 1 GiB of rows resident, well
past the 256 MiB Infinity Cache.  Every time is event-timed around the whole
call (every pass and the host between them), median of --reps, the yardstick in
the same process on a table of its own.

same list, k = 4 frames on the full list, each frame with a device copy of the
list of its own (so the compare pass runs, as it does behind the sync handle),
SGD and Adam:
  merged_ms        one psg_table_update_merged(PSG_PUSH) (path SAME_LIST)
  sequential_ms    the yardstick: 4 consecutive psg_table_update calls on that list
  ratio            merged_ms / sequential_ms
  bytes_ratio      algorithmic bytes per key, merged over sequential:
                   Adam ((4*4 + 8 + 32) W + 16 + 3*8) / (4 (44 W + 16)),
                   SGD  ((4*4 + 8) W + 16 + 3*8) / (4 (12 W + 16))
general, k = 4 frames, each a shuffled quarter of the table drawn on its own
(so the frames overlap), SGD and Adam:
  merged_ms        one psg_table_update_merged(PSG_PUSH) (path SORTED)
  any_ms           the yardstick: psg_table_update_any on the concatenated list
                   (the same sort, occurrences and bytes; with Adam one step per
                   occurrence instead of one per key)
  ratio            merged_ms / any_ms

and at W = 32 the two conditions
  same-list Adam ratio < 1.0          general SGD ratio <= 1.05

--trace NAME (general_merged_sgd or general_any_sgd) runs that one measurement
alone and writes nothing: the program to put behind a kernel trace.
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
LR = 0.01
K = 4


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


def table(width, row_keys, adam, stream):
    """a table that holds every key before anything is timed"""
    n = len(row_keys)
    t = psg.Table(psg.F32, width, 0, KMAX, n)
    full = psg.DeviceBuffer.from_numpy(row_keys)
    scratch = psg.DeviceBuffer(n * width * 4)
    t.handle(psg.PULL, full, None, scratch, n, stream)
    full.free()
    scratch.free()
    if adam:
        t.set_adam(LR)
    return t


def general(width, n, reps, stream, rng, grads, which):
    """K shuffled quarters with overlaps, one behind the other in one buffer;
    which: (name, adam, merged) measurements to take"""
    row_keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(977)
    q = n // K
    cat = np.concatenate([row_keys[rng.permutation(n)[:q]] for _ in range(K)])
    res = {"general_occurrences": len(cat), "general_unique_keys": int(len(np.unique(cat)))}
    dcat = psg.DeviceBuffer.from_numpy(cat)
    kp = [dcat.ptr + 8 * q * j for j in range(K)]
    gp = [grads.ptr + 4 * width * q * j for j in range(K)]  # q * K <= n rows
    for name, adam, merged in which:
        t = table(width, row_keys, adam, stream)
        if merged:
            paths = set()
            ms = measure(lambda i: paths.add(t.update_merged(psg.PUSH, kp, gp, None, [q] * K, LR, i, stream)), reps,
                         stream)
            assert paths == {psg.MERGED_SORTED}, paths
        else:
            ms = measure(lambda i: t.update_any(psg.PUSH, dcat, grads, None, q * K, LR, i, stream), reps, stream)
        t.close()
        res[name] = ms
    dcat.free()
    return res


def case(width, n, reps, stream, rng):
    row_keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(977)
    res = {"dtype": "f32", "width": width, "table_keys": n, "table_bytes": n * width * 4, "frames": K}
    # same list: the full list, K gradient frames, K device copies of the list
    dks = [psg.DeviceBuffer.from_numpy(row_keys) for _ in range(K)]
    dk = dks[0]
    grads = []
    for j in range(K):
        g = psg.DeviceBuffer(n * width * 4)
        g.fill_synth(n * width, psg.F32, 7 + j, 1, -1.0, 1.0)
        grads.append(g)
    for adam in (False, True):
        name = "adam" if adam else "sgd"
        t = table(width, row_keys, adam, stream)
        paths = set()
        merged = measure(lambda i: paths.add(t.update_merged(psg.PUSH, dks, grads, None, [n] * K, LR, i, stream)),
                         reps, stream)
        assert paths == {psg.MERGED_SAME_LIST}, paths
        t.close()
        t = table(width, row_keys, adam, stream)

        def sequential(i):
            for g in grads:
                t.update(psg.PUSH, dk, g, None, n, LR, i, stream)
        seq = measure(sequential, reps, stream)
        t.close()
        mb = ((4 * K + 8 + 32) * width + 16 + 3 * 8) if adam else ((4 * K + 8) * width + 16 + 3 * 8)
        sb = K * ((44 if adam else 12) * width + 16)
        res["same_" + name] = {"merged_ms": merged, "sequential_ms": seq, "ratio": merged / seq,
                               "merged_bytes_per_key": mb, "sequential_bytes_per_key": sb, "bytes_ratio": mb / sb}
    for d in dks:
        d.free()
    g = general(width, n, reps, stream, rng, grads[0],
                [("sgd_merged", False, True), ("sgd_any", False, False), ("adam_merged", True, True),
                 ("adam_any", True, False)])
    res["general_occurrences"], res["general_unique_keys"] = g["general_occurrences"], g["general_unique_keys"]
    for name in ("sgd", "adam"):
        res["general_" + name] = {"merged_ms": g[name + "_merged"], "any_ms": g[name + "_any"],
                                  "ratio": g[name + "_merged"] / g[name + "_any"]}
    for g in grads:
        g.free()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", choices=["general_merged_sgd", "general_any_sgd"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_merged_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_merged_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    rng = np.random.default_rng(5)
    if a.trace:
        for w in (int(x) for x in a.widths.split(",")):
            n = a.table_bytes // (4 * w)
            grads = psg.DeviceBuffer(n * w * 4)
            grads.fill_synth(n * w, psg.F32, 7, 1, -1.0, 1.0)
            r = general(w, n, a.reps, stream, rng, grads, [(a.trace, False, a.trace == "general_merged_sgd")])
            print("rows_merged_bench: trace:", json.dumps({"width": w, **r}), flush=True)
        return
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        cases.append(case(w, a.table_bytes // (4 * w), a.reps, stream, rng))
        print("rows_merged_bench: case done:", json.dumps(cases[-1]), file=sys.stderr, flush=True)
    w32 = [c for c in cases if c["width"] == 32]
    line = {"bench": "rows_merged", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases,
            "w32_same_adam_ratio": w32[0]["same_adam"]["ratio"] if w32 else None,
            "w32_same_adam_below_1": (w32[0]["same_adam"]["ratio"] < 1.0) if w32 else None,
            "w32_general_sgd_ratio": w32[0]["general_sgd"]["ratio"] if w32 else None,
            "w32_general_sgd_within_1_05": (w32[0]["general_sgd"]["ratio"] <= 1.05) if w32 else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
