#!/usr/bin/env python3
"""The two worker kernels of a mean over a sharded bag against the kernels they
stand beside — a record, not a test.  Needs an MI355X; prints ONE JSON line and
writes it to --out.

F32, one process, W = 32, bags of L = 16, ns = 4 partial frames, at the size of
tools/rows_bags_bench.py: n = 1 GiB / (4 W) ids, nb = n / L bags, so a frame
holds nb * W floats.  Each time is event-timed around --inner back-to-back calls
(one call is a fraction of a millisecond) and divided by it, one warm-up, then
the median of --reps; the whole measurement is repeated --repeats times, the
two sides of a comparison alternating, and every repeat's ratio is kept:

  reduce_ms        psg_pool_reduce of the ns frames (the sum fold ZPullPooled runs)
  reduce_mean_ms   psg_pool_reduce_mean of the same frames with nb + 1 offsets
  copy_ms          psg_copy of nb * W floats
  scale_mean_ms    psg_pool_scale_mean of the same floats with the same offsets
  gather_ms        psg_rows_gather of the n f32 weights by the perm psg_route gave
                   for the shuffled skewed list (4-B rows: a whole line per word)

Byte models per bag: reduce (ns + 1) 4 W, reduce_mean that + 16; copy 8 W,
scale_mean that + 16.  Conditions, in every repeat: reduce_mean_ms / reduce_ms
<= model ratio * 1.05, and scale_mean_ms / copy_ms <= model ratio * 1.05.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import psg  # noqa: E402
from rows_pooled_bench import id_lists, measure  # noqa: E402

KMAX = (1 << 64) - 1
ALLOWANCE = 1.05


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--bag", type=int, default=16)
    ap.add_argument("--servers", type=int, default=4)
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_bags_modes_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_bags_modes_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    w, bag, ns = a.width, a.bag, a.servers
    n = a.table_bytes // (4 * w)
    nb = n // bag
    assert nb * bag == n
    count = nb * w
    doff = psg.DeviceBuffer.from_numpy(np.arange(nb + 1, dtype=np.uint64) * np.uint64(bag))
    parts = [psg.DeviceBuffer(count * 4) for _ in range(ns)]
    for j, p in enumerate(parts):
        p.fill_synth(count, psg.F32, 20 + j, 1, -1.0, 1.0)
    out, out_mean = psg.DeviceBuffer(count * 4), psg.DeviceBuffer(count * 4)

    def times(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return measure(run, a.reps, stream) / a.inner

    reduce = lambda: psg.pool_reduce(out, parts, count, psg.F32, stream)
    reduce_mean = lambda: psg.pool_reduce_mean(out_mean, parts, doff, nb, w, psg.F32, stream)
    copy = lambda: psg.copy(out, parts[0], count * 4, stream=stream)
    scale = lambda: psg.pool_scale_mean(out_mean, parts[0], doff, nb, w, stream)

    # what is timed is what is defined: every bag holds `bag` ids
    reduce(), reduce_mean()
    stream.sync()
    s, m = out.download(np.float32, count), out_mean.download(np.float32, count)
    assert np.array_equal((s / np.float32(bag)).view(np.uint32), m.view(np.uint32)), "reduce_mean is not the fold over L"
    scale()
    stream.sync()
    g = parts[0].download(np.float32, count)
    assert np.array_equal((g / np.float32(bag)).view(np.uint32), out_mean.download(np.uint32, count)), "scale_mean"

    model_reduce = ((ns + 1) * 4 * w + 16) / ((ns + 1) * 4 * w)
    model_scale = (8 * w + 16) / (8 * w)
    runs = []
    for _ in range(a.repeats):
        r, rm, c, sm = times(reduce), times(reduce_mean), times(copy), times(scale)
        runs.append({"reduce_ms": r, "reduce_mean_ms": rm, "reduce_mean_over_reduce": rm / r,
                     "copy_ms": c, "scale_mean_ms": sm, "scale_mean_over_copy": sm / c})
        print("rows_bags_modes_bench: repeat done:", json.dumps(runs[-1]), file=sys.stderr, flush=True)

    # the weights of a permuted route: one gather of 4-B rows
    rng = np.random.default_rng(w)
    keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(KMAX // n)
    dq = psg.DeviceBuffer.from_numpy(id_lists(keys, rng)["shuffled"])
    routed, perm = psg.DeviceBuffer(n * 8), psg.DeviceBuffer(n * 4)
    b, e = psg.server_ranges(ns)
    _, ident = psg.route(dq, n, b, e, routed, perm, stream)
    assert not ident
    wts, wts_routed = psg.DeviceBuffer(n * 4), psg.DeviceBuffer(n * 4)
    wts.fill_synth(n, psg.F32, 9, 1, -1.0, 1.0)
    gather_ms = [times(lambda: psg.rows_gather(wts_routed, wts, perm, n, 4, stream)) for _ in range(a.repeats)]

    rr = [x["reduce_mean_over_reduce"] for x in runs]
    sr = [x["scale_mean_over_copy"] for x in runs]
    line = {"bench": "rows_bags_modes", "device": psg.device_pci_bus_id(0), "dtype": "f32", "width": w, "bag": bag,
            "servers": ns, "ids": n, "bags": nb, "inner": a.inner, "reps": a.reps, "repeats": a.repeats, "runs": runs,
            "reduce_bytes_per_bag": (ns + 1) * 4 * w, "reduce_mean_bytes_per_bag": (ns + 1) * 4 * w + 16,
            "copy_bytes_per_bag": 8 * w, "scale_mean_bytes_per_bag": 8 * w + 16,
            "reduce_mean_bound": model_reduce * ALLOWANCE, "scale_mean_bound": model_scale * ALLOWANCE,
            "reduce_mean_within_bound": max(rr) <= model_reduce * ALLOWANCE,
            "scale_mean_within_bound": max(sr) <= model_scale * ALLOWANCE,
            "weights_gather_ms": gather_ms, "weights_gather_bytes_per_id_model": 12}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text + "\n")


if __name__ == "__main__":
    main()
