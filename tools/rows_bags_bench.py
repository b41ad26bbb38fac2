#!/usr/bin/env python3
"""The worker-side cost of a pooled Pull on a sharded table (psg_route +
psg_route_bags + psg_pool_reduce) against the unpooled worker-side cost it
replaces (psg_route + psg_rows_scatter of n rows) — a record, not a test.
Needs an MI355X; prints ONE JSON line and writes it to --out.

F32, one process, W in {8, 32, 128}, n = 1 GiB / (4 W) ids spread over the whole
key range, and the shuffled skewed list of tools/rows_pooled_bench.py at that n
(80 % of the occurrences drawn from all ids, 20 % from a hot 1 %, in random
order), cut into bags of L in {4, 16, 64} consecutive positions, for ns in
{4, 8} servers over psg_server_ranges.  Each time is event-timed around the
whole sequence, one warm-up, then the median of --reps; the whole measurement
is repeated --repeats times and every repeat's ratio is kept:

  unpooled_ms   psg_route of the list, then psg_rows_scatter of n reply rows
                (what ZPullAny's worker does around its servers' replies)
  pooled_ms     psg_route of the list, psg_route_bags of its nb + 1 offsets, then
                psg_pool_reduce of ns partial frames of nb rows
                (what ZPullPooled's worker does)
  pooled_over_unpooled   the ratio of the two

Bytes per id: scatter 4 + 8 W; reduce (ns + 1) 4 W / L; bag routing ns 8 / L plus
its probes.  Condition, at W = 32, L = 16, ns = 4: pooled_over_unpooled <= 1.05
in every repeat.
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


def case(width, n, bags, servers, reps, repeats, stream):
    rng = np.random.default_rng(width)
    keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(KMAX // n)
    q = id_lists(keys, rng)["shuffled"]
    dq = psg.DeviceBuffer.from_numpy(q)
    routed, perm = psg.DeviceBuffer(n * 8), psg.DeviceBuffer(n * 4)
    src, dst = psg.DeviceBuffer(n * width * 4), psg.DeviceBuffer(n * width * 4)
    src.fill_synth(n * width, psg.F32, 7, 1, -1.0, 1.0)
    res = []
    for ns in servers:
        b, e = psg.server_ranges(ns)

        def unpooled():
            kp, ident = psg.route(dq, n, b, e, routed, perm, stream)
            assert not ident
            psg.rows_scatter(dst, src, perm, n, width * 4, stream)

        for bag in bags:
            nb = n // bag
            assert nb * bag == n
            doff = psg.DeviceBuffer.from_numpy(np.arange(nb + 1, dtype=np.uint64) * np.uint64(bag))
            dso = psg.DeviceBuffer(ns * (nb + 1) * 8)
            parts = [psg.DeviceBuffer(nb * width * 4) for _ in range(ns)]
            for j, p in enumerate(parts):
                p.fill_synth(nb * width, psg.F32, 20 + j, 1, -1.0, 1.0)
            out = psg.DeviceBuffer(nb * width * 4)

            def pooled():
                kp, ident = psg.route(dq, n, b, e, routed, perm, stream)
                psg.route_bags(doff, nb, perm, n, kp, dso, stream)
                psg.pool_reduce(out, parts, nb * width, psg.F32, stream)

            runs = []
            for _ in range(repeats):
                u = measure(unpooled, reps, stream)
                p = measure(pooled, reps, stream)
                runs.append({"unpooled_ms": u, "pooled_ms": p, "pooled_over_unpooled": p / u})
            ratios = [r["pooled_over_unpooled"] for r in runs]
            r = {"dtype": "f32", "width": width, "ids": n, "bag": bag, "bags": nb, "servers": ns, "runs": runs,
                 "pooled_over_unpooled_min": min(ratios), "pooled_over_unpooled_max": max(ratios),
                 "scatter_bytes_per_id": 4 + 8 * width, "reduce_bytes_per_id": (ns + 1) * 4 * width / bag}
            res.append(r)
            print("rows_bags_bench: case done:", json.dumps(r), file=sys.stderr, flush=True)
            for x in [doff, dso, out] + parts:
                x.free()
    for x in (dq, routed, perm, src, dst):
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--bags", default="4,16,64")
    ap.add_argument("--servers", default="4,8")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_bags_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_bags_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    ints = lambda s: [int(x) for x in s.split(",")]
    cases = []
    for w in ints(a.widths):
        cases += case(w, a.table_bytes // (4 * w), ints(a.bags), ints(a.servers), a.reps, a.repeats, stream)
    hit = [c for c in cases if (c["width"], c["bag"], c["servers"]) == (32, 16, 4)]
    line = {"bench": "rows_bags", "device": psg.device_pci_bus_id(0), "reps": a.reps, "repeats": a.repeats,
            "cases": cases,
            "pooled_over_unpooled_at_32_16_4": [r["pooled_over_unpooled"] for r in hit[0]["runs"]] if hit else None,
            "within_1_05": (hit[0]["pooled_over_unpooled_max"] <= 1.05) if hit else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text + "\n")


if __name__ == "__main__":
    main()
