#!/usr/bin/env python3
"""The worker's routing pass and row copies (psg_route, psg_rows_gather,
psg_rows_scatter) — a record, not a test.  Needs an MI355X; prints ONE JSON line
and writes it to --out.

F32, W in {8, 32, 128}, n = 1 GiB / (4 W) keys spread over the whole key space,
two servers; the lists of rows_any_bench.py: the distinct keys in a shuffled
order, and as many occurrences drawn Zipf(1.05) over them.  Every time is
event-timed around the whole call, median of --reps.  Per width and list:

  gather, scatter  against psg_copy of n * row_bytes (the same 2 * n * row_bytes
                   of traffic; the best of its launch shapes) in the same process:
                   fraction = copy / kernel
  route            against one stable 8-bit pass, psg_sort_pairs_u64(bits = 8),
                   on the same n (the same bytes; that export also allocates and
                   frees its scratch and copies the result back inside the timed
                   call, psg_route keeps its scratch)
  identity         psg_route of the sorted list (one pass, 8 B a key) against
                   psg_copy of 8 n bytes
  end to end       route + gather + handle_any(Push) on two half-range tables
                   against handle_any(Push) of the list as it is on one table
                   over the whole range; the same for a PushPull, with the
                   scatter of the replies
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
HALF = KMAX // 2


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


def med(fn, reps, stream):
    fn()  # warm-up
    return median([timed(fn, stream) for _ in range(reps)])


def row_keys(n):
    return np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(KMAX // n)


def zipf_ids(n_table, count, rng, s=1.05):
    cdf = np.cumsum(np.arange(1, n_table + 1, dtype=np.float64) ** -s)
    cdf /= cdf[-1]
    return np.minimum(np.searchsorted(cdf, rng.random(count)), n_table - 1)


def best_copy_ms(dst, src, nbytes, reps, stream):
    nbytes -= nbytes % 16
    return min(med(lambda: psg.copy(dst, src, nbytes, u, b, stream), reps, stream) for u, b in ((4, 4), (4, 8), (8, 8)))


def one_list(width, keys, distinct, reps, stream, b, e):
    n, rb = len(keys), width * 4
    nv = n * width
    dk = psg.DeviceBuffer.from_numpy(keys)
    rk, perm = psg.DeviceBuffer(n * 8), psg.DeviceBuffer(n * 4)
    vals, rvals, rout, out = (psg.DeviceBuffer(nv * 4) for _ in range(4))
    vals.fill_synth(nv, psg.F32, 7, 0, 0.0, 16.0)
    res = {"n": n}
    pos, ident = psg.route(dk, n, b, e, rk, perm, stream)
    assert not ident
    res["route_ms"] = med(lambda: psg.route(dk, n, b, e, rk, perm, stream), reps, stream)
    sk, sv = psg.DeviceBuffer(n * 8), psg.DeviceBuffer(n * 4)

    def sort_pass():
        psg.memcpy_d2d(sk, dk, n * 8, stream)
        psg.sort_pairs_u64(sk, sv, n, 8, stream)

    copy_in = med(lambda: psg.memcpy_d2d(sk, dk, n * 8, stream), reps, stream)
    res["sort_pass_ms"] = med(sort_pass, reps, stream) - copy_in
    res["route_over_sort_pass"] = res["route_ms"] / res["sort_pass_ms"]
    sorted_keys = psg.DeviceBuffer.from_numpy(np.sort(keys))
    assert psg.route(sorted_keys, n, b, e, rk, perm, stream)[1]
    res["identity_ms"] = med(lambda: psg.route(sorted_keys, n, b, e, rk, perm, stream), reps, stream)
    res["copy_8n_ms"] = best_copy_ms(sk, sorted_keys, n * 8, reps, stream)
    res["identity_over_copy"] = res["identity_ms"] / res["copy_8n_ms"]
    psg.route(dk, n, b, e, rk, perm, stream)  # perm again: the identity call left it alone, but be plain
    res["gather_ms"] = med(lambda: psg.rows_gather(rvals, vals, perm, n, rb, stream), reps, stream)
    res["scatter_ms"] = med(lambda: psg.rows_scatter(out, rvals, perm, n, rb, stream), reps, stream)
    res["copy_rows_ms"] = best_copy_ms(out, vals, n * rb, reps, stream)
    res["gather_fraction_of_copy"] = res["copy_rows_ms"] / res["gather_ms"]
    res["scatter_fraction_of_copy"] = res["copy_rows_ms"] / res["scatter_ms"]
    res["gather_over_copy"] = res["gather_ms"] / res["copy_rows_ms"]
    res["scatter_over_copy"] = res["scatter_ms"] / res["copy_rows_ms"]
    for x in (sk, sv, sorted_keys):
        x.free()

    # end to end: two half-range tables against one
    full = psg.DeviceBuffer.from_numpy(distinct)
    m = len(distinct)
    cut = int(np.searchsorted(distinct, np.uint64(HALF)))
    pair = [psg.Table(psg.F32, width, 0, HALF, cut), psg.Table(psg.F32, width, HALF, KMAX, m - cut)]
    whole = psg.Table(psg.F32, width, 0, KMAX, m)
    scratch = psg.DeviceBuffer(m * rb)
    pair[0].handle(psg.PULL, full.ptr, None, scratch, cut, stream)  # inserts every key
    pair[1].handle(psg.PULL, full.ptr + cut * 8, None, scratch, m - cut, stream)
    whole.handle(psg.PULL, full, None, scratch, m, stream)
    scratch.free()
    full.free()

    def routed(flags):
        p, _ = psg.route(dk, n, b, e, rk, perm, stream)
        psg.rows_gather(rvals, vals, perm, n, rb, stream)
        for s, t in enumerate(pair):
            lo, cnt = int(p[s]), int(p[s + 1] - p[s])
            t.handle_any(flags, rk.ptr + lo * 8, rvals.ptr + lo * rb, rout.ptr + lo * rb if flags & psg.PULL else None,
                         cnt, stream)
        if flags & psg.PULL:
            psg.rows_scatter(out, rout, perm, n, rb, stream)

    pp = psg.PUSH | psg.PULL
    res["routed_push_ms"] = med(lambda: routed(psg.PUSH), reps, stream)
    res["whole_push_ms"] = med(lambda: whole.handle_any(psg.PUSH, dk, vals, None, n, stream), reps, stream)
    res["routed_pushpull_ms"] = med(lambda: routed(pp), reps, stream)
    res["whole_pushpull_ms"] = med(lambda: whole.handle_any(pp, dk, vals, out, n, stream), reps, stream)
    res["routed_over_whole_push"] = res["routed_push_ms"] / res["whole_push_ms"]
    res["routed_over_whole_pushpull"] = res["routed_pushpull_ms"] / res["whole_pushpull_ms"]
    for t in pair + [whole]:
        t.close()
    for x in (dk, rk, perm, vals, rvals, rout, out):
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_route_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_route_bench: no GPU (this is a measurement: it does not fall back)")
    psg.set_device(0)
    stream = psg.Stream()
    rng = np.random.default_rng(5)
    b, e = psg.server_ranges(2)
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        n = a.table_bytes // (4 * w)
        distinct = row_keys(n)
        c = {"dtype": "f32", "width": w, "row_bytes": 4 * w, "servers": 2}
        c["shuffled"] = one_list(w, rng.permutation(distinct), distinct, a.reps, stream, b, e)
        c["zipf"] = one_list(w, distinct[rng.permutation(n)[zipf_ids(n, n, rng)]], distinct, a.reps, stream, b, e)
        cases.append(c)
        print("rows_route_bench: case done:", json.dumps(c), file=sys.stderr, flush=True)
    ratios = {k: max(c[l][k] for c in cases for l in ("shuffled", "zipf"))
              for k in ("gather_over_copy", "scatter_over_copy", "route_over_sort_pass", "identity_over_copy")}
    line = {"bench": "rows_route", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases,
            "worst_ratios": ratios, "all_within_1p5": all(v <= 1.5 for v in ratios.values())}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
