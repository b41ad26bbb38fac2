#!/usr/bin/env python3
"""What seeded initial rows (psg_table_set_init) cost, and that a table without an
initializer costs what it did — a record, not a test.  Needs an MI355X; prints
ONE JSON line and writes it to --out.

The tool runs itself as child processes, one per library, in the order parent,
branch, parent, branch, parent (--rounds pairs and a last parent).  --parent-lib is the libpsgpu.so of a plain build
of the parent commit, e.g.
    git worktree add /tmp/parent <parent commit>
    make -C /tmp/parent/parameter-server_amd -j16 psgpu
    tools/rows_init_bench.py --parent-lib /tmp/parent/parameter-server_amd/lib/libpsgpu.so
It lacks the three new symbols; the children load it with PSG_LIB_OLDER=1, under
which the binding leaves a missing symbol unbound.  The branch is this tree's
library.  A child (--measure) reports,
event-timed around the whole call, median of --reps, F32:

  insert_w{W}_ms         psg_table_assign(rows = NULL) of 1 Mi new ascending keys into
                         an empty table, W = 32 and 128, NO initializer
  lookup_w32_abs{P}_ms   psg_table_lookup of 1 Mi shuffled ids, P % of them absent
                         (P = 0, 10, 100), table of 1 Mi rows, NO initializer
  pooled_w32_abs{P}_ms   psg_table_lookup_pooled of the same ids in bags of 16
and, where the library has psg_table_set_init (the branch), the same calls on a
table WITH an initializer (..._init_ms) and the generator alone:
  fill_w{W}_init_ms      psg_init_rows of 1 Mi rows (the fill kernel and one
                         synchronisation); fill_w{W}_zero_ms: psg_memset of the same
                         bytes; fill_w{W}_init_gbs: bytes written / time
The memset is NOT the code the fill replaces: that is k_rows_move's scatter of
zero rows inside insert_missing, which no call reaches on its own.  What the
replacement costs in place is insert_w{W}_init_ms against insert_w{W}_ms of the
same child (init_over_plain below).
The parent's range of a quantity is [min, max] over the parent children,
as it is: `inside` says whether a branch child's no-initializer figure lies in
it, and a figure outside it is reported as a miss (all_inside false).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))

KMAX = (1 << 64) - 1
N = 1 << 20
SEED, LO, HI = 12345, -0.05, 0.05


def measure(reps):
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

    def med(fn, stream, before=None):
        xs = []
        for i in range(2 + reps):  # two warm-up rounds
            if before:
                before()
            x = timed(fn, stream)
            if i >= 2:
                xs.append(x)
        return float(np.median(xs))

    psg.set_device(0)
    stream = psg.Stream()
    has_init = hasattr(psg.lib(), "psg_table_set_init")  # unbound on a library of the parent commit
    rng = np.random.default_rng(1)
    keys = np.uint64(2) + np.arange(N, dtype=np.uint64) * np.uint64(977)  # key + 1 is never a key
    dk = psg.DeviceBuffer.from_numpy(keys)
    res = {"has_init": bool(has_init), "keys": N}
    for init in ([False, True] if has_init else [False]):
        tag = "_init" if init else ""
        for w in (32, 128):
            t = psg.Table(psg.F32, w, 0, KMAX, 0)
            if init:
                t.set_init(SEED, LO, HI)
            res[f"insert_w{w}{tag}_ms"] = med(lambda: t.assign(dk, None, N, None, None, stream), stream, before=t.clear)
            assert t.info().size == N
            t.close()
        w = 32
        t = psg.Table(psg.F32, w, 0, KMAX, 0)
        if init:
            t.set_init(SEED, LO, HI)
        t.assign(dk, None, N, None, None, stream)
        out, fnd = psg.DeviceBuffer(N * w * 4), psg.DeviceBuffer(N)
        offs = psg.DeviceBuffer.from_numpy(np.arange(N // 16 + 1, dtype=np.uint64) * np.uint64(16))
        for pct in (0, 10, 100):
            na = N * pct // 100
            q = keys.copy()
            q[rng.choice(N, na, replace=False)] += np.uint64(1)
            dq = psg.DeviceBuffer.from_numpy(rng.permutation(q))
            res[f"lookup_w32_abs{pct}{tag}_ms"] = med(lambda: t.lookup(dq, out, fnd, N, stream), stream)
            res[f"pooled_w32_abs{pct}{tag}_ms"] = med(lambda: t.lookup_pooled(dq, offs, out, N, N // 16, stream), stream)
            dq.free()
        assert t.info().size == N
        t.close()
        for b in (out, fnd, offs):
            b.free()
    if has_init:
        for w in (32, 128):
            buf = psg.DeviceBuffer(N * w * 4)
            res[f"fill_w{w}_init_ms"] = med(lambda: psg.init_rows(buf, dk, N, psg.F32, w, SEED, LO, HI, stream), stream)

            def zero():
                psg._call("psg_memset", buf.ptr, 0, N * w * 4, psg._s(stream))
                stream.sync()

            res[f"fill_w{w}_zero_ms"] = med(zero, stream)
            res[f"fill_w{w}_init_gbs"] = N * w * 4 / (res[f"fill_w{w}_init_ms"] * 1e-3) / 1e9
            res[f"fill_w{w}_zero_gbs"] = N * w * 4 / (res[f"fill_w{w}_zero_ms"] * 1e-3) / 1e9
            buf.free()
    print(json.dumps(res))


def child(lib, reps):
    env = dict(os.environ)
    if lib:
        env["PSG_LIB"] = lib
        env["PSG_LIB_OLDER"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", "--reps", str(reps)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"rows_init_bench: child failed ({lib}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true", help="one child's measurements with the library PSG_LIB names")
    ap.add_argument("--parent-lib", help="libpsgpu.so of the parent commit")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="parent / branch pairs in front of the last parent child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_init_bench.json"))
    a = ap.parse_args()
    if a.measure:
        return measure(a.reps)
    if not a.parent_lib:
        raise SystemExit("rows_init_bench: --parent-lib is needed (this is a comparison with the parent)")
    order = ["parent", "branch"] * a.rounds + ["parent"]
    runs = [child(a.parent_lib if who == "parent" else None, a.reps) for who in order]
    parents = [r for who, r in zip(order, runs) if who == "parent"]
    branches = [r for who, r in zip(order, runs) if who == "branch"]
    assert not any(r["has_init"] for r in parents) and all(r["has_init"] for r in branches)
    no_init = {}
    for k in sorted(parents[0]):
        if not k.endswith("_ms"):
            continue
        ps, bs = [r[k] for r in parents], [r[k] for r in branches]
        no_init[k] = {"parent": ps, "branch": bs, "inside": [min(ps) <= b <= max(ps) for b in bs],
                      "branch_over_parent_median": float(np.median(bs) / np.median(ps))}
    misses = sorted(k for k, v in no_init.items() if not all(v["inside"]))
    with_init = [{k: v for k, v in br.items() if "_init" in k or k.startswith("fill_")} for br in branches]
    over = [{k[:-len("_init_ms")]: br[k] / br[k.replace("_init_ms", "_ms")] for k in br
             if k.endswith("_init_ms") and k.replace("_init_ms", "_ms") in br} for br in branches]
    line = {"bench": "rows_init", "reps": a.reps, "order": order, "no_initializer": no_init,
            "all_inside": not misses, "misses": misses, "with_initializer": with_init, "init_over_plain": over}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
