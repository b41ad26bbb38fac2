#!/usr/bin/env python3
"""What row-wise Adagrad (psg_table_set_adagrad, k_rows_walk_rowwise) costs beside the
SGD and Adam updates of the same build, and that SGD and Adam cost what they did on
the parent commit — a record, not a test.  Needs an MI355X; prints ONE JSON line
and writes it to --out.

The tool runs itself as child processes, one per library, in the order parent,
branch, parent, branch, parent (--rounds pairs and a last parent).  --parent-lib is
the libpsgpu.so of a plain build of the parent commit; it lacks the new symbols and
is loaded with PSG_LIB_OLDER=1.  A child (--measure) reports, event-timed around the
whole call, median of --reps after two warm-up calls, F32, 1 Mi rows present, for
W = 16, 64, 256 and the optimizers its library has, alternating between them:

  strict_w{W}_{opt}_ms   psg_table_update (PUSH) of the 1 Mi ascending keys
  same_w{W}_{opt}_ms     psg_table_update_merged (PUSH), k = 4 frames on that list
  any_w{W}_{opt}_ms      psg_table_update_any (PUSH) of 4 Mi shuffled occurrences
and ..._frac: algorithmic bytes / time over the psg_copy ceiling taken in the same
child (copy_gbs: 1 GiB read + 1 GiB written).  Algorithmic bytes, U unique rows, n
occurrences in k frames: n * (8 key + 4 W gradient) + U * (8 slot + 8 W row read and
written), + U * 32 W for Adam's moments, + U * 16 for Adagrad's accumulator; the
shuffled round's sort is not counted.

The parent's range of a figure is [min, max] over the parent children: `inside`
says whether a branch child's SGD or Adam figure lies in it; misses are listed.
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
K = 4
WIDTHS = (16, 64, 256)
LR = 0.05


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

    psg.set_device(0)
    stream = psg.Stream()
    has = hasattr(psg.lib(), "psg_table_set_adagrad")  # unbound on a library of the parent commit
    opts = ("sgd", "adam", "adagrad") if has else ("sgd", "adam")
    res = {"has_adagrad": bool(has), "keys": N}
    a, b = psg.DeviceBuffer(1 << 30), psg.DeviceBuffer(1 << 30)
    xs = [timed(lambda: psg.copy(b, a, 1 << 30, stream=stream), stream) for _ in range(2 + reps)][2:]
    res["copy_gbs"] = 2 * (1 << 30) / (float(np.median(xs)) * 1e-3) / 1e9
    a.free()
    b.free()
    rng = np.random.default_rng(1)
    keys = np.uint64(2) + np.arange(N, dtype=np.uint64) * np.uint64(977)
    dk = psg.DeviceBuffer.from_numpy(keys)
    dq = psg.DeviceBuffer.from_numpy(rng.permutation(np.tile(keys, K)))
    for w in WIDTHS:
        g = psg.DeviceBuffer(K * N * w * 4)  # K frames of N rows, or K * N occurrences
        g.fill_synth(K * N * w, psg.F32, 7, 1, -1.0, 1.0)
        frames = [g.ptr + j * N * w * 4 for j in range(K)]
        tables = {}
        for opt in opts:
            t = tables[opt] = psg.Table(psg.F32, w, 0, KMAX, 0)
            if opt == "adam":
                t.set_adam(0.01)
            if opt == "adagrad":
                t.set_adagrad(0.1)
            t.assign(dk, None, N, None, None, stream)
        calls = {
            "strict": (lambda t: t.update(psg.PUSH, dk, g, None, N, LR, 0, stream), N),
            "same": (lambda t: t.update_merged(psg.PUSH, [dk] * K, frames, None, [N] * K, LR, 0, stream), K * N),
            "any": (lambda t: t.update_any(psg.PUSH, dq, g, None, K * N, LR, 0, stream), K * N),
        }
        for name, (call, n) in calls.items():
            ms = {opt: [] for opt in opts}
            for i in range(2 + reps):  # the optimizers alternate inside every repetition
                for opt in opts:
                    x = timed(lambda: call(tables[opt]), stream)
                    if i >= 2:
                        ms[opt].append(x)
            for opt in opts:
                nbytes = n * (8 + 4 * w) + N * (8 + 8 * w) + N * {"sgd": 0, "adam": 32 * w, "adagrad": 16}[opt]
                m = float(np.median(ms[opt]))
                res[f"{name}_w{w}_{opt}_ms"] = m
                res[f"{name}_w{w}_{opt}_frac"] = nbytes / (m * 1e-3) / 1e9 / res["copy_gbs"]
        for t in tables.values():
            assert t.info().size == N
            t.close()
        g.free()
    print(json.dumps(res))


def child(lib, reps):
    env = dict(os.environ)
    if lib:
        env["PSG_LIB"] = lib
        env["PSG_LIB_OLDER"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", "--reps", str(reps)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"rows_adagrad_bench: child failed ({lib}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true", help="one child's measurements with the library PSG_LIB names")
    ap.add_argument("--parent-lib", help="libpsgpu.so of the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="parent / branch pairs in front of the last parent child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_adagrad_bench.json"))
    a = ap.parse_args()
    if a.measure:
        return measure(a.reps)
    if not a.parent_lib:
        raise SystemExit("rows_adagrad_bench: --parent-lib is needed (this is a comparison with the parent)")
    order = ["parent", "branch"] * a.rounds + ["parent"]
    runs = [child(a.parent_lib if who == "parent" else None, a.reps) for who in order]
    parents = [r for who, r in zip(order, runs) if who == "parent"]
    branches = [r for who, r in zip(order, runs) if who == "branch"]
    assert not any(r["has_adagrad"] for r in parents) and all(r["has_adagrad"] for r in branches)
    unchanged = {}
    for k in sorted(parents[0]):
        if not k.endswith("_ms"):
            continue
        ps, bs = [r[k] for r in parents], [r[k] for r in branches]
        unchanged[k] = {"parent": ps, "branch": bs, "inside": [min(ps) <= x <= max(ps) for x in bs],
                        "branch_over_parent_median": float(np.median(bs) / np.median(ps))}
    misses = sorted(k for k, v in unchanged.items() if not all(v["inside"]))
    between = {k: [r[k.replace("adagrad", "sgd")] <= r[k] <= r[k.replace("adagrad", "adam")] for r in branches]
               for k in sorted(branches[0]) if k.endswith("_adagrad_ms")}
    line = {"bench": "rows_adagrad", "reps": a.reps, "order": order, "sgd_adam_against_parent": unchanged,
            "all_inside": not misses, "misses": misses, "branch": branches, "adagrad_between_sgd_and_adam": between}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
