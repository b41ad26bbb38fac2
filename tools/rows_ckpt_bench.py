#!/usr/bin/env python3
"""The row table's assign and export (psg_table_assign / psg_table_export) and
its checkpoint files against the calls that move the same rows — a record, not
a test.  Needs an MI355X; prints ONE JSON line and writes it to --out.

For F32 and W in {8, 32, 128}, with n = 1 GiB / (4 W) keys — 1 GiB of rows
resident, well past the 256 MiB Infinity Cache — and the full list of present
keys, each case reports, event-timed around the whole call, median of --reps:

  assign_ms        psg_table_assign, rows only      bytes per key 16 + 8 W
  push_ms          yardstick psg_table_handle(PSG_PUSH) of that list    16 + 12 W
  assign_mom_ms    psg_table_assign with m and v    16 + 40 W
  adam_ms          yardstick psg_table_update(PSG_PUSH), Adam           16 + 44 W
  export_ms        psg_table_export of keys, rows, m and v, the whole table in
                   one call (two copies inside HBM and the moment kernel)
  copy_ms          yardstick psg_copy of as many bytes as export writes
  *_over_*         the ratio of the times; *_bytes_ratio the one the bytes predict

At W = 32 the two conditions
  assign_over_push       must be <= 1.05
  assign_mom_over_adam   must be <= 1.05

--file-rows > 0 also runs tests/_bin/row_ckpt_file (ps::SaveRowTable /
LoadRowTable to a file under --file-dir) with W = 32 and reports its wall
times: the disk is the limit there, not the GPU.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parameter-server_amd", "python"))
import psg  # noqa: E402

KMAX = (1 << 64) - 1
LR = 0.01


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


def case(width, n, reps, stream):
    nvals = n * width
    keys = np.uint64(1) + np.arange(n, dtype=np.uint64) * np.uint64(977)
    dk = psg.DeviceBuffer.from_numpy(keys)
    rows = psg.DeviceBuffer(nvals * 4)
    rows.fill_synth(nvals, psg.F32, 7, 1, -1.0, 1.0)
    m, v = psg.DeviceBuffer(nvals * 8), psg.DeviceBuffer(nvals * 8)
    m.fill_synth(nvals, psg.F64, 8, 1, -1.0, 1.0)
    v.fill_synth(nvals, psg.F64, 9, 1, 0.0, 1e-3)
    res = {"dtype": "f32", "width": width, "keys": n, "table_bytes": nvals * 4}

    t = psg.Table(psg.F32, width, 0, KMAX, n)
    t.assign(dk, rows, n, None, None, stream)  # the table holds every key before anything is timed
    res["assign_ms"] = measure(lambda i: t.assign(dk, rows, n, None, None, stream), reps, stream)
    res["push_ms"] = measure(lambda i: t.handle(psg.PUSH, dk, rows, None, n, stream), reps, stream)
    t.set_adam(LR)
    res["assign_mom_ms"] = measure(lambda i: t.assign(dk, rows, n, m, v, stream), reps, stream)
    res["adam_ms"] = measure(lambda i: t.update(psg.PUSH, dk, rows, None, n, LR, i, stream), reps, stream)

    ko, ro = psg.DeviceBuffer(n * 8), psg.DeviceBuffer(nvals * 4)
    res["export_ms"] = measure(lambda i: t.export(0, n, ko, ro, m, v, stream), reps, stream)
    out_bytes = n * 8 + nvals * 20
    res["export_bytes_written"] = out_bytes
    cb = out_bytes // 16 * 16
    src, dst = psg.DeviceBuffer(cb), psg.DeviceBuffer(cb)
    res["copy_ms"] = measure(lambda i: psg.copy(dst, src, cb, 4, 8, stream), reps, stream)
    for b in (src, dst, ko, ro, m, v, rows, dk):
        b.free()
    t.close()

    res["assign_over_push"] = res["assign_ms"] / res["push_ms"]
    res["assign_over_push_bytes_ratio"] = (16 + 8 * width) / (16 + 12 * width)
    res["assign_mom_over_adam"] = res["assign_mom_ms"] / res["adam_ms"]
    res["assign_mom_over_adam_bytes_ratio"] = (16 + 40 * width) / (16 + 44 * width)
    res["export_over_copy"] = res["export_ms"] / res["copy_ms"]
    res["export_gbs"] = 2 * out_bytes / (res["export_ms"] * 1e-3) / 1e9
    res["copy_gbs"] = 2 * cb / (res["copy_ms"] * 1e-3) / 1e9
    return res


def file_case(rows, directory):
    exe = os.path.join(ROOT, "tests", "_bin", "row_ckpt_file")
    with tempfile.TemporaryDirectory(dir=directory) as d:
        r = subprocess.run([exe, "32", str(rows), os.path.join(d, "table"), "1", "timing"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("rows_ckpt_bench: row_ckpt_file failed: " + r.stderr[-2000:])
    f = dict(re.findall(r"(\w+) ([\d.]+)", r.stdout))
    size, save_ms, load_ms = int(f["file_bytes"]), float(f["save_ms"]), float(f["load_ms"])
    return {"width": 32, "rows": rows, "moments": True, "file_bytes": size, "chunk_bytes": int(f["chunk_bytes"]),
            "save_ms": save_ms, "load_ms": load_ms, "save_gbs": size / save_ms / 1e6, "load_gbs": size / load_ms / 1e6}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", default="8,32,128")
    ap.add_argument("--table-bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--file-rows", type=int, default=(1 << 30) // (4 * 32))
    ap.add_argument("--file-dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_ckpt_bench.json"))
    a = ap.parse_args()
    if psg.device_count() < 1:
        raise SystemExit("rows_ckpt_bench: no GPU (this is a measurement: it does not fall back)")
    files = file_case(a.file_rows, a.file_dir) if a.file_rows > 0 else None  # a process of its own, before this one holds HBM
    psg.set_device(0)
    stream = psg.Stream()
    cases = []
    for w in (int(x) for x in a.widths.split(",")):
        cases.append(case(w, a.table_bytes // (4 * w), a.reps, stream))
        print("rows_ckpt_bench: case done:", json.dumps(cases[-1]), file=sys.stderr, flush=True)
    w32 = [c for c in cases if c["width"] == 32]
    line = {"bench": "rows_ckpt", "device": psg.device_pci_bus_id(0), "reps": a.reps, "cases": cases, "files": files,
            "w32_assign_over_push": w32[0]["assign_over_push"] if w32 else None,
            "w32_assign_within_1_05": (w32[0]["assign_over_push"] <= 1.05) if w32 else None,
            "w32_assign_mom_over_adam": w32[0]["assign_mom_over_adam"] if w32 else None,
            "w32_assign_mom_within_1_05": (w32[0]["assign_mom_over_adam"] <= 1.05) if w32 else None}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
