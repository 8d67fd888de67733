#!/usr/bin/env python3
"""Decode to the host, decode to the device, verify: median seconds in a warm context on the inputs of bench.py's decode legs.

  python tools/device_decode_timing.py --out profiles/r07_device_decode.json
  rocprofv3 --kernel-trace --stats -d DIR -o cmp --output-format csv -- python tools/device_decode_timing.py --kinds text --modes verify_device --runs 3
      (compare_kernel's own time: the kernel_stats CSV; in a run of its own, so that tracing does not touch the wall times above)

host      bce_hip_decompress_device into a caller's host buffer that exists already (bench.py's timed_decode)
device    bce_hip_decompress_to_device into a tensor that exists already (bce_amd.decompress_tensor(out=...))
verify_device / verify_host   bce_hip_verify_device against a tensor / bce_hip_verify_host against host bytes
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bce_amd  # noqa: E402

DESC = {"text": "synth-text v1 seed 1", "natural": "natural corpus v2 (tools/make_corpus.py)", "binary": "binary corpus (tools/make_binary_corpus.py)"}


def load(kind, n):
    if kind == "text":
        return bce_amd.synth_text(1, n)
    path = "/tmp/bce_%s_%d.bin" % (kind, n)
    if not (os.path.exists(path) and os.path.getsize(path) == n):
        tool = "make_corpus.py" if kind == "natural" else "make_binary_corpus.py"
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--out", path, "--size", str(n)], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return np.fromfile(path, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kinds", default="text,natural,binary")
    ap.add_argument("--modes", default="host,device,verify_device,verify_host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.size
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    ctx = bce_amd.api._Ctx(0)
    rows = []
    for kind in args.kinds.split(","):
        data = load(kind, n)
        t_in = torch.from_numpy(data).to(dev)
        torch.cuda.synchronize()
        arch = bce_amd.compress_tensor(t_in, ctx=ctx)
        hbuf = np.zeros(n + 64, dtype=np.uint8)
        dbuf = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        run = {
            "host": lambda: bce_amd.decompress_device(arch, ctx=ctx, out=hbuf) == n,
            "device": lambda: bce_amd.decompress_tensor(arch, out=dbuf, ctx=ctx).numel() == n,
            "verify_device": lambda: bce_amd.verify_tensor(arch, t_in, ctx=ctx) is None,
            "verify_host": lambda: bce_amd.verify(arch, data, ctx=ctx) is None,
        }
        row = {"workload": DESC[kind], "bytes": n, "archive_bytes": len(arch)}
        for mode in args.modes.split(","):
            assert run[mode]()                                  # warm-up: this workload's buffers
            ts = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                ok = run[mode]()
                ts.append(time.perf_counter() - t0)
                assert ok, (kind, mode)
            row[mode] = {"median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "runs": args.runs}
        if "host" in row:
            assert np.array_equal(hbuf[:n], data)
        if "device" in row:
            assert torch.equal(dbuf[:n], t_in)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del t_in, dbuf
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": "median of %d runs, warm context, one MI355X (tools/device_decode_timing.py)" % args.runs, "workloads": rows}, f, indent=1)


if __name__ == "__main__":
    main()
