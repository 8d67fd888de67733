"""Queries per second of the pattern count (kd_count.hip): 10^6 patterns of length 16 cut from 10^8 bytes of synth-text, the index
(K1 + K2) built once and timed apart.  Warm, several repeats, spread stated; a sample of the counts is checked against a scan of
the text.  One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.8 quotes it; profiles/ keeps it).

    python tools/count_rate.py [--size 100000000] [--patterns 1000000] [--length 16] [--repeats 9] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bce_amd  # noqa: E402
from bce_amd import api  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000000)
    ap.add_argument("--patterns", type=int, default=1000000)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--checked", type=int, default=24)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    n, npat, m = a.size, a.patterns, a.length
    text = bce_amd.synth_text(1, n)
    t = torch.from_numpy(text).to("cuda:0")
    starts = np.random.RandomState(16).randint(0, n - m, npat)
    d_starts = torch.from_numpy(starts).to("cuda:0")
    pat = t[d_starts[:, None] + torch.arange(m, device="cuda:0")[None, :]].contiguous().reshape(-1)
    off = torch.arange(npat + 1, device="cuda:0", dtype=torch.int64) * m
    out = torch.zeros(npat, device="cuda:0", dtype=torch.int64)
    torch.cuda.synchronize()

    c = api._Ctx(0)
    build = []
    for _ in range(3):                                               # the first builds the context's buffers
        t0 = time.perf_counter()
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        build.append(time.perf_counter() - t0)
    st = api.stats_of(c)

    dev = []
    for i in range(2 + a.repeats):                                   # two warm-up calls
        t0 = time.perf_counter()
        rf.count_device(pat.data_ptr(), off.data_ptr(), npat, out.data_ptr())      # complete on return
        if i >= 2:
            dev.append(time.perf_counter() - t0)
    counts = out.cpu().numpy().astype(np.uint64)

    h_pat, h_off, h_out = pat.cpu().numpy(), off.cpu().numpy().astype(np.uint64), np.zeros(npat, dtype=np.uint64)
    host = []
    for i in range(2 + a.repeats):
        t0 = time.perf_counter()
        c.check(c.lib.bce_hip_count(c.h, h_pat.ctypes.data, h_off.ctypes.data, npat, h_out.ctypes.data), "bce_hip_count")
        if i >= 2:
            host.append(time.perf_counter() - t0)
    assert (h_out == counts).all()

    tb = text.tobytes()
    for i in range(0, npat, max(1, npat // a.checked)):              # cyclic == linear here unless a match runs across the end
        p = tb[starts[i]:starts[i] + m]
        want, at = 0, tb.find(p)
        while at >= 0:
            want, at = want + 1, tb.find(p, at + 1)
        want += api.seam_count(tb[:m - 1], tb[n - (m - 1):], p)
        assert int(counts[i]) == want, (i, int(counts[i]), want)

    gathers = npat * m * 8 * 2
    d, h = spread(dev), spread(host)
    doc = {"what": "kd_count.hip: cyclic counts of patterns cut from synth-text (seed 1)", "device": torch.cuda.get_device_name(0),
           "n": n, "patterns": npat, "length": m, "repeats": a.repeats,
           "index_build_s": {"first_cold": build[0], "warm": build[1:], "k1_s": st["t_bwt"], "k2_s": st["t_planes"]},
           "count_device_s": d, "count_host_buffers_s": h,
           "queries_per_s_device": npat / d["median"], "queries_per_s_host_buffers": npat / h["median"],
           "granule_gathers": gathers, "dependent_levels_per_pattern": m * 8,
           "gathers_per_s_device": gathers / d["median"], "call_ns_over_chain_length": d["median"] / (m * 8) * 1e9,
           "counts_checked_against_a_scan": a.checked, "mean_count": float(counts.mean())}
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
