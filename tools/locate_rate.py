"""Time of the pattern locate (kd_locate.hip) beside the count (kd_count.hip) on the same batch, in the same run: 10^6 patterns of
length 16 cut from 10^8 bytes of synth-text -- the workload of tools/count_rate.py -- and a second batch of few patterns with many
hits each, the 256 single bytes (total = n).  Warm context, two warm-up calls, nine timed calls, median and range; a sample of the
hit lists is checked against a scan of the text.  The share of a locate spent in its two sorts is measured by timing the sort
hook (bce_hip_sort_pairs_device) on arrays of the locate's row count, with the locate's bit windows.
One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.9 quotes it; profiles/ keeps it).

    python tools/locate_rate.py [--size 100000000] [--patterns 1000000] [--length 16] [--repeats 9] [--out FILE]
"""
import argparse
import ctypes as C
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


def timed(fn, repeats):
    out = []
    for i in range(2 + repeats):                                     # two warm-up calls
        t0 = time.perf_counter()
        fn()                                                         # complete on return
        if i >= 2:
            out.append(time.perf_counter() - t0)
    return spread(out)


def ceil_log2(v):
    return max(0, int(v - 1).bit_length())


def batch(rf, c, name, pat, off, npat, n, repeats, text, tb, ids):
    """Times count, sizing call and full locate (linear and cyclic) of one device-resident batch; spot-checks hit lists."""
    dev = pat.device
    counts = torch.zeros(npat, device=dev, dtype=torch.int64)
    hits = torch.zeros(npat + 1, device=dev, dtype=torch.int64)
    torch.cuda.synchronize()
    doc = {"batch": name, "patterns": npat}
    doc["count_device_s"] = timed(lambda: rf.count_device(pat.data_ptr(), off.data_ptr(), npat, counts.data_ptr()), repeats)
    h_off, h_pat = off.cpu().numpy(), pat.cpu().numpy().tobytes()
    for mode, cyclic in (("linear", False), ("cyclic", True)):
        total = rf.locate_device(pat.data_ptr(), off.data_ptr(), npat, hits.data_ptr(), None, 0, cyclic=cyclic)
        pos = torch.empty(max(total, 1), device=dev, dtype=torch.int32)
        torch.cuda.synchronize()
        d = {"total_hits": total}
        d["sizing_call_s"] = timed(lambda: rf.locate_device(pat.data_ptr(), off.data_ptr(), npat, hits.data_ptr(), None, 0, cyclic=cyclic), repeats)
        d["locate_device_s"] = timed(lambda: rf.locate_device(pat.data_ptr(), off.data_ptr(), npat, hits.data_ptr(), pos.data_ptr(), total, cyclic=cyclic), repeats)
        d["locate_over_count"] = d["locate_device_s"]["median"] / doc["count_device_s"]["median"]
        d["hits_per_s"] = total / d["locate_device_s"]["median"]
        h_hits, h_pos = hits.cpu().numpy(), pos.cpu().numpy()
        if cyclic:
            assert (np.diff(h_hits) == counts.cpu().numpy()).all()
        for i in ids:
            p = h_pat[int(h_off[i]):int(h_off[i + 1])]
            got = h_pos[int(h_hits[i]):int(h_hits[i + 1])].tolist()
            if len(p) == 1:
                assert got == np.flatnonzero(text == p[0]).tolist(), (name, mode, i)
                continue
            want, at = [], tb.find(p)
            while at >= 0:
                want.append(at)
                at = tb.find(p, at + 1)
            if cyclic:                                               # the hits that run across the end
                m = len(p)
                ext = tb[n - (m - 1):] + tb[:m - 1] if m > 1 else b""
                at = ext.find(p)
                while at >= 0:
                    want.append(n - (m - 1) + at)
                    at = ext.find(p, at + 1)
            assert got == want, (name, mode, i, got[:5], want[:5])
        d["hit_lists_checked_against_a_scan"] = len(ids)
        doc[mode] = d
        del pos
    rows = doc["cyclic"]["total_hits"]                               # the two sorts alone, at the row count both modes sort
    key = torch.randint(0, n, (rows,), device=dev, dtype=torch.int32)
    val = torch.randint(0, npat, (rows,), device=dev, dtype=torch.int32)
    torch.cuda.synchronize()
    lib = c.lib

    def sorts():
        c.check(lib.bce_hip_sort_pairs_device(c.h, key.data_ptr(), val.data_ptr(), rows, 0, ceil_log2(n), 9), "sort")
        if npat > 1:
            c.check(lib.bce_hip_sort_pairs_device(c.h, val.data_ptr(), key.data_ptr(), rows, 0, ceil_log2(npat), 9), "sort")

    doc["rows_sorted"] = rows
    doc["sort_bits"] = [ceil_log2(n), ceil_log2(npat) if npat > 1 else 0]
    doc["two_sorts_alone_s"] = timed(sorts, repeats)
    for mode in ("linear", "cyclic"):
        doc[mode]["share_sorting"] = doc["two_sorts_alone_s"]["median"] / doc[mode]["locate_device_s"]["median"]
    return doc


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
    tb = text.tobytes()
    t = torch.from_numpy(text).to("cuda:0")
    starts = np.random.RandomState(16).randint(0, n - m, npat)      # the batch of tools/count_rate.py
    d_starts = torch.from_numpy(starts).to("cuda:0")
    pat = t[d_starts[:, None] + torch.arange(m, device="cuda:0")[None, :]].contiguous().reshape(-1)
    off = torch.arange(npat + 1, device="cuda:0", dtype=torch.int64) * m
    singles = torch.arange(256, device="cuda:0", dtype=torch.uint8)
    soff = torch.arange(257, device="cuda:0", dtype=torch.int64)
    torch.cuda.synchronize()

    c = api._Ctx(0)
    build = []
    for _ in range(3):                                               # the first builds the context's buffers
        t0 = time.perf_counter()
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        build.append(time.perf_counter() - t0)

    doc = {"what": "kd_locate.hip beside kd_count.hip: patterns cut from synth-text (seed 1)", "device": torch.cuda.get_device_name(0),
           "n": n, "length": m, "repeats": a.repeats, "index_build_s": {"first_cold": build[0], "warm": build[1:]},
           "stored_count_figure_s": 0.00236,
           "batches": [batch(rf, c, "cut from the text", pat, off, npat, n, a.repeats, text, tb, list(range(0, npat, max(1, npat // a.checked)))),
                       batch(rf, c, "the 256 single bytes", singles, soff, 256, n, a.repeats, text, tb, [0, 32, 101, 255])]}
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
