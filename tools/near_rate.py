"""Patterns per second of the count with mismatches (kd_near.hip) for k = 0, 1 and 2, beside the exact count (kd_count.hip) on the
same batch: 4096 patterns of 16 bytes cut from the text with one byte altered, on 10^8 bytes of synth-text and on 32 MiB of random
bytes; each index (K1 + K2) built once.  Warm, several repeats, spread stated; a sample of the answers is checked against a brute
force over the text.  One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.17 quotes it; profiles/ keeps it).

    python tools/near_rate.py [--patterns 4096] [--length 16] [--repeats 7] [--out FILE]
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


def timed(fn, repeats, warm=2, budget_s=60.0):
    """`warm` calls, then up to `repeats` timed ones: at least three, and no further one once budget_s has gone by."""
    out, begun = [], time.perf_counter()
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        fn()                                                           # complete on return
        if i >= warm:
            out.append(time.perf_counter() - t0)
        if len(out) >= 3 and time.perf_counter() - begun > budget_s:
            break
    return spread(out)


def workload(c, name, text, npat, m, repeats, checked):
    n = len(text)
    rs = np.random.RandomState(16)
    starts = rs.randint(0, n - m, npat)
    pats = text[starts[:, None] + np.arange(m)[None, :]].copy()
    where = rs.randint(0, m, npat)
    pats[np.arange(npat), where] ^= (1 + rs.randint(0, 255, npat)).astype(np.uint8)     # one byte altered, to any other value
    t = torch.from_numpy(text).to("cuda:0")
    pat = torch.from_numpy(pats.reshape(-1)).to("cuda:0")
    off = torch.arange(npat + 1, device="cuda:0", dtype=torch.int64) * m
    out = torch.zeros(npat * 3, device="cuda:0", dtype=torch.int64)
    torch.cuda.synchronize()
    rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
    doc = {"workload": name, "n": n, "patterns": npat, "length": m}
    exact = timed(lambda: rf.count_device(pat.data_ptr(), off.data_ptr(), npat, out.data_ptr()), repeats)
    doc["count_s"] = exact
    doc["count_patterns_per_s"] = npat / exact["median"]
    counts = {}
    for k in (0, 1, 2):
        s = timed(lambda: rf.count_near_device(pat.data_ptr(), off.data_ptr(), npat, k, out.data_ptr()), repeats, warm=1 if k == 2 else 2)
        counts[k] = out[:npat * (k + 1)].cpu().numpy().reshape(npat, k + 1)
        doc["count_near_k%d_s" % k] = s
        doc["count_near_k%d_patterns_per_s" % k] = npat / s["median"]
        doc["count_near_k%d_mean_hits" % k] = float(counts[k].sum(axis=1).mean())
        print("%s: k = %d, %.4f s a call" % (name, k, s["median"]), file=sys.stderr, flush=True)
    ext = np.concatenate([text, text[:m]])
    for i in range(0, npat, max(1, npat // checked)):                # the brute force: distances of pattern i at every position
        d = np.zeros(n, dtype=np.uint8)
        for j in range(m):
            d += ext[j:j + n] != pats[i, j]
        for k in (0, 1, 2):
            assert counts[k][i].tolist() == np.bincount(d[d <= k], minlength=k + 1)[:k + 1].tolist(), (name, i, k)
    doc["answers_checked_against_a_brute_force"] = checked
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=4096)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--checked", type=int, default=4)
    ap.add_argument("--text-size", type=int, default=100000000)
    ap.add_argument("--rand-size", type=int, default=32 << 20)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    c = api._Ctx(0)
    docs = []
    for name, text in (("synth-text seed 1", bce_amd.synth_text(1, a.text_size)), ("random bytes seed 2", bce_amd.synth_rand(2, a.rand_size))):
        docs.append(workload(c, name, text, a.patterns, a.length, a.repeats, a.checked))
        print(json.dumps(docs[-1]), flush=True)
    doc = {"what": "kd_near.hip: bce_hip_count_near_device for k = 0, 1, 2 beside bce_hip_count_device, one warm context, patterns cut from the text with one byte altered",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "workloads": docs}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
