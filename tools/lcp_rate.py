"""Time of the LCP array and its reductions (kd_lcp.hip) beside the warm index build (K1 + K2) of the same run: 10^8 bytes of
synth-text and, where tools/make_corpus.py can make it, the natural corpus (long repeats: the costly case).  Timed:
bce_hip_lcp_device at the bounds 16, 256 and 4096, bce_hip_kgrams for k = 0..33 (one pass bounded by 33 and 34 reductions) and
bce_hip_longest_repeat (a pass bounded by 4096 and one reduction).  Warm context, two warm-up calls, nine timed calls, median and
range, a host clock around calls that end in the stream wait.  The outputs are checked against the text in the same run: the
classes of k = 1 are the byte histogram and S_0, S_1 give H_0; the records of k = 2, 8, 33 are the classes of the array itself,
counted on the host; the rotations the longest repeat names agree on exactly its length.  Per bound the run also records how far
a wave's lanes diverge: the largest LCP of every 64 consecutive rows over their mean.
--worst BYTES: all-equal bytes, where every lane runs to the bound: bce_hip_lcp_device once at the bound 256, then, under a time
limit sized from that figure, once at 4096 -- the price of the work bound.
One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.11 quotes it; profiles/ keeps it).

    python tools/lcp_rate.py [--size 100000000] [--repeats 9] [--natural] [--worst 16777216] [--out FILE]
"""
import argparse
import json
import os
import subprocess
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


def rot_lcp(tb, a, b, cap):
    n, l = len(tb), 0
    while l < cap and tb[(a + l) % n] == tb[(b + l) % n]:
        l += 1
    return l


def measure(c, name, text, repeats):
    n = len(text)
    tb = text.tobytes()
    t = torch.from_numpy(text).to("cuda:0")
    lcp = torch.zeros(n, device="cuda:0", dtype=torch.int32)
    torch.cuda.synchronize()
    build = []
    for _ in range(3):                                               # the first builds the context's buffers
        t0 = time.perf_counter()
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        build.append(time.perf_counter() - t0)
    warm = min(build[1:])
    doc = {"text": name, "n": n, "index_build_s": {"first_cold": build[0], "warm": build[1:]}}
    for bound in (16, 256, 4096):
        d = timed(lambda: rf.lcp_device(bound, lcp.data_ptr()), repeats)
        d["over_warm_build"] = d["median"] / warm
        d["rows_per_s"] = n / d["median"]
        h = lcp.cpu().numpy()
        d["mean_lcp"] = float(h.mean())
        d["at_the_bound"] = int((h == bound).sum())
        assert h[0] == 0 and h.min() >= 0 and h.max() <= bound
        # wave divergence: the largest over the mean of every 64 consecutive rows (1 = a wave's lanes stop together)
        w = h[:n - n % 64].reshape(-1, 64).astype(np.float64)
        d["wave_max_over_wave_mean"] = float((w.max(axis=1) / np.maximum(w.mean(axis=1), 1.0)).mean())
        doc["lcp_device_%d" % bound] = d
    full = lcp.cpu().numpy()                                         # the array at the bound 4096
    recs = []

    def kg():
        recs[:] = rf.kgrams(range(34))

    d = timed(kg, repeats)
    d["over_warm_build"] = d["median"] / warm
    hist = np.bincount(text, minlength=256)
    assert recs[0].distinct == 1 and recs[0].max_count == n and recs[1].distinct == int((hist > 0).sum()) and recs[1].max_count == int(hist.max())
    assert tb[recs[1].max_pos] == int(hist.argmax()) or hist[tb[recs[1].max_pos]] == hist.max()
    for k in (2, 8, 33):                                             # the array's own classes on the host, from the bound-4096 pass
        starts = np.flatnonzero(np.concatenate([[True], full[1:] < k]))
        sizes = np.diff(np.concatenate([starts, [n]]))
        assert recs[k].distinct == len(starts) and recs[k].once == int((sizes == 1).sum()) and recs[k].max_count == int(sizes.max())
        piece = bytes(tb[(recs[k].max_pos + j) % n] for j in range(k))
        assert (tb + tb[:k]).count(piece) >= 1
    d["entropy_profile"] = [bce_amd.entropy_from_sums(n, recs[k].nlogn_q24, recs[k + 1].nlogn_q24) for k in range(33)]
    p = hist[hist > 0] / n
    assert abs(d["entropy_profile"][0] + float((p * np.log2(p)).sum())) < 2.0 ** -20
    d["distinct"] = [int(r.distinct) for r in recs]
    doc["kgrams_0_33"] = d
    rep = []

    def lr():
        rep[:] = rf.longest_repeat()

    d = timed(lr, repeats)
    d["over_warm_build"] = d["median"] / warm
    ln, a, b = rep
    assert ln == int(full.max()) and (ln == 0 or rot_lcp(tb, a, b, 4096) == ln)
    d["length"], d["at"] = ln, [a, b]
    doc["longest_repeat"] = d
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--natural", action="store_true", help="also the natural corpus of tools/make_corpus.py at --size")
    ap.add_argument("--worst", type=int, default=0, help="all-equal bytes of this size: the bound 256, then 4096 once")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    c = api._Ctx(0)
    doc = {"what": "kd_lcp.hip beside the warm index build (K1 + K2) of the same run", "device": torch.cuda.get_device_name(0),
           "repeats": a.repeats, "texts": [measure(c, "synth_text seed 1", bce_amd.synth_text(1, a.size), a.repeats)]}
    if a.natural:
        path = "/tmp/bce_natural_%d.bin" % a.size
        if not (os.path.exists(path) and os.path.getsize(path) == a.size):
            subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "make_corpus.py"), "--out", path,
                            "--size", str(a.size)], stdout=subprocess.DEVNULL, check=False)
        if os.path.exists(path) and os.path.getsize(path) == a.size:
            doc["texts"].append(measure(c, "natural corpus (tools/make_corpus.py)", np.fromfile(path, dtype=np.uint8), a.repeats))
        else:
            doc["natural"] = "tools/make_corpus.py could not make it here"
    if a.worst:
        n = a.worst
        t = torch.full((n,), 97, device="cuda:0", dtype=torch.uint8)
        lcp = torch.zeros(n, device="cuda:0", dtype=torch.int32)
        torch.cuda.synchronize()
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        w = {"n": n}
        for bound in (16, 256):
            t0 = time.perf_counter()
            rf.lcp_device(bound, lcp.data_ptr())
            w["lcp_device_%d_s" % bound] = time.perf_counter() - t0
        assert int(lcp[1:].min()) == 256 and int(lcp[0]) == 0
        w["expected_4096_s"] = w["lcp_device_256_s"] * 16            # the work is linear in the bound here
        if w["expected_4096_s"] < 120:                               # the time limit of this one call
            t0 = time.perf_counter()
            rf.lcp_device(4096, lcp.data_ptr())
            w["lcp_device_4096_s"] = time.perf_counter() - t0
            assert int(lcp[1:].min()) == 4096
            g = rf.kgrams([0, 1, 4096])
            assert all((r.distinct, r.max_count) == (1, n) for r in g)
        doc["worst_all_equal"] = w
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
