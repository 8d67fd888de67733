"""Time of the list of the most frequent k-grams (kd_lcp.hip: bce_hip_top_kgrams_device) beside the warm index build (K1 + K2) and
the one-k bce_hip_kgrams of the same run: 10^8 bytes of synth-text and, where tools/make_corpus.py can make it, the natural corpus.
Timed: k = 4, 8, 32 with limit = 100 and 65 536, entries and bytes into device memory.  Warm context, two warm-up calls, nine timed
calls, median and range, a host clock around calls that end in the stream wait.  Beside each time: the candidates the threshold
bin lets through (worked out from the call's own size_hist with the rule of top_step.h -- the number the sort runs on), the
threshold and top bins, the key bits sorted, and the distinct k-grams.  The outputs are checked in the same run: distinct and the
first count against bce_hip_kgrams, the counts descending with ties in row order, every k-gram's bytes the cyclic cut at its
position, and the first entries' counts against a count of the bytes in the text on the host.
One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.14 quotes it; profiles/ keeps it).

    python tools/top_rate.py [--size 100000000] [--repeats 9] [--natural] [--out FILE]
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

KS = (4, 8, 32)
LIMITS = (100, 65536)


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


def threshold(hist, want):
    """top_step.h's rule: the largest bin t with sum(hist[t:]) >= want -> (t, candidates, top bin, key bits)."""
    top = max(b for b in range(32) if hist[b])
    t = max(b for b in range(32) if sum(hist[b:]) >= want)
    return t, sum(hist[t:]), top, ((1 << (top + 1)) - 1 - (1 << t)).bit_length()


def measure(c, name, text, repeats):
    n = len(text)
    t = torch.from_numpy(text).to("cuda:0")
    torch.cuda.synchronize()
    build = []
    for _ in range(3):                                               # the first builds the context's buffers
        t0 = time.perf_counter()
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        build.append(time.perf_counter() - t0)
    warm = min(build[1:])
    doc = {"text": name, "n": n, "index_build_s": {"first_cold": build[0], "warm": build[1:]}, "cases": []}
    for k in KS:
        rec = []

        def kg():
            rec[:] = [rf.kgrams(k)]

        one_k = timed(kg, repeats)
        for limit in LIMITS:
            ent = torch.zeros((limit, 3), dtype=torch.int32, device="cuda:0")
            raw = torch.zeros(limit * k, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            res = []

            def top():
                res[:] = rf.top_kgrams_device(k, limit, ent.data_ptr(), raw.data_ptr(), limit * k)

            d = timed(top, repeats)
            found, distinct, hist = res
            e = ent.cpu().numpy().astype(np.int64)[:found]
            g = raw.cpu().numpy()[:found * k].reshape(found, k)
            assert distinct == rec[0].distinct and found == min(limit, distinct) and int(e[0, 0]) == rec[0].max_count and sum(hist) == distinct
            assert (np.diff(e[:, 0]) <= 0).all() and (np.diff(e[:, 1])[np.diff(e[:, 0]) == 0] > 0).all()      # counts descending, ties in row order
            idx = (e[:, 2][:, None] + np.arange(k)[None, :]) % n
            assert np.array_equal(text[idx], g)                                                              # the bytes are the cyclic cut at pos
            ext = np.concatenate([text, text[:k - 1]])
            for i in range(min(found, 3)):                                                                   # the first counts, counted on the host
                at = np.flatnonzero(text == g[i, 0])
                for j in range(1, k):
                    at = at[ext[at + j] == g[i, j]]
                assert len(at) == int(e[i, 0]), (k, limit, i, len(at), int(e[i, 0]))
            tb_, cand, top_bin, bits = threshold(hist, found)
            d.update({"k": k, "limit": limit, "found": found, "distinct": distinct, "threshold_bin": tb_, "top_bin": top_bin, "candidates": cand,
                      "sorted_key_bits": bits, "candidates_over_found": cand / found, "size_hist": hist, "over_warm_build": d["median"] / warm,
                      "kgrams_one_k_s": one_k, "over_kgrams_one_k": d["median"] / one_k["median"], "first": [int(e[0, 0]), g[0].tobytes().decode("latin-1")]})
            doc["cases"].append(d)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--natural", action="store_true", help="also the natural corpus of tools/make_corpus.py at --size")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    c = api._Ctx(0)
    doc = {"what": "bce_hip_top_kgrams_device beside the warm index build (K1 + K2) and the one-k bce_hip_kgrams of the same run",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "texts": [measure(c, "synth_text seed 1", bce_amd.synth_text(1, a.size), a.repeats)]}
    if a.natural:
        path = "/tmp/bce_natural_%d.bin" % a.size
        if not (os.path.exists(path) and os.path.getsize(path) == a.size):
            subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "make_corpus.py"), "--out", path,
                            "--size", str(a.size)], stdout=subprocess.DEVNULL, check=False)
        if os.path.exists(path) and os.path.getsize(path) == a.size:
            doc["texts"].append(measure(c, "natural corpus (tools/make_corpus.py)", np.fromfile(path, dtype=np.uint8), a.repeats))
        else:
            doc["natural"] = "tools/make_corpus.py could not make it here"
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
