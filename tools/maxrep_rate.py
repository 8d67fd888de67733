"""Time of the list of maximal repeats (kd_maxrep.hip: bce_hip_maximal_repeats_device) beside three yardsticks of the same run: the
LCP pass at the same bound (bce_hip_lcp_device), the longest previous factors (bce_hip_lpf_device: the same trees and two searches a
row) and the warm index build (K1 + K2).  10^8 bytes of synth-text and, where tools/make_corpus.py can make it, the natural corpus.
Timed: bounds 256 and 4096, limits 100 and 65 536, the three orders, entries and 64 bytes of each repeat into device memory.  Warm
context, two warm-up calls, nine timed calls, median and range, a host clock around calls that end in the stream wait.  Beside each
time: total, capped and bwt_runs, and what the threshold bin lets through (the library's own BCE_MAXREP_TRACE line of one more,
untimed call: threshold and top bin, candidates, key bits sorted).  The outputs are checked in the same run: the weights descending,
every repeat's bytes the cyclic cut at its position, and the first entries' counts against a count of the bytes on the host.
One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.19 quotes it; profiles/ keeps it).

    python tools/maxrep_rate.py [--size 100000000] [--repeats 9] [--natural] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bce_amd  # noqa: E402
from bce_amd import api  # noqa: E402

BOUNDS = (256, 4096)
LIMITS = (100, 65536)
ORDERS = ("len", "count", "gain")
PER = 64


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


def traced(fn):
    """fn() once with BCE_MAXREP_TRACE set and the process's stderr in a file -> the numbers of the library's line."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["BCE_MAXREP_TRACE"] = "1"
        try:
            fn()
        finally:
            del os.environ["BCE_MAXREP_TRACE"]
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        words = f.read().decode().split()
    return {words[i]: int(words[i + 1]) for i in range(1, len(words) - 1, 2)} if words[:1] == ["maxrep:"] else {}


def weight(order, length, count):
    return (length << 31) | count if order == "len" else (count << 13) | length if order == "count" else length * (count - 1)


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
    words = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    words2 = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for bound in BOUNDS:
        lcp = timed(lambda: c.check(c.lib.bce_hip_lcp_device(c.h, bound, words.data_ptr()), "bce_hip_lcp_device"), repeats)
        lpf = timed(lambda: c.check(c.lib.bce_hip_lpf_device(c.h, bound, words.data_ptr(), words2.data_ptr()), "bce_hip_lpf_device"), repeats)
        for limit in LIMITS:
            ent = torch.zeros((limit, 4), dtype=torch.int32, device="cuda:0")
            raw = torch.zeros((limit, PER), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            for order in ORDERS:
                res = []

                def call():
                    res[:] = [rf.maximal_repeats_device(1, bound, order, limit, ent.data_ptr(), raw.data_ptr(), PER, limit * PER)]

                d = timed(call, repeats)
                trace = traced(call)
                info = res[0]
                found = info["found"]
                e = ent.cpu().numpy().astype(np.int64)[:found]
                g = raw.cpu().numpy()[:found]
                w = [weight(order, int(a), int(b)) for a, b in e[:, :2]]
                assert found == min(limit, info["total"]) and all(x >= y for x, y in zip(w, w[1:])) and (e[:, 1] >= 2).all()
                shown = np.minimum(e[:, 0], PER)
                idx = (e[:, 3][:, None] + np.arange(PER)[None, :]) % n
                assert np.array_equal(np.where(np.arange(PER)[None, :] < shown[:, None], text[idx], 0), g)   # the cyclic cut at pos, zeros behind it
                for i in range(min(found, 3)):                                                               # the first counts, counted on the host
                    ln = int(e[i, 0])
                    if ln >= bound:
                        continue
                    pat = text[(int(e[i, 3]) + np.arange(ln)) % n]
                    ext = np.concatenate([text, text[:ln - 1]])
                    at = np.flatnonzero(text == pat[0])
                    for j in range(1, ln):
                        at = at[ext[at + j] == pat[j]]
                    assert len(at) == int(e[i, 1]), (bound, limit, order, i, len(at), int(e[i, 1]))
                d.update({"max_len": bound, "limit": limit, "order": order, "info": info, "selection": trace,
                          "lcp_device_s": lcp, "lpf_device_s": lpf, "over_lcp": d["median"] / lcp["median"], "over_lpf": d["median"] / lpf["median"],
                          "over_warm_build": d["median"] / warm, "behind_the_lcp_pass_s": d["median"] - lcp["median"],
                          "first": [int(e[0, 0]), int(e[0, 1]), g[0][:int(shown[0])].tobytes().decode("latin-1")] if found else None})
                doc["cases"].append(d)
                print("%s: bound %d, limit %d, %s: %.2f ms" % (name, bound, limit, order, 1e3 * d["median"]), file=sys.stderr, flush=True)
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
    doc = {"what": "bce_hip_maximal_repeats_device beside bce_hip_lcp_device at the same bound, bce_hip_lpf_device and the warm index build (K1 + K2) of the same run",
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
