"""Time of the self-index queries (kd_self.hip) beside the LCP pass of the same context (kd_lcp.hip), in the same run: 10^8 bytes of
synth-text (seed 1) indexed once, and with --natural the natural corpus of tools/make_corpus.py.  Timed at the bounds 16 and 256:
bce_hip_lcp_device (the yardstick: one compare per row), bce_hip_lpf_device (all nearest smaller values over the suffix array, then
two compares per row), bce_hip_self_parse_device at min_len 16 (sizing, and into outputs sized beforehand).  The ABI hands no
suffix array out, so the ANSV by itself is timed twice from outside: bce_hip_lpf_device at max_len 1 (the ANSV over the real suffix
array plus two one-byte compares and the scatter) and bce_hip_nsv_device on a random permutation of n words (no locality at all).
Warm context, two warm-up calls, nine timed calls, median and range.  Every parse is checked: the patch over the text gives the
text back.  One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.15 quotes it; profiles/ keeps it).

    python tools/self_parse_rate.py [--size 100000000] [--natural] [--repeats 9] [--out FILE]
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

MIN_LEN = 16


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


def natural(n):
    path = "/tmp/bce_natural_%d.bin" % n
    if not (os.path.exists(path) and os.path.getsize(path) == n):
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "make_corpus.py"), "--out", path, "--size", str(n)],
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        if r.returncode != 0:
            return None
    return np.fromfile(path, dtype=np.uint8)


def workload(name, text, repeats, c):
    dev = "cuda:0"
    n = len(text)
    t = torch.from_numpy(text).to(dev)
    words = torch.zeros(n, device=dev, dtype=torch.int32)
    more = torch.zeros(n, device=dev, dtype=torch.int32)
    back = torch.zeros(n, device=dev, dtype=torch.uint8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
    doc = {"workload": name, "n": n, "index_k1_k2_s": time.perf_counter() - t0}
    doc["lpf_device_max_len_1_s"] = timed(lambda: rf.lpf_device(1, words.data_ptr(), more.data_ptr()), repeats)
    for max_len in (16, 256):
        lcp = timed(lambda: rf.lcp_device(max_len, words.data_ptr()), repeats)
        lpf = timed(lambda: rf.lpf_device(max_len, words.data_ptr(), more.data_ptr()), repeats)
        lpf_mean = float(words.to(torch.float64).mean())
        info = rf.self_parse_device(MIN_LEN, max_len)
        ops = torch.zeros((info["nops"], 2), device=dev, dtype=torch.int32)
        lits = torch.zeros(max(info["nlits"], 1), device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        sizing = timed(lambda: rf.self_parse_device(MIN_LEN, max_len), repeats)
        full = timed(lambda: rf.self_parse_device(MIN_LEN, max_len, ops.data_ptr(), info["nops"], lits.data_ptr(), info["nlits"]), repeats)
        assert rf.patch_device(ops.data_ptr(), info["nops"], lits.data_ptr(), info["nlits"], back.data_ptr(), n) == n and torch.equal(back, t)
        z = rf.self_parse_device(1, max_len)
        doc["max_len_%d" % max_len] = {
            "lcp_device_s": lcp, "lpf_device_s": lpf, "lpf_over_lcp": lpf["median"] / lcp["median"], "mean_lpf": lpf_mean,
            "self_parse_device_sizing_s": sizing, "self_parse_device_s": full, "chain_and_emission_s": full["median"] - lpf["median"],
            "info_min_len_16": info, "phrases_z_min_len_1": z["ncopies"] + z["nlits"]}
    del rf
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000000)
    ap.add_argument("--natural", action="store_true")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    n = a.size
    c = api._Ctx(0)
    doc = {"what": "kd_self.hip beside kd_lcp.hip on one warm context: lpf, self-parse (min_len 16) and the LCP pass at the bounds 16 and 256",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "workloads": []}
    perm = torch.randperm(n, device="cuda:0", dtype=torch.int32)
    psv = torch.zeros(n, device="cuda:0", dtype=torch.int32)
    nsv = torch.zeros(n, device="cuda:0", dtype=torch.int32)
    torch.cuda.synchronize()

    def hook():
        assert api.nsv_device(perm.data_ptr(), n, psv.data_ptr(), nsv.data_ptr(), c) == 0

    doc["nsv_device_random_permutation_s"] = timed(hook, a.repeats)
    del perm, psv, nsv
    doc["workloads"].append(workload("synth-text seed 1", bce_amd.synth_text(1, n), a.repeats, c))
    if a.natural:
        nat = natural(n)
        doc["workloads"].append(workload("natural corpus", nat, a.repeats, c) if nat is not None else {"workload": "natural corpus", "absent": True})
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
