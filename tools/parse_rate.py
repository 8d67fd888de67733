"""Time of the delta parse and of the patch (kd_parse.hip) beside the search they rest on (kd_match.hip) and beside a plain
device-to-device copy, in the same run: 10^8 bytes of synth-text indexed, a query of 10^6 bytes cut from it with a byte changed every
64 bytes or so (tools/match_rate.py's workload).  Timed, for min_len 16 at max_len 16 and 256: bce_hip_match_device (linear, with
positions) and bce_hip_parse_device into outputs sized beforehand -- the difference is the chain and the emission; then
bce_hip_patch_device of that parse beside a copy of the query's bytes.  With --size-walk: the parse alone
(bce_hip_parse_of_lengths_device) on that many all-literal positions, size / 2048 dependent loads in its one-lane walk, and the patch
of one literal op of that many bytes beside a copy.  Warm context, two warm-up calls, nine timed calls, median and range.  Every
result is checked: the patch gives the query back.  One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.12
quotes it; profiles/ keeps it).

    python tools/parse_rate.py [--size 100000000] [--query 1000000] [--size-walk 100000000] [--repeats 9] [--out FILE]
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


def copy_of(dst, src):
    def run():
        dst.copy_(src)
        torch.cuda.synchronize()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000000)
    ap.add_argument("--query", type=int, default=1000000)
    ap.add_argument("--size-walk", type=int, default=100000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    n, q = a.size, a.query
    dev = "cuda:0"
    text = bce_amd.synth_text(1, n)
    rs = np.random.RandomState(64)
    at = int(rs.randint(0, n - q))
    query = text[at:at + q].copy()
    spoiled = np.cumsum(rs.randint(32, 97, q // 64 + 1))            # every 64 bytes or so
    spoiled = spoiled[spoiled < q]
    query[spoiled] ^= 0x80                                           # (synth-text is 7-bit: these bytes occur nowhere)
    t = torch.from_numpy(text).to(dev)
    d_q = torch.from_numpy(query).to(dev)
    lens = torch.zeros(q, device=dev, dtype=torch.int32)
    pos = torch.zeros(q, device=dev, dtype=torch.int32)
    out = torch.zeros(q, device=dev, dtype=torch.uint8)
    torch.cuda.synchronize()
    c = api._Ctx(0)
    rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
    doc = {"what": "kd_parse.hip beside kd_match.hip and a device-to-device copy: a query cut from synth-text (seed 1), a byte changed every 64 bytes or so",
           "device": torch.cuda.get_device_name(0), "n": n, "query_bytes": q, "changed_bytes": int(len(spoiled)), "min_len": MIN_LEN,
           "repeats": a.repeats}
    doc["copy_query_s"] = timed(copy_of(out, d_q), a.repeats)
    for max_len in (16, 256):
        info = rf.parse_device(d_q.data_ptr(), q, MIN_LEN, max_len)
        ops = torch.zeros((info["nops"], 2), device=dev, dtype=torch.int32)
        lits = torch.zeros(max(info["nlits"], 1), device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        m = timed(lambda: rf.match_device(d_q.data_ptr(), q, max_len, lens.data_ptr(), pos.data_ptr()), a.repeats)
        p = timed(lambda: rf.parse_device(d_q.data_ptr(), q, MIN_LEN, max_len, ops.data_ptr(), info["nops"], lits.data_ptr(), info["nlits"]), a.repeats)
        s = timed(lambda: rf.parse_device(d_q.data_ptr(), q, MIN_LEN, max_len), a.repeats)
        out.zero_()
        torch.cuda.synchronize()
        d = timed(lambda: rf.patch_device(ops.data_ptr(), info["nops"], lits.data_ptr(), info["nlits"], out.data_ptr(), q), a.repeats)
        assert torch.equal(out, d_q)
        doc["max_len_%d" % max_len] = {
            "info": info, "match_device_s": m, "parse_device_s": p, "parse_device_sizing_s": s, "patch_device_s": d,
            "chain_and_emission_s": p["median"] - m["median"], "chain_and_emission_over_search": (p["median"] - m["median"]) / m["median"],
            "patch_over_copy": d["median"] / doc["copy_query_s"]["median"]}
    w = a.size_walk
    if w:
        zeros = torch.zeros(w, device=dev, dtype=torch.int32)
        big = torch.from_numpy(bce_amd.synth_rand(5, w)).to(dev)
        dst = torch.zeros(w, device=dev, dtype=torch.uint8)
        one = torch.tensor([[w, -1]], device=dev, dtype=torch.int32)
        torch.cuda.synchronize()
        info = {}

        def hook():
            rc, got = api.parse_of_lengths_device(zeros.data_ptr(), None, big.data_ptr(), w, 1, c)
            assert rc == 0
            info.update(got)

        h = timed(hook, a.repeats)
        assert info == {"nops": 1, "nlits": w, "ncopies": 0, "copied": 0}
        cp = timed(copy_of(dst, big), a.repeats)
        dst.zero_()
        torch.cuda.synchronize()
        pt = timed(lambda: rf.patch_device(one.data_ptr(), 1, big.data_ptr(), w, dst.data_ptr(), w), a.repeats)
        assert torch.equal(dst, big)
        doc["all_literal"] = {"positions": w, "blocks_walked": (w + 2047) // 2048, "parse_of_lengths_sizing_s": h, "copy_s": cp,
                              "patch_one_literal_op_s": pt, "patch_over_copy": pt["median"] / cp["median"]}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
