"""Time of the match (kd_match.hip) beside the count (kd_count.hip) on the same windows, in the same run: 10^8 bytes of synth-text
indexed, a query of 10^6 bytes cut from it with a byte changed every 64 bytes or so.  Timed: bce_hip_match_device with a bound of 16
and of 256 (linear, with positions; and the bound of 16 without positions and cyclic), bce_hip_coverage_device with min_len 16, and
the query's windows of 16 bytes -- one per end position -- through bce_hip_count_device.  Warm context, two warm-up calls, nine timed
calls, median and range.  The lengths are checked against the counts (a window occurs in the circular text exactly where the cyclic
match reaches the bound) and a sample of them, with their positions, against a scan of the text.
One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.10 quotes it; profiles/ keeps it).

    python tools/match_rate.py [--size 100000000] [--query 1000000] [--repeats 9] [--out FILE]
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

WINDOW = 16


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000000)
    ap.add_argument("--query", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--checked", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    n, q = a.size, a.query
    dev = "cuda:0"
    text = bce_amd.synth_text(1, n)
    tb = text.tobytes()
    rs = np.random.RandomState(64)
    at = int(rs.randint(0, n - q))
    query = text[at:at + q].copy()
    spoiled = np.cumsum(rs.randint(32, 97, q // 64 + 1))            # every 64 bytes or so
    spoiled = spoiled[spoiled < q]
    query[spoiled] ^= 0x80                                           # (synth-text is 7-bit: these bytes occur nowhere)
    qb = query.tobytes()
    t = torch.from_numpy(text).to(dev)
    d_q = torch.from_numpy(query).to(dev)
    nwin = q - WINDOW + 1
    windows = d_q.unfold(0, WINDOW, 1).contiguous().reshape(-1)      # window w = query[w, w + 16): ends at w + 15
    woff = torch.arange(nwin + 1, device=dev, dtype=torch.int64) * WINDOW
    counts = torch.zeros(nwin, device=dev, dtype=torch.int64)
    lens = torch.zeros(q, device=dev, dtype=torch.int32)
    pos = torch.zeros(q, device=dev, dtype=torch.int32)
    torch.cuda.synchronize()

    c = api._Ctx(0)
    build = []
    for _ in range(3):                                               # the first builds the context's buffers
        t0 = time.perf_counter()
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        build.append(time.perf_counter() - t0)

    doc = {"what": "kd_match.hip beside kd_count.hip: a query cut from synth-text (seed 1), a byte changed every 64 bytes or so",
           "device": torch.cuda.get_device_name(0), "n": n, "query_bytes": q, "changed_bytes": int(len(spoiled)), "window": WINDOW,
           "repeats": a.repeats, "index_build_s": {"first_cold": build[0], "warm": build[1:]}}
    doc["count_device_windows_s"] = timed(lambda: rf.count_device(windows.data_ptr(), woff.data_ptr(), nwin, counts.data_ptr()), a.repeats)
    base = doc["count_device_windows_s"]["median"]
    runs = (("match_16_linear", 16, False, True), ("match_16_linear_no_positions", 16, False, False), ("match_16_cyclic", 16, True, True),
            ("match_256_linear", 256, False, True))
    for name, bound, cyclic, with_pos in runs:
        d = timed(lambda: rf.match_device(d_q.data_ptr(), q, bound, lens.data_ptr(), pos.data_ptr() if with_pos else None, cyclic=cyclic), a.repeats)
        d["over_count"] = d["median"] / base
        d["end_positions_per_s"] = q / d["median"]
        h_lens = lens.cpu().numpy().astype(np.int64)
        d["mean_length"] = float(h_lens.mean())
        d["at_the_bound"] = int((h_lens == bound).sum())
        assert (h_lens[1:] <= h_lens[:-1] + 1).all() and h_lens.max() <= bound
        if bound == WINDOW and cyclic:                               # the count's answer on the same windows
            occurs = counts.cpu().numpy() > 0
            assert np.array_equal(h_lens[WINDOW - 1:] == WINDOW, occurs)
            d["windows_that_occur"] = int(occurs.sum())
        if with_pos:                                                 # a sample against a scan of the text
            h_pos = pos.cpu().numpy().astype(np.uint32)
            for i in range(0, q, max(1, q // a.checked)):
                l, p = int(h_lens[i]), int(h_pos[i])
                piece = qb[i - l + 1:i + 1]
                if l == 0:
                    assert p == 0xFFFFFFFF
                else:
                    assert p < n and (cyclic or p + l <= n) and tb[p:p + l] + tb[:max(0, p + l - n)] == piece, (name, i, l, p)
                if l < min(bound, i + 1) and not cyclic:
                    assert tb.find(qb[i - l:i + 1]) < 0, (name, i, l)             # one byte more occurs nowhere
            d["checked_against_a_scan"] = len(range(0, q, max(1, q // a.checked)))
        doc[name] = d
    covered = [0]

    def cover():
        covered[0] = rf.coverage_device(d_q.data_ptr(), q, WINDOW)

    d = timed(cover, a.repeats)
    d["over_count"] = d["median"] / base
    d["covered"] = covered[0]
    rf.match_device(d_q.data_ptr(), q, WINDOW, lens.data_ptr(), None)
    h_lens = lens.cpu().numpy().astype(np.int64)
    mark = np.zeros(q + 1, dtype=np.int64)
    ends = np.flatnonzero(h_lens >= WINDOW)
    np.add.at(mark, ends - h_lens[ends] + 1, 1)
    np.add.at(mark, ends + 1, -1)
    assert covered[0] == int(np.count_nonzero(np.cumsum(mark[:q]) > 0))
    doc["coverage_16_linear"] = d
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
