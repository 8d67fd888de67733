"""Patterns per second of the search within k edits (kd_edit.hip: count and locate, k = 0, 1 and 2) beside the search within k
mismatches (kd_near.hip, the yardstick) on the same batch, in the same process: 4096 patterns of 16 bytes cut from the text, in turn
as cut, one byte altered, one byte removed, one byte doubled; on 10^8 bytes of synth-text and on 32 MiB of random bytes; each index
(K1 + K2) built once.  Warm, several repeats, spread stated; a sample of the answers is checked against tests/edit_ref.py on a window
of the text.  One JSON document on stdout and, with --out, in a file (DESIGN.md section 4.20 quotes it; profiles/ keeps it).

    python tools/edit_rate.py [--patterns 4096] [--length 16] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bce_amd  # noqa: E402
from bce_amd import api  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": xs}


def timed(fn, repeats, warm=1, budget_s=40.0):
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


def batch(text, npat, m, rs):
    n = len(text)
    pats = []
    for i, at in enumerate(rs.randint(0, n - m - 2, npat).tolist()):
        x = 1 + int(rs.randint(0, m - 2))
        kind = i % 4
        if kind == 0:
            p = text[at:at + m].copy()
        elif kind == 1:
            p = text[at:at + m].copy()
            p[x] ^= 1 + int(rs.randint(0, 255))
        elif kind == 2:
            p = np.delete(text[at:at + m + 1], x)
        else:
            p = np.insert(text[at:at + m - 1], x, text[at + x])
        assert len(p) == m
        pats.append(p)
    return np.stack(pats)


def workload(c, name, text, npat, m, repeats, checked):
    import edit_ref
    n = len(text)
    pats = batch(text, npat, m, np.random.RandomState(16))
    dev = "cuda:0"
    t = torch.from_numpy(text).to(dev)
    pat = torch.from_numpy(pats.reshape(-1)).to(dev)
    off = torch.arange(npat + 1, device=dev, dtype=torch.int64) * m
    out = torch.zeros(npat * 3, device=dev, dtype=torch.int64)
    hits = torch.zeros(npat + 1, device=dev, dtype=torch.int64)
    torch.cuda.synchronize()
    rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
    doc = {"workload": name, "n": n, "patterns": npat, "length": m}
    P, O = pat.data_ptr(), off.data_ptr()
    answers = {}
    for k in (0, 1, 2):
        total_near = rf.locate_near_device(P, O, npat, k, hits.data_ptr(), None, None, 0)
        total_edit = rf.locate_edit_device(P, O, npat, k, hits.data_ptr(), None, None, None, 0)
        room = max(total_near, total_edit, 1)
        pos = torch.empty(room, device=dev, dtype=torch.int32)
        lens = torch.empty(room, device=dev, dtype=torch.int16)
        dist = torch.empty(room, device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        runs = (("count_near", lambda: rf.count_near_device(P, O, npat, k, out.data_ptr())),
                ("locate_near", lambda: rf.locate_near_device(P, O, npat, k, hits.data_ptr(), pos.data_ptr(), dist.data_ptr(), room)),
                ("count_edit", lambda: rf.count_edit_device(P, O, npat, k, out.data_ptr())),
                ("locate_edit", lambda: rf.locate_edit_device(P, O, npat, k, hits.data_ptr(), pos.data_ptr(), lens.data_ptr(), dist.data_ptr(), room)))
        for what, fn in runs:
            s = timed(fn, repeats)
            doc["%s_k%d_s" % (what, k)] = s
            doc["%s_k%d_patterns_per_s" % (what, k)] = npat / s["median"]
            print("%s: %s k = %d, %.4f s a call" % (name, what, k, s["median"]), file=sys.stderr, flush=True)
        doc["near_k%d_hits" % k], doc["edit_k%d_hits" % k] = total_near, total_edit
        h = hits.cpu().numpy()
        answers[k] = (h, pos[:total_edit].cpu().numpy(), lens[:total_edit].cpu().numpy(), dist[:total_edit].cpu().numpy())
    doc["count_edit_k2_call_over_a_second"] = doc["count_edit_k2_s"]["median"] > 1.0
    # the definition on a window of the text around a planted pattern: the hits that start inside the window
    for i in range(0, npat, max(1, npat // checked)):
        p = pats[i].tobytes()
        for k in (0, 1, 2):
            h, pos, lens, dist = answers[k]
            got = list(zip(pos[h[i]:h[i + 1]].tolist(), lens[h[i]:h[i + 1]].tolist(), dist[h[i]:h[i + 1]].tolist()))
            assert got, (name, i, k)
            lo = max(0, got[0][0] - 1000)
            hi = min(n, lo + 100000)
            w = edit_ref.hits(text[lo:hi].tobytes(), p, k, cyclic=False)
            want = [(a + lo, b, e) for a, b, e in zip(w[0].tolist(), w[1].tolist(), w[2].tolist())]
            inside = [g for g in got if lo <= g[0] and g[0] + m + k <= hi]
            assert inside == [v for v in want if v[0] + m + k <= hi], (name, i, k)
    doc["answers_checked_against_the_definition"] = checked
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=4096)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
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
    doc = {"what": "kd_edit.hip: bce_hip_count_edit_device / _locate_edit_device for k = 0, 1, 2 beside bce_hip_count_near_device / _locate_near_device, "
                   "one warm context, linear mode, patterns cut from the text: as cut, one byte altered, one removed, one doubled",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "workloads": docs}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
