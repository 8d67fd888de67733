"""Patterns per second of the count by byte classes (kd_classes.hip) beside the exact count (kd_count.hip) on the same literals: 4096
patterns of 16 bytes cut from the text, on 10^8 bytes of synth-text and on 32 MiB of random bytes; each index (K1 + K2) built once.
Measured: one-member classes only; both cases of every letter (text only); 1, 2 and 3 full classes at the pattern's right end (the
root branches) and one in its middle; and a batch of `.{16}` in which every pattern runs to its budget and gives up, at growing
budgets up to BCE_HIP_CLASS_MAX_NODES -- the figure that decides that cap: a batch that exhausts it should stay under about two
seconds -- and the same for `[ab]{40}` on 2^26 bytes over two symbols, the narrowest branching that can exhaust a budget.  A budget
whose call takes longer than --ceiling seconds is the last one tried.  Warm, several repeats, spread stated; one answer of every
variant is checked against a brute force over the text.  One JSON document on stdout and, with --out, in a file (DESIGN.md section
4.18 quotes it; profiles/ keeps it).

The library refuses a budget above BCE_HIP_CLASS_MAX_NODES, so the give-up series ends at the cap of the build it runs on.
profiles/r24_class_rate.json was recorded while that cap was still 2^24 (its "class_max_nodes" says so); to reproduce its rows
above the committed cap, raise BCE_HIP_CLASS_MAX_NODES in include/bce_hip.h and CLASS_MAX_NODES in bce_amd/api.py and rebuild.

    python tools/class_rate.py [--patterns 4096] [--length 16] [--repeats 7] [--out FILE]
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


def timed(fn, repeats, warm=2, budget_s=40.0):
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


def exact_masks(pats):
    """(npat, m) bytes -> (npat, m, 8) masks of one-member classes"""
    masks = np.zeros(pats.shape + (8,), dtype=np.uint32)
    np.put_along_axis(masks, (pats >> 5)[..., None].astype(np.int64), (np.uint32(1) << (pats & 31).astype(np.uint32))[..., None], axis=2)
    return masks


def both_cases(masks, pats):
    lower = ((pats | 0x20) >= 0x61) & ((pats | 0x20) <= 0x7A)
    other = np.where(lower, pats ^ 0x20, pats)
    return masks | exact_masks(other)


def brute(text, masks):
    """the cyclic hits of one pattern, by a scan of the text: the narrowest class first, the others on the positions that are left"""
    n, m = len(text), len(masks)
    ext = np.concatenate([text, text[:m]])
    order = np.argsort([int(np.unpackbits(k.view(np.uint8)).sum()) for k in masks], kind="stable")
    j = int(order[0])
    table = ((masks[j][np.arange(256) >> 5] >> (np.arange(256) & 31).astype(np.uint32)) & 1).astype(bool)
    at = np.flatnonzero(table[ext[j:j + n]])
    for j in order[1:].tolist():
        c = ext[at + j]
        at = at[((masks[j][c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)]
    return len(at)


def give_up(rf, name, pattern, npat, ceiling):
    """a batch of npat copies of `pattern` ((m, 8) masks) at growing budgets, every one of which it exhausts"""
    m = len(pattern)
    d_mask = torch.from_numpy(np.ascontiguousarray(np.tile(pattern, (npat, 1, 1))).reshape(-1).view(np.int32)).to("cuda:0")
    off = torch.arange(npat + 1, device="cuda:0", dtype=torch.int64) * m
    out = torch.zeros(npat, device="cuda:0", dtype=torch.int64)
    work = torch.zeros(npat, device="cuda:0", dtype=torch.int64)
    status = torch.zeros(npat, device="cuda:0", dtype=torch.int32)
    torch.cuda.synchronize()
    rows = []
    for budget in (1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24):
        if budget > api.CLASS_MAX_NODES:
            break
        call = lambda: rf.count_classes_device(d_mask.data_ptr(), off.data_ptr(), npat, out.data_ptr(), status.data_ptr(), work.data_ptr(), max_nodes=budget)  # noqa: E731
        t0 = time.perf_counter()
        call()
        first = time.perf_counter() - t0
        s = spread([first]) if first > ceiling else timed(call, 3, warm=0, budget_s=3 * ceiling)
        over, nodes = status.cpu().numpy(), work.cpu().numpy()
        assert (over == 1).all() and (nodes > budget).all() and not out.cpu().numpy().any()
        rows.append({"max_nodes": budget, "s": s, "mean_work": float(nodes.mean()), "max_work": int(nodes.max())})
        print("%s: %d patterns give up at %d nodes in %.3f s" % (name, npat, budget, s["median"]), file=sys.stderr, flush=True)
        if s["median"] > ceiling:
            break
    return rows


def workload(c, name, text, npat, m, repeats, checked, ceiling, with_case):
    n = len(text)
    rs = np.random.RandomState(16)
    starts = rs.randint(0, n - m, npat)
    pats = text[starts[:, None] + np.arange(m)[None, :]].copy()
    t = torch.from_numpy(text).to("cuda:0")
    pat = torch.from_numpy(pats.reshape(-1)).to("cuda:0")
    off = torch.arange(npat + 1, device="cuda:0", dtype=torch.int64) * m
    out = torch.zeros(npat, device="cuda:0", dtype=torch.int64)
    work = torch.zeros(npat, device="cuda:0", dtype=torch.int64)
    status = torch.zeros(npat, device="cuda:0", dtype=torch.int32)
    torch.cuda.synchronize()
    rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
    doc = {"workload": name, "n": n, "patterns": npat, "length": m}
    s = timed(lambda: rf.count_device(pat.data_ptr(), off.data_ptr(), npat, out.data_ptr()), repeats)
    doc["count_s"], doc["count_patterns_per_s"] = s, npat / s["median"]
    want_exact = out.cpu().numpy().copy()
    base = exact_masks(pats)
    full = np.full(8, 0xFFFFFFFF, dtype=np.uint32)
    variants, checked_here = [("exact", base)], []
    if with_case:
        variants.append(("ignore_case", both_cases(base, pats)))
    for k in (1, 2, 3):
        v = base.copy()
        v[:, m - k:] = full
        variants.append(("full_x%d_at_the_right_end" % k, v))
    v = base.copy()
    v[:, m // 2] = full
    variants.append(("full_x1_in_the_middle", v))
    for label, masks in variants:
        d_mask = torch.from_numpy(np.ascontiguousarray(masks).reshape(-1).view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        s = timed(lambda: rf.count_classes_device(d_mask.data_ptr(), off.data_ptr(), npat, out.data_ptr(), status.data_ptr(), work.data_ptr()), repeats)
        counts, over, nodes = out.cpu().numpy(), status.cpu().numpy(), work.cpu().numpy()
        doc[label] = {"s": s, "patterns_per_s": npat / s["median"], "over": int((over != 0).sum()), "mean_nodes": float(nodes.mean()),
                      "mean_hits": float(counts.mean())}
        if label == "exact":
            assert np.array_equal(counts, want_exact) and not over.any()
        i = (len(doc) * 1009) % npat                                   # one answer of every variant: four and more per input
        if not over[i]:
            assert int(counts[i]) == brute(text, masks[i]), (name, label, i)
            checked_here.append(label)
        print("%s: %s, %.4f s a call, %.0f nodes a pattern" % (name, label, s["median"], nodes.mean()), file=sys.stderr, flush=True)
    doc["answers_checked_against_a_brute_force"] = checked_here
    assert len(checked_here) >= checked
    doc["give_up"] = give_up(rf, name, np.tile(full, (16, 1)), npat, ceiling)            # `.{16}`
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=4096)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--checked", type=int, default=4)
    ap.add_argument("--ceiling", type=float, default=6.0)
    ap.add_argument("--text-size", type=int, default=100000000)
    ap.add_argument("--rand-size", type=int, default=32 << 20)
    ap.add_argument("--binary-size", type=int, default=1 << 26)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    c = api._Ctx(0)
    docs = []
    for name, text, with_case in (("synth-text seed 1", bce_amd.synth_text(1, a.text_size), True), ("random bytes seed 2", bce_amd.synth_rand(2, a.rand_size), False)):
        docs.append(workload(c, name, text, a.patterns, a.length, a.repeats, a.checked, a.ceiling, with_case))
        print(json.dumps(docs[-1]), flush=True)
    # the narrowest branching that can still exhaust a budget: two-member classes on a text of two symbols
    text = (97 + (bce_amd.synth_rand(3, a.binary_size) & 1)).astype(np.uint8)
    t = torch.from_numpy(text).to("cuda:0")
    torch.cuda.synchronize()
    rf = api.RankFile(n=len(text), device_ptr=t.data_ptr(), ctx=c)
    two = np.zeros(8, dtype=np.uint32)
    two[3] = 6                                                         # {a, b}
    docs.append({"workload": "random text over {a, b} seed 3", "n": len(text), "patterns": a.patterns, "length": 40,
                 "give_up": give_up(rf, "two symbols", np.tile(two, (40, 1)), a.patterns, a.ceiling)})
    print(json.dumps(docs[-1]), flush=True)
    doc = {"what": "kd_classes.hip: bce_hip_count_classes_device beside bce_hip_count_device on the same literals, one warm context; give_up: "
                   "a batch of .{16} at growing budgets, every pattern over budget",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "class_max_nodes": api.CLASS_MAX_NODES, "workloads": docs}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
