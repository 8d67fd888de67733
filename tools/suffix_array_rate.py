"""Time of the suffix array as a product and of its checker (kd_sufsort.hip) beside divbwt, the same sort, on one warm context:
bce_hip_suffix_array_device without and with the inverse, bce_hip_sufcheck_device on the array just made, and bce_hip_divbwt (host
buffers: the only form it has, so its time includes n bytes in and n bytes out).  synth-text (seed 3, 2^20 bytes) and synth-rand
(seed 4, 300 000 bytes), the sizes tests/test_gpu_seam.py sorts, and synth-text (seed 1) at --size bytes.  Two warm-up calls, --repeats
timed calls, median and range.  Every array is checked before its time counts.  One JSON document on stdout and, with --out, in a
file (DESIGN.md section 4.16 quotes it; profiles/ keeps it).

    python tools/suffix_array_rate.py [--size 100000000] [--repeats 9] [--out FILE]
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


def workload(name, text, repeats, c):
    dev = "cuda:0"
    n = len(text)
    t = torch.from_numpy(text).to(dev)
    sa = torch.zeros(n, device=dev, dtype=torch.int32)
    isa = torch.zeros(n, device=dev, dtype=torch.int32)
    u = np.empty(n, dtype=np.uint8)
    primary = C.c_uint32(0)
    torch.cuda.synchronize()

    def sort(with_isa):
        assert api.suffix_array_device(t.data_ptr(), n, sa.data_ptr(), isa.data_ptr() if with_isa else None, ctx=c) == 0

    def check():
        assert api.sufcheck_device(t.data_ptr(), sa.data_ptr(), n, c) == (0, None)

    def divbwt():
        c.check(c.lib.bce_hip_divbwt(c.h, text.ctypes.data, u.ctypes.data, n, C.byref(primary)), "bce_hip_divbwt")

    doc = {"workload": name, "n": n}
    doc["divbwt_host_s"] = timed(divbwt, repeats)
    doc["suffix_array_device_s"] = timed(lambda: sort(False), repeats)
    doc["suffix_array_device_with_inverse_s"] = timed(lambda: sort(True), repeats)
    doc["sufcheck_device_s"] = timed(check, repeats)
    assert bool((isa[sa.long()] == torch.arange(n, device=dev, dtype=torch.int32)).all())
    assert int(isa[0]) + 1 == primary.value                          # divbwt's primary index is the row of suffix 0, counted from 1
    doc["array_over_divbwt"] = doc["suffix_array_device_s"]["median"] / doc["divbwt_host_s"]["median"]
    doc["inverse_costs_s"] = doc["suffix_array_device_with_inverse_s"]["median"] - doc["suffix_array_device_s"]["median"]
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    c = api._Ctx(0)
    doc = {"what": "bce_hip_suffix_array_device, bce_hip_sufcheck_device and bce_hip_divbwt on one warm context", "device": torch.cuda.get_device_name(0),
           "repeats": a.repeats, "workloads": []}
    for name, text in (("synth-text seed 3", bce_amd.synth_text(3, 1 << 20)), ("synth-rand seed 4", bce_amd.synth_rand(4, 300000)),
                       ("synth-text seed 1", bce_amd.synth_text(1, a.size))):
        doc["workloads"].append(workload(name, text, a.repeats, c))
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    c.close()


if __name__ == "__main__":
    main()
