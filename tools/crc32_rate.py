"""kd_crc32's kernel beside kd_compare's on the same buffer: run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`
and read the durations of crc32_kernel and compare_kernel from DIR's kernel trace (End_Timestamp - Start_Timestamp).  The script only
makes the calls -- crc32_device on 10^8 and 10^9 bytes of text and of random bytes, six times each (the first builds the tables), and
three verify_device of the 10^8-byte text archive -- and checks every CRC against zlib.  profiles/r08_crc32.json is its record."""
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bce_amd
from bce_amd import api

c = api._Ctx(0)
for kind in ("text", "rand"):
    host = (bce_amd.synth_text if kind == "text" else bce_amd.synth_rand)(1, 10**9)
    t = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    for n in (10**8, 10**9):
        want = zlib.crc32(memoryview(host)[:n])
        for _ in range(6):
            assert api.crc32_device(t.data_ptr(), n, ctx=c) == want
    if kind == "text":
        arch = api.compress(host[:10**8], ctx=c)
        for _ in range(3):
            assert api.verify_device(arch, t.data_ptr(), 10**8, ctx=c) is None
    del t
print("calls done")
