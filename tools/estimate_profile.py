"""Four estimates of synth-text 10^8 B on one context, for a profiler: run under `rocprofv3 --kernel-trace --stats -- python
tools/estimate_profile.py` (the program itself goes after `--`).  Prints the estimate and the flush statistics."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bce_amd  # noqa: E402
from bce_amd import api  # noqa: E402

data = bce_amd.synth_text(1, 10**8)
t = torch.from_numpy(data).to("cuda:0")
torch.cuda.synchronize()
ctx = api._Ctx(0)
for _ in range(4):
    e = bce_amd.estimate_device(t.data_ptr(), t.numel(), ctx=ctx)
st = api.stats_of(ctx)
print(e, "%d records in %d flushes; t_model %.3f ms, of which K4's kernels %.3f ms" % (st["symbols"], st["flushes"], st["t_model"] * 1e3, st["t_model_kernels"] * 1e3))
ctx.close()
