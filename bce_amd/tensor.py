"""Torch plumbing of the device-resident round trip: tensors in HBM in, tensors in HBM out (torch is imported here only).

    arch = compress_tensor(t)                      # t: 1-D uint8 CUDA tensor -> archive bytes (host)
    u = decompress_tensor(arch, device="cuda:0")   # -> 1-D uint8 CUDA tensor; nothing of the text crosses to the host
    assert verify_tensor(arch, t) is None          # decoded and compared on the GPU

Stream rule.  The library runs on a stream of its own and knows nothing of torch's.  So every helper here synchronises
the tensor's CURRENT torch stream on the tensor's device before the call -- whatever produced `t` / `out` there must be
done -- and the call returns only when the library's stream is idle: the result may be used from any stream at once.
A tensor produced on another, non-current stream has to be synchronised by the caller."""
import torch

from . import api


def _device_index(device):
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError("a CUDA (HIP) device is required, not %r: there is no CPU path" % (device,))
    return torch.cuda.current_device() if d.index is None else d.index


def _check(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_cuda:
        raise ValueError("%s must be a 1-D uint8 CUDA tensor" % what)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous (a slice of a 1-D tensor is)" % what)
    return t


def _ready(t):
    """What produced `t` on its device's current stream is done (see the stream rule)."""
    torch.cuda.current_stream(t.device).synchronize()


def compress_tensor(t, config=None, ctx=None):
    """`bce -c` on a 1-D uint8 CUDA tensor (bce_hip_compress_device) -> the archive (host bytes).
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    if t.numel() == 0:
        raise api.BceError(-1, "compress_tensor", "empty input")
    _ready(t)
    arch, _ = api.compress_device(t.data_ptr(), t.numel(), config=config, device=t.device.index, ctx=ctx)
    return arch


def decompress_tensor(archive, device="cuda:0", out=None, ctx=None):
    """The GPU-assisted decoder with the text left on the device (bce_hip_decompress_to_device) -> a 1-D uint8 tensor there.

    `out`: a 1-D uint8 CUDA tensor, or a slice of one (any offset), at least as long as the original: the bytes are
    written to its front, nothing beyond them is touched, and out[:n] comes back.  Too short: BceError (status -5),
    nothing written.  Synchronises out's current stream first; complete on return (see the stream rule)."""
    if out is not None:
        _check(out, "out")
        _ready(out)
        n = api.decompress_to_device(archive, out.data_ptr(), out.numel(), device=out.device.index, ctx=ctx)
        return out[:n]
    dev = _device_index(device)
    own = ctx is None
    c = ctx or api._Ctx(dev)
    try:
        n = api.decompress_to_device(archive, None, 0, ctx=c)
        res = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", dev))
        _ready(res)
        api.decompress_to_device(archive, res.data_ptr(), n, ctx=c)
        return res
    finally:
        if own:
            c.close()


def verify_tensor(archive, t, ctx=None):
    """Does `archive` decode to the bytes of the 1-D uint8 CUDA tensor `t` (or slice)?  Decoded and compared on the GPU
    (bce_hip_verify_device).  -> None when it does, else the first index at which they differ (min of the two sizes when
    only the sizes differ).  Synchronises t's current stream first."""
    _check(t, "t")
    _ready(t)
    return api.verify_device(archive, t.data_ptr() if t.numel() else None, t.numel(), device=t.device.index, ctx=ctx)
