"""Torch plumbing of the device-resident round trip: tensors in HBM in, tensors in HBM out (torch is imported here only).

    arch = compress_tensor(t)                      # t: 1-D uint8 CUDA tensor -> archive bytes (host)
    u = decompress_tensor(arch, device="cuda:0")   # -> 1-D uint8 CUDA tensor; nothing of the text crosses to the host
    assert verify_tensor(arch, t) is None          # decoded and compared on the GPU

    blob = compress_tensor_blocks(t)               # any size >= 1 (blocks below 2^31 each) -> a checked BCEM container (version 2)
    u = decompress_container_tensor(blob)          # every block decoded into its slice and tested against its CRC-32 there
    assert test_container(blob) is None            # ... or only tested: nothing is kept

Stream rule.  The library runs on a stream of its own and knows nothing of torch's.  So every helper here synchronises
the tensor's CURRENT torch stream on the tensor's device before the call -- whatever produced `t` / `out` there must be
done -- and the call returns only when the library's stream is idle: the result may be used from any stream at once.
A tensor produced on another, non-current stream has to be synchronised by the caller."""
import numpy as np
import torch

from . import api, container
from .sharding import block_range


_MAX_BLOCK = (1 << 31) - 1          # a block obeys the reference's n < 2^31


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


def estimate_tensor(t, config=None, ctx=None):
    """The size `compress_tensor(t, config)` would give, without coding (bce_hip_estimate_device) -> api.Estimate.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    if t.numel() == 0:
        raise api.BceError(-1, "estimate_tensor", "empty input")
    _ready(t)
    return api.estimate_device(t.data_ptr(), t.numel(), config=config, device=t.device.index, ctx=ctx)


def count_tensor(t, patterns, ctx=None):
    """How often `patterns` (one bytes-like -> int, a sequence -> numpy uint64 array) occur in the 1-D uint8 CUDA tensor `t` (or
    slice, any offset), overlapping matches counted: indexed where it lies (K1, K2) and counted from the index
    (api.RankFile.count); of the text only the few bytes at its two ends that the longest pattern asks for reach the host.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "count_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        return api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c).count(patterns)
    finally:
        if own:
            c.close()


def count_in_archive(blob, patterns, device="cuda:0"):
    """count_tensor on what an archive holds: a plain archive or a BCEM container of either version is decoded into ONE tensor
    on the device (decompress_container_tensor: a version-2 container's blocks are tested against their CRC-32 there), indexed
    and counted there -- matches across block boundaries included.  A container of 2^31 bytes or more: ValueError (one index
    covers one text), before anything is decoded."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return count_tensor(decompress_container_tensor(blob, device=device), patterns)


def locate_tensor(t, patterns, cyclic=False, ctx=None):
    """Where `patterns` (one bytes-like or a sequence of them) occur in the 1-D uint8 CUDA tensor `t` (or slice, any offset) ->
    (offsets, positions), both tensors on t's device: int64[npat + 1] and int32[total] (positions are below 2^31).  Pattern p owns
    positions[offsets[p]:offsets[p + 1]], ascending byte offsets into t.  cyclic: as api.RankFile.locate (False: an empty pattern
    raises ValueError).  The text is indexed where it lies and the hits are gathered, filtered and ordered there
    (bce_hip_locate_device, a sizing call first); of the answer only its total reaches the host.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "locate_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    pats = [api._as_u8(patterns)] if api._is_one_pattern(patterns) else [api._as_u8(p) for p in patterns]
    if not cyclic and any(len(p) == 0 for p in pats):
        raise ValueError("an empty pattern has no linear hits (cyclic=True: every position)")
    offsets = torch.zeros(len(pats) + 1, dtype=torch.int64, device=t.device)
    if not pats:
        return offsets, torch.empty(0, dtype=torch.int32, device=t.device)
    lens = np.zeros(len(pats) + 1, dtype=np.int64)
    lens[1:] = np.cumsum([len(p) for p in pats], dtype=np.int64)
    flat = np.concatenate(pats) if int(lens[-1]) else np.zeros(1, dtype=np.uint8)
    d_pat, d_off = torch.from_numpy(flat).to(t.device), torch.from_numpy(lens).to(t.device)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        total = rf.locate_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), offsets.data_ptr(), None, 0, cyclic=cyclic)
        positions = torch.empty(total, dtype=torch.int32, device=t.device)
        if total:
            torch.cuda.current_stream(t.device).synchronize()        # (the allocator may hand out memory a queued kernel still uses)
            rf.locate_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), offsets.data_ptr(), positions.data_ptr(), total, cyclic=cyclic)
        return offsets, positions
    finally:
        if own:
            c.close()


def locate_in_archive(blob, patterns, cyclic=False, device="cuda:0"):
    """locate_tensor on what an archive holds, decoded as count_in_archive decodes it: into ONE tensor on the device, so the
    offsets run over the concatenated blocks and hits across block boundaries are found.  -> (offsets, positions) on `device`."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return locate_tensor(decompress_container_tensor(blob, device=device), patterns, cyclic=cyclic)


def count_near_tensor(t, patterns, k, cyclic=False, ctx=None):
    """The hits of `patterns` within k mismatches in the 1-D uint8 CUDA tensor `t` (or slice, any offset), per distance: one
    bytes-like -> a numpy uint64 array of k + 1, a sequence -> shape (npat, k + 1) (api.RankFile.count_near).  Indexed where it
    lies; of the text only the few bytes at its two ends that the longest pattern asks for reach the host.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "count_near_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        return api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c).count_near(patterns, k, cyclic=cyclic)
    finally:
        if own:
            c.close()


def count_near_in_archive(blob, patterns, k, cyclic=False, device="cuda:0"):
    """count_near_tensor on what an archive holds, decoded as count_in_archive decodes it: hits across block boundaries included."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return count_near_tensor(decompress_container_tensor(blob, device=device), patterns, k, cyclic=cyclic)


def locate_near_tensor(t, patterns, k, cyclic=False, ctx=None):
    """Where `patterns` occur within k mismatches in the 1-D uint8 CUDA tensor `t` (or slice, any offset) -> (offsets, positions,
    dists), all tensors on t's device: int64[npat + 1], int32[total] and uint8[total].  Pattern p owns
    positions[offsets[p]:offsets[p + 1]], ascending byte offsets into t, and dists holds the distance of each.  cyclic and k: as
    api.RankFile.locate_near.  Searched, gathered and ordered on the device (bce_hip_locate_near_device, a sizing call first); of
    the answer only its total reaches the host.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "locate_near_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    if not 0 <= int(k) <= api.NEAR_MAX_K:
        raise ValueError("k = %r, outside 0 .. %d" % (k, api.NEAR_MAX_K))
    pats = [api._as_u8(patterns)] if api._is_one_pattern(patterns) else [api._as_u8(p) for p in patterns]
    if not cyclic and any(len(p) == 0 for p in pats):
        raise ValueError("an empty pattern has no linear hits (cyclic=True: every position, at distance 0)")
    offsets = torch.zeros(len(pats) + 1, dtype=torch.int64, device=t.device)
    if not pats:
        return offsets, torch.empty(0, dtype=torch.int32, device=t.device), torch.empty(0, dtype=torch.uint8, device=t.device)
    lens = np.zeros(len(pats) + 1, dtype=np.int64)
    lens[1:] = np.cumsum([len(p) for p in pats], dtype=np.int64)
    flat = np.concatenate(pats) if int(lens[-1]) else np.zeros(1, dtype=np.uint8)
    d_pat, d_off = torch.from_numpy(flat).to(t.device), torch.from_numpy(lens).to(t.device)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        total = rf.locate_near_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), k, offsets.data_ptr(), None, None, 0, cyclic=cyclic)
        positions = torch.empty(total, dtype=torch.int32, device=t.device)
        dists = torch.empty(total, dtype=torch.uint8, device=t.device)
        if total:
            torch.cuda.current_stream(t.device).synchronize()        # (the allocator may hand out memory a queued kernel still uses)
            rf.locate_near_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), k, offsets.data_ptr(), positions.data_ptr(), dists.data_ptr(), total,
                                  cyclic=cyclic)
        return offsets, positions, dists
    finally:
        if own:
            c.close()


def locate_near_in_archive(blob, patterns, k, cyclic=False, device="cuda:0"):
    """locate_near_tensor on what an archive holds, decoded as count_in_archive decodes it -> (offsets, positions, dists) on `device`."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return locate_near_tensor(decompress_container_tensor(blob, device=device), patterns, k, cyclic=cyclic)


def count_edit_tensor(t, patterns, k, cyclic=False, ctx=None):
    """The hits of `patterns` within k edits in the 1-D uint8 CUDA tensor `t` (or slice, any offset), per distance: one bytes-like
    -> a numpy uint64 array of k + 1, a sequence -> shape (npat, k + 1) (api.RankFile.count_edit).  Indexed, searched and
    reduced where it lies.  Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "count_edit_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        return api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c).count_edit(patterns, k, cyclic=cyclic)
    finally:
        if own:
            c.close()


def count_edit_in_archive(blob, patterns, k, cyclic=False, device="cuda:0"):
    """count_edit_tensor on what an archive holds, decoded as count_in_archive decodes it: hits across block boundaries included."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return count_edit_tensor(decompress_container_tensor(blob, device=device), patterns, k, cyclic=cyclic)


def locate_edit_tensor(t, patterns, k, cyclic=False, ctx=None):
    """Where `patterns` occur within k edits in the 1-D uint8 CUDA tensor `t` (or slice, any offset) -> (offsets, positions, lens,
    dists), all tensors on t's device: int64[npat + 1], int32[total], int16[total] and uint8[total].  Pattern p owns
    positions[offsets[p]:offsets[p + 1]], ascending byte offsets into t; lens and dists hold the length and the distance of the
    best alignment that starts at each.  cyclic and k: as api.RankFile.locate_edit.  Searched, reduced and ordered on the device
    (bce_hip_locate_edit_device, a sizing call first); of the answer only its total reaches the host.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "locate_edit_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    if not 0 <= int(k) <= api.EDIT_MAX_K:
        raise ValueError("k = %r, outside 0 .. %d" % (k, api.EDIT_MAX_K))
    pats = [api._as_u8(patterns)] if api._is_one_pattern(patterns) else [api._as_u8(p) for p in patterns]
    if not cyclic and any(len(p) == 0 for p in pats):
        raise ValueError("an empty pattern has no linear hits (cyclic=True: every position, at distance 0)")
    if any(len(p) > api.EDIT_MAX_LEN for p in pats):
        raise ValueError("a pattern of more than %d bytes" % api.EDIT_MAX_LEN)
    offsets = torch.zeros(len(pats) + 1, dtype=torch.int64, device=t.device)
    if not pats:
        return (offsets, torch.empty(0, dtype=torch.int32, device=t.device), torch.empty(0, dtype=torch.int16, device=t.device),
                torch.empty(0, dtype=torch.uint8, device=t.device))
    ends = np.zeros(len(pats) + 1, dtype=np.int64)
    ends[1:] = np.cumsum([len(p) for p in pats], dtype=np.int64)
    flat = np.concatenate(pats) if int(ends[-1]) else np.zeros(1, dtype=np.uint8)
    d_pat, d_off = torch.from_numpy(flat).to(t.device), torch.from_numpy(ends).to(t.device)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        total = rf.locate_edit_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), k, offsets.data_ptr(), None, None, None, 0, cyclic=cyclic)
        positions = torch.empty(total, dtype=torch.int32, device=t.device)
        lens = torch.empty(total, dtype=torch.int16, device=t.device)
        dists = torch.empty(total, dtype=torch.uint8, device=t.device)
        if total:
            torch.cuda.current_stream(t.device).synchronize()        # (the allocator may hand out memory a queued kernel still uses)
            rf.locate_edit_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), k, offsets.data_ptr(), positions.data_ptr(), lens.data_ptr(),
                                  dists.data_ptr(), total, cyclic=cyclic)
        return offsets, positions, lens, dists
    finally:
        if own:
            c.close()


def locate_edit_in_archive(blob, patterns, k, cyclic=False, device="cuda:0"):
    """locate_edit_tensor on what an archive holds, decoded as count_in_archive decodes it -> (offsets, positions, lens, dists) on `device`."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return locate_edit_tensor(decompress_container_tensor(blob, device=device), patterns, k, cyclic=cyclic)


def count_classes_tensor(t, patterns, cyclic=False, max_nodes=None, ignore_case=False, ctx=None):
    """The hits of patterns of byte classes in the 1-D uint8 CUDA tensor `t` (or slice, any offset) -> (counts, over), numpy, as
    api.RankFile.count_classes.  Indexed where it lies; of the text only the few bytes at its two ends that the longest pattern
    asks for reach the host.  Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "count_classes_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        return api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c).count_classes(patterns, cyclic=cyclic, max_nodes=max_nodes, ignore_case=ignore_case)
    finally:
        if own:
            c.close()


def count_classes_in_archive(blob, patterns, cyclic=False, max_nodes=None, ignore_case=False, device="cuda:0"):
    """count_classes_tensor on what an archive holds, decoded as count_in_archive decodes it: hits across block boundaries included."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return count_classes_tensor(decompress_container_tensor(blob, device=device), patterns, cyclic=cyclic, max_nodes=max_nodes, ignore_case=ignore_case)


def locate_classes_tensor(t, patterns, cyclic=False, max_nodes=None, ignore_case=False, ctx=None):
    """Where patterns of byte classes occur in the 1-D uint8 CUDA tensor `t` (or slice, any offset) -> (offsets, positions, over),
    all tensors on t's device: int64[npat + 1], int32[total] and bool[npat].  Pattern p owns positions[offsets[p]:offsets[p + 1]],
    ascending byte offsets into t; over[p]: its search ran out of `max_nodes` and it has none.  Patterns, cyclic, max_nodes and
    ignore_case: as api.RankFile.locate_classes.  Searched, gathered and ordered on the device (bce_hip_locate_classes_device, a
    sizing call first); of the answer only its total reaches the host.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "locate_classes_tensor", "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        _ready(t)
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        _, pats, flat, lens, _ = rf._class_args(patterns, cyclic, max_nodes, ignore_case, "hits")
        offsets = torch.zeros(len(pats) + 1, dtype=torch.int64, device=t.device)
        status = torch.zeros(len(pats), dtype=torch.int32, device=t.device)
        if not pats:
            return offsets, torch.empty(0, dtype=torch.int32, device=t.device), status != 0
        d_mask, d_off = torch.from_numpy(flat.view(np.int32)).to(t.device), torch.from_numpy(lens.astype(np.int64)).to(t.device)
        torch.cuda.current_stream(t.device).synchronize()
        args = (d_mask.data_ptr(), d_off.data_ptr(), len(pats), offsets.data_ptr(), status.data_ptr())
        total = rf.locate_classes_device(*args, None, 0, cyclic=cyclic, max_nodes=max_nodes)
        positions = torch.empty(total, dtype=torch.int32, device=t.device)
        if total:
            torch.cuda.current_stream(t.device).synchronize()        # (the allocator may hand out memory a queued kernel still uses)
            rf.locate_classes_device(*args, positions.data_ptr(), total, cyclic=cyclic, max_nodes=max_nodes)
        return offsets, positions, status != 0
    finally:
        if own:
            c.close()


def locate_classes_in_archive(blob, patterns, cyclic=False, max_nodes=None, ignore_case=False, device="cuda:0"):
    """locate_classes_tensor on what an archive holds, decoded as count_in_archive decodes it -> (offsets, positions, over) on `device`."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return locate_classes_tensor(decompress_container_tensor(blob, device=device), patterns, cyclic=cyclic, max_nodes=max_nodes, ignore_case=ignore_case)


def _match_args(t, query, what):
    _check(t, "t")
    _check(query, "query")
    if query.device != t.device:
        raise ValueError("query must lie on t's device")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, what, "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    if query.numel() > _MAX_BLOCK:
        raise ValueError("a query is less than 2^31 bytes, not %d" % query.numel())
    return n


def match_tensor(t, query, max_len, cyclic=False, positions=True, ctx=None):
    """The matching statistics of the 1-D uint8 CUDA tensor `query` against the 1-D uint8 CUDA tensor `t` (slices at any offset,
    same device) -> (lens, pos), int32 tensors on that device as long as the query: as api.RankFile.match, with positions of -1
    (0xFFFFFFFF) where lens is 0, pos None with positions=False.  The text is indexed where it lies and the query searched where
    it lies (bce_hip_match_device); nothing of either reaches the host.
    Synchronises the current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    n = _match_args(t, query, "match_tensor")
    q = query.numel()
    lens = torch.zeros(q, dtype=torch.int32, device=t.device)
    pos = torch.full((q,), -1, dtype=torch.int32, device=t.device) if positions else None
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        if q:
            rf.match_device(query.data_ptr(), q, max_len, lens.data_ptr(), pos.data_ptr() if positions else None, cyclic=cyclic)
        return lens, pos
    finally:
        if own:
            c.close()


def coverage_tensor(t, query, min_len, cyclic=False, ctx=None) -> int:
    """How many bytes of the CUDA tensor `query` lie in strings of min_len bytes or more that occur in the CUDA tensor `t` (both 1-D
    uint8, same device): api.RankFile.coverage with both buffers where they lie (bce_hip_coverage_device); 8 bytes reach the host.
    Synchronises the current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    n = _match_args(t, query, "coverage_tensor")
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        return rf.coverage_device(query.data_ptr() if query.numel() else None, query.numel(), min_len, cyclic=cyclic)
    finally:
        if own:
            c.close()


def parse_tensor(t, query, min_len, max_len=api.PARSE_MAX_LEN, ctx=None):
    """The 1-D uint8 CUDA tensor `query` as copies out of the 1-D uint8 CUDA tensor `t` plus literal bytes (api.RankFile.parse with
    both buffers where they lie: bce_hip_parse_device, a sizing call and the full call) -> (ops, lits, info): ops an int32 tensor
    (nops, 2) of (len, src) on that device, src == -1 (0xFFFFFFFF) for a run of literal bytes; lits a uint8 tensor; info a dict.
    Nothing but info reaches the host.  Synchronises the current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    n = _match_args(t, query, "parse_tensor")
    q = query.numel()
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c)
        info = rf.parse_device(query.data_ptr() if q else None, q, min_len, max_len)
        ops = torch.zeros((info["nops"], 2), dtype=torch.int32, device=t.device)
        lits = torch.zeros(info["nlits"], dtype=torch.uint8, device=t.device)
        if q:
            torch.cuda.synchronize(t.device)
            info = rf.parse_device(query.data_ptr(), q, min_len, max_len, ops.data_ptr(), info["nops"], lits.data_ptr() if info["nlits"] else None, info["nlits"])
        return ops, lits, info
    finally:
        if own:
            c.close()


def patch_tensor(t, ops, lits, out=None, ctx=None):
    """The bytes that `ops` (an int32 CUDA tensor (nops, 2) of (len, src)) and `lits` (a uint8 CUDA tensor) describe over the 1-D
    uint8 CUDA tensor `t` (bce_hip_patch_device: validated, sized, then copied on the GPU) -> a uint8 tensor on that device: `out`
    (its first bytes; it must be large enough) or a new one.  Only the result's length reaches the host."""
    n = _match_args(t, lits, "patch_tensor")
    if not isinstance(ops, torch.Tensor) or ops.dtype != torch.int32 or ops.dim() != 2 or ops.shape[1] != 2 or ops.device != t.device or not ops.is_contiguous():
        raise ValueError("ops must be a contiguous int32 tensor (nops, 2) on t's device")
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rf = api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c, build=False, index=False)
        args = (ops.data_ptr() if ops.shape[0] else None, ops.shape[0], lits.data_ptr() if lits.numel() else None, lits.numel())
        total = rf.patch_device(*args)
        if out is None:
            out = torch.zeros(total, dtype=torch.uint8, device=t.device)
            torch.cuda.synchronize(t.device)
        else:
            _check(out, "out")
            if out.device != t.device or out.numel() < total:
                raise ValueError("out must hold %d bytes on t's device" % total)
        if total:
            rf.patch_device(*(args + (out.data_ptr(), out.numel())))
        return out[:total]
    finally:
        if own:
            c.close()


def coverage_in_archive(blob, query, min_len, cyclic=False, device="cuda:0") -> int:
    """coverage_tensor on what an archive holds, decoded as count_in_archive decodes it: into ONE tensor on the device, so matches
    across block boundaries count.  `query`: a bytes-like (it is sent to the device) or a 1-D uint8 CUDA tensor there."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    if not isinstance(query, torch.Tensor):
        query = torch.from_numpy(api._as_u8(query).copy()).to(device)
    return coverage_tensor(decompress_container_tensor(blob, device=device), query, min_len, cyclic=cyclic)


def _indexed(t, what, ctx, use):
    """use(RankFile of the 1-D uint8 CUDA tensor t, indexed where it lies) with a context of t's device."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, what, "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one index covers one text of less than 2^31 bytes, not %d" % n)
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        return use(api.RankFile(n=n, device_ptr=t.data_ptr(), ctx=c))
    finally:
        if own:
            c.close()


def lcp_tensor(t, max_len, ctx=None):
    """The LCP array of the sorted rotations of the circular text in the 1-D uint8 CUDA tensor `t` -> an int32 tensor of n words on
    t's device (api.RankFile.lcp; the values are at most 4096).  The text is indexed where it lies and the array is written where
    it stays (bce_hip_lcp_device); nothing reaches the host.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    def use(rf):
        out = torch.zeros(t.numel(), dtype=torch.int32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()            # (the zero fill is done before the library's stream writes)
        rf.lcp_device(max_len, out.data_ptr())
        return out
    return _indexed(t, "lcp_tensor", ctx, use)


def lpf_tensor(t, max_len=api.PARSE_MAX_LEN, ctx=None):
    """The longest previous factors of the linear text in the 1-D uint8 CUDA tensor `t` (api.RankFile.lpf, everything left where it
    is: bce_hip_lpf_device) -> (lpf, src), int32 tensors of n words on t's device; src == -1 (0xFFFFFFFF) where lpf == 0.  Nothing
    reaches the host.  Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    def use(rf):
        out = torch.zeros(t.numel(), dtype=torch.int32, device=t.device)
        src = torch.zeros(t.numel(), dtype=torch.int32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()            # (the zero fills are done before the library's stream writes)
        rf.lpf_device(max_len, out.data_ptr(), src.data_ptr())
        return out, src
    return _indexed(t, "lpf_tensor", ctx, use)


def _sorted_text(t, what):
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, what, "empty input")
    if n > _MAX_BLOCK:
        raise ValueError("one suffix array covers one text of less than 2^31 bytes, not %d" % n)
    return n


def suffix_array_tensor(t, inverse=False, ctx=None):
    """The suffix array of the linear text in the 1-D uint8 CUDA tensor `t` (bce_hip_suffix_array_device) -> an int32 tensor of n
    rows on t's device, or (sa, isa) with inverse=True.  The text is sorted where it lies and the arrays are written where they
    stay; only the status reaches the host.  The context's compression state is dropped.
    Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    n = _sorted_text(t, "suffix_array_tensor")
    sa = torch.zeros(n, dtype=torch.int32, device=t.device)
    isa = torch.zeros(n, dtype=torch.int32, device=t.device) if inverse else None
    _ready(t)                                                         # (the zero fills too are done before the library's stream writes)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        c.check(api.suffix_array_device(t.data_ptr(), n, sa.data_ptr(), isa.data_ptr() if inverse else None, ctx=c), "bce_hip_suffix_array_device")
        return (sa, isa) if inverse else sa
    finally:
        if own:
            c.close()


def sufcheck_tensor(t, sa, ctx=None):
    """Is the 1-D int32 CUDA tensor `sa` the suffix array of the 1-D uint8 CUDA tensor `t`?  Checked where both lie
    (bce_hip_sufcheck_device) -> what api.sufcheck returns: None, or (reason, index).  Twelve bytes reach the host.
    Synchronises the current stream of t's device first; `ctx` (an api._Ctx of t's device) is reused if given."""
    n = _sorted_text(t, "sufcheck_tensor")
    if not isinstance(sa, torch.Tensor) or sa.dtype != torch.int32 or sa.dim() != 1 or sa.device != t.device or not sa.is_contiguous() or sa.numel() != n:
        raise ValueError("sa must be a contiguous 1-D int32 tensor of t's length on t's device")
    _ready(t)
    own = ctx is None
    c = ctx or api._Ctx(t.device.index)
    try:
        rc, verdict = api.sufcheck_device(t.data_ptr(), sa.data_ptr(), n, c)
        c.check(rc, "bce_hip_sufcheck_device")
        return verdict
    finally:
        if own:
            c.close()


def self_parse_tensor(t, min_len, max_len=api.PARSE_MAX_LEN, ctx=None):
    """The 1-D uint8 CUDA tensor `t` as copies of its own earlier bytes plus literal bytes (api.RankFile.self_parse with the outputs
    where they stay: bce_hip_self_parse_device, a sizing call and the full call) -> (ops, lits, info) as parse_tensor gives them.
    Nothing but info reaches the host."""
    def use(rf):
        info = rf.self_parse_device(min_len, max_len)
        ops = torch.zeros((info["nops"], 2), dtype=torch.int32, device=t.device)
        lits = torch.zeros(info["nlits"], dtype=torch.uint8, device=t.device)
        torch.cuda.synchronize(t.device)
        info = rf.self_parse_device(min_len, max_len, ops.data_ptr(), info["nops"], lits.data_ptr() if info["nlits"] else None, info["nlits"])
        return ops, lits, info
    return _indexed(t, "self_parse_tensor", ctx, use)


def self_parse_in_archive(blob, min_len, max_len=api.PARSE_MAX_LEN, device="cuda:0"):
    """self_parse_tensor on what an archive holds, decoded as count_in_archive decodes it: into ONE tensor on the device, so a
    copy may reach back across block boundaries.  A container of 2^31 bytes or more: ValueError, before anything is decoded."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return self_parse_tensor(decompress_container_tensor(blob, device=device), min_len, max_len)


def kgrams_tensor(t, ks, ctx=None):
    """api.RankFile.kgrams of the 1-D uint8 CUDA tensor `t`, indexed and reduced where it lies; 32 bytes per k reach the host."""
    return _indexed(t, "kgrams_tensor", ctx, lambda rf: rf.kgrams(ks))


def entropy_profile_tensor(t, K, ctx=None):
    """[H_0 .. H_K] of the circular text in the 1-D uint8 CUDA tensor `t` (api.RankFile.entropy_profile)."""
    return _indexed(t, "entropy_profile_tensor", ctx, lambda rf: rf.entropy_profile(K))


def entropy_profile_in_archive(blob, K, device="cuda:0"):
    """entropy_profile_tensor on what an archive holds, decoded as count_in_archive decodes it: into ONE tensor on the device, so
    the profile is that of the concatenated blocks.  A container of 2^31 bytes or more: ValueError, before anything is decoded."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return entropy_profile_tensor(decompress_container_tensor(blob, device=device), K)


def top_kgrams_tensor(t, k, limit, with_bytes=True, ctx=None):
    """The `limit` most frequent cyclic k-grams of the 1-D uint8 CUDA tensor `t` (api.RankFile.top_kgrams with everything left on
    the device: bce_hip_top_kgrams_device) -> (entries, grams, distinct, size_hist): entries an int32 tensor (found, 3) of (count,
    row, pos) on t's device, by count descending and equal counts in the order of the bytes; grams a uint8 tensor (found, k) of the
    k-grams (None with with_bytes=False); distinct and size_hist as api.TopKGrams has them.  Only those 33 numbers and `found`
    reach the host.  Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    k, limit = api._top_limit(k, limit)
    sound = 1 <= limit <= api.TOP_MAX and k <= api.MATCH_MAX_LEN          # (otherwise the library refuses: no room is made)

    def use(rf):
        ent = torch.zeros((limit if sound else 1, 3), dtype=torch.int32, device=t.device)
        grams = torch.zeros((limit if sound else 1, max(k, 1) if sound else 1), dtype=torch.uint8, device=t.device) if with_bytes else None
        torch.cuda.current_stream(t.device).synchronize()            # (the zero fills are done before the library's stream writes)
        found, distinct, hist = rf.top_kgrams_device(k, limit, ent.data_ptr(), grams.data_ptr() if with_bytes else None, limit * k if with_bytes else 0)
        if with_bytes:
            grams = grams.reshape(-1)[:found * k].reshape(found, k)
        return ent[:found], grams, distinct, hist
    return _indexed(t, "top_kgrams_tensor", ctx, use)


def top_kgrams_in_archive(blob, k, limit, with_bytes=True, device="cuda:0"):
    """top_kgrams_tensor on what an archive holds, decoded as count_in_archive decodes it: into ONE tensor on the device, so the
    k-grams across block boundaries count.  A container of 2^31 bytes or more: ValueError, before anything is decoded."""
    total = sum(t[0] for t in _blocks_of(blob))
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return top_kgrams_tensor(decompress_container_tensor(blob, device=device), k, limit, with_bytes=with_bytes)


def maximal_repeats_tensor(t, min_len=1, max_len=api.MATCH_MAX_LEN, order="len", limit=100, bytes_per=64, ctx=None):
    """The maximal repeats of the circular text in the 1-D uint8 CUDA tensor `t` (api.RankFile.maximal_repeats with everything left
    on the device: bce_hip_maximal_repeats_device) -> (entries, strings, info): entries an int32 tensor (found, 4) of (len, count,
    row, pos) on t's device, heaviest first; strings a uint8 tensor (found, bytes_per), every row the first min(len, bytes_per)
    bytes of its repeat and zeros behind them (None with bytes_per=0); info the dict (total, capped, bwt_runs, found), all that
    reaches the host.  Synchronises t's current stream first; `ctx` (an api._Ctx of t's device) is reused if given."""
    min_len, max_len, order, limit, bytes_per = api._maxrep_args(min_len, max_len, order, limit, bytes_per)
    sound = 1 <= limit <= api.TOP_MAX and bytes_per <= api.MAXREP_BYTES_MAX   # (otherwise the library refuses: no room is made)

    def use(rf):
        ent = torch.zeros((limit if sound else 1, 4), dtype=torch.int32, device=t.device)
        raw = torch.zeros((limit if sound else 1, bytes_per if sound else 1), dtype=torch.uint8, device=t.device) if bytes_per else None
        torch.cuda.current_stream(t.device).synchronize()            # (the zero fills are done before the library's stream writes)
        info = rf.maximal_repeats_device(min_len, max_len, order, limit, ent.data_ptr(), raw.data_ptr() if bytes_per else None, bytes_per,
                                         limit * bytes_per if bytes_per else 0)
        return ent[:info["found"]], raw[:info["found"]] if bytes_per else None, info
    return _indexed(t, "maximal_repeats_tensor", ctx, use)


def maximal_repeats_in_archive(blob, min_len=1, max_len=api.MATCH_MAX_LEN, order="len", limit=100, bytes_per=64, device="cuda:0", per_block=False):
    """maximal_repeats_tensor on what an archive holds, decoded as count_in_archive decodes it: into ONE tensor on the device, so
    the repeats across block boundaries count.  A container of 2^31 bytes or more: ValueError, before anything is decoded.
    per_block: every block of a container is a text of its own -- a list with one (entries, strings, info) per block (one for a
    plain archive), each block decoded into a tensor of its own and indexed there."""
    table = _blocks_of(blob)
    if per_block:
        view = memoryview(blob)
        return [maximal_repeats_tensor(decompress_container_tensor(bytes(view[pos:pos + alen]), device=device), min_len, max_len, order, limit, bytes_per)
                for _raw, pos, alen, _crc in table]
    total = sum(t[0] for t in table)
    if total > _MAX_BLOCK:
        raise ValueError("the archive holds %d bytes: one index covers one text of less than 2^31" % total)
    return maximal_repeats_tensor(decompress_container_tensor(blob, device=device), min_len, max_len, order, limit, bytes_per)


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


def compress_tensor_blocks(t, blocks=None, config=None, contexts=4, checksum=True):
    """A 1-D uint8 CUDA tensor of ANY size >= 1 -> a BCEM container (host bytes): `blocks` contiguous blocks
    (sharding.block_range; default: the fewest that keep every block below 2^31 bytes), each compressed from its slice in
    HBM by a pool of `contexts` gated contexts of t's device.  checksum=True: a version-2 container with the CRC-32 of
    every block, taken on the device by the context that compresses it; False: version 1, what `bce -cN` writes.
    Synchronises t's current stream first."""
    _check(t, "t")
    n = t.numel()
    if n == 0:
        raise api.BceError(-1, "compress_tensor_blocks", "empty input")
    if blocks is None:
        blocks = (n + _MAX_BLOCK - 1) // _MAX_BLOCK
    blocks = int(blocks)
    if blocks < 1 or blocks > n or (n + blocks - 1) // blocks > _MAX_BLOCK:
        raise ValueError("%d blocks do not split %d bytes into blocks of 1 .. 2^31 - 1 bytes" % (blocks, n))
    _ready(t)
    ranges = [block_range(n, blocks, b) for b in range(blocks)]
    base = t.data_ptr()
    with api.ContextPool(contexts, t.device.index) as pool:
        res = pool.compress_many([(base + lo, hi - lo) for lo, hi in ranges], config=config, on_device=True, with_crc=checksum)
    sizes = [hi - lo for lo, hi in ranges]
    if checksum:
        return container.pack_blocks([bytes(a) for a, _ in res], sizes, [c for _, c in res])
    return container.pack_blocks([bytes(a) for a in res], sizes)


def _blocks_of(blob):
    """(table, checked): the blocks of a container, or the one block of a plain archive; every raw size is the one the
    block's own header states (the CLI's rule: a lying table is refused before anything is written)."""
    if bytes(blob[:4]) == container.MAGIC:
        table = container.block_table(blob)
    else:
        table = [(api.decoded_size(blob), 0, len(blob), None)]
    for b, (raw, pos, alen, _crc) in enumerate(table):
        if raw < 1 or raw > _MAX_BLOCK or api.decoded_size(memoryview(blob)[pos:pos + alen]) != raw:
            raise ValueError("block %d: the table's size is not the block's own" % b)
    return table


def decompress_container_tensor(blob, device="cuda:0", out=None, check=True):
    """A BCEM container (either version) or a plain archive -> ONE 1-D uint8 tensor on the device: every block is decoded
    straight into its slice (bce_hip_decompress_to_device), nothing of the text crosses to the host.  With `check`, a
    version-2 container's blocks are tested there against the table's CRC-32 (bce_hip_crc32_device): ChecksumError
    names the first block that differs -- the slices behind it have not been written.  `out`: as decompress_tensor."""
    table = _blocks_of(blob)
    total = sum(t[0] for t in table)
    if out is not None:
        _check(out, "out")
        if out.numel() < total:
            raise api.BceError(-5, "decompress_container_tensor", "out holds %d bytes, the container %d" % (out.numel(), total))
        res = out[:total]
    else:
        res = torch.empty(total, dtype=torch.uint8, device=torch.device("cuda", _device_index(device)))
    _ready(res)
    view = memoryview(blob)
    c = api._Ctx(res.device.index)
    try:
        at = 0
        for b, (raw, pos, alen, crc) in enumerate(table):
            ptr = res.data_ptr() + at
            api.decompress_to_device(view[pos:pos + alen], ptr, raw, ctx=c)
            if check and crc is not None:
                got = api.crc32_device(ptr, raw, ctx=c)
                if got != crc:
                    raise api.ChecksumError(b, crc, got)
            at += raw
    finally:
        c.close()
    return res


def test_container(blob, device="cuda:0", raise_on_refusal=False):
    """Test a version-2 container against its own CRC-32s: every block is decoded on the GPU into the context's buffer and
    checksummed there (bce_hip_decode_crc32); nothing is kept.  -> None when every block matches, else the index of the
    first that does not -- or that the decoder refuses by itself (status -1: the block does not parse, -6: it decodes to
    nonsense; -6 is also what a consistency failure of the decoder's own would give, so raise_on_refusal=True hands that
    BceError, with the library's message, to the caller instead).  ValueError: nothing to check (a plain archive, a version-1 container)."""
    if bytes(blob[:4]) != container.MAGIC:
        raise ValueError("a plain archive carries no checksum: verify it against the original (verify_tensor)")
    table = _blocks_of(blob)
    if any(t[3] is None for t in table):
        raise ValueError("a version-1 container carries no checksum: verify it against the original")
    view = memoryview(blob)
    c = api._Ctx(_device_index(device))
    try:
        for b, (raw, pos, alen, crc) in enumerate(table):
            try:
                n, got = api.decode_crc32(view[pos:pos + alen], ctx=c)
            except api.BceError as e:
                if e.status in (-1, -6) and not raise_on_refusal:   # the decoder itself refuses the block
                    return b
                raise
            if n != raw or got != crc:
                return b
    finally:
        c.close()
    return None


test_container.__test__ = False      # (a library function, not a test: its name starts with "test")
