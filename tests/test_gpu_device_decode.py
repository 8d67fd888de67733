"""GPU: the decoder with the text left on the device (bce_hip_decompress_to_device) and the on-device check of an archive against
its original (bce_hip_verify_device / _host; kd_compare.hip), through bce_amd.tensor.

Archives come from the oracle (the reference's `-c`), as in test_gpu_decode.py.  Every comparison is exact."""
import re

import numpy as np
import pytest
import torch

import bce_amd
import oracle
from conftest import edge_inputs

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
OVERFLOW = -5


def _byte_cases():
    cases = list(edge_inputs())
    cases += [
        ("text-300k", oracle.synth_text(3, 300000)),
        ("rand-100k", oracle.synth_rand(4, 100000)),
        ("text-2M", oracle.synth_text(1, 2 << 20)),
        ("periodic-x7", oracle.synth_text(2, 5000) * 7),
    ]
    return cases


BYTE_CASES = _byte_cases()


@pytest.fixture
def ctx():
    torch.zeros(1, device="cuda:0")                  # (torch's runtime first, then the library's context: as smoke())
    c = bce_amd.api._Ctx(0)
    yield c
    c.close()


def _gpu(data, offset=0):
    """`data` as a uint8 tensor on the device that starts `offset` bytes into its allocation."""
    buf = torch.empty(len(data) + offset, dtype=torch.uint8, device="cuda:0")
    t = buf[offset:]
    if len(data):
        t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    torch.cuda.synchronize()
    return t


# ---- 1. bytes ----
@pytest.mark.parametrize("name,data", BYTE_CASES, ids=[c[0] for c in BYTE_CASES])
def test_decode_to_device_gives_the_input(name, data, ctx):
    data = bytes(data)
    arch = oracle.compress(data)
    t = bce_amd.decompress_tensor(arch, ctx=ctx)
    assert t.is_cuda and t.dtype == torch.uint8 and t.shape == (len(data),)
    got = t.cpu().numpy().tobytes()
    assert got == data
    assert got == bce_amd.decompress_device(arch, ctx=ctx)
    assert bce_amd.decompress_tensor(arch).cpu().numpy().tobytes() == data        # a context of its own


def test_decode_to_device_custom_config(ctx):
    data = oracle.synth_text(12, 200000)
    cfg, _ = oracle.scan(data)
    arch = oracle.compress(data, bytes(cfg))
    got = bce_amd.decompress_tensor(arch, ctx=ctx).cpu().numpy().tobytes()
    assert got == data == bce_amd.decompress_device(arch, ctx=ctx)


def test_size_query_and_null_archive(ctx):
    data = oracle.synth_text(3, 5000)
    arch = oracle.compress(data)
    assert bce_amd.decompress_to_device(arch, None, 0, ctx=ctx) == len(data)
    import ctypes as C
    n, fd = C.c_size_t(), C.c_uint64(7)
    t = _gpu(data)
    assert ctx.lib.bce_hip_decompress_to_device(ctx.h, None, 16, t.data_ptr(), len(data), C.byref(n)) == -1
    assert ctx.lib.bce_hip_verify_device(ctx.h, None, 16, t.data_ptr(), len(data), C.byref(fd)) == -1
    assert ctx.lib.bce_hip_verify_host(ctx.h, None, 16, None, 0, C.byref(fd)) == -1
    assert fd.value == 7
    assert torch.equal(bce_amd.decompress_tensor(arch, ctx=ctx), t)              # the context is none the worse


# ---- 2. bounds ----
BOUND_CASES = [("len-97", oracle.synth_text(5, 97)), ("len-3073", oracle.synth_text(7, 3073)), ("text-300k", oracle.synth_text(3, 300000)),
               ("periodic-x7", oracle.synth_text(2, 5000) * 7), ("one-byte", b"a")]


@pytest.mark.parametrize("name,data", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_decode_into_a_slice_touches_nothing_else(name, data, ctx):
    data = bytes(data)
    n = len(data)
    arch = oracle.compress(data)
    want = np.frombuffer(data, dtype=np.uint8)
    for k in (0, 1, 3, 16):
        buf = torch.full((n + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
        res = bce_amd.decompress_tensor(arch, out=buf[k:k + n], ctx=ctx)
        assert res.data_ptr() == buf.data_ptr() + k and res.numel() == n
        h = buf.cpu().numpy()
        assert np.array_equal(h[k:k + n], want), k
        assert (h[:k] == PATTERN).all() and (h[k + n:] == PATTERN).all(), k     # a vector store that overruns would show here
        if n > 1:
            # one byte too few: refused, nothing written anywhere
            buf = torch.full((n + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
            with pytest.raises(bce_amd.BceError) as e:
                bce_amd.decompress_tensor(arch, out=buf[k:k + n - 1], ctx=ctx)
            assert e.value.status == OVERFLOW
            assert (buf.cpu().numpy() == PATTERN).all(), k


# ---- 3. verify ----
VERIFY_INPUTS = [("n1", b"q"), ("n2", b"qr"), ("n97", oracle.synth_text(5, 97)), ("n3073", oracle.synth_text(7, 3073)),
                 ("n2Mi", oracle.synth_text(1, 2 << 20))]


@pytest.mark.parametrize("name,data", VERIFY_INPUTS, ids=[c[0] for c in VERIFY_INPUTS])
def test_verify_reports_the_first_difference(name, data, ctx):
    data = bytes(data)
    n = len(data)
    arch = oracle.compress(data)
    # equal: host bytes, and a tensor at offsets 0 and 1
    assert bce_amd.verify(arch, data, ctx=ctx) is None
    for off in (0, 1):
        assert bce_amd.verify_tensor(arch, _gpu(data, off), ctx=ctx) is None

    def flipped(*idx):
        b = bytearray(data)
        for i in idx:
            b[i] ^= 0x40
        return bytes(b)

    flips = sorted({i for i in (0, 1, 15, 16, 17, n // 2, n - 1) if 0 <= i < n})
    for i in flips:
        bad = flipped(i)
        assert bce_amd.verify(arch, bad, ctx=ctx) == i, i
        for off in (0, 1):
            assert bce_amd.verify_tensor(arch, _gpu(bad, off), ctx=ctx) == i, (i, off)
    # two flips: the smaller index
    if n >= 2:
        pairs = [(0, n - 1), (n // 2, n - 1)] + ([(17, n // 2), (n // 3, n - 2)] if n > 40 else [])
        for i, j in pairs:
            if i == j:
                continue
            bad = flipped(i, j)
            assert bce_amd.verify(arch, bad, ctx=ctx) == min(i, j)
            assert bce_amd.verify_tensor(arch, _gpu(bad, 1), ctx=ctx) == min(i, j)
    # one byte short, one byte long: min(n, decoded size); a difference in the common prefix wins
    short, long_ = data[:-1], data + b"!"
    assert bce_amd.verify(arch, short, ctx=ctx) == n - 1
    assert bce_amd.verify(arch, long_, ctx=ctx) == n
    assert bce_amd.verify_tensor(arch, _gpu(short, 1), ctx=ctx) == n - 1
    assert bce_amd.verify_tensor(arch, _gpu(long_, 1), ctx=ctx) == n
    if n >= 3:
        assert bce_amd.verify(arch, flipped(1) + b"!", ctx=ctx) == 1
        assert bce_amd.verify_tensor(arch, _gpu(flipped(1)[:-1], 3), ctx=ctx) == 1
    # the context still decodes
    assert bce_amd.decompress_tensor(arch, ctx=ctx).cpu().numpy().tobytes() == data


def test_verify_passes_the_decoders_status_on(ctx):
    data = oracle.synth_text(5, 100000)
    arch = oracle.compress(data)
    with pytest.raises(bce_amd.BceError):
        bce_amd.verify(arch[:7], data, ctx=ctx)
    with pytest.raises(bce_amd.BceError):
        bce_amd.verify_tensor(b"", _gpu(data), ctx=ctx)
    assert bce_amd.verify(arch, data, ctx=ctx) is None


# ---- 4. routes and memory modes ----
MODE_INPUTS = {"text-300k": lambda: oracle.synth_text(3, 300000), "rand-100k": lambda: oracle.synth_rand(4, 100000)}
MODE_CASES = ["grow", "groups", "alloc-retry", "give-back", "force-host-tail"]


@pytest.mark.parametrize("mode", MODE_CASES)
@pytest.mark.parametrize("name", list(MODE_INPUTS))
def test_to_device_under_routes_and_memory_modes(name, mode, ctx, capfd, monkeypatch):
    data = MODE_INPUTS[name]()
    arch = oracle.compress(data)
    monkeypatch.setenv("BCE_ALLOC_TRACE", "1")
    monkeypatch.setenv("BCE_DEC_TIMING", "1")

    def knob(k, v):
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, k, v), "bce_hip_debug_set")
    if mode == "grow":
        knob(12, 1 << 30)
    elif mode == "groups":
        knob(13, 4096)
    elif mode == "alloc-retry":
        assert bce_amd.compress(data, ctx=ctx) == arch          # (the encoder's buffers: what the first failed allocation gives back)
        knob(14, 3)
    elif mode == "give-back":
        monkeypatch.setenv("BCE_DEC_GIVE_BACK", "1")
    elif mode == "force-host-tail":
        monkeypatch.setenv("BCE_DEC_FORCE_HOST_TAIL", "1")
    s0 = bce_amd.stats_of(ctx)
    capfd.readouterr()
    t = bce_amd.decompress_tensor(arch, ctx=ctx)
    err = capfd.readouterr().err
    s1 = bce_amd.stats_of(ctx)
    assert t.cpu().numpy().tobytes() == data
    assert s1["dec_restarts"] == s0["dec_restarts"]
    assert "gpu decode: text left on the device" in err, err[-2000:]
    if mode == "grow":
        assert s1["dec_list_grows"] > s0["dec_list_grows"], (s0, s1)
    elif mode == "groups":
        assert s1["dec_split_rounds"] > s0["dec_split_rounds"], (s0, s1)
    elif mode == "alloc-retry":
        assert "out of device memory in phase 4" in err, err[-2000:]
        knob(14, 0)
    elif mode == "give-back":
        assert "node lists and query buffers given back" in err, err[-2000:]
    elif mode == "force-host-tail":
        # (the switch skips the tail probe and marks the tail query-heavy; whether a tail then goes to the host is the input's affair)
        assert re.search(r"gpu decode: tail probe: 0 rounds, 0 query rounds through the mailbox since it began; query-heavy 1", err), err[-2000:]
    # verify on the same route
    assert bce_amd.verify_tensor(arch, t, ctx=ctx) is None


# ---- 5. context reuse ----
def test_one_context_through_every_entry_point(ctx):
    data = oracle.synth_text(31, 250000)
    arch = oracle.compress(data)
    want = _gpu(data)
    assert torch.equal(bce_amd.decompress_tensor(arch, ctx=ctx), want)              # to the device
    assert bce_amd.decompress_device(arch, ctx=ctx) == data                         # to the host
    assert bce_amd.compress(data, ctx=ctx) == arch                                  # an encode
    assert bce_amd.verify_tensor(arch, want, ctx=ctx) is None                       # verify
    assert bce_amd.verify(arch, data, ctx=ctx) is None
    rf = bce_amd.RankFile(oracle.synth_text(3, 100000), ctx=ctx)                     # the stepping interface
    bce = bce_amd.BCE()
    bce.code_begin(rf)
    for _ in range(4):
        assert bce.code_round(rf) > 0
    u, primary = oracle.divbwt(data)                                                 # the libdivsufsort seam's inverse BWT
    a = np.frombuffer(u, dtype=np.uint8).copy()
    out = np.zeros(len(a), dtype=np.uint8)
    ctx.check(ctx.lib.bce_hip_inverse_bwt(ctx.h, a.ctypes.data, out.ctypes.data, len(a), primary), "bce_hip_inverse_bwt")
    assert out.tobytes() == data
    buf = torch.full((len(data) + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    res = bce_amd.decompress_tensor(arch, out=buf[5:], ctx=ctx)                      # to the device again
    assert torch.equal(res, want) and (buf[:5] == PATTERN).all() and (buf[5 + len(data):] == PATTERN).all()
    assert bce_amd.compress_tensor(want, ctx=ctx) == arch
    assert bce_amd.compress(data, ctx=ctx) == arch


# ---- 6. no host bounce ----
def _kinds(err):
    """The decoder's summary lines, each cut at its first digit."""
    return [re.split(r"\d", line, 1)[0] for line in err.splitlines() if line.startswith("gpu decode:")]


def test_the_text_is_not_copied_to_the_host(ctx, capfd, monkeypatch):
    data = oracle.synth_text(3, 300000)
    arch = oracle.compress(data)
    monkeypatch.setenv("BCE_DEC_TIMING", "1")
    bce_amd.decompress_device(arch, ctx=ctx)                                        # (warm: both runs below find the same buffers)
    capfd.readouterr()
    assert bce_amd.decompress_device(arch, ctx=ctx) == data
    host = capfd.readouterr().err
    t = bce_amd.decompress_tensor(arch, out=torch.empty(len(data), dtype=torch.uint8, device="cuda:0"), ctx=ctx)
    dev = capfd.readouterr().err
    assert t.cpu().numpy().tobytes() == data
    mark = "gpu decode: text left on the device"
    # the host path prints what it always printed: the inverse BWT's line, nothing about the device
    assert mark not in host and "gpu decode: inverse BWT (" in host and "gpu decode: planes + unbwt" in host, host[-2000:]
    # the device path: the same lines, and one of its own where the copy would be
    assert dev.count(mark) == 1 and "no copy to the host" in dev, dev[-2000:]
    hk, dk = _kinds(host), _kinds(dev)
    assert {k for k in dk if not k.startswith(mark)} == set(hk), (hk, dk)
    assert dk.index(next(k for k in dk if k.startswith(mark))) < dk.index("gpu decode: inverse BWT (one cycle, ")
    assert bce_amd.verify_tensor(arch, t, ctx=ctx) is None
    ver = capfd.readouterr().err
    assert "gpu decode: text left on the device, compared there with 300000 B of device memory" in ver, ver[-2000:]
