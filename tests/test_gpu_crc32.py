"""GPU: the CRC-32 pass over device memory (kd_crc32.hip) against zlib.crc32: any alignment, any length (0 .. beyond 2^32),
constant, random and text data; the input's CRC in a compressing context; decode-and-checksum without a host copy."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import bce_amd
import oracle
from bce_amd import api
from conftest import edge_inputs

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 10**8]


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _source(kind):
    n = 10**8 + 64
    if kind == "constant":
        return np.full(n, 0x5A, dtype=np.uint8)
    if kind == "random":
        return bce_amd.synth_rand(11, n)
    return bce_amd.synth_text(3, n)


@pytest.mark.parametrize("kind", ["constant", "random", "text"])
def test_crc32_device_is_zlibs_on_slices_of_one_tensor(ctx, kind):
    host = _source(kind)
    t = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    hb = memoryview(host)                                   # (slices without a copy)
    for off in range(18):
        for n in LENGTHS:
            got = api.crc32_device(t.data_ptr() + off, n, ctx=ctx)
            assert got == zlib.crc32(hb[off:off + n]), (kind, off, n, hex(got))


def test_crc32_device_beyond_2_to_the_32(ctx):
    n = (1 << 32) + 5
    t = torch.empty(n + 3, dtype=torch.uint8, device="cuda:0")
    # filled on the device: a byte pattern with a long period, so that a piece lost, doubled or misplaced changes the CRC
    step = 1 << 28
    for lo in range(0, n + 3, step):
        hi = min(n + 3, lo + step)
        i = torch.arange(lo, hi, dtype=torch.int64, device="cuda:0")
        t[lo:hi] = ((i * 2654435761 + (i >> 13)) >> 7).to(torch.uint8)
        del i
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    for off in (0, 3):
        want = zlib.crc32(memoryview(host)[off:off + n])
        assert api.crc32_device(t.data_ptr() + off, n, ctx=ctx) == want, off


def test_crc32_device_arguments(ctx):
    crc = C.c_uint32(9)
    assert ctx.lib.bce_hip_crc32_device(ctx.h, None, 0, C.byref(crc)) == 0 and crc.value == 0      # n == 0: d ignored
    assert ctx.lib.bce_hip_crc32_device(ctx.h, None, 16, C.byref(crc)) == E_ARG
    t = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.lib.bce_hip_crc32_device(ctx.h, t.data_ptr(), 16, None) == E_ARG
    n = C.c_size_t(0)
    a = np.frombuffer(oracle.compress(b"abracadabra"), dtype=np.uint8)
    assert ctx.lib.bce_hip_decode_crc32(ctx.h, a.ctypes.data, len(a), C.byref(n), None) == E_ARG
    assert ctx.lib.bce_hip_decode_crc32(ctx.h, a.ctypes.data, len(a), None, C.byref(crc)) == E_ARG
    assert ctx.lib.bce_hip_decode_crc32(ctx.h, None, 0, C.byref(n), C.byref(crc)) == E_ARG
    assert ctx.lib.bce_hip_input_crc32(ctx.h, None) == E_ARG


def test_input_crc32_after_either_load_and_its_window():
    c = api._Ctx(0)
    try:
        crc = C.c_uint32(5)
        assert c.lib.bce_hip_input_crc32(c.h, C.byref(crc)) == E_STATE and crc.value == 5          # nothing loaded yet
        data = bce_amd.synth_text(21, 300001)
        want = zlib.crc32(data.tobytes())
        c.check(c.lib.bce_hip_load_host(c.h, data.ctypes.data, len(data)), "load_host")
        assert api.input_crc32(c) == want
        t = torch.from_numpy(data).to("cuda:0")
        torch.cuda.synchronize()
        c.check(c.lib.bce_hip_load_device(c.h, t.data_ptr() + 1, len(data) - 1), "load_device")      # (an odd start)
        want1 = zlib.crc32(data.tobytes()[1:])
        assert api.input_crc32(c) == want1
        # the context keeps the input through every stage of the compression: the window stays open
        rf = api.RankFile(n=len(data) - 1, device_ptr=t.data_ptr() + 1, ctx=c)
        assert api.input_crc32(c) == want1
        arch = api.BCE().encode(rf)
        assert bytes(arch) == oracle.compress(data.tobytes()[1:])
        assert api.input_crc32(c) == want1
        # ... until the buffer is taken for something else: a decode, an injected BWT
        assert api.decode_crc32(arch, ctx=c) == (len(data) - 1, want1)
        assert c.lib.bce_hip_input_crc32(c.h, C.byref(crc)) == E_STATE
        c.check(c.lib.bce_hip_load_host(c.h, data.ctypes.data, 1000), "load_host")
        assert api.input_crc32(c) == zlib.crc32(data.tobytes()[:1000])
        bwt = np.zeros(10, dtype=np.uint8)
        c.check(c.lib.bce_hip_set_bwt(c.h, bwt.ctypes.data, 10, 0), "set_bwt")
        assert c.lib.bce_hip_input_crc32(c.h, C.byref(crc)) == E_STATE
    finally:
        c.close()


@pytest.mark.parametrize("name,data", edge_inputs(), ids=[n for n, _ in edge_inputs()])
def test_decode_crc32_of_oracle_archives(ctx, name, data):
    assert api.decode_crc32(oracle.compress(data), ctx=ctx) == (len(data), zlib.crc32(data))


def test_decode_crc32_of_ten_million_bytes_and_of_garbage(ctx):
    data = bce_amd.synth_text(8, 10**7)
    arch = oracle.compress(data.tobytes())
    assert api.decode_crc32(arch, ctx=ctx) == (10**7, zlib.crc32(data.tobytes()))
    n, crc = C.c_size_t(3), C.c_uint32(4)
    bad = np.frombuffer(b"\xff" * 64, dtype=np.uint8)
    assert ctx.lib.bce_hip_decode_crc32(ctx.h, bad.ctypes.data, len(bad), C.byref(n), C.byref(crc)) != 0
    assert (n.value, crc.value) == (3, 4)                     # outputs untouched
    # the host copy's companion: the same word beside the bytes
    out = np.empty(10**7, dtype=np.uint8)
    m = C.c_size_t()
    a = np.frombuffer(bytes(arch), dtype=np.uint8)
    ctx.check(ctx.lib.bce_hip_decompress_device_crc32(ctx.h, a.ctypes.data, len(a), out.ctypes.data, out.size, C.byref(m), C.byref(crc)),
              "bce_hip_decompress_device_crc32")
    assert m.value == 10**7 and crc.value == zlib.crc32(data.tobytes()) and np.array_equal(out, data)
