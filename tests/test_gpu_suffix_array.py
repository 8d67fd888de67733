"""GPU: the suffix array as a product (bce_hip_suffix_array / _device through bce_amd.suffix_array, suffix_array_device and
suffix_array_tensor) against tests/sa_ref.py: the array and its inverse on small and awkward texts; at 2^20 bytes of text and 300 000
random bytes the linear check, the inverse and the reference project's BWT; the device form between guard words; the refusals; and
what the call leaves of the context."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
import oracle
import sa_ref
from bce_amd import api

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _cases():
    rs = np.random.RandomState(31)
    out = [("n1", b"q"), ("n2", b"ba"), ("n2eq", b"aa"), ("n3", b"aba")]
    for n in (255, 256, 257, 2047, 2048, 2049):                           # K1's workgroup and chunk sizes
        out.append(("text%d" % n, oracle.synth_text(n, n)))
    out.append(("rand65537", oracle.synth_rand(3, 65537)))
    out.append(("one-symbol", b"\x07" * 1000))
    out.append(("two-symbols", bytes(rs.choice([65, 66], 3001).astype(np.uint8))))
    out.append(("256-symbols", bytes(range(256)) * 5 + bytes(rs.randint(0, 256, 777).astype(np.uint8))))
    out.append(("zeros-inside", bytes(rs.choice([0, 0, 0, 1, 255], 2500).astype(np.uint8)) + b"\x00\x00"))   # the sentinel sorts below byte 0
    out.append(("a5000", b"a" * 5000))
    out.append(("ab4000", b"ab" * 4000))
    out.append(("abc3333ab", b"abc" * 3333 + b"ab"))
    return out


CASES = _cases()


@pytest.mark.parametrize("name,t", CASES, ids=[c[0] for c in CASES])
def test_array_and_inverse_are_the_references(ctx, name, t):
    want = sa_ref.suffix_array(t)
    sa, isa = bce_amd.suffix_array(t, inverse=True, ctx=ctx)
    assert sa.dtype == np.int32 and isa.dtype == np.int32
    assert np.array_equal(sa, want), name
    assert np.array_equal(isa, sa_ref.inverse(want)), name
    assert np.array_equal(bce_amd.suffix_array(t, ctx=ctx), want)          # without the inverse


@pytest.fixture(scope="module")
def big():
    """name -> (text, suffix array and inverse from the GPU): sorted once, shared"""
    out = {}
    c = api._Ctx(0)
    for name, t in (("text", oracle.synth_text(3, 1 << 20)), ("rand", oracle.synth_rand(4, 300000))):
        out[name] = (t,) + bce_amd.suffix_array(t, inverse=True, ctx=c)
    c.close()
    return out


@pytest.mark.parametrize("name", ["text", "rand"])
def test_large_arrays_three_ways(big, name):
    t, sa, isa = big[name]
    n = len(t)
    assert sa_ref.check(t, sa) == (sa_ref.OK, sa_ref.NONE)                 # linear, vectorised: sorted and a permutation
    assert np.array_equal(isa[sa], np.arange(n, dtype=np.int32))
    assert sa_ref.bwt_of(t, sa) == oracle.divbwt(t)                        # the reference project's own sort, through the BWT


def test_device_form_writes_its_arrays_and_nothing_beside_them(ctx):
    t = oracle.synth_text(8, 70001)
    n = len(t)
    want = sa_ref.suffix_array(t)
    d = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to(DEV)
    for with_isa in (True, False):
        g_sa = torch.full((n + 8,), -5, dtype=torch.int32, device=DEV)
        g_isa = torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        rc = api.suffix_array_device(d.data_ptr(), n, g_sa.data_ptr() + 16, g_isa.data_ptr() + 16 if with_isa else None, ctx=ctx)
        assert rc == 0
        h_sa, h_isa = g_sa.cpu().numpy(), g_isa.cpu().numpy()
        assert (h_sa[:4] == -5).all() and (h_sa[n + 4:] == -5).all() and np.array_equal(h_sa[4:n + 4], want)
        if with_isa:
            assert (h_isa[:4] == -7).all() and (h_isa[n + 4:] == -7).all() and np.array_equal(h_isa[4:n + 4], sa_ref.inverse(want))
        else:
            assert (h_isa == -7).all()                                     # d_isa = NULL: nothing of it is written
        assert d.cpu().numpy().tobytes() == t                              # the input is only read


def test_tensor_helpers(ctx):
    t = oracle.synth_rand(12, 5003)
    d = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to(DEV)
    want = sa_ref.suffix_array(t)
    sa, isa = bce_amd.suffix_array_tensor(d, inverse=True, ctx=ctx)
    assert sa.dtype == torch.int32 and sa.device == d.device and isa.device == d.device
    assert np.array_equal(sa.cpu().numpy(), want) and np.array_equal(isa.cpu().numpy(), sa_ref.inverse(want))
    assert np.array_equal(bce_amd.suffix_array_tensor(d).cpu().numpy(), want)       # a context of its own
    assert bce_amd.sufcheck_tensor(d, sa, ctx=ctx) is None
    bad = sa.clone()
    bad[[10, 11]] = bad[[11, 10]]
    assert bce_amd.sufcheck_tensor(d, bad, ctx=ctx) == sa_ref.verdict(t, bad.cpu().numpy())
    with pytest.raises(ValueError):
        bce_amd.suffix_array_tensor(d.cpu())
    with pytest.raises(ValueError):
        bce_amd.sufcheck_tensor(d, sa[:-1])


def test_refusals_come_before_any_device_call(ctx):
    lib, h = ctx.lib, ctx.h
    a, sa = np.zeros(8, dtype=np.uint8), np.full(8, -3, dtype=np.int32)
    A, S = a.ctypes.data, sa.ctypes.data
    assert lib.bce_hip_suffix_array(None, A, 8, S, None) == E_ARG
    assert lib.bce_hip_suffix_array(h, None, 8, S, None) == E_ARG and lib.bce_hip_suffix_array(h, A, 8, None, S) == E_ARG
    assert lib.bce_hip_suffix_array(h, A, 0, S, None) == E_ARG
    # 2^31 - 1 and more: refused on the size alone -- a device call would read 2 GB behind these eight bytes
    for n in (0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        assert lib.bce_hip_suffix_array(h, A, n, S, None) == E_ARG
        assert lib.bce_hip_suffix_array_device(h, 0x1000, n, 0x2000, None) == E_ARG
    assert lib.bce_hip_suffix_array_device(None, 0x1000, 8, 0x2000, None) == E_ARG
    assert lib.bce_hip_suffix_array_device(h, None, 8, 0x2000, None) == E_ARG and lib.bce_hip_suffix_array_device(h, 0x1000, 8, None, 0x2000) == E_ARG
    assert lib.bce_hip_suffix_array_device(h, 0x1000, 0, 0x2000, None) == E_ARG
    assert (sa == -3).all()
    with pytest.raises(bce_amd.BceError):
        bce_amd.suffix_array(b"", ctx=ctx)


def test_the_compression_state_is_dropped_and_a_later_compression_is_a_fresh_ones(ctx):
    t = np.frombuffer(oracle.synth_text(14, 40000), dtype=np.uint8)
    fresh = bytes(bce_amd.compress(t))
    rf = api.RankFile(t, ctx=ctx)
    assert rf.count(b"the") >= 0                                           # the context is indexed ...
    other = oracle.synth_rand(15, 9000)
    assert np.array_equal(bce_amd.suffix_array(other, ctx=ctx), sa_ref.suffix_array(other))
    # ... and after the sort it is not: the queries are refused, they do not read the planes or the order of another text
    lib, h = ctx.lib, ctx.h
    pat, off, cnt = np.frombuffer(b"the", dtype=np.uint8).copy(), np.array([0, 3], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    assert lib.bce_hip_count(h, pat.ctypes.data, off.ctypes.data, 1, cnt.ctypes.data) == E_STATE
    total, hits = C.c_uint64(0), np.zeros(2, dtype=np.uint64)
    assert lib.bce_hip_locate(h, pat.ctypes.data, off.ctypes.data, 1, 1, hits.ctypes.data, None, 0, C.byref(total)) == E_STATE
    lcp = np.zeros(len(t), dtype=np.uint32)
    assert lib.bce_hip_lcp(h, 16, lcp.ctypes.data) == E_STATE
    crc = C.c_uint32(0)
    assert lib.bce_hip_input_crc32(h, C.byref(crc)) == E_STATE
    assert lib.bce_hip_encode(h) == E_STATE
    assert bytes(bce_amd.compress(t, ctx=ctx)) == fresh
    assert bytes(api.BCE().encode(api.RankFile(t, ctx=ctx))) == fresh
