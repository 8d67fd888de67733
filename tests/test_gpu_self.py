"""GPU: what the indexed text repeats of itself (kd_self.hip through bce_hip_lpf / _lpf_device, bce_hip_self_parse / _self_parse_device,
RankFile.lpf / self_parse, lpf_tensor, self_parse_tensor, self_parse_in_archive) against tests/lpf_ref.py: the longest previous factors
exactly, every source by content and order, the parse decoded without the text and patched over it, info, the fewest phrases at min_len
1, host == device == tensor == archive results, the states and arguments that are refused, and that nothing else in the context moves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import lpf_ref as ref
from test_count_cpu import _texts
from test_lpf_cpu import TAIL_REPEATS_HEAD

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_OVERFLOW = -1, -4, -5
NONE = 0xFFFFFFFF
BOUNDS = (1, 3, 7, 4096)
MIN_LENS = (1, 3, 8)
BIG = ("one", "a4200", "ab2048", "pasted", "rand65536")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _big(name):
    if name == "one":
        return b"x"
    if name == "a4200":                                                   # lpf[i] = min(n - i, 4096) for i >= 1
        return b"a" * 4200
    if name == "ab2048":                                                  # equal rotations: the sort leaves them in any order
        return b"ab" * 2048
    if name == "pasted":                                                  # a slice of 9 000 bytes pasted twice into 70 000
        t = bce_amd.synth_text(21, 52000).tobytes()
        piece = t[7000:16000]
        return t[:30000] + piece + t[30000:45000] + piece + t[45000:]
    return bce_amd.synth_rand(5, 65536).tobytes()


@functools.lru_cache(maxsize=None)
def _want_lpf(name, L):
    return ref.lpf(_big(name), L)


def _small_texts():
    return _texts()[0] + TAIL_REPEATS_HEAD + [b"ab" * 9, b"abc" * 7, b"a" * 19]


def _check_parse(text, lpf_want, m, ops, lits, info, rf=None):
    want = ref.chain(lpf_want, text, m)
    ref.check(text, want, ops, lits, info)
    assert ref.decode(ops, lits) == text                                  # the sequential decoder: ops and literal bytes only
    assert info["nlits"] + info["copied"] == len(text) and info["nops"] - info["ncopies"] == sum(1 for p in want[0] if not p[2])
    if rf is not None:
        assert rf.patch(ops, lits).tobytes() == text                      # and the patch over the text


def test_small_texts_every_bound_lpf_sources_and_parse(ctx):
    texts = _small_texts()
    assert len(texts) == 57 + 9
    for t in texts:
        rf = api.RankFile(np.frombuffer(t, dtype=np.uint8), ctx=ctx)
        for L in BOUNDS:
            want = ref.lpf_brute(t, L)
            lpf, src = rf.lpf(L)
            assert lpf.tolist() == want, (t, L)
            ref.check_src(t, lpf, src)
            assert rf.lpf(L, sources=False)[1] is None
            for m in (m for m in MIN_LENS if m <= L):
                ops, lits, info = rf.self_parse(m, L)
                _check_parse(t, want, m, ops, lits, info, rf)
                if m == 1:
                    assert info["ncopies"] + info["nlits"] == ref.fewest_phrases(t, L), (t, L)
    assert ref.lpf_brute(b"abcXabc", 4096) == [0, 0, 0, 0, 3, 2, 1]       # the cyclic match would run on: lpf stops at n - i


@pytest.mark.parametrize("name", BIG)
def test_lpf_is_the_reference_and_every_source_holds(ctx, name):
    t = _big(name)
    rf = api.RankFile(np.frombuffer(t, dtype=np.uint8), ctx=ctx)
    for L in (16, 4096):
        want = _want_lpf(name, L)
        lpf, src = rf.lpf(L)
        assert np.array_equal(lpf, np.array(want, dtype=np.uint32)), (name, L)
        ref.check_src(t, lpf, src)
    if name == "a4200":
        assert _want_lpf(name, 4096) == [0] + [min(4200 - i, 4096) for i in range(1, 4200)]
    if name == "pasted":
        assert max(_want_lpf(name, 4096)) == 4096 and _want_lpf(name, 4096)[30000] == 4096
    if name == "one":
        assert lpf.tolist() == [0] and src.tolist() == [NONE]


@pytest.mark.parametrize("name", BIG)
def test_self_parse_decodes_patches_and_agrees_through_every_entry_point(ctx, name):
    t = _big(name)
    arr = np.frombuffer(t, dtype=np.uint8)
    d = torch.from_numpy(arr.copy()).to(DEV)
    plain = bytes(bce_amd.compress(arr)) if name in ("a4200", "pasted") else None
    rf = api.RankFile(arr, ctx=ctx)
    for m, L in ((1, 4096), (16, 256), (8, 16)):
        want = _want_lpf(name, L) if L in (16, 4096) else ref.lpf(t, L)
        ops, lits, info = rf.self_parse(m, L)
        _check_parse(t, want, m, ops, lits, info, rf)
        # device entry: sizing, then into guarded buffers
        sized = rf.self_parse_device(m, L)
        assert sized == info
        g_ops = torch.full((2 * info["nops"] + 3,), -5, dtype=torch.int32, device=DEV)
        g_lits = torch.full((info["nlits"] + 6,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        if info["nops"] > 1:
            with pytest.raises(api.BceError) as e:
                rf.self_parse_device(m, L, g_ops[1:].data_ptr(), info["nops"] - 1, g_lits[3:].data_ptr(), info["nlits"])
            assert e.value.status == E_OVERFLOW and bool((g_ops == -5).all()) and bool((g_lits == 0xA5).all())
        assert rf.self_parse_device(m, L, g_ops[1:].data_ptr(), info["nops"], g_lits[3:].data_ptr() if info["nlits"] else None, info["nlits"]) == info
        go, gl = g_ops.cpu().numpy(), g_lits.cpu().numpy()
        assert go[0] == -5 and (go[-2:] == -5).all() and (gl[:3] == 0xA5).all() and (gl[3 + info["nlits"]:] == 0xA5).all()
        dev_ops = go[1:-2].view(np.uint32).reshape(-1, 2)
        assert [l for l, _s in ref.pairs(dev_ops)] == [l for l, _s in ref.pairs(ops)] and gl[3:3 + info["nlits"]].tobytes() == lits.tobytes()
        _check_parse(t, want, m, dev_ops, gl[3:3 + info["nlits"]], info)
        # tensors
        t_ops, t_lits, t_info = bce_amd.self_parse_tensor(d, m, L, ctx=ctx)
        assert t_info == info and np.array_equal(t_ops.cpu().numpy().view(np.uint32), dev_ops) and t_lits.cpu().numpy().tobytes() == lits.tobytes()
        if plain is not None and L == 256:
            a_ops, a_lits, a_info = bce_amd.self_parse_in_archive(plain, m, L)
            assert a_info == info and np.array_equal(a_ops.cpu().numpy().view(np.uint32), dev_ops) and a_lits.cpu().numpy().tobytes() == lits.tobytes()
        rf = api.RankFile(arr, ctx=ctx)                                   # (the tensor calls indexed their own copy in this context)
    t_lpf, t_src = bce_amd.lpf_tensor(d, 16, ctx=ctx)
    assert np.array_equal(t_lpf.cpu().numpy().view(np.uint32), np.array(_want_lpf(name, 16), dtype=np.uint32))
    ref.check_src(t, t_lpf.cpu().numpy().view(np.uint32), t_src.cpu().numpy().view(np.uint32))
    if name == "a4200":                                                   # the one-call forms, contexts of their own
        assert bce_amd.lpf(arr, 16, sources=False)[0].tolist() == _want_lpf(name, 16) and bce_amd.self_parse(arr, 8, 16)[2] == info


def test_self_parse_in_a_checked_container_reaches_across_blocks():
    data = bce_amd.synth_text(41, 6000).tobytes() * 2                     # the second block repeats the first
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEV)
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)                    # what `bce -C2` writes
    assert len(container.block_table(blob)) == 2
    ops, lits, info = bce_amd.self_parse_in_archive(blob, 16, 4096)
    want = ref.self_parse(data, 16, 4096)
    assert info == want[2] and ref.decode(ops.cpu().numpy().view(np.uint32), lits.cpu().numpy().tobytes()) == data
    assert info["copied"] >= 6000


# ---- states and refusals ----------------------------------------------------------------------------------------------------------

def _calls(c, lpf, src, ops, lits, info, min_len=1, max_len=16):
    lib = c.lib
    return [lambda: lib.bce_hip_lpf(c.h, max_len, lpf.ctypes.data, src.ctypes.data),
            lambda: lib.bce_hip_lpf_device(c.h, max_len, lpf.ctypes.data, src.ctypes.data),
            lambda: lib.bce_hip_self_parse(c.h, min_len, max_len, ops.ctypes.data, len(ops) // 2, lits.ctypes.data, len(lits), C.byref(info)),
            lambda: lib.bce_hip_self_parse_device(c.h, min_len, max_len, ops.ctypes.data, len(ops) // 2, lits.ctypes.data, len(lits), C.byref(info))]


def _untouched(lpf, src, ops, lits, info):
    return (lpf == 7).all() and (src == 8).all() and (ops == 9).all() and (lits == 10).all() and (info.nops, info.nlits, info.ncopies, info.copied) == (1, 2, 3, 4)


def test_injected_bwt_and_missing_planes_are_refused_in_the_locates_words():
    text = b"abracadabra" * 9 + b"x"
    bwt, row0 = count_ref.bwt_of_rotations(text)
    n = len(text)
    lpf, src, ops, lits = np.full(n, 7, dtype=np.uint32), np.full(n, 8, dtype=np.uint32), np.full(2 * n, 9, dtype=np.uint32), np.full(n, 10, dtype=np.uint8)
    info = api.ParseInfo(1, 2, 3, 4)
    c = api._Ctx(0)
    try:
        for call in _calls(c, lpf, src, ops, lits, info):
            assert call() == E_STATE and b"holds no planes" in c.lib.bce_hip_last_error(c.h)
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)                    # behind bce_hip_set_bwt
        for call in _calls(c, lpf, src, ops, lits, info):
            assert call() == E_STATE and b"no suffix array behind an injected BWT" in c.lib.bce_hip_last_error(c.h)
        for use in (lambda: rf.lpf(16), lambda: rf.self_parse(4, 16)):
            with pytest.raises(api.BceError) as e:
                use()
            assert e.value.status == E_STATE
        assert _untouched(lpf, src, ops, lits, info)
    finally:
        c.close()


def test_refusal_order_arguments_then_state_then_null_outputs():
    text = bce_amd.synth_text(5, 20000)
    n = len(text)
    lpf, src, ops, lits = np.full(n, 7, dtype=np.uint32), np.full(n, 8, dtype=np.uint32), np.full(2 * n, 9, dtype=np.uint32), np.full(n, 10, dtype=np.uint8)
    info = api.ParseInfo(1, 2, 3, 4)
    c = api._Ctx(0)
    try:
        lib = c.lib
        api.RankFile(text, ctx=c, build=False)                            # loaded, K1 done, no planes yet
        for call in _calls(c, lpf, src, ops, lits, info):
            assert call() == E_STATE
        for call in _calls(c, lpf, src, ops, lits, info, max_len=0) + _calls(c, lpf, src, ops, lits, info, max_len=4097) + _calls(c, lpf, src, ops, lits, info, 17, 16)[2:]:
            assert call() == E_ARG                                        # the arguments come before the state
        assert lib.bce_hip_lpf(c.h, 16, None, None) == E_STATE and lib.bce_hip_lpf_device(c.h, 16, None, None) == E_STATE   # the state before a null output
        for fn in (lib.bce_hip_self_parse, lib.bce_hip_self_parse_device):
            assert fn(c.h, 1, 16, None, 1, None, 0, C.byref(info)) == E_ARG and fn(c.h, 1, 16, None, 0, None, 1, C.byref(info)) == E_ARG
            assert fn(c.h, 1, 16, None, 0, None, 0, None) == E_ARG
        rf = api.RankFile(text, ctx=c)
        for call in _calls(c, lpf, src, ops, lits, info, max_len=0) + _calls(c, lpf, src, ops, lits, info, 0, 16)[2:] + _calls(c, lpf, src, ops, lits, info, 1, 0xFFFFFFFF):
            assert call() == E_ARG
        assert lib.bce_hip_lpf(c.h, 16, None, src.ctypes.data) == E_ARG and lib.bce_hip_lpf_device(c.h, 16, None, None) == E_ARG
        assert _untouched(lpf, src, ops, lits, info)
        with pytest.raises(api.BceError):
            rf.lpf(0)
        with pytest.raises(api.BceError):
            rf.self_parse(17, 16)
        assert rf.self_parse_device(16, 256)["nops"] >= 1                 # a sizing call succeeds
        # a decode takes the planes, the suffix array and the text away
        fresh = bytes(bce_amd.compress(text))
        assert bce_amd.decompress_device(fresh, ctx=c) == text.tobytes()
        for call in _calls(c, lpf, src, ops, lits, info):
            assert call() == E_STATE
        assert _untouched(lpf, src, ops, lits, info)
    finally:
        c.close()


def test_the_calls_leave_the_compression_and_the_other_queries_alone():
    text = bce_amd.synth_text(5, 50000)
    tb = text.tobytes()
    fresh = bytes(bce_amd.compress(text))
    c = api._Ctx(0)
    try:
        rf = api.RankFile(text, ctx=c)
        pats = [tb[i * 97:i * 97 + 1 + i % 40] for i in range(100)]
        counts = rf.count(pats).tolist()
        lcp = rf.lcp(300)
        lpf, src = rf.lpf(300)
        parsed = rf.self_parse(16, 300)
        assert ref.decode(parsed[0], parsed[1]) == tb
        assert bytes(api.BCE().encode(rf)) == fresh                       # the calls, then encode: the archive of a fresh context
        again, src2 = rf.lpf(300)
        assert np.array_equal(again, lpf) and np.array_equal(src2, src) and lpf.tolist() == ref.lpf(tb, 300)
        p2 = rf.self_parse(16, 300)
        assert np.array_equal(p2[0], parsed[0]) and np.array_equal(p2[1], parsed[1]) and p2[2] == parsed[2]
        assert rf.count(pats).tolist() == counts and np.array_equal(rf.lcp(300), lcp)
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()
