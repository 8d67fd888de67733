"""GPU: a second buffer as a delta against the indexed text (kd_parse.hip through bce_hip_parse / _parse_device, bce_hip_patch /
_patch_device, RankFile.parse / patch, parse_tensor / patch_tensor, delta / apply_delta) against the chain walked in Python on the
brute-force lengths (tests/parse_ref.py): the structure exactly, every copy by content (which occurrence is named is not
specified), the round trip through every entry point, sizing and overflow, the states and arguments that are refused, and that
nothing else in the context moves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import match_ref
import parse_ref as ref
from test_gpu_match import _text

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_OVERFLOW = -1, -4, -5
PB = 2048                                                                 # positions per block of the parse
Q_SIZES = (1, 63, 64, 65, 255, 256, 257, PB - 1, PB, PB + 1, 2 * PB + 1)
TEXT_NAMES = ("n1", "n2", "n97", "abracadabra", "a300", "ab150", "text6144", "rand6144", "text100000")
MIN_LENS = (1, 4, 16)


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _top(name):
    """the largest bound this text is asked with: 4096 up to 6144 bytes, else 300 (match_ref is a brute force)"""
    return 4096 if len(_text(name)) <= 6144 else 300


def _bounds(name, m):
    return sorted({L for L in (m, 16, 300, 4096) if m <= L <= _top(name)})


@functools.lru_cache(maxsize=None)
def _queries(name):
    """Pieces of every size in Q_SIZES cut from the circular text, a byte spoiled every 40 bytes or so; the text's end followed by
    its beginning (a copy must not cross the end); zeros; the text itself (its first 500 bytes for the long one)."""
    text = _text(name)
    n = len(text)
    rs = np.random.RandomState(n + 1)
    qs = []
    for q in Q_SIZES:
        piece = bytearray(count_ref.cyclic_cut(text, int(rs.randint(0, n)), q))
        for at in range(int(rs.randint(0, 40)), q, 40):
            piece[at] ^= 0x80
        qs.append(bytes(piece))
    wrap = text + text[:min(n, 5)] if n <= 300 else text[-8:] + text[:8]
    qs += [wrap, b"\x00" * 100, text if n <= 6144 else text[:500]]
    return qs


@functools.lru_cache(maxsize=None)
def _full(name, k):
    out = match_ref.match_lens(_text(name), _queries(name)[k], _top(name))
    out.setflags(write=False)
    return out


def _want(name, k, m, L):
    """the reference's parse: the chain on the full lengths cut at the bound ("occurs" is monotone in the length)"""
    return ref.parse_of_lengths(np.minimum(_full(name, k), L), _queries(name)[k], m)


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_parse_is_the_reference_chain_and_patch_undoes_it(ctx, name):
    text = _text(name)
    rf = api.RankFile(text, ctx=ctx)
    runs = copies = 0
    for k, q in enumerate(_queries(name)):
        for m in MIN_LENS:
            for L in _bounds(name, m):
                ops, lits, info = rf.parse(q, m, L)
                assert ops.dtype == api.OP_DTYPE and lits.dtype == np.uint8
                want = _want(name, k, m, L)
                ref.check(text, q, want, ops, lits, info)
                assert rf.patch(ops, lits).tobytes() == q, (name, k, m, L)
                runs += info["nops"] - info["ncopies"]
                copies += info["ncopies"]
    assert runs and copies
    ops, lits, info = rf.parse(b"", 4)
    assert len(ops) == 0 and len(lits) == 0 and info == {"nops": 0, "nlits": 0, "ncopies": 0, "copied": 0}
    assert len(rf.patch(ops, lits)) == 0


@pytest.mark.parametrize("name", ("n1", "n97", "ab150", "text6144"))
def test_device_and_tensor_entry_points_with_guard_words(ctx, name):
    text = _text(name)
    rf = api.RankFile(text, ctx=ctx)
    dev = "cuda:0"
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    for k in (0, 3, 8, 10, len(Q_SIZES)):
        q = _queries(name)[k]
        buf = torch.zeros(len(q) + 7, dtype=torch.uint8, device=dev)
        buf[3:3 + len(q)] = torch.from_numpy(np.frombuffer(q, dtype=np.uint8).copy()).to(dev)
        d_q = buf[3:3 + len(q)]
        assert d_q.data_ptr() % 2 == 1
        for m, L in ((1, 16), (4, 4), (16, 300)):
            want = _want(name, k, m, L)
            torch.cuda.synchronize()
            info = rf.parse_device(d_q.data_ptr(), len(q), m, L)                                  # the sizing call
            assert info == want[2]
            nops, nlits = info["nops"], info["nlits"]
            ops_buf = torch.full((2 * nops + 3,), -5, dtype=torch.int32, device=dev)             # the ops at an odd word
            lits_buf = torch.full((nlits + 6,), 0xA5, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            info = rf.parse_device(d_q.data_ptr(), len(q), m, L, ops_buf[1:].data_ptr(), nops, lits_buf[3:].data_ptr() if nlits else None, nlits)
            got = ops_buf.cpu().numpy()
            assert got[0] == -5 and (got[-2:] == -5).all()
            gl = lits_buf.cpu().numpy()
            assert (gl[:3] == 0xA5).all() and (gl[3 + nlits:] == 0xA5).all()
            ref.check(text, q, want, got[1:-2].view(np.uint32).reshape(-1, 2), gl[3:3 + nlits], info)
            out_buf = torch.full((len(q) + 9,), 0x5A, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            for lead in (1, 5):                                                                   # the result at odd addresses
                out_buf.fill_(0x5A)
                torch.cuda.synchronize()
                total = rf.patch_device(ops_buf[1:].data_ptr(), nops, lits_buf[3:].data_ptr() if nlits else None, nlits,
                                        out_buf[lead:].data_ptr(), len(q))
                go = out_buf.cpu().numpy()
                assert total == len(q) and go[lead:lead + len(q)].tobytes() == q
                assert (go[:lead] == 0x5A).all() and (go[lead + len(q):] == 0x5A).all()
            assert rf.patch_device(ops_buf[1:].data_ptr(), nops, lits_buf[3:].data_ptr() if nlits else None, nlits) == len(q)
        ops_t, lits_t, info = bce_amd.parse_tensor(t, d_q, 4, ctx=ctx)
        assert ops_t.dtype == torch.int32 and ops_t.shape == (info["nops"], 2) and lits_t.dtype == torch.uint8 and ops_t.device == t.device
        ref.check(text, q, _want(name, k, 4, 256), ops_t.cpu().numpy().view(np.uint32), lits_t.cpu().numpy(), info)
        back = bce_amd.patch_tensor(t, ops_t, lits_t, ctx=ctx)
        assert back.cpu().numpy().tobytes() == q
        room = torch.zeros(len(q) + 5, dtype=torch.uint8, device=dev)
        assert bce_amd.patch_tensor(t, ops_t, lits_t, out=room).cpu().numpy().tobytes() == q      # a context of its own
        rf = api.RankFile(text, ctx=ctx)                                                           # (the tensor calls loaded t into ctx)
    with pytest.raises(ValueError):
        bce_amd.parse_tensor(t, d_q.cpu(), 4)
    ops, lits, info = bce_amd.parse(text, q, 4)
    ref.check(text, q, _want(name, k, 4, 256), ops, lits, info)
    assert bce_amd.patch(text, ops, lits).tobytes() == q


def test_sizing_then_overflow_leaves_the_outputs_untouched(ctx):
    text = _text("text6144")
    q = np.frombuffer(_queries("text6144")[8], dtype=np.uint8)
    api.RankFile(text, ctx=ctx)
    lib = ctx.lib
    info = api.ParseInfo()
    assert lib.bce_hip_parse(ctx.h, q.ctypes.data, len(q), 4, 256, None, 0, None, 0, C.byref(info)) == 0
    want = _want("text6144", 8, 4, 256)[2]
    assert info.as_dict() == want and want["nops"] > 3 and want["nlits"] > 3
    nops, nlits = want["nops"], want["nlits"]
    d_q = torch.from_numpy(q.copy()).to("cuda:0")
    for ops_cap, lits_cap in ((nops - 1, nlits), (nops, nlits - 1), (0, nlits), (nops, 0)):
        ops, lits, info = np.full((nops, 2), 7, dtype=np.uint32), np.full(nlits, 9, dtype=np.uint8), api.ParseInfo()
        assert lib.bce_hip_parse(ctx.h, q.ctypes.data, len(q), 4, 256, ops.ctypes.data, ops_cap, lits.ctypes.data, lits_cap, C.byref(info)) == E_OVERFLOW
        assert info.as_dict() == want and (ops == 7).all() and (lits == 9).all()
        d_ops = torch.full((nops, 2), 7, dtype=torch.int32, device="cuda:0")
        d_lits = torch.full((nlits,), 9, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        info = api.ParseInfo()
        assert lib.bce_hip_parse_device(ctx.h, d_q.data_ptr(), len(q), 4, 256, d_ops.data_ptr(), ops_cap, d_lits.data_ptr(), lits_cap, C.byref(info)) == E_OVERFLOW
        assert info.as_dict() == want and bool((d_ops == 7).all()) and bool((d_lits == 9).all())
    ops, lits, total = np.zeros((nops, 2), dtype=np.uint32), np.zeros(nlits, dtype=np.uint8), C.c_uint64(0)
    assert lib.bce_hip_parse(ctx.h, q.ctypes.data, len(q), 4, 256, ops.ctypes.data, nops, lits.ctypes.data, nlits, C.byref(info)) == 0
    out = np.full(len(q), 3, dtype=np.uint8)
    assert lib.bce_hip_patch(ctx.h, ops.ctypes.data, nops, lits.ctypes.data, nlits, out.ctypes.data, len(q) - 1, C.byref(total)) == E_OVERFLOW
    assert total.value == len(q) and (out == 3).all()
    assert lib.bce_hip_patch(ctx.h, ops.ctypes.data, nops, lits.ctypes.data, nlits, out.ctypes.data, len(q), C.byref(total)) == 0
    assert out.tobytes() == q.tobytes()


def test_refused_arguments_and_states():
    text = bce_amd.synth_text(5, 20000)
    q = np.frombuffer(text[100:164].tobytes(), dtype=np.uint8)
    c = api._Ctx(0)
    try:
        lib = c.lib
        ops, lits, info, total = np.full((64, 2), 7, dtype=np.uint32), np.full(64, 9, dtype=np.uint8), api.ParseInfo(1, 2, 3, 4), C.c_uint64(5)
        args = (c.h, q.ctypes.data, 64, 4, 16, ops.ctypes.data, 64, lits.ctypes.data, 64, C.byref(info))
        for fn in (lib.bce_hip_parse, lib.bce_hip_parse_device):
            assert fn(*args) == E_STATE and b"holds no planes" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_patch(c.h, ops.ctypes.data, 1, None, 0, None, 0, C.byref(total)) == E_STATE
        api.RankFile(text, ctx=c, build=False)
        assert lib.bce_hip_parse(*args) == E_STATE
        rf = api.RankFile(text, ctx=c)
        for fn in (lib.bce_hip_parse, lib.bce_hip_parse_device):         # every refusal comes before a launch: host pointers are never read
            for m, L in ((0, 16), (17, 16), (4, 4097), (4, 0), (0xFFFFFFFF, 0xFFFFFFFF)):
                assert fn(*(args[:3] + (m, L) + args[5:])) == E_ARG
            assert fn(*(args[:2] + (1 << 31,) + args[3:])) == E_ARG
            assert fn(*(args[:9] + (None,))) == E_ARG
            assert fn(c.h, None, 64, 4, 16, ops.ctypes.data, 64, lits.ctypes.data, 64, C.byref(info)) == E_ARG
            assert fn(c.h, q.ctypes.data, 64, 4, 16, None, 64, lits.ctypes.data, 64, C.byref(info)) == E_ARG
            assert fn(c.h, q.ctypes.data, 64, 4, 16, ops.ctypes.data, 64, None, 64, C.byref(info)) == E_ARG
            assert (info.nops, info.nlits, info.ncopies, info.copied) == (1, 2, 3, 4)
            assert fn(c.h, None, 0, 4, 16, None, 0, None, 0, C.byref(info)) == 0 and info.as_dict() == {"nops": 0, "nlits": 0, "ncopies": 0, "copied": 0}
            info = api.ParseInfo(1, 2, 3, 4)
        for fn in (lib.bce_hip_patch, lib.bce_hip_patch_device):
            assert fn(c.h, ops.ctypes.data, 1 << 31, None, 0, None, 0, C.byref(total)) == E_ARG
            assert fn(c.h, None, 1, None, 0, None, 0, C.byref(total)) == E_ARG
            assert fn(c.h, ops.ctypes.data, 1, None, 1, None, 0, C.byref(total)) == E_ARG
            assert fn(c.h, ops.ctypes.data, 1, None, 0, None, 5, C.byref(total)) == E_ARG
            assert fn(c.h, ops.ctypes.data, 1, None, 0, None, 0, None) == E_ARG
            assert total.value == 5
            assert fn(c.h, None, 0, None, 0, None, 0, C.byref(total)) == 0 and total.value == 0
            total.value = 5
        assert (ops == 7).all() and (lits == 9).all()
        with pytest.raises(api.BceError):
            rf.parse(b"abc", 0)
        # a decode takes the planes, the suffix array and the text away
        fresh = bytes(bce_amd.compress(text))
        assert bce_amd.decompress_device(fresh, ctx=c) == text.tobytes()
        assert lib.bce_hip_parse(*args) == E_STATE
        one = np.array([[3, 0]], dtype=np.uint32)
        assert lib.bce_hip_patch(c.h, one.ctypes.data, 1, None, 0, None, 0, C.byref(total)) == E_STATE
    finally:
        c.close()


def test_injected_bwt_is_refused_in_the_locates_words():
    text = b"abracadabra" * 9 + b"x"
    bwt, row0 = count_ref.bwt_of_rotations(text)
    q = np.frombuffer(b"cadabraabra", dtype=np.uint8)
    c = api._Ctx(0)
    try:
        api.RankFile(bwt=bwt, offset=row0, ctx=c)
        info, total = api.ParseInfo(), C.c_uint64(0)
        assert c.lib.bce_hip_parse(c.h, q.ctypes.data, len(q), 4, 16, None, 0, None, 0, C.byref(info)) == E_STATE
        assert b"no suffix array behind an injected BWT" in c.lib.bce_hip_last_error(c.h)
        one = np.array([[3, 0]], dtype=np.uint32)
        assert c.lib.bce_hip_patch(c.h, one.ctypes.data, 1, None, 0, None, 0, C.byref(total)) == E_STATE
    finally:
        c.close()


def test_parse_leaves_the_compression_alone():
    text = bce_amd.synth_text(5, 50000)
    tb = text.tobytes()
    fresh = bytes(bce_amd.compress(text))
    query = bytearray(tb[20000:24000] + tb[-100:] + tb[:100])
    for at in range(11, len(query), 53):
        query[at] ^= 0x80
    query = bytes(query)
    c = api._Ctx(0)
    try:
        rf = api.RankFile(text, ctx=c)
        ops, lits, info = rf.parse(query, 16, 300)
        ref.check(tb, query, ref.parse(tb, query, 16, 300), ops, lits, info)
        assert rf.patch(ops, lits).tobytes() == query
        assert bytes(api.BCE().encode(rf)) == fresh                      # parse and patch, then encode: the archive of a fresh context
        again = rf.parse(query, 16, 300)
        assert np.array_equal(again[0]["len"], ops["len"]) and again[2] == info and rf.patch(*again[:2]).tobytes() == query
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()


def test_delta_round_trip_and_the_crc_refusals():
    base = bce_amd.synth_text(9, 30000).tobytes()
    new = bytearray(base[5000:12000] + b"something new in the middle" + base[100:2100] + base[-50:] + base[:50])
    for at in range(7, len(new), 301):
        new[at] ^= 0x40
    new = bytes(new)
    blob = bce_amd.delta(base, new)
    d = container.unpack_delta(blob)
    assert (d["n"], d["q"], d["min_len"], d["max_len"]) == (len(base), len(new), 16, 256)
    assert d["base_crc"] == bce_amd.crc32(base) and d["crc"] == bce_amd.crc32(new)
    ph, wlits, winfo = ref.parse(base, new, 16, 256)
    ref.check(base, new, (ph, wlits, winfo), d["ops"], d["lits"], {"nops": len(d["ops"]), "nlits": len(d["lits"]), "ncopies": winfo["ncopies"], "copied": winfo["copied"]})
    assert len(blob) == 56 + 8 * winfo["nops"] + winfo["nlits"] < len(new)
    assert container.pack_delta(d["n"], d["base_crc"], d["q"], d["crc"], d["min_len"], d["max_len"], d["ops"], d["lits"]) == blob
    assert bce_amd.apply_delta(base, blob) == new
    wrong = bytearray(base)
    wrong[12345] ^= 1
    with pytest.raises(bce_amd.ChecksumError):
        bce_amd.apply_delta(bytes(wrong), blob)                           # another base of the same size
    with pytest.raises(bce_amd.ChecksumError):
        bce_amd.apply_delta(base[:-1], blob)
    lied = bytearray(blob)
    lied[28:32] = (d["crc"] ^ 1).to_bytes(4, "little")                   # the result's CRC-32
    with pytest.raises(bce_amd.ChecksumError):
        bce_amd.apply_delta(base, bytes(lied))
    with pytest.raises(ValueError):
        bce_amd.apply_delta(base, blob[:-1])
    assert bce_amd.apply_delta(base, bce_amd.delta(base, b"")) == b""
    assert bce_amd.apply_delta(base, bce_amd.delta(base, base, min_len=1, max_len=4096)) == base
