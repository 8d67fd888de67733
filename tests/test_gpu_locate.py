"""GPU: pattern positions from the BWT planes and K1's suffix array (kd_locate.hip through bce_hip_locate / _locate_device,
RankFile.locate, locate, locate_tensor, locate_in_archive) against brute-force scans of the same text in Python / numpy: the hit
lists themselves, cyclic and linear, their order, the CSR offsets, the overflow protocol, the states in which the call is refused,
and that nothing else in the context moves."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import locate_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_OVERFLOW = -1, -4, -5
LINEAR = 1
SIZES = (1, 2, 95, 96, 97, 3071, 3072, 3073, 6144)     # the granule holds 96 positions, the chunk 3072 (tests/test_gpu_count.py)
GUARD = 0xDEADBEEF


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _texts(n):
    return [("synth_text", bce_amd.synth_text(n, n).tobytes()), ("synth_rand", bce_amd.synth_rand(n + 1, n).tobytes()),
            ("all-equal", b"z" * n), ("period-2", (b"ab" * n)[:n]), ("period-3", (b"abc" * n)[:n]),
            ("all-256", (bytes(range(256)) * (n // 256 + 1))[:n])]


def _patterns(text):
    """Every byte value alone; substrings at the wrap; m = n, n + 1, 3 n; absent bytes; the empty pattern (last)."""
    n = len(text)
    pats = [bytes([v]) for v in range(256)]
    for m in (2, 3, 8, 64):
        for back in (1, m // 2, m - 1):
            pats.append(count_ref.cyclic_cut(text, n - min(back, n), m))
    pats += [count_ref.cyclic_cut(text, 0, n), count_ref.cyclic_cut(text, n // 3, n), count_ref.cyclic_cut(text, 0, n + 1),
             count_ref.cyclic_cut(text, n - 1, n + 1)]
    if n <= 97:
        pats += [count_ref.cyclic_cut(text, 0, 3 * n), count_ref.cyclic_cut(text, n // 2, 3 * n)]
    pats += [b"\x00", b"\xff", text[:2] + b"\x00", b"\xff" + text[:3], b""]
    return pats


def _want(text, pats, cyclic):
    """locate_ref's lists; the single bytes and the empty pattern from numpy (the same sets, cheaper)."""
    arr = np.frombuffer(text, dtype=np.uint8)
    out = []
    for p in pats:
        if len(p) == 0:
            out.append(list(range(len(text))))
        elif len(p) == 1:
            out.append(np.flatnonzero(arr == p[0]).tolist())
        else:
            out.append(ref.cyclic_hits(text, p) if cyclic else ref.linear_hits(text, p))
    return out


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == np.uint32 and g.ndim == 1, i
        assert g.tolist() == w, i


@pytest.mark.parametrize("n", SIZES)
def test_hits_are_the_brute_force_hits_at_the_layout_boundaries(ctx, n):
    for name, text in _texts(n):
        pats = _patterns(text)
        rf = api.RankFile(text, ctx=ctx)
        got = rf.locate(pats, cyclic=True)
        _same(got, _want(text, pats, True))
        assert sorted(np.concatenate(got[:256]).tolist()) == list(range(n)), (name, n)      # the 256 single bytes: a permutation
        lin = pats[:-1]
        got = rf.locate(lin)
        _same(got, _want(text, lin, False))
        assert [len(g) for g in got] == rf.count(lin).tolist(), (name, n)
        one = rf.locate(lin[260])                                                             # one pattern: one array
        assert isinstance(one, np.ndarray) and one.dtype == np.uint32 and one.tolist() == ref.linear_hits(text, lin[260])


@pytest.mark.parametrize("npat", (1, 63, 64, 65, 256, 257, 1000))
def test_batches_of_mixed_lengths(ctx, npat):
    """Lengths 1..64 mixed inside one batch, every fifth pattern spoiled: empty segments between full ones."""
    text = bce_amd.synth_text(31, 5000).tobytes()
    rs = np.random.RandomState(npat)
    pats = []
    for i in range(npat):
        m, at = int(rs.randint(1, 65)), int(rs.randint(0, len(text)))
        p = bytearray(count_ref.cyclic_cut(text, at, m))
        if i % 5 == 4:
            p[int(rs.randint(0, m))] ^= 0x80                            # (synth_text is 7-bit: this byte occurs nowhere)
        pats.append(bytes(p))
    rf = api.RankFile(text, ctx=ctx)
    _same(rf.locate(pats, cyclic=True), _want(text, pats, True))
    got = rf.locate(pats)
    _same(got, _want(text, pats, False))
    assert [len(g) for g in got] == rf.count(pats).tolist()
    assert all(len(got[i]) == 0 for i in range(4, npat, 5))


def test_wide_intervals_all_equal_text(ctx):
    text = b"z" * 6144
    rf = api.RankFile(text, ctx=ctx)
    pats = [b"z", b"zz", text]
    lin, cyc = rf.locate(pats), rf.locate(pats, cyclic=True)
    assert [len(h) for h in lin] == [6144, 6143, 1] and [len(h) for h in cyc] == [6144] * 3
    for h in cyc:
        assert h.tolist() == list(range(6144))
    assert lin[0].tolist() == list(range(6144)) and lin[1].tolist() == list(range(6143)) and lin[2].tolist() == [0]


def test_wide_intervals_among_short_ones_above_the_sorts_plan_changes(ctx):
    """A period-2 text of 200 000 bytes: every pattern cut from it owns 100 000 rows, a segment of some four hundred workgroups.
    34 of them among 400 short patterns of a second half of ordinary text make 3.4 million rows, above the sizes at which
    radix_sort_pairs changes its plan (tests/test_gpu_sort.py: 4096, 256 * 4096 + 1, 768 * 4096 + 1), in both passes."""
    half = 200000
    tail = bce_amd.synth_text(9, 5000).tobytes().upper()               # no 'a' or 'b' in it
    assert b"a" not in tail and b"b" not in tail
    text = b"ab" * (half // 2) + tail
    rs = np.random.RandomState(5)
    shorts = [tail[at:at + int(rs.randint(2, 9))] for at in rs.randint(0, len(tail) - 9, 400)]
    wide = [(b"ab" * 9)[s:s + m] for m in range(1, 18) for s in (0, 1)]
    pats = []
    for i, s in enumerate(shorts):                                       # the wide ones spread among the short
        pats.append(s)
        if i % 11 == 0 and i // 11 < len(wide):
            pats.append(wide[i // 11])
    assert sum(p in wide for p in pats) == len(wide) == 34
    rf = api.RankFile(text, ctx=ctx)
    lin = rf.locate(pats, max_hits=1 << 23)
    cyc = rf.locate(pats, cyclic=True, max_hits=1 << 23)
    assert sum(len(h) for h in cyc) > 768 * 4096 + 1
    for p, gl, gc in zip(pats, lin, cyc):
        if p in wide:
            first = 0 if p[0] == ord("a") else 1
            # the match needs len(p) bytes of the periodic half (the other half has no 'a' or 'b'): cyclic and linear hits agree
            last = half - len(p)
            want = np.arange(first, last + 1, 2, dtype=np.uint32)
            assert np.array_equal(gl, want) and np.array_equal(gc, want), p
            assert 100000 - 9 <= len(want) <= 100000
        else:
            w = ref.linear_hits(text, p)
            assert gl.tolist() == w and gc.tolist() == ref.cyclic_hits(text, p), p
    for p in (b"ab", b"ba", b"a"):
        assert len(lin[pats.index(p)]) == {b"ab": 100000, b"ba": 99999, b"a": 100000}[p]
    # the pure period-2 text: 100 000 hits each, cyclic; the match of "ba" across the end is not a linear one
    rf = api.RankFile(b"ab" * (half // 2), ctx=ctx)
    cyc, lin = rf.locate([b"ab", b"ba", b"a"], cyclic=True), rf.locate([b"ab", b"ba", b"a"])
    assert [len(h) for h in cyc] == [100000] * 3 and [len(h) for h in lin] == [100000, 99999, 100000]
    assert np.array_equal(cyc[1], np.arange(1, half, 2)) and np.array_equal(lin[1], np.arange(1, half - 1, 2)) and np.array_equal(lin[0], np.arange(0, half, 2))


# ---- the overflow protocol ------------------------------------------------------------------------------------------------------

def _batch(text):
    pats = [text[10:14], b"e", text[-3:] + text[:2], b"\xff", text[100:103], b"th"]
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    return pats, np.frombuffer(b"".join(pats), dtype=np.uint8).copy(), off


@pytest.mark.parametrize("flags", (0, LINEAR))
def test_overflow_protocol_with_host_buffers(ctx, flags):
    text = bce_amd.synth_text(12, 4000).tobytes()
    pats, flat, off = _batch(text)
    want = _want(text, pats, flags == 0)
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    tot = want_off[-1]
    assert len(ref.cyclic_hits(text, pats[2])) == len(ref.linear_hits(text, pats[2])) + 1        # (one hit runs across the end)
    api.RankFile(text, ctx=ctx)
    lib, npat = ctx.lib, len(pats)

    def call(pos, cap):
        hits, total = np.full(npat + 1, 77, dtype=np.uint64), C.c_uint64(123)
        rc = lib.bce_hip_locate(ctx.h, flat.ctypes.data, off.ctypes.data, npat, flags, hits.ctypes.data, None if pos is None else pos.ctypes.data, cap, C.byref(total))
        return rc, hits.tolist(), total.value

    assert call(None, 0) == (0, want_off, tot)                           # the sizing call
    pos = np.full(tot + 2, GUARD, dtype=np.uint32)
    assert call(pos[1:], tot - 1) == (E_OVERFLOW, want_off, tot)
    assert (pos == GUARD).all()                                          # no byte of positions written
    assert b"room for" in lib.bce_hip_last_error(ctx.h)
    assert call(pos[1:], tot) == (0, want_off, tot)
    assert pos[0] == GUARD and pos[-1] == GUARD and pos[1:-1].tolist() == [v for w in want for v in w]
    assert call(pos[1:], 1 << 40) == (0, want_off, tot)                  # room to spare is room enough


@pytest.mark.parametrize("flags", (0, LINEAR))
def test_overflow_protocol_with_device_buffers_at_odd_element_offsets(ctx, flags):
    text = bce_amd.synth_text(12, 4000).tobytes()
    pats, flat, off = _batch(text)
    want = _want(text, pats, flags == 0)
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    tot, npat = want_off[-1], len(pats)
    dev = "cuda:0"
    d_pat = torch.from_numpy(flat).to(dev)
    d_off = torch.zeros(npat + 4, dtype=torch.int64, device=dev)
    d_off[3:3 + npat + 1] = torch.from_numpy(off.astype(np.int64)).to(dev)
    hits_buf = torch.full((npat + 1 + 4,), -5, dtype=torch.int64, device=dev)
    pos_buf = torch.full((tot + 6,), -7, dtype=torch.int32, device=dev)
    d_hits, d_pos = hits_buf[1:1 + npat + 1], pos_buf[3:3 + tot]        # slices at odd element offsets; guard words around them
    torch.cuda.synchronize()
    rf = api.RankFile(text, ctx=ctx)
    args = (d_pat.data_ptr(), d_off[3:].data_ptr(), npat, d_hits.data_ptr())
    assert rf.locate_device(*args, None, 0, cyclic=flags == 0) == tot     # the sizing call
    assert d_hits.cpu().tolist() == want_off and (pos_buf == -7).all()
    hits_buf.fill_(-5)
    torch.cuda.synchronize()
    total = C.c_uint64(0)
    rc = ctx.lib.bce_hip_locate_device(ctx.h, *args[:3], flags, args[3], d_pos.data_ptr(), tot - 1, C.byref(total))
    assert rc == E_OVERFLOW and total.value == tot and d_hits.cpu().tolist() == want_off
    assert (pos_buf == -7).all()
    assert rf.locate_device(*args, d_pos.data_ptr(), tot, cyclic=flags == 0) == tot
    assert d_pos.cpu().tolist() == [v for w in want for v in w]
    assert hits_buf[0].item() == -5 and (hits_buf[npat + 2:] == -5).all() and (pos_buf[:3] == -7).all() and (pos_buf[3 + tot:] == -7).all()
    # decreasing offsets: found by the kernel; the context stays usable
    d_off[3 + 2] = d_off[3 + 4]
    torch.cuda.synchronize()
    with pytest.raises(api.BceError) as e:
        rf.locate_device(*args, d_pos.data_ptr(), tot, cyclic=flags == 0)
    assert e.value.status == E_ARG and "offsets decrease" in str(e.value)
    assert rf.locate(pats[0]).tolist() == ref.linear_hits(text, pats[0])


# ---- states and refusals ----------------------------------------------------------------------------------------------------------

def test_states_in_which_the_locate_is_refused():
    text = bce_amd.synth_text(5, 20000)
    tb = text.tobytes()
    fresh = bytes(bce_amd.compress(text))
    c = api._Ctx(0)
    try:
        lib = c.lib
        pat, off = (C.c_uint8 * 2)(*b"e "), (C.c_uint64 * 2)(0, 2)
        hits, pos, total = (C.c_uint64 * 2)(7, 7), (C.c_uint32 * 4)(9, 9, 9, 9), C.c_uint64(5)
        args = (c.h, C.addressof(pat), C.addressof(off), 1, LINEAR, C.addressof(hits), None, 0, C.byref(total))
        assert lib.bce_hip_locate(*args) == E_STATE and b"holds no planes" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_device(*args) == E_STATE
        api.RankFile(text, ctx=c, build=False)                          # loaded, K1 done, no planes yet
        assert lib.bce_hip_locate(*args) == E_STATE and list(hits) == [7, 7]
        rf = api.RankFile(text, ctx=c)
        want = ref.linear_hits(tb, b"e ")
        assert rf.locate(b"e ").tolist() == want and len(want) > 4
        # argument errors
        bad = (C.c_uint64 * 3)(0, 2, 1)
        assert lib.bce_hip_locate(c.h, C.addressof(pat), C.addressof(bad), 2, 0, C.addressof(hits), None, 0, C.byref(total)) == E_ARG
        assert b"offsets decrease" in lib.bce_hip_last_error(c.h)
        for flags in (2, 3, 0x80000000):
            assert lib.bce_hip_locate(*(args[:4] + (flags,) + args[5:])) == E_ARG
            assert lib.bce_hip_locate_device(*(args[:4] + (flags,) + args[5:])) == E_ARG
        assert lib.bce_hip_locate(c.h, C.addressof(pat), None, 1, 0, C.addressof(hits), None, 0, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate(c.h, C.addressof(pat), C.addressof(off), 1, 0, None, None, 0, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate(c.h, C.addressof(pat), C.addressof(off), 1, 0, C.addressof(hits), None, 4, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate(c.h, C.addressof(pat), C.addressof(off), 1, 0, C.addressof(hits), C.addressof(pos), 4, None) == E_ARG
        assert lib.bce_hip_locate_device(c.h, None, C.addressof(off), 1, 0, C.addressof(hits), None, 0, C.byref(total)) == E_ARG
        assert list(pos) == [9] * 4
        # no patterns at all
        total.value, hits[0] = 5, 7
        assert lib.bce_hip_locate(c.h, None, None, 0, LINEAR, C.addressof(hits), None, 0, C.byref(total)) == 0 and total.value == 0 and hits[0] == 0
        total.value = 5
        assert lib.bce_hip_locate(c.h, None, None, 0, 0, None, None, 0, C.byref(total)) == 0 and total.value == 0
        assert lib.bce_hip_locate_device(c.h, None, None, 0, 0, None, None, 0, C.byref(total)) == 0
        assert rf.locate([]) == []
        # max_hits: refused after the sizing call, with the total named
        with pytest.raises(ValueError, match=str(len(want))):
            rf.locate(b"e ", max_hits=len(want) - 1)
        assert len(rf.locate(b"e ", max_hits=len(want))) == len(want)
        with pytest.raises(ValueError):
            rf.locate(b"")
        with pytest.raises(ValueError):
            rf.locate([b"a", b""])
        # a decode takes the planes and the suffix array away
        assert bce_amd.decompress_device(fresh, ctx=c) == tb
        assert lib.bce_hip_locate(*args) == E_STATE
        # an injected BWT: planes, but no suffix array behind them
        bwt, row0 = count_ref.bwt_of_rotations(b"abracadabra")
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)
        assert rf.count(b"abra", cyclic=True) == 2
        assert lib.bce_hip_locate(*args) == E_STATE and b"no suffix array behind an injected BWT" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_device(*args) == E_STATE
        with pytest.raises(api.BceError) as e:
            rf.locate(b"abra", cyclic=True)
        assert e.value.status == E_STATE
        with pytest.raises(ValueError):
            rf.locate(b"abra")
    finally:
        c.close()


def test_max_hits_is_checked_before_any_room_is_made(ctx, monkeypatch):
    rf = api.RankFile(b"z" * 5000, ctx=ctx)
    made = []
    real = api._positions_buffer
    monkeypatch.setattr(api, "_positions_buffer", lambda total: made.append(total) or real(total))
    with pytest.raises(ValueError, match="5000"):
        rf.locate(b"z", max_hits=4999)
    assert made == []
    assert len(rf.locate(b"z", max_hits=5000)) == 5000 and made == [5000]


def test_more_than_two_to_the_31_rows_are_sized_exactly_and_refused(ctx):
    """300 empty patterns own 2^24 cyclic rows each: 5.03e9 rows, past 2^31 - 1 (the limit of one call) and past 2^32 (the scan's
    totals are u64).  The sizing call writes exact offsets and total and answers BCE_HIP_E_OVERFLOW; nothing is gathered."""
    n, npat = 1 << 24, 300
    rf = api.RankFile(bce_amd.synth_text(24, n), ctx=ctx)
    off, hits, total = np.zeros(npat + 1, dtype=np.uint64), np.full(npat + 1, 77, dtype=np.uint64), C.c_uint64(1)
    pat = np.zeros(1, dtype=np.uint8)
    for fn, arrays in ((ctx.lib.bce_hip_locate, (pat, off, hits)), (ctx.lib.bce_hip_locate_device, None)):
        if arrays is None:
            d_pat, d_off = torch.zeros(1, dtype=torch.uint8, device="cuda:0"), torch.zeros(npat + 1, dtype=torch.int64, device="cuda:0")
            d_hits = torch.full((npat + 1,), 77, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            ptrs = (d_pat.data_ptr(), d_off.data_ptr(), d_hits.data_ptr())
        else:
            ptrs = tuple(a.ctypes.data for a in arrays)
        total.value = 1
        assert fn(ctx.h, ptrs[0], ptrs[1], npat, 0, ptrs[2], None, 0, C.byref(total)) == E_OVERFLOW
        assert total.value == npat * n > 1 << 32 and b"2^31 - 1" in ctx.lib.bce_hip_last_error(ctx.h)
        got = hits.tolist() if arrays is not None else d_hits.cpu().tolist()
        assert got == [p * n for p in range(npat + 1)]
    with pytest.raises(ValueError, match=str(npat * n)):               # Python names the total, as for any batch above max_hits
        rf.locate([b""] * npat, cyclic=True)
    assert ctx.lib.bce_hip_locate(ctx.h, pat.ctypes.data, off.ctypes.data, 127, 0, hits.ctypes.data, None, 0, C.byref(total)) == 0   # 127 * 2^24 rows: inside the limit
    assert total.value == 127 * n


# ---- nothing else moves ---------------------------------------------------------------------------------------------------------

def test_locate_leaves_the_compression_alone_and_outlives_it():
    text = bce_amd.synth_text(5, 50000)
    tb = text.tobytes()
    fresh = bytes(bce_amd.compress(text))
    c = api._Ctx(0)
    try:
        rf = api.RankFile(text, ctx=c)
        pats = [tb[i * 97:i * 97 + 1 + i % 40] for i in range(400)]
        counts = rf.count(pats).tolist()
        before = rf.locate(pats)
        assert [len(h) for h in before] == counts
        _same(before, [ref.linear_hits(tb, p) for p in pats])
        cyc = rf.locate(pats, cyclic=True)
        # locate, then encode: the archive of a fresh context
        assert bytes(api.BCE().encode(rf)) == fresh

        def same_hits():
            for a, b in zip(rf.locate(pats), before):
                assert np.array_equal(a, b)
            for a, b in zip(rf.locate(pats, cyclic=True), cyc):
                assert np.array_equal(a, b)

        # encode, then locate, on the suffix array that encode's depth-first tail has read: the same hits
        same_hits()
        # estimate (it loads and indexes the text again in this context) and count, then locate; a count after a locate is unchanged
        assert bce_amd.estimate(text, ctx=c).bytes == len(fresh)
        assert rf.count(pats).tolist() == counts
        same_hits()
        assert rf.count(pats).tolist() == counts
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def test_module_level_locate_and_limit(ctx):
    tb = bce_amd.synth_text(17, 9000).tobytes()
    pats = [b"e", tb[:9], tb[-4:] + tb[:5], b"\xff", tb + b"x"]
    want = [ref.linear_hits(tb, p) for p in pats]
    _same(bce_amd.locate(tb, pats), want)
    _same(bce_amd.locate(tb, pats, ctx=ctx), want)
    assert bce_amd.locate(tb, pats[1]).tolist() == want[1]
    _same(bce_amd.locate(tb, pats, cyclic=True), [ref.cyclic_hits(tb, p) for p in pats])
    assert len(want[0]) > 7
    _same(bce_amd.locate(tb, pats, limit=7), [w[:7] for w in want])      # the first 7 of each, in text order
    _same(bce_amd.locate(tb, pats, limit=0), [[] for _ in want])
    assert bce_amd.locate(tb, b"e", limit=3).tolist() == want[0][:3]
    with pytest.raises(ValueError):
        bce_amd.locate(tb, b"e", limit=-1)


def _split(offsets, positions, dev):
    assert offsets.dtype == torch.int64 and positions.dtype == torch.int32 and offsets.device == dev and positions.device == dev
    off = offsets.cpu().tolist()
    assert off[0] == 0 and off[-1] == positions.numel()
    pos = positions.cpu().tolist()
    return [pos[a:b] for a, b in zip(off, off[1:])]


def test_locate_tensor_on_a_slice_at_an_odd_offset(ctx):
    data = bce_amd.synth_text(17, 9000)
    big = torch.from_numpy(data).to("cuda:0")
    t = big[1237:1237 + 4099]
    tb = data[1237:1237 + 4099].tobytes()
    assert t.data_ptr() % 2 == 1
    pats = [tb[:9], tb[-9:], tb[-4:] + tb[:5], tb[2000:2033], b"e", tb + b"x", data[1230:1240].tobytes()]
    want = [ref.linear_hits(tb, p) for p in pats]
    assert len(ref.cyclic_hits(tb, pats[2])) == len(want[2]) + 1        # (the match across the seam is what must go)
    assert _split(*bce_amd.locate_tensor(t, pats, ctx=ctx), t.device) == want
    assert _split(*bce_amd.locate_tensor(t, pats[3]), t.device) == [want[3]]                     # a context of its own
    assert _split(*bce_amd.locate_tensor(t, pats, cyclic=True, ctx=ctx), t.device) == [ref.cyclic_hits(tb, p) for p in pats]
    off, pos = bce_amd.locate_tensor(t, [b"\xff", b"\xfe"], ctx=ctx)     # nothing found: an empty tensor
    assert off.tolist() == [0, 0, 0] and pos.numel() == 0 and pos.dtype == torch.int32
    off, pos = bce_amd.locate_tensor(t, [], ctx=ctx)
    assert off.tolist() == [0] and pos.numel() == 0
    with pytest.raises(ValueError):
        bce_amd.locate_tensor(big[::2], b"e")
    with pytest.raises(ValueError):
        bce_amd.locate_tensor(t, b"")


def test_locate_in_archive():
    data = bce_amd.synth_text(41, 10000).tobytes()
    dev = torch.device("cuda:0")
    plain = bytes(bce_amd.compress(data[:4000]))
    pats = [b"the", data[100:108], data[3990:4000], data[3995:4000] + data[:3]]
    assert _split(*bce_amd.locate_in_archive(plain, pats), dev) == [ref.linear_hits(data[:4000], p) for p in pats]
    assert _split(*bce_amd.locate_in_archive(plain, pats, cyclic=True), dev) == [ref.cyclic_hits(data[:4000], p) for p in pats]
    # a checked container of 3 blocks; a pattern that straddles a block boundary: offsets run over the concatenated blocks
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=3)
    table = container.block_table(blob)
    assert len(table) == 3 and all(e[3] is not None for e in table)
    cut = table[0][0]
    pats = [data[cut - 6:cut + 6], data[cut + table[1][0] - 1:cut + table[1][0] + 9], b"e", data[-5:] + data[:5]]
    want = [ref.linear_hits(data, p) for p in pats]
    assert cut - 6 in want[0] and cut + table[1][0] - 1 in want[1]
    assert _split(*bce_amd.locate_in_archive(blob, pats), dev) == want
    assert _split(*bce_amd.locate_in_archive(blob, pats[0]), dev) == [want[0]]
    bad = bytearray(blob)
    bad[12 + 24 * 1 + 16] ^= 1                                           # one flipped text CRC
    with pytest.raises(api.ChecksumError) as e:
        bce_amd.locate_in_archive(bytes(bad), pats)
    assert e.value.block == 1
    blob1 = bce_amd.compress_tensor_blocks(t, blocks=3, checksum=False)  # a -c3 container: no checksums, the same hits
    assert _split(*bce_amd.locate_in_archive(blob1, pats), dev) == want
