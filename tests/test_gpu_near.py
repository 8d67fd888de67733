"""GPU: counts and positions within k mismatches (kd_near.hip through bce_hip_count_near / _locate_near and their _device forms,
RankFile.count_near / locate_near, the tensor and archive wrappers) against the brute force of tests/near_ref.py over the same text:
counts per distance and hit lists with their distances, cyclic and linear, on the smallest shapes at which the wave's walk can go
wrong; the locate's protocol; the states in which the calls are refused; and that nothing else in the context moves."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import near_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_OVERFLOW = -1, -4, -5
LINEAR = 1
GUARD = 0xDEADBEEF


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def four():
    """n = 200 000 over 4 symbols, seeded: (text, a RankFile of it in a context of its own)."""
    text = bytes(np.random.RandomState(7).randint(97, 101, 200000).astype(np.uint8))
    c = api._Ctx(0)
    yield text, api.RankFile(text, ctx=c)
    c.close()


def _check(rf, text, pats, k, cyclic, want_d=None):
    """count_near and locate_near of one batch against the brute force; -> the hits in all"""
    d = want_d or [ref.distances(text, p) for p in pats]
    n = len(text)
    use = [p for p in pats if cyclic or len(p)]
    d = [e for p, e in zip(pats, d) if cyclic or len(p)]
    win = [e if cyclic else e[:max(n - len(p) + 1, 0)] for p, e in zip(use, d)]
    counts = rf.count_near(use, k, cyclic=cyclic)
    assert counts.dtype == np.uint64 and counts.shape == (len(use), k + 1)
    assert counts.tolist() == [np.bincount(w[w <= k], minlength=k + 1)[:k + 1].tolist() for w in win]
    got = rf.locate_near(use, k, cyclic=cyclic)
    assert len(got) == len(use)
    for (pos, dist), w, p in zip(got, win, use):
        at = np.flatnonzero(w <= k)
        assert pos.dtype == np.uint32 and dist.dtype == np.uint8
        assert np.array_equal(pos, at) and np.array_equal(dist, w[at]), (p, k, cyclic)
    return int(counts.sum())


@pytest.mark.parametrize("text", ref.SMALL, ids=lambda t: "%s-%d" % (t[:4].hex(), len(t)))
def test_small_texts_are_the_brute_force(ctx, text):
    """Periodic ties and m > n, k >= m, the empty pattern (cyclic only), an absent byte; bytes(range(256)) * 3: a root interval
    with 256 different candidate bytes, so every lane's four candidates and the ballot's full width are used."""
    rf = api.RankFile(text, ctx=ctx)
    pats = ref.patterns_for(text)
    d = [ref.distances(text, p) for p in pats]
    for k in (0, 1, 2):
        for cyclic in (True, False):
            _check(rf, text, pats, k, cyclic, d)
    assert rf.count_near(b"", 2, cyclic=True).tolist() == [len(text), 0, 0]
    if len(text) >= 2:
        assert rf.count_near(text[:2], 2, cyclic=True).sum() == len(text)          # k >= m: every position, each under its distance
    with pytest.raises(ValueError):
        rf.count_near(b"", 1)
    with pytest.raises(ValueError):
        rf.locate_near([b"a", b""], 1)


def _mixed_batch(text, rs, npat):
    """Half cut from the text with 0 to 3 bytes altered, half random over its alphabet; lengths 8 to 24, mixed."""
    n, pats = len(text), []
    for i in range(npat):
        m = 8 + int(rs.randint(0, 17)) if i % 5 else 8
        if i % 2:
            pats.append(bytes(rs.randint(97, 101, m).astype(np.uint8)))
        else:
            p = ref.cyclic_cut(text, int(rs.randint(0, n)), m)
            pats.append(ref.altered(p, sorted(rs.choice(m, i // 2 % 4, replace=False).tolist()), text))
    return pats


def test_a_batch_of_300_mixed_patterns_on_four_symbols(four):
    """More than one workgroup, lengths that differ within a wave's neighbourhood; k = 2 gives thousands of final intervals per
    pattern, and the first-mismatch children (three per position here) become the next frame dozens of times per pattern."""
    text, rf = four
    pats = _mixed_batch(text, np.random.RandomState(11), 300)
    d = [ref.distances(text, p) for p in pats]
    for k, cyclic in ((0, False), (1, True), (2, True), (2, False)):
        hits = _check(rf, text, pats, k, cyclic, d)
    assert hits == sum(int((e[:len(text) - len(p) + 1] <= 2).sum()) for p, e in zip(pats, d)) > 50000
    assert rf.count(pats).tolist() == rf.count_near(pats, 0)[:, 0].tolist()


def test_random_bytes_where_the_exact_child_dies_and_the_others_live(ctx):
    n = 1 << 20
    text = bytes(np.random.RandomState(3).randint(0, 256, n).astype(np.uint8))
    rf = api.RankFile(text, ctx=ctx)
    rs = np.random.RandomState(4)
    pats = [bytes(rs.randint(0, 256, 6).astype(np.uint8)) for _ in range(56)] + [ref.altered(text[i:i + 6], [i % 6], text) for i in range(1000, 9000, 1000)]
    assert len(pats) == 64
    d = [ref.distances(text, p) for p in pats]
    assert sum(int((e == 0).sum()) for e in d) < 8 <= sum(int((e <= 2).sum()) for e in d)
    for k, cyclic in ((1, True), (2, True), (2, False)):
        _check(rf, text, pats, k, cyclic, d)


def test_a_locate_past_one_scan_block_and_one_waves_segment(four):
    """m = 3, k = 1 on the 4-symbol text: over 10^4 hits for one pattern next to patterns with none, 2100 patterns in all (past one
    2048-element scan block).  Ascending positions, the distance at each reported position, the offsets' differences, and the
    linear total short of the cyclic one by exactly the straddling hits."""
    text, rf = four
    n = len(text)
    pats = [b"abc", b"\x00\x01\x02", b"zzz", text[-2:] + text[:1], text[-1:] + text[:2]] + [b"\x01\x02\x03\x04"] * 2095
    lib, c = rf._c.lib, rf._c
    flat = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    d = [ref.distances(text, p) for p in pats[:5]]
    totals = {}
    for flags in (0, LINEAR):
        hits, total = np.zeros(len(pats) + 1, dtype=np.uint64), C.c_uint64(0)
        assert lib.bce_hip_locate_near(c.h, flat.ctypes.data, off.ctypes.data, len(pats), 1, flags, hits.ctypes.data, None, None, 0, C.byref(total)) == 0
        pos, dist = np.full(total.value, GUARD, dtype=np.uint32), np.full(total.value, 9, dtype=np.uint8)
        assert lib.bce_hip_locate_near(c.h, flat.ctypes.data, off.ctypes.data, len(pats), 1, flags, hits.ctypes.data, pos.ctypes.data, dist.ctypes.data,
                                       total.value, C.byref(total)) == 0
        counts = rf.count_near(pats, 1, cyclic=flags == 0).sum(axis=1)
        assert np.array_equal(np.diff(hits), counts) and hits[0] == 0 and hits[-1] == total.value
        assert counts[0] > 10000 and counts[1] == counts[2] == 0 and not counts[5:].any()
        for i in range(5):
            seg, ds = pos[int(hits[i]):int(hits[i + 1])], dist[int(hits[i]):int(hits[i + 1])]
            assert (np.diff(seg.astype(np.int64)) > 0).all()
            assert np.array_equal(ds, d[i][seg]) and (ds <= 1).all()
            want = np.flatnonzero(d[i] <= 1)
            assert np.array_equal(seg, want if flags == 0 else want[want + 3 <= n])
        totals[flags] = total.value
    straddle = sum(int((e[n - 2:] <= 1).sum()) for e in d)
    assert straddle >= 2 and totals[0] - totals[LINEAR] == straddle


# ---- the protocol ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", (0, LINEAR))
def test_overflow_protocol_with_host_and_device_buffers(ctx, flags):
    text = bce_amd.synth_text(12, 4000).tobytes()
    pats = [text[10:14], b"e", text[-3:] + text[:2], b"\xff", text[100:103], b"th"]
    flat = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    want = [ref.hits(text, p, 1, flags == 0) for p in pats]
    want_off = np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    want_pos, want_dist = np.concatenate([w[0] for w in want]).tolist(), np.concatenate([w[1] for w in want]).tolist()
    tot, npat = want_off[-1], len(pats)
    rf = api.RankFile(text, ctx=ctx)
    lib = ctx.lib

    def call(pos, dist, cap):
        hits, total = np.full(npat + 1, 77, dtype=np.uint64), C.c_uint64(123)
        rc = lib.bce_hip_locate_near(ctx.h, flat.ctypes.data, off.ctypes.data, npat, 1, flags, hits.ctypes.data, None if pos is None else pos.ctypes.data,
                                     None if dist is None else dist.ctypes.data, cap, C.byref(total))
        return rc, hits.tolist(), total.value

    assert call(None, None, 0) == (0, want_off, tot)                      # the sizing call
    pos, dist = np.full(tot + 2, GUARD, dtype=np.uint32), np.full(tot + 2, 9, dtype=np.uint8)
    assert call(pos[1:], dist[1:], tot - 1) == (E_OVERFLOW, want_off, tot)
    assert (pos == GUARD).all() and (dist == 9).all()                     # nothing of the two outputs written
    assert b"room for" in lib.bce_hip_last_error(ctx.h)
    assert call(pos[1:], dist[1:], tot) == (0, want_off, tot)
    assert pos[0] == GUARD and pos[-1] == GUARD and pos[1:-1].tolist() == want_pos
    assert dist[0] == 9 and dist[-1] == 9 and dist[1:-1].tolist() == want_dist
    assert call(pos[1:], None, tot)[0] == E_ARG and call(None, dist[1:], 0)[0] == E_ARG   # positions and distances: together or not at all
    # the same with device buffers, slices at odd element offsets with guard words around them
    dev = "cuda:0"
    d_pat = torch.from_numpy(flat).to(dev)
    d_off = torch.zeros(npat + 4, dtype=torch.int64, device=dev)
    d_off[3:3 + npat + 1] = torch.from_numpy(off.astype(np.int64)).to(dev)
    hits_buf = torch.full((npat + 1 + 4,), -5, dtype=torch.int64, device=dev)
    pos_buf = torch.full((tot + 6,), -7, dtype=torch.int32, device=dev)
    dist_buf = torch.full((tot + 6,), 9, dtype=torch.uint8, device=dev)
    d_hits, d_pos, d_dist = hits_buf[1:1 + npat + 1], pos_buf[3:3 + tot], dist_buf[3:3 + tot]
    torch.cuda.synchronize()
    args = (d_pat.data_ptr(), d_off[3:].data_ptr(), npat, 1, d_hits.data_ptr())
    assert rf.locate_near_device(*args, None, None, 0, cyclic=flags == 0) == tot
    assert d_hits.cpu().tolist() == want_off and (pos_buf == -7).all() and (dist_buf == 9).all()
    total = C.c_uint64(0)
    rc = lib.bce_hip_locate_near_device(ctx.h, *args[:4], flags, args[4], d_pos.data_ptr(), d_dist.data_ptr(), tot - 1, C.byref(total))
    assert rc == E_OVERFLOW and total.value == tot and d_hits.cpu().tolist() == want_off
    assert (pos_buf == -7).all() and (dist_buf == 9).all()
    assert rf.locate_near_device(*args, d_pos.data_ptr(), d_dist.data_ptr(), tot, cyclic=flags == 0) == tot
    assert d_pos.cpu().tolist() == want_pos and d_dist.cpu().tolist() == want_dist
    assert hits_buf[0].item() == -5 and (hits_buf[npat + 2:] == -5).all() and (pos_buf[:3] == -7).all() and (pos_buf[3 + tot:] == -7).all()
    assert (dist_buf[:3] == 9).all() and (dist_buf[3 + tot:] == 9).all()
    # count_near_device: npat * (k + 1) words
    d_cnt = torch.full((npat * 2 + 2,), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rf.count_near_device(args[0], args[1], npat, 1, d_cnt[1:].data_ptr())
    assert d_cnt[1:-1].cpu().tolist() == np.concatenate([ref.counts(text, p, 1) for p in pats]).tolist() and d_cnt[0] == -3 and d_cnt[-1] == -3
    # decreasing offsets and a pattern of 4097 bytes: found by the kernel; the context stays usable
    d_off[3 + 2] = d_off[3 + 4]
    torch.cuda.synchronize()
    for fn in (lambda: rf.locate_near_device(*args, d_pos.data_ptr(), d_dist.data_ptr(), tot, cyclic=flags == 0),
               lambda: rf.count_near_device(args[0], args[1], npat, 1, d_cnt[1:].data_ptr())):
        with pytest.raises(api.BceError) as e:
            fn()
        assert e.value.status == E_ARG and "offsets decrease" in str(e.value)
    long_pat = torch.full((4097,), 101, dtype=torch.uint8, device=dev)
    long_off = torch.tensor([0, 4097], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(api.BceError) as e:
        rf.count_near_device(long_pat.data_ptr(), long_off.data_ptr(), 1, 1, d_cnt[1:].data_ptr())
    assert e.value.status == E_ARG and "4096" in str(e.value)
    with pytest.raises(api.BceError) as e:
        rf.locate_near_device(long_pat.data_ptr(), long_off.data_ptr(), 1, 1, d_hits.data_ptr(), None, None, 0)
    assert e.value.status == E_ARG
    long_off[1] = 4096                                                   # the bound itself is served
    torch.cuda.synchronize()
    rf.count_near_device(long_pat.data_ptr(), long_off.data_ptr(), 1, 1, d_cnt[1:].data_ptr())
    assert d_cnt[1:3].cpu().tolist() == [0, 0]
    assert rf.locate_near(pats[0], 1)[0].tolist() == ref.hits(text, pats[0], 1, False)[0].tolist()


def test_states_and_arguments_that_are_refused():
    text = bce_amd.synth_text(5, 20000)
    tb = text.tobytes()
    c = api._Ctx(0)
    try:
        lib, a = c.lib, C.addressof
        pat, off = (C.c_uint8 * 2)(*b"e "), (C.c_uint64 * 2)(0, 2)
        hits, cnt, total = (C.c_uint64 * 2)(7, 7), (C.c_uint64 * 3)(7, 7, 7), C.c_uint64(5)
        largs = (c.h, a(pat), a(off), 1, 1, LINEAR, a(hits), None, None, 0, C.byref(total))
        cargs = (c.h, a(pat), a(off), 1, 1, a(cnt))
        assert lib.bce_hip_locate_near(*largs) == E_STATE and b"holds no planes" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_near_device(*largs) == E_STATE and lib.bce_hip_count_near(*cargs) == E_STATE
        assert lib.bce_hip_count_near_device(*cargs) == E_STATE
        for k in (3, 4, 0xFFFFFFFF):                                     # k is judged before the state
            assert lib.bce_hip_count_near(*(cargs[:4] + (k,) + cargs[5:])) == E_ARG
            assert lib.bce_hip_count_near_device(*(cargs[:4] + (k,) + cargs[5:])) == E_ARG
            assert lib.bce_hip_locate_near(*(largs[:4] + (k,) + largs[5:])) == E_ARG
            assert lib.bce_hip_locate_near_device(*(largs[:4] + (k,) + largs[5:])) == E_ARG
        rf = api.RankFile(text, ctx=c)
        assert list(hits) == [7, 7] and list(cnt) == [7, 7, 7]
        want = ref.hits(tb, b"e ", 1, False)
        got = rf.locate_near(b"e ", 1)
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and len(want[0]) > 100
        for k in (3, 0xFFFFFFFF):
            assert lib.bce_hip_count_near(*(cargs[:4] + (k,) + cargs[5:])) == E_ARG
            assert lib.bce_hip_locate_near(*(largs[:4] + (k,) + largs[5:])) == E_ARG
        for bad_k in (3, -1):
            with pytest.raises(ValueError):
                rf.count_near(b"e ", bad_k)
            with pytest.raises(ValueError):
                rf.locate_near(b"e ", bad_k)
        # m = 4097 with host buffers; 4096 is served
        big = np.full(4097, 101, dtype=np.uint8)
        boff = (C.c_uint64 * 2)(0, 4097)
        assert lib.bce_hip_count_near(c.h, big.ctypes.data, a(boff), 1, 1, a(cnt)) == E_ARG and b"4096" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_near(c.h, big.ctypes.data, a(boff), 1, 1, 0, a(hits), None, None, 0, C.byref(total)) == E_ARG
        with pytest.raises(ValueError):
            rf.count_near(big.tobytes(), 1)
        assert rf.count_near(big[:4096].tobytes(), 2).tolist() == [0, 0, 0]
        # decreasing offsets, flag bits, null arrays
        bad = (C.c_uint64 * 3)(0, 2, 1)
        assert lib.bce_hip_count_near(c.h, a(pat), a(bad), 2, 1, a(cnt)) == E_ARG and b"offsets decrease" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_near(c.h, a(pat), a(bad), 2, 1, 0, a(hits), None, None, 0, C.byref(total)) == E_ARG
        for flags in (2, 3, 0x80000000):
            assert lib.bce_hip_locate_near(*(largs[:5] + (flags,) + largs[6:])) == E_ARG
            assert lib.bce_hip_locate_near_device(*(largs[:5] + (flags,) + largs[6:])) == E_ARG
        assert lib.bce_hip_count_near(c.h, a(pat), a(off), 1, 1, None) == E_ARG
        assert lib.bce_hip_count_near(c.h, a(pat), None, 1, 1, a(cnt)) == E_ARG
        assert lib.bce_hip_locate_near(c.h, a(pat), a(off), 1, 1, 0, None, None, None, 0, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate_near(c.h, a(pat), a(off), 1, 1, 0, a(hits), None, None, 4, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate_near(c.h, a(pat), a(off), 1, 1, 0, a(hits), None, None, 0, None) == E_ARG
        # no patterns at all
        total.value, hits[0] = 5, 7
        assert lib.bce_hip_locate_near(c.h, None, None, 0, 2, LINEAR, a(hits), None, None, 0, C.byref(total)) == 0 and total.value == 0 and hits[0] == 0
        assert lib.bce_hip_locate_near_device(c.h, None, None, 0, 2, 0, None, None, None, 0, C.byref(total)) == 0
        assert lib.bce_hip_count_near(c.h, None, None, 0, 2, None) == 0 and lib.bce_hip_count_near_device(c.h, None, None, 0, 2, None) == 0
        assert rf.locate_near([], 1) == [] and rf.count_near([], 1).shape == (0, 2)
        # max_hits and limit: locate()'s rules
        with pytest.raises(ValueError, match=str(len(want[0]))):
            rf.locate_near(b"e ", 1, max_hits=len(want[0]) - 1)
        pos, dist = rf.locate_near(b"e ", 1, limit=7)
        assert pos.tolist() == want[0][:7].tolist() and dist.tolist() == want[1][:7].tolist()
        # an injected BWT: planes, but no suffix array behind them -- counts work, positions do not
        bwt, row0 = count_ref.bwt_of_rotations(b"abracadabra")
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)
        assert rf.count_near(b"abra", 1, cyclic=True).tolist() == ref.counts(b"abracadabra", b"abra", 1).tolist()
        assert rf.count_near([b"abra", b"cad", b""], 2, cyclic=True).tolist() == [ref.counts(b"abracadabra", p, 2).tolist() for p in (b"abra", b"cad", b"")]
        assert lib.bce_hip_locate_near(*largs) == E_STATE and b"no suffix array behind an injected BWT" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_near_device(*largs) == E_STATE
        with pytest.raises(api.BceError) as e:
            rf.locate_near(b"abra", 1, cyclic=True)
        assert e.value.status == E_STATE
        with pytest.raises(ValueError):
            rf.locate_near(b"abra", 1)
        with pytest.raises(ValueError):
            rf.count_near(b"abra", 1)
    finally:
        c.close()


def test_k_zero_is_count_and_locate(four):
    text, rf = four
    pats = _mixed_batch(text, np.random.RandomState(21), 80) + [text[:3], text[-2:] + text[:2], b"a", text[5:9] * 3, b"zz"]
    for cyclic in (False, True):
        assert rf.count_near(pats, 0, cyclic=cyclic)[:, 0].tolist() == rf.count(pats, cyclic=cyclic).tolist()
        for (pos, dist), want in zip(rf.locate_near(pats, 0, cyclic=cyclic), rf.locate(pats, cyclic=cyclic)):
            assert np.array_equal(pos, want) and not dist.any()
    assert rf.count_near(b"", 0, cyclic=True).tolist() == [rf.count(b"", cyclic=True)]


def test_the_queries_leave_the_compression_alone_and_outlive_it():
    text = bce_amd.synth_text(5, 50000)
    tb = text.tobytes()
    fresh = bytes(bce_amd.compress(text))
    c = api._Ctx(0)
    try:
        rf = api.RankFile(text, ctx=c)
        pats = [tb[i * 97:i * 97 + 4 + i % 12] for i in range(100)]
        counts = rf.count_near(pats, 2)
        assert counts.tolist() == [ref.counts(tb, p, 2, False).tolist() for p in pats]
        before = rf.locate_near(pats, 1)
        assert bytes(api.BCE().encode(rf)) == fresh                     # queries, then encode: the archive of a fresh context
        assert np.array_equal(rf.count_near(pats, 2), counts)           # and after it, on the planes it has read
        for (p0, d0), (p1, d1) in zip(before, rf.locate_near(pats, 1)):
            assert np.array_equal(p0, p1) and np.array_equal(d0, d1)
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def _split(offsets, positions, dists, dev):
    assert offsets.dtype == torch.int64 and positions.dtype == torch.int32 and dists.dtype == torch.uint8
    assert offsets.device == dev and positions.device == dev and dists.device == dev
    off = offsets.cpu().tolist()
    assert off[0] == 0 and off[-1] == positions.numel() == dists.numel()
    pos, dist = positions.cpu().tolist(), dists.cpu().tolist()
    return [(pos[a:b], dist[a:b]) for a, b in zip(off, off[1:])]


def _want(text, pats, k, cyclic):
    return [tuple(v.tolist() for v in ref.hits(text, p, k, cyclic)) for p in pats]


def test_module_level_and_tensor_functions_on_a_slice_at_an_odd_offset(ctx):
    data = bce_amd.synth_text(17, 9000)
    big = torch.from_numpy(data).to("cuda:0")
    t = big[1237:1237 + 4099]
    tb = data[1237:1237 + 4099].tobytes()
    assert t.data_ptr() % 2 == 1
    pats = [tb[:9], tb[-9:], tb[-4:] + tb[:5], ref.altered(tb[2000:2033], [0, 32], tb), b"e", tb + b"x", data[1230:1240].tobytes()]
    pats = [p for p in pats if len(p) <= 4096]
    for k, cyclic in ((1, False), (2, True)):
        want = _want(tb, pats, k, cyclic)
        assert _split(*bce_amd.locate_near_tensor(t, pats, k, cyclic=cyclic, ctx=ctx), t.device) == want
        assert bce_amd.count_near_tensor(t, pats, k, cyclic=cyclic, ctx=ctx).tolist() == [ref.counts(tb, p, k, cyclic).tolist() for p in pats]
        got = bce_amd.locate_near(tb, pats, k, cyclic=cyclic)
        assert [(p.tolist(), d.tolist()) for p, d in got] == want
        assert bce_amd.count_near(tb, pats, k, cyclic=cyclic).tolist() == [ref.counts(tb, p, k, cyclic).tolist() for p in pats]
    assert _split(*bce_amd.locate_near_tensor(t, pats[3], 2), t.device) == _want(tb, pats[3:4], 2, False)     # a context of its own
    assert bce_amd.count_near_tensor(t, pats[3], 2).tolist() == ref.counts(tb, pats[3], 2, False).tolist()
    off, pos, dist = bce_amd.locate_near_tensor(t, [b"\xff\xfe\xfd", b"\xfe\xfd\xfc\xfb"], 2, ctx=ctx)   # nothing found: empty tensors
    assert off.tolist() == [0, 0, 0] and pos.numel() == 0 and dist.numel() == 0 and dist.dtype == torch.uint8
    off, pos, dist = bce_amd.locate_near_tensor(t, [], 1, ctx=ctx)
    assert off.tolist() == [0] and pos.numel() == 0
    with pytest.raises(ValueError):
        bce_amd.locate_near_tensor(t, b"", 1)
    with pytest.raises(ValueError):
        bce_amd.locate_near_tensor(t, b"e", 3)


def test_in_archive_on_a_plain_archive_and_across_a_block_boundary():
    data = bce_amd.synth_text(41, 10000).tobytes()
    dev = torch.device("cuda:0")
    plain = bytes(bce_amd.compress(data[:4000]))
    pats = [b"the", ref.altered(data[100:108], [3], data), data[3990:4000], data[3995:4000] + data[:3]]
    for cyclic in (False, True):
        assert _split(*bce_amd.locate_near_in_archive(plain, pats, 1, cyclic=cyclic), dev) == _want(data[:4000], pats, 1, cyclic)
        assert bce_amd.count_near_in_archive(plain, pats, 1, cyclic=cyclic).tolist() == [ref.counts(data[:4000], p, 1, cyclic).tolist() for p in pats]
    # a checked container of two blocks; a pattern placed across the block boundary, one byte altered on either side of it
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)
    table = container.block_table(blob)
    assert len(table) == 2 and all(e[3] is not None for e in table)
    cut = table[0][0]
    pats = [ref.altered(data[cut - 6:cut + 6], [5, 6], data), data[cut - 1:cut + 9], b"e", data[-5:] + data[:5]]
    want = _want(data, pats, 2, False)
    assert (cut - 6, 2) in zip(*want[0]) and (cut - 1, 0) in zip(*want[1])
    assert _split(*bce_amd.locate_near_in_archive(blob, pats, 2), dev) == want
    assert bce_amd.count_near_in_archive(blob, pats, 2).tolist() == [ref.counts(data, p, 2, False).tolist() for p in pats]
    assert bce_amd.count_near_in_archive(blob, pats[0], 2).tolist() == ref.counts(data, pats[0], 2, False).tolist()
