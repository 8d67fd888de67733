"""GPU: counts and positions within k edits (kd_edit.hip through bce_hip_count_edit / _locate_edit and their _device forms,
RankFile.count_edit / locate_edit, the tensor and archive wrappers) against the definition in tests/edit_ref.py over the same text:
positions, lengths, distances, hit offsets and counts per distance, cyclic and linear, on the smallest shapes at which the wave's
walk and the reduce can go wrong; the locate's protocol; the states in which the calls are refused; and that nothing else in the
context moves."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import edit_ref as ref
import near_ref

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
    """edit_ref.four_case(): (text, patterns, their tables, a RankFile of the text in a context of its own)."""
    text, pats = ref.four_case()
    c = api._Ctx(0)
    yield text, pats, [ref.table(text, p) for p in pats], api.RankFile(text, ctx=c)
    c.close()


def _check(rf, text, pats, k, cyclic, tables=None):
    """count_edit and locate_edit of one batch against the definition; -> (the hits in all, those whose length is not m)"""
    tables = tables or [ref.table(text, p) for p in pats]
    n = len(text)
    use = [(p, E) for p, E in zip(pats, tables) if cyclic or len(p)]
    want = [ref.hits_of(E, len(p), n, k, cyclic) for p, E in use]
    counts = rf.count_edit([p for p, _ in use], k, cyclic=cyclic)
    assert counts.dtype == np.uint64 and counts.shape == (len(use), k + 1)
    assert counts.tolist() == [ref.counts_of(w[2], k).tolist() for w in want]
    got = rf.locate_edit([p for p, _ in use], k, cyclic=cyclic)
    assert len(got) == len(use)
    other = 0
    for (pos, lens, dist), w, (p, _) in zip(got, want, use):
        assert pos.dtype == np.uint32 and lens.dtype == np.uint16 and dist.dtype == np.uint8
        assert np.array_equal(pos, w[0]) and np.array_equal(lens, w[1]) and np.array_equal(dist, w[2]), (p, k, cyclic)
        other += int((lens != len(p)).sum())
    return int(counts.sum()), other


@pytest.mark.parametrize("text", near_ref.SMALL, ids=lambda t: "%s-%d" % (t[:4].hex(), len(t)))
def test_small_texts_are_the_definition(ctx, text):
    """Periodic ties and m > n, k >= m, the empty pattern (cyclic only), an absent byte, indels planted at the second byte, in the
    middle and at the second-to-last byte; bytes(range(256)) * 3: a root interval with 256 different candidate bytes."""
    rf = api.RankFile(text, ctx=ctx)
    pats = ref.patterns_for(text)
    tables = [ref.table(text, p) for p in pats]
    for k in (0, 1, 2):
        for cyclic in (True, False):
            _check(rf, text, pats, k, cyclic, tables)
    assert rf.count_edit(b"", 2, cyclic=True).tolist() == [len(text), 0, 0]
    pos, lens, dist = rf.locate_edit(b"", 1, cyclic=True)
    assert pos.tolist() == list(range(len(text))) and not lens.any() and not dist.any()
    if len(text) >= 2:
        assert rf.count_edit(text[:2], 2, cyclic=True).sum() == len(text)          # k >= m: every position, each under its distance
    with pytest.raises(ValueError):
        rf.count_edit(b"", 1)
    with pytest.raises(ValueError):
        rf.locate_edit([b"a", b""], 1)


@pytest.mark.parametrize("part", range(4))
def test_texts_of_every_alphabet_with_planted_edits(ctx, part):
    """All of near_ref.texts(), a quarter a case (its last, the 768-byte text, is near_ref.SMALL's above): the seven fixed ones,
    bytes(range(256)) among them, and 50 of 1 to 40 bytes over 2, 3 and 256 symbols; every pattern of edit_ref.patterns_for, all
    k, both modes."""
    texts = near_ref.texts()
    assert len(texts) == 58 and texts[-1] == near_ref.SMALL[5]
    for text in texts[:-1][part::4]:
        rf = api.RankFile(text, ctx=ctx)
        pats = ref.patterns_for(text)
        tables = [ref.table(text, p) for p in pats]
        for k in (0, 1, 2):
            for cyclic in (True, False):
                _check(rf, text, pats, k, cyclic, tables)


def test_a_text_of_one_symbol_leaves_each_position_once(ctx):
    """Every script lands on the same rows: hundreds of candidates per position, one head each, at distance 0 and length 8."""
    text, p = b"a" * 4096, b"a" * 8
    rf = api.RankFile(text, ctx=ctx)
    for cyclic in (True, False):
        pos, lens, dist = rf.locate_edit(p, 2, cyclic=cyclic)
        want = ref.hits(text, p, 2, cyclic)
        assert np.array_equal(pos, want[0]) and np.array_equal(lens, want[1]) and np.array_equal(dist, want[2])
        assert rf.count_edit(p, 2, cyclic=cyclic).tolist() == ref.counts_of(want[2], 2).tolist()
    pos, lens, dist = rf.locate_edit(p, 2, cyclic=True)
    assert pos.tolist() == list(range(4096)) and (lens == 8).all() and not dist.any()
    pos, lens, dist = rf.locate_edit(p, 2)                               # the last positions: through shorter alignments, deletions
    assert pos.tolist() == list(range(4096 - 6 + 1)) and lens[-3:].tolist() == [8, 7, 6] and dist[-3:].tolist() == [0, 1, 2]


def test_a_batch_of_mixed_planted_patterns_on_four_symbols(four):
    """More than one workgroup, lengths that differ within a wave; positions that are candidates at three lengths and more, hits
    whose best length is not m (tests/test_edit_cpu.py asserts both of the case)."""
    text, pats, tables, rf = four
    for k, cyclic in ((0, False), (1, True), (1, False), (2, True), (2, False)):
        hits, other = _check(rf, text, pats, k, cyclic, tables)
    assert hits > 50000 and other > 1000


def test_random_bytes_where_most_children_die(ctx):
    text, pats = ref.random_case()
    rf = api.RankFile(text, ctx=ctx)
    tables = [ref.table(text, p) for p in pats]
    for cyclic in (True, False):
        hits, other = _check(rf, text, pats, 2, cyclic, tables)
        assert hits >= 8 and other >= 4


def test_a_locate_past_one_scan_block_and_one_waves_segment(four):
    """2100 patterns (past one 2048-element scan block), k = 1: over 10^4 hits for one pattern next to patterns with none.  The
    offsets' differences are the counts, positions ascend, and every record is the definition's."""
    text, rf = four[0], four[3]
    n = len(text)
    text2, pats = ref.scan_case()
    assert text2 == text
    lib, c = rf._c.lib, rf._c
    flat = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    tables = [ref.table(text, p) for p in pats[:5]]
    for flags in (0, LINEAR):
        hits, total = np.zeros(len(pats) + 1, dtype=np.uint64), C.c_uint64(0)
        assert lib.bce_hip_locate_edit(c.h, flat.ctypes.data, off.ctypes.data, len(pats), 1, flags, hits.ctypes.data, None, None, None, 0,
                                       C.byref(total)) == 0
        pos, lens, dist = np.full(total.value, GUARD, dtype=np.uint32), np.full(total.value, 7, dtype=np.uint16), np.full(total.value, 9, dtype=np.uint8)
        assert lib.bce_hip_locate_edit(c.h, flat.ctypes.data, off.ctypes.data, len(pats), 1, flags, hits.ctypes.data, pos.ctypes.data, lens.ctypes.data,
                                       dist.ctypes.data, total.value, C.byref(total)) == 0
        counts = rf.count_edit(pats, 1, cyclic=flags == 0)
        assert np.array_equal(np.diff(hits), counts.sum(axis=1)) and hits[0] == 0 and hits[-1] == total.value
        assert counts[0].sum() > 10000 and not counts[1].any() and not counts[2].any() and not counts[5:].any()
        for i in range(5):
            a, b = int(hits[i]), int(hits[i + 1])
            want = ref.hits_of(tables[i], len(pats[i]), n, 1, flags == 0)
            assert np.array_equal(pos[a:b], want[0]) and np.array_equal(lens[a:b], want[1]) and np.array_equal(dist[a:b], want[2])
            assert counts[i].tolist() == ref.counts_of(want[2], 1).tolist()


def test_linear_mode_restricts_the_lengths_before_the_minimum(ctx):
    """The header's example at the end of a text: cyclic (n - 3, distance 0, length 4), linear (n - 3, distance 2, length 3)."""
    text, p = ref.linear_case()
    n = len(text)
    rf = api.RankFile(text, ctx=ctx)
    for cyclic, want in ((True, (n - 3, 4, 0)), (False, (n - 3, 3, 2))):
        pos, lens, dist = rf.locate_edit(p, 2, cyclic=cyclic)
        full = ref.hits(text, p, 2, cyclic)
        assert np.array_equal(pos, full[0]) and np.array_equal(lens, full[1]) and np.array_equal(dist, full[2])
        at = pos.tolist().index(n - 3)
        assert (int(pos[at]), int(lens[at]), int(dist[at])) == want
        assert rf.count_edit(p, 2, cyclic=cyclic).tolist() == ref.counts_of(full[2], 2).tolist()
    assert n - 3 not in rf.locate_edit(p, 1)[0].tolist() and n - 3 in rf.locate_edit(p, 1, cyclic=True)[0].tolist()


def test_k_zero_is_count_and_locate(four):
    text, pats, _, rf = four
    pats = pats + [text[:3], text[-2:] + text[:2], b"a", text[5:9] * 3, b"zz"]
    for cyclic in (False, True):
        assert rf.count_edit(pats, 0, cyclic=cyclic)[:, 0].tolist() == rf.count(pats, cyclic=cyclic).tolist()
        for (pos, lens, dist), want, p in zip(rf.locate_edit(pats, 0, cyclic=cyclic), rf.locate(pats, cyclic=cyclic), pats):
            assert np.array_equal(pos, want) and not dist.any() and (lens == len(p)).all()
    assert rf.count_edit(b"", 0, cyclic=True).tolist() == [rf.count(b"", cyclic=True)]


def test_patterns_of_one_byte_are_the_hamming_search(four):
    text, _, _, rf = four
    pats = [b"a", b"d", b"z", b"\x00"]
    for k in (0, 1, 2):
        for cyclic in (False, True):
            assert rf.count_edit(pats, k, cyclic=cyclic).tolist() == rf.count_near(pats, k, cyclic=cyclic).tolist()
            for (pos, lens, dist), (npos, ndist) in zip(rf.locate_edit(pats, k, cyclic=cyclic), rf.locate_near(pats, k, cyclic=cyclic)):
                assert np.array_equal(pos, npos) and np.array_equal(dist, ndist) and (lens == 1).all()
    assert rf.count_edit(b"", 2, cyclic=True).tolist() == rf.count_near(b"", 2, cyclic=True).tolist()


# ---- the protocol ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", (0, LINEAR))
def test_overflow_protocol_with_host_and_device_buffers(ctx, flags):
    text = bce_amd.synth_text(12, 4000).tobytes()
    pats = [text[10:14], b"e", text[-3:] + text[:2], b"\xff", text[100:102] + text[103:106], b"th", text[-4:]]
    flat = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    want = [ref.hits(text, p, 1, flags == 0) for p in pats]
    want_off = np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    want_pos, want_len, want_dist = (np.concatenate([w[i] for w in want]).tolist() for i in range(3))
    tot, npat = want_off[-1], len(pats)
    rf = api.RankFile(text, ctx=ctx)
    lib = ctx.lib
    ptr = lambda v: None if v is None else v.ctypes.data  # noqa: E731

    def call(pos, lens, dist, cap):
        hits, total = np.full(npat + 1, 77, dtype=np.uint64), C.c_uint64(123)
        rc = lib.bce_hip_locate_edit(ctx.h, flat.ctypes.data, off.ctypes.data, npat, 1, flags, hits.ctypes.data, ptr(pos), ptr(lens), ptr(dist), cap,
                                     C.byref(total))
        return rc, hits.tolist(), total.value

    assert call(None, None, None, 0) == (0, want_off, tot)                # the sizing call
    pos, lens, dist = np.full(tot + 2, GUARD, dtype=np.uint32), np.full(tot + 2, 7, dtype=np.uint16), np.full(tot + 2, 9, dtype=np.uint8)
    assert call(pos[1:], lens[1:], dist[1:], tot - 1) == (E_OVERFLOW, want_off, tot)
    assert (pos == GUARD).all() and (lens == 7).all() and (dist == 9).all()   # nothing of the three outputs written
    assert b"room for" in lib.bce_hip_last_error(ctx.h)
    assert call(pos[1:], lens[1:], dist[1:], tot) == (0, want_off, tot)
    assert pos[0] == GUARD and pos[-1] == GUARD and pos[1:-1].tolist() == want_pos
    assert lens[0] == 7 and lens[-1] == 7 and lens[1:-1].tolist() == want_len
    assert dist[0] == 9 and dist[-1] == 9 and dist[1:-1].tolist() == want_dist
    assert call(pos[1:], lens[1:], None, tot)[0] == E_ARG and call(pos[1:], None, dist[1:], tot)[0] == E_ARG   # together or not at all
    assert call(None, None, dist[1:], 0)[0] == E_ARG
    # the same with device buffers, slices at odd element offsets with guard words around them
    dev = "cuda:0"
    d_pat = torch.from_numpy(flat).to(dev)
    d_off = torch.zeros(npat + 4, dtype=torch.int64, device=dev)
    d_off[3:3 + npat + 1] = torch.from_numpy(off.astype(np.int64)).to(dev)
    hits_buf = torch.full((npat + 1 + 4,), -5, dtype=torch.int64, device=dev)
    pos_buf = torch.full((tot + 6,), -7, dtype=torch.int32, device=dev)
    len_buf = torch.full((tot + 6,), -2, dtype=torch.int16, device=dev)
    dist_buf = torch.full((tot + 6,), 9, dtype=torch.uint8, device=dev)
    d_hits, d_pos, d_len, d_dist = hits_buf[1:1 + npat + 1], pos_buf[3:3 + tot], len_buf[3:3 + tot], dist_buf[3:3 + tot]
    torch.cuda.synchronize()
    args = (d_pat.data_ptr(), d_off[3:].data_ptr(), npat, 1, d_hits.data_ptr())
    assert rf.locate_edit_device(*args, None, None, None, 0, cyclic=flags == 0) == tot
    assert d_hits.cpu().tolist() == want_off and (pos_buf == -7).all() and (len_buf == -2).all() and (dist_buf == 9).all()
    total = C.c_uint64(0)
    rc = lib.bce_hip_locate_edit_device(ctx.h, *args[:4], flags, args[4], d_pos.data_ptr(), d_len.data_ptr(), d_dist.data_ptr(), tot - 1, C.byref(total))
    assert rc == E_OVERFLOW and total.value == tot and d_hits.cpu().tolist() == want_off
    assert (pos_buf == -7).all() and (len_buf == -2).all() and (dist_buf == 9).all()
    assert rf.locate_edit_device(*args, d_pos.data_ptr(), d_len.data_ptr(), d_dist.data_ptr(), tot, cyclic=flags == 0) == tot
    assert d_pos.cpu().tolist() == want_pos and d_len.cpu().tolist() == want_len and d_dist.cpu().tolist() == want_dist
    assert hits_buf[0].item() == -5 and (hits_buf[npat + 2:] == -5).all() and (pos_buf[:3] == -7).all() and (pos_buf[3 + tot:] == -7).all()
    assert (len_buf[:3] == -2).all() and (len_buf[3 + tot:] == -2).all() and (dist_buf[:3] == 9).all() and (dist_buf[3 + tot:] == 9).all()
    # count_edit_device: npat * (k + 1) words
    d_cnt = torch.full((npat * 2 + 2,), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rf.count_edit_device(args[0], args[1], npat, 1, d_cnt[1:].data_ptr(), cyclic=flags == 0)
    assert d_cnt[1:-1].cpu().tolist() == np.concatenate([ref.counts_of(w[2], 1) for w in want]).tolist() and d_cnt[0] == -3 and d_cnt[-1] == -3
    # decreasing offsets and a pattern of 4097 bytes: found by the kernel; the context stays usable
    d_off[3 + 2] = d_off[3 + 4]
    torch.cuda.synchronize()
    for fn in (lambda: rf.locate_edit_device(*args, d_pos.data_ptr(), d_len.data_ptr(), d_dist.data_ptr(), tot, cyclic=flags == 0),
               lambda: rf.count_edit_device(args[0], args[1], npat, 1, d_cnt[1:].data_ptr())):
        with pytest.raises(api.BceError) as e:
            fn()
        assert e.value.status == E_ARG and "offsets decrease" in str(e.value)
    long_pat = torch.full((4097,), 101, dtype=torch.uint8, device=dev)
    long_off = torch.tensor([0, 4097], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(api.BceError) as e:
        rf.count_edit_device(long_pat.data_ptr(), long_off.data_ptr(), 1, 1, d_cnt[1:].data_ptr())
    assert e.value.status == E_ARG and "4096" in str(e.value)
    with pytest.raises(api.BceError) as e:
        rf.locate_edit_device(long_pat.data_ptr(), long_off.data_ptr(), 1, 1, d_hits.data_ptr(), None, None, None, 0)
    assert e.value.status == E_ARG
    long_off[1] = 4096                                                   # the bound itself is served
    torch.cuda.synchronize()
    rf.count_edit_device(long_pat.data_ptr(), long_off.data_ptr(), 1, 1, d_cnt[1:].data_ptr())
    assert d_cnt[1:3].cpu().tolist() == [0, 0]
    assert rf.locate_edit(pats[0], 1)[0].tolist() == ref.hits(text, pats[0], 1, False)[0].tolist()


def test_states_and_arguments_that_are_refused():
    text = bce_amd.synth_text(5, 20000)
    tb = text.tobytes()
    c = api._Ctx(0)
    try:
        lib, a = c.lib, C.addressof
        pat, off = (C.c_uint8 * 2)(*b"e "), (C.c_uint64 * 2)(0, 2)
        hits, cnt, total = (C.c_uint64 * 2)(7, 7), (C.c_uint64 * 3)(7, 7, 7), C.c_uint64(5)
        largs = (c.h, a(pat), a(off), 1, 1, LINEAR, a(hits), None, None, None, 0, C.byref(total))
        cargs = (c.h, a(pat), a(off), 1, 1, LINEAR, a(cnt))
        fns = ((lib.bce_hip_locate_edit, largs), (lib.bce_hip_locate_edit_device, largs), (lib.bce_hip_count_edit, cargs), (lib.bce_hip_count_edit_device, cargs))
        for fn, args in fns:                                             # no planes yet
            assert fn(*args) == E_STATE and b"holds no planes" in lib.bce_hip_last_error(c.h)

        def refused_arguments():
            for fn, args in fns:
                for k in (3, 4, 0xFFFFFFFF):                             # k, the flags and npat's cap are judged before the state
                    assert fn(*(args[:4] + (k,) + args[5:])) == E_ARG
                for flags in (2, 3, 0x80000000):
                    assert fn(*(args[:5] + (flags,) + args[6:])) == E_ARG
                for npat in (api.EDIT_MAX_PATTERNS + 1, 0xFFFFFFFF):     # before any offset is read
                    assert fn(*(args[:3] + (npat,) + args[4:])) == E_ARG

        refused_arguments()
        rf = api.RankFile(text, ctx=c)
        refused_arguments()
        assert list(hits) == [7, 7] and list(cnt) == [7, 7, 7]
        want = ref.hits(tb, b"e ", 1, False)
        got = rf.locate_edit(b"e ", 1)
        assert all(g.tolist() == w.tolist() for g, w in zip(got, want)) and len(want[0]) > 100
        for bad_k in (3, -1):
            with pytest.raises(ValueError):
                rf.count_edit(b"e ", bad_k)
            with pytest.raises(ValueError):
                rf.locate_edit(b"e ", bad_k)
        # m = 4097 with host buffers; 4096 is served
        big = np.full(4097, 101, dtype=np.uint8)
        boff = (C.c_uint64 * 2)(0, 4097)
        assert lib.bce_hip_count_edit(c.h, big.ctypes.data, a(boff), 1, 1, 0, a(cnt)) == E_ARG and b"4096" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_edit(c.h, big.ctypes.data, a(boff), 1, 1, 0, a(hits), None, None, None, 0, C.byref(total)) == E_ARG
        with pytest.raises(ValueError):
            rf.count_edit(big.tobytes(), 1)
        with pytest.raises(ValueError):
            rf.locate_edit(big.tobytes(), 1)
        assert rf.count_edit(big[:4096].tobytes(), 2).tolist() == [0, 0, 0]
        # decreasing offsets, null arrays
        bad = (C.c_uint64 * 3)(0, 2, 1)
        assert lib.bce_hip_count_edit(c.h, a(pat), a(bad), 2, 1, 0, a(cnt)) == E_ARG and b"offsets decrease" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_edit(c.h, a(pat), a(bad), 2, 1, 0, a(hits), None, None, None, 0, C.byref(total)) == E_ARG
        assert lib.bce_hip_count_edit(c.h, a(pat), a(off), 1, 1, 0, None) == E_ARG
        assert lib.bce_hip_count_edit(c.h, a(pat), None, 1, 1, 0, a(cnt)) == E_ARG
        assert lib.bce_hip_locate_edit(c.h, a(pat), a(off), 1, 1, 0, None, None, None, None, 0, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate_edit(c.h, a(pat), a(off), 1, 1, 0, a(hits), None, None, None, 4, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate_edit(c.h, a(pat), a(off), 1, 1, 0, a(hits), None, None, None, 0, None) == E_ARG
        # no patterns at all
        total.value, hits[0] = 5, 7
        assert lib.bce_hip_locate_edit(c.h, None, None, 0, 2, LINEAR, a(hits), None, None, None, 0, C.byref(total)) == 0 and total.value == 0 and hits[0] == 0
        assert lib.bce_hip_locate_edit_device(c.h, None, None, 0, 2, 0, None, None, None, None, 0, C.byref(total)) == 0
        assert lib.bce_hip_count_edit(c.h, None, None, 0, 2, 0, None) == 0 and lib.bce_hip_count_edit_device(c.h, None, None, 0, 2, 0, None) == 0
        assert rf.locate_edit([], 1) == [] and rf.count_edit([], 1).shape == (0, 2)
        # max_hits and limit: locate()'s rules
        with pytest.raises(ValueError, match=str(len(want[0]))):
            rf.locate_edit(b"e ", 1, max_hits=len(want[0]) - 1)
        pos, lens, dist = rf.locate_edit(b"e ", 1, limit=7)
        assert pos.tolist() == want[0][:7].tolist() and lens.tolist() == want[1][:7].tolist() and dist.tolist() == want[2][:7].tolist()
        # an injected BWT: planes, but no suffix array behind them -- neither positions nor counts
        bwt, row0 = count_ref.bwt_of_rotations(b"abracadabra")
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)
        assert rf.count_near(b"abra", 1, cyclic=True).sum() > 0
        for fn, args in fns:
            assert fn(*args) == E_STATE and b"no suffix array behind an injected BWT" in lib.bce_hip_last_error(c.h)
        for call in (rf.locate_edit, rf.count_edit):
            with pytest.raises(api.BceError) as e:
                call(b"abra", 1, cyclic=True)
            assert e.value.status == E_STATE
            with pytest.raises(ValueError):
                call(b"abra", 1)
    finally:
        c.close()


def test_the_queries_leave_the_compression_alone_and_outlive_it():
    text = bce_amd.synth_text(5, 50000)
    tb = text.tobytes()
    fresh = bytes(bce_amd.compress(text))
    c = api._Ctx(0)
    try:
        rf = api.RankFile(text, ctx=c)
        pats = [tb[i * 97:i * 97 + 4 + i % 12] for i in range(60)] + [tb[i * 89:i * 89 + 5] + tb[i * 89 + 6:i * 89 + 12] for i in range(40)]
        counts = rf.count_edit(pats, 2)
        assert counts.tolist() == [ref.counts(tb, p, 2, False).tolist() for p in pats]
        before = rf.locate_edit(pats, 1)
        assert bytes(api.BCE().encode(rf)) == fresh                     # queries, then encode: the archive of a fresh context
        assert np.array_equal(rf.count_edit(pats, 2), counts)           # and after it, on the planes it has read
        for b0, b1 in zip(before, rf.locate_edit(pats, 1)):
            assert all(np.array_equal(x, y) for x, y in zip(b0, b1))
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def _split(offsets, positions, lens, dists, dev):
    assert offsets.dtype == torch.int64 and positions.dtype == torch.int32 and lens.dtype == torch.int16 and dists.dtype == torch.uint8
    assert offsets.device == dev and positions.device == dev and lens.device == dev and dists.device == dev
    off = offsets.cpu().tolist()
    assert off[0] == 0 and off[-1] == positions.numel() == lens.numel() == dists.numel()
    pos, ln, dist = positions.cpu().tolist(), lens.cpu().tolist(), dists.cpu().tolist()
    return [(pos[a:b], ln[a:b], dist[a:b]) for a, b in zip(off, off[1:])]


def _want(text, pats, k, cyclic):
    return [tuple(v.tolist() for v in ref.hits(text, p, k, cyclic)) for p in pats]


def _want_counts(text, pats, k, cyclic):
    return [ref.counts(text, p, k, cyclic).tolist() for p in pats]


def test_module_level_and_tensor_functions_on_a_slice_at_an_odd_offset(ctx):
    data = bce_amd.synth_text(17, 9000)
    big = torch.from_numpy(data).to("cuda:0")
    t = big[1237:1237 + 4099]
    tb = data[1237:1237 + 4099].tobytes()
    assert t.data_ptr() % 2 == 1
    pats = [tb[:9], tb[-9:], tb[-4:] + tb[:5], tb[2000:2016] + tb[2017:2033], tb[300:310] + b"q" + tb[310:320], b"e", data[1230:1240].tobytes()]
    for k, cyclic in ((1, False), (2, True)):
        want = _want(tb, pats, k, cyclic)
        assert _split(*bce_amd.locate_edit_tensor(t, pats, k, cyclic=cyclic, ctx=ctx), t.device) == want
        assert bce_amd.count_edit_tensor(t, pats, k, cyclic=cyclic, ctx=ctx).tolist() == _want_counts(tb, pats, k, cyclic)
        got = bce_amd.locate_edit(tb, pats, k, cyclic=cyclic)
        assert [tuple(v.tolist() for v in g) for g in got] == want
        assert bce_amd.count_edit(tb, pats, k, cyclic=cyclic).tolist() == _want_counts(tb, pats, k, cyclic)
    assert (2000, 33, 1) in zip(*_want(tb, pats[3:4], 1, False)[0]) and (300, 20, 1) in zip(*_want(tb, pats[4:5], 1, False)[0])
    assert _split(*bce_amd.locate_edit_tensor(t, pats[3], 2), t.device) == _want(tb, pats[3:4], 2, False)     # a context of its own
    assert bce_amd.count_edit_tensor(t, pats[3], 2).tolist() == ref.counts(tb, pats[3], 2, False).tolist()
    off, pos, lens, dist = bce_amd.locate_edit_tensor(t, [b"\xff\xfe\xfd\xfc\xfb", b"\xfe\xfd\xfc\xfb\xfa"], 2, ctx=ctx)   # nothing found: empty tensors
    assert off.tolist() == [0, 0, 0] and pos.numel() == 0 and lens.numel() == 0 and dist.numel() == 0 and lens.dtype == torch.int16
    off, pos, lens, dist = bce_amd.locate_edit_tensor(t, [], 1, ctx=ctx)
    assert off.tolist() == [0] and pos.numel() == 0
    with pytest.raises(ValueError):
        bce_amd.locate_edit_tensor(t, b"", 1)
    with pytest.raises(ValueError):
        bce_amd.locate_edit_tensor(t, b"e", 3)
    with pytest.raises(ValueError):
        bce_amd.locate_edit_tensor(t, b"e" * 4097, 1)


def test_in_archive_on_a_plain_archive_and_across_a_block_boundary():
    data = bce_amd.synth_text(41, 10000).tobytes()
    dev = torch.device("cuda:0")
    plain = bytes(bce_amd.compress(data[:4000]))
    pats = [b"the", data[100:104] + data[105:109], data[3990:4000], data[3995:4000] + data[:3]]
    for cyclic in (False, True):
        assert _split(*bce_amd.locate_edit_in_archive(plain, pats, 1, cyclic=cyclic), dev) == _want(data[:4000], pats, 1, cyclic)
        assert bce_amd.count_edit_in_archive(plain, pats, 1, cyclic=cyclic).tolist() == _want_counts(data[:4000], pats, 1, cyclic)
    # a checked container of two blocks; patterns placed across the block boundary, a byte dropped and a byte doubled at it
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)
    table = container.block_table(blob)
    assert len(table) == 2 and all(e[3] is not None for e in table)
    cut = table[0][0]
    pats = [data[cut - 6:cut] + data[cut + 1:cut + 7], data[cut - 6:cut + 1] + data[cut:cut + 6], data[cut - 1:cut + 9], b"e", data[-5:] + data[:5]]
    want = _want(data, pats, 2, False)
    assert (cut - 6, 13, 1) in zip(*want[0]) and (cut - 6, 12, 1) in zip(*want[1]) and (cut - 1, 10, 0) in zip(*want[2])
    assert _split(*bce_amd.locate_edit_in_archive(blob, pats, 2), dev) == want
    assert bce_amd.count_edit_in_archive(blob, pats, 2).tolist() == _want_counts(data, pats, 2, False)
    assert bce_amd.count_edit_in_archive(blob, pats[0], 2).tolist() == ref.counts(data, pats[0], 2, False).tolist()
