"""GPU: what the indexed text holds by itself (kd_lcp.hip through bce_hip_lcp / _lcp_device, bce_hip_kgrams, bce_hip_longest_repeat,
RankFile.lcp / kgrams / entropy_profile / longest_repeat, lcp_tensor, entropy_profile_in_archive) against references computed from
the text alone (tests/repeat_ref.py): the capped LCP array exactly, the k-gram records exactly (max_pos checked, never compared),
the entropy profile, the longest repeat, the states and arguments that are refused, and that nothing else in the context moves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import locate_ref
import match_ref
import repeat_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
NONE = 0xFFFFFFFF
BOUNDS = (1, 16, 300, 4096)
KS = (0, 1, 2, 3, 8, 16, 300, 4096)
SYNTH = (1, 2, 3, 7, 8, 9,                    # the eight-byte word against the wrap
         63, 64, 65, 255, 256, 257,           # wave and workgroup edges
         2047, 2048, 2049, 4097)              # scan-block edges
TEXT_NAMES = tuple("n%d" % n for n in SYNTH) + ("abracadabra", "a300", "ab150", "a5000rand", "text6144", "rand6144", "text100000", "planted", "seam")
SEAM_H = 250


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def log2q(c):
    return api.cost_q24(1, c)


@functools.lru_cache(maxsize=None)
def _text(name):
    fixed = {"abracadabra": b"abracadabra", "a300": b"a" * 300, "ab150": b"ab" * 150}
    if name in fixed:
        return fixed[name]
    if name == "a5000rand":                                               # one class across three scan blocks
        return b"a" * 5000 + bce_amd.synth_rand(3, 1144).tobytes()
    if name == "planted":                                                 # a piece of 5000 bytes twice: the repeat passes the bound
        r, piece = bce_amd.synth_rand(11, 2000).tobytes(), bce_amd.synth_rand(12, 5000).tobytes()
        return r[:1000] + piece + r[1000:] + piece
    if name == "seam":                                                    # a repeat of 600 bytes, one copy across the text's end
        R, filler = bce_amd.synth_rand(13, 600).tobytes(), bce_amd.synth_rand(14, 1500).tobytes()
        return R[SEAM_H:] + filler + R + R[:SEAM_H]
    if name.startswith("rand"):
        return bce_amd.synth_rand(3, int(name[4:])).tobytes()
    n = int(name[1:] if name[0] == "n" else name[4:])
    return bce_amd.synth_text(n, n).tobytes()


def _top(name):
    """The largest bound (and k) this text is asked with: the reference sorts n windows of that many bytes."""
    return 4096 if len(_text(name)) <= 12000 else 300


def _bounds(name):
    return tuple(b for b in BOUNDS if b <= _top(name))


@functools.lru_cache(maxsize=None)
def _full(name):
    out = ref.capped_lcp(_text(name), _top(name))
    out.setflags(write=False)
    return out


def _want(name, bound):
    """The capped array under `bound`: rows sorted by their first 4096 bytes are sorted by their first `bound` too, and the array
    does not depend on the order of ties, so it is the array of the largest bound cut at this one."""
    return np.minimum(_full(name), bound)


@functools.lru_cache(maxsize=None)
def _record(name, k):
    return ref.kgram_record(_text(name), k, log2q)


def _check_record(name, k, g):
    text = _text(name)
    assert (g.distinct, g.once, g.nlogn_q24, g.max_count) == _record(name, k), (name, k, g)
    assert g.max_pos < len(text)
    assert count_ref.cyclic_count(text, count_ref.cyclic_cut(text, g.max_pos, k)) == g.max_count, (name, k, g)


def test_the_reference_cut_at_a_bound_is_the_reference_under_that_bound():
    for name in ("abracadabra", "ab150", "n257", "seam"):
        for bound in (1, 16, 300):
            assert np.array_equal(ref.capped_lcp(_text(name), bound), _want(name, bound)), (name, bound)
    assert _full("a300").tolist() == [0] + [4096] * 299 and _full("ab150").tolist() == [0] + [4096] * 149 + [0] + [4096] * 149
    assert int(_full("planted").max()) == 4096 and 600 <= int(_full("seam").max()) < 620


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_lcp_is_the_capped_lcp_of_the_text_through_every_entry_point(ctx, name):
    text = _text(name)
    n = len(text)
    rf = api.RankFile(text, ctx=ctx)
    for bound in _bounds(name):
        want = _want(name, bound)
        got = rf.lcp(bound)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (name, bound, np.flatnonzero(got != want)[:5])
        buf = torch.full((n + 2,), -5, dtype=torch.int32, device="cuda:0")    # guard words on both sides
        torch.cuda.synchronize()
        rf.lcp_device(bound, buf[1:].data_ptr())
        got = buf.cpu().numpy()
        assert got[0] == -5 and got[-1] == -5 and np.array_equal(got[1:-1].astype(np.uint32), want), (name, bound)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    bound = _bounds(name)[-2]
    out = bce_amd.lcp_tensor(t, bound, ctx=ctx)
    assert out.dtype == torch.int32 and out.device == t.device and np.array_equal(out.cpu().numpy().astype(np.uint32), _want(name, bound))
    if n <= 300:
        out = bce_amd.lcp_tensor(t[1:] if n > 1 else t, 16)                 # a slice at an odd offset, a context of its own
        assert np.array_equal(out.cpu().numpy().astype(np.uint32), ref.capped_lcp(text[1:] if n > 1 else text, 16))


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_kgram_records_are_the_counted_ones(ctx, name):
    text = _text(name)
    rf = api.RankFile(text, ctx=ctx)
    ks = [k for k in KS if k <= _top(name)]
    recs = rf.kgrams(ks)
    assert len(recs) == len(ks)
    for k, g in zip(ks, recs):
        _check_record(name, k, g)
    one = rf.kgrams(ks[-1])                                               # one k: one record, its own pass
    assert isinstance(one, api.KGram) and one.as_dict() == {**recs[-1].as_dict(), "max_pos": one.max_pos}
    g = rf.kgrams(0)
    assert (g.distinct, g.once, g.max_count) == (1, int(len(text) == 1), len(text)) and g.nlogn_q24 == len(text) * log2q(len(text))
    if name == "a300":                                                    # every row tied: one class of n for every k
        assert all((r.distinct, r.once, r.max_count) == (1, 0, 300) for r in recs)
    if name == "a5000rand":                                               # the run of equal bytes: one class over three scan blocks
        assert rf.kgrams(300).max_count == 5000 - 299


@pytest.mark.parametrize("name", ("n1", "n9", "n257", "abracadabra", "ab150", "a5000rand", "text6144", "seam"))
def test_all_64_ks_in_one_call_and_the_entropy_profile(ctx, name):
    text = _text(name)
    n = len(text)
    rf = api.RankFile(text, ctx=ctx)
    recs = rf.kgrams(range(64))
    assert len(recs) == 64
    for k, g in enumerate(recs):
        _check_record(name, k, g)
    mixed = rf.kgrams([5, 0, 63, 5, 1])                                   # any order, repeats
    assert [(g.distinct, g.nlogn_q24) for g in mixed] == [(recs[k].distinct, recs[k].nlogn_q24) for k in (5, 0, 63, 5, 1)]
    prof = rf.entropy_profile(62)
    assert len(prof) == 63
    for k, h in enumerate(prof):
        assert h == ref.entropy_q24(n, _record(name, k)[2], _record(name, k + 1)[2])
    for k in (0, 1, 2, 3, 8):                                             # 2^-20: tests/test_repeat_cpu.py derives it
        assert abs(prof[k] - ref.entropy_float(text, k)) <= 2.0 ** -20, (name, k)
    assert rf.entropy_profile(0) == prof[:1] and rf.entropy_profile(3) == prof[:4]
    with pytest.raises(ValueError):
        rf.entropy_profile(63)
    if name == "abracadabra":
        assert bce_amd.entropy_profile(text, 3) == prof[:4] and bce_amd.kgrams(text, 2).distinct == 8
        t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
        assert bce_amd.entropy_profile_tensor(t, 3) == prof[:4] and bce_amd.kgrams_tensor(t, [2])[0].distinct == 8


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_longest_repeat_is_the_largest_lcp_and_its_rotations_agree(ctx, name):
    text = _text(name)
    n = len(text)
    rf = api.RankFile(text, ctx=ctx)
    for bound in _bounds(name):
        want = int(_want(name, bound).max())
        ln, a, b = rf.longest_repeat(bound)
        assert ln == want, (name, bound)
        if ln == 0:
            assert (a, b) == (NONE, NONE)
            continue
        assert a < n and b < n and a != b
        # the two rotations agree on exactly that many bytes -- or on at least the bound, where the length is the bound
        assert ref.rot_lcp(text, a, b, bound) == ln, (name, bound, ln, a, b)
    if _top(name) == 4096:
        assert rf.longest_repeat() == rf.longest_repeat(4096)
    if name == "n1":
        assert rf.longest_repeat() == (0, NONE, NONE)
    if name == "planted":
        assert rf.longest_repeat()[0] == min(5000, 4096) and bce_amd.longest_repeat(text)[0] == 4096
    if name == "seam":
        ln, a, b = rf.longest_repeat()
        assert ln >= 600 and max(a, b) + ln > n                          # one of the two copies runs across the text's end


def test_entropy_profile_in_archive_plain_and_checked_container():
    data = bce_amd.synth_text(41, 10000).tobytes()
    plain = bytes(bce_amd.compress(data[:4000]))
    want = [ref.entropy_q24(4000, ref.kgram_record(data[:4000], k, log2q)[2], ref.kgram_record(data[:4000], k + 1, log2q)[2]) for k in range(5)]
    assert bce_amd.entropy_profile_in_archive(plain, 4) == want
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)                   # what `bce -C2` writes
    assert len(container.block_table(blob)) == 2 and all(e[3] is not None for e in container.block_table(blob))
    whole = [ref.entropy_q24(10000, ref.kgram_record(data, k, log2q)[2], ref.kgram_record(data, k + 1, log2q)[2]) for k in range(5)]
    assert bce_amd.entropy_profile_in_archive(blob, 4) == whole and whole != want


# ---- states and refusals ----------------------------------------------------------------------------------------------------------

def _calls(c, lcp, ks, recs, ln, a, b, max_len=16, nk=3):
    lib = c.lib
    return [lambda: lib.bce_hip_lcp(c.h, max_len, lcp.ctypes.data),
            lambda: lib.bce_hip_lcp_device(c.h, max_len, lcp.ctypes.data),
            lambda: lib.bce_hip_kgrams(c.h, ks.ctypes.data, nk, C.addressof(recs)),
            lambda: lib.bce_hip_longest_repeat(c.h, max_len, C.byref(ln), C.byref(a), C.byref(b))]


def test_injected_bwt_and_missing_planes_are_refused_in_the_locates_words():
    text = b"abracadabra" * 9 + b"x"
    bwt, row0 = count_ref.bwt_of_rotations(text)
    lcp, ks, recs = np.full(len(text), 7, dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint32), (api.KGram * 3)()
    ln, a, b = C.c_uint32(5), C.c_uint32(6), C.c_uint32(7)
    c = api._Ctx(0)
    try:
        for call in _calls(c, lcp, ks, recs, ln, a, b):
            assert call() == E_STATE and b"holds no planes" in c.lib.bce_hip_last_error(c.h)
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)
        for call in _calls(c, lcp, ks, recs, ln, a, b):
            assert call() == E_STATE and b"no suffix array behind an injected BWT" in c.lib.bce_hip_last_error(c.h)
        for use in (lambda: rf.lcp(16), lambda: rf.kgrams(2), lambda: rf.entropy_profile(2), lambda: rf.longest_repeat()):
            with pytest.raises(api.BceError) as e:
                use()
            assert e.value.status == E_STATE
        assert (lcp == 7).all() and (ln.value, a.value, b.value) == (5, 6, 7) and all(r.distinct == 0 for r in recs)
    finally:
        c.close()


def test_refused_arguments_and_states():
    text = bce_amd.synth_text(5, 20000)
    lcp, recs = np.full(20000, 7, dtype=np.uint32), (api.KGram * 65)()
    ks, bad = np.arange(65, dtype=np.uint32), np.array([0, 4097, 1], dtype=np.uint32)
    ln, a, b = C.c_uint32(5), C.c_uint32(6), C.c_uint32(7)
    c = api._Ctx(0)
    try:
        lib = c.lib
        api.RankFile(text, ctx=c, build=False)                            # loaded, K1 done, no planes yet
        for call in _calls(c, lcp, ks, recs, ln, a, b):
            assert call() == E_STATE
        rf = api.RankFile(text, ctx=c)
        for max_len in (0, 4097, 0xFFFFFFFF):                             # every refusal comes before a launch
            for call in _calls(c, lcp, ks, recs, ln, a, b, max_len=max_len)[:2] + _calls(c, lcp, ks, recs, ln, a, b, max_len=max_len)[3:]:
                assert call() == E_ARG
        assert lib.bce_hip_kgrams(c.h, bad.ctypes.data, 3, C.addressof(recs)) == E_ARG and b"4097" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_kgrams(c.h, ks.ctypes.data, 65, C.addressof(recs)) == E_ARG
        assert lib.bce_hip_kgrams(c.h, None, 3, C.addressof(recs)) == E_ARG
        assert lib.bce_hip_kgrams(c.h, ks.ctypes.data, 3, None) == E_ARG
        assert lib.bce_hip_kgrams(c.h, None, 0, None) == 0                # no k: nothing to do
        assert lib.bce_hip_lcp(c.h, 16, None) == E_ARG and lib.bce_hip_lcp_device(c.h, 16, None) == E_ARG
        for args in ((None, C.byref(a), C.byref(b)), (C.byref(ln), None, C.byref(b)), (C.byref(ln), C.byref(a), None)):
            assert lib.bce_hip_longest_repeat(c.h, 16, *args) == E_ARG
        assert (lcp == 7).all() and (ln.value, a.value, b.value) == (5, 6, 7) and all(r.distinct == 0 and r.max_count == 0 for r in recs)
        with pytest.raises(api.BceError):
            rf.lcp(0)
        with pytest.raises(api.BceError):
            rf.kgrams(4097)
        assert rf.kgrams([]) == []
        assert rf.kgrams(range(64))[63].distinct == ref.kgram_record(text.tobytes(), 63, log2q)[0]
        # a decode takes the planes, the suffix array and the text away
        fresh = bytes(bce_amd.compress(text))
        assert bce_amd.decompress_device(fresh, ctx=c) == text.tobytes()
        for call in _calls(c, lcp, ks, recs, ln, a, b):
            assert call() == E_STATE
        assert (lcp == 7).all()
    finally:
        c.close()


# ---- nothing else moves ---------------------------------------------------------------------------------------------------------

def test_the_calls_leave_the_compression_the_count_the_locate_and_the_match_alone():
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
        pats = [tb[i * 97:i * 97 + 1 + i % 40] for i in range(200)]
        counts = rf.count(pats).tolist()
        hits = rf.locate(pats)
        lens, pos = rf.match(query, 300)
        want = ref.capped_lcp(tb, 300)
        assert np.array_equal(rf.lcp(300), want)
        recs = rf.kgrams(range(34))
        rep = rf.longest_repeat()
        assert rep[0] == int(rf.lcp(4096).max()) >= int(want.max())
        crc = C.c_uint32(0)
        assert c.lib.bce_hip_input_crc32(c.h, C.byref(crc)) == 0 and crc.value == bce_amd.crc32(tb)
        # the calls, then encode: the archive of a fresh context; then the same answers on the arrays the encoder has read
        assert bytes(api.BCE().encode(rf)) == fresh
        assert np.array_equal(rf.lcp(300), want) and rf.longest_repeat() == rep
        assert [g.as_dict() for g in rf.kgrams(range(34))] == [g.as_dict() for g in recs]
        assert rf.count(pats).tolist() == counts
        for x, y in zip(rf.locate(pats), hits):
            assert np.array_equal(x, y)
        assert [h.tolist() for h in hits[:20]] == [locate_ref.linear_hits(tb, p) for p in pats[:20]]
        again, pos2 = rf.match(query, 300)
        assert np.array_equal(again, lens) and np.array_equal(lens, match_ref.match_lens(tb, query, 300))
        match_ref.check_positions(tb, query, again, pos2, False)
        assert c.lib.bce_hip_input_crc32(c.h, C.byref(crc)) == 0 and crc.value == bce_amd.crc32(tb)
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()
