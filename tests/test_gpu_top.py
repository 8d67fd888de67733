"""GPU: the list of the most frequent k-grams (kd_lcp.hip through bce_hip_top_kgrams / _top_kgrams_device, RankFile.top_kgrams /
top_kgrams_device, top_kgrams_tensor, top_kgrams_in_archive) against a reference computed from the text alone (tests/top_ref.py):
count, row, bytes, found, distinct and size_hist exactly; pos is checked, never compared -- its cyclic cut must be the bytes.  The
states and arguments that are refused, and that nothing else in the context moves."""
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
import top_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
KS = (0, 1, 2, 3, 8, 16, 300, 4096)
TEXT_NAMES = ("n1", "n2", "n9", "n257", "n2049", "n4097", "abracadabra", "a300", "ab150", "a5000rand", "text6144", "rand6144", "text100000", "seam")
SEAM_H = 250


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _text(name):
    """The texts of tests/test_gpu_repeat.py, rebuilt here."""
    fixed = {"abracadabra": b"abracadabra", "a300": b"a" * 300, "ab150": b"ab" * 150}
    if name in fixed:
        return fixed[name]
    if name == "a5000rand":                                               # one class across three scan blocks
        return b"a" * 5000 + bce_amd.synth_rand(3, 1144).tobytes()
    if name == "seam":                                                    # a repeat of 600 bytes, one copy across the text's end
        R, filler = bce_amd.synth_rand(13, 600).tobytes(), bce_amd.synth_rand(14, 1500).tobytes()
        return R[SEAM_H:] + filler + R + R[:SEAM_H]
    if name.startswith("rand"):
        return bce_amd.synth_rand(3, int(name[4:])).tobytes()
    n = int(name[1:] if name[0] == "n" else name[4:])
    return bce_amd.synth_text(n, n).tobytes()


def _ks(name):
    return tuple(k for k in KS if k <= (4096 if len(_text(name)) <= 12000 else 300))


@functools.lru_cache(maxsize=None)
def _all(name, k):
    """The whole list of (name, k): every limit's answer is a prefix of it."""
    return ref.top_kgrams(_text(name), k, 1 << 30)


def _limits(distinct):
    return sorted(set(v for v in (1, 2, distinct - 1, distinct, distinct + 1, 1000) if v >= 1))


def _check(name, k, limit, ents, distinct, hist, with_bytes=True):
    """ents: (count, pos, row, bytes or None) per entry."""
    text = _text(name)
    want, d, h = _all(name, k)
    assert (distinct, list(hist)) == (d, h), (name, k, limit)
    assert len(ents) == min(limit, d), (name, k, limit, len(ents))
    want = want[:len(ents)]
    if [(g[0], g[2]) for g in ents] != [(count, row) for count, row, _ in want]:
        e = next(i for i, (g, w) in enumerate(zip(ents, want)) if (g[0], g[2]) != w[:2])
        raise AssertionError((name, k, limit, e, ents[e][:3], want[e][:2]))
    ext = text * (k // len(text) + 2)
    assert all(g[1] < len(text) and ext[g[1]:g[1] + k] == w[2] for g, w in zip(ents, want)), (name, k, limit)   # the cyclic cut at pos
    assert count_ref.cyclic_cut(text, ents[0][1], k) == want[0][2]
    assert [g[3] for g in ents] == [w[2] if with_bytes else None for w in want], (name, k, limit)


def test_the_reference_on_the_texts_whose_answer_is_known():
    assert _all("abracadabra", 2)[0][:3] == [(2, 1, b"ab"), (2, 5, b"br"), (2, 9, b"ra")]
    assert _all("a300", 300) == ([(300, 0, b"a" * 300)], 1, [0] * 8 + [1] + [0] * 23)
    assert _all("ab150", 3)[0] == [(150, 0, b"aba"), (150, 150, b"bab")]           # the tie: `ab...` first
    first = _all("a5000rand", 300)[0][0]                                           # a class across three scan blocks
    assert (first[0], first[2]) == (5000 - 299, b"a" * 300) and first[1] + first[0] > 2 * 2048 > 2048 > first[1]
    assert _all("rand6144", 3)[1:] == (6142, [6140, 2] + [0] * 30)                 # two 3-grams of the random bytes occur twice ...
    ents, d, h = _all("rand6144", 8)                                               # ... from k = 8 on there is none
    assert d == 6144 and h == [6144] + [0] * 31 and [r for _, r, _ in ents] == list(range(6144))   # all singletons: the N lowest rows
    assert _all("n1", 16) == ([(1, 0, _text("n1") * 16)], 1, [1] + [0] * 31)


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_the_list_is_the_counted_one_for_every_k_and_limit(ctx, name):
    rf = api.RankFile(_text(name), ctx=ctx)
    for k in _ks(name):
        d = _all(name, k)[1]
        for limit in _limits(d):
            got = rf.top_kgrams(k, limit)
            assert isinstance(got, api.TopKGrams)
            _check(name, k, limit, got, got.distinct, got.size_hist)
        got = rf.top_kgrams(k, 2, with_bytes=False)
        _check(name, k, 2, got, got.distinct, got.size_hist, with_bytes=False)
        assert rf.kgrams(k).distinct == d and rf.kgrams(k).max_count == _all(name, k)[0][0][0]


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_the_device_and_tensor_entry_points_give_the_same_list(ctx, name):
    text = _text(name)
    rf = api.RankFile(text, ctx=ctx)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    for k in _ks(name):
        d = _all(name, k)[1]
        for limit in sorted(set((2, d))):
            ent = torch.full((limit * 3 + 2,), -5, dtype=torch.int32, device="cuda:0")    # guard words on both sides
            raw = torch.full((limit * k + 2,), 0xEE, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            found, distinct, hist = rf.top_kgrams_device(k, limit, ent[1:].data_ptr(), raw[1:].data_ptr(), limit * k)
            e, b = ent.cpu().numpy(), raw.cpu().numpy()
            assert e[0] == -5 and (e[1 + 3 * found:] == -5).all() and b[0] == 0xEE and (b[1 + found * k:] == 0xEE).all(), (name, k, limit)
            e = e[1:1 + 3 * found].astype(np.uint32).reshape(found, 3)
            ents = [(int(e[i, 0]), int(e[i, 2]), int(e[i, 1]), b[1 + i * k:1 + (i + 1) * k].tobytes()) for i in range(found)]
            _check(name, k, limit, ents, distinct, hist)
        found, distinct, hist = rf.top_kgrams_device(k, 3, ent[1:].data_ptr())              # no bytes wanted
        assert (found, distinct, hist) == (min(3, d), d, _all(name, k)[2])
        ent, grams, distinct, hist = bce_amd.top_kgrams_tensor(t, k, 1000, ctx=ctx)
        assert ent.dtype == torch.int32 and ent.device == t.device and grams.dtype == torch.uint8 and tuple(grams.shape) == (ent.shape[0], k)
        e, g = ent.cpu().numpy().astype(np.uint32), grams.cpu().numpy()
        _check(name, k, 1000, [(int(e[i, 0]), int(e[i, 2]), int(e[i, 1]), g[i].tobytes()) for i in range(len(e))], distinct, hist)
    if len(text) <= 300:
        cut = text[1:] if len(text) > 1 else text                          # a slice at an odd offset, a context of its own
        ent, grams, distinct, hist = bce_amd.top_kgrams_tensor(t[1:] if len(text) > 1 else t, 2, 5, with_bytes=False)
        want, d, h = ref.top_kgrams(cut, 2, 5)
        assert grams is None and (distinct, hist) == (d, h) and [(int(a), int(b)) for a, b, _ in ent.cpu().numpy()] == [(c, r) for c, r, _ in want]


def test_module_level_call_and_the_round_trip_through_an_archive():
    data = bce_amd.synth_text(41, 10000).tobytes()
    want, d, h = ref.top_kgrams(data, 4, 20)
    got = bce_amd.top_kgrams(data, 4, 20)
    assert [(c, r, g) for c, _, r, g in got] == want and (got.distinct, got.size_hist) == (d, h)
    plain = bytes(bce_amd.compress(data[:4000]))
    ent, grams, distinct, hist = bce_amd.top_kgrams_in_archive(plain, 4, 20)
    w4, d4, h4 = ref.top_kgrams(data[:4000], 4, 20)
    assert (distinct, hist) == (d4, h4) and [(int(a), int(b)) for a, b, _ in ent.cpu().numpy()] == [(c, r) for c, r, _ in w4]
    assert [bytes(g) for g in grams.cpu().numpy()] == [g for _, _, g in w4]
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)                   # what `bce -C2` writes
    assert len(container.block_table(blob)) == 2 and all(e[3] is not None for e in container.block_table(blob))
    ent, grams, distinct, hist = bce_amd.top_kgrams_in_archive(blob, 4, 20)
    assert (distinct, hist) == (d, h) and [(int(a), int(b)) for a, b, _ in ent.cpu().numpy()] == [(c, r) for c, r, _ in want] and want != w4
    assert [bytes(g) for g in grams.cpu().numpy()] == [g for _, _, g in want]


# ---- states and refusals ----------------------------------------------------------------------------------------------------------

class _Outs:
    def __init__(self, limit=4, k=8):
        self.out, self.raw = (api.TopKGram * limit)(), (C.c_uint8 * (limit * k))(*([9] * (limit * k)))
        for e in self.out:
            e.count, e.row, e.pos = 11, 12, 13
        self.found, self.distinct, self.hist = C.c_uint32(5), C.c_uint64(6), (C.c_uint64 * 32)(*([7] * 32))
        self.tail = (C.byref(self.found), C.byref(self.distinct), C.addressof(self.hist))

    def untouched(self):
        return (all((e.count, e.row, e.pos) == (11, 12, 13) for e in self.out) and set(self.raw) == {9}
                and (self.found.value, self.distinct.value, list(self.hist)) == (5, 6, [7] * 32))


def _calls(c, o, k=8, limit=4, cap=32):
    lib = c.lib
    return [lambda: lib.bce_hip_top_kgrams(c.h, k, limit, C.addressof(o.out), C.addressof(o.raw), cap, *o.tail),
            lambda: lib.bce_hip_top_kgrams_device(c.h, k, limit, C.addressof(o.out), C.addressof(o.raw), cap, *o.tail)]


def test_injected_bwt_and_missing_planes_are_refused_in_the_kgrams_words():
    text = b"abracadabra" * 9 + b"x"
    bwt, row0 = count_ref.bwt_of_rotations(text)
    o = _Outs()
    c = api._Ctx(0)
    try:
        for call in _calls(c, o):
            assert call() == E_STATE and b"holds no planes" in c.lib.bce_hip_last_error(c.h)
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)
        for call in _calls(c, o):
            assert call() == E_STATE and b"no suffix array behind an injected BWT" in c.lib.bce_hip_last_error(c.h)
        with pytest.raises(api.BceError) as e:
            rf.top_kgrams(2, 3)
        assert e.value.status == E_STATE and o.untouched()
    finally:
        c.close()


def test_refused_arguments_and_states_leave_the_outputs_untouched():
    text = bce_amd.synth_text(5, 20000)
    o = _Outs()
    c = api._Ctx(0)
    try:
        lib = c.lib
        api.RankFile(text, ctx=c, build=False)                            # loaded, K1 done, no planes yet
        for call in _calls(c, o):
            assert call() == E_STATE
        rf = api.RankFile(text, ctx=c)
        for kw, word in ((dict(k=4097), b"4097"), (dict(limit=0), b"limit"), (dict(limit=(1 << 20) + 1), b"limit"), (dict(cap=31), b"31")):
            for call in _calls(c, o, **kw):                                # every refusal comes before a launch, with its words
                assert call() == E_ARG and word in lib.bce_hip_last_error(c.h), kw
        for fn in (lib.bce_hip_top_kgrams, lib.bce_hip_top_kgrams_device):
            assert fn(c.h, 8, 4, C.addressof(o.out), C.addressof(o.raw), 32, None, C.byref(o.distinct), C.addressof(o.hist)) == E_ARG   # a null found
            assert fn(c.h, 8, 4, None, C.addressof(o.raw), 32, *o.tail) == E_ARG                                                        # a null out
            assert fn(c.h, 4097, 4, None, None, 0, *o.tail) == E_ARG
        assert o.untouched()
        # bytes, distinct and size_hist are optional; a cap is not looked at without bytes
        assert lib.bce_hip_top_kgrams(c.h, 8, 4, C.addressof(o.out), None, 0, C.byref(o.found), None, None) == 0
        assert o.found.value == 4 and o.distinct.value == 6 and set(o.raw) == {9} and list(o.hist) == [7] * 32
        assert [(e.count, e.row) for e in o.out] == [(cnt, row) for cnt, row, _ in ref.top_kgrams(text.tobytes(), 8, 4)[0]]
        with pytest.raises(api.BceError):
            rf.top_kgrams(4097, 1)
        with pytest.raises(api.BceError):
            rf.top_kgrams(2, 0)
        with pytest.raises(api.BceError):
            bce_amd.top_kgrams_tensor(torch.zeros(10, dtype=torch.uint8, device="cuda:0"), 2, (1 << 20) + 1)
        # a decode takes the planes, the suffix array and the text away
        fresh = bytes(bce_amd.compress(text))
        assert bce_amd.decompress_device(fresh, ctx=c) == text.tobytes()
        o = _Outs()
        for call in _calls(c, o):
            assert call() == E_STATE
        assert o.untouched()
    finally:
        c.close()


# ---- nothing else moves ---------------------------------------------------------------------------------------------------------

def test_the_call_leaves_the_compression_and_the_other_queries_alone():
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
        recs = [g.as_dict() for g in rf.kgrams(range(34))]
        want = ref.top_kgrams(tb, 6, 500)
        for k, limit in ((6, 500), (1, 300), (300, 1 << 20), (0, 1)):
            got = rf.top_kgrams(k, limit)
            assert got.distinct == recs[k]["distinct"] if k < 34 else True
        got = rf.top_kgrams(6, 500)
        assert ([(cnt, row, g) for cnt, _, row, g in got], got.distinct, got.size_hist) == want
        # the calls, then encode: the archive of a fresh context; then the same answers on the arrays the encoder has read
        assert bytes(api.BCE().encode(rf)) == fresh
        again = rf.top_kgrams(6, 500)
        assert [(e[0], e[2], e[3]) for e in again] == [(e[0], e[2], e[3]) for e in got] and again.size_hist == got.size_hist
        assert [g.as_dict() for g in rf.kgrams(range(34))] == recs
        assert rf.count(pats).tolist() == counts
        for x, y in zip(rf.locate(pats), hits):
            assert np.array_equal(x, y)
        assert [h.tolist() for h in hits[:20]] == [locate_ref.linear_hits(tb, p) for p in pats[:20]]
        lens2, pos2 = rf.match(query, 300)
        assert np.array_equal(lens2, lens) and np.array_equal(lens, match_ref.match_lens(tb, query, 300))
        match_ref.check_positions(tb, query, lens2, pos2, False)
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()
