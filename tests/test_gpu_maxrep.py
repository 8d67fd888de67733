"""GPU: the list of maximal repeats (kd_maxrep.hip through bce_hip_maximal_repeats / _maximal_repeats_device, RankFile.maximal_repeats /
maximal_repeats_device, maximal_repeats_tensor, maximal_repeats_in_archive) against a reference computed from the text alone
(tests/maxrep_ref.py): len, count, row, total, capped, bwt_runs and found exactly; pos is checked, never compared -- the cyclic cut of
the text there must be the bytes, and the index must count them `count` times.  The states and arguments that are refused, and that
nothing else in the context moves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import maxrep_ref as ref
import sa_ref
import top_ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
ORDERS = ("len", "count", "gain")
TEXT_NAMES = ("n1", "abracadabra", "mississippi", "abcXabc", "abab", "abra3", "a300", "ab2048", "abra200", "paste70000", "rand65536", "text100000")
KNOWN = {  # name: (max_len, (len, count, row) by length, BWT runs)
    "abracadabra": (64, [(4, 2, 1), (1, 5, 0)], 7),
    "mississippi": (64, [(4, 2, 2), (1, 4, 0), (1, 4, 7), (1, 2, 5)], 8),
    "abcXabc": (64, [(3, 2, 1)], 4),
    "abab": (64, [], 2),
    "abra3": (8, [(4, 6, 3), (1, 15, 0)], 7),
    "n1": (64, [], 1),
    "a300": (64, [], 1),
    "ab2048": (4096, [], 2),
}


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _text(name):
    fixed = {"n1": b"z", "abracadabra": b"abracadabra", "mississippi": b"mississippi", "abcXabc": b"abcXabc", "abab": b"abab",
             "abra3": b"abracadabra" * 3, "a300": b"a" * 300, "ab2048": b"ab" * 2048, "abra200": b"abracadabra" * 200}
    if name in fixed:
        return fixed[name]
    if name == "paste70000":                                              # a block of 5000 bytes twice: repeats at the bound, "4096+"
        body, block = bce_amd.synth_rand(21, 60000).tobytes(), bce_amd.synth_rand(22, 5000).tobytes()
        return body[:20000] + block + body[20000:45000] + block + body[45000:]
    if name.startswith("rand"):
        return bce_amd.synth_rand(3, int(name[4:])).tobytes()
    return bce_amd.synth_text(1, int(name[4:])).tobytes()


def _bound(name):
    return KNOWN[name][0] if name in KNOWN else 4096


@functools.lru_cache(maxsize=None)
def _arrays(name):
    """(lcp at the text's bound, bw) of the reference's own sort: computed once, shared by every order and least length."""
    text = _text(name)
    sa = ref.rotation_order(text)
    return ref.lcp_of_order(text, sa, _bound(name)), ref.bwt_of(text, sa)


@functools.lru_cache(maxsize=None)
def _all(name, order, min_len):
    """The whole list of (name, order, min_len) as (len, count, row): every limit's answer is a prefix of it."""
    lcp, bw = _arrays(name)
    ents, info = ref.of_arrays(lcp, np.zeros(len(lcp), dtype=np.int64), bw, min_len, _bound(name), order, 1 << 30)
    return [e[:3] for e in ents], info


def _check(name, order, min_len, limit, ents, strs, info, bytes_per):
    text = _text(name)
    want, winfo = _all(name, order, min_len)
    assert info == dict(winfo, found=min(limit, winfo["total"])), (name, order, min_len, limit, info, winfo)
    assert len(ents) == info["found"]
    got = [(int(e["len"]), int(e["count"]), int(e["row"])) for e in ents]
    if got != want[:len(got)]:
        e = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
        raise AssertionError((name, order, min_len, limit, e, got[e], want[e]))
    assert all(int(e["pos"]) < len(text) for e in ents)
    if bytes_per:
        ext = text * (bytes_per // len(text) + 2)
        for e, s in zip(ents, strs):                                         # the cyclic cut at pos
            assert s == ext[int(e["pos"]):int(e["pos"]) + min(int(e["len"]), bytes_per)], (name, order, e)
    else:
        assert strs is None


def test_the_reference_on_the_texts_whose_answer_is_known():
    for name, (L, want, runs) in KNOWN.items():
        assert _all(name, "len", 1) == (want, {"total": len(want), "capped": 0, "bwt_runs": runs, "found": len(want)}), name
    ents, info = _all("paste70000", "len", 1)
    assert info["capped"] == 1 and ents[0][:2] == (4096, 2) and ents[1][0] < 10       # the pasted block, then what random bytes repeat
    assert _all("abra200", "len", 1)[0] == [(4, 400, 200), (1, 1000, 0)]           # the eleven classes at the bound extend to the left
    assert _all("rand65536", "count", 1)[0][0][0] == 1 and _all("rand65536", "count", 1)[1]["total"] > 256


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_the_list_is_the_reference_list_for_every_order_length_and_limit(ctx, name):
    text = _text(name)
    L = _bound(name)
    rf = api.RankFile(text, ctx=ctx)
    longest = max([e[0] for e in _all(name, "len", 1)[0]] or [1])
    for order in ORDERS:
        for min_len in sorted(set((1, 2, longest, min(longest + 1, L)))):
            total = _all(name, order, min_len)[1]["total"]
            for limit in sorted(set(v for v in (1, 3, total, total + 1) if 1 <= v <= api.TOP_MAX)):
                per = 5 if limit > 2000 else 4096 if L == 4096 else 64
                ents, strs, info = rf.maximal_repeats(min_len=min_len, max_len=L, order=order, limit=limit, bytes_per=per)
                _check(name, order, min_len, limit, ents, strs, info, per)
    for per in (0, 5):
        ents, strs, info = rf.maximal_repeats(min_len=1, max_len=L, order="gain", limit=50, bytes_per=per)
        _check(name, "gain", 1, 50, ents, strs, info, per)
    assert info["bwt_runs"] == _independent_bwt_runs(text)
    # every uncapped entry's string occurs `count` times in the circular text
    ents, strs, info = rf.maximal_repeats(min_len=1, max_len=L, order="gain", limit=200, bytes_per=4096)
    pats = [s for e, s in zip(ents, strs) if e["len"] < L]
    if pats:
        assert rf.count(pats, cyclic=True).tolist() == [int(e["count"]) for e in ents if e["len"] < L], name


def _independent_bwt_runs(text):
    """The runs of the BWT from a sort that shares nothing with the reference's: the suffixes of the doubled text (rotations that
    are equal are preceded by equal bytes, so their order does not matter)."""
    n = len(text)
    if n <= 300:
        return ref.bwt_runs(np.frombuffer(count_ref.bwt_of_rotations(text)[0], dtype=np.uint8))
    sa = sa_ref.suffix_array(text + text)
    return ref.bwt_runs(ref.bwt_of(text, sa[sa < n]))


@pytest.mark.parametrize("name", ("n1", "abracadabra", "a300", "abra200", "paste70000", "text100000"))
def test_the_device_and_tensor_entry_points_give_the_same_list(ctx, name):
    text = _text(name)
    L = _bound(name)
    rf = api.RankFile(text, ctx=ctx)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    for order in ORDERS:
        for limit, per in ((7, 5), (300, 64)):
            host, hstr, hinfo = rf.maximal_repeats(min_len=1, max_len=L, order=order, limit=limit, bytes_per=per)
            ent = torch.full((limit * 4 + 2,), -5, dtype=torch.int32, device="cuda:0")    # guard words on both sides
            raw = torch.full((limit * per + 2,), 0xEE, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            info = rf.maximal_repeats_device(1, L, order, limit, ent[1:].data_ptr(), raw[1:].data_ptr(), per, limit * per)
            found = info["found"]
            e, b = ent.cpu().numpy(), raw.cpu().numpy()
            assert e[0] == -5 and (e[1 + 4 * found:] == -5).all() and b[0] == 0xEE and (b[1 + found * per:] == 0xEE).all(), (name, order, limit)
            assert info == hinfo and np.array_equal(e[1:1 + 4 * found].view(np.uint32), host.view(np.uint32).reshape(-1))   # pos included: one context, one sort
            slots = b[1:1 + found * per].reshape(found, per)
            for i, s in enumerate(hstr):                                     # the string, then zeros to the slot's end
                assert slots[i, :len(s)].tobytes() == s and not slots[i, len(s):].any()
            info2 = rf.maximal_repeats_device(1, L, order, limit, ent[1:].data_ptr())          # no bytes wanted
            assert info2 == hinfo
        ent, strs, info = bce_amd.maximal_repeats_tensor(t, 1, L, order, 1000, 16, ctx=ctx)
        assert ent.dtype == torch.int32 and ent.device == t.device and tuple(ent.shape) == (info["found"], 4) and tuple(strs.shape) == (info["found"], 16)
        e = np.ascontiguousarray(ent.cpu().numpy()).view(np.uint32)
        rec = np.zeros(len(e), dtype=api.MAXREP_DTYPE)
        for j, f in enumerate(api.MAXREP_DTYPE.names):
            rec[f] = e[:, j]
        s = strs.cpu().numpy()
        _check(name, order, 1, 1000, rec, [s[i, :min(int(rec[i]["len"]), 16)].tobytes() for i in range(len(rec))], info, 16)
    if 1 < len(text) <= 300:                                                  # a slice at an odd offset, a context of its own
        ent, strs, info = bce_amd.maximal_repeats_tensor(t[1:], 1, 64, "len", 5, 0)
        want, winfo = ref.of_text(text[1:], 1, 64, "len", 5)
        assert strs is None and info == winfo and [tuple(int(v) for v in row[:3]) for row in ent.cpu().numpy()] == want


def test_module_level_call_and_an_archive_as_one_text_and_block_by_block():
    data = bce_amd.synth_text(41, 10000).tobytes()
    want, winfo = ref.of_text(data, 3, 4096, "gain", 20)
    ents, strs, info = bce_amd.maximal_repeats(data, min_len=3, order="gain", limit=20, bytes_per=8)
    assert [(int(e["len"]), int(e["count"]), int(e["row"])) for e in ents] == want and info == winfo
    assert all(s == count_ref.cyclic_cut(data, int(e["pos"]), min(int(e["len"]), 8)) for e, s in zip(ents, strs))
    plain = bytes(bce_amd.compress(data[:4000]))
    ent, raw, info = bce_amd.maximal_repeats_in_archive(plain, 3, 4096, "gain", 20, 8)
    w4, i4 = ref.of_text(data[:4000], 3, 4096, "gain", 20)
    assert info == i4 and [tuple(int(v) for v in row[:3]) for row in ent.cpu().numpy()] == w4 and want != w4
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)                   # what `bce -C2` writes
    table = container.block_table(blob)
    assert len(table) == 2
    ent, raw, info = bce_amd.maximal_repeats_in_archive(blob, 3, 4096, "gain", 20, 8)      # one text: repeats across the blocks count
    assert info == winfo and [tuple(int(v) for v in row[:3]) for row in ent.cpu().numpy()] == want
    per = bce_amd.maximal_repeats_in_archive(blob, 3, 4096, "gain", 20, 8, per_block=True)
    assert len(per) == 2
    at = 0
    for (ent, raw, info), (size, _pos, _alen, _crc) in zip(per, table):     # every block a text of its own
        wb, ib = ref.of_text(data[at:at + size], 3, 4096, "gain", 20)
        assert info == ib and [tuple(int(v) for v in row[:3]) for row in ent.cpu().numpy()] == wb
        at += size
    assert at == len(data) and len(bce_amd.maximal_repeats_in_archive(plain, per_block=True)) == 1


# ---- states and refusals ----------------------------------------------------------------------------------------------------------

class _Outs:
    def __init__(self, limit=4, per=8):
        self.out = np.full(limit, 7, dtype=api.MAXREP_DTYPE)
        self.raw = np.full(limit * per, 9, dtype=np.uint8)
        self.info = api.MaxRepInfo(1, 2, 3, 4, 5)

    def untouched(self):
        i = self.info
        return ((self.out == np.full(len(self.out), 7, dtype=api.MAXREP_DTYPE)).all() and (self.raw == 9).all()
                and (i.total, i.capped, i.bwt_runs, i.found, i.reserved) == (1, 2, 3, 4, 5))


def _calls(c, o, min_len=1, max_len=64, order=0, limit=4, per=8, cap=32):
    lib = c.lib
    args = (min_len, max_len, order, limit, o.out.ctypes.data, o.raw.ctypes.data, per, cap, C.byref(o.info))
    return [lambda: lib.bce_hip_maximal_repeats(c.h, *args), lambda: lib.bce_hip_maximal_repeats_device(c.h, *args)]


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
            rf.maximal_repeats()
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
        for kw, word in ((dict(max_len=4097), b"4097"), (dict(max_len=0), b"bound"), (dict(min_len=0), b"least length"), (dict(min_len=65), b"least length"),
                         (dict(order=3), b"order"), (dict(limit=0), b"limit"), (dict(limit=(1 << 20) + 1), b"limit"), (dict(per=4097), b"4097"),
                         (dict(cap=31), b"31")):
            for call in _calls(c, o, **kw):                                # every refusal comes before a launch, with its words
                assert call() == E_ARG and word in lib.bce_hip_last_error(c.h), kw
        for fn in (lib.bce_hip_maximal_repeats, lib.bce_hip_maximal_repeats_device):
            assert fn(c.h, 1, 64, 0, 4, o.out.ctypes.data, o.raw.ctypes.data, 8, 32, None) == E_ARG                  # a null info
            assert fn(c.h, 1, 64, 0, 4, None, o.raw.ctypes.data, 8, 32, C.byref(o.info)) == E_ARG                    # a null out
        assert o.untouched()
        # bytes are optional; a cap is not looked at without them
        assert lib.bce_hip_maximal_repeats(c.h, 2, 64, 2, 4, o.out.ctypes.data, None, 8, 0, C.byref(o.info)) == 0
        want, winfo = ref.of_text(text.tobytes(), 2, 64, "gain", 4)
        assert [(int(e["len"]), int(e["count"]), int(e["row"])) for e in o.out] == want and (o.raw == 9).all()
        assert (o.info.total, o.info.capped, o.info.bwt_runs, o.info.found) == (winfo["total"], winfo["capped"], winfo["bwt_runs"], 4)
        for bad in (dict(max_len=4097), dict(limit=0), dict(min_len=0), dict(bytes_per=4097)):
            with pytest.raises(api.BceError):
                rf.maximal_repeats(**bad)
        with pytest.raises(ValueError):
            rf.maximal_repeats(order="size")
        with pytest.raises(api.BceError):
            bce_amd.maximal_repeats_tensor(torch.zeros(10, dtype=torch.uint8, device="cuda:0"), limit=(1 << 20) + 1)
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
    c = api._Ctx(0)
    try:
        rf = api.RankFile(text, ctx=c)
        pats = [tb[i * 97:i * 97 + 1 + i % 40] for i in range(200)]
        counts = rf.count(pats).tolist()
        top = rf.top_kgrams(6, 500)
        lpf = rf.lpf(64)
        first = rf.maximal_repeats(min_len=4, max_len=300, order="gain", limit=500, bytes_per=32)
        for order, min_len, max_len, limit in (("len", 1, 4096, 1 << 20), ("count", 2, 2, 3), ("gain", 300, 300, 1)):
            rf.maximal_repeats(min_len=min_len, max_len=max_len, order=order, limit=limit, bytes_per=0)
        # the calls, then encode: the archive of a fresh context; then the same answers on the arrays the encoder has read
        assert bytes(api.BCE().encode(rf)) == fresh
        again = rf.maximal_repeats(min_len=4, max_len=300, order="gain", limit=500, bytes_per=32)
        assert np.array_equal(again[0], first[0]) and again[1:] == first[1:]
        assert [(int(e["len"]), int(e["count"]), int(e["row"])) for e in first[0]] == ref.of_text(tb, 4, 300, "gain", 500)[0]
        assert rf.count(pats).tolist() == counts
        t2 = rf.top_kgrams(6, 500)
        assert [(e[0], e[2], e[3]) for e in t2] == [(e[0], e[2], e[3]) for e in top] and t2.size_hist == top.size_hist
        assert ([(cnt, row, g) for cnt, _, row, g in t2], t2.distinct, t2.size_hist) == top_ref.top_kgrams(tb, 6, 500)
        l2 = rf.lpf(64)
        assert all(np.array_equal(a, b) for a, b in zip(l2, lpf))                   # the trees are rebuilt by whoever needs them
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()
