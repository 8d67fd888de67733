"""GPU: the matching statistics of a second buffer against the indexed text (kd_match.hip through bce_hip_match / _match_device,
bce_hip_coverage / _coverage_device, RankFile.match / coverage, match, coverage, match_tensor, coverage_tensor, coverage_in_archive)
against brute-force scans of the same text in Python (tests/match_ref.py): the lengths in both modes, every position checked (never
compared: which occurrence is reported is not specified), the coverage, the states and arguments that are refused, and that nothing
else in the context moves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref
import locate_ref
import match_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
LINEAR = 1
NONE = 0xFFFFFFFF
BOUNDS = (1, 16, 300, 4096)
Q_SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 2049)      # wave (64), workgroup (256) and scan-block (2048) edges
# the granule holds 96 positions and n + 1 are laid out: n = 95, 96, 97, 191, 192, 193 stand on both sides of its edges
TEXT_NAMES = ("n1", "n2", "n95", "n96", "n97", "n191", "n192", "n193", "abracadabra", "a300", "ab150", "text6144", "rand6144", "text100000")


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _text(name):
    fixed = {"abracadabra": b"abracadabra", "a300": b"a" * 300, "ab150": b"ab" * 150}
    if name in fixed:
        return fixed[name]
    if name.startswith("rand"):
        return bce_amd.synth_rand(3, int(name[4:])).tobytes()
    n = int(name[1:] if name[0] == "n" else name[4:])
    return bce_amd.synth_text(n, n).tobytes()


@functools.lru_cache(maxsize=None)
def _queries(name):
    """Pieces of every size in Q_SIZES cut from the circular text, a byte spoiled every 40 bytes or so; the text's end followed by
    its beginning (for a short or periodic text: the whole text, then its beginning); zeros, which only the random text holds; the text."""
    text = _text(name)
    n = len(text)
    rs = np.random.RandomState(n)
    qs = []
    for q in Q_SIZES:
        piece = bytearray(count_ref.cyclic_cut(text, int(rs.randint(0, n)), q))
        for at in range(int(rs.randint(0, 40)), q, 40):
            piece[at] ^= 0x80
        qs.append(bytes(piece))
    wrap = text + text[:min(n, 5)] if n <= 300 else text[-8:] + text[:8]
    qs += [wrap, b"\x00" * 100, text if n <= 6144 else text[:500]]
    return qs, len(Q_SIZES)                                               # (the queries, the index of the wrap query)


@functools.lru_cache(maxsize=None)
def _full(name, k, cyclic):
    """The reference's lengths of query k under the largest bound this text is asked with (4096 up to 6144 bytes, else 300: the
    brute force stays short), computed once."""
    text = _text(name)
    out = ref.match_lens(text, _queries(name)[0][k], 4096 if len(text) <= 6144 else 300, cyclic)
    out.setflags(write=False)
    return out


def _want(name, k, cyclic, bound):
    """match_ref's lengths under `bound`: the largest l <= min(bound, i + 1) that occurs.  "Occurs" is monotone in l (match_ref
    bisects on that), so this is the full length cut at the bound."""
    return np.minimum(_full(name, k, cyclic), bound)


def _bounds(name):
    return BOUNDS if len(_text(name)) <= 6144 else BOUNDS[:3]


def test_the_reference_cut_at_a_bound_is_the_reference_under_that_bound():
    for name in ("abracadabra", "ab150", "n97"):
        for k in (3, len(Q_SIZES), len(Q_SIZES) + 2):
            for cyclic in (False, True):
                for bound in (1, 16, 300):
                    assert np.array_equal(ref.match_lens(_text(name), _queries(name)[0][k], bound, cyclic), _want(name, k, cyclic, bound))


@pytest.mark.parametrize("name", TEXT_NAMES)
def test_lengths_and_positions_are_the_brute_force_ones(ctx, name):
    text = _text(name)
    qs, wrap = _queries(name)
    top = _bounds(name)[-1]
    assert not np.array_equal(_want(name, wrap, True, top), _want(name, wrap, False, top))      # across the end: the modes differ
    rf = api.RankFile(text, ctx=ctx)
    for k, q in enumerate(qs):
        for cyclic in (False, True):
            for bound in _bounds(name):
                lens, pos = rf.match(q, bound, cyclic=cyclic)
                assert lens.dtype == np.uint32 and pos.dtype == np.uint32
                assert np.array_equal(lens, _want(name, k, cyclic, bound)), (name, k, cyclic, bound)
                assert np.array_equal(pos == NONE, lens == 0)
                ref.check_positions(text, q, lens, pos, cyclic)
                only, none = rf.match(q, bound, cyclic=cyclic, positions=False)                  # pos_out == NULL: the same lengths
                assert none is None and np.array_equal(only, lens)
    if len(text) <= 6144:                                                 # the text against itself: everything up to the bound
        lens, pos = rf.match(text, 4096)
        assert lens.tolist() == [min(4096, i + 1) for i in range(len(text))]
    if 0 not in text:                                                     # (the random text holds every byte value)
        lens, pos = rf.match(b"\x00" * 100, 16)
        assert not lens.any() and (pos == NONE).all()


@pytest.mark.parametrize("name", ("n1", "n97", "ab150", "text6144"))
def test_host_and_device_entry_points_agree(ctx, name):
    text = _text(name)
    qs, _ = _queries(name)
    rf = api.RankFile(text, ctx=ctx)
    dev = "cuda:0"
    for k in (0, 3, 8, len(Q_SIZES)):
        q = qs[k]
        buf = torch.zeros(len(q) + 7, dtype=torch.uint8, device=dev)
        buf[3:3 + len(q)] = torch.from_numpy(np.frombuffer(q, dtype=np.uint8).copy()).to(dev)
        d_q = buf[3:3 + len(q)]                                           # a slice at an odd offset; guard words around the outputs
        assert d_q.data_ptr() % 2 == 1
        for cyclic in (False, True):
            for bound in (1, 16, 4096):
                lens_buf = torch.full((len(q) + 2,), -5, dtype=torch.int32, device=dev)
                pos_buf = torch.full((len(q) + 2,), -7, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                rf.match_device(d_q.data_ptr(), len(q), bound, lens_buf[1:].data_ptr(), pos_buf[1:].data_ptr(), cyclic=cyclic)
                lens, pos = rf.match(q, bound, cyclic=cyclic)
                got = lens_buf.cpu().numpy()
                assert got[0] == -5 and got[-1] == -5 and np.array_equal(got[1:-1].astype(np.uint32), lens)
                got = pos_buf.cpu().numpy()
                assert got[0] == -7 and got[-1] == -7
                ref.check_positions(text, q, lens, got[1:-1].astype(np.uint32), cyclic)
                lens_buf.fill_(-5)
                torch.cuda.synchronize()
                rf.match_device(d_q.data_ptr(), len(q), bound, lens_buf[1:].data_ptr(), None, cyclic=cyclic)
                assert np.array_equal(lens_buf.cpu().numpy()[1:-1].astype(np.uint32), lens)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    lens, pos = bce_amd.match_tensor(t, d_q, 16, ctx=ctx)
    assert lens.dtype == torch.int32 and pos.dtype == torch.int32 and lens.device == t.device
    want, _ = rf.match(q, 16)
    assert np.array_equal(lens.cpu().numpy().astype(np.uint32), want)
    ref.check_positions(text, q, want, pos.cpu().numpy().astype(np.uint32), False)
    lens, pos = bce_amd.match_tensor(t, d_q, 16, cyclic=True, positions=False)                   # a context of its own
    assert pos is None and np.array_equal(lens.cpu().numpy().astype(np.uint32), rf.match(q, 16, cyclic=True)[0])
    lens, pos = bce_amd.match(text, q, 16)
    assert np.array_equal(lens, want)
    with pytest.raises(ValueError):
        bce_amd.match_tensor(t, d_q.cpu(), 16)                           # the query must lie on the device too


# ---- coverage -----------------------------------------------------------------------------------------------------------------------

def _c_coverage(ctx, q, min_len, flags):
    arr = np.frombuffer(q, dtype=np.uint8)
    out = C.c_uint64(123)
    assert ctx.lib.bce_hip_coverage(ctx.h, arr.ctypes.data, len(arr), min_len, flags, C.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("name", ("n1", "n96", "abracadabra", "a300", "ab150", "text6144", "text100000"))
def test_coverage_is_the_reference_through_every_entry_point(ctx, name):
    text = _text(name)
    qs, _ = _queries(name)
    rf = api.RankFile(text, ctx=ctx)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    for k, q in enumerate(qs):
        d_q = torch.from_numpy(np.frombuffer(q, dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        for cyclic in (False, True):
            for m in (1, 4, 16):
                want = ref.covered(_want(name, k, cyclic, m), m)
                assert want == ref.covered(_full(name, k, cyclic), m)     # (a search bounded at min_len covers what the full one does)
                assert _c_coverage(ctx, q, m, 0 if cyclic else LINEAR) == want, (name, k, cyclic, m)
                assert rf.coverage(q, m, cyclic=cyclic) == want
                assert rf.coverage_device(d_q.data_ptr(), len(q), m, cyclic=cyclic) == want
        if k in (2, len(qs) - 1):
            assert bce_amd.coverage_tensor(t, d_q, 4, ctx=ctx) == ref.covered(_want(name, k, False, 4), 4)
            rf = api.RankFile(text, ctx=ctx)                              # (coverage_tensor indexed t in this context: the same text)
    assert rf.coverage(b"\x00" * 5000, 1) == 0


def test_coverage_carries_a_long_match_over_several_scan_blocks(ctx):
    """min_len 4096 on a query of three scan blocks (2048 elements each): the windows that end in the third block cover bytes of
    the first.  One spoiled byte at 5000: the matches of 4096 bytes end at 4095 .. 4999, so exactly the first 5000 bytes count."""
    text = _text("text6144")
    q = bytearray(text)
    q[5000] ^= 0x80
    q = bytes(q)
    rf = api.RankFile(text, ctx=ctx)
    for cyclic in (False, True):
        want = ref.coverage(text, q, 4096, cyclic)
        assert rf.coverage(q, 4096, cyclic=cyclic) == want
    assert ref.coverage(text, q, 4096) == 5000
    assert rf.coverage(text, 4096) == 6144 and rf.coverage(text[:4095], 4096) == 0 and rf.coverage(text[:4096], 4096) == 4096
    assert bce_amd.coverage(text, q, 4096) == 5000


def test_coverage_in_archive_plain_and_checked_container():
    data = bce_amd.synth_text(41, 10000).tobytes()
    query = bytearray(data[2000:4500] + data[9000:] + data[:700])
    for at in range(17, len(query), 97):
        query[at] ^= 0x80
    query = bytes(query)
    plain = bytes(bce_amd.compress(data[:4000]))
    for m in (1, 4, 16):
        assert bce_amd.coverage_in_archive(plain, query, m) == ref.coverage(data[:4000], query, m)
        assert bce_amd.coverage_in_archive(plain, query, m, cyclic=True) == ref.coverage(data[:4000], query, m, True)
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)                   # what `bce -C2` writes
    assert len(container.block_table(blob)) == 2 and all(e[3] is not None for e in container.block_table(blob))
    d_q = torch.from_numpy(np.frombuffer(query, dtype=np.uint8).copy()).to("cuda:0")
    for m in (1, 4, 16):
        want = ref.coverage(data, query, m)
        assert bce_amd.coverage_in_archive(blob, query, m) == want
        assert bce_amd.coverage_in_archive(blob, d_q, m) == want         # the query already on the device
    assert ref.coverage(data, query, 16) > ref.coverage(data[:4000], query, 16) > 0


# ---- states and refusals ----------------------------------------------------------------------------------------------------------

def test_injected_bwt_cyclic_lengths_only():
    text = b"abracadabra" * 9 + b"x"
    bwt, row0 = count_ref.bwt_of_rotations(text)
    q = b"cadabraabra" + b"xabra" + b"\x00" + b"dab"
    c = api._Ctx(0)
    try:
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)
        for bound in (1, 16, 4096):
            lens, pos = rf.match(q, bound, cyclic=True, positions=False)
            assert pos is None and np.array_equal(lens, ref.match_lens(text, q, bound, True))
        assert rf.coverage(q, 4, cyclic=True) == ref.coverage(text, q, 4, True)
        with pytest.raises(ValueError):
            rf.match(q, 16)
        with pytest.raises(ValueError):
            rf.coverage(q, 16)
        with pytest.raises(api.BceError) as e:
            rf.match(q, 16, cyclic=True)                                  # positions: there is no suffix array
        assert e.value.status == E_STATE and "no suffix array behind an injected BWT" in str(e.value)
        arr, lens, cov = np.frombuffer(q, dtype=np.uint8), np.full(len(q), 7, dtype=np.uint32), C.c_uint64(5)
        assert c.lib.bce_hip_match(c.h, arr.ctypes.data, len(q), 16, LINEAR, lens.ctypes.data, None) == E_STATE
        assert c.lib.bce_hip_coverage(c.h, arr.ctypes.data, len(q), 16, LINEAR, C.byref(cov)) == E_STATE
        assert (lens == 7).all()
    finally:
        c.close()


def test_refused_arguments_and_states():
    text = bce_amd.synth_text(5, 20000)
    q = np.frombuffer(text[100:164].tobytes(), dtype=np.uint8)
    c = api._Ctx(0)
    try:
        lib = c.lib
        lens, pos, cov = np.full(64, 7, dtype=np.uint32), np.full(64, 9, dtype=np.uint32), C.c_uint64(5)
        args = (c.h, q.ctypes.data, 64, 16, LINEAR, lens.ctypes.data, pos.ctypes.data)
        for fn in (lib.bce_hip_match, lib.bce_hip_match_device):
            assert fn(*args) == E_STATE and b"holds no planes" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_coverage(c.h, q.ctypes.data, 64, 16, 0, C.byref(cov)) == E_STATE
        api.RankFile(text, ctx=c, build=False)                            # loaded, K1 done, no planes yet
        assert lib.bce_hip_match(*args) == E_STATE
        rf = api.RankFile(text, ctx=c)
        for fn in (lib.bce_hip_match, lib.bce_hip_match_device):         # every refusal comes before a launch: host pointers are never read
            for bound in (0, 4097, 0xFFFFFFFF):
                assert fn(*(args[:3] + (bound,) + args[4:])) == E_ARG
            for flags in (2, 3, 0x80000000):
                assert fn(*(args[:4] + (flags,) + args[5:])) == E_ARG
            assert fn(*(args[:2] + (1 << 31,) + args[3:])) == E_ARG
            assert fn(c.h, None, 64, 16, LINEAR, lens.ctypes.data, None) == E_ARG
            assert fn(c.h, q.ctypes.data, 64, 16, LINEAR, None, None) == E_ARG
            assert fn(c.h, None, 0, 16, LINEAR, None, None) == 0          # no query: nothing to do
        for fn in (lib.bce_hip_coverage, lib.bce_hip_coverage_device):
            for bound in (0, 4097):
                assert fn(c.h, q.ctypes.data, 64, bound, LINEAR, C.byref(cov)) == E_ARG
            assert fn(c.h, q.ctypes.data, 64, 16, 2, C.byref(cov)) == E_ARG
            assert fn(c.h, q.ctypes.data, 64, 16, LINEAR, None) == E_ARG
            assert fn(c.h, None, 64, 16, LINEAR, C.byref(cov)) == E_ARG
            cov.value = 5
            assert fn(c.h, None, 0, 16, LINEAR, C.byref(cov)) == 0 and cov.value == 0
        assert (lens == 7).all() and (pos == 9).all()
        with pytest.raises(api.BceError):
            rf.match(b"abc", 0)
        lens, pos = rf.match(b"", 16)
        assert len(lens) == 0 and len(pos) == 0 and rf.coverage(b"", 16) == 0
        # a decode takes the planes and the suffix array away
        fresh = bytes(bce_amd.compress(text))
        assert bce_amd.decompress_device(fresh, ctx=c) == text.tobytes()
        assert lib.bce_hip_match(*args) == E_STATE
    finally:
        c.close()


# ---- nothing else moves ---------------------------------------------------------------------------------------------------------

def test_match_leaves_the_compression_the_count_and_the_locate_alone():
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
        assert np.array_equal(lens, ref.match_lens(tb, query, 300))
        ref.check_positions(tb, query, lens, pos, False)
        cyc, _ = rf.match(query, 300, cyclic=True)
        cov = rf.coverage(query, 16)
        assert cov == ref.covered(lens, 16)
        # match, then encode: the archive of a fresh context; then the same answers on the suffix array the encoder has read
        assert bytes(api.BCE().encode(rf)) == fresh
        again, pos = rf.match(query, 300)
        assert np.array_equal(again, lens) and np.array_equal(rf.match(query, 300, cyclic=True)[0], cyc) and rf.coverage(query, 16) == cov
        ref.check_positions(tb, query, again, pos, False)
        assert rf.count(pats).tolist() == counts
        for a, b in zip(rf.locate(pats), hits):
            assert np.array_equal(a, b)
        assert [h.tolist() for h in hits[:20]] == [locate_ref.linear_hits(tb, p) for p in pats[:20]]
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
    finally:
        c.close()
