"""GPU: pattern counts from the BWT planes (kd_count.hip through bce_hip_count / _count_device, RankFile.count, count_tensor,
count_in_archive) against brute-force counts of the same text in Python / numpy.  K1, the K2 planes, the rank directory and
zeros[] are checked together here without the coder: a wrong BWT byte, granule or zeros[] entry moves some count."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import count_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -4
SIZES = (1, 2, 95, 96, 97, 3071, 3072, 3073, 6144)     # the granule holds 96 positions, the chunk 3072: rank(n) sits in the last granule or a new one


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
    """Every byte value alone; substrings at the wrap; m = n, n + 1, 3 n; absent bytes; the empty pattern."""
    n = len(text)
    pats = [bytes([v]) for v in range(256)]
    for m in (2, 3, 8, 64):
        for back in (1, m // 2, m - 1):
            pats.append(ref.cyclic_cut(text, n - min(back, n), m))
    pats += [ref.cyclic_cut(text, 0, n), ref.cyclic_cut(text, n // 3, n), ref.cyclic_cut(text, 0, n + 1), ref.cyclic_cut(text, n - 1, n + 1)]
    if n <= 97:
        pats += [ref.cyclic_cut(text, 0, 3 * n), ref.cyclic_cut(text, n // 2, 3 * n)]
    pats += [b"\x00", b"\xff", text[:2] + b"\x00", b"\xff" + text[:3], b""]
    return pats


def _want_cyclic(text, pats):
    """Brute force, made affordable: the single bytes from a histogram, long patterns by where their first bytes match."""
    n = len(text)
    hist = np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256)
    ext = text * 2
    out = []
    for p in pats:
        m = len(p)
        if m == 0:
            out.append(n)
        elif m == 1:
            out.append(int(hist[p[0]]))
        elif m <= n:
            out.append(ref.linear_count(ext[:n + m - 1], p))         # the circular text unrolled once: a scan of n + m - 1 bytes
        else:
            out.append(ref.cyclic_count(text, p))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_counts_are_the_brute_force_counts_at_the_layout_boundaries(ctx, n):
    for name, text in _texts(n):
        pats = _patterns(text)
        want = _want_cyclic(text, pats)
        rf = api.RankFile(text, ctx=ctx)
        got = rf.count(pats, cyclic=True)
        assert got.dtype == np.uint64 and got.tolist() == want, (name, n)
        assert int(got[:256].sum()) == n
        lin = [p for p in pats if p]
        assert rf.count(lin).tolist() == [ref.linear_count(text, p) for p in lin], (name, n)
        assert rf.count(lin[260]) == ref.linear_count(text, lin[260]) and isinstance(rf.count(lin[260]), int)    # one pattern: an int


@pytest.mark.parametrize("npat", (1, 63, 64, 65, 256, 257, 1000))
def test_batches_of_mixed_lengths(ctx, npat):
    """Lengths 1..64 mixed inside one batch -- the lanes of a wave finish at different times --, with patterns that die early."""
    text = bce_amd.synth_text(31, 5000).tobytes()
    rs = np.random.RandomState(npat)
    pats = []
    for i in range(npat):
        m, at = int(rs.randint(1, 65)), int(rs.randint(0, len(text)))
        p = bytearray(ref.cyclic_cut(text, at, m))
        if i % 5 == 4:
            p[int(rs.randint(0, m))] ^= 0x80                            # (synth_text is 7-bit: this byte occurs nowhere)
        pats.append(bytes(p))
    rf = api.RankFile(text, ctx=ctx)
    assert rf.count(pats, cyclic=True).tolist() == _want_cyclic(text, pats)
    assert rf.count(pats).tolist() == [ref.linear_count(text, p) for p in pats]


def test_injected_bwt_counts_cyclically_and_has_no_linear_count(ctx):
    """K2 + count without K1: the BWT of the rotations sorted in Python."""
    for text in (b"abracadabra", b"abab" * 30, bce_amd.synth_text(3, 700).tobytes()):
        bwt, row0 = ref.bwt_of_rotations(text)
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=ctx)
        pats = _patterns(text)
        assert rf.count(pats, cyclic=True).tolist() == _want_cyclic(text, pats)
        assert rf.count(b"", cyclic=True) == len(text)
        with pytest.raises(ValueError):
            rf.count(b"abra")
    rf = api.RankFile(b"abracadabra", ctx=ctx)
    with pytest.raises(ValueError):
        rf.count(b"")
    with pytest.raises(ValueError):
        rf.count([b"a", b""])
    assert rf.count([]).tolist() == [] and rf.count(b"abra") == 2 and rf.count(b"abra", cyclic=True) == 2 and rf.count(b"aabr", cyclic=True) == 1


def test_count_device_takes_patterns_built_in_a_tensor(ctx):
    text = bce_amd.synth_text(8, 4000)
    t = torch.from_numpy(text).to("cuda:0")
    m, npat = 5, 300
    starts = torch.arange(npat, device="cuda:0") * 13
    pat = t[(starts[:, None] + torch.arange(m, device="cuda:0")[None, :]) % len(text)].contiguous().reshape(-1)   # cut on the device
    off = (torch.arange(npat + 1, device="cuda:0", dtype=torch.int64) * m)
    out = torch.full((npat,), -1, device="cuda:0", dtype=torch.int64)
    torch.cuda.synchronize()
    rf = api.RankFile(n=len(text), device_ptr=t.data_ptr(), ctx=ctx)
    rf.count_device(pat.data_ptr(), off.data_ptr(), npat, out.data_ptr())
    tb = text.tobytes()
    assert out.cpu().tolist() == [ref.cyclic_count(tb, ref.cyclic_cut(tb, 13 * i, m)) for i in range(npat)]
    # decreasing offsets: found by the kernel; the context stays usable
    off[7] = off[9]
    torch.cuda.synchronize()
    with pytest.raises(api.BceError) as e:
        rf.count_device(pat.data_ptr(), off.data_ptr(), npat, out.data_ptr())
    assert e.value.status == E_ARG and "offsets decrease" in str(e.value)
    assert rf.count(tb[:7]) == ref.linear_count(tb, tb[:7])
    # null arrays, and no patterns at all
    with pytest.raises(api.BceError) as e:
        rf.count_device(None, off.data_ptr(), npat, out.data_ptr())
    assert e.value.status == E_ARG
    rf.count_device(None, None, 0, None)


def test_host_arguments_are_checked(ctx):
    lib = ctx.lib
    rf = api.RankFile(b"abracadabra", ctx=ctx)
    pat, out = (C.c_uint8 * 4)(*b"abra"), (C.c_uint64 * 2)(7, 7)
    bad = (C.c_uint64 * 3)(0, 4, 2)
    assert lib.bce_hip_count(ctx.h, C.addressof(pat), C.addressof(bad), 2, C.addressof(out)) == E_ARG
    assert b"offsets decrease" in lib.bce_hip_last_error(ctx.h) and list(out) == [7, 7]
    assert lib.bce_hip_count(ctx.h, None, None, 0, None) == 0
    assert lib.bce_hip_count(ctx.h, C.addressof(pat), None, 1, C.addressof(out)) == E_ARG
    ok = (C.c_uint64 * 3)(0, 4, 4)                                       # "abra", then the empty pattern
    assert lib.bce_hip_count(ctx.h, C.addressof(pat), C.addressof(ok), 2, C.addressof(out)) == 0 and list(out) == [2, 11]
    assert rf.size() == 11


def test_count_tensor_on_a_slice_at_an_odd_offset(ctx):
    data = bce_amd.synth_text(17, 9000)
    big = torch.from_numpy(data).to("cuda:0")
    t = big[1237:1237 + 4099]
    tb = data[1237:1237 + 4099].tobytes()
    assert t.data_ptr() % 2 == 1
    pats = [tb[:9], tb[-9:], tb[-4:] + tb[:5], tb[2000:2033], b"e", tb + b"x", data[1230:1240].tobytes()]
    want = [ref.linear_count(tb, p) for p in pats]
    assert ref.cyclic_count(tb, pats[2]) == want[2] + 1                # (the match across the seam is what must come off)
    assert bce_amd.count_tensor(t, pats, ctx=ctx).tolist() == want
    assert bce_amd.count_tensor(t, pats[3]) == want[3]                 # a context of its own
    assert bce_amd.count(tb, pats).tolist() == want                    # the same from host bytes
    with pytest.raises(ValueError):
        bce_amd.count_tensor(big[::2], b"e")


def test_count_needs_planes_and_leaves_the_compression_alone():
    text = bce_amd.synth_text(5, 50000)
    tb = text.tobytes()
    fresh = bytes(bce_amd.compress(text))
    c = api._Ctx(0)
    try:
        lib = c.lib
        pat, off, out = (C.c_uint8 * 4)(*b"the "), (C.c_uint64 * 2)(0, 4), (C.c_uint64 * 1)(7)
        args = (c.h, C.addressof(pat), C.addressof(off), 1, C.addressof(out))
        assert lib.bce_hip_count(*args) == E_STATE and b"holds no planes" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_count_device(*args) == E_STATE
        rf = api.RankFile(text, ctx=c, build=False)                      # loaded, K1 done, no planes yet
        assert lib.bce_hip_count(*args) == E_STATE and out[0] == 7
        rf = api.RankFile(text, ctx=c)
        pats = [tb[i * 97:i * 97 + 1 + i % 40] for i in range(400)]
        want = [ref.linear_count(tb, p) for p in pats]
        assert rf.count(pats).tolist() == want
        # count, then encode: the archive of a fresh context; then count again: the same numbers
        assert bytes(api.BCE().encode(rf)) == fresh
        assert rf.count(pats).tolist() == want
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
        # a decode takes the planes away
        assert bce_amd.decompress_device(fresh, ctx=c) == tb
        assert lib.bce_hip_count(*args) == E_STATE
    finally:
        c.close()


def test_two_million_bytes_ten_thousand_patterns(ctx):
    """Many granules per plane (20 834) and 40 workgroups; the reference is a sliding-window compare on a 200-pattern subset."""
    n, npat, m = 2000000, 10000, 8
    text = bce_amd.synth_text(77, n)
    starts = np.random.RandomState(7).randint(0, n - m, npat)
    pats = np.stack([text[s:s + m] for s in starts])
    rf = api.RankFile(text, ctx=ctx)
    got = rf.count([p for p in pats])
    assert got.shape == (npat,) and int(got.min()) >= 1
    sub = np.arange(0, npat, npat // 200)
    assert got[sub].tolist() == ref.sliding_counts(text, pats[sub], m).tolist()


def test_count_in_archive():
    data = bce_amd.synth_text(41, 10000).tobytes()
    # a plain archive of 4000 bytes
    plain = bytes(bce_amd.compress(data[:4000]))
    pats = [b"the", data[100:108], data[3990:4000], data[3995:4000] + data[:3]]
    assert bce_amd.count_in_archive(plain, pats).tolist() == [ref.linear_count(data[:4000], p) for p in pats]
    # a version-2 container of 3 blocks; a pattern that straddles a block boundary
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=3)
    table = container.block_table(blob)
    assert len(table) == 3 and all(e[3] is not None for e in table)
    cut = table[0][0]
    pats = [data[cut - 6:cut + 6], data[cut + table[1][0] - 1:cut + table[1][0] + 9], b"e", data[-5:] + data[:5]]
    want = [ref.linear_count(data, p) for p in pats]
    assert want[0] >= 1 and want[1] >= 1
    assert bce_amd.count_in_archive(blob, pats).tolist() == want
    assert bce_amd.count_in_archive(blob, pats[0]) == want[0]
    # one flipped text CRC
    bad = bytearray(blob)
    bad[12 + 24 * 1 + 16] ^= 1
    with pytest.raises(api.ChecksumError) as e:
        bce_amd.count_in_archive(bytes(bad), pats)
    assert e.value.block == 1
    # version 1: no checksums, the same counts
    blob1 = bce_amd.compress_tensor_blocks(t, blocks=3, checksum=False)
    assert bce_amd.count_in_archive(blob1, pats).tolist() == want


def test_count_in_archive_refuses_two_gib_before_decoding():
    """The sizes come from the blocks' own headers: two blocks of 2^30 bytes each are one text too long for one index."""
    data = bce_amd.synth_text(2, 3000).tobytes()
    arch = bytes(bce_amd.compress(data))
    assert api.decoded_size(arch) == 3000
    blob = container.pack_blocks([arch] * 2, [3000, 3000])
    assert bce_amd.count_in_archive(blob, b"e") == 2 * ref.linear_count(data, b"e")
    import bce_amd.tensor as tensor
    old = tensor._MAX_BLOCK
    tensor._MAX_BLOCK = 5999                                             # the same rule at a size a test can hold
    try:
        with pytest.raises(ValueError):
            bce_amd.count_in_archive(blob, b"e")
    finally:
        tensor._MAX_BLOCK = old
