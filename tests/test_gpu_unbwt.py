"""GPU: the back end of the GPU decoder (kd_backend.hip) alone, through its two test hooks, compared exactly with the plain
reference of tests/unbwt_ref.py.

bce_hip_planes_from_ranks_device: sparse boundary ranks -> plane words and word ranks (fill_chunkmax / fill_chunkscan / fill_kernel)
-> granules -> bytes (gran_from_words_kernel, access_kernel).  The words and ranks judge the fill without access_kernel; the bytes
judge access_kernel on words and ranks already found right.  Sizes around a word, a granule and one to three chunks of 8192; known
boundaries forced onto those edges; long gaps carried over many chunks, and over the 1024 chunks one trip of the chunk scan takes.
bce_hip_unbwt_device: BWT bytes -> text, at every row count where lf_walk's walker stride changes, on periodic texts (the cycle
written once, then unrolled) and on bytes that are no BWT.  Every output lies between guard bytes, which stay as they were, and a
refused input leaves the output itself as it was.  tests/test_unbwt_ref_cpu.py holds the reference and the rank arrays to their
side of the bargain on the CPU.

Each case asserts the route it is there for: chunk count, walker count (from the stride the test computes itself), cycle length."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
import oracle
import unbwt_cases as cases
import unbwt_ref as ref
from bce_amd import api

pytestmark = pytest.mark.gpu
E_ARG, E_INTERNAL = -1, -6
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def last_error(ctx):
    return ctx.lib.bce_hip_last_error(ctx.h).decode()


class Guarded:
    """`nbytes` of device memory, `shift` bytes off 64-byte alignment, between two guards; all of it holds FILL."""

    def __init__(self, nbytes, shift=0):
        self.nbytes, self.lo = nbytes, GUARD + shift
        self.t = torch.full((self.lo + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.t.data_ptr() + self.lo

    def read(self, dtype=np.uint8):
        """The body; the guards must be as they were."""
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == FILL).all() and (h[self.lo + self.nbytes:] == FILL).all(), "guard bytes written"
        return h[self.lo:self.lo + self.nbytes].copy().view(dtype)

    def untouched(self):
        return bool((self.read() == FILL).all())


def to_device(a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    t = torch.from_numpy(a.view(np.uint8).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def run_planes(ctx, R, n, outputs=True):
    """-> (status, bytes buffer, words buffer, word-rank buffer); the guards are checked when the buffers are read."""
    dR = to_device(R)
    wb = 8 * ref.plane_words(n) * 4
    bwt, words, rankw = Guarded(n, shift=n % 3), Guarded(wb) if outputs else None, Guarded(wb) if outputs else None
    rc = api.planes_from_ranks_device(dR.data_ptr(), n, bwt.ptr, ctx, words.ptr if outputs else None, rankw.ptr if outputs else None)
    torch.cuda.synchronize()
    return rc, bwt, words, rankw


def check_planes(ctx, case):
    rc, bwt, words, rankw = run_planes(ctx, case.R, case.n)
    assert rc == 0, (case.name, last_error(ctx))
    W = ref.plane_words(case.n)
    got_w, got_r = words.read(np.uint32).reshape(8, W), rankw.read(np.uint32).reshape(8, W)
    assert np.array_equal(got_w, case.words), (case.name, "words", np.argwhere(got_w != case.words)[:4])
    assert np.array_equal(got_r, case.rankw), (case.name, "rankw", np.argwhere(got_r != case.rankw)[:4])
    got = bwt.read()
    assert np.array_equal(got, case.data), (case.name, "bytes", np.flatnonzero(got != case.data)[:4])


# ---- fill and access ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", cases.FILL_SIZES)
def test_fill_and_access_at_word_granule_and_chunk_sizes(ctx, n):
    assert ref.fill_chunks(n) == n // 8192 + 1
    last = None
    for case in cases.fill_cases(n):
        assert ref.gaps_constant(case.R), case.name
        check_planes(ctx, case)
        last = case
    rc, bwt, _, _ = run_planes(ctx, last.R, n, outputs=False)     # the two optional outputs left out
    assert rc == 0 and np.array_equal(bwt.read(), last.data)


def test_fill_boundaries_on_chunk_word_and_granule_edges(ctx):
    names = []
    for case in cases.edge_fill_cases():
        assert ref.gaps_constant(case.R), case.name
        check_planes(ctx, case)
        names.append(case.name)
    assert "only-boundary-at-8191" in names and "only-boundary-at-8192" in names and "ones-zeros-mixed" in names


def test_fill_carries_a_boundary_over_more_than_1024_chunks(ctx):
    for case in cases.big_cases():
        assert ref.fill_chunks(case.n) > 1024                     # the chunk scan's second trip
        assert ref.gaps_constant(case.R), case.name
        known = np.flatnonzero(case.R[0] != ref.K_UNKNOWN)
        assert np.diff(known).max() > 200 * ref.FG_CHUNK          # a gap of hundreds of chunks
        check_planes(ctx, case)


def test_fill_refuses_mixed_gaps_decreasing_ranks_and_unknown_ends(ctx):
    good = next(iter(cases.edge_fill_cases()))
    seen = 0
    for case in cases.refused_fill_cases():
        assert not ref.gaps_constant(case.R), case.name
        rc, bwt, words, rankw = run_planes(ctx, case.R, case.n)
        assert rc == E_INTERNAL, case.name
        assert last_error(ctx) == "decode: a mixed gap was never split"
        assert bwt.untouched() and words.untouched() and rankw.untouched(), case.name
        seen += 1
    assert seen == 5
    n = good.n
    for p, i, v in ((0, 0, ref.K_UNKNOWN), (3, 0, ref.K_UNKNOWN), (7, n, ref.K_UNKNOWN), (2, n, n + 1), (4, 0, 1)):
        R = good.R.copy()
        R[p, i] = v
        rc, bwt, words, rankw = run_planes(ctx, R, n)
        assert rc == E_ARG, (p, i, v)
        assert bwt.untouched() and words.untouched() and rankw.untouched()
    d = to_device(good.R)
    out = Guarded(n)
    lib, h = ctx.lib, ctx.h
    assert lib.bce_hip_planes_from_ranks_device(None, d.data_ptr(), n, out.ptr, None, None) == E_ARG
    assert lib.bce_hip_planes_from_ranks_device(h, None, n, out.ptr, None, None) == E_ARG
    assert lib.bce_hip_planes_from_ranks_device(h, d.data_ptr(), n, None, None, None) == E_ARG
    assert lib.bce_hip_planes_from_ranks_device(h, d.data_ptr(), 0, out.ptr, None, None) == E_ARG
    assert lib.bce_hip_planes_from_ranks_device(h, d.data_ptr(), 0x7FFFFFFF, out.ptr, None, None) == E_ARG
    assert out.untouched()
    check_planes(ctx, good)                                       # ... and the context goes on working


# ---- inverse BWT -------------------------------------------------------------------------------------------------------------

def run_unbwt(ctx, bwt, off, shift=1):
    a = np.ascontiguousarray(bwt, dtype=np.uint8)
    d = to_device(a)
    out = Guarded(len(a), shift=shift)
    rc, lc, m = api.unbwt_device(d.data_ptr(), len(a), off, out.ptr, ctx)
    torch.cuda.synchronize()
    return rc, lc, m, out


def my_walkers(rows):
    sh = 0
    while (rows >> sh) > (1 << 19):
        sh += 1
    while sh < 8 and (rows >> (sh + 1)) >= 4096:
        sh += 1
    return ((rows - 1) >> sh) + 1, sh


def check_unbwt(ctx, bwt, off, want_text=None, want_lc=None, name=""):
    """The hook against the reference: status, cycle length, walkers, text -- or the refusal, the output as it was."""
    n = len(bwt)
    text, lc = ref.inverse(bwt, off)
    if want_lc is not None:
        assert lc == want_lc, (name, lc)
    rc, got_lc, m, out = run_unbwt(ctx, bwt, off)
    assert got_lc == lc, (name, got_lc, lc)
    assert m == my_walkers(n)[0], (name, m)
    if text is None:
        assert rc == E_INTERNAL, name
        assert last_error(ctx) == "decode: LF cycle of length %d in %d rows" % (lc, n)
        assert out.untouched(), name
        return False
    assert rc == 0, (name, last_error(ctx))
    got = out.read()
    assert np.array_equal(got, text), (name, np.flatnonzero(got != text)[:4])
    if want_text is not None:
        assert got.tobytes() == bytes(want_text), name
    return True


@pytest.fixture(scope="module")
def long_texts():
    n = (1 << 20) + 1
    rs = np.random.RandomState(21)
    return {"synth_text": oracle.synth_text(13, n), "four-symbols": rs.choice([0x20, 0x61, 0x62, 0xF0], n).astype(np.uint8).tobytes()}


@pytest.mark.parametrize("k", range(8))
def test_unbwt_at_every_walker_threshold(ctx, long_texts, k):
    T = 8192 << k
    assert [my_walkers(T + d)[1] for d in (-1, 0, 1)] == [k, k + 1, k + 1]      # the stride changes exactly here
    for kind, full in long_texts.items():
        for n in (T - 1, T, T + 1):
            data = full[:n]
            bwt, off = oracle.bwt_stage(data)
            assert check_unbwt(ctx, bwt, off, want_text=data, want_lc=n, name="%s/%d" % (kind, n))
    data = long_texts["synth_text"][:T + 1]                         # a ragged last walker, every offset
    bwt, off = oracle.bwt_stage(data)
    assert my_walkers(T + 1)[0] == (T >> (k + 1)) + 1               # the last walker starts at row T and has one row
    for o in (0, 1, T):
        assert check_unbwt(ctx, bwt, o, want_text=np.roll(np.frombuffer(data, dtype=np.uint8), o - off).tobytes(), name="off=%d" % o)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257])
def test_unbwt_small_sizes_and_offsets(ctx, n):
    data = oracle.synth_text(n, n)
    bwt, off = oracle.bwt_stage(data)
    text, lc = ref.inverse(bwt, off)
    assert text.tobytes() == data
    for o in sorted({0, 1 % n, n - 1, off}):
        assert check_unbwt(ctx, bwt, o, want_text=np.roll(text, o - off).tobytes(), name="n=%d off=%d" % (n, o))
    # the hook reduces the offset modulo n, as the decoder reduces the archive's
    for o in (n, n + 1, 5 * n + off, 0xFFFFFFFF):
        rc, got_lc, m, out = run_unbwt(ctx, bwt, o)
        assert rc == 0 and got_lc == lc
        assert out.read().tobytes() == np.roll(text, o % n - off).tobytes(), o


def periodic_texts():
    rs = np.random.RandomState(31)
    unit = lambda p, symbols=256: bytes(rs.randint(0, symbols, p - 1).astype(np.uint8)) + b"\xfe"   # (0xFE once: the unit is primitive)
    out = [("constant-1", b"z", 1), ("constant-8193", b"z" * 8193, 1), ("constant-16384", b"\x00" * 16384, 1),
           ("ab-x500", b"ab" * 500, 2), ("ab-x8192", b"ab" * 8192, 2), ("ab-x8193", b"ab" * 8193, 2)]
    for p, T in ((3, 8192), (7, 16384), (257, 32768), (4099, 1 << 20)):
        u = unit(p, 4 if p < 300 else 256)
        for label, reps in (("below", T // p), ("above", T // p + 1)):
            out.append(("unit%d-%s-%d" % (p, label, T), u * reps, p))
    for p, T in ((4096, 8192), (4096, 65536), (2048, 1 << 20)):    # powers of two: n lands ON the threshold
        out.append(("unit%d-on-%d" % (p, T), unit(p) * (T // p), p))
    out.append(("halves-8192", oracle.synth_text(5, 8192) * 2, 8192))
    out.append(("halves-300001", oracle.synth_text(6, 300001) * 2, 300001))
    out.append(("unit1001-x37", unit(1001) * 37, 1001))            # n = 37037: no multiple of its stride 2^3
    return out


PERIODIC = periodic_texts()


@pytest.mark.parametrize("name,data,lc", PERIODIC, ids=[p[0] for p in PERIODIC])
def test_unbwt_periodic_texts(ctx, name, data, lc):
    n = len(data)
    bwt, off = oracle.bwt_stage(data)
    m, sh = my_walkers(n)
    if name == "unit1001-x37":
        assert n % (1 << sh) != 0
    if name.startswith("unit") and "-on-" in name:
        assert n in (8192, 65536, 1 << 20)
    if "-below-" in name:
        T = int(name.rsplit("-", 1)[1])
        assert n < T and my_walkers(n)[1] + 1 == my_walkers(T)[1]
    if "-above-" in name:
        T = int(name.rsplit("-", 1)[1])
        assert n > T and my_walkers(n)[1] == my_walkers(T)[1]
    assert check_unbwt(ctx, bwt, off, want_text=data, want_lc=lc, name=name)
    if n > 1:
        assert lc < n                                                # the periodic route: the cycle, then expand_cycle_kernel
        for o in (0, 1, n - 1):
            assert check_unbwt(ctx, bwt, o, want_lc=lc, name="%s off=%d" % (name, o))


def test_unbwt_refuses_what_is_no_bwt(ctx):
    rs = np.random.RandomState(41)
    refused = accepted = 0
    primitive = [oracle.synth_text(8, 8193), oracle.synth_text(8, 20000), bytes(rs.randint(0, 4, 16385).astype(np.uint8))]
    periodic = [b"abcabcabd" * 3000, oracle.synth_text(2, 5000) * 7, bytes(rs.randint(0, 256, 257).astype(np.uint8)) * 64]
    for data in primitive + periodic:
        bwt, off = oracle.bwt_stage(data)
        n = len(bwt)
        for trial in range(6):
            bad = bwt.copy()
            if data in primitive:                                   # two bytes swapped
                i, j = rs.randint(0, n, 2)
                bad[i], bad[j] = bwt[j], bwt[i]
            else:                                                   # one byte changed
                i = rs.randint(0, n)
                bad[i] ^= 1 << rs.randint(0, 8)
            ok = check_unbwt(ctx, bad, off, name="bad %d/%d" % (n, trial))
            accepted, refused = accepted + ok, refused + (not ok)
    assert refused >= 12                                            # (most damaged arrays are refused; the reference says which)
    # rows 0 and 2 are a cycle of their own: length 2 in 5 rows
    assert not check_unbwt(ctx, np.frombuffer(b"bbaab", dtype=np.uint8), 0, want_lc=2)
    # no BWT of anything, but row 0 is a cycle of length 1, which divides 8: a constant text, as the decoder would give
    assert check_unbwt(ctx, np.frombuffer(b"abababab", dtype=np.uint8), 0, want_text=b"a" * 8, want_lc=1)
    d, out = to_device(np.zeros(16, dtype=np.uint8)), Guarded(16)
    lib, h = ctx.lib, ctx.h
    lc, m = C.c_uint64(7), C.c_uint32(7)
    assert lib.bce_hip_unbwt_device(None, d.data_ptr(), 16, 0, out.ptr, C.byref(lc), C.byref(m)) == E_ARG
    assert lib.bce_hip_unbwt_device(h, None, 16, 0, out.ptr, C.byref(lc), C.byref(m)) == E_ARG
    assert lib.bce_hip_unbwt_device(h, d.data_ptr(), 16, 0, None, C.byref(lc), C.byref(m)) == E_ARG
    assert lib.bce_hip_unbwt_device(h, d.data_ptr(), 0, 0, out.ptr, C.byref(lc), C.byref(m)) == E_ARG
    assert lib.bce_hip_unbwt_device(h, d.data_ptr(), 0x7FFFFFFF, 0, out.ptr, C.byref(lc), C.byref(m)) == E_ARG
    assert (lc.value, m.value) == (7, 7) and out.untouched()
    assert lib.bce_hip_unbwt_device(h, d.data_ptr(), 16, 3, out.ptr, None, None) == 0       # the two reports are optional
    assert out.read().tobytes() == b"\x00" * 16
    assert check_unbwt(ctx, *oracle.bwt_stage(primitive[0]), want_text=primitive[0])         # ... and the context goes on working


# ---- the seam: n + 1 rows ----------------------------------------------------------------------------------------------------

def seam_inverse(ctx, u, idx):
    a = np.frombuffer(bytes(u), dtype=np.uint8).copy()
    out = np.full(len(a) + 2 * GUARD, FILL, dtype=np.uint8)
    rc = ctx.lib.bce_hip_inverse_bwt(ctx.h, a.ctypes.data, out[GUARD:].ctypes.data, len(a), idx)
    assert (out[:GUARD] == FILL).all() and (out[GUARD + len(a):] == FILL).all()
    return rc, out[GUARD:GUARD + len(a)]


@pytest.mark.parametrize("k", range(8))
def test_seam_at_every_walker_threshold(ctx, long_texts, k):
    T = 8192 << k
    body = np.frombuffer(long_texts["synth_text"], dtype=np.uint8)
    assert body.min() > 0 and body.max() < 255
    for n in (T - 2, T - 1, T):                                      # n + 1 rows: below, on and above the threshold
        assert [my_walkers(n + 1)[1]] == [k if n + 1 < T else k + 1]
        first = b"\x00" + body[:n - 1].tobytes()                     # the whole text is the smallest suffix: idx = 1
        last = b"\xff" + body[:n - 1].tobytes()                      # ... the largest: idx = n
        middle = body[:n].tobytes()
        for t, where in ((first, "first"), (last, "last"), (middle, "middle")):
            u, p = oracle.divbwt(t)
            assert {"first": p == 1, "last": p == n, "middle": 1 < p < n}[where], (where, p)
            rc, got = seam_inverse(ctx, u, p)
            assert rc == 0 and got.tobytes() == t == oracle.inverse_bwt(u, p), (n, where)
    # a wrong index: the n + 1 rows are no longer one cycle (the reference says so), and nothing is written
    n = T - 1
    u, p = oracle.divbwt(body[:n].tobytes())
    wrong = p + 1 if p < n else p - 1
    if ref.seam_inverse(np.frombuffer(u, dtype=np.uint8), wrong) is None:
        rc, got = seam_inverse(ctx, u, wrong)
        assert rc == E_ARG and (got == FILL).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8193, 300000, 1 << 20])
def test_ranks_of_a_real_decode_through_both_hooks(ctx, n):
    data = oracle.synth_text(17, n)
    bwt, off = oracle.bwt_stage(data)
    case = cases.Case("real/%d" % n, bwt)                            # what the rounds leave: the minimal set of every level
    assert ref.gaps_constant(case.R)
    rc, d_bwt, words, rankw = run_planes(ctx, case.R, n)
    assert rc == 0, last_error(ctx)
    assert np.array_equal(d_bwt.read(), bwt)
    out = Guarded(n, shift=3)
    rc, lc, m = api.unbwt_device(d_bwt.ptr, n, off, out.ptr, ctx)    # straight from the first hook's output, on the device
    assert rc == 0 and lc == n and m == my_walkers(n)[0]
    assert out.read().tobytes() == data
    assert (d_bwt.read() == bwt).all() and np.array_equal(words.read(np.uint32).reshape(8, -1), case.words)
    assert bce_amd.decompress_device(oracle.compress(data), ctx=ctx) == data


def test_hooks_leave_the_context_fit_for_encode_and_decode(ctx):
    data = oracle.synth_text(19, 300000)
    archive = bce_amd.compress(data, ctx=ctx)
    assert archive == oracle.compress(data)
    assert bce_amd.decompress_device(archive, ctx=ctx) == data
    for hook in ("planes", "unbwt", "refused"):
        if hook == "planes":
            check_planes(ctx, next(iter(cases.edge_fill_cases())))
        elif hook == "unbwt":
            assert check_unbwt(ctx, *oracle.bwt_stage(b"abcabcabd" * 3000), want_lc=9)
        else:
            rc, _, _, _ = run_planes(ctx, next(iter(cases.refused_fill_cases())).R, 20000)
            assert rc == E_INTERNAL
            assert not check_unbwt(ctx, np.frombuffer(b"bbaab", dtype=np.uint8), 0)
        assert bce_amd.compress(data, ctx=ctx) == archive, hook
        assert bce_amd.decompress_device(archive, ctx=ctx) == data, hook
