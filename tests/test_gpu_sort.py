"""GPU: the radix sorter (radix_sort.hip) alone, through bce_hip_sort_pairs_device / bce_hip_sort_wide_device, against numpy's
stable argsort of the window's digits.  Exact: keys (the bits outside the window included) and values of every pair, so a result
that is sorted but not stable fails.  Every bit window at every digit width, the sizes at which the plan changes (one block ->
many, one chunk per block -> two, a row scan with a carry), the wide sort's digits in lo, across the words and in hi, and the key
distributions that take the histogram's whole-wave shortcut."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
import oracle
from bce_amd import api

pytestmark = pytest.mark.gpu
E_ARG = -1
K4_SHIFT, K4_BITS = 10, 19                       # bce_core.h: kSymRunShift, kSymRunBits
GUARD_FRONT, GUARD_BACK = 5, 7                   # words around every array handed to the sorter; they must come back untouched

# pairs: chunk 4096, at most 768 blocks; the row scan carries from 257 blocks on; two chunks per block above 768 chunks
PAIR_SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 256 * 4096 + 1, 768 * 4096, 768 * 4096 + 1,
              2 * 768 * 4096 + 4097]
PAIR_SIZE_WINDOWS = [(0, 27, 9), (5, 27, 8), (22, 10, 10)]       # bits 0-27, 5-32, 22-32: digits of 9; 7, 7, 7, 6; 10
# wide: the scatter's chunk is 2048 (the histogram strides 4096), at most 1024 blocks
WIDE_SIZES = [2047, 2048, 2049, 4095, 4096, 4097, 256 * 2048 + 1, 1024 * 2048, 1024 * 2048 + 1]
WIDE_SIZE_BITS = [31, 32, 33, 40, 60, 64]

CALLERS = [("k1-first-0-27-9", 0, 27, 9), ("k1-doubling-0-32-8", 0, 32, 8), ("k1-ranks-0-19-10", 0, 19, 10),
           ("k3-tail-0-11-9", 0, 11, 9), ("k3-tail-1-10-9", 1, 10, 9), ("k3-tail-2-9-9", 2, 9, 9), ("k3-tail-3-8-9", 3, 8, 9),
           ("decoder-rows-0-9-9", 0, 9, 9), ("decoder-bytes-0-8-8", 0, 8, 8), ("k4-slots-%d-%d-10" % (K4_SHIFT, K4_BITS), K4_SHIFT, K4_BITS, 10)]


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _guarded(a, seed):
    """`a` (u32) in device memory between guard words -> (tensor, pointer of a[0], the host image of the whole tensor)"""
    g = np.random.RandomState(seed).randint(0, 1 << 32, GUARD_FRONT + GUARD_BACK, dtype=np.uint64).astype(np.uint32)
    host = np.concatenate([g[:GUARD_FRONT], a, g[GUARD_FRONT:]])
    t = torch.from_numpy(host.view(np.int32)).to("cuda:0")
    return t, t.data_ptr() + 4 * GUARD_FRONT, host


def _back(t, host, n, what):
    got = t.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:GUARD_FRONT], host[:GUARD_FRONT]) and np.array_equal(got[GUARD_FRONT + n:], host[GUARD_FRONT + n:]), \
        "%s: words outside the array were written" % what
    return got[GUARD_FRONT:GUARD_FRONT + n]


def sort_pairs(ctx, key, val, first_bit, bits, mdb):
    n = len(key)
    tk, pk, hk = _guarded(key, 1)
    tv, pv, hv = _guarded(val, 2)
    torch.cuda.synchronize()
    api.sort_pairs_device(pk, pv, n, first_bit, bits, mdb, ctx)
    return _back(tk, hk, n, "keys"), _back(tv, hv, n, "values")


def sort_wide(ctx, lo, hi, val, bits, mdb):
    n = len(lo)
    tl, pl, hl = _guarded(lo, 1)
    th, ph, hh = _guarded(hi, 2)
    tv, pv, hv = _guarded(val, 3)
    torch.cuda.synchronize()
    api.sort_wide_device(pl, ph, pv, n, bits, mdb, ctx)
    return _back(tl, hl, n, "lo"), _back(th, hh, n, "hi"), _back(tv, hv, n, "values")


def _narrow(d, bits):
    # (numpy sorts 16-bit integers stably with a radix sort of its own: much faster than its merge sort at 10^6 and more)
    return d.astype(np.uint16) if bits <= 16 else (d.astype(np.uint32) if bits <= 32 else d)


def pair_perm(key, first_bit, bits):
    d = (key.astype(np.uint64) >> np.uint64(first_bit)) & np.uint64((1 << bits) - 1)
    return np.argsort(_narrow(d, bits), kind="stable")


def wide_perm(lo, hi, bits):
    k = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    return np.argsort(_narrow(k & np.uint64((1 << bits) - 1), bits), kind="stable")


def u32(rs, n):
    return rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def check_pairs(ctx, key, first_bit, bits, mdb, val=None, perm=None):
    n = len(key)
    val = np.arange(n, dtype=np.uint32) if val is None else val
    perm = pair_perm(key, first_bit, bits) if perm is None else perm
    ko, vo = sort_pairs(ctx, key, val, first_bit, bits, mdb)
    where = "n=%d bits [%d, %d) digits <= %d" % (n, first_bit, first_bit + bits, mdb)
    assert np.array_equal(vo, val[perm]), "values, " + where
    assert np.array_equal(ko, key[perm]), "keys, " + where


def check_wide(ctx, lo, hi, bits, mdb, val=None):
    n = len(lo)
    val = np.arange(n, dtype=np.uint32) if val is None else val
    perm = wide_perm(lo, hi, bits)
    lo_o, hi_o, vo = sort_wide(ctx, lo, hi, val, bits, mdb)
    where = "wide n=%d bits [0, %d) digits <= %d" % (n, bits, mdb)
    assert np.array_equal(vo, val[perm]), "values, " + where
    assert np.array_equal(lo_o, lo[perm]) and np.array_equal(hi_o, hi[perm]), "keys, " + where


# ---- every window -----------------------------------------------------------------------------------------------------------

_WINDOW_CASES = {}


def window_case(n):
    """keys of one size and the reference permutation of every window: computed once, shared by the digit widths, never changed"""
    if n not in _WINDOW_CASES:
        key = u32(np.random.RandomState(n), n)
        key.setflags(write=False)
        perms = {(f, b): pair_perm(key, f, b) for f in range(33) for b in range(0, 33 - f)}
        _WINDOW_CASES[n] = (key, perms)
    return _WINDOW_CASES[n]


@pytest.mark.parametrize("mdb", [8, 9, 10])
@pytest.mark.parametrize("n", [4097, 8191])
def test_pairs_every_window(ctx, n, mdb):
    """every (first_bit, bits) inside 32 bits: every scatter instantiation (digits of 10, 9, 8, 7, 6 and the runtime width),
    shifts up to 31; the keys stay on the device and only the sorted copy comes back"""
    key, perms = window_case(n)
    val = np.arange(n, dtype=np.uint32)
    tk0, tv0 = torch.from_numpy(key.view(np.int32).copy()).to("cuda:0"), torch.from_numpy(val.view(np.int32)).to("cuda:0")
    bad = []
    for (first_bit, bits), perm in perms.items():
        tk, tv = tk0.clone(), tv0.clone()
        torch.cuda.synchronize()
        api.sort_pairs_device(tk.data_ptr(), tv.data_ptr(), n, first_bit, bits, mdb, ctx)
        ko, vo = tk.cpu().numpy().view(np.uint32), tv.cpu().numpy().view(np.uint32)
        if not (np.array_equal(vo, perm.astype(np.uint32)) and np.array_equal(ko, key[perm])):
            bad.append((first_bit, bits))
    assert not bad, "windows (first_bit, bits) sorted wrongly with digits <= %d at n = %d: %s" % (mdb, n, bad[:40])


@pytest.mark.parametrize("n", [4097, 8191])
@pytest.mark.parametrize("name,first_bit,bits,mdb", CALLERS, ids=[c[0] for c in CALLERS])
def test_pairs_callers_windows(ctx, name, first_bit, bits, mdb, n):
    key, perms = window_case(n)
    check_pairs(ctx, key, first_bit, bits, mdb, perm=perms[(first_bit, bits)])


@pytest.mark.parametrize("mdb", [8, 9, 10])
def test_wide_every_width(ctx, mdb):
    """bits 0..64 at n = 4097: the digits of a pass lie in lo, across the two words, in hi"""
    rs = np.random.RandomState(64 + mdb)
    lo, hi = u32(rs, 4097), u32(rs, 4097)
    for bits in range(0, 65):
        check_wide(ctx, lo, hi, bits, mdb)


# ---- sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", PAIR_SIZES)
def test_pairs_sizes(ctx, n):
    rs = np.random.RandomState(n % 100003)
    key = u32(rs, n)
    for first_bit, bits, mdb in PAIR_SIZE_WINDOWS:
        check_pairs(ctx, key, first_bit, bits, mdb)
    if n <= 8193:
        for _, first_bit, bits, mdb in CALLERS:
            check_pairs(ctx, key, first_bit, bits, mdb)


@pytest.mark.parametrize("n", WIDE_SIZES)
def test_wide_sizes(ctx, n):
    rs = np.random.RandomState(n % 100003)
    lo, hi = u32(rs, n), u32(rs, n)
    for bits in WIDE_SIZE_BITS:
        check_wide(ctx, lo, hi, bits, 9 if bits in (33, 60) else 10)


def test_values_are_carried_not_recomputed(ctx):
    rs = np.random.RandomState(5)
    n = 3 * 4096 + 37
    key, val = u32(rs, n) & np.uint32(0x0003FFFF), u32(rs, n)          # (18 bits over 12 325 keys: equal keys do occur)
    check_pairs(ctx, key, 0, 27, 9, val=val)
    check_pairs(ctx, key, 3, 15, 8, val=val)
    lo, hi = u32(rs, n) & np.uint32(0xFF), u32(rs, n) & np.uint32(0x1F)
    check_wide(ctx, lo, hi, 37, 9, val=val)


# ---- key distributions, each at a ragged size --------------------------------------------------------------------------------

def digits(kind, n, bits, rs):
    nbins, i = 1 << bits, np.arange(n, dtype=np.uint64)
    if kind == "uniform":
        return rs.randint(0, nbins, n).astype(np.uint64)
    if kind == "all-equal":
        return np.full(n, nbins - 1, dtype=np.uint64)
    if kind == "one-per-wave":                   # the 64 keys of a wave share a digit: the histogram adds 64 at once; the last wave is ragged
        return (i // np.uint64(64) * np.uint64(7)) % np.uint64(nbins)
    if kind == "ascending":
        return i * np.uint64(nbins) // np.uint64(n)
    if kind == "descending":
        return np.uint64(nbins - 1) - i * np.uint64(nbins) // np.uint64(n)
    assert kind == "all-but-three"
    d = np.full(n, nbins // 2, dtype=np.uint64)
    d[0], d[n // 2], d[n - 1] = nbins - 1, 0, nbins // 2 - 1
    return d


KINDS = ["uniform", "all-equal", "one-per-wave", "ascending", "descending", "all-but-three"]
DIST_N = [3 * 4096 + 37, 2 * 4096 + 64 * 5]      # a last wave of 37 keys; whole waves only, a last chunk of 5


@pytest.mark.parametrize("kind", KINDS)
def test_pairs_distributions(ctx, kind):
    """the window's digits follow `kind`, the bits outside the window are random"""
    for n in DIST_N:
        for first_bit, bits, mdb in [(0, 8, 8), (7, 10, 10), (23, 9, 9), (26, 6, 8), (11, 3, 9), (2, 27, 9), (12, 20, 10)]:
            rs = np.random.RandomState(first_bit * 64 + bits)
            window = np.uint32(((1 << bits) - 1) << first_bit)
            key = (u32(rs, n) & ~window) | (digits(kind, n, bits, rs) << np.uint64(first_bit)).astype(np.uint32)
            check_pairs(ctx, key, first_bit, bits, mdb)
            if kind == "all-equal":              # the window constant, the outside bits random: nothing may move
                ko, vo = sort_pairs(ctx, key, np.arange(n, dtype=np.uint32), first_bit, bits, mdb)
                assert np.array_equal(ko, key) and np.array_equal(vo, np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("kind", KINDS)
def test_wide_distributions(ctx, kind):
    """the top digit of the window follows `kind` -- in lo, across the words, in hi --, the bits below it are random or zero"""
    for n in [3 * 2048 + 37, 2 * 4096 + 64 * 5]:
        for bits, top, mdb, low_random in [(9, 9, 9, False), (30, 10, 10, True), (37, 9, 10, False), (37, 9, 10, True), (64, 9, 10, False), (50, 8, 8, True)]:
            rs = np.random.RandomState(bits)
            k = digits(kind, n, top, rs) << np.uint64(bits - top)
            if low_random and bits > top:
                k |= rs.randint(0, 1 << 62, n, dtype=np.uint64) & np.uint64((1 << (bits - top)) - 1)
            if bits < 64:                        # bits above the window: random, and they must not matter
                k |= rs.randint(0, 1 << 62, n, dtype=np.uint64) << np.uint64(bits)
            lo, hi = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32), (k >> np.uint64(32)).astype(np.uint32)
            check_wide(ctx, lo, hi, bits, mdb)
            if kind == "all-equal" and not low_random:
                lo_o, hi_o, vo = sort_wide(ctx, lo, hi, np.arange(n, dtype=np.uint32), bits, mdb)
                assert np.array_equal(lo_o, lo) and np.array_equal(hi_o, hi) and np.array_equal(vo, np.arange(n, dtype=np.uint32))


# ---- arguments, and the context around the hooks ---------------------------------------------------------------------------

def test_argument_errors_leave_the_arrays_and_the_context_alone(ctx):
    rs = np.random.RandomState(9)
    n = 5000
    key, val = u32(rs, n), u32(rs, n)
    tk, pk, hk = _guarded(key, 1)
    tv, pv, hv = _guarded(val, 2)
    tw, pw, hw = _guarded(val, 3)
    torch.cuda.synchronize()
    lib, h = ctx.lib, ctx.h
    for first_bit, bits in [(0, 33), (1, 32), (32, 1), (31, 2), (16, 17), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF), (33, 0)]:
        assert lib.bce_hip_sort_pairs_device(h, pk, pv, n, first_bit, bits, 9) == E_ARG, (first_bit, bits)
        assert lib.bce_hip_sort_pairs_device(h, pk, pv, 0, first_bit, bits, 9) == E_ARG, (first_bit, bits)
    assert lib.bce_hip_sort_pairs_device(None, pk, pv, n, 0, 8, 8) == E_ARG
    assert lib.bce_hip_sort_pairs_device(h, None, pv, n, 0, 8, 8) == E_ARG
    assert lib.bce_hip_sort_pairs_device(h, pk, None, 1, 0, 8, 8) == E_ARG
    assert lib.bce_hip_sort_wide_device(h, pk, pv, pw, n, 65, 9) == E_ARG
    assert lib.bce_hip_sort_wide_device(None, pk, pv, pw, n, 40, 9) == E_ARG
    for nulled in range(3):
        p = [pk, pv, pw]
        p[nulled] = None
        assert lib.bce_hip_sort_wide_device(h, p[0], p[1], p[2], n, 40, 9) == E_ARG
    # successes that touch nothing: no pairs (null pointers allowed), one pair, no bits
    assert lib.bce_hip_sort_pairs_device(h, None, None, 0, 0, 32, 8) == 0
    assert lib.bce_hip_sort_wide_device(h, None, None, None, 0, 64, 8) == 0
    assert lib.bce_hip_sort_pairs_device(h, pk, pv, 1, 0, 32, 8) == 0
    assert lib.bce_hip_sort_wide_device(h, pk, pv, pw, 1, 64, 8) == 0
    assert lib.bce_hip_sort_pairs_device(h, pk, pv, n, 32, 0, 8) == 0
    assert lib.bce_hip_sort_wide_device(h, pk, pv, pw, n, 0, 8) == 0
    assert np.array_equal(_back(tk, hk, n, "keys"), key) and np.array_equal(_back(tv, hv, n, "values"), val)
    assert np.array_equal(_back(tw, hw, n, "third"), val)
    # a digit width outside 1..10 counts as 8, as for the sorter's callers
    for mdb in (0, 11, 8):
        check_pairs(ctx, key, 4, 21, mdb)
    check_wide(ctx, key, val, 47, 9)


def test_hooks_between_the_stages_leave_the_archive_the_oracles():
    data = bce_amd.synth_text(31, 150001)
    want = oracle.compress(data.tobytes())
    rs = np.random.RandomState(3)
    key = u32(rs, 20000)
    a = torch.from_numpy(rs.randint(0, 256, 70001).astype(np.uint8)).to("cuda:0")
    b = a.clone()
    b[60000] ^= 0x10
    c = api._Ctx(0)
    try:
        def hooks():
            check_pairs(c, key, 0, 27, 9)
            check_pairs(c, key, K4_SHIFT, K4_BITS, 10)
            check_wide(c, key, key[::-1].copy(), 45, 9)
            torch.cuda.synchronize()
            assert api.compare_device(a.data_ptr() + 1, b.data_ptr() + 1, 70000, c) == 59999
            assert api.compare_device(a.data_ptr(), b.data_ptr(), 60000, c) is None

        hooks()
        c.check(c.lib.bce_hip_load_host(c.h, data.ctypes.data, len(data)), "bce_hip_load_host")
        hooks()
        off = C.c_uint32()
        c.check(c.lib.bce_hip_bwt(c.h, C.byref(off)), "bce_hip_bwt")
        hooks()
        c.check(c.lib.bce_hip_build_planes(c.h, None), "bce_hip_build_planes")
        hooks()
        c.check(c.lib.bce_hip_encode(c.h), "bce_hip_encode")
        hooks()
        assert bytes(api.archive_of(c)) == want
        assert api.decompress_device(want, ctx=c) == data.tobytes()
        hooks()
    finally:
        c.close()
