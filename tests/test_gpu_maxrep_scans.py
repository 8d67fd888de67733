"""GPU: the launches behind bce_hip_maximal_repeats alone, through the hook bce_hip_maxrep_of_arrays_device, on synthetic LCP arrays
and preceding bytes that put intervals, their representatives, the changes of the BWT and the candidates across any block (B = 2048
rows) and any pass (P = 256 blocks) of the one-workgroup kernels: the searches in the block trees and through the top tree, the
prefix count's carry, the histogram, the candidates' offsets and the stable 64-bit sort, with the launches and geometry of the real
call.  The arrays' intervals have a closed form, which is checked against the stack reference of tests/maxrep_ref.py (itself
checked against a brute force in tests/test_maxrep_cpu.py) at the sizes a Python loop can take."""
import ctypes as C

import numpy as np
import pytest
import torch

from bce_amd import api

import maxrep_ref as ref

pytestmark = pytest.mark.gpu
E_ARG = -1
B = ref.BLOCK
P = ref.PASS                                   # 524 288
GRID = (1, 2, 2047, 2048, 2049, 4097, P - 1, P + 1, 2 * P + 1)
GUARD = -0x21524111                            # 0xDEADBEEF as an int32
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()
    torch.cuda.empty_cache()


def _guarded(words):
    """The words as int32 at element 1 of a device tensor -- 4-byte aligned and no more -- with guard words around them."""
    buf = torch.full((len(words) + 4,), GUARD, dtype=torch.int32, device=DEV)
    buf[1:1 + len(words)] = torch.from_numpy(np.asarray(words).astype(np.uint32).view(np.int32)).to(DEV)
    return buf, buf[1:1 + len(words)]


def _guarded_bytes(b):
    buf = torch.full((len(b) + 2,), 0xEE, dtype=torch.uint8, device=DEV)
    buf[1:1 + len(b)] = torch.from_numpy(np.asarray(b, dtype=np.uint8)).to(DEV)
    return buf, buf[1:1 + len(b)]


def _untouched(buf, words):
    got = buf.cpu().numpy()
    return got[0] == GUARD and (got[1 + len(words):] == GUARD).all() and np.array_equal(got[1:1 + len(words)].view(np.uint32), words)


# ---- arrays whose intervals are known: (lcp, l, p, q, r) with one entry per LCP interval, r its representative ---------------------

def _iv(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 4)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def _step(n):
    return max(1, -(-n // 4000))               # rows per stair, so that the values stay below 4096


def ascending(n):
    """Stairs upwards: the interval of value v runs from its first stair to the LAST row; deep nesting, one shared end."""
    s = _step(n)
    lcp = np.zeros(n, dtype=np.uint32)
    lcp[1:] = 1 + (np.arange(1, n) - 1) // s
    v = np.arange(1, int(lcp.max()) + 1 if n > 1 else 1)
    first = 1 + (v - 1) * s
    return lcp, v, first - 1, np.full(len(v), n), first


def descending(n):
    """Stairs downwards: every interval starts in row 0 and ends where the next lower stair begins; one shared first row."""
    s = _step(n)
    lcp = np.zeros(n, dtype=np.uint32)
    if n > 1:
        H = 1 + (n - 2) // s
        lcp[1:] = H - (np.arange(1, n) - 1) // s
        v = np.arange(1, H + 1)
        first = 1 + (H - v) * s                # the first row of value v
        q = np.where(v > 1, first + s, n)
        return lcp, v, np.zeros(H, dtype=np.int64), np.minimum(q, n), first
    return lcp, *_iv([])


def mountain(n):
    """Up to the middle and down again: the rows of value >= v lie around the middle, both ends are far from most of them."""
    s = _step(n // 2 + 1)
    lcp = np.zeros(n, dtype=np.uint32)
    r = np.arange(1, n)
    lcp[1:] = 1 + np.minimum(r - 1, n - 1 - r) // s
    v = np.arange(1, int(lcp.max()) + 1 if n > 1 else 1)
    lo, hi = 1 + (v - 1) * s, n - 1 - (v - 1) * s
    return lcp, v, lo - 1, np.where(v > 1, hi + 1, n), lo


def plateau(n, value=77):
    """One value from row 1000 to row n - 1000 (from row 1 to the last where n is small): one interval over every edge there is, and
    every row but one finds a row of its own value above it."""
    a, b = (1000, n - 1000) if n > 2001 else (1, n)
    lcp = np.zeros(n, dtype=np.uint32)
    lcp[a:b] = value
    return (lcp, *_iv([(value, a - 1, b, a)] if n > 1 else []))


def pairs(n, seed=5):
    """Rows 2i + 1 carry a value in 4 .. 7 and rows 2i carry 0: n // 2 intervals of two rows, every weight in one bin for every
    order, equal weights in every block."""
    lcp = np.zeros(n, dtype=np.uint32)
    odd = np.arange(1, n, 2)
    lcp[odd] = np.random.RandomState(seed).randint(4, 8, len(odd))
    return lcp, lcp[odd].astype(np.int64), odd - 1, np.minimum(odd + 1, n), odd


FAMILIES = (ascending, descending, mountain, plateau, pairs)


def _bytes_for(n, kind):
    rs = np.random.RandomState(n + 17)
    if kind == "alternate":
        return (np.arange(n) % 2).astype(np.uint8)
    if kind == "sparse":                       # a change every few thousand rows: left-maximality differs from interval to interval
        return np.cumsum(rs.randint(0, 3000, n) == 0).astype(np.uint8)
    return rs.randint(0, 256, n).astype(np.uint8)


def expected(l, p, q, r, bw, min_len, max_len, order):
    """The whole list in the device's order from the intervals: (len, count, row) arrays and the info but for found."""
    D = np.concatenate(([0], np.cumsum(bw[1:] != bw[:-1]))).astype(np.int64)
    keep = (D[q - 1] - D[p] > 0) & (l >= min_len) if len(l) else np.zeros(0, dtype=bool)
    l, p, q, r = l[keep], p[keep], q[keep], r[keep]
    c = q - p
    w = (l << 31) | c if order == 0 else (c << 13) | l if order == 1 else l * (c - 1)
    idx = np.lexsort((r, -w))
    info = {"total": len(l), "capped": int(np.count_nonzero(l == max_len)), "bwt_runs": int(D[-1]) + 1}
    return l[idx], c[idx], p[idx], info


def _ask_and_check(ctx, name, lcp, ivs, bw, cases, limits=None):
    n = len(lcp)
    sa = np.random.RandomState(n + 1).permutation(n).astype(np.uint32)      # a position names its row
    lbuf, d_lcp = _guarded(lcp)
    sbuf, d_sa = _guarded(sa)
    bbuf, d_bw = _guarded_bytes(bw)
    torch.cuda.synchronize()
    for min_len, max_len, order in cases:
        l, c, p, info = expected(*ivs, bw, min_len, max_len, order)
        total = info["total"]
        for limit in limits or sorted(set(v for v in (1, 2, 1000, total - 1, total, total + 1) if 1 <= v <= api.TOP_MAX)):
            got, ginfo = api.maxrep_of_arrays_device(d_lcp.data_ptr(), n, d_sa.data_ptr(), d_bw.data_ptr(), min_len, max_len, order, limit, ctx)
            want = min(limit, total)
            assert ginfo == dict(info, found=want) and len(got) == want, (name, n, min_len, max_len, order, limit, ginfo, info)
            ok = np.array_equal(got["len"], l[:want]) and np.array_equal(got["count"], c[:want]) and np.array_equal(got["row"], p[:want])
            if not ok:
                e = int(np.flatnonzero((got["len"] != l[:want]) | (got["count"] != c[:want]) | (got["row"] != p[:want]))[0])
                raise AssertionError((name, n, min_len, max_len, order, limit, e, got[e], int(l[e]), int(c[e]), int(p[e])))
            assert np.array_equal(got["pos"], sa[p[:want]]), (name, n, order, limit)
    got = bbuf.cpu().numpy()
    assert _untouched(lbuf, lcp) and _untouched(sbuf, sa) and got[0] == got[-1] == 0xEE and np.array_equal(got[1:-1], bw), (name, n)


def test_the_closed_forms_are_the_stack_reference():
    for n in (1, 2, 3, 2049, 4097, 131073):
        for fam in FAMILIES:
            lcp, l, p, q, r = fam(n)
            assert lcp[0] == 0 and lcp.max() <= 4096
            for kind in ("alternate", "sparse"):
                bw = _bytes_for(n, kind)
                D = np.concatenate(([0], np.cumsum(bw[1:] != bw[:-1])))
                want = sorted((int(a), int(c - b), int(b), int(d)) for a, b, c, d in zip(l, p, q, r) if D[c - 1] - D[b] > 0)
                assert sorted(ref.intervals(lcp, bw)) == want, (fam.__name__, n, kind)
    lcp, l, p, q, r = mountain(2 * P + 1)                                      # what the large sizes are for
    assert len(l) > 3000 and (p // B != (q - 1) // B).sum() > 3000 and ((q - p) > P).sum() > 1500
    assert len(pairs(2 * P + 1)[1]) == P > 256 * B - 1                          # candidates beyond one block and beyond one pass


@pytest.mark.parametrize("n", GRID)
def test_staircases_mountain_plateau_and_pairs(ctx, n):
    for fam in FAMILIES:
        lcp, *ivs = fam(n)
        top = int(lcp.max())
        for kind in ("alternate", "sparse", "random"):
            bw = _bytes_for(n, kind)
            cases = [(1, 4096, 0), (1, max(top, 1), 1), (2, 4096, 2)] if kind != "random" else [(max(1, top // 2), 4096, 0)]
            _ask_and_check(ctx, "%s, %s bytes" % (fam.__name__, kind), lcp, ivs, bw, cases)


def test_an_interval_that_starts_in_block_0_is_represented_in_block_1_and_ends_in_block_3(ctx):
    n = 4 * B + 1
    lcp = np.zeros(n, dtype=np.uint32)
    lcp[2041:2100] = 9                                                         # above the interval's value: its first rows do not represent it
    lcp[2100] = 5                                                              # the lowest row that carries 5
    lcp[2101:6200] = 7
    lcp[3000] = lcp[5000] = 5                                                  # further rows of 5: they find row 2100, or each other
    ivs = _iv([(9, 2040, 2100, 2041), (5, 2040, 6200, 2100), (7, 2100, 3000, 2101), (7, 3000, 5000, 3001), (7, 5000, 6200, 5001)])
    bw = _bytes_for(n, "alternate")
    assert sorted(ref.intervals(lcp, bw)) == sorted(zip(*(a.tolist() for a in (ivs[0], ivs[2] - ivs[1], ivs[1], ivs[3]))))
    assert 2040 // B == 0 and 2100 // B == 1 and 6199 // B == 3
    _ask_and_check(ctx, "across four blocks", lcp, ivs, bw, [(1, 4096, o) for o in range(3)])


@pytest.mark.parametrize("n", (4097, P + 1))
def test_one_change_of_the_preceding_byte_at_the_ends_of_an_interval_and_at_block_edges(ctx, n):
    """bw constant but for ONE change in row c: the plateau [p, q) is left-maximal exactly when p < c <= q - 1."""
    lcp, *ivs = plateau(n)
    p, q = int(ivs[1][0]), int(ivs[2][0])
    for c in (p - 1, p, p + 1, p + 2, B - 1, B, B + 1, 2 * B, n // 2, q - 2, q - 1, q, q + 1, n - 1) + ((P - 1, P) if n > P else ()):
        bw = np.zeros(n, dtype=np.uint8)
        bw[c:] = 1
        l, cnt, row, info = expected(*ivs, bw, 1, 4096, 0)
        assert info["total"] == (1 if p < c <= q - 1 else 0) and info["bwt_runs"] == 2, c
        _ask_and_check(ctx, "a change in row %d of [%d, %d)" % (c, p, q), lcp, ivs, bw, [(1, 4096, 0)], limits=(1, 5))
    bw = np.zeros(n, dtype=np.uint8)                                           # two changes outside, none inside
    bw[p:q] = 1
    assert expected(*ivs, bw, 1, 4096, 0)[3] == {"total": 0, "capped": 0, "bwt_runs": 3}
    _ask_and_check(ctx, "changes in rows p and q only", lcp, ivs, bw, [(1, 4096, 0)], limits=(3,))


def test_a_weight_of_two_to_the_32_goes_through_the_64_bit_key(ctx):
    n = 2 * P + 1
    lcp, *ivs = plateau(n, 4096)
    lcp[:] = 4096
    lcp[0] = 0
    ivs = _iv([(4096, 0, n, 1)])
    bw = _bytes_for(n, "sparse")
    assert ref.weight("gain", 4096, n) == 1 << 32
    _ask_and_check(ctx, "all words 4096", lcp, ivs, bw, [(1, 4096, 2), (4096, 4096, 0), (1, 4096, 1)], limits=(1, 2))
    # the same sort with keys on both sides of 2^32: by length, len 1 weighs 2^31 + count and len 2 weighs 2^32 + count
    lcp2, l, p, q, r = pairs(n)
    l = 1 + l % 2
    lcp2[r] = l
    lcp2[101:900002] = 4096                                                    # and one interval of 900 002 rows, from row 100 to row 900 002
    keep = ~((r > 100) & (r <= 900001))
    ivs = tuple(np.concatenate((a[keep], [b])) for a, b in zip((l, p, q, r), (4096, 100, 900002, 101)))
    bw = _bytes_for(n, "alternate")
    assert ref.weight("len", 1, 2) < 1 << 32 < ref.weight("len", 2, 2) and set(ivs[0].tolist()) == {1, 2, 4096}
    _ask_and_check(ctx, "one heavy repeat among light ones", lcp2, ivs, bw, [(1, 4096, 0), (1, 4096, 2)], limits=(1, 3, 300000))


def test_equal_weights_keep_the_order_of_their_rows_across_blocks_and_passes(ctx):
    n = 2 * P + 1
    lcp, l, p, q, r = pairs(n)
    lcp[lcp > 0] = 6                                                           # every weight the same: nothing to sort, all candidates
    bw = _bytes_for(n, "alternate")
    args = _device_args(lcp, bw)
    for limit in (1, 1000, P - 1, P, P + 1):
        got, info = api.maxrep_of_arrays_device(*args, 1, 4096, 0, limit, ctx)
        assert info == {"total": P, "capped": 0, "bwt_runs": n, "found": min(limit, P)}
        assert np.array_equal(got["row"], 2 * np.arange(min(limit, P))) and (got["len"] == 6).all() and (got["count"] == 2).all()


_KEEP = []


def _device_args(lcp, bw):
    """(ptr_lcp, n, ptr_sa, ptr_bw) of device copies that stay alive for the module."""
    n = len(lcp)
    d_lcp = torch.from_numpy(lcp.astype(np.uint32).view(np.int32)).to(DEV)
    d_sa = torch.arange(n, dtype=torch.int32, device=DEV)
    d_bw = torch.from_numpy(np.asarray(bw, dtype=np.uint8)).to(DEV)
    torch.cuda.synchronize()
    _KEEP[:] = [d_lcp, d_sa, d_bw]
    return d_lcp.data_ptr(), n, d_sa.data_ptr(), d_bw.data_ptr()


def test_the_hook_refuses_bad_arguments_before_any_device_call(ctx):
    words = torch.zeros(8, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    lib, p = ctx.lib, words.data_ptr()
    out = np.full(4, 7, dtype=api.MAXREP_DTYPE)
    info = api.MaxRepInfo(1, 2, 3, 4, 5)
    o, i = out.ctypes.data, C.byref(info)
    for args in ((None, 8, p, p, 1, 64, 0, 4, o, i), (p, 8, None, p, 1, 64, 0, 4, o, i), (p, 8, p, None, 1, 64, 0, 4, o, i), (p, 0, p, p, 1, 64, 0, 4, o, i),
                 (p, 1 << 31, p, p, 1, 64, 0, 4, o, i), (p, 8, p, p, 0, 64, 0, 4, o, i), (p, 8, p, p, 65, 64, 0, 4, o, i), (p, 8, p, p, 1, 4097, 0, 4, o, i),
                 (p, 8, p, p, 1, 64, 3, 4, o, i), (p, 8, p, p, 1, 64, 0, 0, o, i), (p, 8, p, p, 1, 64, 0, (1 << 20) + 1, o, i),
                 (p, 8, p, p, 1, 64, 0, 4, None, i), (p, 8, p, p, 1, 64, 0, 4, o, None)):
        assert lib.bce_hip_maxrep_of_arrays_device(ctx.h, *args) == E_ARG, args
    assert (out == np.full(4, 7, dtype=api.MAXREP_DTYPE)).all() and (info.total, info.capped, info.bwt_runs, info.found, info.reserved) == (1, 2, 3, 4, 5)
    got, ginfo = api.maxrep_of_arrays_device(p, 8, p, p, 1, 64, 0, 4, ctx)    # eight zeros: no interval, one run
    assert len(got) == 0 and ginfo == {"total": 0, "capped": 0, "bwt_runs": 1, "found": 0}
    got, ginfo = api.maxrep_of_arrays_device(p, 1, p, p, 1, 64, 0, 4, ctx)    # one row
    assert len(got) == 0 and ginfo == {"total": 0, "capped": 0, "bwt_runs": 1, "found": 0}
