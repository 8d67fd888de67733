"""GPU: counts and positions of patterns of byte classes (kd_classes.hip through bce_hip_count_classes / _locate_classes and their
_device forms, RankFile.count_classes / locate_classes, the tensor and archive wrappers) against the brute force of
tests/class_ref.py over the same text: counts, hit lists and the node count, cyclic and linear, on the smallest shapes at which the
wave's walk can go wrong; the budget; the locate's protocol; the states in which the calls are refused; and that nothing else in
the context moves."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container

import class_ref as ref
import count_ref
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
def ab():
    """n = 4096 over {a, b}, seeded: (text, a RankFile of it in a context of its own)."""
    text = bytes(np.random.RandomState(19).randint(97, 99, 4096).astype(np.uint8))
    c = api._Ctx(0)
    yield text, api.RankFile(text, ctx=c)
    c.close()


@pytest.fixture(scope="module")
def four():
    """n = 200 000 over 4 symbols, seeded: (text, a RankFile of it in a context of its own)."""
    text = bytes(np.random.RandomState(7).randint(97, 101, 200000).astype(np.uint8))
    c = api._Ctx(0)
    yield text, api.RankFile(text, ctx=c)
    c.close()


def _wide(masks):
    return int((np.unpackbits(masks.view(np.uint8), axis=1).sum(axis=1) > 1).sum()) if len(masks) else 0


def _check(rf, text, pats, cyclic, want_nodes=None):
    """count_classes and locate_classes of one batch against the brute force, everything within the default budget; -> the hits"""
    use = [p for p in pats if cyclic or len(p)]
    want = [ref.hits(text, p, cyclic) for p in use]
    counts, over, work = rf.count_classes(use, cyclic=cyclic, return_work=True)
    assert counts.dtype == np.uint64 and counts.shape == (len(use),) and over.dtype == bool and not over.any()
    assert counts.tolist() == [len(w) for w in want]
    nodes = want_nodes if want_nodes is not None else [ref.nodes(text, p) for p in use]
    assert work.tolist() == nodes                                        # exactly nodes(P), whatever the order of the walk
    got, over = rf.locate_classes(use, cyclic=cyclic)
    assert len(got) == len(use) and not over.any()
    for pos, w, p in zip(got, want, use):
        assert pos.dtype == np.uint32 and np.array_equal(pos, w), (len(p), cyclic)
    return int(counts.sum())


@pytest.mark.parametrize("text", near_ref.SMALL, ids=lambda t: "%s-%d" % (t[:4].hex(), len(t)))
def test_small_texts_are_the_brute_force(ctx, text):
    """Periodic ties and m > n, the empty pattern (cyclic only), an empty class, a byte the text lacks, one wide class at the first,
    a middle and the last position, 64 wide classes; bytes(range(256)) * 3 with the full class: a root interval with 256 different
    candidate bytes, so every lane's four candidates and the ballot's full width are used."""
    rf = api.RankFile(text, ctx=ctx)
    pats = ref.cases_for(text)
    assert _wide(pats[-1]) == 65 and _wide(pats[-2]) == 64
    with pytest.raises(ValueError):
        rf.count_classes(pats[-1:], cyclic=True)
    pats = pats[:-1]
    nodes = [ref.nodes(text, p) for p in pats]
    _check(rf, text, pats, True, nodes)
    _check(rf, text, pats, False, [v for p, v in zip(pats, nodes) if len(p)])
    assert rf.count_classes(np.zeros((0, 8), dtype=np.uint32), cyclic=True) == (len(text), False)
    with pytest.raises(ValueError):
        rf.count_classes(b"")
    with pytest.raises(ValueError):
        rf.locate_classes([b"a", b""])
    # one-member classes only: the exact search's answers
    cuts = [near_ref.cyclic_cut(text, s, m) for s in (0, len(text) // 2) for m in (1, 2, len(text), len(text) + 1)]
    for cyclic in (True, False):
        assert rf.count_classes([ref.exact(p) for p in cuts], cyclic=cyclic)[0].tolist() == rf.count(cuts, cyclic=cyclic).tolist()
        for got, want in zip(rf.locate_classes([ref.exact(p) for p in cuts], cyclic=cyclic)[0], rf.locate(cuts, cyclic=cyclic)):
            assert np.array_equal(got, want)


def test_class_sizes_on_both_sides_of_the_lane_boundaries(ctx):
    """1, 2, 63, 64, 65, 255 and 256 members, as a run of byte values that straddles 63 | 64 (lane 63 of q = 0, lane 0 of q = 1) and
    as a seeded scatter; the class at the pattern's right end (the root branches), in its middle, and twice in a row (a frame
    whose children open frames).  64 KiB of random bytes: every byte value has rows at the root."""
    n = 1 << 16
    text = bytes(np.random.RandomState(3).randint(0, 256, n).astype(np.uint8))
    rf = api.RankFile(text, ctx=ctx)
    rs = np.random.RandomState(8)
    pats = []
    for k in (1, 2, 63, 64, 65, 255, 256):
        for members in ([(62 + i) % 256 for i in range(k)], sorted(rs.permutation(256)[:k].tolist())):
            at = int(rs.randint(0, n - 8))
            left, right = [[c] for c in text[at:at + 2]], [[c] for c in text[at + 3:at + 4]]
            pats += [ref.masks_of(left + [members]), ref.masks_of(left + [members] + right), ref.masks_of([members, members])]
    for cyclic in (True, False):
        hits = _check(rf, text, pats, cyclic)
    assert hits > 100000


def test_stack_depth_on_a_binary_text(ab):
    """[ab]{12}: thousands of nodes and every frame level down to the 12th; 64 two-member classes left of, and right of, three
    exact ones, left of twelve full ones, and in between exact ones -- most branches die early: one member of a class is a byte the
    text lacks, or the exact classes in between thin the intervals; 65 wide classes and 4097 classes are refused by the kernel,
    4096 are served."""
    text, rf = ab
    twelve = api.compile_classes(b"[ab]{12}")
    assert ref.nodes(text, twelve) > 5000 and _wide(twelve) == 12
    dying = lambda cut: [[c, 0x78] for c in cut]                         # noqa: E731  (two members, one of which the text lacks)
    left = ref.masks_of(dying(text[200:264]) + [[c] for c in text[264:267]])
    right = ref.masks_of([[c] for c in text[100:103]] + dying(text[103:167]))
    both = ref.masks_of(dying(text[912:964]) + [[c] for c in text[964:968]] + [[97, 98]] * 12)
    mixed = ref.masks_of([m for c in near_ref.cyclic_cut(text, 500, 64) for m in ([97, 98], [c])])
    assert all(ref.nodes(text, p) <= api.CLASS_MAX_NODES for p in (left, right, both, mixed))
    assert [_wide(p) for p in (left, right, both, mixed)] == [64] * 4
    pats = [twelve, left, right, both, mixed, api.compile_classes(b"a[ab]{11}b"), api.compile_classes(b"[ab]{13}a{2}")]
    for cyclic in (True, False):
        hits = _check(rf, text, pats, cyclic)
    assert hits > 4096
    lib, c, a = rf._c.lib, rf._c, C.addressof
    out, status, total = (C.c_uint64 * 2)(7, 7), (C.c_uint32 * 1)(7), C.c_uint64(0)
    for masks, word in ((ref.wide_run(text, 65), b"more than 64"), (np.tile(ref.exact(b"a"), (4097, 1)), b"4096")):
        masks = np.ascontiguousarray(masks)
        off = (C.c_uint64 * 2)(0, len(masks))
        assert lib.bce_hip_count_classes(c.h, masks.ctypes.data, a(off), 1, 0, a(out), None, a(status)) == E_ARG and word in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_classes(c.h, masks.ctypes.data, a(off), 1, 0, 0, a(out), a(status), None, 0, C.byref(total)) == E_ARG
        d_mask, d_off = torch.from_numpy(masks.view(np.int32)).to("cuda:0"), torch.tensor([0, len(masks)], dtype=torch.int64, device="cuda:0")
        d_out, d_st = torch.zeros(2, dtype=torch.int64, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(api.BceError) as e:
            rf.count_classes_device(d_mask.data_ptr(), d_off.data_ptr(), 1, d_out.data_ptr(), d_st.data_ptr())
        assert e.value.status == E_ARG
        with pytest.raises(api.BceError) as e:
            rf.locate_classes_device(d_mask.data_ptr(), d_off.data_ptr(), 1, d_out.data_ptr(), d_st.data_ptr(), None, 0)
        assert e.value.status == E_ARG
    longest = np.ascontiguousarray(np.tile(ref.exact(b"a"), (4096, 1)))
    assert rf.count_classes(longest, cyclic=True) == (0, False)
    assert rf.count_classes(twelve, cyclic=True)[0] == ref.count(text, twelve)          # the context stays usable


def test_the_budget_is_exact_reported_and_per_pattern(ab, four):
    """max_nodes = nodes(P): complete; nodes(P) - 1: over, count 0, no positions, work above the budget.  A batch that mixes both
    returns the full answers of the patterns within budget.  `.{4}` on 200 000 bytes at a budget of 16 stops at once."""
    text, rf = ab
    pats = [api.compile_classes(e) for e in (b"[ab]{12}", b".[ab]{5}a", b"ab[ab]ba", b"abba", b".", b"[ab]{9}[^a]")]
    pats.append(ref.masks_of([[97, 98]] * 10 + [[c, 0x78] for c in text[700:754]]))       # 64 wide classes
    for p in pats:
        want, hits = ref.nodes(text, p), ref.hits(text, p)
        assert want > 1
        assert rf.count_classes(p, cyclic=True, max_nodes=want, return_work=True) == (len(hits), False, want)
        count, over, work = rf.count_classes(p, cyclic=True, max_nodes=want - 1, return_work=True)
        assert (count, over) == (0, True) and want - 1 < work <= want
        pos, over = rf.locate_classes(p, cyclic=True, max_nodes=want)
        assert not over and np.array_equal(pos, hits)
        for cyclic in (True, False):
            pos, over = rf.locate_classes(p, cyclic=cyclic, max_nodes=want - 1)
            assert over and len(pos) == 0
    # mixed: the budget of the third pattern; the first two are over it, the others within
    nodes = [ref.nodes(text, p) for p in pats]
    budget = nodes[2]
    counts, over, work = rf.count_classes(pats, cyclic=True, max_nodes=budget, return_work=True)
    assert over.tolist() == [v > budget for v in nodes] and 0 < int(over.sum()) < len(pats)
    assert counts.tolist() == [0 if o else ref.count(text, p) for p, o in zip(pats, over)]
    assert all(w == v if not o else w > budget for w, v, o in zip(work.tolist(), nodes, over))
    for cyclic in (True, False):
        got, over2 = rf.locate_classes(pats, cyclic=cyclic, max_nodes=budget)
        assert over2.tolist() == over.tolist()
        for pos, p, o in zip(got, pats, over):
            assert np.array_equal(pos, ref.hits(text, p, cyclic) if not o else np.zeros(0, dtype=np.uint32))
    for bad in (0, -1, api.CLASS_MAX_NODES + 1):
        with pytest.raises(ValueError):
            rf.count_classes(pats[0], max_nodes=bad)
    assert rf.count_classes(pats[0], max_nodes=api.CLASS_MAX_NODES) == (ref.count(text, pats[0], cyclic=False), False)
    # the walk stops within one expansion and one finish of crossing the budget
    text4, rf4 = four
    dots = api.compile_classes(b".{4}")
    count, over, work = rf4.count_classes(dots, max_nodes=16, return_work=True)
    assert (count, over) == (0, True) and 16 < work <= 16 + 4 * 4             # (a complete walk would count all 340)
    assert rf4.count_classes(dots, return_work=True) == (len(text4) - 3, False, 4 + 16 + 64 + 256)
    # a tree far larger than the budget: the walk is over within 256 m steps of crossing it, long before the tree's end
    eight = api.compile_classes(b".{8}")
    whole = ref.nodes(text4, eight)
    assert sum(4 ** j for j in range(1, 9)) >= whole > api.CLASS_MAX_NODES
    for budget in (16, 1000, 20000):
        count, over, work = rf4.count_classes(eight, max_nodes=budget, return_work=True)
        assert (count, over) == (0, True) and budget < work <= budget + 256 * 8 < whole // 3
        pos, over = rf4.locate_classes(eight, cyclic=True, max_nodes=budget)
        assert over and len(pos) == 0


@pytest.mark.parametrize("npat", (1, 4, 5, 257))
def test_workgroup_shapes(ab, npat):
    """One wave per pattern, four patterns a workgroup: a lone wave, a full workgroup, one wave into the next, 65 workgroups."""
    text, rf = ab
    kinds = [api.compile_classes(e) for e in (b"ab[ab]{3}", b"abab", b".{3}b", b"[ab]{10}", b"b.a.b", b"[^a]b", b"a{5}[ab]")]
    want = [(ref.hits(text, p, False), ref.nodes(text, p)) for p in kinds]
    pats = [kinds[i % len(kinds)] for i in range(npat)]
    counts, over, work = rf.count_classes(pats, return_work=True)
    assert not over.any() and counts.tolist() == [len(want[i % len(kinds)][0]) for i in range(npat)]
    assert work.tolist() == [want[i % len(kinds)][1] for i in range(npat)]
    got, over = rf.locate_classes(pats)
    assert not over.any() and all(np.array_equal(g, want[i % len(kinds)][0]) for i, g in enumerate(got))


def test_locate_reads_narrow_and_wide_intervals_and_drops_hits_across_the_end(four):
    """One full class in front of exact cuts of 3, 5 and 10 bytes: answer intervals of hundreds of rows (the wave reads them
    together), of 9 .. 64 rows and of 8 rows or fewer (their own lane reads them); patterns cut across the text's end, whose hits
    there the linear mode drops."""
    text, rf = four
    n = len(text)
    rs = np.random.RandomState(31)
    pats = []
    for m in (3, 5, 10):
        for at in rs.randint(0, n - 16, 6).tolist():
            pats.append(ref.masks_of([ref.ANY] + [[c] for c in text[at:at + m]]))
            pats.append(ref.masks_of([[c] for c in text[at:at + m]] + [[97, 99]]))
    pats += [ref.masks_of([[c] for c in text[-3:]] + [ref.ANY] + [[c] for c in text[1:3]]), ref.masks_of([ref.ANY] + [[c] for c in text[-1:] + text[:2]])]
    rows = [len(ref.hits(text, p)) / 4 for p in pats[:-2:2]]
    assert min(rows) <= 8 and any(8 < r <= 64 for r in rows) and max(rows) > 64
    cyc = _check(rf, text, pats, True)
    lin = _check(rf, text, pats, False)
    across = sum(int((ref.hits(text, p) + len(p) > n).sum()) for p in pats)
    assert across >= 2 and cyc - lin == across


# ---- the protocol ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", (0, LINEAR))
def test_overflow_protocol_with_host_and_device_buffers(ctx, flags):
    text = bce_amd.synth_text(12, 4000).tobytes()
    pats = [api.compile_classes(e) for e in (b"t[aeiou]", b"e", b"[a-z] [a-z]", b"\xff", b"[^ -~]", b"th.")] + [ref.masks_of([[c] for c in text[-3:]] + [ref.ANY] + [[text[1]]])]
    flat = np.ascontiguousarray(np.concatenate(pats).reshape(-1))
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    want = [ref.hits(text, p, flags == 0) for p in pats]
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    want_pos = np.concatenate(want).tolist()
    tot, npat = want_off[-1], len(pats)
    assert tot > 100
    rf = api.RankFile(text, ctx=ctx)
    lib = ctx.lib

    def call(pos, cap):
        hits, status, total = np.full(npat + 1, 77, dtype=np.uint64), np.full(npat + 2, 9, dtype=np.uint32), C.c_uint64(123)
        rc = lib.bce_hip_locate_classes(ctx.h, flat.ctypes.data, off.ctypes.data, npat, 0, flags, hits.ctypes.data, status[1:].ctypes.data,
                                        None if pos is None else pos.ctypes.data, cap, C.byref(total))
        assert status[0] == 9 and status[-1] == 9
        return rc, hits.tolist(), status[1:-1].tolist(), total.value

    ok = [0] * npat
    assert call(None, 0) == (0, want_off, ok, tot)                        # the sizing call
    pos = np.full(tot + 2, GUARD, dtype=np.uint32)
    assert call(pos[1:], tot - 1) == (E_OVERFLOW, want_off, ok, tot)
    assert (pos == GUARD).all()                                           # nothing of the output written
    assert b"room for" in lib.bce_hip_last_error(ctx.h)
    assert call(pos[1:], tot) == (0, want_off, ok, tot)
    assert pos[0] == GUARD and pos[-1] == GUARD and pos[1:-1].tolist() == want_pos
    # the same with device buffers, slices at odd element offsets with guard words around them
    dev = "cuda:0"
    d_mask = torch.from_numpy(flat.view(np.int32)).to(dev)
    d_off = torch.zeros(npat + 4, dtype=torch.int64, device=dev)
    d_off[3:3 + npat + 1] = torch.from_numpy(off.astype(np.int64)).to(dev)
    hits_buf = torch.full((npat + 1 + 4,), -5, dtype=torch.int64, device=dev)
    st_buf = torch.full((npat + 4,), -6, dtype=torch.int32, device=dev)
    pos_buf = torch.full((tot + 6,), -7, dtype=torch.int32, device=dev)
    d_hits, d_st, d_pos = hits_buf[1:1 + npat + 1], st_buf[1:1 + npat], pos_buf[3:3 + tot]
    torch.cuda.synchronize()
    args = (d_mask.data_ptr(), d_off[3:].data_ptr(), npat, d_hits.data_ptr(), d_st.data_ptr())
    assert rf.locate_classes_device(*args, None, 0, cyclic=flags == 0) == tot
    assert d_hits.cpu().tolist() == want_off and d_st.cpu().tolist() == ok and (pos_buf == -7).all()
    total = C.c_uint64(0)
    rc = lib.bce_hip_locate_classes_device(ctx.h, args[0], args[1], npat, 0, flags, args[3], args[4], d_pos.data_ptr(), tot - 1, C.byref(total))
    assert rc == E_OVERFLOW and total.value == tot and d_hits.cpu().tolist() == want_off and (pos_buf == -7).all()
    assert rf.locate_classes_device(*args, d_pos.data_ptr(), tot, cyclic=flags == 0) == tot
    assert d_pos.cpu().tolist() == want_pos
    assert hits_buf[0].item() == -5 and (hits_buf[npat + 2:] == -5).all() and (pos_buf[:3] == -7).all() and (pos_buf[3 + tot:] == -7).all()
    assert st_buf[0].item() == -6 and (st_buf[npat + 1:] == -6).all()
    # count_classes_device: counts, verdicts and nodes, with and without the third array
    d_cnt = torch.full((npat + 2,), -3, dtype=torch.int64, device=dev)
    d_work = torch.full((npat + 2,), -4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rf.count_classes_device(args[0], args[1], npat, d_cnt[1:].data_ptr(), d_st.data_ptr(), d_work[1:].data_ptr())
    assert d_cnt[1:-1].cpu().tolist() == [ref.count(text, p) for p in pats] and d_cnt[0] == -3 and d_cnt[-1] == -3
    assert d_work[1:-1].cpu().tolist() == [ref.nodes(text, p) for p in pats] and d_work[0] == -4 and d_work[-1] == -4
    d_cnt[1:-1] = -3
    torch.cuda.synchronize()
    rf.count_classes_device(args[0], args[1], npat, d_cnt[1:].data_ptr(), d_st.data_ptr(), None, max_nodes=40)
    nodes = [ref.nodes(text, p) for p in pats]
    assert d_st.cpu().tolist() == [int(v > 40) for v in nodes] and 0 < sum(v > 40 for v in nodes) < npat
    assert d_cnt[1:-1].cpu().tolist() == [0 if v > 40 else ref.count(text, p) for p, v in zip(pats, nodes)]
    # decreasing offsets: found by the kernel; the context stays usable
    d_off[3 + 2] = d_off[3 + 4]
    torch.cuda.synchronize()
    for fn in (lambda: rf.locate_classes_device(*args, d_pos.data_ptr(), tot, cyclic=flags == 0),
               lambda: rf.count_classes_device(args[0], args[1], npat, d_cnt[1:].data_ptr(), d_st.data_ptr())):
        with pytest.raises(api.BceError) as e:
            fn()
        assert e.value.status == E_ARG and "offsets decrease" in str(e.value)
    assert np.array_equal(rf.locate_classes(pats[0], cyclic=flags == 0)[0], want[0])


def test_a_batch_of_more_than_2_31_rows_is_sized_exactly_and_refused(four):
    """The empty pattern owns all n rows: repeated until the batch passes 2^31 - 1 cyclic rows, the sizing call and the full call
    both come back with BCE_HIP_E_OVERFLOW, exact offsets and total, whatever cap is, and nothing of the positions written."""
    text, rf = four
    n, lib, c = len(text), rf._c.lib, rf._c
    npat = (1 << 31) // n + 1
    assert (npat - 1) * n <= (1 << 31) - 1 < npat * n
    off = np.zeros(npat + 1, dtype=np.uint64)
    masks = np.zeros(8, dtype=np.uint32)
    want = (np.arange(npat + 1, dtype=np.uint64) * np.uint64(n)).tolist()
    pos = np.full(4, GUARD, dtype=np.uint32)
    for out, cap in ((None, 0), (pos, 4)):
        hits, status, total = np.full(npat + 1, 77, dtype=np.uint64), np.full(npat, 9, dtype=np.uint32), C.c_uint64(123)
        rc = lib.bce_hip_locate_classes(c.h, masks.ctypes.data, off.ctypes.data, npat, 0, 0, hits.ctypes.data, status.ctypes.data,
                                        None if out is None else out.ctypes.data, cap, C.byref(total))
        assert rc == E_OVERFLOW and total.value == npat * n and hits.tolist() == want and not status.any()
        assert b"2^31 - 1" in lib.bce_hip_last_error(c.h) and (pos == GUARD).all()
    hits, status, total = np.zeros(npat, dtype=np.uint64), np.zeros(npat - 1, dtype=np.uint32), C.c_uint64(0)      # one pattern fewer: sized
    assert lib.bce_hip_locate_classes(c.h, masks.ctypes.data, off.ctypes.data, npat - 1, 0, 0, hits.ctypes.data, status.ctypes.data, None, 0,
                                      C.byref(total)) == 0 and total.value == (npat - 1) * n


def test_states_and_arguments_that_are_refused():
    text = bce_amd.synth_text(5, 20000)
    tb = text.tobytes()
    c = api._Ctx(0)
    try:
        lib, a = c.lib, C.addressof
        masks = np.ascontiguousarray(api.compile_classes(b"[eE] "))
        off = (C.c_uint64 * 2)(0, 2)
        hits, cnt, status, total = (C.c_uint64 * 2)(7, 7), (C.c_uint64 * 1)(7), (C.c_uint32 * 1)(7), C.c_uint64(5)
        largs = (c.h, masks.ctypes.data, a(off), 1, 0, LINEAR, a(hits), a(status), None, 0, C.byref(total))
        cargs = (c.h, masks.ctypes.data, a(off), 1, 0, a(cnt), None, a(status))
        assert lib.bce_hip_locate_classes(*largs) == E_STATE and b"holds no planes" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_classes_device(*largs) == E_STATE and lib.bce_hip_count_classes(*cargs) == E_STATE
        assert lib.bce_hip_count_classes_device(*cargs) == E_STATE
        for budget in (api.CLASS_MAX_NODES + 1, 0xFFFFFFFF):             # the budget is judged before the state
            assert lib.bce_hip_count_classes(*(cargs[:4] + (budget,) + cargs[5:])) == E_ARG
            assert lib.bce_hip_count_classes_device(*(cargs[:4] + (budget,) + cargs[5:])) == E_ARG
            assert lib.bce_hip_locate_classes(*(largs[:4] + (budget,) + largs[5:])) == E_ARG
            assert lib.bce_hip_locate_classes_device(*(largs[:4] + (budget,) + largs[5:])) == E_ARG
        fresh = bytes(bce_amd.compress(text))
        rf = api.RankFile(text, ctx=c)
        assert list(hits) == [7, 7] and list(cnt) == [7] and list(status) == [7]
        want = ref.hits(tb, masks, False)
        pos, over = rf.locate_classes(masks)
        assert not over and np.array_equal(pos, want) and len(want) > 100
        assert rf.locate_classes(b"e ", ignore_case=True)[0].tolist() == want.tolist() == rf.locate_classes("[Ee] ")[0].tolist()
        assert rf.count_classes(b"e ", ignore_case=True) == (len(want), False) and rf.count_classes(b"e ")[0] == rf.count(b"e ")
        # flag bits, null arrays, decreasing offsets
        for flags in (2, 3, 0x80000000):
            assert lib.bce_hip_locate_classes(*(largs[:5] + (flags,) + largs[6:])) == E_ARG
            assert lib.bce_hip_locate_classes_device(*(largs[:5] + (flags,) + largs[6:])) == E_ARG
        assert lib.bce_hip_count_classes(c.h, masks.ctypes.data, a(off), 1, 0, None, None, a(status)) == E_ARG
        assert lib.bce_hip_count_classes(c.h, masks.ctypes.data, a(off), 1, 0, a(cnt), None, None) == E_ARG
        assert lib.bce_hip_count_classes(c.h, masks.ctypes.data, None, 1, 0, a(cnt), None, a(status)) == E_ARG
        assert lib.bce_hip_count_classes(c.h, None, a(off), 1, 0, a(cnt), None, a(status)) == E_ARG
        assert lib.bce_hip_locate_classes(c.h, masks.ctypes.data, a(off), 1, 0, 0, None, a(status), None, 0, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate_classes(c.h, masks.ctypes.data, a(off), 1, 0, 0, a(hits), None, None, 0, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate_classes(c.h, masks.ctypes.data, a(off), 1, 0, 0, a(hits), a(status), None, 4, C.byref(total)) == E_ARG
        assert lib.bce_hip_locate_classes(c.h, masks.ctypes.data, a(off), 1, 0, 0, a(hits), a(status), None, 0, None) == E_ARG
        bad = (C.c_uint64 * 3)(0, 2, 1)
        assert lib.bce_hip_count_classes(c.h, masks.ctypes.data, a(bad), 2, 0, a(cnt), None, a(status)) == E_ARG and b"offsets decrease" in lib.bce_hip_last_error(c.h)
        # no patterns at all
        total.value, hits[0] = 5, 7
        assert lib.bce_hip_locate_classes(c.h, None, None, 0, 0, LINEAR, a(hits), None, None, 0, C.byref(total)) == 0 and total.value == 0 and hits[0] == 0
        assert lib.bce_hip_locate_classes_device(c.h, None, None, 0, 0, 0, None, None, None, 0, C.byref(total)) == 0
        assert lib.bce_hip_count_classes(c.h, None, None, 0, 0, None, None, None) == 0 and lib.bce_hip_count_classes_device(c.h, None, None, 0, 0, None, None, None) == 0
        got, over = rf.locate_classes([])
        assert got == [] and over.shape == (0,) and rf.count_classes([])[0].shape == (0,)
        # max_hits and limit: locate()'s rules
        with pytest.raises(ValueError, match=str(len(want))):
            rf.locate_classes(masks, max_hits=len(want) - 1)
        assert rf.locate_classes(masks, limit=7)[0].tolist() == want[:7].tolist()
        # nothing else in the context has moved: an encode after the queries gives the archive of a fresh context, and so does a compress
        assert bytes(api.BCE().encode(rf)) == fresh
        assert rf.count_classes(masks) == (len(want), False) and rf.count(b"e ") == tb.count(b"e ")
        assert bytes(bce_amd.compress(text, ctx=c)) == fresh
        # an injected BWT: planes, but no suffix array behind them -- counts work, positions do not
        bwt, row0 = count_ref.bwt_of_rotations(b"abracadabra")
        rf = api.RankFile(bwt=bwt, offset=row0, ctx=c)
        assert rf.count_classes(b"a[bc]", cyclic=True) == (ref.count(b"abracadabra", api.compile_classes(b"a[bc]")), False)
        assert lib.bce_hip_locate_classes(*largs) == E_STATE and b"no suffix array behind an injected BWT" in lib.bce_hip_last_error(c.h)
        assert lib.bce_hip_locate_classes_device(*largs) == E_STATE
        with pytest.raises(api.BceError) as e:
            rf.locate_classes(b"a[bc]", cyclic=True)
        assert e.value.status == E_STATE
        with pytest.raises(ValueError):
            rf.locate_classes(b"a[bc]")
        with pytest.raises(ValueError):
            rf.count_classes(b"a[bc]")
    finally:
        c.close()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def _split(offsets, positions, over, dev):
    assert offsets.dtype == torch.int64 and positions.dtype == torch.int32 and over.dtype == torch.bool
    assert offsets.device == dev and positions.device == dev and over.device == dev
    off = offsets.cpu().tolist()
    assert off[0] == 0 and off[-1] == positions.numel() and over.numel() == len(off) - 1
    pos = positions.cpu().tolist()
    return [pos[a:b] for a, b in zip(off, off[1:])], over.cpu().tolist()


def test_module_level_and_tensor_functions_on_a_slice_at_an_odd_offset(ctx):
    data = bce_amd.synth_text(17, 9000)
    big = torch.from_numpy(data).to("cuda:0")
    t = big[1237:1237 + 4099]
    tb = data[1237:1237 + 4099].tobytes()
    assert t.data_ptr() % 2 == 1
    exprs = [b"t[hH]e", b"[a-z]{3} ", b". .", ref.masks_of([[c] for c in tb[-4:]] + [ref.ANY] + [[c] for c in tb[1:3]]), b"[^ -~]", "é"]
    masks = [api._as_classes(e, False) for e in exprs]
    for cyclic in (False, True):
        want = [ref.hits(tb, p, cyclic).tolist() for p in masks]
        assert _split(*bce_amd.locate_classes_tensor(t, exprs, cyclic=cyclic, ctx=ctx), t.device) == (want, [False] * len(exprs))
        counts, over = bce_amd.count_classes_tensor(t, exprs, cyclic=cyclic, ctx=ctx)
        assert counts.tolist() == [len(w) for w in want] and not over.any()
        got, over = bce_amd.locate_classes(tb, masks, cyclic=cyclic)
        assert [g.tolist() for g in got] == want and not over.any()
        assert bce_amd.count_classes(tb, exprs, cyclic=cyclic)[0].tolist() == [len(w) for w in want]
    want = ref.hits(tb, api.compile_classes(b"the", ignore_case=True), False).tolist()
    assert _split(*bce_amd.locate_classes_tensor(t, b"the", ignore_case=True), t.device) == ([want], [False])   # a context of its own
    assert bce_amd.count_classes_tensor(t, b"the", ignore_case=True) == (len(want), False)
    nodes = ref.nodes(tb, masks[1])
    off, pos, over = bce_amd.locate_classes_tensor(t, exprs[:2], max_nodes=nodes - 1, ctx=ctx)       # the second pattern gives up
    assert over.tolist() == [False, True] and off.tolist() == [0, len(ref.hits(tb, masks[0], False)), len(ref.hits(tb, masks[0], False))]
    off, pos, over = bce_amd.locate_classes_tensor(t, [b"\xff\xfe", b"[\xf0-\xff]{3}"], ctx=ctx)      # nothing found: empty tensors
    assert off.tolist() == [0, 0, 0] and pos.numel() == 0 and over.tolist() == [False, False]
    off, pos, over = bce_amd.locate_classes_tensor(t, [], ctx=ctx)
    assert off.tolist() == [0] and pos.numel() == 0 and over.numel() == 0
    with pytest.raises(ValueError):
        bce_amd.locate_classes_tensor(t, b"", ctx=ctx)
    with pytest.raises(ValueError):
        bce_amd.locate_classes_tensor(t, b"a[", ctx=ctx)


def test_in_archive_on_a_plain_archive_and_across_a_block_boundary():
    data = bce_amd.synth_text(41, 10000).tobytes()
    dev = torch.device("cuda:0")
    plain = bytes(bce_amd.compress(data[:4000]))
    exprs = [b"t.e", b"[A-Z][a-z]", ref.masks_of([[c] for c in data[3995:4000]] + [ref.ANY] + [[c] for c in data[1:3]])]
    for cyclic in (False, True):
        want = [ref.hits(data[:4000], api._as_classes(e, False), cyclic).tolist() for e in exprs]
        assert _split(*bce_amd.locate_classes_in_archive(plain, exprs, cyclic=cyclic), dev) == (want, [False] * 3)
        assert bce_amd.count_classes_in_archive(plain, exprs, cyclic=cyclic)[0].tolist() == [len(w) for w in want]
    # a checked container of two blocks; a pattern placed across the block boundary, a full class on either side of it
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=2)
    table = container.block_table(blob)
    assert len(table) == 2 and all(e[3] is not None for e in table)
    cut = table[0][0]
    pats = [ref.masks_of([[c] for c in data[cut - 5:cut - 1]] + [ref.ANY, ref.ANY] + [[c] for c in data[cut + 1:cut + 5]]), api.compile_classes(b"the", ignore_case=True)]
    want = [ref.hits(data, p, False).tolist() for p in pats]
    assert cut - 5 in want[0]
    assert _split(*bce_amd.locate_classes_in_archive(blob, pats), dev) == (want, [False, False])
    assert bce_amd.count_classes_in_archive(blob, pats)[0].tolist() == [len(w) for w in want]
    assert bce_amd.count_classes_in_archive(blob, b"the", ignore_case=True) == (len(want[1]), False)
