"""GPU: the suffix-array checker (kd_sufsort.hip through bce_hip_sufcheck / _device) against tests/sa_ref.py's check(): sound arrays
pass; every planted defect gives exactly the reference's reason and index, at the first and last rows, across a block of 2048 rows
and across one pass of the top-level walk (256 blocks); the lower stage and the lower row win; the refusals; and a check between
bce_hip_build_planes and bce_hip_encode leaves the archive alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
import oracle
import sa_ref
from bce_amd import api

pytestmark = pytest.mark.gpu
E_ARG = -1
DEV = "cuda:0"
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def raw(ctx, t, sa):
    """(status, reason, bad) of bce_hip_sufcheck on host arrays"""
    a = np.frombuffer(bytes(t), dtype=np.uint8)
    s = np.ascontiguousarray(sa).view(np.uint32)
    bad, reason = C.c_uint64(7), C.c_uint32(7)
    rc = ctx.lib.bce_hip_sufcheck(ctx.h, a.ctypes.data, s.ctypes.data, len(a), C.byref(bad), C.byref(reason))
    return rc, reason.value, bad.value


SMALL = [("n1", b"q"), ("n2", b"ba"), ("n3", b"aba"), ("abracadabra", b"abracadabra"), ("text255", oracle.synth_text(1, 255)),
         ("text256", oracle.synth_text(2, 256)), ("text257", oracle.synth_text(3, 257)), ("text2047", oracle.synth_text(4, 2047)),
         ("rand2048", oracle.synth_rand(5, 2048)), ("text2049", oracle.synth_text(6, 2049)), ("rand65537", oracle.synth_rand(3, 65537)),
         ("a5000", b"a" * 5000), ("ab4000", b"ab" * 4000), ("abc3333ab", b"abc" * 3333 + b"ab"), ("zeros", bytes(3000) + b"\x01\x00")]


@pytest.mark.parametrize("name,t", SMALL, ids=[c[0] for c in SMALL])
def test_sound_arrays_pass_and_every_defect_gets_the_references_verdict(ctx, name, t):
    sa = sa_ref.suffix_array(t)
    assert raw(ctx, t, sa) == (0, sa_ref.OK, U64_MAX)
    assert bce_amd.sufcheck(t, sa, ctx=ctx) is None
    for what, bad in sa_ref.mutations(t, sa):
        assert raw(ctx, t, bad) == (0,) + sa_ref.check(t, bad), (name, what)


@pytest.fixture(scope="module")
def big():
    """2^20 bytes of text and their suffix array: sorted on the GPU, and proven sorted by the reference's linear check"""
    t = oracle.synth_text(3, 1 << 20)
    sa = bce_amd.suffix_array(t)
    assert sa_ref.check(t, sa) == (sa_ref.OK, sa_ref.NONE)
    return t, sa


def test_defects_across_a_pass_of_the_top_level_walk(ctx, big):
    """1 048 576 rows are 512 blocks, two passes of the walk: defects at rows 524 287 / 524 288 and in the last block included."""
    t, sa = big
    assert raw(ctx, t, sa) == (0, sa_ref.OK, U64_MAX)
    names = []
    for what, bad in sa_ref.mutations(t, sa):
        assert raw(ctx, t, bad) == (0,) + sa_ref.check(t, bad), what
        names.append(what)
    assert "rows 524287 and 524288 swapped" in names and "entry n at row 524288" in names and "entry with bit 31 at row 1048575" in names


def test_the_lower_stage_and_the_lower_row_win(ctx, big):
    t, sa = big
    n = len(t)
    got = {what: raw(ctx, t, bad) for what, bad in sa_ref.mutations(t, sa) if " and " in what and "swapped" not in what}
    assert got["order at row 2 and range at the last row"] == (0, sa_ref.RANGE, n - 1)
    assert got["range at rows 3 and n - 2"] == (0, sa_ref.RANGE, 3)
    assert got["order at row 2 and a missing position"][1] == sa_ref.MISSING
    # two defects of one stage in different passes of the walk: the lower row, whichever block is reduced first
    m = sa.view(np.uint32).copy()
    m[[600000, 600001]] = m[[600001, 600000]]
    m[[1000, 1001]] = m[[1001, 1000]]
    want = sa_ref.check(t, m)
    assert want[0] == sa_ref.ORDER and want[1] in (1000, 1001, 1002) and raw(ctx, t, m) == (0,) + want


def test_past_two_passes_on_arrays_of_the_callers(ctx):
    """n = 2 * 524 288 + 1 equal bytes: the suffix array is n - 1 .. 0, written with arange; one defect in the last block (the third
    pass of the walk) each time, on device arrays."""
    n = 2 * sa_ref.PASS + 1
    t = np.full(n, 0x61, dtype=np.uint8)
    sound = np.arange(n - 1, -1, -1, dtype=np.int64).astype(np.uint32)
    d_t = torch.from_numpy(t).to(DEV)

    def run(arr):
        d_sa = torch.from_numpy(arr.view(np.int32)).to(DEV)
        torch.cuda.synchronize()
        rc, verdict = api.sufcheck_device(d_t.data_ptr(), d_sa.data_ptr(), n, ctx)
        assert rc == 0
        assert np.array_equal(d_sa.cpu().numpy().view(np.uint32), arr)     # the array is only read
        return verdict

    assert sa_ref.check(t, sound) == (sa_ref.OK, sa_ref.NONE) and run(sound) is None
    for edit in ("swap", "range", "twice"):
        m = sound.copy()
        if edit == "swap":
            m[[n - 2, n - 1]] = m[[n - 1, n - 2]]
        elif edit == "range":
            m[n - 1] = n
        else:
            m[n - 1] = m[n - 2]
        want = sa_ref.verdict(t, m)
        assert want is not None and (edit == "twice" or want[1] >= 2 * sa_ref.PASS - 1)
        assert run(m) == want, edit
    assert want == ("missing", 0)


def test_refusals_leave_the_outputs_alone(ctx):
    lib, h = ctx.lib, ctx.h
    a, sa = np.zeros(8, dtype=np.uint8), np.arange(8, dtype=np.uint32)
    A, S = a.ctypes.data, sa.ctypes.data
    bad, reason = C.c_uint64(77), C.c_uint32(77)
    B, R = C.byref(bad), C.byref(reason)
    for args in ((None, A, S, 8, B, R), (h, None, S, 8, B, R), (h, A, None, 8, B, R), (h, A, S, 8, None, R), (h, A, S, 8, B, None), (h, A, S, 0, B, R),
                 (h, A, S, 0x80000000, B, R), (h, A, S, 0xFFFFFFFF, B, R)):
        assert lib.bce_hip_sufcheck(*args) == E_ARG, args
        dev = (args[0], None if args[1] is None else 0x1000, None if args[2] is None else 0x2000) + args[3:]
        assert lib.bce_hip_sufcheck_device(*dev) == E_ARG, args
    assert bad.value == 77 and reason.value == 77
    with pytest.raises(ValueError):
        bce_amd.sufcheck(b"abc", np.arange(2, dtype=np.int32), ctx=ctx)


def test_a_check_between_the_planes_and_the_encode_changes_nothing(ctx):
    t = np.frombuffer(oracle.synth_text(14, 40000), dtype=np.uint8)
    fresh = bytes(bce_amd.compress(t))
    other = oracle.synth_rand(15, 9000)
    other_sa = sa_ref.suffix_array(other)
    rf = api.RankFile(t, ctx=ctx)                                          # load, K1, planes
    assert bce_amd.sufcheck(other, other_sa, ctx=ctx) is None
    assert bce_amd.sufcheck(other, other_sa[::-1].copy(), ctx=ctx) == sa_ref.verdict(other, other_sa[::-1].copy())
    assert rf.count(b"the") == t.tobytes().count(b"the")                   # the index still answers ...
    assert bytes(api.BCE().encode(rf)) == fresh                            # ... and the archive is a fresh context's
