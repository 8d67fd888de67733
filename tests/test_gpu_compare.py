"""GPU: the first-difference kernel (kd_compare.hip) alone, through bce_hip_compare_device, against numpy's first index of
a != b.  Both buffers lie inside larger allocations whose bytes around them differ between the two, so a read outside [0, m) shows
up as a difference that is not there.  Small sizes exhaustively at every alignment of `a` (its unaligned head runs here for the
first time); 48 MiB + 7 with differences at the lane, wave, unit-stride, chunk and grid-stride boundaries, alone and in pairs of
which the smaller must win."""
import ctypes as C

import numpy as np
import pytest
import torch

from bce_amd import api

pytestmark = pytest.mark.gpu
E_ARG = -1
PAD = 64                                         # bytes around the compared range (a multiple of 16: `a`'s alignment is its offset's)
LANES, PER_LANE, GRID = 256, 4, 2048             # kd_compare.hip: lanes per workgroup, 16-byte units per lane and pass, most workgroups
CHUNK = LANES * PER_LANE                         # units per workgroup and pass


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


class Pair:
    """m equal bytes at `a_off` / `b_off` bytes into two allocations; around them each byte of one is the other's complement."""

    def __init__(self, m, a_off, b_off, seed):
        r = np.frombuffer(np.random.RandomState(seed).bytes(PAD + m + PAD), dtype=np.uint8).copy()
        other = r ^ np.uint8(0xFF)
        other[PAD:PAD + m] = r[PAD:PAD + m]
        ha, hb = np.zeros(len(r) + 16, dtype=np.uint8), np.zeros(len(r) + 16, dtype=np.uint8)
        ha[a_off:a_off + len(r)] = r
        hb[b_off:b_off + len(r)] = other
        self.m = m
        self.ta, self.tb = torch.from_numpy(ha).to("cuda:0"), torch.from_numpy(hb).to("cuda:0")
        assert self.ta.data_ptr() % 16 == 0 and self.tb.data_ptr() % 16 == 0
        self.a0, self.b0 = a_off + PAD, b_off + PAD
        self.pa, self.pb = self.ta.data_ptr() + self.a0, self.tb.data_ptr() + self.b0
        self.head = min(m, -self.pa % 16)        # the kernel's split of [0, m): head bytes, 16-byte units, tail bytes
        self.units = (m - self.head) // 16
        self.tail = m - self.head - 16 * self.units

    def flip(self, positions):
        for i, p in enumerate(positions):        # (in `a` and in `b` by turns: whichever side holds the difference)
            t, base = (self.ta, self.a0) if (p + i) & 1 else (self.tb, self.b0)
            t[base + p:base + p + 1].bitwise_xor_(1 << (p % 8))

    def first_diff(self, ctx, positions=()):
        self.flip(positions)
        torch.cuda.synchronize()
        try:
            return api.compare_device(self.pa, self.pb, self.m, ctx)
        finally:
            self.flip(positions)                 # (the same flips again: equal once more)

    def unit(self, u, byte=0):
        assert 0 <= u < self.units
        return self.head + 16 * u + byte


@pytest.mark.parametrize("m", [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100])
def test_small_every_alignment_every_position(ctx, m):
    for a_off in range(16):
        for b_off in (0, 3):
            p = Pair(m, a_off, b_off, seed=m * 64 + a_off * 4 + b_off)
            assert p.head == (16 - a_off) % 16 or p.head == m
            assert p.first_diff(ctx) is None, (m, a_off, b_off)
            for pos in range(m):
                assert p.first_diff(ctx, [pos]) == pos, (m, a_off, b_off, pos)
            # two differences: the smaller one wins
            for lo, hi in [(0, m - 1), (m // 3, m // 2), (m // 2, m - 1)]:
                if lo < hi:
                    assert p.first_diff(ctx, [hi, lo]) == lo, (m, a_off, b_off, lo, hi)


LARGE_M = 48 * (1 << 20) + 7


@pytest.fixture(scope="module", params=[(0, 3), (5, 0)], ids=["a+0,b+3", "a+5,b+0"])
def large(request):
    a_off, b_off = request.param
    p = Pair(LARGE_M, a_off, b_off, seed=48 + a_off)
    assert p.head == (16 - a_off) % 16 and p.units > (GRID + 1) * CHUNK + CHUNK     # a second grid-stride pass, more than a chunk of it
    yield p
    del p


def boundary_units(p):
    return [0, 63, 64, 255, 256, 1023, 1024, (GRID - 1) * CHUNK + CHUNK - 1, GRID * CHUNK, p.units - 1]


def test_large_equal_and_single_differences(ctx, large):
    p = large
    assert p.first_diff(ctx) is None
    for u in boundary_units(p):
        for byte in (0, 3, 4, 15):
            assert p.first_diff(ctx, [p.unit(u, byte)]) == p.unit(u, byte), (u, byte)
    assert p.tail > 0
    for pos in list(range(p.head)) + list(range(p.m - p.tail, p.m)):
        assert p.first_diff(ctx, [pos]) == pos, pos


def test_large_pairs_the_smaller_wins(ctx, large):
    p = large
    last_first_pass, second_pass = (GRID - 1) * CHUNK, GRID * CHUNK          # workgroup 2047's first chunk; workgroup 0's second
    pairs = []
    for h in sorted({0, p.head - 1} if p.head else ()):                      # a head byte + any unit
        pairs += [(h, p.unit(u)) for u in (0, 1024, second_pass, p.units - 1)]
    for lane in (0, 77, 255):                                               # the last chunk of the first pass + the first of the second
        pairs += [(p.unit(last_first_pass + lane, 5), p.unit(second_pass + lane, 2)),
                  (p.unit(last_first_pass + 3 * LANES + lane), p.unit(second_pass + lane))]
    pairs += [(p.unit(second_pass + 7), p.unit(second_pass + CHUNK + 3)),     # two chunks of the second pass
              (p.unit(5), p.unit(second_pass + 5))]                         # workgroup 0's own two chunks
    for base in (0, 5 * CHUNK, second_pass):                                # two of one lane's four units
        for lane in (0, 77, 255):
            pairs += [(p.unit(base + 1 * LANES + lane, 9), p.unit(base + 3 * LANES + lane, 1)),
                      (p.unit(base + lane, 15), p.unit(base + 2 * LANES + lane)),
                      (p.unit(base + 2 * LANES + lane), p.unit(base + 3 * LANES + lane))]
    pairs += [(p.unit(u), p.m - 1 - t) for u in (0, 1023, second_pass, p.units - 1) for t in (0, p.tail - 1)]     # a unit + a tail byte
    pairs += [(p.m - p.tail, p.m - 1)]
    for u in (0, 64, second_pass + 1, p.units - 1):                         # two bytes of one unit, in different words
        pairs += [(p.unit(u, 2), p.unit(u, 9)), (p.unit(u, 7), p.unit(u, 12)), (p.unit(u, 0), p.unit(u, 15))]
    for lo, hi in pairs:
        assert lo < hi
        assert p.first_diff(ctx, [hi, lo]) == lo, (lo, hi)
        assert p.first_diff(ctx, [lo, hi]) == lo, (lo, hi)


def test_arguments(ctx):
    t = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    fd = C.c_uint64(7)
    lib, h, d = ctx.lib, ctx.h, t.data_ptr()
    assert lib.bce_hip_compare_device(h, None, None, 0, C.byref(fd)) == 0 and fd.value == (1 << 64) - 1      # n == 0: equal, pointers ignored
    fd.value = 7
    assert lib.bce_hip_compare_device(h, d, d + 1, 0, C.byref(fd)) == 0 and fd.value == (1 << 64) - 1
    fd.value = 7
    assert lib.bce_hip_compare_device(None, d, d, 16, C.byref(fd)) == E_ARG
    assert lib.bce_hip_compare_device(h, None, d, 16, C.byref(fd)) == E_ARG
    assert lib.bce_hip_compare_device(h, d, None, 16, C.byref(fd)) == E_ARG
    assert lib.bce_hip_compare_device(h, d, d, 16, None) == E_ARG
    assert fd.value == 7
    assert api.compare_device(d + 1, d + 2, 60, ctx) is None          # (zeros against zeros, a buffer against itself shifted)
    t[40] = 1
    torch.cuda.synchronize()
    assert api.compare_device(d + 1, d + 2, 60, ctx) == 38
