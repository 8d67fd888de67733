"""GPU: K2 (k2_planes.hip) on bytes of the test's choosing, injected with bce_hip_set_bwt, against the definition in numpy:
plane j = bit j of the bytes in the order "stable sort by their low j bits".  Every plane bit, the zero counts, and rank1 at the
granule (96) and chunk (3072) boundaries, where the cumulative counts and the shuffled payload meet; sizes up to two chunks per
block; planes that are all ones, all zeros, or hold a single one in their last position."""
import numpy as np
import pytest

import bce_amd
from bce_amd import api

pytestmark = pytest.mark.gpu
GRANULE, CHUNK, MAXB = 96, 3072, 1024            # k2_planes.hip: positions per rank granule, per chunk; blocks (two chunks each beyond)
SIZES = [1, 11, 12, 13, 95, 96, 97, 3071, 3072, 3073, 6143, 6144, 6145, CHUNK * MAXB - 1, CHUNK * MAXB, CHUNK * MAXB + 1,
         2 * CHUNK * MAXB + 100]
CONTENTS = ["random", "zeros", "ones", "zeros-then-ff", "00-then-ones", "cycle"]


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def content(kind, n):
    if kind == "random":
        return np.frombuffer(np.random.RandomState(n % 65521).bytes(n), dtype=np.uint8).copy()
    if kind == "cycle":
        return (np.arange(n, dtype=np.uint32) & 0xFF).astype(np.uint8)
    b = np.full(n, 0xFF if kind in ("ones", "00-then-ones") else 0x00, dtype=np.uint8)
    if kind == "zeros-then-ff":
        b[n - 1] = 0xFF                              # every plane: a single one, in the last position
    if kind == "00-then-ones":
        b[0] = 0x00                                  # every plane: all ones but position 0
    return b


def reference_planes(b):
    """-> the eight planes as 0/1 bytes"""
    planes, cur = [], b
    for j in range(8):
        bit = (cur >> j) & 1
        planes.append(bit)
        cur = np.concatenate([cur[bit == 0], cur[bit == 1]])          # stable: zeros first, each side in its order
    return planes


def rank_queries(n):
    q = [np.arange(0, n + 2, step, dtype=np.int64) + d for step in (GRANULE, CHUNK) for d in (-1, 0, 1)]
    q += [np.array([0, n]), np.random.RandomState(n % 65521).randint(0, n + 1, 2000)]
    return np.unique(np.clip(np.concatenate(q), 0, n)).astype(np.uint32)


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("n", SIZES)
def test_planes_zeros_and_rank(ctx, n, kind):
    b = content(kind, n)
    ref = reference_planes(b)
    rf = bce_amd.RankFile(bwt=b, offset=0, ctx=ctx)
    assert rf.zeros == [int(n - p.sum(dtype=np.int64)) for p in ref]
    idx = rank_queries(n)
    for j in range(8):
        assert np.array_equal(rf.plane_bits(j), ref[j]), "plane %d" % j
        cum = np.concatenate([[0], np.cumsum(ref[j], dtype=np.int64)])
        got = rf.rank1(j, idx)
        wrong = np.nonzero(got != cum[idx])[0]
        assert wrong.size == 0, "rank1 of plane %d at %s: %s, expected %s" % (j, idx[wrong[:8]], got[wrong[:8]], cum[idx[wrong[:8]]])
