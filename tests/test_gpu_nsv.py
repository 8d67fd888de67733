"""GPU: all nearest smaller values alone (bce_hip_nsv_device: the tree, top and solve launches of kd_self.hip with the geometry of
the real call) against closed forms and the stack of tests/lpf_ref.py: one block, its edges, several blocks, and past a power of two
and past 2048 blocks, where the tree over the blocks' minima has another level."""
import numpy as np
import pytest
import torch

from bce_amd import api

import lpf_ref as ref

pytestmark = pytest.mark.gpu
E_ARG = -1
B = 2048
NONE = 0xFFFFFFFF
SMALL = (1, 2, B - 1, B, B + 1, 2 * B + 1)
SIZES = SMALL + (3 * (1 << 20) + 5, (1 << 22) + 1)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _nsv(ctx, vals):
    """the hook on a numpy array of uint32 (or a CUDA int32 tensor) -> (psv, nsv) as int64 tensors on the device, NONE = 2^32 - 1;
    both outputs guarded by a word on either side"""
    d = vals if isinstance(vals, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vals, dtype=np.uint32).view(np.int32)).to(DEV)
    n = d.numel()
    out = torch.full((2, n + 2), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    assert api.nsv_device(d.data_ptr(), n, out[0, 1:].data_ptr(), out[1, 1:].data_ptr(), ctx) == 0
    assert bool((out[:, 0] == -7).all()) and bool((out[:, -1] == -7).all())
    return (out[0, 1:-1].to(torch.int64) & 0xFFFFFFFF), (out[1, 1:-1].to(torch.int64) & 0xFFFFFFFF)


def _same(got, want):
    assert got.shape == want.shape
    bad = torch.nonzero(got != want)
    assert bad.numel() == 0, (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def _idx(n):
    return torch.arange(n, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("n", SIZES)
def test_ascending_and_descending(ctx, n):
    r = _idx(n)
    none = torch.full_like(r, NONE)
    psv, nsv = _nsv(ctx, r.to(torch.int32))
    _same(psv, torch.where(r > 0, r - 1, none))
    _same(nsv, none)
    psv, nsv = _nsv(ctx, (n - 1 - r).to(torch.int32))
    _same(psv, none)
    _same(nsv, torch.where(r < n - 1, r + 1, none))


@pytest.mark.parametrize("n", SIZES)
def test_the_mountain_has_every_far_distance_once_on_each_side(ctx, n):
    """a[p] = 2 p + 1, a[m + p] = 2 (m - 1 - p), p < m: row p's smaller value below is row 2 m - 1 - p, row m + p's above is row
    m - 2 - p, so half the answers on each side lie outside the row's block, at every distance.  A mountain has 2 m rows: an odd n
    is rounded up."""
    m = (n + 1) // 2
    p = _idx(m)
    none = torch.full_like(p, NONE)
    psv, nsv = _nsv(ctx, torch.cat([2 * p + 1, 2 * (m - 1 - p)]).to(torch.int32))
    _same(psv, torch.cat([torch.where(p > 0, p - 1, none), torch.where(p < m - 1, m - 2 - p, none)]))
    _same(nsv, torch.cat([2 * m - 1 - p, torch.where(p < m - 1, m + p + 1, none)]))


@pytest.mark.parametrize("n", SIZES)
def test_sawtooth_of_descending_blocks_with_ascending_minima(ctx, n):
    """block b holds b * W + (W - 1 - i), i < W, W = 2048 (and a smaller W that straddles blocks): inside a tooth everything above
    is larger, so psv is the LAST row of the tooth before -- its minimum, always in the neighbouring block -- and nsv the next row."""
    for W in (B, 1000):
        r = _idx(n)
        b, i = r // W, r % W
        none = torch.full_like(r, NONE)
        psv, nsv = _nsv(ctx, (b * W + (W - 1 - i)).to(torch.int32))
        _same(psv, torch.where(b > 0, b * W - 1, none))
        _same(nsv, torch.where((i < W - 1) & (r < n - 1), r + 1, none))


@pytest.mark.parametrize("n", SIZES)
def test_equal_values_are_never_smaller(ctx, n):
    r = _idx(n)
    none = torch.full_like(r, NONE)
    for word in (0, 7, -1):                                               # (-1: 0xFFFFFFFF, the value of the padding leaves)
        psv, nsv = _nsv(ctx, torch.full((n,), word, dtype=torch.int32, device=DEV))
        _same(psv, none)
        _same(nsv, none)
    for run in (3, B, B + 1):                                             # runs of equal values, ascending: the row before the run; none below
        psv, nsv = _nsv(ctx, (r // run).to(torch.int32))
        _same(psv, torch.where(r >= run, (r // run) * run - 1, none))
        _same(nsv, none)
        psv, nsv = _nsv(ctx, ((n - 1 - r) // run).to(torch.int32))        # descending: the mirror image
        first = n - ((n - 1 - r) // run) * run                            # the first row of the next run
        _same(psv, none)
        _same(nsv, torch.where(first < n, first, none))


@pytest.mark.parametrize("n", SMALL + (5 * B + 77, 1 << 17))
def test_random_permutations_and_random_values_against_the_stack(ctx, n):
    rs = np.random.RandomState(n % 9973)
    for vals in (rs.permutation(n).astype(np.uint32), rs.randint(0, 50, n).astype(np.uint32), rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)):
        want = ref.ansv(vals)
        got = _nsv(ctx, vals)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy().astype(np.uint32), w)


def test_refused_arguments(ctx):
    d = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = d.data_ptr()
    assert api.nsv_device(None, 4, p, p, ctx) == E_ARG and api.nsv_device(p, 4, None, p, ctx) == E_ARG and api.nsv_device(p, 4, p, None, ctx) == E_ARG
    assert api.nsv_device(p, 0, p, p, ctx) == E_ARG and api.nsv_device(p, 1 << 31, p, p, ctx) == E_ARG
