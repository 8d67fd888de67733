"""GPU: the self-parse's chain alone on synthetic lengths (bce_hip_self_parse_of_lpf_device: the mirrors, kd_parse's launches and the
turn of kd_self.hip with the geometry of the real call), past one block (2048 positions) and past one pass of the top kernel (256
blocks), against the chain of tests/lpf_ref.py on the same arrays; sizing, overflow and info."""
import ctypes as C

import numpy as np
import pytest
import torch

from bce_amd import api

import lpf_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_OVERFLOW = -1, -5
PB, P = 2048, 256                                                         # positions per block; blocks per pass of the top kernel
LIT = 0xFFFFFFFF
SIZES = (1, PB - 1, PB, PB + 1, P * PB + 1, 2 * P * PB + 1)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _text(n):
    return ((np.arange(n, dtype=np.uint64) * 2654435761 >> 7) & 0xFF).astype(np.uint8)


def _hook(ctx, lens, text, min_len, src=None):
    """sizing call, both overflows, then the full call into guarded buffers at odd offsets -> (ops (nops, 2) uint32, lits uint8, info)"""
    n = len(lens)
    d_len = torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    d_src = None if src is None else torch.from_numpy(np.asarray(src, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    d_t = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), text])).to(DEV)[1:]
    torch.cuda.synchronize()
    ptrs = (d_len.data_ptr(), None if d_src is None else d_src.data_ptr(), d_t.data_ptr(), n, min_len, ctx)
    rc, info = api.self_parse_of_lpf_device(*ptrs)
    assert rc == 0
    nops, nlits = info["nops"], info["nlits"]
    ops = torch.full((2 * nops + 3,), -5, dtype=torch.int32, device=DEV)
    lits = torch.full((nlits + 6,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for ops_cap, lits_cap in ((nops - 1, nlits), (nops, nlits - 1)):
        if ops_cap >= 0 and lits_cap >= 0:
            rc, again = api.self_parse_of_lpf_device(*ptrs, ptr_ops=ops[1:].data_ptr(), ops_cap=ops_cap, ptr_lits=lits[3:].data_ptr(), lits_cap=lits_cap)
            assert rc == E_OVERFLOW and again == info and bool((ops == -5).all()) and bool((lits == 0xA5).all())       # no byte written
    rc, again = api.self_parse_of_lpf_device(*ptrs, ptr_ops=ops[1:].data_ptr(), ops_cap=nops, ptr_lits=lits[3:].data_ptr() if nlits else None, lits_cap=nlits)
    assert rc == 0 and again == info
    go, gl = ops.cpu().numpy(), lits.cpu().numpy()
    assert go[0] == -5 and (go[-2:] == -5).all() and (gl[:3] == 0xA5).all() and (gl[3 + nlits:] == 0xA5).all()
    return go[1:-2].view(np.uint32).reshape(-1, 2), gl[3:3 + nlits], info


def _check(ctx, lens, min_len, src=None):
    lens = np.asarray(lens, dtype=np.uint32)
    text = _text(len(lens))
    ph, wl, winfo = ref.chain(lens, text.tobytes(), min_len)
    ops, lits, info = _hook(ctx, lens, text, min_len, src)
    assert info == winfo and winfo["nlits"] + winfo["copied"] == len(lens) and lits.tobytes() == wl
    assert ops[:, 0].tolist() == [p[1] for p in ph]
    assert ops[:, 1].tolist() == [(0 if src is None else int(src[s])) if cp else LIT for s, _l, cp in ph]      # a copy names the source of its FIRST position
    return ph


@pytest.mark.parametrize("n", SIZES)
def test_all_zero_is_one_literal_run_across_every_block(ctx, n):
    assert _check(ctx, np.zeros(n, dtype=np.uint32), 1) == [(0, n, False)]
    _check(ctx, np.minimum(np.arange(n, 0, -1), 5), 6)                    # lengths everywhere, all of them too short


@pytest.mark.parametrize("n", SIZES)
def test_jumps_of_5000_go_over_whole_blocks(ctx, n):
    ph = _check(ctx, np.minimum(np.arange(n, 0, -1), 5000), 1, src=np.arange(n, dtype=np.uint32) ^ 0x2A)
    assert all(cp for _s, _l, cp in ph) and [l for _s, l, _c in ph[:-1]] == [5000] * (len(ph) - 1) and ph[-1][0] + ph[-1][1] == n


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K", (2, 7, PB - 1, PB))
def test_copies_and_single_literals_alternate_across_block_edges(ctx, n, K):
    """position s: a copy of K bytes where s mod (K + 1) == 0, else too short: copy, literal, copy, literal ... so that with K =
    2047 every block edge is a phrase edge and with K = 2048 the edges drift through the blocks"""
    s = np.arange(n)
    lens = np.minimum(np.where(s % (K + 1) == 0, K, 1), n - s)
    ph = _check(ctx, lens, 2, src=(s * 3 + 1).astype(np.uint32))
    if n > 2 * K + 2:
        assert ph[:4] == [(0, K, True), (K, 1, False), (K + 1, K, True), (2 * K + 1, 1, False)]


@pytest.mark.parametrize("land", (0, -1, 1))
def test_chains_that_land_on_the_edges_of_the_mirrored_blocks(ctx, land):
    """the chain runs over the arrays written at n - 1 - s, so its blocks are counted from the text's END: copies built so that each
    one's successor s + l is the mirror of b * PB + land, for every b of 6 blocks and across the pass edge -- the exit of a mirrored
    block is the last position of the block below, its first position, or its second"""
    for n, blocks in ((6 * PB + 3, range(1, 6)), ((P + 2) * PB + 3, (P - 1, P, P + 1))):
        lens = np.zeros(n, dtype=np.uint32)
        s = 0
        for b in sorted(blocks, reverse=True):
            target = n - 1 - (b * PB + land)                              # the position whose mirror is b * PB + land
            lens[s] = target - s
            s = target
        lens[s] = 3                                                       # and a short copy from there
        ph = _check(ctx, lens, 2, src=np.arange(n, dtype=np.uint32) ^ 0x55)
        assert sum(1 for p in ph if p[2]) == len(list(blocks)) + 1


@pytest.mark.parametrize("seed", range(6))
def test_random_lengths_and_min_len(ctx, seed):
    rs = np.random.RandomState(seed)
    n = int(rs.choice([777, PB + 17, 5 * PB + 1, 40 * PB + 3, P * PB + 2 * PB + 9, 300 * PB + 5]))
    cap = np.arange(n, 0, -1)
    kind = seed % 3
    lens = rs.randint(0, 9000, size=n) if kind == 0 else (rs.randint(0, 40, size=n) if kind == 1 else rs.randint(0, 100000, size=n) * (rs.randint(0, 50, size=n) == 0))
    lens = np.minimum(lens, cap).astype(np.uint32)
    min_len = int(rs.choice([1, 2, 16, 100, 4096]))
    _check(ctx, lens, min_len)
    _check(ctx, lens, min_len, src=rs.randint(0, 1 << 31, size=n).astype(np.uint32))


def test_hook_refusals(ctx):
    info = api.ParseInfo(1, 2, 3, 4)
    lib = ctx.lib
    d = torch.zeros(16, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p = d.data_ptr()
    fn = lib.bce_hip_self_parse_of_lpf_device
    assert fn(ctx.h, p, None, p, 4, 0, None, 0, None, 0, C.byref(info)) == E_ARG
    assert fn(ctx.h, p, None, p, 4, 4097, None, 0, None, 0, C.byref(info)) == E_ARG
    assert fn(ctx.h, p, None, p, 1 << 31, 1, None, 0, None, 0, C.byref(info)) == E_ARG
    assert fn(ctx.h, None, None, p, 4, 1, None, 0, None, 0, C.byref(info)) == E_ARG
    assert fn(ctx.h, p, None, None, 4, 1, None, 0, None, 0, C.byref(info)) == E_ARG
    assert fn(ctx.h, p, None, p, 4, 1, None, 1, None, 0, C.byref(info)) == E_ARG
    assert fn(ctx.h, p, None, p, 4, 1, None, 0, None, 0, None) == E_ARG
    assert (info.nops, info.nlits, info.ncopies, info.copied) == (1, 2, 3, 4)
    assert fn(ctx.h, None, None, None, 0, 1, None, 0, None, 0, C.byref(info)) == 0 and info.nops == 0
