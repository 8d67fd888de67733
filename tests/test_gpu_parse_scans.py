"""GPU: the parse alone on synthetic lengths (bce_hip_parse_of_lengths_device: exits, walk, mark, count, top, emit and the
run-length rule of kd_parse.hip with the launches of the real call) and the patch alone on op lists written by hand, both past one
block (2048 positions / ops) and past one pass of the top kernels (256 blocks), against tests/parse_ref.py on the same arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api

import parse_ref as ref

pytestmark = pytest.mark.gpu
E_ARG, E_OVERFLOW = -1, -5
PB, P = 2048, 256                                                         # positions per block; blocks per pass of the top kernel
LIT = 0xFFFFFFFF
SIZES = (1, 2, PB - 1, PB, PB + 1, 2 * PB + 1, (P - 1) * PB, P * PB + 1, 2 * P * PB + 1)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    c = api._Ctx(0)
    yield c
    c.close()


def _query(q):
    return ((np.arange(q, dtype=np.uint64) * 2654435761 >> 7) & 0xFF).astype(np.uint8)


def _hook(ctx, lens, query, min_len, pos=None):
    """sizing call, then the full call into guarded buffers at odd offsets -> (ops (nops, 2) uint32, lits uint8, info)"""
    q = len(lens)
    d_len = torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    d_pos = None if pos is None else torch.from_numpy(np.asarray(pos, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    d_q = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), query])).to(DEV)[1:]
    torch.cuda.synchronize()
    ptrs = (d_len.data_ptr(), None if d_pos is None else d_pos.data_ptr(), d_q.data_ptr(), q, min_len, ctx)
    rc, info = api.parse_of_lengths_device(*ptrs)
    assert rc == 0
    nops, nlits = info["nops"], info["nlits"]
    ops = torch.full((2 * nops + 3,), -5, dtype=torch.int32, device=DEV)
    lits = torch.full((nlits + 6,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for ops_cap, lits_cap in ((nops - 1, nlits), (nops, nlits - 1)):
        if ops_cap >= 0 and lits_cap >= 0:
            rc, again = api.parse_of_lengths_device(*ptrs, ptr_ops=ops[1:].data_ptr(), ops_cap=ops_cap, ptr_lits=lits[3:].data_ptr(), lits_cap=lits_cap)
            assert rc == E_OVERFLOW and again == info and bool((ops == -5).all()) and bool((lits == 0xA5).all())
    rc, again = api.parse_of_lengths_device(*ptrs, ptr_ops=ops[1:].data_ptr(), ops_cap=nops, ptr_lits=lits[3:].data_ptr() if nlits else None, lits_cap=nlits)
    assert rc == 0 and again == info
    go, gl = ops.cpu().numpy(), lits.cpu().numpy()
    assert go[0] == -5 and (go[-2:] == -5).all() and (gl[:3] == 0xA5).all() and (gl[3 + nlits:] == 0xA5).all()
    return go[1:-2].view(np.uint32).reshape(-1, 2), gl[3:3 + nlits], info


def _check(ctx, lens, min_len, pos=None):
    lens = np.asarray(lens, dtype=np.uint32)
    query = _query(len(lens))
    want = ref.parse_of_lengths(lens, query.tobytes(), min_len)
    ops, lits, info = _hook(ctx, lens, query, min_len, pos)
    if pos is None:
        ref.check(b"", query, want, ops, lits, info, positions=False)
    else:                                                  # every copy names the position of its END element
        assert info == want[2] and lits.tobytes() == want[1]
        assert ops[:, 0].tolist() == [p[1] for p in want[0]]
        assert ops[:, 1].tolist() == [int(pos[s + l - 1]) if cp else LIT for s, l, cp in want[0]]
    return want


@pytest.mark.parametrize("q", SIZES)
def test_all_literal_one_run_across_every_block_and_pass(ctx, q):
    want = _check(ctx, np.zeros(q, dtype=np.uint32), 1)
    assert want[0] == [(0, q, False)]
    _check(ctx, np.minimum(np.arange(1, q + 1), 5), 6)                    # lengths everywhere, all of them too short


@pytest.mark.parametrize("q", SIZES)
@pytest.mark.parametrize("K", (1, 7, PB))
def test_copies_back_to_back_with_a_literal_head(ctx, q, K):
    if K > 1 and q % K == 0:                                              # (K = 1: every byte a copy, there is no head)
        q += 1
    want = _check(ctx, np.minimum(np.arange(1, q + 1), K), K)
    ph = want[0]
    assert all(p[2] and p[1] == K for p in ph[1:] if q >= K) and ph[-1][0] + ph[-1][1] == q
    if q > K > 1:
        assert ph[0] == (0, q % K, False)                                 # the head: q mod K literal bytes in one run


def test_one_jump_over_blocks_that_are_never_entered(ctx):
    for q in (3 * PB + 6, 5 * PB + 100, P * PB + 3 * PB + 7):
        lens = np.zeros(q, dtype=np.uint32)
        lens[q - 1] = 3 * PB + 5
        want = _check(ctx, lens, 2)
        assert want[0] == [(0, q - 3 * PB - 5, False), (q - 3 * PB - 5, 3 * PB + 5, True)]
    lens = np.zeros(4 * PB, dtype=np.uint32)
    lens[4 * PB - 1] = 4 * PB                                             # one copy covers everything: position 0 too
    assert _check(ctx, lens, 2)[0] == [(0, 4 * PB, True)]


@pytest.mark.parametrize("land", (0, -1, 1))
def test_chains_that_land_on_block_edges(ctx, land):
    """copies built to end exactly on b * PB + land, for every b of 6 blocks and across the pass edge: the exit of a block is the
    last position of the block below, its first position, or its second"""
    for q, blocks in ((6 * PB + 3, range(1, 6)), ((P + 2) * PB + 3, (P - 1, P, P + 1))):
        lens = np.zeros(q, dtype=np.uint32)
        e = q - 1
        for b in sorted(blocks, reverse=True):
            target = b * PB + land                                        # the node the copy that ends at e jumps to
            lens[e] = e - target
            e = target
        lens[e] = 3                                                       # and a short copy from there
        want = _check(ctx, lens, 2, pos=np.arange(q, dtype=np.uint32) ^ 0x55)
        assert sum(1 for p in want[0] if p[2]) == len(list(blocks)) + 1


def test_chain_ends_with_a_copy_at_0_and_with_a_literal_at_0(ctx):
    for q in (1, 5, PB, PB + 1, 3 * PB + 2):
        lens = np.zeros(q, dtype=np.uint32)
        lens[q - 1] = q
        assert _check(ctx, lens, 1)[0] == [(0, q, True)]
        if q > 1:
            lens[q - 1] = q - 1
            assert _check(ctx, lens, 1)[0] == [(0, 1, False), (1, q - 1, True)]
            lens = np.zeros(q, dtype=np.uint32)
            lens[0] = 1                                                   # a copy of one byte that covers position 0, literals behind it
            assert _check(ctx, lens, 1)[0] == [(0, 1, True), (1, q - 1, False)]


@pytest.mark.parametrize("seed", range(6))
def test_random_lengths_and_min_len(ctx, seed):
    rs = np.random.RandomState(seed)
    q = int(rs.choice([777, PB + 17, 5 * PB + 1, 40 * PB + 3, P * PB + 2 * PB + 9, 300 * PB + 5]))
    cap = np.minimum(np.arange(1, q + 1), 4096)
    kind = seed % 3
    lens = rs.randint(0, 4097, size=q) if kind == 0 else (rs.randint(0, 40, size=q) if kind == 1 else rs.randint(0, 4097, size=q) * (rs.randint(0, 50, size=q) == 0))
    lens = np.minimum(lens, cap).astype(np.uint32)
    min_len = int(rs.choice([1, 2, 16, 100, 4096]))
    _check(ctx, lens, min_len)
    _check(ctx, lens, min_len, pos=rs.randint(0, 1 << 31, size=q).astype(np.uint32))


def test_hook_refusals(ctx):
    info = api.ParseInfo(1, 2, 3, 4)
    lib = ctx.lib
    d = torch.zeros(16, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p = d.data_ptr()
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, p, None, p, 4, 0, None, 0, None, 0, C.byref(info)) == E_ARG
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, p, None, p, 4, 4097, None, 0, None, 0, C.byref(info)) == E_ARG
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, p, None, p, 1 << 31, 1, None, 0, None, 0, C.byref(info)) == E_ARG
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, None, None, p, 4, 1, None, 0, None, 0, C.byref(info)) == E_ARG
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, p, None, None, 4, 1, None, 0, None, 0, C.byref(info)) == E_ARG
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, p, None, p, 4, 1, None, 1, None, 0, C.byref(info)) == E_ARG
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, p, None, p, 4, 1, None, 0, None, 0, None) == E_ARG
    assert (info.nops, info.nlits, info.ncopies, info.copied) == (1, 2, 3, 4)
    assert lib.bce_hip_parse_of_lengths_device(ctx.h, None, None, None, 0, 1, None, 0, None, 0, C.byref(info)) == 0 and info.nops == 0


# ---- the patch alone ----------------------------------------------------------------------------------------------------------------

N = (1 << 20) + 3


@pytest.fixture(scope="module")
def loaded():
    """a context that holds a text of 2^20 + 3 bytes, loaded and nothing more: all the patch reads"""
    text = bce_amd.synth_rand(11, N)
    c = api._Ctx(0)
    rf = api.RankFile(text, ctx=c, build=False, index=False)
    yield rf, text
    c.close()


def _patch_dev(rf, ops, lits, lead=1, cap=None):
    """through bce_hip_patch_device into a guarded buffer whose result begins `lead` bytes behind an aligned address"""
    ops = np.asarray(ops, dtype=np.uint32).reshape(-1, 2)
    d_ops = torch.from_numpy(np.concatenate([np.zeros(1, np.uint32), ops.reshape(-1)]).view(np.int32)).to(DEV)[1:]
    d_lits = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), np.asarray(lits, dtype=np.uint8)])).to(DEV)[1:]
    want_len = int(ops[:, 0].astype(np.uint64).sum())
    total = rf.patch_device(d_ops.data_ptr(), len(ops), d_lits.data_ptr() if len(lits) else None, len(lits))
    assert total == want_len
    out = torch.full((32 + total + 40,), 0x5A, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    at = 32 - out.data_ptr() % 16 + lead
    assert rf.patch_device(d_ops.data_ptr(), len(ops), d_lits.data_ptr() if len(lits) else None, len(lits), out[at:].data_ptr(), total if cap is None else cap) == total
    go = out.cpu().numpy()
    assert (go[:at] == 0x5A).all() and (go[at + total:] == 0x5A).all()
    return go[at:at + total]


def test_patch_one_long_literal_and_one_long_copy(loaded):
    rf, text = loaded
    lits = bce_amd.synth_rand(12, N)
    for lead in (0, 1, 15):
        assert np.array_equal(_patch_dev(rf, [(N, LIT)], lits, lead), lits)
        assert np.array_equal(_patch_dev(rf, [(N, 0)], [], lead), text)
    assert np.array_equal(_patch_dev(rf, [(N - 5, 5), (N - 1, LIT), (N, 0)], lits[:N - 1], 3), np.concatenate([text[5:], lits[:N - 1], text]))
    assert np.array_equal(rf.patch([(N - 5, 5), (7, LIT)], lits[:7]), np.concatenate([text[5:], lits[:7]]))     # host buffers


def test_patch_one_byte_ops_past_one_block(loaded):
    rf, text = loaded
    for nops in (2 * PB + 1, P * PB + 5):
        ops = np.zeros((nops, 2), dtype=np.uint32)
        ops[:, 0] = 1
        ops[0::2, 1] = LIT
        ops[1::2, 1] = (np.arange(nops // 2, dtype=np.uint64) * 7919 % N).astype(np.uint32)
        lits = bce_amd.synth_rand(13, (nops + 1) // 2)
        got = _patch_dev(rf, ops, lits, 7)
        assert np.array_equal(got[0::2], lits) and np.array_equal(got[1::2], text[ops[1::2, 1]])


def test_patch_every_alignment_of_source_and_destination(loaded):
    rf, text = loaded
    lits = bce_amd.synth_rand(14, 4000)
    for dst in range(16):
        ops, parts, at = [], [], 0
        for src in range(8):                                              # copies and literal runs from every source alignment, 100 bytes or so each
            ops += [(97 + src, 1000 * src + src), (3 + src, LIT)]
            parts += [text[1000 * src + src:1000 * src + src + 97 + src], lits[at:at + 3 + src]]
            at += 3 + src
        ops.append((200, LIT))
        parts.append(lits[at:at + 200])
        assert np.array_equal(_patch_dev(rf, ops, lits[:at + 200], dst), np.concatenate(parts)), dst


MALFORMED = [                                                              # (ops, nlits, words of the refusal): as tests/test_parse_cpu.py
    ([(3, 0), (0, 2)], 0, "an op of length 0"),
    ([(0, LIT)], 0, "an op of length 0"),
    ([(4, N - 3)], 0, "past the end of the text"),
    ([(1, N)], 0, "past the end of the text"),                            # src = n
    ([(0x7FFFFFFF, 1)], 0, "past the end of the text"),
    ([(2, LIT), (3, 0)], 1, "do not add up"),
    ([(2, LIT), (3, 0)], 3, "do not add up"),
    ([(N, 0)] * 2047 + [(N - 1, 0)], 0, "2^31 bytes or more"),            # 2048 (2^20 + 3) - 1 > 2^31 - 1, by the lengths alone
    ([(5, 0)] * (2 * PB) + [(0, 7)], 0, "an op of length 0"),              # in the third block
]


def test_patch_refuses_every_malformed_kind_and_goes_on(loaded):
    rf, text = loaded
    c = rf._c
    lits = torch.full((8,), 65, dtype=torch.uint8, device=DEV)
    out = torch.full((4096,), 0x5A, dtype=torch.uint8, device=DEV)
    for ops, nlits, why in MALFORMED:
        arr = np.array(ops, dtype=np.uint32)
        d_ops = torch.from_numpy(arr.view(np.int32)).to(DEV)
        torch.cuda.synchronize()
        total = C.c_uint64(77)
        for d_out, cap in ((None, 0), (out.data_ptr(), 4096)):
            assert c.lib.bce_hip_patch_device(c.h, d_ops.data_ptr(), len(arr), lits.data_ptr(), nlits, d_out, cap, C.byref(total)) == E_ARG
            assert why in c.lib.bce_hip_last_error(c.h).decode() and total.value == 77
        host = np.full(64, 3, dtype=np.uint8)
        hl = np.full(8, 65, dtype=np.uint8)
        assert c.lib.bce_hip_patch(c.h, arr.ctypes.data, len(arr), hl.ctypes.data, nlits, host.ctypes.data, 64, C.byref(total)) == E_ARG
        assert (host == 3).all() and total.value == 77
        assert bool((out == 0x5A).all())
        assert np.array_equal(rf.patch([(5, 1), (2, LIT)], b"AA"), np.concatenate([text[1:6], [65, 65]]))     # the context is usable afterwards
    with pytest.raises(api.BceError) as e:
        rf.patch([(1, N)], b"")
    assert e.value.status == E_ARG and "past the end of the text" in str(e.value)
    # too small an output: the exact length, nothing written
    total = C.c_uint64(0)
    d_ops = torch.from_numpy(np.array([(100, 0), (3, LIT)], dtype=np.uint32).view(np.int32)).to(DEV)
    torch.cuda.synchronize()
    assert c.lib.bce_hip_patch_device(c.h, d_ops.data_ptr(), 2, lits.data_ptr(), 3, out.data_ptr(), 102, C.byref(total)) == E_OVERFLOW
    assert total.value == 103 and bool((out == 0x5A).all())
