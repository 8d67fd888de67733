"""GPU: device allocations that fail for real (test knob 14) -- the node lists' fallback sizes, an out-of-memory error that leaves
nothing behind, and the inverse BWT of the seam after the stepping interface.

Knob 14 asks hipMalloc for more than the device holds (hipMemGetInfo's total + 1 GiB) where an allocation is to fail, so the
error is the runtime's own and stays set until it is read, exactly as on a full device (BCE_HIP_TEST_OOM, by contrast, frees an
allocation that succeeded and only ever fails a first attempt).  1 = a node list's first-choice size fails both attempts,
2 = every attempt of a node list's growth fails, 3 = the first attempt of every allocation fails.  Per context: no child process."""
import re

import numpy as np
import pytest

import bce_amd
import oracle
from test_gpu_decode_bounded import NAMES, _case

pytestmark = pytest.mark.gpu

NOMEM = -3


def _knobs(ctx, **kv):
    for k, v in kv.items():
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, int(k[1:]), v), "bce_hip_debug_set")


# the inputs of test_gpu_parity.py::test_node_lists_grow_when_a_round_does_not_fit (lists of 4096 nodes, rounds only)
ENC_INPUTS = {"rand-300k": lambda: oracle.synth_rand(2, 300000), "text-2M": lambda: oracle.synth_text(9, 2_000_000),
              "mixed": lambda: oracle.synth_rand(5, 70000) + oracle.synth_text(5, 500000)}


@pytest.mark.parametrize("name", list(ENC_INPUTS))
def test_encoder_lists_fall_back_when_the_doubled_size_does_not_fit(name, capfd, monkeypatch):
    """Knob 14 = 1: every doubled list (k3_grow_lists' first choice) fails twice, with ctx_trim between; the list is made with
    need + need / 16 + 4096 nodes instead -- the size the trace prints for every growth -- and the archive is the oracle's.  The
    runtime's error of the failed retry is cleared (ensure): otherwise the next launch check would report it."""
    monkeypatch.setenv("BCE_ALLOC_TRACE", "1")
    data = ENC_INPUTS[name]()
    n = len(data)
    ctx = bce_amd.api._Ctx(0)
    try:
        _knobs(ctx, k12=1 << 30, k1=1, k14=1)        # (k1: no depth-first tail, which would take these inputs over before the lists fill)
        capfd.readouterr()
        rf = bce_amd.RankFile(data, ctx=ctx)
        assert bce_amd.BCE().encode(rf) == oracle.compress(data)
        err = capfd.readouterr().err
        st = bce_amd.stats(rf)
        assert st["list_grows"] >= 2, st
        grows = re.findall(r"k3: round \d+ needs lists of (\d+) nodes: parity \d now holds (\d+) per list", err)
        assert len(grows) == st["list_grows"], err[-3000:]
        for need, held in grows:
            need, held = int(need), int(held)
            assert held == min(need + need // 16 + 4096, n // 2 + 2), (need, held)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", NAMES)
def test_decoder_lists_fall_back_when_the_larger_size_does_not_fit(name, capfd, monkeypatch):
    """Knob 14 = 1 on the bounded-memory inputs with lists of 4096 nodes: every list the decoder grows (grow_lists' first choice,
    1.25 x the need) fails twice; the list is made with exactly the need and the children pass runs again from the answers."""
    monkeypatch.setenv("BCE_ALLOC_TRACE", "1")
    data, arch = _case(name)
    ctx = bce_amd.api._Ctx(0)
    try:
        _knobs(ctx, k12=1 << 30, k14=1)
        s0 = bce_amd.stats_of(ctx)
        capfd.readouterr()
        out = np.empty(len(data), dtype=np.uint8)
        assert bce_amd.decompress_device(arch, ctx=ctx, out=out) == len(data)
        err = capfd.readouterr().err
        assert out.tobytes() == data
        s1 = bce_amd.stats_of(ctx)
        assert s1["dec_restarts"] - s0["dec_restarts"] == 0
        grows = s1["dec_list_grows"] - s0["dec_list_grows"]
        assert grows >= 2
        sizes = [(int(a), int(b)) for a, b in
                 re.findall(r"does not fit the node lists: the children of plane \d \((\d+) nodes\) in plane \d's list of \d+ \(parity \d\), grown in place to (\d+)", err)]
        assert len(sizes) == grows, err[-3000:]
        assert all(want == need for need, want in sizes), sizes
    finally:
        ctx.close()


def test_a_list_growth_that_finds_no_memory_fails_cleanly(monkeypatch):
    """Knob 14 = 2: no attempt of a list growth succeeds.  The encode and the decode end with BCE_HIP_E_NOMEM and the documented
    message -- never another code, never an error of the runtime that was left behind.  Then, the knob cleared, the same context
    on the same thread compresses and decodes the same input correctly, its lists growing for real: no stale error and no half
    released list survives."""
    data = oracle.synth_rand(2, 300000)
    arch = oracle.compress(data)
    ctx = bce_amd.api._Ctx(0)
    try:
        _knobs(ctx, k12=1 << 30, k1=1, k14=2)
        with pytest.raises(bce_amd.BceError) as e:
            bce_amd.compress(data, ctx=ctx)
        assert e.value.status == NOMEM and "k3: no device memory for node lists of" in str(e.value), str(e.value)
        with pytest.raises(bce_amd.BceError) as e:
            bce_amd.decompress_device(arch, ctx=ctx)
        assert e.value.status == NOMEM and "decode: no device memory for a node list of" in str(e.value), str(e.value)
        _knobs(ctx, k14=0)
        g0, s0 = bce_amd.stats_of(ctx)["dec_list_grows"], bce_amd.stats_of(ctx)["dec_restarts"]
        assert bce_amd.decompress_device(arch, ctx=ctx) == data
        s1 = bce_amd.stats_of(ctx)
        assert s1["dec_list_grows"] - g0 >= 2 and s1["dec_restarts"] == s0
        rf = bce_amd.RankFile(data, ctx=ctx)
        assert bce_amd.BCE().encode(rf) == arch
        assert bce_amd.stats(rf)["list_grows"] >= 2
        _knobs(ctx, k12=0, k1=0)
        assert bce_amd.compress(data, ctx=ctx) == arch
        assert bce_amd.decompress_device(arch, ctx=ctx) == data
    finally:
        ctx.close()


def test_inverse_bwt_after_the_stepping_interface(capfd, monkeypatch):
    """bce_hip_inverse_bwt on a context the stepping interface has run rounds in, with the first attempt of every allocation
    failing (knob 14 = 3): what goes back (ctx_trim) is what phase 5, the seam's inverse BWT, does not hold -- not phase 3's
    list, which would include buffers the transform has just allocated.  The stepping calls leave phase 0 behind."""
    monkeypatch.setenv("BCE_ALLOC_TRACE", "1")
    ctx = bce_amd.api._Ctx(0)
    try:
        rf = bce_amd.RankFile(oracle.synth_text(3, 100000), ctx=ctx)
        bce = bce_amd.BCE()
        bce.code_begin(rf)
        for _ in range(4):
            bce.code_round(rf)
        data = oracle.synth_text(4, 300000)          # (larger than the stepping input: every buffer of the transform is allocated anew)
        u, primary = oracle.divbwt(data)
        _knobs(ctx, k14=3)
        capfd.readouterr()
        a = np.frombuffer(u, dtype=np.uint8).copy()
        out = np.zeros(len(a), dtype=np.uint8)
        ctx.check(ctx.lib.bce_hip_inverse_bwt(ctx.h, a.ctypes.data, out.ctypes.data, len(a), primary), "bce_hip_inverse_bwt")
        err = capfd.readouterr().err
        assert out.tobytes() == data == oracle.inverse_bwt(u, primary)
        assert "out of device memory in phase 5" in err, err[-2000:]
        assert "in phase 3" not in err, err[-2000:]
        _knobs(ctx, k14=0)
        assert bce_amd.compress(data, ctx=ctx) == oracle.compress(data)
    finally:
        ctx.close()


def test_knob_14_takes_only_its_modes():
    ctx = bce_amd.api._Ctx(0)
    try:
        assert ctx.lib.bce_hip_debug_set(ctx.h, 14, 4) == -1
        assert ctx.lib.bce_hip_debug_set(ctx.h, 14, 0) == 0
    finally:
        ctx.close()
