"""GPU: the GPU-assisted decoder (kd_decode.hip) in bounded memory -- every archive `bce -c` writes decodes with `bce -d`.

Two mechanisms keep a decode's memory bounded whatever the input: node lists of their own per (parity, plane) that grow in
place in the middle of a round (a plane's decoder is never asked twice, no decode starts again), and per-round query buffers
sized to a query budget -- a round with more nodes runs plane group by plane group.  Both are forced at small sizes here with
test knobs 12 (small lists) and 13 (small budget), against the oracle's archives; then the largest input runs in full."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bce_amd
import oracle
from conftest import ROOT, fullsize_input, load_fullsize_golden

pytestmark = pytest.mark.gpu


def _long_zero_run():
    """Text with duplicated stretches and a long run of zeros (as _with_long_tail in test_gpu_decode.py, smaller)."""
    # (oracle.synth_text, not bce_amd's: loading the HIP library while the tests are collected, before torch, takes the
    #  device away from torch in the same process)
    t = np.frombuffer(oracle.synth_text(7, 1_000_000), dtype=np.uint8)
    return np.concatenate([t, t[200000:400000], np.zeros(120000, dtype=np.uint8), t[500000:650000], t[:77777]]).tobytes()


NAMES = ["text-3M", "rand-400k", "zero-run"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(input, the oracle's archive of it), made the first time a test asks (not while the tests are collected)."""
    data = {"text-3M": lambda: oracle.synth_text(12, 3_000_000), "rand-400k": lambda: oracle.synth_rand(12, 400_000),
            "zero-run": _long_zero_run}[name]()
    return data, oracle.compress(data)


def _decode(arch, want, knobs):
    ctx = bce_amd.api._Ctx(0)
    try:
        for k, v in knobs.items():
            ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, k, v), "bce_hip_debug_set")
        s0 = bce_amd.stats_of(ctx)
        out = np.empty(len(want), dtype=np.uint8)
        assert bce_amd.decompress_device(arch, ctx=ctx, out=out) == len(want)
        assert out.tobytes() == want
        s1 = bce_amd.stats_of(ctx)
        return {k: s1[k] - s0[k] for k in ("dec_restarts", "dec_list_grows", "dec_split_rounds")}
    finally:
        ctx.close()


@pytest.mark.parametrize("env", [{}, {"BCE_DEC_NO_MAILBOX": "1"}, {"BCE_DEC_NO_SPLIT": "1"}], ids=["lanes", "no-mailbox", "no-split"])
@pytest.mark.parametrize("budget", [4096, 65536])
@pytest.mark.parametrize("name", NAMES)
def test_rounds_over_the_query_budget_run_in_plane_groups(name, budget, env, monkeypatch):
    """Knob 13 lowers the query budget: every round with more nodes runs its planes in groups that share the query and
    answer buffers one after the other -- plane by plane in the six-launch rounds (busiest first), in plane order where all
    planes go at once (BCE_DEC_NO_SPLIT).  The exact input comes back and the rounds are counted."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    data, arch = _case(name)
    d = _decode(arch, data, {13: budget})
    assert d["dec_split_rounds"] >= 1, d
    assert d["dec_restarts"] == 0 and d["dec_list_grows"] == 0, d


@pytest.mark.parametrize("budget", [0, 4096])
@pytest.mark.parametrize("name", NAMES)
def test_node_lists_grow_in_place(name, budget):
    """Knob 12 = 2^30: lists of 4096 nodes.  A plane whose children do not fit has its one list replaced and its children
    pass run again from the answers it already has -- no decode starts again.  Alone and with a small query budget."""
    knobs = {12: 1 << 30}
    if budget:
        knobs[13] = budget
    data, arch = _case(name)
    d = _decode(arch, data, knobs)
    assert d["dec_restarts"] == 0 and d["dec_list_grows"] >= 2, d
    if budget:
        assert d["dec_split_rounds"] >= 1, d


_CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
import bce_amd, oracle
from test_gpu_decode_bounded import NAMES, _case, _decode
for name in NAMES:
    data, arch = _case(name)
    for knobs in ({13: 4096}, {12: 1 << 30}, {12: 1 << 30, 13: 4096}):
        d = _decode(arch, data, knobs)
        assert d["dec_restarts"] == 0, (name, knobs, d)
        assert d["dec_list_grows"] >= (2 if 12 in knobs else 0) and d["dec_split_rounds"] >= (1 if 13 in knobs else 0), (name, knobs, d)
print("CHILD_OK")
'''


@pytest.mark.parametrize("every", ["3", "5"])
def test_out_of_memory_inside_a_decode(every):
    """BCE_HIP_TEST_OOM=k: every k-th device allocation of the process is reported out of memory at its first attempt (read
    once per process: a child).  The grown lists, the group buffers and the stages after the rounds then go through ctx_trim and
    a second attempt, which succeeds.  (The exact-need fallback of a list that still does not fit, and the error cleared after
    a failed second attempt, take allocations that fail for real: test knob 14 in test_gpu_oom.py.)"""
    env = dict(os.environ, BCE_HIP_TEST_OOM=every, PYTHONPATH=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=900, env=env, cwd=os.path.join(ROOT, "tests"))
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_a_second_decode_does_not_grow():
    """After a decode whose lists grew (knob 12), the same context without the knob decodes the same archive again and grows
    nothing: its lists start at their default size, which this input never outgrows."""
    data, arch = _case("rand-400k")
    ctx = bce_amd.api._Ctx(0)
    try:
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 12, 1 << 30), "bce_hip_debug_set")
        assert bce_amd.decompress_device(arch, ctx=ctx) == data
        assert bce_amd.stats_of(ctx)["dec_list_grows"] >= 2
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 12, 0), "bce_hip_debug_set")
        g0 = bce_amd.stats_of(ctx)["dec_list_grows"]
        assert bce_amd.decompress_device(arch, ctx=ctx) == data
        assert bce_amd.stats_of(ctx)["dec_list_grows"] == g0
    finally:
        ctx.close()


def test_lists_given_back_after_the_rounds(monkeypatch, capfd):
    """BCE_DEC_GIVE_BACK=1: the lists and query buffers go back when the rounds end, as they do by themselves where the device
    would not hold the planes and the inverse BWT twice beside them.  The same context decodes again (the lists are made anew),
    with grown lists and plane groups too."""
    monkeypatch.setenv("BCE_DEC_GIVE_BACK", "1")
    monkeypatch.setenv("BCE_ALLOC_TRACE", "1")
    ctx = bce_amd.api._Ctx(0)
    try:
        for name in NAMES:
            data, arch = _case(name)
            capfd.readouterr()
            assert bce_amd.decompress_device(arch, ctx=ctx) == data
            assert "node lists and query buffers given back" in capfd.readouterr().err
        data, arch = _case("text-3M")
        for k, v in ((12, 1 << 30), (13, 4096)):
            ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, k, v), "bce_hip_debug_set")
        assert bce_amd.decompress_device(arch, ctx=ctx) == data
        assert bce_amd.decompress_device(arch, ctx=ctx) == data
    finally:
        ctx.close()


GOLD = load_fullsize_golden()


@pytest.mark.timeout(2400)
def test_random_1p5e9_decodes_without_a_restart():
    """1.5 * 10^9 random bytes: the archive the oracle made (its known answer), decoded with no restart -- a list that would have
    been too small grows in place instead."""
    v = GOLD["synth-rand-1.5e9"]
    data = fullsize_input(v)
    assert data is not None and len(data) == v["n"]
    ctx = bce_amd.api._Ctx(0)
    try:
        rf = bce_amd.RankFile(data, ctx=ctx)
        arch = bce_amd.BCE().encode(rf)
        assert len(arch) == v["archive_bytes"] and hashlib.sha256(arch).hexdigest() == v["archive_sha256"]
        del data, rf
        r0 = bce_amd.stats_of(ctx)["dec_restarts"]
        out = np.empty(v["n"], dtype=np.uint8)
        assert bce_amd.decompress_device(arch, ctx=ctx, out=out) == v["n"]
        assert hashlib.sha256(out).hexdigest() == v["input_sha256"]
        assert bce_amd.stats_of(ctx)["dec_restarts"] - r0 == 0
    finally:
        ctx.close()


ARCH_2P31M2 = (2166438056, "d37c2d07a1654589f51e615947e58cd40590a8929be24694ffd68f2effcab2a7")
INPUT_2P31M2 = "aaf5b2dbd3c34c586af1abdda8cd87ee4281edb84e8f070a32cf3d777cfd1c9a"


@pytest.mark.timeout(2400)
def test_the_worst_realistic_input_decodes(tmp_path):
    """2^31 - 2 random bytes, the input whose decode ended in BCE_HIP_E_NOMEM: encoded on the GPU (the archive of record), decoded
    in the same context through decompress_device, then by `bce -d` from a file in a process of its own."""
    n = (1 << 31) - 2
    data = bce_amd.synth_rand(1, n)
    ctx = bce_amd.api._Ctx(0)
    try:
        rf = bce_amd.RankFile(data, ctx=ctx)
        arch = bce_amd.BCE().encode(rf)
        assert (len(arch), hashlib.sha256(arch).hexdigest()) == ARCH_2P31M2
        assert hashlib.sha256(data).hexdigest() == INPUT_2P31M2
        del data, rf
        r0 = bce_amd.stats_of(ctx)["dec_restarts"]
        out = np.empty(n, dtype=np.uint8)
        assert bce_amd.decompress_device(arch, ctx=ctx, out=out) == n
        assert hashlib.sha256(out).hexdigest() == INPUT_2P31M2
        assert bce_amd.stats_of(ctx)["dec_restarts"] - r0 == 0
        del out
    finally:
        ctx.close()
    src, dst = tmp_path / "in.bce", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(arch)
    del arch
    r = subprocess.run([os.path.join(ROOT, "bce_amd", "bin", "bce"), "-d", str(dst), str(src)], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    src.unlink()
    h = hashlib.sha256()
    with open(dst, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    assert h.hexdigest() == INPUT_2P31M2
