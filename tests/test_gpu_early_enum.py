"""GPU: the one-shot compression starts the enumeration on the first sort's order (api.hip compress_early):
K1's first sort, a provisional BWT and its planes, the rounds below 8 h, then the rest of K1, the final BWT, the planes
again and the remaining rounds.  Every archive must be the oracle's and the one the old order of stages gives
(BCE_HIP_EARLY_ENUM=0); BCE_HIP_EARLY_TRACE=1 says on stderr where the rounds paused, so each case can check that it took the
way it is meant to test.  (tests/test_partial_order_cpu.py has the argument's check on the CPU.)"""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import bce_amd
import oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
TRACE = re.compile(r"early: h (\d+) limit (\d+) (paused|finished) at round (\d+) \(([a-z ]+)\) symbols (\d+) .* first_sort_final (\d)")

_ORACLE = {}


def want(data):
    """The oracle's archive of `data`, computed once per input."""
    key = (len(data), hash(data))
    if key not in _ORACLE:
        _ORACLE[key] = oracle.compress(data)
    return _ORACLE[key]


def on_device(data):
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def one_shot(ctx, t, **kw):
    arch, st = bce_amd.compress_device(t.data_ptr(), t.numel(), ctx=ctx, **kw)
    return bytes(arch), st


def traces(capfd):
    return [dict(h=int(m[0]), limit=int(m[1]), paused=m[2] == "paused", round=int(m[3]), why=m[4], symbols=int(m[5]), final=int(m[6]))
            for m in TRACE.findall(capfd.readouterr().err)]


@pytest.fixture
def ctx():
    c = bce_amd.api._Ctx(0)
    yield c
    c.close()


@pytest.fixture
def early(monkeypatch):
    monkeypatch.setenv("BCE_HIP_EARLY_TRACE", "1")
    monkeypatch.delenv("BCE_HIP_EARLY_ENUM", raising=False)
    monkeypatch.delenv("BCE_HIP_EARLY_CAP", raising=False)
    return monkeypatch


def both_orders(ctx, data, early, capfd, **kw):
    """Compress with the early rounds and with the old order of stages: both the oracle's archive.  -> the early run's trace."""
    t = on_device(data)
    capfd.readouterr()
    a, st = one_shot(ctx, t, **kw)
    tr = traces(capfd)
    assert len(tr) == 1, "the early route was not taken"
    early.setenv("BCE_HIP_EARLY_ENUM", "0")
    b, st0 = one_shot(ctx, t, **kw)
    early.delenv("BCE_HIP_EARLY_ENUM")
    assert traces(capfd) == []                                   # (the switch restores the old order)
    assert a == b == want(data)
    assert st["nodes"] == st0["nodes"] and st["rounds"] == st0["rounds"] and st["symbols"] == st0["symbols"]
    return tr[0]


def alphabet_text(seed, n, sigma):
    """n bytes over `sigma` symbols, skewed; the last eighth repeats the first, so the first sort leaves ties."""
    body = bytes(np.random.RandomState(seed).choice(np.arange(48, 48 + sigma, dtype=np.uint8), n - n // 8, p=np.arange(1, sigma + 1) / (sigma * (sigma + 1) / 2)))
    return body + body[:n // 8]


ORDINARY = {
    "text-1M": (lambda: oracle.synth_text(21, 1 << 20), None),
    "rand-256K": (lambda: oracle.synth_rand(22, 256 << 10), 8),          # 8-bit symbols: h = 8
    "sigma32-256K": (lambda: alphabet_text(23, 256 << 10, 32), 12),      # 5 bits: h = 12
    "sigma33-256K": (lambda: alphabet_text(24, 256 << 10, 33), 10),      # 6 bits: h = 10, the first alphabet past 12 symbols a key
    "sigma16-256K": (lambda: alphabet_text(25, 256 << 10, 16), 16),      # 4 bits: 16 symbols, the key's most
}


@pytest.mark.parametrize("name", list(ORDINARY))
def test_ordinary_inputs(name, ctx, early, capfd):
    make, h = ORDINARY[name]
    data = make()
    tr = both_orders(ctx, data, early, capfd)
    assert tr["limit"] == 8 * tr["h"] and (h is None or tr["h"] == h)
    if name == "rand-256K":
        assert tr["final"] == 1                                  # (random bytes differ within 8: no second gather or plane build)
        assert tr["why"] in ("end", "tail due") and tr["round"] < tr["limit"]   # the rounds end, or go depth-first, before the cap
    else:
        assert tr["final"] == 0                                  # (the first sort left ties: second gather, second plane build)
        assert tr["paused"] and tr["symbols"] > 0                # the coders had work before K1 finished


def test_cli_takes_the_same_route(tmp_path, early):
    data = oracle.synth_text(21, 1 << 20)
    src, dst = tmp_path / "in.txt", tmp_path / "out.bce"
    src.write_bytes(data)
    for env in ({}, {"BCE_HIP_EARLY_ENUM": "0"}, {"BCE_HIP_EARLY_CAP": "9"}):
        r = subprocess.run([EXE, "-c", str(dst), str(src)], capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout + r.stderr
        assert dst.read_bytes() == want(data)
        assert bool(TRACE.search(r.stderr)) == ("BCE_HIP_EARLY_ENUM" not in env)


TEXT_256K = oracle.synth_text(26, 256 << 10)


@pytest.mark.parametrize("cap", [0, 1, 7, 8, 9, 17, 1000])
def test_cap_lowered(cap, ctx, early, capfd):
    """Pauses in the ramp-up (the LDS tail kernel's rounds), in a one-launch round, either side of the plane 7 -> 0 wrap, and a
    cap above the limit (it never raises it)."""
    early.setenv("BCE_HIP_EARLY_CAP", str(cap))
    tr = both_orders(ctx, TEXT_256K, early, capfd)
    assert tr["limit"] == min(cap, 8 * tr["h"])
    assert tr["paused"] and tr["round"] <= tr["limit"]
    if cap <= 9:
        assert tr["round"] == cap and tr["why"] == "limit"


def _sweep(ctx, data, early, capfd, caps, **kw):
    """The pause on every round of `caps`: whatever else ends a batch there, or one round to either side, meets it."""
    t = on_device(data)
    early.setenv("BCE_HIP_EARLY_ENUM", "0")
    base, st0 = one_shot(ctx, t, **kw)
    early.delenv("BCE_HIP_EARLY_ENUM")
    assert base == want(data)
    capfd.readouterr()
    seen = set()
    for cap in caps:
        early.setenv("BCE_HIP_EARLY_CAP", str(cap))
        a, st = one_shot(ctx, t, **kw)
        assert a == base, cap
        assert st["nodes"] == st0["nodes"] and st["rounds"] == st0["rounds"] and st["symbols"] == st0["symbols"], cap
    for tr in traces(capfd):
        assert tr["paused"]
        seen.add(tr["round"])
    return st0, seen


def test_pause_meets_a_full_symbol_buffer(ctx, early, capfd):
    """A tiny symbol buffer: from the ramp-up on nearly every batch ends in need_flush, and some rounds grow the buffer."""
    st0, seen = _sweep(ctx, TEXT_256K, early, capfd, range(1, 33), symbol_capacity=3000)
    assert st0["flushes"] > 20 and len(seen) >= 8


def test_pause_meets_a_split_round(ctx, early, capfd):
    early.setenv("BCE_HIP_SPLIT_SYMS", "8000")
    st0, seen = _sweep(ctx, TEXT_256K, early, capfd, range(8, 33), symbol_capacity=4000)
    assert st0["split_rounds"] >= 3 and len(seen) >= 5


def test_pause_meets_growing_lists(ctx, early, capfd):
    ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 12, 64), "debug_set")      # node lists that start at n / 64 and grow
    st0, seen = _sweep(ctx, TEXT_256K, early, capfd, range(4, 33))
    assert st0["list_grows"] >= 1 and len(seen) >= 5


def test_pause_between_wide_rounds(ctx, early, capfd):
    ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 4, 1), "debug_set")        # no one-launch rounds: the wide kernels from the ramp-up on
    _sweep(ctx, TEXT_256K, early, capfd, range(6, 30, 3))


DEGENERATE = {
    "len-1": b"z", "len-2": b"ab", "len-2-equal": b"aa", "len-11": oracle.synth_text(27, 11), "len-12": oracle.synth_text(27, 12),
    "len-13": oracle.synth_text(27, 13), "len-300": oracle.synth_text(27, 300),
    "one-byte-64K": b"q" * 65536,
    "ab-64K": b"ab" * 32768,
    "abcabd": b"abcabd" * 3000 + b"x",
    "settled-by-first-sort": bytes(np.random.RandomState(28).permutation(np.arange(256, dtype=np.uint8))),   # every rotation differs in its first byte
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_inputs(name, ctx, early, capfd):
    data = DEGENERATE[name]
    t = on_device(data)
    capfd.readouterr()
    a, st = one_shot(ctx, t)
    tr = traces(capfd)
    early.setenv("BCE_HIP_EARLY_ENUM", "0")
    b, st0 = one_shot(ctx, t)
    assert a == b == want(data)
    assert st["nodes"] == st0["nodes"] and st["symbols"] == st0["symbols"]
    if len(data) == 1:
        assert tr == []                                          # (one byte: K1 has no sort to split)
        return
    assert len(tr) == 1
    # inputs no longer than the key (few symbols: 16 of them) and inputs whose rotations all differ within it: the first sort's
    # order is the final one -- no second gather, no second plane build.  Periodic inputs keep their ties to the last round.
    if name in ("len-2", "len-2-equal", "len-11", "len-12", "len-13", "settled-by-first-sort"):
        assert tr[0]["final"] == 1, tr
    if name in ("one-byte-64K", "ab-64K", "abcabd"):
        assert tr[0]["final"] == 0, tr


def test_reused_context_big_small_big(ctx, early, capfd):
    big, small = oracle.synth_text(29, 1 << 20), oracle.synth_text(30, 5000)
    for data in (big, small, big, oracle.synth_rand(31, 300000), small):
        a, _ = one_shot(ctx, on_device(data))
        assert a == want(data)
    assert len(traces(capfd)) == 5
    # what the context holds afterwards is the finished index: the final BWT and its planes, not the provisional ones
    one_shot(ctx, on_device(big))
    bwt_ref, _ = oracle.bwt_stage(big)
    out = np.empty(len(big), dtype=np.uint8)
    ctx.check(ctx.lib.bce_hip_get_bwt(ctx.h, out.ctypes.data), "bce_hip_get_bwt")
    assert np.array_equal(out, bwt_ref)
    bits = oracle.plane_bits(bwt_ref)
    for plane in (0, 7):
        ctx.check(ctx.lib.bce_hip_get_plane_bits(ctx.h, plane, out.ctypes.data), "bce_hip_get_plane_bits")
        assert np.array_equal(out, bits[plane])


def test_two_gated_contexts_take_turns(early):
    """Two gated contexts, one host thread each, four 1 MiB inputs: the gate is held from the early rounds to the last flush and
    lent behind flushes, K1's second half of one context runs beside the other's work."""
    inputs = [oracle.synth_text(40 + i, 1 << 20) for i in range(4)]
    tens = [on_device(d) for d in inputs]
    ctxs = [bce_amd.api._Ctx(0) for _ in range(2)]
    results, errors, lock, nxt = [None] * 4, [], threading.Lock(), [0]

    def worker(c):
        try:
            c.check(c.lib.bce_hip_set_gated(c.h, 1), "bce_hip_set_gated")
            while True:
                with lock:
                    if errors or nxt[0] >= len(inputs):
                        return
                    i = nxt[0]
                    nxt[0] += 1
                results[i] = one_shot(c, tens[i])[0]
        except Exception as e:
            with lock:
                errors.append(e)
        finally:
            c.lib.bce_hip_set_gated(c.h, 1)

    try:
        th = [threading.Thread(target=worker, args=(c,)) for c in ctxs]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors
        for i, d in enumerate(inputs):
            assert results[i] == want(d), i
    finally:
        for c in ctxs:
            c.close()


_CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
import bce_amd, oracle
ctx = bce_amd.api._Ctx(0)
cases = [oracle.synth_text(51, 256 << 10), oracle.synth_rand(52, 180000), oracle.synth_text(53, 1 << 20), oracle.synth_text(51, 256 << 10)]
for i, data in enumerate(cases):
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    ref = oracle.compress(data)
    for div in (0, 64):
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 12, div), "debug_set")
        arch, st = bce_amd.compress_device(t.data_ptr(), len(data), ctx=ctx)
        assert bytes(arch) == ref, (i, div)
        assert st["nodes"] == 8 * len(data) - 8, (i, st)
ctx.close()
print("CHILD_OK")
'''


@pytest.mark.parametrize("env", [{"BCE_HIP_TEST_OOM": "3"}, {"BCE_HIP_TEST_OOM": "7"}, {"BCE_HIP_CAP32": "1000"},
                                 {"BCE_HIP_TEST_OOM": "5", "BCE_HIP_CAP32": "5000", "BCE_HIP_EARLY_CAP": "20"}])
def test_allocation_failures_and_wide_list_indexing(env):
    """BCE_HIP_TEST_OOM=k fails every k-th device allocation at its first attempt: ctx_trim runs in K1's first half, the provisional
    plane build, the early rounds (phase 6: nothing of the encoder's may go), K1's second half and the resumed rounds.
    BCE_HIP_CAP32=k reads lists of more than k nodes with the 64-bit index.  Both are read once per process: a child."""
    e = dict(os.environ, BCE_HIP_EARLY_TRACE="1", **env)
    e.pop("BCE_HIP_EARLY_ENUM", None)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert len(TRACE.findall(r.stderr)) == 8


def test_plane_mask_mode_gives_the_same_streams(early):
    data = oracle.synth_text(60, 256 << 10)
    t = on_device(data)
    streams = []
    for order in ("early", "0"):
        c = bce_amd.api._Ctx(0)
        try:
            if order == "0":
                early.setenv("BCE_HIP_EARLY_ENUM", "0")
            bce_amd.set_plane_mask(c, 0x0F)
            one_shot(c, t)
            streams.append([bce_amd.plane_stream(c, p).tobytes() for p in range(4)])
        finally:
            c.close()
    assert streams[0] == streams[1] and all(len(s) > 0 for s in streams[0])
    full = bce_amd.api._Ctx(0)
    try:
        one_shot(full, t)
        assert [bce_amd.plane_stream(full, p).tobytes() for p in range(4)] == streams[0]
    finally:
        full.close()
