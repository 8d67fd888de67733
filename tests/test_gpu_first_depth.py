"""GPU: the one-shot compression at every depth of K1's first sort, with the preceding byte carried in the key and without
(api.hip compress_early, k1_bwt.hip k1_first_sort / k1_provisional_bwt).

BCE_K1_KEYBITS forces the depth (h = keybits / bits per symbol), BCE_HIP_CARRY_BYTE=0 the gather.  Every archive must be the
oracle's, and the BCE_HIP_EARLY_TRACE line must name the route the case is meant to test: the depth it got and whether the byte
was carried (8 + h * bits <= 64).  The staged route (bce_hip_bwt) takes no part in any of this and must give the oracle's BWT.
(tests/test_first_depth_cpu.py has the argument's check on the CPU.)"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bce_amd
import oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
TRACE = re.compile(r"early: h (\d+) limit (\d+) (paused|finished) .* depth asked (\d+) got (\d+) carry (\d) plane (\d) early records (\d+) of (\d+) "
                   r"idle ([0-9.]+) ms first_sort_final (\d)")

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


def traces(text):
    return [dict(h=int(m[0]), limit=int(m[1]), paused=m[2] == "paused", asked=int(m[3]), got=int(m[4]), carry=int(m[5]), plane=int(m[6]),
                 early=int(m[7]), records=int(m[8]), idle=float(m[9]), final=int(m[10])) for m in TRACE.findall(text)]


def symbol_bits(data):
    sigma = len(set(data))
    return max(1, (sigma - 1).bit_length())


def most_symbols(bits):
    return min(64 // bits, 16)


def route(data, h, carry):
    """(depth, carried) the forced route must report for this input."""
    bits = symbol_bits(data)
    got = min(h, most_symbols(bits))
    return got, int(bool(carry) and 8 + got * bits <= 64)


@pytest.fixture
def ctx():
    c = bce_amd.api._Ctx(0)
    yield c
    c.close()


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("BCE_HIP_EARLY_TRACE", "1")
    for k in ("BCE_HIP_EARLY_ENUM", "BCE_HIP_EARLY_CAP", "BCE_K1_KEYBITS", "BCE_HIP_CARRY_BYTE"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def force(env, data, h, carry):
    env.setenv("BCE_K1_KEYBITS", str(h * symbol_bits(data)))
    env.setenv("BCE_HIP_CARRY_BYTE", "1" if carry else "0")


def forced(ctx, env, capfd, data, t, h, carry):
    """One compression at depth h: the oracle's archive by the route asked for.  -> (trace, stats)"""
    force(env, data, h, carry)
    capfd.readouterr()
    arch, st = bce_amd.compress_device(t.data_ptr(), t.numel(), ctx=ctx)
    tr = traces(capfd.readouterr().err)
    assert len(tr) == 1, "the early route was not taken"
    tr = tr[0]
    assert bytes(arch) == want(data), (h, carry)
    assert (tr["got"], tr["carry"]) == route(data, h, carry), (h, carry, tr)
    assert tr["h"] == tr["got"] and tr["limit"] == 8 * tr["h"]
    assert tr["early"] <= tr["records"]
    return tr, st


def sigma40_text(seed, n):
    """n bytes over 40 symbols (6 bits each: 9 of them leave room for the byte, 10 do not); the last eighth repeats the first."""
    body = bytes(np.random.RandomState(seed).choice(np.arange(48, 88, dtype=np.uint8), n - n // 8, p=np.arange(1, 41) / 820.0))
    return body + body[:n // 8]


def de_bruijn_pairs(sigma, base=64):
    """sigma^2 bytes over sigma symbols in which every cyclic pair occurs once: all rotations differ within two symbols."""
    a, seq = [0] * (2 * sigma), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, sigma):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(base + s for s in seq)


INPUTS = {
    "text-64K": (lambda: oracle.synth_text(71, 64 << 10), (7, 8, 9, 10, 11, 12)),          # 5-bit symbols: the byte rides up to h = 11
    "text-1M+1": (lambda: oracle.synth_text(72, (1 << 20) + 1), (7, 8, 9, 10, 11, 12)),
    "sigma40-70001": (lambda: sigma40_text(73, 70001), (7, 8, 9, 10)),                     # 6-bit: h <= 9 carries, h = 10 does not
    "rand-64K": (lambda: oracle.synth_rand(74, 64 << 10), (7, 8)),                         # bytes: h = 7 carries, h = 8 gathers
    "ab": (lambda: b"ab" * 4097, (7, 12)),
    "one-byte": (lambda: b"q" * 5000, (7, 12)),
    "two-bytes": (lambda: b"ba", (7, 12)),                                                 # h >= n
    "300B": (lambda: bytes((i * 37 + (i >> 3)) & 0xFF for i in range(300)), (7, 8)),
}
_DATA = {}


def data_of(name):
    if name not in _DATA:
        _DATA[name] = bytes(INPUTS[name][0]())
    return _DATA[name]


@pytest.mark.parametrize("name", list(INPUTS))
def test_every_depth_with_and_without_the_carried_byte(name, ctx, env, capfd):
    data = data_of(name)
    t = on_device(data)
    seen = set()
    stats = []
    for h in INPUTS[name][1]:
        for carry in (1, 0):
            tr, st = forced(ctx, env, capfd, data, t, h, carry)
            seen.add((tr["got"], tr["carry"]))
            stats.append((st["nodes"], st["symbols"], st["rounds"]))
    assert len(set(stats)) == 1                                   # the result's counts do not move with the route
    if name in ("text-64K", "text-1M+1"):
        assert {(h, 1) for h in range(7, 12)} | {(h, 0) for h in range(7, 13)} == seen
    if name == "sigma40-70001":
        assert {(7, 1), (8, 1), (9, 1), (10, 0), (9, 0)} <= seen and (10, 1) not in seen
    if name == "rand-64K":
        assert seen == {(7, 1), (7, 0), (8, 0)}


def test_first_sort_already_final_with_the_byte_carried(ctx, env, capfd):
    """All rotations differ within two symbols: the first sort's order is final, so the bytes read off the keys ARE the BWT (no
    gather at all, no second plane build)."""
    data = de_bruijn_pairs(32)
    t8 = np.frombuffer(data, dtype=np.uint8)
    n = len(data)
    assert n == 1024 and symbol_bits(data) == 5
    pairs = t8.astype(np.int64) * 256 + np.roll(t8, -1)
    assert len(np.unique(pairs)) == n                             # checked here: every cyclic 2-gram, so every h-gram, is distinct
    t = on_device(data)
    for h in (7, 11, 12):
        for carry in (1, 0):
            tr, _ = forced(ctx, env, capfd, data, t, h, carry)
            assert tr["final"] == 1
    force(env, data, 7, 1)
    bce_amd.compress_device(t.data_ptr(), n, ctx=ctx)
    out = np.empty(n, dtype=np.uint8)
    ctx.check(ctx.lib.bce_hip_get_bwt(ctx.h, out.ctypes.data), "bce_hip_get_bwt")
    assert np.array_equal(out, oracle.bwt_stage(data)[0])


def test_reused_context_big_small_big_across_routes(ctx, env, capfd):
    big, small, rand = data_of("text-1M+1"), data_of("300B"), data_of("rand-64K")
    tb, ts, tr_ = on_device(big), on_device(small), on_device(rand)
    for data, t, h, carry in ((big, tb, 8, 1), (small, ts, 7, 1), (big, tb, 12, 0), (rand, tr_, 7, 1), (small, ts, 8, 0), (big, tb, 10, 1), (rand, tr_, 8, 1)):
        forced(ctx, env, capfd, data, t, h, carry)
    # what the context holds afterwards is the finished index of the last input, not the carried provisional one
    forced(ctx, env, capfd, big, tb, 9, 1)
    bwt_ref, _ = oracle.bwt_stage(big)
    out = np.empty(len(big), dtype=np.uint8)
    ctx.check(ctx.lib.bce_hip_get_bwt(ctx.h, out.ctypes.data), "bce_hip_get_bwt")
    assert np.array_equal(out, bwt_ref)


def test_cli_takes_the_same_route(tmp_path, env):
    data = data_of("text-1M+1")
    src, dst = tmp_path / "in.txt", tmp_path / "out.bce"
    src.write_bytes(data)
    bits = symbol_bits(data)
    for h, carry in ((8, 1), (8, 0), (12, 1)):
        e = dict(os.environ, BCE_K1_KEYBITS=str(h * bits), BCE_HIP_CARRY_BYTE=str(carry))
        r = subprocess.run([EXE, "-c", str(dst), str(src)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stdout + r.stderr
        assert dst.read_bytes() == want(data)
        tr = traces(r.stderr)
        assert len(tr) == 1 and (tr[0]["got"], tr[0]["carry"]) == route(data, h, carry), r.stderr


@pytest.mark.parametrize("name", ["text-64K", "sigma40-70001"])
def test_staged_bwt_is_unchanged(name, env):
    """bce_hip_bwt keeps the full key and the gather: the oracle's BWT and offset, and no early route."""
    data = data_of(name)
    bwt, off = oracle.bwt_stage(data)
    rf = bce_amd.RankFile(data, build=False)
    try:
        assert rf.offset() == off and bytes(rf.bwt()) == bytes(bwt)
    finally:
        rf.close()
