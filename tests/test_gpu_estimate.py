"""GPU: bce_hip_estimate -- the archive's size from the model's code lengths, summed on the device (k4_cost.hip).  The sums are
integers, so they are compared EXACTLY with what the oracle's own coder operations sum to (tests/golden/estimate_oracle.json,
made on the CPU), however the rounds and flushes are cut; at size the estimate is compared with the archive the same context
makes next, and timed against it."""
import ctypes as C
import hashlib
import os
import re
import statistics
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

import bce_amd
import oracle
from bce_amd import api
from conftest import ROOT, golden_input, load_fullsize_golden, load_golden

import estimate_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
GOLD = ref.load_golden()
VEC = {(v["name"], v["config"]): v for v in GOLD["vectors"]}
CONFIGS = {"default": None, "scanned": ref.custom_config()}


def _check(e, v, cfg):
    assert e.plane_cost_q24 == v["plane_cost_q24"], v["name"]
    assert e.plane_steps == v["plane_steps"], v["name"]
    assert e.bytes == ref.archive_bytes(v["n"], v["offset"], v["plane_cost_q24"], cfg) == v["archive_bytes"], v["name"]
    assert e.plane_bits == [c / float(1 << 24) for c in v["plane_cost_q24"]]


@pytest.mark.parametrize("cfg_name", ["default", "scanned"])
def test_sums_equal_the_oracles_exactly(cfg_name):
    cfg = CONFIGS[cfg_name]
    ctx = api._Ctx(0)
    try:
        for name, data in ref.inputs():
            _check(bce_amd.estimate(data, cfg), VEC[(name, cfg_name)], cfg)                 # a context of its own
            e = bce_amd.estimate(data, cfg, ctx=ctx)                                        # a context that is reused
            _check(e, VEC[(name, cfg_name)], cfg)
            st = api.stats_of(ctx)
            assert st["symbols"] == sum(e.plane_steps) and st["t_coder"] == 0 and st["t_coder_busy"] == 0, st
            assert st["nodes"] == 8 * len(data) - 8 or len(set(data)) < 3, st
    finally:
        ctx.close()


def test_sums_do_not_depend_on_how_rounds_and_flushes_are_cut(monkeypatch):
    """Small symbol buffers (many flushes, list growth), rounds split plane group by plane group (BCE_HIP_SPLIT_SYMS: K3Args::pmask /
    repeat), the model on a stream of its own (knob 11), no depth-first tail (knob 1): the same sixteen words."""
    names = ("synth-text-1e5", "synth-rand-1e5", "synth-text-1e6")
    data = dict(ref.inputs())

    def run(name, cap=0, knobs=()):
        ctx = api._Ctx(0)
        try:
            ctx.check(ctx.lib.bce_hip_set_symbol_capacity(ctx.h, cap), "bce_hip_set_symbol_capacity")
            for k, val in knobs:
                ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, k, val), "bce_hip_debug_set")
            e = bce_amd.estimate(data[name], ctx=ctx)
            return e, api.stats_of(ctx)
        finally:
            ctx.close()

    for name in names:
        for cap in (3000, 40000):
            e, st = run(name, cap)
            _check(e, VEC[(name, "default")], None)
            assert st["flushes"] >= 4, st
        for knobs in (((11, 1),), ((1, 1),), ((12, 64),)):
            e, st = run(name, 0, knobs)
            _check(e, VEC[(name, "default")], None)
    monkeypatch.setenv("BCE_HIP_SPLIT_SYMS", "20000")
    for name in names:
        for cap in (30000, 9000):
            e, st = run(name, cap)
            _check(e, VEC[(name, "default")], None)
            assert st["split_rounds"] >= 1 or name == "synth-text-1e5", (name, cap, st)     # (its rounds are the narrowest of the three)


_CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import bce_amd
import estimate_ref as ref
vec = {(v["name"], v["config"]): v for v in ref.load_golden()["vectors"]}
for name, data in ref.inputs():
    e = bce_amd.estimate(data)
    v = vec[(name, "default")]
    assert (e.plane_cost_q24, e.plane_steps, e.bytes) == (v["plane_cost_q24"], v["plane_steps"], v["archive_bytes"]), name
print("CHILD_OK")
'''


def test_sums_with_the_wide_list_indexing():
    """BCE_HIP_CAP32 is read once per process: a child process runs the estimates with lists beyond 1000 nodes read the wide way."""
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, BCE_HIP_CAP32="1000"))
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_arguments_in_a_live_context_and_an_encode_after_an_estimate():
    data = oracle.synth_text(21, 300000)
    want = oracle.compress(data)
    ctx = api._Ctx(0)
    try:
        lib, h = ctx.lib, ctx.h
        a = np.frombuffer(data, dtype=np.uint8)
        n = C.c_size_t(5)
        assert lib.bce_hip_estimate_host(h, None, 10, None, None, C.byref(n)) == -1
        assert lib.bce_hip_estimate_device(h, None, 10, None, None, C.byref(n)) == -1
        assert lib.bce_hip_estimate_host(h, a.ctypes.data, 0, None, None, C.byref(n)) == lib.bce_hip_compress(h, a.ctypes.data, 0, None, 0, None) == -1
        assert lib.bce_hip_estimate(h, None, None, C.byref(n)) == -4 and n.value == 5            # nothing loaded: a stage out of order
        # every output may be null, alone or together
        cost, steps = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
        assert lib.bce_hip_estimate_host(h, a.ctypes.data, len(a), None, None, None) == 0
        assert lib.bce_hip_estimate_host(h, a.ctypes.data, len(a), cost, None, None) == 0
        assert lib.bce_hip_estimate_host(h, a.ctypes.data, len(a), None, steps, C.byref(n)) == 0
        full = bce_amd.estimate(data, ctx=ctx)
        assert full.plane_cost_q24 == list(cost) and full.plane_steps == list(steps) and full.bytes == n.value
        assert abs(full.bytes - len(want)) <= ref.error_bound(len(want), GOLD["worst_rel_error"])
        # staged: estimate, then encode the same loaded input; then estimate again with the archive still there
        rf = bce_amd.RankFile(data, ctx=ctx)
        assert lib.bce_hip_estimate(h, cost, steps, C.byref(n)) == 0 and list(cost) == full.plane_cost_q24 and n.value == full.bytes
        assert bytes(bce_amd.BCE().encode(rf)) == want
        assert lib.bce_hip_estimate(h, cost, steps, C.byref(n)) == 0 and list(cost) == full.plane_cost_q24
        assert bytes(api.archive_of(ctx)) == want
        assert bytes(bce_amd.compress(data, ctx=ctx)) == want
    finally:
        ctx.close()


def test_estimate_is_of_the_whole_archive_whatever_the_plane_mask():
    """bce_hip_set_plane_mask makes the rounds of an ENCODE record only the owned planes' symbols (K3Args::pmask); an estimate
    records all of them, leaves the mask as it was, and the masked encode behind it codes what it coded before."""
    data = dict(ref.inputs())
    for name in ("synth-text-1e5", "synth-rand-1e5", "abracadabra"):
        want = oracle.compress(data[name])
        ctx = api._Ctx(0)
        try:
            assert bytes(bce_amd.compress(data[name], ctx=ctx)) == want
            full = [api.plane_stream(ctx, p) for p in range(8)]
            steps = VEC[(name, "default")]["plane_steps"]
            for mask in (0x0F, 0xA1, 0x00):
                api.set_plane_mask(ctx, mask)
                _check(bce_amd.estimate(data[name], ctx=ctx), VEC[(name, "default")], None)
                st = api.stats_of(ctx)
                assert st["symbols"] == sum(VEC[(name, "default")]["plane_steps"]), (name, mask, st)
                bce_amd.compress(data[name], ctx=ctx)                                       # the mask still holds for an encode
                for p in range(8):
                    mine = api.plane_stream(ctx, p)
                    if steps[p] >= 1000:          # (a plane with no or a handful of symbols can have the same few words either way)
                        assert ((mask >> p) & 1) == int(np.array_equal(mine, full[p])), (name, mask, p)
            api.set_plane_mask(ctx, 0xFF)
            assert bytes(bce_amd.compress(data[name], ctx=ctx)) == want
        finally:
            ctx.close()


def _coder_report(err):
    """BCE_HIP_CODER_DEBUG's lines: per plane (symbols, words) as the encode's coder threads counted them."""
    rows = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"coder (\d): busy [0-9.]+ ms, (\d+) symbols, (\d+) words", err)}
    assert sorted(rows) == list(range(8)), err[-2000:]
    return rows


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["synth-text-1e8", "synth-rand-32Mi"])
def test_estimate_then_compress_on_one_context_at_size(name, monkeypatch, capfd):
    v = load_fullsize_golden()[name]
    data = getattr(bce_amd, v["kind"])(v["seed"], v["n"])
    t = torch.from_numpy(data).to("cuda:0")
    torch.cuda.synchronize()
    ctx = api._Ctx(0)
    try:
        e1 = bce_amd.estimate_tensor(t, ctx=ctx)
        st_e = api.stats_of(ctx)
        e2 = bce_amd.estimate_device(t.data_ptr(), t.numel(), ctx=ctx)
        assert (e1.plane_cost_q24, e1.plane_steps, e1.bytes) == (e2.plane_cost_q24, e2.plane_steps, e2.bytes)      # two runs: identical sums
        monkeypatch.setenv("BCE_HIP_CODER_DEBUG", "1")
        capfd.readouterr()
        arch, st_c = bce_amd.compress_device(t.data_ptr(), t.numel(), ctx=ctx)
        report = _coder_report(capfd.readouterr().err)
        monkeypatch.delenv("BCE_HIP_CODER_DEBUG")
    finally:
        ctx.close()
    # the symbols the encode reports, plane by plane, and in all
    assert e1.plane_steps == [report[p][0] for p in range(8)]
    assert sum(e1.plane_steps) == st_c["symbols"] == st_e["symbols"] and st_e["nodes"] == st_c["nodes"] == 8 * v["n"] - 8
    assert st_e["t_coder"] == 0
    # the archive after an estimate: the oracle's, and a fresh context's
    assert len(arch) == v["archive_bytes"] and hashlib.sha256(arch).hexdigest() == v["archive_sha256"]
    fresh, _ = bce_amd.compress_device(t.data_ptr(), t.numel())
    assert bytes(fresh) == bytes(arch)
    bound = ref.error_bound(len(arch), GOLD["worst_rel_error"])
    words = [ref.stream_words(c) for c in e1.plane_cost_q24]
    print("\n%s: estimate %d B, archive %d B, error %+d B (%+.2e; bound %.0f B); per-plane stream words estimated - coded: %s" % (
        name, e1.bytes, len(arch), e1.bytes - len(arch), (e1.bytes - len(arch)) / len(arch), bound, [words[p] - report[p][1] for p in range(8)]))
    assert abs(e1.bytes - len(arch)) <= bound
    assert abs(e1.bytes - len(arch)) <= ref.tight_bound(sum(e1.plane_steps))               # the reasoned bound: tens of bytes


def test_one_context_of_a_pool_estimates_while_another_compresses():
    gv = [v for v in load_golden() if v["name"] == "synth-text-8m"][0]
    data = golden_input(gv)
    solo = bce_amd.estimate(data)
    out, errors = {}, []
    with bce_amd.ContextPool(2) as pool:
        def work(c, what):
            try:
                c.check(c.lib.bce_hip_set_gated(c.h, 1), "bce_hip_set_gated")
                for i in range(3):
                    out[(what, i)] = bce_amd.estimate(data, ctx=c) if what == "estimate" else bytes(bce_amd.compress(data, ctx=c))
            except Exception as e:      # noqa: BLE001
                errors.append(e)
            finally:
                c.lib.bce_hip_set_gated(c.h, 1)      # (not a restore: the call, with either value, gives the gate back if a failed stage left it held)
        th = [threading.Thread(target=work, args=(pool.ctxs[0], "estimate")), threading.Thread(target=work, args=(pool.ctxs[1], "compress"))]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errors, errors
    for i in range(3):
        arch, e = out[("compress", i)], out[("estimate", i)]
        assert len(arch) == gv["archive_bytes"] and hashlib.sha256(arch).hexdigest() == gv["archive_sha256"]
        assert (e.plane_cost_q24, e.plane_steps, e.bytes) == (solo.plane_cost_q24, solo.plane_steps, solo.bytes)


def test_cli_estimate_prints_the_librarys_number_and_writes_nothing(tmp_path):
    data = oracle.synth_text(9, 5 * 10**6)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    cfgf = tmp_path / "scanned.bcc"
    cfgf.write_bytes(CONFIGS["scanned"])
    work = tmp_path / "cwd"
    work.mkdir()
    for args, cfg in (([str(f)], None), ([str(f), str(cfgf)], CONFIGS["scanned"])):
        r = subprocess.run([EXE, "-e"] + args, capture_output=True, text=True, cwd=work, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        m = re.search(r"Estimated size: (\d+) B \(ratio ([0-9.]+)\)", r.stdout)
        e = bce_amd.estimate(data, cfg)
        assert m and int(m.group(1)) == e.bytes and abs(float(m.group(2)) - e.bytes / len(data)) < 1e-4, r.stdout
        planes = re.search(r"Plane bits:((?: [0-9.]+){8})\n", r.stdout)
        assert planes and [float(x) for x in planes.group(1).split()] == [round(b, 1) for b in e.plane_bits], r.stdout
        assert os.listdir(work) == [] and sorted(os.listdir(tmp_path)) == ["cwd", "in.bin", "scanned.bcc"]
    r = subprocess.run([EXE, "-e", str(tmp_path / "missing")], capture_output=True, text=True, cwd=work)
    assert r.returncode == 255 and "Error loading file" in r.stdout
    (tmp_path / "empty").write_bytes(b"")
    r = subprocess.run([EXE, "-e", str(tmp_path / "empty")], capture_output=True, text=True, cwd=work)
    assert r.returncode == 255 and "Error loading file" in r.stdout


@pytest.mark.timeout(900)
def test_estimate_is_faster_than_compress_on_a_warm_context():
    """Median of 5 estimate_device against median of 5 compress_device (the existing path: the yardstick) of synth_text(1, 10^8),
    one warm context, one process.  Asserted: the estimate is faster.  The figures are printed (DESIGN.md 5 quotes a run)."""
    data = bce_amd.synth_text(1, 10**8)
    t = torch.from_numpy(data).to("cuda:0")
    torch.cuda.synchronize()
    ctx = api._Ctx(0)
    try:
        for _ in range(2):                                           # warm: buffers, pinned staging, both paths
            bce_amd.compress_device(t.data_ptr(), t.numel(), ctx=ctx)
            bce_amd.estimate_device(t.data_ptr(), t.numel(), ctx=ctx)
        te, tc, cost_ms = [], [], []
        for _ in range(5):
            t0 = time.perf_counter()
            bce_amd.estimate_device(t.data_ptr(), t.numel(), ctx=ctx)
            te.append(time.perf_counter() - t0)
            st = api.stats_of(ctx)
            cost_ms.append((st["t_model"] - st["t_model_kernels"]) * 1e3)
            t0 = time.perf_counter()
            bce_amd.compress_device(t.data_ptr(), t.numel(), ctx=ctx)
            tc.append(time.perf_counter() - t0)
        st = api.stats_of(ctx)
    finally:
        ctx.close()
    me, mc = statistics.median(te), statistics.median(tc)
    print("\nestimate_device %.1f ms (min %.1f, max %.1f), compress_device %.1f ms (min %.1f, max %.1f): ratio %.2f; cost kernels + run tables %.2f ms of GPU time for %d records"
          % (me * 1e3, min(te) * 1e3, max(te) * 1e3, mc * 1e3, min(tc) * 1e3, max(tc) * 1e3, mc / me, statistics.median(cost_ms), st["symbols"]))
    assert me < mc
