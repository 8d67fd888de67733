"""GPU: the K4 model kernels (bce_amd/csrc/k4_model.hip) on their own, against the sequential reference.

bce_hip_model_flush hands K4 records of the test's choosing -- the streams of tests/model_cases.py, one per route and edge of a
flush (tests/test_model_cpu.py proves on the CPU that each stream has the property it is named for) -- and gives back the raw
64-bit model records and the number of long runs the window kernel queued.  Every case: bit-exact on every record against
emul_model (tests/core_emul.cpp, bce_core.h's model_step in a loop); the same with the stream cut into flushes in several ways,
the counters going through HBM in between; the counters afterwards, by k probe records per touched slot; and the long-run count
of every flush against the runs of 256 and more records the test counts itself.

Mutants of k4_model.hip (arithmetic only; built on a scratch copy, never committed) that this file was run against, with the
first case that caught each:
  k4_replay's halving          C = (C + 1) >> 1                        size-onerun-k2-255
  the general long walk        C = ((C + cle + 1) >> 1) + (h - cle)    size-onerun-k3-256
  the k = 2 walker             c1 = (s1 + cle1 + 1) >> 1               tail-long-k2-1100-rag37
  the emit kernel's start      stateW[..] + 1 on lane 0                size-onerun-k2-256
"""
import time

import numpy as np
import pytest

import bce_amd
import model_cases as mc
import oracle
from bce_amd.api import Model, _Ctx

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx(0)
    yield c
    c.close()


def fields(rec):
    rec = int(rec)
    return "cum %d freq %d total %d esc %#x" % (rec & 0x1FFF, ((rec >> 13) & 0xFF) + 1, (rec >> 21) & 0x1FFF, rec >> 34)


def explain(keys, lo, hi, got, want, what):
    """the first record of flush [lo, hi) that differs: where it sits in the sorted array and in its run"""
    i = int(np.flatnonzero(got != want)[0])
    order, starts, lens, _ = mc.run_table(keys[lo:hi])
    pos = int(np.flatnonzero(order == i)[0])
    r = int(np.searchsorted(starts, pos, side="right") - 1)
    kw = int(keys[lo + i])
    return ("%s: record %d (flush [%d, %d), %d wrong): plane %d slot %d k %d sym %d; sorted position %d = lane %d of window %d; "
            "record %d of a run of %d that starts on lane %d; got %s, want %s"
            % (what, lo + i, lo, hi, int((got != want).sum()), kw >> 26, (kw >> 10) & 0xFFFF, (kw >> 5) & 31, kw & 31, pos, pos % 64,
               pos // 64, pos - int(starts[r]), int(lens[r]), int(starts[r]) % 64, fields(got[i]), fields(want[i])))


def run_plan(model, keys, escs, cuts, want, what):
    """begin, then the stream in the plan's flushes: every flush's records and long-run count"""
    model.begin()
    for lo, hi in mc.segments(len(keys), cuts):
        got, nq = model.flush(keys[lo:hi], escs[lo:hi])
        assert (got == want[lo:hi]).all(), explain(keys, lo, hi, got, want[lo:hi], what)
        exp = mc.long_run_count(keys[lo:hi]) if hi - lo >= mc.LONG else 0
        assert nq == exp, "%s: flush [%d, %d) queued %d long runs, its records hold %d runs of >= 256" % (what, lo, hi, nq, exp)


@pytest.mark.parametrize("name,build", CASES, ids=[n for n, _ in CASES])
def test_model_kernels_match_the_reference(ctx, name, build):
    case = build()
    t0 = time.time()
    ref = mc.Reference(case.config)
    want = ref.step(case.keys, case.escs)
    pk, pe = case.probes()
    want_probe = ref.step(pk, pe)
    model = Model(config=case.config, ctx=ctx)
    plans = mc.flush_plans(case, want)
    for pname, cuts in plans.items():
        what = "%s, plan %s (%d flushes)" % (name, pname, len(cuts) + 1)
        run_plan(model, case.keys, case.escs, cuts, want, what)
        got, _ = model.flush(pk, pe)            # the counters the plan left behind, k records per touched slot
        assert (got == want_probe).all(), explain(pk, 0, len(pk), got, want_probe, what + ", probe of the counters")
    print("%s: %d records, %d probes, plans %s, %.2f s" % (name, len(case.keys), len(pk), " ".join(plans), time.time() - t0))


def test_empty_flush_and_order_of_calls(ctx):
    fresh = _Ctx(0)
    try:
        one = np.array([0 | (2 << 5)], np.uint32)
        with pytest.raises(bce_amd.BceError) as e:
            Model(ctx=fresh).flush(one, np.zeros(1, np.uint32))
        assert e.value.status == -4                                     # BCE_HIP_E_STATE: no begin
        m = Model(ctx=fresh)
        m.begin()                                                       # needs no loaded input
        got, nq = m.flush(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        assert len(got) == 0 and nq == 0
        got, nq = m.flush(one, np.zeros(1, np.uint32))
        assert (got == mc.Reference().step(one, np.zeros(1, np.uint32))).all() and nq == 0
    finally:
        fresh.close()


def test_natural_records_replayed_through_both_interfaces():
    """The records K3 emits for 300 000 bytes of text: bce_hip_enum_model (flushed after uneven numbers of rounds) and
    bce_hip_model_flush on a fresh begin (cut at other, uneven places) agree, and both agree with the reference."""
    data = oracle.synth_text(2, 300000)
    rf = bce_amd.RankFile(data)
    try:
        bce = bce_amd.BCE()
        bce.code_begin(rf)
        cap = 8 * len(data)
        flush_after = {1, 2, 5, 6, 13, 14, 15, 31, 50, 90}
        syms, ops, r = [], [], 0
        while True:
            nxt = bce.code_round(rf)
            r += 1
            assert r < 100000
            if r in flush_after or nxt == 0:
                s = bce.code_symbols(rf, cap)
                o = bce.code_model(rf, cap)
                assert len(s) == len(o)
                syms.append(s)
                ops.append(o)
            if nxt == 0:
                break
        assert len(syms) >= 5
        syms, ops = np.concatenate(syms), np.concatenate(ops)
        n = len(syms)
        assert n > 100000
        keys = (syms[:, 1] | (syms[:, 2] << 5) | (syms[:, 5] << 10) | (syms[:, 0] << 26)).astype(np.uint32)
        escs = (syms[:, 4] | (syms[:, 3] << 27)).astype(np.uint32)
        want = mc.Reference().step(keys, escs)
        want3 = np.stack([want & np.uint64(0x1FFF), ((want >> np.uint64(13)) & np.uint64(0xFF)) + np.uint64(1),
                          (want >> np.uint64(21)) & np.uint64(0x1FFF)], axis=1).astype(np.uint32)
        assert (ops == want3).all(), "bce_hip_enum_model, record %d" % int(np.flatnonzero((ops != want3).any(axis=1))[0])
        rng = np.random.RandomState(5)
        cuts = sorted(set(int(x) for x in np.concatenate([rng.randint(1, n, 7), [1, 65, n - 1]])))
        run_plan(Model(ctx=rf._c), keys, escs, cuts, want, "natural records")
        run_plan(Model(ctx=rf._c), keys, escs, [], want, "natural records, one flush")
    finally:
        rf.close()


def test_records_that_would_leave_the_counter_array_are_refused(ctx):
    """One record of each invalid kind, behind valid ones: BCE_HIP_E_ARG, nothing applied; the context goes on, bit-exact."""
    geo = mc.Geometry()
    rng = np.random.RandomState(6)
    g, k = geo.pick(rng, 50)
    a = mc.make_stream([(g[i], k[i], rng.randint(0, k[i], 300)) for i in range(50)], rng)
    b = mc.make_stream([(g[i], k[i], rng.randint(0, k[i], 300)) for i in range(50)], rng)
    ref = mc.Reference()
    want_a = ref.step(*a)
    model = Model(ctx=ctx)
    model.begin()
    got, _ = model.flush(*a)
    assert (got == want_a).all()
    last31 = int(geo.ctxoff[0, 31] + geo.nctx[0, 31] - 1)
    bad = [
        ("plane 8", 0 | (2 << 5) | (1 << 29), 0),
        ("plane 15", 0 | (2 << 5) | (7 << 26) | (1 << 29), 0),
        ("k = 0", 0, 0),
        ("k = 1", 0 | (1 << 5), 0),
        ("sym = k", 2 | (2 << 5), 0),
        ("sym > k", 31 | (30 << 5) | (int(geo.ctxoff[0, 30]) << 10), 0),
        ("slot below the k's block", 0 | (3 << 5) | (0 << 10), 0),
        ("slot behind the k's block", 0 | (2 << 5) | (1024 << 10), 0),
        ("slot behind the plane's last", 0 | (31 << 5) | ((last31 + 1) << 10), 0),
        ("slot 65535", 0 | (31 << 5) | (65535 << 10), 0),
        ("nesc > 0 with k < 16", 0 | (15 << 5) | (int(geo.ctxoff[0, 15]) << 10), 1 << 27),
        ("nesc = 28", 0 | (16 << 5) | (int(geo.ctxoff[0, 16]) << 10), 28 << 27),
        ("nesc = 31", 0 | (16 << 5) | (int(geo.ctxoff[0, 16]) << 10), (31 << 27) | 5),
        ("escape bits at or above nesc", 0 | (16 << 5) | (int(geo.ctxoff[0, 16]) << 10), (2 << 27) | 4),
        ("escape bits with nesc = 0, k < 16", 0 | (2 << 5), 1),
    ]
    for what, kw, ew in bad:
        keys = np.concatenate([b[0][:500], [kw]]).astype(np.uint32)
        escs = np.concatenate([b[1][:500], [ew]]).astype(np.uint32)
        with pytest.raises(bce_amd.BceError) as e:
            model.flush(keys, escs)
        assert e.value.status == -1, what
    # the valid neighbours of each of them are accepted
    for kw, ew in ((0 | (2 << 5) | (1023 << 10), 0),
                   (0 | (16 << 5) | (int(geo.ctxoff[0, 16]) << 10), (27 << 27) | (1 << 26))):
        one_k, one_e = np.array([kw], np.uint32), np.array([ew], np.uint32)
        got, _ = model.flush(one_k, one_e)
        assert (got == ref.step(one_k, one_e)).all()
    want_b = ref.step(*b)                      # (the reference went through the two accepted records as well)
    got, _ = model.flush(*b)
    assert (got == want_b).all(), explain(b[0], 0, len(b[0]), got, want_b, "the flush behind the refused ones")
