"""CPU: the sequential reference of the K4 model (tests/core_emul.cpp emul_model = bce_core.h's model_step in a loop) against
the rule written out in plain Python, on every record stream of tests/model_cases.py; and, for every stream, the properties it
was built for -- which runs are long, on which lane the reference halves, ... -- computed from the records alone.
tests/test_gpu_model.py puts the same streams through the kernels."""
import numpy as np
import pytest

import model_cases as mc

CASES = mc.all_cases()
PY_RECORDS = 60000      # plain Python takes some microseconds per record: longer streams are compared on this prefix


@pytest.mark.parametrize("name,build", CASES, ids=[n for n, _ in CASES])
def test_reference_and_coverage(name, build):
    case = build()
    assert case.name == name
    n = len(case.keys)
    ref = mc.Reference(case.config)
    # fed in the case's own flushes: the state the caller keeps between calls is the model's whole memory
    out = np.concatenate([ref.step(case.keys[a:b], case.escs[a:b]) for a, b in mc.segments(n, case.cuts)])
    m = min(n, PY_RECORDS)
    want, slots = mc.python_model(case.keys[:m], case.escs[:m])
    assert (out[:m] == want).all(), "record %d" % int(np.flatnonzero(out[:m] != want)[0])
    if m == n:      # ... and the probe records spell out the counters the Python model ends with
        pk, pe = case.probes()
        got = ref.step(pk, pe)
        want, _ = mc.python_model(pk, pe, slots)
        assert (got == want).all()
    an = mc.Analysis(case, out)
    assert case.checks
    for what, fn in case.checks:
        assert fn(an), "%s: no longer %s" % (name, what)
    # every flush of every plan: the long-run count the GPU test will demand is defined
    plans = mc.flush_plans(case, out)
    assert plans["one"] == [] and ("cut64" in plans) == (n > 64)
    for cuts in plans.values():
        assert cuts == sorted(set(cuts)) and all(0 < c < n for c in cuts)


def test_the_families_cover_the_list():
    names = [n for n, _ in CASES]
    for n in (1, 63, 64, 65, 255, 256, 257):
        assert "size-mixed-%d" % n in names and "size-onerun-k2-%d" % n in names and "size-onerun-k3-%d" % n in names
    for must in ("short-runs-3000-slots", "threshold-k2", "threshold-k5", "long-const0", "long-uniform", "long-skew", "long-k31-sym30",
                 "long-group-boundary", "long-halving-lanes", "long-halving-in-head", "k2-zeros", "k2-ones", "k2-alt", "k2-half", "k2-rare",
                 "k2-group-boundary", "k2-counters-carried-at-0xFE", "k2-halving-in-group-edge-windows", "many-long-runs",
                 "planes-default", "planes-random", "planes-bits0", "planes-bits5", "mix-config-bits0", "escape-words", "mix-default-4M"):
        assert must in names


def test_reference_refuses_records_outside_the_config():
    ref = mc.Reference()
    ok = mc.pack_keys(0, 2, [1])
    assert len(ref.step(ok, np.zeros(1, np.uint32))) == 1
    for bad in (0 | (2 << 5) | (1024 << 10),          # slot 1024 belongs to k = 3
                2 | (2 << 5),                         # sym >= k
                0 | (1 << 5),                         # k < 2
                0 | (2 << 5) | (8 << 26)):            # plane 8
        with pytest.raises(ValueError):
            ref.step(np.array([bad], np.uint32), np.zeros(1, np.uint32))


def test_flush_plans_cut_where_a_counter_reaches_0xFE():
    L = mc.Layout()
    L.run(2, np.zeros(600, np.uint32))
    keys, escs = L.stream(1)
    case = mc.Case("x", keys, escs)
    out = mc.Reference().step(keys, escs)
    plans = mc.flush_plans(case, out)
    # zeros from zero counters: the counter is 0xFE behind record 253, halves on 254, is 0xFE again behind 254 + 127, ...
    assert plans["at0xFE"][:2] == [254, 254 + 128]
    assert mc.out_freq(out)[254] == 0xFF and mc.out_freq(out)[253] == 0xFE
    assert plans["cut1"] == list(range(1, 600)) and plans["cut64"] == list(range(64, 600, 64)) and "cut1000" not in plans
