"""GPU: `bce -s` on every enumeration route, record by record.  In scan mode every K3 kernel runs a second instantiation that
writes one scan_pack word per symbol (k3_count2 / k3_tiles / k3_small / k3_tail <true>, the traw branch of k3_dfs.hip,
kd_place_raw_kernel); the archive-equality tests never set scan_mode.  Here the test hook bce_hip_scan_records returns the
words the eight ScanCoders are fed, and they are held against the oracle's trace packed by tests/scanrec_ref.py -- on a
mismatch the plane, the index and both words unpacked are named -- then bce_hip_scan runs on the same context and must give
oracle.scan's table and its nine doubles.  Everything is exact.  tests/test_scanrec_cpu.py checks the reference on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bce_amd
import estimate_ref
import oracle
import scanrec_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

E_ARG, E_NOMEM, E_STATE, E_OVERFLOW = -1, -3, -4, -5


# ---- running one case -------------------------------------------------------------------------------------------------------------
def _set_knobs(ctx, knobs):
    for k, v in knobs.items():
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, k, v), "bce_hip_debug_set")


def _rank_file(name, ctx):
    data = ref.family_input(name)
    if name in ref.INJECTED:
        bwt, off = oracle.bwt_stage(data)
        return bce_amd.RankFile(bwt=bwt, offset=off, ctx=ctx)
    return bce_amd.RankFile(data, ctx=ctx)


def scan_records(ctx, cap_words):
    """bce_hip_scan_records -> (status, the eight streams or None, counts)."""
    out = np.full(max(cap_words, 1), 0xDEADBEEF, dtype=np.uint32)
    counts = (C.c_uint64 * 8)()
    rc = ctx.lib.bce_hip_scan_records(ctx.h, out.ctypes.data, cap_words, counts)
    counts = [int(v) for v in counts]
    if rc != 0:
        return rc, (None if rc != E_OVERFLOW else out), counts
    ends = np.cumsum([0] + counts)
    return rc, [out[ends[p]:ends[p + 1]] for p in range(8)], counts


def scan(ctx):
    cfg = np.zeros(288, dtype=np.uint8)
    res = (C.c_double * 9)()
    ctx.check(ctx.lib.bce_hip_scan(ctx.h, cfg.ctypes.data, res), "bce_hip_scan")
    return cfg.tobytes(), tuple(res)


def check_records(ctx, name):
    """The records of the loaded input against the reference; -> bce_hip_stats after the call."""
    want, _, _ = ref.family_reference(name)
    rc, got, counts = scan_records(ctx, 8 * len(ref.family_input(name)) + 64)      # (a node codes at most one symbol)
    assert rc == 0, (rc, ctx.lib.bce_hip_last_error(ctx.h).decode())
    bad = ref.first_mismatch(got, want)
    assert bad is None, "%s: %s" % (name, bad)
    st = bce_amd.stats_of(ctx)
    assert sum(counts) == st["symbols"] == sum(len(w) for w in want)
    return st


def check_scan(ctx, name):
    _, cfg_want, res_want = ref.family_reference(name)
    cfg, res = scan(ctx)
    assert cfg == cfg_want, name
    assert res == res_want, name
    return bce_amd.stats_of(ctx)


def run_case(name, knobs=None, capacity=0):
    """One family on a context with the knobs set: the records, then the table on the same input and context.
    -> the statistics after the records."""
    ctx = bce_amd.api._Ctx(0)
    try:
        _set_knobs(ctx, knobs or {})
        ctx.check(ctx.lib.bce_hip_set_symbol_capacity(ctx.h, capacity), "bce_hip_set_symbol_capacity")
        _rank_file(name, ctx)
        st = check_records(ctx, name)
        st2 = check_scan(ctx, name)
        for key in ("nodes", "rounds", "symbols"):                                      # the hook's statistics are the scan's
            assert st[key] == st2[key], (key, st[key], st2[key])                      # (flushes and spine_levels depend on timing)
        return st
    finally:
        ctx.close()


def encode_stats(name):
    ctx = bce_amd.api._Ctx(0)
    try:
        rf = _rank_file(name, ctx)
        arch = bce_amd.BCE().encode(rf)
        assert arch == oracle.compress(ref.family_input(name))
        return bce_amd.stats(rf)
    finally:
        ctx.close()


_default = {}


def default_stats(name):
    """The statistics of the family's scan with no knob (run once: the evidence of a knob is a difference from them)."""
    if name not in _default:
        _default[name] = run_case(name)
    return _default[name]


# ---- every family, no knob ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.FAMILIES) + list(ref.INJECTED))
def test_scan_records_and_table_of_every_family(name):
    st = default_stats(name)
    enc = encode_stats(name)
    for key in ("nodes", "rounds", "symbols"):                                         # the same enumeration as `bce -c`'s
        assert st[key] == enc[key], (key, st[key], enc[key])
    data = ref.family_input(name)
    if ref.is_primitive(data):
        assert st["nodes"] == 8 * len(data) - 8


# ---- the four knob families under every knob ----------------------------------------------------------------------------------------
# (id, test knobs, environment, symbol capacity)
VARIANTS = [
    ("no-dfs", {1: 1}, {}, 0),
    ("rounds-only", {1: 1, 2: 1}, {}, 0),
    ("wide-rounds-only", {1: 1, 2: 1, 4: 1}, {}, 0),
    ("no-small", {4: 1}, {}, 0),
    ("three-launch-rounds", {6: 1}, {}, 0),
    ("no-skip", {3: 1}, {}, 0),
    ("dfs-short-passes", {0: 9}, {}, 0),
    ("no-local", {7: 1}, {}, 0),
    ("local-from-64", {8: 64}, {}, 0),
    ("local-budget-3", {8: 64, 9: 3}, {}, 0),
    ("tail-from-round-17", {8: 64, 10: 17}, {}, 0),
    ("k4-beside-k3", {11: 1}, {}, 0),                      # scan mode ignores it: the same records
    ("lists-grow-no-dfs", {12: 1 << 30, 1: 1}, {}, 0),
    ("env-scan-no-dfs", {}, {"BCE_HIP_SCAN_NO_DFS": "1"}, 0),
    ("env-no-spine", {}, {"BCE_HIP_NO_SPINE": "1"}, 0),
    ("capacity-1000", {}, {}, 1000),
    ("capacity-40000", {}, {}, 40000),
]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("name", ref.KNOB_FAMILIES)
def test_scan_records_and_table_under_every_knob(name, variant, monkeypatch):
    vid, knobs, env, capacity = variant
    base = default_stats(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = run_case(name, knobs, capacity)
    assert st["nodes"] == base["nodes"] and st["symbols"] == base["symbols"]
    # proof that the route ran (unconditional: without it the default route gives the same words and the case proves nothing)
    if name == "spine" and vid == "env-no-spine":
        assert st["spine_levels"] == 0
    if name == "rand-64k" and vid == "capacity-1000":
        assert st["flushes"] > 5, st
    if name == "repeat" and vid == "capacity-1000":
        # the tail's own symbols exceed the 1000 records: k3_grow_symbols regrew scanrec under it (the records above are right)
        assert st["flushes"] >= 1, st
    if name == "rand-64k" and vid == "lists-grow-no-dfs":
        assert st["list_grows"] >= 2, st
    if name == "repeat" and vid in ("no-dfs", "env-scan-no-dfs"):
        assert st["k3_launches"] > base["k3_launches"], (st["k3_launches"], base["k3_launches"])


# The spine input is _spine_input("zero-runs") with ref.SPINE_RUNS = 25 runs in ref.SPINE_TEXT = 40 000 bytes of text (70 683 bytes).
# Of the run counts tried on the MI355X -- 200 (323 428 bytes) down to 25 in steps of 25 -- every one had spine bursts in the default
# encode: spine_levels 20847, 20531, 18355, 15522, 12768, 12109, 9339 and, at 25 runs, 5096.  (The count varies by a few
# levels from run to run: which walker reaches a chain first depends on timing.)
def test_spine_bursts_feed_the_scan_branch():
    st = default_stats("spine")
    assert st["spine_levels"] > 0, st
    assert encode_stats("spine")["spine_levels"] > 0


@pytest.mark.parametrize("name", ["stair-period2-twice", "stair-zeros"])
def test_staircases_are_expanded_in_scan_mode(name, capfd, monkeypatch):
    """The closed forms (stair_event, stairs_run, kd_jobs_kernel) must run in scan mode on the inputs made for them."""
    monkeypatch.setenv("BCE_HIP_DFS_DEBUG", "1")
    capfd.readouterr()
    run_case(name)
    err = capfd.readouterr().err
    m = re.findall(r"stairs (\d+) \+ (\d+) of several regions \((\d+) symbols\)", err)
    assert m, err[-2000:]
    single, several = max(int(a) for a, _, _ in m), max(int(b) for _, b, _ in m)
    assert single >= 1, m
    if name == "stair-period2-twice":
        assert several >= 1, m
    else:                                      # the 9000-byte run is above KD_JOB_MIN: it goes to the staircase jobs
        jobs = [int(v) for v in re.findall(r"staircase jobs so far: (\d+)", err)]
        assert jobs and max(jobs) >= 1, err[-2000:]


# ---- one context, alternating ---------------------------------------------------------------------------------------------------------
def test_scan_encode_records_estimate_scan_on_one_context():
    """A scan_mode that sticks, or a dfs buffer carved once with and once without the raw array, shows in the call after."""
    name = "stair-period2-twice"
    data = ref.family_input(name)
    arch = oracle.compress(data)
    n, offset, plane_cost, plane_steps = estimate_ref.oracle_sums(data)
    ctx = bce_amd.api._Ctx(0)
    try:
        rf = bce_amd.RankFile(data, ctx=ctx)
        check_scan(ctx, name)
        assert bce_amd.BCE().encode(rf) == arch
        check_records(ctx, name)
        cost, steps, size = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), C.c_size_t()
        ctx.check(ctx.lib.bce_hip_estimate(ctx.h, cost, steps, C.byref(size)), "bce_hip_estimate")
        assert list(cost) == plane_cost and list(steps) == plane_steps
        assert size.value == estimate_ref.archive_bytes(n, offset, plane_cost)
        check_scan(ctx, name)
        assert bce_amd.BCE().encode(rf) == arch              # and the archive after the last scan
    finally:
        ctx.close()


def test_a_scan_that_finds_no_memory_fails_cleanly():
    """Knob 14 = 2 with lists of 4096 nodes (knob 12) and no depth-first tail (knob 1): the first list growth is refused.  Both
    calls end with BCE_HIP_E_NOMEM; the knobs cleared, the same context encodes to the oracle's archive and scans to its table."""
    name = "rand-64k"
    data = ref.family_input(name)
    ctx = bce_amd.api._Ctx(0)
    try:
        _set_knobs(ctx, {12: 1 << 30, 1: 1, 14: 2})
        bce_amd.RankFile(data, ctx=ctx)
        rc, _, _ = scan_records(ctx, 8 * len(data))
        assert rc == E_NOMEM and "k3: no device memory for node lists of" in ctx.lib.bce_hip_last_error(ctx.h).decode()
        bce_amd.RankFile(data, ctx=ctx)
        with pytest.raises(bce_amd.BceError) as e:
            scan(ctx)
        assert e.value.status == E_NOMEM, str(e.value)
        _set_knobs(ctx, {12: 0, 1: 0, 14: 0})
        rf = bce_amd.RankFile(data, ctx=ctx)
        assert bce_amd.BCE().encode(rf) == oracle.compress(data)
        check_scan(ctx, name)
        check_records(ctx, name)
    finally:
        ctx.close()


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_scan_records_arguments():
    name = "edge-len-3073"
    data = ref.family_input(name)
    want, _, _ = ref.family_reference(name)
    total = sum(len(w) for w in want)
    ctx = bce_amd.api._Ctx(0)
    try:
        counts = (C.c_uint64 * 8)()
        out = np.zeros(total, dtype=np.uint32)
        assert ctx.lib.bce_hip_scan_records(ctx.h, out.ctypes.data, total, counts) == E_STATE            # nothing loaded
        bce_amd.RankFile(data, ctx=ctx, build=False)
        assert ctx.lib.bce_hip_scan_records(ctx.h, out.ctypes.data, total, counts) == E_STATE            # before build_planes
        assert ctx.lib.bce_hip_scan_records(None, out.ctypes.data, total, counts) == E_ARG
        bce_amd.RankFile(data, ctx=ctx)
        assert ctx.lib.bce_hip_scan_records(ctx.h, out.ctypes.data, total, None) == E_ARG                # null counts
        assert ctx.lib.bce_hip_scan_records(ctx.h, None, total, counts) == E_ARG
        rc, out, counts = scan_records(ctx, total - 1)                                                   # one word short
        assert rc == E_OVERFLOW and counts == [len(w) for w in want]
        assert (out == 0xDEADBEEF).all()                                                                 # out untouched
        rc, got, counts = scan_records(ctx, total)                                                       # exactly enough
        assert rc == 0 and ref.first_mismatch(got, want) is None
        check_scan(ctx, name)
    finally:
        ctx.close()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_scan_of_a_staircase_file(tmp_path):
    name = "stair-period2-twice"
    _, cfg_want, res_want = ref.family_reference(name)
    src, cf = tmp_path / "in.bin", tmp_path / "c.bcc"
    src.write_bytes(ref.family_input(name))
    r = subprocess.run([os.path.join(ROOT, "bce_amd", "bin", "bce"), "-s", str(cf), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert cf.read_bytes() == cfg_want
    assert re.findall(r"Result size: (\S+) B", r.stdout) == ["%.1f" % v for v in res_want]
