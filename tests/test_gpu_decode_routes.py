"""GPU: every route of the GPU-assisted decoder (kd_decode.hip drives; kd_rounds.hip, kd_tail.hip, kd_host_tail.hip) against the oracle's archives, under list growth and small query
budgets -- the exact input comes back, and every case shows from the decoder's own summary lines that its route and its memory
mode actually ran.

The decoder picks a route per round: one launch (dec_small_kernel), six launches plane by plane, or all planes at once
(BCE_DEC_NO_SPLIT); the tail kernels (dec_tail64_kernel / dec_tail_kernel, with or without the mailbox); the host tail
(dec_host_tail), entered early where eight CPUs of one L3 domain are there for it, after the probe, or forced; and the lists handed
back after the rounds.  Environment switches force each one (ROUTES); test knobs 12 (lists of 4096 nodes that grow in place) and
13 (a query budget of 4096 nodes: plane groups) force the memory modes (MODES).  The product is covered in three layers: every
route x every mode on text and random bytes, every other family x every route, every other family x every mode.

Evidence comes from the lines BCE_DEC_TIMING / BCE_ALLOC_TRACE print (_metrics) and from bce_hip_stats deltas.  A route is proven
by comparing the case with the same family and mode on the default route (_baseline): it must hold what the switch promises
(holds) and the family must reach the code the switch changes (reaches) -- except where NOT_REACHED says why it cannot."""
import functools
import re

import numpy as np
import pytest

import bce_amd
import oracle
from test_gpu_decode_bounded import _long_zero_run
from test_gpu_tail import many_copies, repeat_input

pytestmark = pytest.mark.gpu


def _query_tail():
    """The query-heavy tail of test_tail_query_rounds_with_and_without_the_mailbox: a row leaves a run or a table every few rounds."""
    text = oracle.synth_text(23, 80000)
    return (text[:30000] + bytes(6000) + text[30000:50000] + (b"\x00\x02" * 2500) + b"\x07" + text[50000:] +
            bytes(3000) + b"\x01" + (b"\x00\x02" * 1800))


def _low_planes():
    """Binary with constant high planes: every byte is x << 3 with x < 4 (planes 0-2 and 5-7 hold one value)."""
    return (np.random.RandomState(5).randint(0, 4, 600000).astype(np.uint8) << 3).tobytes()


# (input, config or None).  Built the first time a test asks: oracle.synth_*, not bce_amd's -- loading the HIP library while the
# tests are collected takes the device away from torch in the same process (see test_gpu_decode_bounded.py).
_FAMILIES = {
    "text": lambda: (oracle.synth_text(12, 1_000_000), None),
    "rand": lambda: (oracle.synth_rand(12, 400_000), None),
    "low-planes": lambda: (_low_planes(), None),
    "zero-run": lambda: (_long_zero_run(), None),
    "many-copies": lambda: (many_copies(700, 1000, 31), None),
    "repeat": lambda: (repeat_input(1 << 20, 20000), None),
    "periodic": lambda: (oracle.synth_text(2, 200_000) * 5, None),       # five LF cycles: expand_cycle_kernel
    "query-tail": lambda: (_query_tail(), None),
    "cfg-random": lambda: (oracle.synth_text(14, 400_000), np.random.RandomState(7).randint(0, 6, 288).astype(np.uint8).tobytes()),
    "cfg-0": lambda: (oracle.synth_text(14, 400_000), bytes(288)),
    "cfg-5": lambda: (oracle.synth_text(14, 400_000), bytes([5]) * 288),
}
FAMILIES = list(_FAMILIES)
WIDE = ["text", "rand"]                          # every route x every mode
OTHERS = [f for f in FAMILIES if f not in WIDE]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(input, the oracle's archive of it)."""
    data, cfg = _FAMILIES[name]()
    return data, oracle.compress(data, cfg)


ROUTES = {
    "default": {},
    "no-split": {"BCE_DEC_NO_SPLIT": "1"},
    "no-small": {"BCE_DEC_NO_SMALL": "1"},
    "no-small-no-split": {"BCE_DEC_NO_SMALL": "1", "BCE_DEC_NO_SPLIT": "1"},
    "no-mailbox": {"BCE_DEC_NO_MAILBOX": "1"},
    "no-tail": {"BCE_DEC_NO_TAIL": "1"},
    "host-enter-0": {"BCE_DEC_HOST_ENTER": "0"},
    "host-enter-200k": {"BCE_DEC_HOST_ENTER": "200000"},
    "force-host-tail": {"BCE_DEC_FORCE_HOST_TAIL": "1"},
    "no-host-tail": {"BCE_DEC_NO_HOST_TAIL": "1"},
    "tail-serial": {"BCE_DEC_TAIL_SERIAL": "1"},
    "no-early-pin": {"BCE_DEC_NO_EARLY_PIN": "1"},
    "no-probe": {"BCE_DEC_NO_PROBE": "1"},
    # (the registered mapping BCE_DEC_NO_HUGE switches off is made from 256 MB of boundary ranks on: BCE_HIP_REG_MIN=1 makes it here)
    "no-huge": {"BCE_DEC_NO_HUGE": "1", "BCE_HIP_REG_MIN": "1"},
    "tail-nopin": {"BCE_DEC_TAIL_NOPIN": "1"},
    "give-back": {"BCE_DEC_GIVE_BACK": "1"},
}
_ALL_SWITCHES = sorted({k for env in ROUTES.values() for k in env})

MODES = {"none": {}, "grow": {12: 1 << 30}, "groups": {13: 4096}, "grow+groups": {12: 1 << 30, 13: 4096}}


def _metrics(err):
    """What the decoder's summary lines say about one decode (BCE_DEC_TIMING=1, BCE_ALLOC_TRACE=1)."""
    def one(pat, cast=int):
        m = re.search(pat, err)
        assert m, "summary line missing: %r\n%s" % (pat, err[-3000:])
        return tuple(cast(g) if g is not None else None for g in m.groups()) if len(m.groups()) > 1 else cast(m.group(1))
    rounds, tail_rounds, mbox = one(r"gpu decode: (\d+) rounds \((\d+) of them in the tail kernels, (\d+) query rounds answered through the mailbox\)")
    ncpu, early = one(r"host tail CPUs: (\d+) of one L3 domain in the affinity mask, \d+ hardware threads: tails go to the host early (\d)")
    probe_rounds, _, _ = one(r"tail probe: (\d+) rounds, (\d+) query rounds through the mailbox since it began; query-heavy (\d)")
    groups, _, grown = one(r"(\d+) rounds over the query budget of (\d+) nodes run in plane groups, (\d+) node lists grown in place")
    host = re.findall(r"gpu decode: (\d+) rounds of the (deep )?tail on the host( from \d+ nodes a round on)?", err)
    on = re.findall(r"gpu decode: host tail on (one thread|eight threads of one L3 domain|eight threads, not pinned)", err)
    return {
        "rounds": rounds, "tail_rounds": tail_rounds, "mbox": mbox, "ncpu": ncpu, "ccx": bool(early), "probe_rounds": probe_rounds,
        "group_rounds": groups, "grown": grown,
        "small": one(r"(\d+) rounds in two launches \(dec_small_kernel\)"),
        "six": one(r"(\d+) six-launch rounds plane by plane"),
        "host_rounds": sum(int(r) for r, _, _ in host),
        "host_tail": bool(host),
        "host_early": any(f for _, _, f in host),                     # entered at a round of <= BCE_DEC_HOST_ENTER nodes
        "host_deep": any(d for _, d, _ in host),                      # after a long chain in the wave kernel
        "host_on": on,
        "early_pin": "beside the rounds" in err,
        "given_back": "node lists and query buffers given back" in err,
        "grow_lines": len(re.findall(r"does not fit the node lists: .* grown in place to \d+", err)),
    }


def _decode(family, knobs, capfd):
    """Decode the family's archive in a fresh context with `knobs`, under the trace switches: (stats deltas, _metrics)."""
    data, arch = _case(family)
    ctx = bce_amd.api._Ctx(0)
    try:
        for k, v in knobs.items():
            ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, k, v), "bce_hip_debug_set")
        s0 = bce_amd.stats_of(ctx)
        capfd.readouterr()
        out = np.empty(len(data), dtype=np.uint8)
        assert bce_amd.decompress_device(arch, ctx=ctx, out=out) == len(data)
        err = capfd.readouterr().err
        assert out.tobytes() == data, family
        s1 = bce_amd.stats_of(ctx)
    finally:
        ctx.close()
    d = {k: s1[k] - s0[k] for k in ("dec_restarts", "dec_list_grows", "dec_split_rounds", "reg_maps")}
    return d, _metrics(err)


def _run(family, route, mode, capfd, monkeypatch):
    for k in _ALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BCE_DEC_TIMING", "1")
    monkeypatch.setenv("BCE_ALLOC_TRACE", "1")
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    d, m = _decode(family, MODES[mode], capfd)
    # the memory mode ran, and no decode started again
    assert d["dec_restarts"] == 0, d
    assert m["grown"] == d["dec_list_grows"] == m["grow_lines"] and m["group_rounds"] == d["dec_split_rounds"], (d, m)
    if 12 in MODES[mode]:
        assert d["dec_list_grows"] >= 1, d
    else:
        assert d["dec_list_grows"] == 0, d                          # (the default lists hold every round of these inputs)
    if 13 in MODES[mode]:
        assert d["dec_split_rounds"] >= 1, d
    else:
        assert d["dec_split_rounds"] == 0, d
    return d, m


_BASE = {}


def _baseline(family, mode, capfd):
    """The same family and mode on the default route (decoded once per session)."""
    if (family, mode) not in _BASE:
        with pytest.MonkeyPatch.context() as mp:
            _BASE[(family, mode)] = _run(family, "default", mode, capfd, mp)
    return _BASE[(family, mode)]



# Per route: what the switch promises (holds: this case's metrics m) and what shows that the family reaches the code it changes
# (reaches: the same family and mode on the default route, b; this case's m where the route's own effect is what counts).
_HOST_ON = {"one thread", "eight threads of one L3 domain", "eight threads, not pinned"}
RULES = {
    "default": (lambda m: m["rounds"] > 0, lambda b, m: True),
    "no-split": (lambda m: m["six"] == 0, lambda b, m: b["six"] > 0),
    "no-small": (lambda m: m["small"] == 0, lambda b, m: b["small"] > 0),
    "no-small-no-split": (lambda m: m["small"] == 0 and m["six"] == 0, lambda b, m: b["small"] > 0),
    "no-mailbox": (lambda m: m["mbox"] == 0, lambda b, m: b["mbox"] > 0),
    "no-tail": (lambda m: m["tail_rounds"] == 0 and not m["host_tail"], lambda b, m: b["tail_rounds"] > 0),
    # (the early entry itself -- a round of 2049 .. BCE_DEC_HOST_ENTER nodes with 512 x as many still to come, and at most n -- needs
    #  inputs of tens of MB: test_decoder_paths_of_round_three_agree.  Here: no early entry, and the tail reaches the host after the probe)
    "host-enter-0": (lambda m: not m["host_early"], lambda b, m: m["host_tail"]),
    "host-enter-200k": (lambda m: m["rounds"] > 0, lambda b, m: m["host_tail"]),
    "force-host-tail": (lambda m: m["probe_rounds"] == 0 and m["host_tail"], lambda b, m: b["probe_rounds"] > 0),
    "no-host-tail": (lambda m: not m["host_tail"] and not m["host_on"], lambda b, m: b["host_tail"]),
    "tail-serial": (lambda m: not m["ccx"] and set(m["host_on"]) <= {"one thread"}, lambda b, m: m["host_tail"]),
    "no-early-pin": (lambda m: not m["early_pin"], lambda b, m: b["early_pin"]),
    "no-probe": (lambda m: m["probe_rounds"] == 0, lambda b, m: b["probe_rounds"] > 0),
    "no-huge": (lambda m: True, lambda b, m: m["host_tail"]),          # (reg_maps: in test_routes_* below, against a control)
    "tail-nopin": (lambda m: m["ncpu"] == 0 and not m["ccx"] and set(m["host_on"]) <= {"eight threads, not pinned"}, lambda b, m: b["ccx"]),
    "give-back": (lambda m: m["given_back"], lambda b, m: not b["given_back"]),
}
assert set(RULES) == set(ROUTES)

# (family, mode) pairs that cannot reach what a route changes, and why.  Anything else must reach it.
_SHORT_TAIL = {"text", "rand", "low-planes", "periodic", "cfg-random", "cfg-0", "cfg-5"}   # no tail long enough for the host
NOT_REACHED = {
    # every round of these fits the one-launch kernel (<= DS_MAXNODES nodes, twice that in every list): no six-launch round to switch off
    "no-split": {(f, "none") for f in FAMILIES if f not in ("rand", "low-planes")},
    "host-enter-0": {(f, m) for f in _SHORT_TAIL for m in MODES},
    "host-enter-200k": {(f, m) for f in _SHORT_TAIL for m in MODES},
    "no-host-tail": {(f, m) for f in _SHORT_TAIL for m in MODES},
    # without eight CPUs of one L3 domain a tail goes to the host only after a long chain, which many-copies' are not
    "tail-serial": {(f, m) for f in _SHORT_TAIL | {"many-copies"} for m in MODES},
    "no-huge": {(f, m) for f in _SHORT_TAIL for m in MODES},
    # the boundary ranks are pinned beside the rounds only where a long tail shows half-way through: the zero run
    "no-early-pin": {(f, m) for f in FAMILIES if f != "zero-run" for m in MODES},
}
_NEEDS_CCX = {"tail-nopin"}                      # what the route switches off is only there with eight CPUs of one L3 domain


def _route_case(family, route, mode, capfd, monkeypatch):
    _, b = _baseline(family, mode, capfd)
    if route in _NEEDS_CCX and not b["ccx"]:
        pytest.skip("needs eight CPUs of one L3 domain in the affinity mask (tail_cpus()); this machine offers %d" % b["ncpu"])
    d, m = _baseline(family, mode, capfd) if route == "default" else _run(family, route, mode, capfd, monkeypatch)
    holds, reaches = RULES[route]
    assert holds(m), (route, m)
    if (family, mode) in NOT_REACHED.get(route, ()):
        return
    assert reaches(b, m), ("%s does not reach what %s changes" % (family, route), b, m)
    if route == "no-huge":
        # the boundary ranks' pinned copy is an ordinary hipHostMalloc now; with the registered mapping allowed, it is one
        assert d["reg_maps"] == 0, d
        monkeypatch.delenv("BCE_DEC_NO_HUGE")
        d2, m2 = _decode(family, MODES[mode], capfd)
        assert m2["host_tail"] and d2["reg_maps"] >= 1, (d2, m2)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("family", WIDE)
def test_routes_under_memory_modes(family, route, mode, capfd, monkeypatch):
    """Text and random bytes: every route under every memory mode."""
    _route_case(family, route, mode, capfd, monkeypatch)


# (zero-run x no-tail: its 1.6 M chain rounds one by one take a minute -- the tail kernels and the host exist for them; the
#  ten other families run no-tail)
_ROUTE_CASES = [(f, r) for f in OTHERS for r in ROUTES if (f, r) != ("zero-run", "no-tail")]


@pytest.mark.parametrize("family,route", _ROUTE_CASES, ids=["%s-%s" % c for c in _ROUTE_CASES])
def test_routes(family, route, capfd, monkeypatch):
    """Every other family on every route (no memory mode)."""
    _route_case(family, route, "none", capfd, monkeypatch)


# (many-copies x grow: its widest rounds fit lists of 4096 nodes -- seven hundred copies of one block share their contexts)
_MODE_CASES = [(f, m) for f in OTHERS for m in MODES if m != "none" and not (f == "many-copies" and 12 in MODES[m])]


@pytest.mark.parametrize("family,mode", _MODE_CASES, ids=["%s-%s" % c for c in _MODE_CASES])
def test_memory_modes(family, mode, capfd, monkeypatch):
    """Every other family under every memory mode, on the default route (the modes' evidence: _run)."""
    _run(family, "default", mode, capfd, monkeypatch)


def test_one_context_hands_its_buffers_from_decode_to_decode(capfd, monkeypatch):
    """One context for a sequence: grown lists (knob 12, with plane groups), then lists given back after the rounds, a small
    archive after the grown one, an encode after a decode that grew its lists (the oracle's archive), and the first archive again
    on the lists the context holds by then."""
    monkeypatch.setenv("BCE_ALLOC_TRACE", "1")
    ctx = bce_amd.api._Ctx(0)
    try:
        def dec(family, expect_grows, given_back=False):
            data, arch = _case(family)
            s0 = bce_amd.stats_of(ctx)
            capfd.readouterr()
            assert bce_amd.decompress_device(arch, ctx=ctx) == data, family
            err = capfd.readouterr().err
            s1 = bce_amd.stats_of(ctx)
            assert s1["dec_restarts"] == s0["dec_restarts"]
            assert (s1["dec_list_grows"] > s0["dec_list_grows"]) == expect_grows, (family, s0, s1)
            assert ("node lists and query buffers given back" in err) == given_back, err[-2000:]
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 12, 1 << 30), "bce_hip_debug_set")
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 13, 4096), "bce_hip_debug_set")
        dec("text", True)
        dec("rand", True)
        monkeypatch.setenv("BCE_DEC_GIVE_BACK", "1")
        dec("text", True, given_back=True)
        monkeypatch.delenv("BCE_DEC_GIVE_BACK")
        dec("query-tail", True)
        dec("rand", True)
        data, _ = _case("cfg-5")
        assert bce_amd.compress(data, config=bytes([5]) * 288, ctx=ctx) == _case("cfg-5")[1]
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 12, 0), "bce_hip_debug_set")
        ctx.check(ctx.lib.bce_hip_debug_set(ctx.h, 13, 0), "bce_hip_debug_set")
        dec("text", False)
        dec("zero-run", False)
    finally:
        ctx.close()
