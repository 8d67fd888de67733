"""CPU: the rules the parse and patch kernels share with the host (bce_amd/csrc/parse_step.h) compiled by g++ into a stand-alone
program under ASan + UBSan and driven through the kernels' block decomposition with blocks of 4 and 8 positions
(tests/parse_emul.cpp), against the chain walked one position at a time in Python (tests/parse_ref.py): structure, literal bytes,
info, every copy by content, the round trip; that the parse with min_len 1 has the fewest phrases (a dynamic programme); the patch
validator on every malformed kind; the delta file's reader; the new symbols, structures and names."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bce_amd
from bce_amd import api, container
from conftest import ROOT

import match_ref
import parse_ref as ref
from test_count_cpu import _texts
from test_match_cpu import _queries_for

SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
MIN_LENS = (1, 3, 8)
NONE = 0xFFFFFFFF


def _bounds(m):
    return sorted({L for L in (m, 7, 4096) if L >= m})


def _build_emul():
    exe = os.path.join(ROOT, "tests", "_build", "parse_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "parse_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def _words(v):
    return ",".join(str(int(x)) for x in v) or "-"


def _positions(text, query, lens):
    return [text.find(query[i - l + 1:i + 1]) if l else NONE for i, l in enumerate(np.asarray(lens).tolist())]


def _run(emul, tmp_path, lines):
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _parsed(line):
    w = line.split(" ")
    assert w[0] == "parse" and len(w) == 8, line
    ops = np.array([] if w[1] == "-" else [[int(x) for x in p.split(":")] for p in w[1].split(",")], dtype=np.uint32).reshape(-1, 2)
    lits = b"" if w[2] == "-" else bytes.fromhex(w[2])
    info = dict(zip(("nops", "nlits", "ncopies", "copied"), map(int, w[3:7])))
    return ops, lits, info, (b"" if w[7] == "-" else bytes.fromhex(w[7]))


def test_blocks_of_4_and_8_give_the_chain_of_the_reference(tmp_path):
    emul = _build_emul()
    texts, rs = _texts()
    assert len(texts) == 57
    cases, lines = [], []
    for t in texts:
        for q in _queries_for(t, rs):
            lens = {L: match_ref.match_lens(t, q, L) for L in sorted({L for m in MIN_LENS for L in _bounds(m)})}
            for m in MIN_LENS:
                for L in _bounds(m):
                    pos = _positions(t, q, lens[L])
                    for B in (4, 8):
                        cases.append((t, q, m, lens[L]))
                        lines.append("parse %d %d %s %s %s %s" % (B, m, _hex(t), _words(lens[L]), _words(pos), _hex(q)))
    assert len(cases) > 3000
    crossing = 0
    for (t, q, m, lens), line in zip(cases, _run(emul, tmp_path, lines)):
        ops, lits, info, back = _parsed(line)
        want = ref.parse_of_lengths(lens, q, m)
        ref.check(t, q, want, ops, lits, info)
        assert back == q                                                   # the emulator's patch of its own parse
        assert info["nlits"] + info["copied"] == len(q) and info["nops"] - info["ncopies"] == sum(1 for p in want[0] if not p[2])
        crossing += any(ln > 8 for _s, ln, _c in want[0])
    assert crossing > 200                                                  # phrases longer than a block: runs and jumps cross blocks
    # what the cases cover
    ph, lits, info = ref.parse(b"abracadabra", b"xabracxx", 3, 4096)
    assert ph == [(0, 1, False), (1, 5, True), (6, 2, False)] and lits == b"xxx" and info == {"nops": 3, "nlits": 3, "ncopies": 1, "copied": 5}
    assert ref.parse(b"abracadabra", b"raab", 1, 4096)[0] == [(0, 2, True), (2, 2, True)]          # linear: no copy across the end
    assert ref.parse(b"ab", b"", 1, 1) == ([], b"", {"nops": 0, "nlits": 0, "ncopies": 0, "copied": 0})


def test_min_len_1_has_the_fewest_phrases(tmp_path):
    """Against a dynamic programme over all parses into substrings of the text of at most max_len bytes and single literal
    bytes, every literal byte counted as a phrase: 400 random small texts and queries, five bounds, through the emulator."""
    emul = _build_emul()
    rs = np.random.RandomState(20240607)
    cases, lines = [], []
    for k in range(400):
        sigma = 2 + k % 3
        t = bytes(rs.randint(97, 97 + sigma, size=rs.randint(1, 24)).astype(np.uint8))
        q = bytes(rs.randint(97, 97 + sigma + (k % 2), size=rs.randint(1, 30)).astype(np.uint8))
        for L in (1, 2, 3, 5, 4096):
            lens = match_ref.match_lens(t, q, L)
            cases.append((t, q, L))
            lines.append("parse %d 1 %s %s %s %s" % (4 + 4 * (k % 2), _hex(t), _words(lens), _words(_positions(t, q, lens)), _hex(q)))
    for (t, q, L), line in zip(cases, _run(emul, tmp_path, lines)):
        ops, lits, info, back = _parsed(line)
        assert back == q
        assert info["ncopies"] + info["nlits"] == ref.fewest_phrases(t, q, L), (t, q, L)
    assert ref.fewest_phrases(b"abc", b"abcab", 4096) == 2 and ref.fewest_phrases(b"abc", b"abcab", 2) == 3 and ref.fewest_phrases(b"a", b"bb", 9) == 2


LIT = NONE
MALFORMED = [                                                              # (ops, claimed nlits, literal bytes, words of the refusal)
    ([(3, 0), (0, 2)], 0, b"", "an op of length 0"),
    ([(0, LIT)], 0, b"", "an op of length 0"),
    ([(4, 8)], 0, b"", "past the end of the text"),                       # abracadabra: 8 + 4 > 11
    ([(1, 11)], 0, b"", "past the end of the text"),                      # src = n
    ([(0x7FFFFFFF, 1)], 0, b"", "past the end of the text"),
    ([(2, LIT), (3, 0)], 1, b"x", "do not add up"),                       # literal sum long
    ([(2, LIT), (3, 0)], 3, b"xyz", "do not add up"),                     # literal sum short
    ([(3, 0)], 1, b"x", "do not add up"),
    ([(0x7FFFFFFF, LIT), (1, LIT)], 0x80000000, b"", "2^31 bytes or more"),       # by the lengths alone
    ([(0x7FFFFFFF, LIT), (0x7FFFFFFF, LIT), (2, LIT)], 0x100000000, b"", "2^31 bytes or more"),
]


def test_patch_validator_and_copy(tmp_path):
    emul = _build_emul()
    text = b"abracadabra"
    lines = ["patch %d %d %s %s %s" % (B, nl, _hex(text), ",".join("%d:%d" % o for o in ops), _hex(lits)) for ops, nl, lits, _ in MALFORMED for B in (4, 8)]
    good = [([(11, 0)], b""), ([(5, LIT)], b"hello"), ([(1, 10), (2, LIT), (4, 7), (1, LIT), (11, 0), (3, 8)], b"xyz"),
            ([(1, i % 11) if i % 2 else (1, LIT) for i in range(41)], b"Q" * 21), ([(3, 4)] * 30, b"")]
    lines += ["patch %d %d %s %s %s" % (B, len(lits), _hex(text), ",".join("%d:%d" % o for o in ops), _hex(lits)) for ops, lits in good for B in (4, 8)]
    lines.append("patch 4 0 %s - -" % _hex(text))
    out = _run(emul, tmp_path, lines)
    k = 0
    for _ops, _nl, _lits, why in MALFORMED:
        for _B in (4, 8):
            assert out[k].startswith("patch bad patch: ") and why in out[k], (out[k], why)
            k += 1
    for ops, lits in good:
        for _B in (4, 8):
            assert out[k] == "patch ok " + _hex(ref.apply(text, ops, lits)), (ops, out[k])
            k += 1
    assert out[k] == "patch ok -"


def test_emulator_refuses_malformed_input(tmp_path):
    emul = _build_emul()
    for text in ("parse 5 1 61 1 0 61\n", "parse 4 1 61 2 0 61\n", "parse 4 1 61 1,1 0 61\n", "patch 4 0 61 1:0:2 -\n", "what 4 1 61 1 0 61\n", "parse 4 0 61 1 0 61\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


# ---- the delta file ---------------------------------------------------------------------------------------------------------------

def test_delta_file_reader_judges_before_any_device():
    ops = np.array([(3, LIT), (5, 2)], dtype=api.OP_DTYPE)
    blob = container.pack_delta(11, 0x12345678, 8, 0x9ABCDEF0, 3, 256, ops, np.frombuffer(b"xyz", dtype=np.uint8))
    assert len(blob) == 56 + 16 + 3 and blob[:4] == b"BCED"
    d = container.unpack_delta(blob)
    assert (d["n"], d["base_crc"], d["q"], d["crc"], d["min_len"], d["max_len"]) == (11, 0x12345678, 8, 0x9ABCDEF0, 3, 256)
    assert d["ops"].tolist() == [[3, LIT], [5, 2]] and d["lits"].tobytes() == b"xyz"
    assert container.pack_delta(11, 0x12345678, 8, 0x9ABCDEF0, 3, 256, d["ops"], d["lits"]) == blob          # pairs as well as records
    head = struct.Struct("<4sIQIQIIIQQ")
    fields = list(head.unpack_from(blob))

    def with_field(i, v, tail=blob[56:]):
        f = list(fields)
        f[i] = v
        return head.pack(*f) + tail

    bad = [blob[:k] for k in (0, 3, 4, 55, 56, 60, len(blob) - 1)] + [blob + b"\0", b"BCEM" + blob[4:], with_field(1, 2), with_field(1, 0),
           with_field(8, 3), with_field(8, 1), with_field(9, 2), with_field(9, 4), with_field(8, 1 << 61), with_field(8, (1 << 61) + 2),
           with_field(9, (1 << 64) - 13), with_field(8, (1 << 64) - 1), with_field(4, 1 << 31), with_field(2, 1 << 31), with_field(4, 1 << 63)]
    for b in bad:
        with pytest.raises(ValueError):
            container.unpack_delta(b)
    empty = container.pack_delta(5, 1, 0, 0, 16, 256, np.zeros(0, dtype=api.OP_DTYPE), b"")
    assert len(empty) == 56 and container.unpack_delta(empty)["ops"].shape == (0, 2)


# ---- ABI, names -------------------------------------------------------------------------------------------------------------------

NEW = {"bce_hip_parse": 10, "bce_hip_parse_device": 10, "bce_hip_patch": 8, "bce_hip_patch_device": 8, "bce_hip_parse_of_lengths_device": 11}


def _struct_fields(src, name):
    body = src[src.index("typedef struct %s {" % name):src.index("} %s;" % name)]
    want = []
    for ctype, names in re.findall(r"\b(uint64_t|uint32_t)\s+([^;]+);", body):
        want += [(nm.strip(), {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}[ctype]) for nm in names.split(",")]
    return want


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert src.index("bce_hip_longest_repeat(") < src.index("bce_hip_parse(") < src.index("bce_hip_sort_pairs_device(")   # a section of its own after the LCP's
    assert re.search(r"#define\s+BCE_HIP_OP_LITERAL\s+0xFFFFFFFFu", src) and api.OP_LITERAL == 0xFFFFFFFF
    assert _struct_fields(src, "bce_hip_op") == list(api.Op._fields_) and C.sizeof(api.Op) == 8 and api.OP_DTYPE.itemsize == 8
    assert api.OP_DTYPE.names == ("len", "src")
    assert _struct_fields(src, "bce_hip_parse_info") == list(api.ParseInfo._fields_) and C.sizeof(api.ParseInfo) == 32
    for name in ("parse", "patch", "delta", "apply_delta", "parse_tensor", "patch_tensor", "ParseInfo"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("parse", "parse_device", "patch", "patch_device"):
        assert callable(getattr(bce_amd.RankFile, name)), name
    assert callable(container.pack_delta) and callable(container.unpack_delta)
    import inspect
    assert inspect.signature(bce_amd.RankFile.parse).parameters["max_len"].default == 256
    assert inspect.signature(bce_amd.delta).parameters["max_len"].default == 256 and inspect.signature(bce_amd.delta).parameters["min_len"].default == 16


def test_null_context_and_refused_arguments_leave_the_outputs_untouched():
    lib = bce_amd.load_library()
    qry = (C.c_uint8 * 4)(97, 98, 99, 100)
    ops, lits, out = (C.c_uint32 * 8)(*([7] * 8)), (C.c_uint8 * 4)(9, 9, 9, 9), (C.c_uint8 * 4)(5, 5, 5, 5)
    info, total = api.ParseInfo(1, 2, 3, 4), C.c_uint64(77)
    for fn in (lib.bce_hip_parse, lib.bce_hip_parse_device):
        assert fn(None, C.addressof(qry), 4, 1, 16, C.addressof(ops), 4, C.addressof(lits), 4, C.byref(info)) == -1
        assert fn(None, None, 0, 1, 16, None, 0, None, 0, C.byref(info)) == -1
    assert lib.bce_hip_parse_of_lengths_device(None, None, None, None, 0, 1, None, 0, None, 0, C.byref(info)) == -1
    for fn in (lib.bce_hip_patch, lib.bce_hip_patch_device):
        assert fn(None, C.addressof(ops), 4, C.addressof(lits), 4, C.addressof(out), 4, C.byref(total)) == -1
        assert fn(None, None, 0, None, 0, None, 0, C.byref(total)) == -1
    assert list(ops) == [7] * 8 and list(lits) == [9] * 4 and list(out) == [5] * 4 and total.value == 77
    assert (info.nops, info.nlits, info.ncopies, info.copied) == (1, 2, 3, 4)


# ---- the command line without a device ----------------------------------------------------------------------------------------------

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")


def test_usage_has_the_four_delta_paragraphs_after_the_kgram_ones():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    at = lines.index("  bce -gkd K archive.bce")
    heads = ["  bce -gr MINLEN file query_file out.bcd", "  bce -grd MINLEN archive.bce query_file out.bcd", "  bce -ga file in.bcd out_file",
             "  bce -gad archive.bce in.bcd out_file"]
    for k, head in enumerate(heads):
        assert lines[at + 2 + 3 * k] == "" and lines[at + 3 + 3 * k] == head and lines[at + 4 + 3 * k].startswith("   ")
    for args in (["-gr"], ["-gr", "16", "f", "q"], ["-gr", "16", "f", "q", "o", "x"], ["-gr", "0", "f", "q", "o"], ["-gr", "4097", "f", "q", "o"],
                 ["-gr", "16x", "f", "q", "o"], ["-gr", "", "f", "q", "o"], ["-grx", "16", "f", "q", "o"], ["-grd", "16", "a", "q"],
                 ["-ga"], ["-ga", "f", "d"], ["-ga", "f", "d", "o", "x"], ["-gax", "f", "d", "o"], ["-gadx", "a", "d", "o"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_delta_without_a_device_answers_as_the_match_does(tmp_path):
    """The CLI as tests/test_match_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the parse's and
    the patch's entry points are weak references and stay unresolved.  The files are read and judged before the device is missed: the
    base and the query with -gm's words and exit codes, a malformed delta file as -d answers a malformed archive."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_parse")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f, qf, empty, missing = tmp_path / "in.txt", tmp_path / "query.txt", tmp_path / "empty", tmp_path / "missing"
    f.write_bytes(b"abracadabra" * 100)
    qf.write_bytes(b"cadabra abra")
    empty.write_bytes(b"")
    good = tmp_path / "good.bcd"
    good.write_bytes(container.pack_delta(1100, 1, 12, 2, 4, 256, np.array([[7, 4], [5, LIT]], dtype=np.uint32), b" abra"))
    blob = good.read_bytes()
    head = struct.Struct("<4sIQIQIIIQQ")
    fields = list(head.unpack_from(blob))
    bads = [blob[:-1], blob + b"x", blob[:55], blob[:3], b"BCEM" + blob[4:], head.pack(*(fields[:1] + [2] + fields[2:])) + blob[56:],
            head.pack(*(fields[:8] + [1 << 61] + fields[9:])) + blob[56:], head.pack(*(fields[:9] + [(1 << 64) - 11])) + blob[56:],
            head.pack(*(fields[:4] + [1 << 31] + fields[5:])) + blob[56:]]
    before = sorted(os.listdir(tmp_path))

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, cwd=tmp_path)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
        return r

    out = tmp_path / "out"
    for dflag in ("", "d"):
        for file in (missing, empty, f):                                 # the base: -gm's answer, for both commands
            a = run("-gm" + dflag, 4, file, qf)
            for b in (run("-gr" + dflag, 4, file, qf, out), run("-ga" + dflag, file, good, out)):
                assert a.returncode == b.returncode != 0 and a.stdout == b.stdout, (file, dflag, b.stdout)
        for query in (missing, empty):                                   # the query of -gr is a plain file: -gm's words
            a, b = run("-gm" + dflag, 4, f, query), run("-gr" + dflag, 4, f, query, out)
            assert a.returncode == b.returncode == 255 and a.stdout == b.stdout and "Error loading file" in b.stdout
        r = run("-ga" + dflag, f, missing, out)
        assert r.returncode == 255 and "Archive not found." in r.stdout
        for k, bad in enumerate([b""] + bads):                           # a malformed delta: refused before the device is missed
            (tmp_path / "bad.bcd").write_bytes(bad)
            r = run("-ga" + dflag, f, tmp_path / "bad.bcd", out)
            assert r.returncode == 254 and "Could not read Archive." in r.stdout and "HIP device" not in r.stdout, (k, r.stdout)
        os.remove(tmp_path / "bad.bcd")
    for r in (run("-gr", 4, f, qf, out), run("-ga", f, good, out)):
        assert r.returncode == 253 and "No usable HIP device" in r.stdout
    assert sorted(os.listdir(tmp_path)) == before
