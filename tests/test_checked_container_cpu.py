"""CPU: the checked container (BCEM version 2) and its CRC-32: the host routines against zlib, the container's Python side, the
CLI's `-ds` on good, lying and damaged version-2 containers (also under ASan + UBSan), the new symbols, usage text and the answer
`bce -t archive` gives without a GPU."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bce_amd
import oracle
from bce_amd import api, container
from conftest import ROOT

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
E_ARG = -1
MISMATCH = re.compile(r"Checksum mismatch in block (\d+): table ([0-9A-F]{8}), decoded ([0-9A-F]{8})")


# ---- the checksum, host side ------------------------------------------------------------------------------------------------

def test_crc32_is_zlibs_for_every_length_and_start_offset():
    buf = np.random.RandomState(3).randint(0, 256, 70000).astype(np.uint8).tobytes()
    lengths = list(range(0, 301)) + [4095, 4096, 4097, 65535, 65536, 65537]
    for off in range(16):
        for n in lengths:
            assert api.crc32(buf[off:off + n]) == zlib.crc32(buf[off:off + n]), (off, n)
    # the same through the C entry point on one buffer, so that the pointer itself has every alignment
    lib = bce_amd.load_library()
    arr = np.frombuffer(buf, dtype=np.uint8)
    for off in range(16):
        for n in (0, 1, 7, 8, 9, 63, 300, 4097):
            assert lib.bce_hip_crc32(0, arr.ctypes.data + off, n) == zlib.crc32(buf[off:off + n]), (off, n)


def test_crc32_chained_calls_equal_one_call():
    buf = oracle.synth_text(5, 100000)
    want = zlib.crc32(buf)
    for cuts in ([0], [1], [7, 8, 9], [4096], [33333, 66666], list(range(0, 100000, 9973))):
        crc, prev = 0, 0
        for c in cuts + [len(buf)]:
            crc = api.crc32(buf[prev:c], crc)
            prev = c
        assert crc == want, cuts
    assert api.crc32(b"") == 0 and api.crc32(b"", 0x1234) == 0x1234


def test_crc32_combine_is_the_crc_of_the_concatenation():
    buf = np.random.RandomState(4).randint(0, 256, 50000).astype(np.uint8).tobytes()
    for cut in (0, 1, 2, 15, 16, 17, 4095, 4096, 12345, 49999, 50000):
        a, b = buf[:cut], buf[cut:]
        assert api.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(buf), cut
    # len_b = 0: B is empty, its CRC is 0, A's comes back
    assert api.crc32_combine(0xDEADBEEF, 0, 0) == 0xDEADBEEF
    # lengths of 2^32 and more need only the number: B = zeros, whose CRC zlib gives piece by piece
    piece = bytes(1 << 24)
    for len_b in (1 << 32, (1 << 32) + 5):
        crc_b = 0
        whole = zlib.crc32(b"head of the file")
        left = len_b
        while left:
            m = min(left, len(piece))
            crc_b = zlib.crc32(piece[:m], crc_b)
            whole = zlib.crc32(piece[:m], whole)
            left -= m
        assert api.crc32_combine(zlib.crc32(b"head of the file"), crc_b, len_b) == whole, len_b


# ---- the container, Python side ---------------------------------------------------------------------------------------------

def test_pack_blocks_without_crcs_is_version_1_byte_for_byte():
    blob = container.pack_blocks([b"abc", b"de"], [10, 20])
    assert blob == (b"BCEM\x01\x00\x00\x00\x02\x00\x00\x00"
                    b"\x0a\x00\x00\x00\x00\x00\x00\x00\x03\x00\x00\x00\x00\x00\x00\x00"
                    b"\x14\x00\x00\x00\x00\x00\x00\x00\x02\x00\x00\x00\x00\x00\x00\x00"
                    b"abcde")
    assert container.pack_blocks([b"abc", b"de"], [10, 20], crcs=None) == blob
    assert container.block_table(blob) == [(10, 44, 3, None), (20, 47, 2, None)]


def test_version_2_round_trips_through_block_table_and_unpack_blocks():
    archives, raws, crcs = [b"abc", b"", b"defgh"], [10, 2**40, 7], [0x11223344, 0, 0xFFFFFFFF]
    blob = container.pack_blocks(archives, raws, crcs)
    assert blob[:12] == b"BCEM\x02\x00\x00\x00\x03\x00\x00\x00"
    assert blob[12:36] == struct.pack("<QQII", 10, 3, 0x11223344, 0)
    assert len(blob) == 12 + 3 * 24 + 8
    assert container.unpack_blocks(blob) == (archives, raws)
    table = container.block_table(blob)
    assert [(t[0], t[2], t[3]) for t in table] == [(10, 3, 0x11223344), (2**40, 0, 0), (7, 5, 0xFFFFFFFF)]
    assert [blob[t[1]:t[1] + t[2]] for t in table] == archives
    with pytest.raises(ValueError):
        container.pack_blocks(archives, raws, crcs[:2])


def test_hostile_version_2_tables_are_refused():
    good = container.pack_blocks([b"abc", b"de"], [10, 20], [1, 2])
    container.block_table(good)
    bad = []
    for alen in (2**64 - 1, 2**64 - 3, len(good), 2**40):          # an archive size that wraps or lies beyond the blob
        b = bytearray(good)
        b[12 + 8:12 + 16] = struct.pack("<Q", alen)
        bad.append(bytes(b))
    b = bytearray(good)
    b[8:12] = struct.pack("<I", 1000)                               # a table beyond the blob
    bad.append(bytes(b))
    bad.append(good[:30])
    for word in (1, 0x80000000):                                     # a reserved word that is not 0
        b = bytearray(good)
        b[12 + 24 + 20:12 + 24 + 24] = struct.pack("<I", word)
        bad.append(bytes(b))
    bad.append(good + b"x")                                          # trailing bytes
    bad.append(good[:-1])
    b = bytearray(good)
    b[4:8] = struct.pack("<I", 3)                                    # a version nobody wrote
    bad.append(bytes(b))
    for blob in bad:
        with pytest.raises(ValueError):
            container.block_table(blob)
        with pytest.raises(ValueError):
            container.unpack_blocks(blob)


# ---- `bce -ds` on version-2 containers --------------------------------------------------------------------------------------

def _parts():
    return [oracle.synth_text(41, 4000), oracle.synth_text(42, 300), b"a" * 50]


def _damaged_block(archive, text):
    """`archive` with one byte of its coded stream altered so that it still decodes -- to other bytes of the same length."""
    rs = np.random.RandomState(7)
    for _ in range(200):                                             # (bounded: nearly every flip near the end still decodes)
        b = bytearray(archive)
        b[len(b) - 1 - int(rs.randint(0, len(b) // 4))] ^= 1 << int(rs.randint(8))
        try:
            got = bce_amd.decompress(bytes(b))
        except bce_amd.BceError:
            continue
        if len(got) == len(text) and got != text:
            return bytes(b), got
    return None, None


@pytest.fixture(scope="module")
def containers(tmp_path_factory):
    """good / a lying CRC in block 1 / a damaged stream in block 0, as files: name -> (path, bad block or None, decoded CRC)."""
    d = tmp_path_factory.mktemp("v2")
    parts = _parts()
    archives = [oracle.compress(p) for p in parts]
    crcs = [zlib.crc32(p) for p in parts]
    sizes = [len(p) for p in parts]
    out = {}
    (d / "good.bcem").write_bytes(container.pack_blocks(archives, sizes, crcs))
    out["good"] = (d / "good.bcem", None, None)
    (d / "crc.bcem").write_bytes(container.pack_blocks(archives, sizes, [crcs[0], crcs[1] ^ 0x00100000, crcs[2]]))
    out["crc"] = (d / "crc.bcem", 1, crcs[1])
    damaged, got = _damaged_block(archives[0], parts[0])
    assert damaged is not None, "no single-byte damage of block 0 found that still decodes"
    (d / "stream.bcem").write_bytes(container.pack_blocks([damaged] + archives[1:], sizes, crcs))
    out["stream"] = (d / "stream.bcem", 0, zlib.crc32(got))
    return out


def _check_ds(exe, containers, tmp_path, env=None):
    out = tmp_path / "o"
    parts = _parts()
    for name, (path, bad_block, decoded_crc) in containers.items():
        out.unlink(missing_ok=True)
        r = subprocess.run([exe, "-ds", str(out), str(path)], capture_output=True, text=True, env=env)
        assert r.returncode not in (98, 99) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        if bad_block is None:
            assert r.returncode == 0, (name, r.returncode, r.stdout)
            assert out.read_bytes() == b"".join(parts)
            continue
        m = MISMATCH.search(r.stdout)
        assert m, (name, r.stdout)
        table_crc = container.block_table(path.read_bytes())[bad_block][3]
        assert (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16)) == (bad_block, table_crc, decoded_crc), (name, r.stdout)
        assert r.returncode == 252 and not out.exists(), (name, r.returncode)       # (-4: a failed decode's status)


def test_cli_ds_checks_every_block_of_a_version_2_container(containers, tmp_path):
    _check_ds(EXE, containers, tmp_path)
    # the one-block checked container takes the same road
    data = oracle.synth_text(43, 2000)
    arc, out = tmp_path / "one.bcem", tmp_path / "one.out"
    arc.write_bytes(container.pack_blocks([oracle.compress(data)], [len(data)], [zlib.crc32(data)]))
    r = subprocess.run([EXE, "-ds", str(out), str(arc)], capture_output=True, text=True)
    assert r.returncode == 0 and out.read_bytes() == data
    arc.write_bytes(container.pack_blocks([oracle.compress(data)], [len(data)], [zlib.crc32(data) ^ 1]))
    out.unlink()
    r = subprocess.run([EXE, "-ds", str(out), str(arc)], capture_output=True, text=True)
    assert r.returncode == 252 and MISMATCH.search(r.stdout).group(1) == "0" and not out.exists()


def test_cli_ds_refuses_hostile_version_2_tables(tmp_path):
    parts = _parts()[:2]
    archives = [oracle.compress(p) for p in parts]
    crcs = [zlib.crc32(p) for p in parts]
    out, bad = tmp_path / "o", tmp_path / "bad.bcem"
    blobs = [container.pack_blocks(archives, t, crcs) for t in
             ([2**64 - 100, 300], [4000, 2**64 - 4000], [2**31, 300], [2**40, 300], [0, 300], [4001, 300], [3999, 300], [4000, 301])]
    good = container.pack_blocks(archives, [len(p) for p in parts], crcs)
    for alen in (2**64 - 1, len(good), 2**40):
        b = bytearray(good)
        b[12 + 8:12 + 16] = struct.pack("<Q", alen)
        blobs.append(bytes(b))
    b = bytearray(good)
    b[12 + 20:12 + 24] = struct.pack("<I", 7)                        # reserved word
    blobs.append(bytes(b))
    b = bytearray(good)
    b[8:12] = struct.pack("<I", 2**31)                               # a table far beyond the file
    blobs.append(bytes(b))
    for blob in blobs:
        out.unlink(missing_ok=True)
        bad.write_bytes(blob)
        r = subprocess.run([EXE, "-ds", str(out), str(bad)], capture_output=True, text=True)
        assert r.returncode == 254 and "Could not read Archive." in r.stdout and not out.exists(), (r.returncode, r.stdout)


@pytest.fixture(scope="module")
def asan_cli_v2():
    """The CLI + host decoder + host coder as a CPU-only binary under AddressSanitizer and UBSan (tests/test_decoder_cpu.py's
    recipe; the GPU entry points this change adds are weak references there and stay unresolved)."""
    out = os.path.join(ROOT, "tests", "_build", "bce_asan_v2")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", out] + src + ["-lpthread"])
    return out


def test_sanitized_ds_on_version_2_containers(asan_cli_v2, containers, tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    _check_ds(asan_cli_v2, containers, tmp_path, env=env)
    # without a device: -d and the self-test say so, cleanly
    path = containers["good"][0]
    for args in (["-d", str(tmp_path / "o2"), str(path)], ["-t", str(path)]):
        r = subprocess.run([asan_cli_v2] + args, capture_output=True, text=True, env=env)
        assert r.returncode == 253 and "No usable HIP device" in r.stdout and "Sanitizer" not in r.stderr, (args, r.returncode, r.stdout, r.stderr[-2000:])
    assert not (tmp_path / "o2").exists()


# ---- ABI, usage, the self-test's answer without a GPU -----------------------------------------------------------------------

NEW = {"bce_hip_crc32": (C.c_uint32, 3), "bce_hip_crc32_combine": (C.c_uint32, 3), "bce_hip_crc32_device": (C.c_int, 4),
       "bce_hip_input_crc32": (C.c_int, 2), "bce_hip_decode_crc32": (C.c_int, 5), "bce_hip_decompress_device_crc32": (C.c_int, 7)}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = open(os.path.join(ROOT, "include", "bce_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, (res, nargs) in NEW.items():
        assert hasattr(lib, name), name
        assert re.search(r"\b(int|uint32_t)\s+%s\s*\(" % name, src), name
        assert name in bound and bound[name][0] is res and len(bound[name][1]) == nargs, name
    for name in ("crc32", "crc32_combine", "crc32_device", "decode_crc32", "ChecksumError", "compress_tensor_blocks",
                 "decompress_container_tensor", "test_container"):
        assert callable(getattr(bce_amd, name)), name
    assert issubclass(bce_amd.ChecksumError, bce_amd.BceError)
    e = bce_amd.ChecksumError(3, 0x12345678, 0x9ABCDEF0)
    assert (e.block, e.expected, e.actual) == (3, 0x12345678, 0x9ABCDEF0) and "block 3" in str(e)


def test_null_arguments_to_the_gpu_entry_points_are_refused_before_any_device_call():
    lib = bce_amd.load_library()
    buf = (C.c_uint8 * 16)()
    crc, n = C.c_uint32(77), C.c_size_t(5)
    a = C.addressof(buf)
    assert lib.bce_hip_crc32_device(None, a, 16, C.byref(crc)) == E_ARG
    assert lib.bce_hip_crc32_device(None, None, 0, C.byref(crc)) == E_ARG
    assert lib.bce_hip_input_crc32(None, C.byref(crc)) == E_ARG
    assert lib.bce_hip_decode_crc32(None, a, 16, C.byref(n), C.byref(crc)) == E_ARG
    assert lib.bce_hip_decode_crc32(None, None, 0, C.byref(n), C.byref(crc)) == E_ARG
    assert lib.bce_hip_decompress_device_crc32(None, a, 16, None, 0, C.byref(n), C.byref(crc)) == E_ARG
    assert crc.value == 77 and n.value == 5                         # nothing reported
    # (a null crc in a live context: tests/test_gpu_crc32.py -- a context needs a device)


def test_usage_has_the_two_new_paragraphs_after_the_existing_ones():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    out = r.stdout
    assert "  bce -CN archive.bcem file [config.bcc]\n   As -cN with N = 1..64" in out
    assert "  bce -t archive.bcem\n   Tests a -CN archive against its own checksums" in out
    assert "exit status 0 = sound, 1 = a block differs, 2 = the archive carries no checksum" in out
    assert out.index("  bce -cN archive.bcem file [config.bcc]") < out.index("  bce -CN archive.bcem file") < out.index("  bce -t archive.bcem\n")
    # -C without a block count of 1..64 is no command
    for flag in ("-C", "-C0", "-C65"):
        r = subprocess.run([EXE, flag, "a", "b"], capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout


def test_self_test_of_an_archive_without_checksums_answers_without_a_gpu(tmp_path):
    data = oracle.synth_text(44, 3000)
    plain, v1 = tmp_path / "a.bce", tmp_path / "a.bcem"
    plain.write_bytes(oracle.compress(data))
    v1.write_bytes(container.pack_blocks([oracle.compress(data[:1000]), oracle.compress(data[1000:])], [1000, 2000]))
    for path in (plain, v1):
        r = subprocess.run([EXE, "-t", str(path)], capture_output=True, text=True)
        assert r.returncode == 2, (r.returncode, r.stdout)
        assert "Archive carries no checksum: test it against the file (bce -t file archive)" in r.stdout
        assert "No usable HIP device" not in r.stdout
    r = subprocess.run([EXE, "-t", str(tmp_path / "missing")], capture_output=True, text=True)
    assert r.returncode == 255 and "Archive not found." in r.stdout
