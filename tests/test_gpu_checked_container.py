"""GPU: the checked container (BCEM version 2) end to end: `bce -CN`, `-d` / `-ds` / `-t archive` on it, good and damaged; the
tensor path -- compress_tensor_blocks, decompress_container_tensor, test_container -- up to an input beyond 2^31 bytes."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest
import torch

import bce_amd
from bce_amd import api, container
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
MISMATCH = re.compile(r"Checksum mismatch in block (\d+): table ([0-9A-F]{8}), decoded ([0-9A-F]{8})")


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def _flip_block(blob, block, text):
    """`blob` with one byte inside `block`'s coded stream flipped so that the block still decodes -- on the host decoder, to other
    bytes of the same length -- or None.  A bounded search: offsets from the block's end backwards.  -> (damaged blob, CRC-32 of
    what the host decoder makes of the block).
    (The GPU-assisted decoder refuses such a block by itself nearly always: measured here, 200 of 200 flips spread over a block of
    10^6 bytes of text -- its inverse BWT insists on ONE cycle through all rows, which a damaged BWT has with probability ~1/n.  So
    for `-d` and `-t archive` the flip must end in a refusal that names the block or the decoder's own; the checksum path itself is
    exercised on the GPU with a block that decodes perfectly to OTHER bytes: _swap_block.)"""
    _raw, pos, alen, _crc = container.block_table(blob)[block]
    for k in range(1, 120):
        b = bytearray(blob)
        b[pos + alen - 1 - 37 * k] ^= 0x10
        try:
            got = bce_amd.decompress(bytes(b[pos:pos + alen]))
        except bce_amd.BceError:
            continue
        if len(got) == len(text) and got != text:
            return bytes(b), zlib.crc32(got)
    return None


def _swap_block(blob, block, other_text):
    """`blob` (version 2) with `block`'s archive replaced by a sound archive of `other_text` (same length, other bytes): the table
    keeps the CRC of the original block, so every decoder decodes the block without complaint -- to bytes the table does not vouch for."""
    archives, raws = container.unpack_blocks(blob)
    assert len(other_text) == raws[block]
    archives[block] = bytes(api.compress(other_text))
    return container.pack_blocks(archives, raws, [t[3] for t in container.block_table(blob)])


def test_cli_checked_container_of_three_blocks(tmp_path):
    data = bce_amd.synth_text(31, 3 * 10**6 + 1).tobytes()
    src, c3, C3, out = tmp_path / "in", tmp_path / "c3.bcem", tmp_path / "C3.bcem", tmp_path / "out"
    src.write_bytes(data)
    assert _bce("-c3", c3, src).returncode == 0
    r = _bce("-C3", C3, src)
    assert r.returncode == 0 and "Compressed from %d B -> %d B in " % (len(data), C3.stat().st_size) in r.stdout, r.stdout + r.stderr
    blob = C3.read_bytes()
    assert container.unpack_blocks(blob) == container.unpack_blocks(c3.read_bytes())       # exactly -c3's archives
    table = container.block_table(blob)
    los = [0, table[0][0], table[0][0] + table[1][0], len(data)]
    assert los[1:3] == [10**6 + 1, 2 * 10**6 + 1]
    assert [t[3] for t in table] == [zlib.crc32(data[los[b]:los[b + 1]]) for b in range(3)]
    for flag in ("-d", "-ds"):
        out.unlink(missing_ok=True)
        r = _bce(flag, out, C3)
        assert r.returncode == 0 and out.read_bytes() == data, (flag, r.stdout + r.stderr)
    out.unlink()
    before = _listing(tmp_path)
    r = _bce("-t", C3)
    assert r.returncode == 0 and "Archive OK: %d B -> %d B in " % (len(blob), len(data)) in r.stdout, r.stdout + r.stderr
    assert _bce("-t", src, C3).returncode == 0                                             # against the file: as before
    assert _listing(tmp_path) == before
    # a version-1 container has nothing to test itself with
    r = _bce("-t", c3)
    assert r.returncode == 2 and "Archive carries no checksum" in r.stdout

    # one byte of block 1's coded stream flipped, so that the block still decodes (host decoder: see _flip_block)
    text1 = data[los[1]:los[2]]
    found = _flip_block(blob, 1, text1)
    assert found is not None, "no flip inside block 1 found that still decodes"
    bad_blob, host_crc = found
    bad = tmp_path / "bad.bcem"
    bad.write_bytes(bad_blob)
    before = _listing(tmp_path)

    def refused(args, statuses, crc):
        """no output, nothing written; block 1 named with (table, decoded) = (the table's, crc) -- or, crc None, the GPU decoder's own refusal"""
        r = _bce(*args)
        assert "Archive OK" not in r.stdout and "Decompressed from" not in r.stdout, r.stdout
        assert _listing(tmp_path) == before and not out.exists()
        assert r.returncode in statuses, (args, r.returncode, r.stdout)
        m = MISMATCH.search(r.stdout)
        if crc is None and not m:
            assert "Decompression failed" in r.stdout and r.returncode == 252, (args, r.stdout)
            return
        assert m, (args, r.stdout + r.stderr)
        assert (int(m.group(1)), int(m.group(2), 16)) == (1, table[1][3]) and int(m.group(3), 16) != table[1][3], r.stdout
        if crc is not None:
            assert int(m.group(3), 16) == crc, r.stdout

    refused(("-ds", out, bad), (252,), host_crc)
    refused(("-d", out, bad), (252,), None)
    refused(("-t", bad), (1, 252), None)
    # block 1 replaced by a sound archive of other bytes: every decoder decodes it, and the checksum alone tells
    other = bytearray(text1)
    other[len(other) // 2] ^= 0x20
    bad.write_bytes(_swap_block(blob, 1, bytes(other)))
    before = _listing(tmp_path)
    other_crc = zlib.crc32(bytes(other))
    refused(("-ds", out, bad), (252,), other_crc)
    refused(("-d", out, bad), (252,), other_crc)
    refused(("-t", bad), (1,), other_crc)
    # a lying table entry is found the same way
    lie = bytearray(blob)
    lie[12 + 2 * 24 + 16] ^= 1
    bad.write_bytes(bytes(lie))
    r = _bce("-t", bad)
    assert r.returncode == 1 and MISMATCH.search(r.stdout).group(1) == "2"


def test_cli_checked_container_of_one_byte(tmp_path):
    src, arc, out = tmp_path / "in", tmp_path / "a.bcem", tmp_path / "out"
    src.write_bytes(b"Q")
    r = _bce("-C1", arc, src)
    assert r.returncode == 0, r.stdout + r.stderr
    table = container.block_table(arc.read_bytes())
    assert [(t[0], t[3]) for t in table] == [(1, zlib.crc32(b"Q"))]
    assert container.unpack_blocks(arc.read_bytes())[0] == [bytes(api.compress(b"Q"))]
    assert _bce("-t", arc).returncode == 0
    for flag in ("-d", "-ds"):
        out.unlink(missing_ok=True)
        assert _bce(flag, out, arc).returncode == 0 and out.read_bytes() == b"Q"
    # more blocks than bytes: no archive, never a plain one in a checked one's place
    arc.unlink()
    r = _bce("-C2", arc, src)
    assert r.returncode != 0 and not arc.exists()


def test_last_chance_context_gives_crcs_too(tmp_path):
    data = bce_amd.synth_text(33, 400000).tobytes()
    src, arc = tmp_path / "in", tmp_path / "a.bcem"
    src.write_bytes(data)
    r = subprocess.run([EXE, "-C4", str(arc), str(src)], capture_output=True, text=True, env=dict(os.environ, BCE_CLI_TEST_NOMEM_BLOCK="all"))
    assert r.returncode == 0, r.stdout + r.stderr
    table = container.block_table(arc.read_bytes())
    assert [t[3] for t in table] == [zlib.crc32(data[b * 100000:(b + 1) * 100000]) for b in range(4)]
    assert _bce("-t", arc).returncode == 0


@pytest.mark.parametrize("blocks", [1, 2, 5])
def test_tensor_blocks_round_trip(blocks):
    host = bce_amd.synth_text(40 + blocks, 5 * 10**6 + 3)
    t = torch.from_numpy(host).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=blocks)
    table = container.block_table(blob)
    assert len(table) == blocks and sum(x[0] for x in table) == t.numel()
    at = 0
    for raw, _pos, _alen, crc in table:
        assert crc == zlib.crc32(host[at:at + raw].tobytes())
        at += raw
    u = bce_amd.decompress_container_tensor(blob)
    assert u.device == t.device and torch.equal(u, t)
    assert bce_amd.test_container(blob) is None
    # version 1 on request: what pack_blocks writes without CRCs, readable the same way, nothing to test
    v1 = bce_amd.compress_tensor_blocks(t, blocks=blocks, checksum=False)
    assert v1 == container.pack_blocks(*container.unpack_blocks(blob))
    assert torch.equal(bce_amd.decompress_container_tensor(v1), t)
    with pytest.raises(ValueError):
        bce_amd.test_container(v1)
    # a plain archive is accepted as well
    if blocks == 1:
        plain = container.unpack_blocks(blob)[0][0]
        assert torch.equal(bce_amd.decompress_container_tensor(plain), t)
        with pytest.raises(ValueError):
            bce_amd.test_container(plain)


def test_tensor_blocks_corruption_is_found_and_later_slices_stay_untouched():
    host = bce_amd.synth_text(50, 5 * 10**6)
    t = torch.from_numpy(host).to("cuda:0")
    blob = bce_amd.compress_tensor_blocks(t, blocks=5)
    text2 = host[2 * 10**6:3 * 10**6].tobytes()
    # a flipped byte in block 2's stream (it still decodes on the host decoder): the block is found, whichever check catches it
    found = _flip_block(blob, 2, text2)
    assert found is not None, "no flip inside block 2 found that still decodes"
    assert bce_amd.test_container(found[0]) == 2
    out = torch.full((5 * 10**6 + 100,), 0xEE, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(bce_amd.BceError):                                                  # (ChecksumError is one)
        bce_amd.decompress_container_tensor(found[0], out=out)
    assert torch.equal(out[:2 * 10**6], t[:2 * 10**6]) and bool((out[3 * 10**6:] == 0xEE).all())
    # block 2 replaced by a sound archive of other bytes: only the checksum tells
    other = bytearray(text2)
    other[123456] ^= 1
    bad, bad_crc = _swap_block(blob, 2, bytes(other)), zlib.crc32(bytes(other))
    assert bce_amd.test_container(bad) == 2
    out.fill_(0xEE)
    with pytest.raises(bce_amd.ChecksumError) as e:
        bce_amd.decompress_container_tensor(bad, out=out)
    assert (e.value.block, e.value.expected, e.value.actual) == (2, container.block_table(blob)[2][3], bad_crc)
    assert torch.equal(out[:2 * 10**6], t[:2 * 10**6])                                     # the blocks before it are sound
    assert bool((out[3 * 10**6:] == 0xEE).all())                                           # nothing behind the bad block's slice was written
    # check=False hands the bytes over as they are
    u = bce_amd.decompress_container_tensor(bad, check=False)
    assert torch.equal(u[:2 * 10**6], t[:2 * 10**6]) and not torch.equal(u, t)
    # a lying size in the table is refused before anything is written
    lie = bytearray(blob)
    lie[12:20] = (10**6 + 1).to_bytes(8, "little")
    out.fill_(0xEE)
    with pytest.raises(ValueError):
        bce_amd.decompress_container_tensor(bytes(lie), out=out)
    assert bool((out == 0xEE).all())


def test_tensor_of_more_than_2_to_the_31_bytes():
    """An input no single archive can hold: two blocks, round trip on the device, and the whole input's CRC from the blocks'."""
    n = (1 << 31) + 4096
    host = bce_amd.synth_text(1, n)
    t = torch.from_numpy(host).to("cuda:0")
    with pytest.raises(bce_amd.BceError):
        bce_amd.compress_tensor(t)                                                         # the reference's n < 2^31
    blob = bce_amd.compress_tensor_blocks(t, contexts=1)                                  # (one context: a block of 2^30 bytes fills the device's share)
    table = container.block_table(blob)
    assert [x[0] for x in table] == [n // 2, n // 2]
    whole = api.crc32_combine(table[0][3], table[1][3], table[1][0])
    assert whole == zlib.crc32(memoryview(host))
    u = bce_amd.decompress_container_tensor(blob)
    assert torch.equal(u, t)
