"""Multi-block container for block-sharded compression.

The reference has no multi-block format (one block per archive, bce.cpp:1151-1157); this is an extension for
the sharded path only.  A plain single-block `.bce` archive is NOT wrapped, so it stays reference-compatible.

layout (little-endian):  b"BCEM" | u32 version=1 | u32 nblocks | nblocks x (u64 raw_bytes, u64 archive_bytes) | archives...
Every embedded archive is exactly what `bce -c` produces for that block alone (parity is per block).

Version 2 (`bce -CN`, pack_blocks with `crcs`) is the checked container: the same archives behind a table of
nblocks x (u64 raw_bytes, u64 archive_bytes, u32 crc32, u32 0), where crc32 is the CRC-32 of the block's TEXT as zlib.crc32
computes it.  Whoever decodes a block can test it without the original (`bce -d`, `bce -ds`, `bce -t archive`,
tensor.decompress_container_tensor, tensor.test_container); the CRC of the whole file follows from the blocks' by
crc32_combine.  Version 1 stays readable and stays what `bce -cN` and pack_blocks without `crcs` write, byte for byte.
"""
import struct

MAGIC = b"BCEM"


def pack_blocks(archives, raw_sizes, crcs=None):
    """The container of `archives`; with `crcs` (the CRC-32 of every block's text) a version-2 one."""
    if len(archives) != len(raw_sizes):
        raise ValueError("one raw size per archive")
    if crcs is None:
        out = [MAGIC, struct.pack("<II", 1, len(archives))]
        for a, r in zip(archives, raw_sizes):
            out.append(struct.pack("<QQ", r, len(a)))
    else:
        if len(crcs) != len(archives):
            raise ValueError("one CRC-32 per archive")
        out = [MAGIC, struct.pack("<II", 2, len(archives))]
        for a, r, c in zip(archives, raw_sizes, crcs):
            out.append(struct.pack("<QQII", r, len(a), c & 0xFFFFFFFF, 0))
    out.extend(archives)
    return b"".join(out)


def block_table(blob):
    """One entry per block: (raw_bytes, offset of the archive in `blob`, archive_bytes, crc32 or None for version 1).
    ValueError: not a container, an unknown version, a table or an archive beyond the blob, a reserved word that is
    not 0, bytes behind the last archive."""
    if bytes(blob[:4]) != MAGIC or len(blob) < 12:
        raise ValueError("not a BCEM container")
    ver, nb = struct.unpack_from("<II", blob, 4)
    if ver not in (1, 2):
        raise ValueError("unknown container version %d" % ver)
    entry = 16 if ver == 1 else 24
    pos = 12 + nb * entry
    if pos > len(blob):
        raise ValueError("container table beyond the end")
    table = []
    for b in range(nb):
        if ver == 1:
            raw, alen = struct.unpack_from("<QQ", blob, 12 + b * entry)
            crc = None
        else:
            raw, alen, crc, reserved = struct.unpack_from("<QQII", blob, 12 + b * entry)
            if reserved != 0:
                raise ValueError("reserved word of block %d is not 0" % b)
        if alen > len(blob) - pos:
            raise ValueError("archive of block %d beyond the end" % b)
        table.append((raw, pos, alen, crc))
        pos += alen
    if pos != len(blob):
        raise ValueError("trailing bytes in container")
    return table


def unpack_blocks(blob):
    """-> (archives, raw sizes) of a version-1 or version-2 container."""
    table = block_table(blob)
    return [bytes(blob[pos:pos + alen]) for _raw, pos, alen, _crc in table], [t[0] for t in table]


# ---- the delta file (`bce -gr` / `bce -ga`, api.delta / api.apply_delta) ------------------------------------------------------------
# A second buffer written against a base: copies out of the base plus literal bytes (bce_hip_parse).  A plain file; `bce -c`
# compresses it.  layout (little-endian):
#   b"BCED" | u32 version=1 | u64 n | u32 crc32(base) | u64 q | u32 crc32(result) | u32 min_len | u32 max_len | u64 nops | u64 nlits
#   | nops x (u32 len, u32 src)  (src == 0xFFFFFFFF: the next len literal bytes; else base[src : src + len]) | nlits bytes
DELTA_MAGIC = b"BCED"
DELTA_HEADER = struct.Struct("<4sIQIQIIIQQ")             # 56 bytes
DELTA_MAX = 0x7FFFFFFF                                   # a base and a result have fewer than 2^31 bytes


def pack_delta(n, base_crc, q, crc, min_len, max_len, ops, lits):
    """The delta file of `ops` (a numpy array of (len, src) records or pairs) and `lits` (uint8)."""
    import numpy as np
    ops = np.ascontiguousarray(ops)
    if ops.dtype.names is None:
        ops = np.ascontiguousarray(ops, dtype="<u4").reshape(-1, 2)
    lits = np.ascontiguousarray(lits, dtype=np.uint8).tobytes() if isinstance(lits, np.ndarray) else bytes(lits)
    nops = ops.shape[0]
    return b"".join([DELTA_HEADER.pack(DELTA_MAGIC, 1, n, base_crc & 0xFFFFFFFF, q, crc & 0xFFFFFFFF, min_len, max_len, nops, len(lits)),
                     ops.tobytes(), lits])


def unpack_delta(blob):
    """-> a dict: n, base_crc, q, crc, min_len, max_len, ops (an (nops, 2) uint32 array of (len, src)), lits (uint8).
    ValueError: not a delta file, an unknown version, sizes that do not add up to the file's length (judged without overflow:
    nops = 2^61 is a lie, not a wrap), a base or a result of 2^31 bytes or more.  Nothing here touches a device."""
    import numpy as np
    blob = bytes(blob)
    if len(blob) < DELTA_HEADER.size or blob[:4] != DELTA_MAGIC:
        raise ValueError("not a BCED delta file")
    _, ver, n, base_crc, q, crc, min_len, max_len, nops, nlits = DELTA_HEADER.unpack_from(blob, 0)
    if ver != 1:
        raise ValueError("unknown delta version %d" % ver)
    room = len(blob) - DELTA_HEADER.size
    if nops > room // 8 or nlits != room - nops * 8:
        raise ValueError("the delta's sizes do not add up to its length")
    if q > DELTA_MAX or n > DELTA_MAX or n == 0 and nops:
        raise ValueError("a delta of 2^31 bytes or more, or against nothing")
    ops = np.frombuffer(blob, dtype="<u4", count=nops * 2, offset=DELTA_HEADER.size).reshape(-1, 2)
    lits = np.frombuffer(blob, dtype=np.uint8, count=nlits, offset=DELTA_HEADER.size + nops * 8)
    return {"n": n, "base_crc": base_crc, "q": q, "crc": crc, "min_len": min_len, "max_len": max_len, "ops": ops, "lits": lits}
