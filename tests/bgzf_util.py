"""BGZF test inputs: a writer on Python's zlib alone (members of gzip with a `BC` extra subfield, what bgzip / htslib write), the matrix
of deflate settings the decoder tests walk, and the generator of damaged files both the host and the device tests draw from."""
import struct
import zlib

import numpy as np

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# every setting the decoder must read: stored (level 0), fixed codes (Z_FIXED), dynamic codes (the rest), an empty stored block inside
SETTINGS = [dict(level=0), dict(level=1), dict(level=6), dict(level=9), dict(strategy=zlib.Z_FIXED), dict(strategy=zlib.Z_HUFFMAN_ONLY),
            dict(strategy=zlib.Z_RLE), dict(flush_at=1000)]
MEMBER_SIZES = (65280, 4096)


def bgzf_block(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    payload = (c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()) if flush_at else c.compress(data) + c.flush()
    bsize = len(payload) + 25                     # must stay <= 65535
    assert bsize <= 65535
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize)
            + payload + struct.pack("<II", zlib.crc32(data), len(data)))


def bgzf_members(text, member=65280, **kw):
    """the members of `text` cut every `member` bytes (no end-of-file member)"""
    return [bgzf_block(text[i:i + member], **kw) for i in range(0, len(text), member)]


def bgzf_bytes(text, member=65280, eof=True, **kw):
    return b"".join(bgzf_members(text, member, **kw)) + (EOF_MEMBER if eof else b"")


def fasta_text(seed, n_reads, lo=60, hi=250):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_reads):
        out.append(b">r%d\n" % i + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(lo, hi)))) + b"\n")
    return b"".join(out)


MUTATIONS = ("payload", "crc", "isize", "bsize", "truncate", "header_bytes", "second_subfield")
MUST_ACCEPT = ("header_bytes", "second_subfield")  # bytes no reader of BGZF looks at; an extra subfield next to BC is legal


def mutated_files(n=400, seed=20240611, text=None):
    """n damaged BGZF files, the same for every caller: (kind, bytes). Settings and member sizes go round the matrix, the kind of
    damage round MUTATIONS; which member and which byte comes from the seeded generator."""
    rng = np.random.default_rng(seed)
    text = text if text is not None else fasta_text(seed, 900)
    base = {}
    out = []
    for k in range(n):
        si, member = k % len(SETTINGS), MEMBER_SIZES[(k // len(SETTINGS)) % 2]
        if (si, member) not in base:
            base[(si, member)] = bgzf_members(text, member, **SETTINGS[si])
        mem = list(base[(si, member)])
        kind = MUTATIONS[(k // (2 * len(SETTINGS)) + k) % len(MUTATIONS)]
        j = int(rng.integers(0, len(mem)))
        m = bytearray(mem[j])
        if kind == "payload":
            m[int(rng.integers(18, len(m) - 8))] ^= int(rng.integers(1, 256))
        elif kind == "crc":
            m[len(m) - 8 + int(rng.integers(0, 4))] ^= int(rng.integers(1, 256))
        elif kind == "isize":
            m[len(m) - 4 + int(rng.integers(0, 4))] ^= int(rng.integers(1, 256))
        elif kind == "bsize":
            m[16 + int(rng.integers(0, 2))] ^= int(rng.integers(1, 256))
        elif kind == "header_bytes":
            for p in range(4, 10):
                m[p] = int(rng.integers(0, 256))
        elif kind == "second_subfield":
            sub = b"XY" + struct.pack("<H", 3) + b"abc"
            bsize = struct.unpack_from("<H", m, 16)[0] + len(sub)
            bc = b"BC" + struct.pack("<HH", 2, bsize)
            m = bytearray(bytes(m[:10]) + struct.pack("<H", 6 + len(sub)) + (sub + bc if rng.random() < 0.5 else bc + sub) + bytes(m[18:]))
        mem[j] = bytes(m)
        data = b"".join(mem) + EOF_MEMBER
        if kind == "truncate":
            data = data[:int(rng.integers(1, len(data)))]
        out.append((kind, data))
    return out
