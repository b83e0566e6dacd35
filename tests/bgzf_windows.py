"""The windows of a BGZF file's text that the window decoder must clip right, the same list for the host tool (inflate_check --window) and
the device (disco_inflate_bgzf_window), and the files they are cut out of: members of 700, 4096 and 65280 text bytes in every deflate
setting of tests/bgzf_util.py (stored and compressed), and one file with empty members between the others."""
import functools
import gzip

from tests import bgzf_util as bz

WINDOW_MEMBERS = (700, 4096, 65280)
FILES = [(member, si) for member in WINDOW_MEMBERS for si in range(len(bz.SETTINGS))]


@functools.lru_cache(maxsize=None)
def file_text(member):
    """about six members of the small sizes, three and a short one of the large"""
    return bz.fasta_text(17, 40 if member == 700 else (160 if member == 4096 else 1300))


def plain_file(member, si):
    """(file bytes, text, text offsets at which its members begin)"""
    text = file_text(member)
    return bz.bgzf_bytes(text, member, **bz.SETTINGS[si]), text, list(range(0, len(text), member))


def middle(bounds):
    """the member whose boundaries windows() works on: B1 = bounds[middle], B2 the next one"""
    return max(1, len(bounds) // 2 - 1)


def file_with_empty_members():
    """members of 700 bytes with an empty one exactly on B1 (between two members), two more on B2 and one at the very end; the bounds
    list the places of the members that have text"""
    text = file_text(700)
    mem = bz.bgzf_members(text, 700)
    bounds = list(range(0, len(text), 700))
    k = middle(bounds)
    data = b"".join(mem[:k]) + bz.EOF_MEMBER + mem[k] + bz.EOF_MEMBER * 2 + b"".join(mem[k + 1:]) + bz.EOF_MEMBER
    assert gzip.decompress(data) == text and len(mem) >= 6
    return data, text, bounds


def windows(bounds, total):
    """sorted (lo, n): around the member boundaries B1 < B2 in the middle of the file —
    a window inside one member (cut at both ends), one byte, a member cut at its front only / at its back only / two members cut at the
    far ends; edges on a boundary and one byte to either side; the first byte of a member at the 16-byte multiples of the destination
    (the destination of text byte x is out + x - lo) and one byte to either side, the window's end likewise; the ends of the text"""
    k = middle(bounds)
    B1, B2 = bounds[k], (bounds[k + 1] if k + 1 < len(bounds) else total)
    B3 = bounds[k + 2] if k + 2 < len(bounds) else total
    size = B2 - B1
    mid = B1 + size // 3
    w = {(0, total), (0, total + 100), (0, 1), (0, 0), (total - 1, 1), (total - 3, 10), (total, 5), (total + 7, 3), (1, total - 2)}
    w |= {(mid, max(1, size // 3)), (mid, 1), (mid, B2 - mid), (B1, mid - B1), (mid, B2 + (B3 - B2) // 2 - mid), (B1 - 5, B3 - B1 + 9)}
    for lo in (B1 - 1, B1, B1 + 1):
        for hi in (B2 - 1, B2, B2 + 1, B1 + 2):
            if hi > lo:
                w.add((lo, hi - lo))
    w |= {(B1 - 1, 1), (B1, 1), (B1 - 1, 2), (B2 - 1, 1), (B2 - 2, 2), (B2 - 2, 3)}
    for back in (0, 16, 48):
        for dl in (-1, 0, 1):
            lo = B1 - back + dl
            if lo < 0:
                continue
            for body in (16, 64, 16 * (size // 16 + 3)):
                for dn in (-1, 0, 1):
                    w.add((lo, body + dn))
    return sorted(x for x in w if x[0] >= 0 and x[1] >= 0)


def corrupt_crc(data, member_starts_in_file, k):
    """the file with one bit of member k's CRC32 flipped (member k: bytes [starts[k], starts[k + 1]) of the file)"""
    d = bytearray(data)
    d[member_starts_in_file[k + 1] - 6] ^= 0x40
    return bytes(d)


def member_offsets(data):
    """file offsets of the members by their BSIZE fields (the writer's fixed 18-byte header), the file's end last"""
    off, at = [], 0
    while at < len(data):
        off.append(at)
        at += (data[at + 16] | data[at + 17] << 8) + 1
    assert at == len(data)
    return off + [at]
