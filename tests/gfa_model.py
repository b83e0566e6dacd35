"""<prefix>.gfa as plain Python (include/disco_hip.h, disco_write_gfa): the model tests/test_gpu_gfa.py and tests/test_gfa_host.py hold
the device's bytes and gfa_check's to, and a parser with the two checks that need nothing but the file."""
from __future__ import annotations

import numpy as np

HEADER = b"H\tVN:Z:1.0\n"
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def unpack(packed: np.ndarray, lens: np.ndarray):
    """rows of 2-bit bases (32 a word, MSB first, A0 C1 G2 T3) -> one bytes object per read"""
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    shifts = (62 - 2 * np.arange(32)).astype(np.uint64)
    codes = ((packed[:, :, None] >> shifts[None, None, :]) & np.uint64(3)).astype(np.uint8).reshape(len(packed), -1)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [text[i, :int(lens[i])].tobytes() for i in range(len(packed))]


def c_fields(orient: int, len1: int, len2: int, start: int):
    """(sign, pos) of a contained row: forward for orientation 0 and 3; at `start` where the hit was the oriented prefix (3, 2), ending at
    len1 - start where it was the oriented suffix (0, 1)"""
    return ("+" if orient in (0, 3) else "-"), (start if orient in (3, 2) else len1 - start - len2)


def model(seqs, lens, names, edges, subs, rows) -> bytes:
    """seqs: the reads' bases (bytes) or None (no sequences); names: file index by read id; edges: disco_fetch_edges' records in their
    order; subs: None (exact overlaps) or the substitutions by edge; rows: disco_fetch_contained's records, any order"""
    out = [HEADER]
    for i in range(len(lens)):
        out.append(b"S\t%d\t%s\tLN:i:%d\n" % (int(names[i]), b"*" if seqs is None else seqs[i], int(lens[i])))
    for x, e in enumerate(edges):
        o = int(e["orient"])
        nm = b"" if subs is None else b"\tNM:i:%d" % int(subs[x])
        out.append(b"L\t%d\t%s\t%d\t%s\t%dM%s\n" % (int(names[int(e["src"])]), b"+" if o & 2 else b"-", int(names[int(e["dst"])]), b"+" if o & 1 else b"-",
                                                   int(e["len_src"]) - int(e["offset"]), nm))
    for r in rows[np.lexsort((rows["contained"], rows["j"], rows["super"]))] if len(rows) else []:
        sign, pos = c_fields(int(r["orient"]), int(r["len1"]), int(r["len2"]), int(r["start"]))
        out.append(b"C\t%d\t+\t%d\t%s\t%d\t%dM\n" % (int(names[int(r["super"])]), int(names[int(r["contained"])]), sign.encode(), pos, int(r["len2"])))
    return b"".join(out)


def parse(text: bytes):
    """-> (S: name -> (bases or None, LN), L: [(src, so, dst, do, ovl, nm or None)], C: [(container, contained, o, pos, len2)]); the line
    kinds in the file's order H, S, L, C, every line complete"""
    assert text.startswith(HEADER) and text.endswith(b"\n")
    S, L, Cc, order = {}, [], [], []
    for line in text[len(HEADER):-1].split(b"\n"):
        f = line.split(b"\t")
        if not order or order[-1] != f[0]:
            order.append(f[0])
        if f[0] == b"S":
            assert len(f) == 4 and f[3].startswith(b"LN:i:") and int(f[1]) not in S
            ln = int(f[3][5:])
            assert f[2] == b"*" or (len(f[2]) == ln and not f[2].translate(None, b"ACGT"))
            S[int(f[1])] = (None if f[2] == b"*" else f[2], ln)
        elif f[0] == b"L":
            assert len(f) in (6, 7) and f[2] in (b"+", b"-") and f[4] in (b"+", b"-") and f[5].endswith(b"M")
            nm = None
            if len(f) == 7:
                assert f[6].startswith(b"NM:i:")
                nm = int(f[6][5:])
            L.append((int(f[1]), f[2].decode(), int(f[3]), f[4].decode(), int(f[5][:-1]), nm))
        elif f[0] == b"C":
            assert len(f) == 7 and f[2] == b"+" and f[4] in (b"+", b"-") and f[6].endswith(b"M")
            Cc.append((int(f[1]), int(f[3]), f[4].decode(), int(f[5]), int(f[6][:-1])))
        else:
            raise AssertionError(line[:40])
    assert order == [k for k in (b"S", b"L", b"C") if k in order]
    return S, L, Cc


def oriented(seq: bytes, sign: str) -> bytes:
    return seq if sign == "+" else seq.translate(COMP)[::-1]


def mismatches(a: bytes, b: bytes) -> int:
    assert len(a) == len(b)
    return int(np.count_nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)))


def semantic_check(text: bytes, max_subs: int = 0):
    """what a GFA reader takes the lines to say, from the file alone: the last ovl bases of oriented src are the first ovl bases of
    oriented dst; the oriented contained read is container[pos : pos + len2] — up to max_subs mismatches, which an L line's NM counts"""
    S, L, Cc = parse(text)
    for src, so, dst, do, ovl, nm in L:
        a, b = oriented(S[src][0], so), oriented(S[dst][0], do)
        assert 0 < ovl <= min(len(a), len(b)), (src, dst, ovl)
        mm = mismatches(a[len(a) - ovl:], b[:ovl])
        assert mm <= max_subs, (src, so, dst, do, ovl, mm)
        assert (nm is None and max_subs == 0) or nm == mm, (src, dst, nm, mm)
    for sup, con, o, pos, len2 in Cc:
        a, b = S[sup][0], oriented(S[con][0], o)
        assert len(b) == len2 and 0 <= pos and pos + len2 <= len(a), (sup, con, pos, len2)
        assert mismatches(a[pos:pos + len2], b) <= max_subs, (sup, con, o, pos)
    return len(S), len(L), len(Cc)
