"""<prefix>.unitigs.gfa as plain Python (include/disco_hip.h, disco_write_gfa_chains): the model tests/test_gpu_gfa_chains.py and
tests/test_gfa_chains_host.py hold the device's bytes and gfa_chains_check's to. It follows the rule literally — a chain is walked read
by read, every read laid over what is there from the base it begins at, with string slices and no prefix sums — and has the checks that
need nothing but the file."""
from __future__ import annotations

import numpy as np

HEADER = b"H\tVN:Z:1.0\n"
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def oriented(seq: bytes, plus: bool) -> bytes:
    return seq if plus else seq.translate(COMP)[::-1]


def interior(comp, links):
    """flag per link: its target is an interior read of its composite edge (every link but the last)"""
    inside = np.ones(len(links), dtype=bool)
    for c in comp:
        inside[int(c["first_link"]) + int(c["n_links"]) - 1] = False
    return inside


def chain_segment(seqs, lens, c, links):
    """(bases or None, LN, RC) of composite edge c: read r_j = l_j.to begins l_j.offset bases behind r_{j-1} and is who is read from there on"""
    ls = links[int(c["first_link"]):int(c["first_link"]) + int(c["n_links"])]
    m = len(ls) - 1
    assert m >= 1
    start, seg, ln = 0, b"", 0
    for j in range(m):
        r = int(ls[j]["to"])
        if j:
            start += int(ls[j]["offset"])
        ln = start + int(lens[r])
        if seqs is not None:
            assert start <= len(seg)
            seg = seg[:start] + oriented(seqs[r], bool(int(ls[j]["orient"]) & 1))
    return (None if seqs is None else seg), ln, m


def model(seqs, lens, names, contained, edges, absorbed, comp, links) -> bytes:
    """seqs: the reads' bases (bytes) or None (no sequences); names: file index by read id; contained: flag per read; edges:
    disco_fetch_edges' records in their order, absorbed: their flags; comp, links: what disco_fetch_chains returns"""
    skip = np.array(contained, dtype=bool).copy()
    skip[links["to"][interior(comp, links)].astype(np.int64)] = True
    out = [HEADER]
    for i in range(len(lens)):
        if not skip[i]:
            out.append(b"S\t%d\t%s\tLN:i:%d\n" % (int(names[i]), b"*" if seqs is None else seqs[i], int(lens[i])))
    for k, c in enumerate(comp):
        seg, ln, m = chain_segment(seqs, lens, c, links)
        out.append(b"S\tc%d\t%s\tLN:i:%d\tRC:i:%d\n" % (k, b"*" if seg is None else seg, ln, m))
    for x, e in enumerate(edges):
        if not absorbed[x]:
            o = int(e["orient"])
            out.append(b"L\t%d\t%s\t%d\t%s\t%dM\n" % (int(names[int(e["src"])]), b"+" if o & 2 else b"-", int(names[int(e["dst"])]), b"+" if o & 1 else b"-",
                                                     int(e["len_src"]) - int(e["offset"])))
    for k, c in enumerate(comp):
        first, n = int(c["first_link"]), int(c["n_links"])
        l0, ln_ = links[first], links[first + n - 1]
        a, b, last = int(c["a"]), int(c["b"]), int(links[first + n - 2]["to"])
        out.append(b"L\t%d\t%s\tc%d\t+\t%dM\n" % (int(names[a]), b"+" if int(l0["orient"]) & 2 else b"-", k, int(lens[a]) - int(l0["offset"])))
        out.append(b"L\tc%d\t+\t%d\t%s\t%dM\n" % (k, int(names[b]), b"+" if int(ln_["orient"]) & 1 else b"-", int(lens[last]) - int(ln_["offset"])))
    return b"".join(out)


def parse(text: bytes):
    """-> (S: name (bytes) -> (bases or None, LN, RC or None) in the file's order, L: [(src, so, dst, do, ovl)] with names as bytes); the
    line kinds in the order H, S, L, every line complete, the read segments before the chain segments"""
    assert text.startswith(HEADER) and text.endswith(b"\n")
    S, L, order, seen_chain = {}, [], [], False
    body = text[len(HEADER):-1]
    for line in body.split(b"\n") if body else []:
        f = line.split(b"\t")
        if not order or order[-1] != f[0]:
            order.append(f[0])
        if f[0] == b"S":
            chain = f[1].startswith(b"c")
            assert len(f) == (5 if chain else 4) and f[3].startswith(b"LN:i:"), line[:60]
            assert f[1] not in S, f[1]                                       # no segment name occurs twice
            assert (f[1][1:] if chain else f[1]).isdigit()
            assert not chain or f[4].startswith(b"RC:i:")
            assert chain or not seen_chain                                   # reads first, then chains
            seen_chain = chain
            ln = int(f[3][5:])
            assert f[2] == b"*" or (len(f[2]) == ln and not f[2].translate(None, b"ACGT")), f[1]   # LN is the length of the bases
            S[f[1]] = (None if f[2] == b"*" else f[2], ln, int(f[4][5:]) if chain else None)
        elif f[0] == b"L":
            assert len(f) == 6 and f[2] in (b"+", b"-") and f[4] in (b"+", b"-") and f[5].endswith(b"M"), line
            L.append((f[1], f[2].decode(), f[3], f[4].decode(), int(f[5][:-1])))
        else:
            raise AssertionError(line[:40])
    assert order == [k for k in (b"S", b"L") if k in order]
    return S, L


def semantic_check(text: bytes):
    """from the file alone: every name of an L line has an S line, and the last ovl bases of oriented src are the first ovl bases of
    oriented dst (parse has held every LN to its bases and every name to being the only one). -> (read segments, chain segments, L lines)"""
    S, L = parse(text)
    for src, so, dst, do, ovl in L:
        assert src in S and dst in S, (src, dst)
        assert 0 < ovl <= min(S[src][1], S[dst][1]), (src, dst, ovl)
        if S[src][0] is not None:
            a, b = oriented(S[src][0], so == "+"), oriented(S[dst][0], do == "+")
            assert a[len(a) - ovl:] == b[:ovl], (src, so, dst, do, ovl)
    n_chain = sum(k.startswith(b"c") for k in S)
    return len(S) - n_chain, n_chain, len(L)


def merged_chains(text: bytes):
    """every chain segment of the file merged with its two end reads by the overlaps of its head and tail link: oriented a, the segment
    from base ovl_a on, oriented b from base ovl_b on"""
    S, L = parse(text)
    head = {dst: (src, so, ovl) for src, so, dst, do, ovl in L if dst.startswith(b"c")}
    tail = {src: (dst, do, ovl) for src, so, dst, do, ovl in L if src.startswith(b"c")}
    out = []
    for k in (k for k in S if k.startswith(b"c")):
        (a, sa, oa), (b, sb, ob) = head[k], tail[k]
        out.append(oriented(S[a][0], sa == "+") + S[k][0][oa:] + oriented(S[b][0], sb == "+")[ob:])
    return out
