"""<prefix>.unitigs.reads as plain Python (include/disco_hip.h, disco_write_unitig_reads): the model tests/test_gpu_unitig_reads.py and
tests/test_unitig_reads_host.py hold the device's bytes and unitig_reads_check's to. It follows the rule literally — every contained
read walks to its root one hop after the other, no doubling, and a chain's reads are counted chain by chain — and has the checks that
need nothing but the file, <prefix>.unitigs.gfa beside it and the reads."""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import gfa_chains_model as gcm

HEADER = b"H\tunitig-reads\t1\n"


def direct(rows):
    """contained read -> (container, p, plus): oriented x is container[p, p + len[x]) — the C line of <prefix>.gfa"""
    out = {}
    for r in rows:
        o, start = int(r["orient"]), int(r["start"])
        p = start if o in (3, 2) else int(r["len1"]) - start - int(r["len2"])
        out[int(r["contained"])] = (int(r["super"]), p, o in (0, 3))
    return out


def root_of(x, lens, step):
    """(root, pos, plus, hops) of read x, walked hop by hop: x at (pos, s) of y and y at (q, t) of z -> x at q + pos, s of z when t is
    plus and at q + len[y] - pos - len[x], not s when t is minus. A walk that comes back to a read it has seen is a cycle"""
    y, pos, plus, hops, seen = x, 0, True, 0, {x}
    while y in step:
        z, q, t = step[y]
        if not 0 <= z < len(lens):
            raise ValueError("read %d has a row that names no read" % y)
        pos, plus = (q + pos, plus) if t else (q + int(lens[y]) - pos - int(lens[x]), not plus)
        y, hops = z, hops + 1
        if y in seen:
            raise ValueError("the containment rows hold a cycle through read %d" % y)
        seen.add(y)
    return y, pos, plus, hops


def chain_places(comp, links):
    """interior read -> (k, s_j, forward)"""
    out = {}
    for k, c in enumerate(comp):
        ls = links[int(c["first_link"]):int(c["first_link"]) + int(c["n_links"])]
        s = 0
        for j in range(len(ls) - 1):
            if j:
                s += int(ls[j]["offset"])
            out[int(ls[j]["to"])] = (k, s, bool(int(ls[j]["orient"]) & 1))
    return out


def placements(lens, rows, comp, links):
    """per read (segment: ("c", k) or ("r", read id), plus, start, root, hops)"""
    step, on_chain = direct(rows), chain_places(comp, links)
    out = []
    for x in range(len(lens)):
        r, pos, plus, hops = root_of(x, lens, step)
        if r in on_chain:
            k, s, forward = on_chain[r]
            start, plus = (s + pos, plus) if forward else (s + int(lens[r]) - pos - int(lens[x]), not plus)
            out.append((("c", k), plus, start, r, hops))
        else:
            out.append((("r", r), plus, pos, r, hops))
    return out


def model(lens, names, rows, comp, links, depth_only=False) -> bytes:
    """lens: the reads' lengths; names: file index by read id; rows: disco_fetch_contained's records; comp, links: what
    disco_fetch_chains returns"""
    names = [int(v) for v in names]
    place = placements(lens, rows, comp, links)
    reads, bases = Counter(), Counter()
    for x, (seg, _plus, _start, _r, _hops) in enumerate(place):
        reads[seg] += 1
        bases[seg] += int(lens[x])
    contained = {int(r["contained"]) for r in rows}
    inside = set(chain_places(comp, links))
    out = [HEADER]
    for i in range(len(lens)):
        if i not in contained and i not in inside:
            out.append(b"U\t%d\t%d\t%d\t%d\n" % (names[i], int(lens[i]), reads[("r", i)], bases[("r", i)]))
    for k, c in enumerate(comp):
        _, ln, _ = gcm.chain_segment(None, lens, c, links)
        out.append(b"U\tc%d\t%d\t%d\t%d\n" % (k, ln, reads[("c", k)], bases[("c", k)]))
    if not depth_only:
        for x, (seg, plus, start, r, hops) in enumerate(place):
            name = b"c%d" % seg[1] if seg[0] == "c" else b"%d" % names[seg[1]]
            out.append(b"R\t%d\t%s\t%s\t%d\t%d\t%d\t%d\n" % (names[x], name, b"+" if plus else b"-", start, int(lens[x]), names[r], hops))
    return b"".join(out)


def parse(text: bytes):
    """-> (U: [(segment, LN, reads, bases)], R: [(read, segment, strand, start, len, root, hops)]) with names as bytes; H, then U, then R"""
    assert text.startswith(HEADER) and text.endswith(b"\n")
    U, R = [], []
    body = text[len(HEADER):-1]
    for line in body.split(b"\n") if body else []:
        f = line.split(b"\t")
        if f[0] == b"U":
            assert len(f) == 5 and not R, line
            assert all(v.isdigit() for v in f[2:]) and (f[1][1:] if f[1].startswith(b"c") else f[1]).isdigit(), line
            U.append((f[1], int(f[2]), int(f[3]), int(f[4])))
        elif f[0] == b"R":
            assert len(f) == 8 and f[3] in (b"+", b"-"), line
            assert all(v.isdigit() for v in (f[1], f[4], f[5], f[6], f[7])), line
            R.append((f[1], f[2], f[3].decode(), int(f[4]), int(f[5]), f[6], int(f[7])))
        else:
            raise AssertionError(line[:40])
    return U, R


def semantic_check(reads_text: bytes, unitigs_gfa_text: bytes, read_seqs, names=None):
    """from the two files and the reads (read_seqs: bases by read id, names: file index by read id, id + 1 without): every read has
    exactly one R line, in order; every segment of the GFA exactly one U line, in S-line order, with its LN; reads and bases are the
    aggregates of the R lines; segment[start:start + len] is the oriented read; hops == 0 iff root == read.
    -> (U lines, R lines, R lines on chain segments, R lines that are '-', hops histogram as a list)"""
    U, R = parse(reads_text)
    S, _ = gcm.parse(unitigs_gfa_text)
    names = [i + 1 for i in range(len(read_seqs))] if names is None else [int(v) for v in names]
    assert [int(r[0]) for r in R] == names
    assert [(u[0], u[1]) for u in U] == [(k, v[1]) for k, v in S.items()]
    reads, bases = Counter(), Counter()
    for x, (read, seg, strand, start, ln, root, hops) in enumerate(R):
        seq = read_seqs[x]
        assert ln == len(seq) and seg in S, read
        assert 0 <= start and start + ln <= S[seg][1], read
        if S[seg][0] is not None:
            assert S[seg][0][start:start + ln] == gcm.oriented(seq, strand == "+"), (read, seg, strand, start)
        assert (hops == 0) == (root == read), read
        reads[seg] += 1
        bases[seg] += ln
    for seg, _ln, nr, nb in U:
        assert (nr, nb) == (reads[seg], bases[seg]), seg
    hist = Counter(r[6] for r in R)
    return len(U), len(R), sum(r[1].startswith(b"c") for r in R), sum(r[2] == "-" for r in R), [hist[h] for h in range(max(hist) + 1)] if hist else []


def depth_only_is_prefix(depth_text: bytes, full_text: bytes):
    """the depth-only file is the H and U lines of the full one"""
    U, R = parse(depth_text)
    assert not R and full_text.startswith(depth_text)
    rest = full_text[len(depth_text):]
    assert rest == b"" or rest.startswith(b"R\t")
    assert b"\nU\t" not in rest
    return len(U)
