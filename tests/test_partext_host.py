"""CPU: the item functions behind the ParSimpleEdges lines (disco_amd/csrc/disco_partext.h) built as plain C++ behind
disco_amd/bin/partext_check — one "lane" per item: header or inner read, found by binary search in the two prefix tables, the link
resolved forward, reversed or inline. The expected lines are formatted here from the definition in disco_amd/host/parsimple.h:
    src \\t dst \\t orient,offset,offset+len(dst),0,0 \\t (file_index[to],orient&1,offset) for every link but the last \\n"""
import os
import subprocess

import pytest

from disco_amd import build

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")


def _twin(o):
    return ((o >> 1) ^ 1) | (((o & 1) ^ 1) << 1)


class Case:
    """reads 0..n-1 with lengths; composite edges are (a, [links]) with links (to, offset, orient)"""

    def __init__(self, lengths, file_index=None, n_files=1):
        self.len, self.fi, self.n_files = list(lengths), file_index, n_files
        self.comp, self.links, self.edges, self.pieces = [], [], [], []

    def composite(self, a, links):
        self.comp.append(dict(a=a, b=links[-1][0], offset=sum(l[1] for l in links), orient=(links[0][2] & 2) | (links[-1][2] & 1), n=len(links), first=len(self.links)))
        self.links += links
        return len(self.comp) - 1

    def piece_links(self, p):
        """the links a piece stands for, in its direction — parsimple.cpp's Graph::append_links"""
        kind, a, off, o = p
        if kind == 0:
            return [(a, off, o)]
        c = self.comp[a]
        ls = self.links[c["first"]:c["first"] + c["n"]]
        if kind == 1:
            return list(ls)
        out = []
        for j in range(len(ls) - 1, -1, -1):
            frm = ls[j - 1][0] if j else c["a"]
            out.append((frm, self.len[ls[j][0]] + ls[j][1] - self.len[frm], _twin(ls[j][2])))
        return out

    def edge(self, src, file, pieces):
        """an edge out of src made of these pieces: header numbers derived from its links"""
        ls = [l for p in pieces for l in self.piece_links(p)]
        self.edges.append(dict(src=src, dst=ls[-1][0], offset=sum(l[1] for l in ls), orient=(ls[0][2] & 2) | (ls[-1][2] & 1), file=file, first=len(self.pieces), n=len(pieces)))
        self.pieces += pieces

    def idx(self, r):
        return self.fi[r] if self.fi else r + 1

    def expected(self):
        files = [b""] * self.n_files
        for e in self.edges:
            ls = [l for p in self.pieces[e["first"]:e["first"] + e["n"]] for l in self.piece_links(p)]
            line = f"{self.idx(e['src'])}\t{self.idx(e['dst'])}\t{e['orient']},{e['offset']},{e['offset'] + self.len[e['dst']]},0,0\t"
            line += "".join(f"({self.idx(to)},{o & 1},{off})" for to, off, o in ls[:-1]) + "\n"
            files[e["file"]] += line.encode()
        return files

    def write(self, path):
        w = [f"{len(self.len)} {self.n_files} {1 if self.fi else 0}", " ".join(map(str, self.len))]
        if self.fi:
            w.append(" ".join(map(str, self.fi)))
        w.append(str(len(self.comp)))
        w += [f"{c['a']} {c['b']} {c['offset']} {c['orient']} {c['n']} {c['first']}" for c in self.comp]
        w.append(str(len(self.links)))
        w += [f"{a} {b} {c}" for a, b, c in self.links]
        w.append(str(len(self.edges)))
        w += [f"{e['src']} {e['dst']} {e['offset']} {e['orient']} {e['file']} {e['first']} {e['n']}" for e in self.edges]
        w.append(str(len(self.pieces)))
        w += [" ".join(map(str, p)) for p in self.pieces]
        open(path, "w").write("\n".join(w) + "\n")


def _check(tmp_path, case):
    build.build_host()
    path = str(tmp_path / "case.txt")
    case.write(path)
    p = subprocess.run([os.path.join(BIN, "partext_check"), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    want = case.expected()
    off = [int(x) for x in p.stderr.decode().split("offsets")[1].split()]
    assert len(off) == case.n_files + 1 and off[0] == 0 and off[-1] == len(p.stdout)
    got = [p.stdout[off[t]:off[t + 1]] for t in range(case.n_files)]
    assert got == want
    return got


# nine reads of mixed lengths; a chain 0 -> 3 -> 5 -> 2 -> 7 with mixed orientations
LEN = [100, 140, 96, 120, 250, 101, 99, 180, 133]
CHAIN = [(3, 40, 3), (5, 61, 2), (2, 17, 1), (7, 88, 3)]


def test_a_simple_edge_has_no_inner_read(tmp_path):
    c = Case(LEN)
    c.edge(1, 0, [(0, 4, 33, 2)])
    assert _check(tmp_path, c) == [b"2\t5\t2,33,283,0,0\t\n"]


def test_one_forward_composite(tmp_path):
    c = Case(LEN)
    k = c.composite(0, CHAIN)
    c.edge(0, 0, [(1, k, 0, 0)])
    assert _check(tmp_path, c) == [b"1\t8\t3,206,386,0,0\t(4,1,40)(6,0,61)(3,1,17)\n"]


def test_the_same_composite_reversed(tmp_path):
    c = Case(LEN)
    k = c.composite(0, CHAIN)
    c.edge(7, 0, [(2, k, 0, 0)])
    got = _check(tmp_path, c)[0]
    # the reverse walk 7 -> 2 -> 5 -> 3 -> 0: offsets len[to] + offset - len[from], twinned orientations
    assert got == b"8\t1\t0,286,386,0,0\t(3,0,172)(6,1,12)(4,0,42)\n"


def test_an_edge_of_three_pieces(tmp_path):
    c = Case(LEN)
    k0 = c.composite(6, [(8, 30, 3), (1, 12, 3)])       # used reversed: 1 -> 8 -> 6
    k1 = c.composite(4, [(0, 77, 2), (3, 5, 1), (5, 9, 3)])
    c.edge(1, 0, [(2, k0, 0, 0), (0, 4, 50, 1), (1, k1, 0, 0)])
    got = _check(tmp_path, c)[0]
    assert got.count(b"(") == 2 + 1 + 3 - 1


def test_an_inline_link_reversed_by_the_description(tmp_path):
    """the host pass recomputes an inline link when it turns an edge round; the device prints what it is given"""
    c = Case(LEN)
    k = c.composite(0, CHAIN)
    fwd = (0, 1, 60, 3)                                    # 7 -> 1, continuing the chain
    c.edge(0, 0, [(1, k, 0, 0), fwd])
    rev = (0, 7, LEN[1] + 60 - LEN[7], _twin(3))           # 1 -> 7
    c.edge(1, 0, [rev, (2, k, 0, 0)])
    a, b = _check(tmp_path, c)[0].splitlines()
    assert a.count(b"(") == b.count(b"(") == 4
    assert b.split(b"\t")[3].startswith(b"(8,0,")          # the reversed inline link leads into read 7 (index 8), twin(3) & 1 == 0


def test_file_indices_that_are_not_id_plus_one_and_change_width(tmp_path):
    fi = [9, 10, 99, 100, 101, 999, 1000, 123456789012, 7]
    c = Case(LEN, file_index=fi)
    k = c.composite(0, CHAIN)
    c.edge(0, 0, [(1, k, 0, 0)])
    c.edge(7, 0, [(2, k, 0, 0)])
    c.edge(8, 0, [(0, 1, 3, 0)])
    got = _check(tmp_path, c)[0]
    assert got.startswith(b"9\t123456789012\t") and b"(100,1,40)(999,0,61)(99,1,17)" in got and got.endswith(b"7\t10\t0,3,143,0,0\t\n")


def test_two_files_one_of_them_empty(tmp_path):
    for empty in (0, 1, 2):
        c = Case(LEN, n_files=3)
        k = c.composite(0, CHAIN)
        files = [t for t in range(3) if t != empty]
        c.edge(0, files[0], [(1, k, 0, 0)])
        c.edge(1, files[0], [(0, 4, 33, 2)])
        c.edge(7, files[1], [(2, k, 0, 0)])
        got = _check(tmp_path, c)
        assert got[empty] == b"" and all(got[t] for t in files)


@pytest.mark.parametrize("what", ["composite", "pieces", "files", "read"])
def test_the_tool_refuses_what_the_library_refuses(tmp_path, what):
    build.build_host()
    c = Case(LEN, n_files=2)
    k = c.composite(0, CHAIN)
    c.edge(0, 1, [(1, k, 0, 0)])
    c.edge(1, 1, [(0, 4, 33, 2)])
    if what == "composite":
        c.pieces[0] = (1, 5, 0, 0)
    elif what == "pieces":
        c.edges[1]["n"] = 2
    elif what == "files":
        c.edges[1]["file"] = 0
    else:
        c.pieces[1] = (0, len(LEN), 1, 0)
    path = str(tmp_path / "bad.txt")
    c.write(path)
    p = subprocess.run([os.path.join(BIN, "partext_check"), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and p.stdout == b""
