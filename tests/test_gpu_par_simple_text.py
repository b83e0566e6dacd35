"""-m gpu : the ParSimpleEdges lines from the GPU through the C-ABI — what the host pass gets after a chain contraction
(disco_fetch_chain_residue, disco_fetch_chain_first_edges) and what the device formats from a description of the final edges and its
own link arrays (disco_format_par_simple, disco_amd/csrc/disco_partext.h), against a few lines of Python on the links
disco_fetch_chains returns."""
import os

import numpy as np
import pytest

from disco_amd import buildgraph, readgen

pytestmark = pytest.mark.gpu


def _twin(o):
    return ((o >> 1) ^ 1) | (((o & 1) ^ 1) << 1)


SPECS = {
    "small": dict(seed=5, n_reads=30_000, read_len=110, cov=20.0, n_contigs=6, len_max=190),   # mixed lengths, 6 contigs
    "errors": dict(seed=22, n_reads=60_000, read_len=100, cov=25.0, n_contigs=12, len_max=220),  # + substitutions: tips and bubbles, a residue
    "long": dict(seed=15, n_reads=400_000, read_len=150, cov=30.0, n_contigs=4),               # chains far longer than a block and a scan tile
}


class Graph:
    """one graph and one contraction, shared by the tests of a read set; nothing here is changed by them"""

    def __init__(self, name, min_ovl):
        spec = readgen.GenSpec.coverage(**SPECS[name])
        self.g = g = buildgraph.BuildGraph(min_overlap=40)
        g.generate_reads(spec)
        if name == "errors":
            g.substitute_bases(5, 2000)
        g.run_graph()
        self.n = spec.n_reads
        self._lines = {}
        self.edges = g.fetch_edges()
        if min_ovl == "median":   # a filter that bites: half of the overlaps pass it
            min_ovl = int(np.median(self.edges["len_src"].astype(np.int64) - self.edges["offset"]))
        self.min_ovl = min_ovl
        self.comp, self.links, self.absorbed = g.contract_chains(min_ovl)
        self.res_index, self.res_edges = g.chain_residue()
        self.first_edge = g.chain_first_edges(len(self.comp))
        self.end_first, self.end_last_rev = g.chain_end_links(len(self.comp))
        self.length = np.zeros(self.n, dtype=np.int64)
        self.length[self.edges["src"].astype(np.int64)] = self.edges["len_src"]
        self.length[self.edges["dst"].astype(np.int64)] = self.edges["len_dst"]

    def round_one(self, n_files):
        """the graph after the device's round: every composite edge as one piece (forward if a <= b, else reversed), every residue
        edge as an inline link; sorted by (file, src, dst). Returns the description and, per described edge, its links."""
        ef = self.g.fetch_edge_files(n_files).astype(np.int64)
        L = self.length
        recs = []
        for k, c in enumerate(self.comp):
            a, b, off, o = int(c["a"]), int(c["b"]), int(c["offset"]), int(c["orient"])
            f = int(ef[int(self.first_edge[k])])
            if a <= b:
                recs.append((f, a, b, off, o, (1, k, 0, 0)))
            else:
                recs.append((f, b, a, int(L[b]) + off - int(L[a]), _twin(o), (2, k, 0, 0)))
        for i, e in zip(self.res_index, self.res_edges):
            recs.append((int(ef[int(i)]), int(e["src"]), int(e["dst"]), int(e["offset"]), int(e["orient"]), (0, int(e["dst"]), int(e["offset"]), int(e["orient"]))))
        recs.sort(key=lambda r: r[:5])
        edges = np.zeros(len(recs), dtype=buildgraph.PS_EDGE_DTYPE)
        pieces = np.zeros(len(recs), dtype=buildgraph.PS_PIECE_DTYPE)
        for i, (f, s, d, off, o, p) in enumerate(recs):
            edges[i] = (s, d, off, o, f, i, 1, 0)
            pieces[i] = p
        return edges, pieces

    def links_of(self, piece):
        kind, a, off, o = (int(x) for x in piece)
        if kind == 0:
            return [(a, off, o)]
        c = self.comp[a]
        ls = self.links[int(c["first_link"]):int(c["first_link"]) + int(c["n_links"])]
        to, offs, ori = ls["to"].astype(np.int64), ls["offset"].astype(np.int64), ls["orient"].astype(np.int64)
        if kind == 1:
            return list(zip(to.tolist(), offs.tolist(), ori.tolist()))
        frm = np.concatenate([[int(c["a"])], to[:-1]])
        roff = self.length[to] + offs - self.length[frm]
        rori = ((ori >> 1) ^ 1) | (((ori & 1) ^ 1) << 1)
        return list(zip(frm[::-1].tolist(), roff[::-1].tolist(), rori[::-1].tolist()))

    def expected(self, edges, pieces, n_files, file_index):
        idx = (lambda r: int(file_index[r])) if file_index is not None else (lambda r: r + 1)
        files = [[] for _ in range(n_files)]
        for e in edges:
            mine = pieces[int(e["first_piece"]):int(e["first_piece"]) + int(e["n_pieces"])]
            off = int(e["offset"])
            key = (file_index is not None, int(e["src"]), int(e["dst"]), off, int(e["orient"]), mine.tobytes())
            if key not in self._lines:   # (a line does not depend on the file it goes to: formatted once per set of files)
                ls = [l for p in mine for l in self.links_of(p)]
                self._lines[key] = (f"{idx(int(e['src']))}\t{idx(int(e['dst']))}\t{int(e['orient'])},{off},{off + int(self.length[int(e['dst'])])},0,0\t"
                                    + "".join(f"({idx(to)},{o & 1},{lo})" for to, lo, o in ls[:-1]) + "\n")
            files[int(e["file"])].append(self._lines[key])
        return ["".join(x).encode() for x in files]


_graphs = {}


def _graph(name, min_ovl):
    if (name, min_ovl) not in _graphs:
        _graphs[(name, min_ovl)] = Graph(name, min_ovl)
    return _graphs[(name, min_ovl)]


@pytest.fixture(scope="module", autouse=True)
def _close_graphs():
    yield
    for G in _graphs.values():
        G.g.close()
    _graphs.clear()


@pytest.mark.parametrize("name,min_ovl", [("small", 40), ("small", "median"), ("errors", 45), ("errors", "median"), ("long", 45)])
def test_residue_is_what_the_filter_passes_and_no_composite_took(name, min_ovl):
    G = _graph(name, min_ovl)
    kept = (G.edges["len_src"].astype(np.int64) - G.edges["offset"]) >= G.min_ovl
    if min_ovl == "median":
        assert 0 < kept.sum() < len(kept)                      # the filter bites
    want = np.nonzero(kept & (G.absorbed == 0))[0]
    if name == "errors":                                       # (error-free contigs are chains from end to end: nothing is left over)
        assert len(want) > 20
    assert np.array_equal(G.res_index.astype(np.int64), want)
    assert np.array_equal(G.res_edges, G.edges[want])
    # first edges: absorbed, and the edge joins the composite's a to its first link's read
    assert len(G.comp) > 0 and G.absorbed[G.first_edge.astype(np.int64)].all()
    fe = G.edges[G.first_edge.astype(np.int64)]
    first_to = G.links["to"][G.comp["first_link"].astype(np.int64)]
    ends = np.stack([np.minimum(G.comp["a"], first_to), np.maximum(G.comp["a"], first_to)])
    assert np.array_equal(np.stack([np.minimum(fe["src"], fe["dst"]), np.maximum(fe["src"], fe["dst"])]), ends)
    # end links: the first link a composite edge prints forward, and turned round (what the host pass orders the sides of a bubble by)
    assert np.array_equal(G.end_first, G.links[G.comp["first_link"].astype(np.int64)])
    for k in np.argsort(-G.comp["n_links"].astype(np.int64))[:50]:
        assert tuple(int(x) for x in G.end_last_rev[k]) == G.links_of((2, int(k), 0, 0))[0]


def test_residue_of_a_contraction_of_host_edges_and_of_an_empty_filter():
    g = buildgraph.BuildGraph(min_overlap=40)
    try:
        g.generate_reads(readgen.GenSpec.coverage(**SPECS["errors"]))
        g.substitute_bases(5, 2000)
        g.run_graph()
        edges = g.fetch_edges()
        mo = int(np.median(edges["len_src"].astype(np.int64) - edges["offset"]))
        g.contract_chains(mo)
        idx0, rec0 = g.chain_residue()
        g.contract_chains(mo, edges=edges)
        idx, rec = g.chain_residue(records=False)
        assert rec is None
        kept = (edges["len_src"].astype(np.int64) - edges["offset"]) >= mo
        _c, _l, absorbed = g.contract_chains(mo, edges=edges)
        assert np.array_equal(idx.astype(np.int64), np.nonzero(kept & (absorbed == 0))[0])
        assert len(idx0) > 0 and np.array_equal(idx, idx0) and np.array_equal(rec0, edges[idx0.astype(np.int64)])   # as from the resident edges
        with pytest.raises(buildgraph.DiscoError, match=r"error -4:"):
            g.chain_residue(records=True)                       # the caller holds the records: DISCO_E_STATE
        g.contract_chains(10_000)                               # a filter no overlap passes
        idx, rec = g.chain_residue()
        assert len(idx) == 0 and len(rec) == 0 and len(g.chain_first_edges(0)) == 0
    finally:
        g.close()


@pytest.mark.parametrize("name,min_ovl", [("small", 40), ("errors", 45), ("long", 45)])
def test_lines_of_the_round_one_graph_equal_pythons(name, min_ovl):
    G = _graph(name, min_ovl)
    assert (G.comp["a"] <= G.comp["b"]).any() and (G.comp["a"] > G.comp["b"]).any()   # both directions are printed
    if name == "long":
        assert int(G.comp["n_links"].max()) > 65_536
    fi = (np.arange(G.n, dtype=np.uint64) * 3 + 97)            # not id + 1; crosses 99 -> 100 and every later width
    for n_files in (1, 3, 7):
        edges, pieces = G.round_one(n_files)
        assert (pieces["kind"] == 1).any() and (pieces["kind"] == 2).any() and ((pieces["kind"] == 0).any() or name != "errors")
        for file_index in (None, fi):
            off = G.g.format_par_simple(edges, pieces, n_files, file_index)
            text = G.g.fetch_par_simple_text(int(off[-1]))
            got = [text[int(off[t]):int(off[t + 1])] for t in range(n_files)]
            want = G.expected(edges, pieces, n_files, file_index)
            assert [len(x) for x in got] == [len(x) for x in want]
            assert got == want


def test_text_into_real_descriptors_and_empty_files(tmp_path):
    G = _graph("small", 40)
    edges, pieces = G.round_one(3)
    edges = edges.copy()
    edges["file"] = np.where(edges["file"] == 0, 0, 4)          # five files, three of them empty
    off = G.g.format_par_simple(edges, pieces, 5)
    text = G.g.fetch_par_simple_text(int(off[-1]))
    assert off[1] == off[2] == off[3] == off[4] and 0 < off[1] < off[5]
    paths = [str(tmp_path / f"f{t}.txt") for t in range(5)]
    fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths]
    try:
        G.g.write_par_simple_text(fds)
    finally:
        for fd in fds:
            os.close(fd)
    assert [open(p, "rb").read() for p in paths] == [text[int(off[t]):int(off[t + 1])] for t in range(5)]
    with pytest.raises(buildgraph.DiscoError, match=r"error -4:"):
        G.g.write_par_simple_text(fds[:2])                      # formatted for five files


def test_errors_leave_the_context_usable_and_the_other_texts_alone():
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(readgen.GenSpec.coverage(**SPECS["small"]))
        g.run_graph()
        e1 = np.zeros(1, dtype=buildgraph.PS_EDGE_DTYPE)
        p1 = np.zeros(1, dtype=buildgraph.PS_PIECE_DTYPE)
        e1[0] = (0, 1, 5, 0, 0, 0, 1, 0)
        p1[0] = (0, 1, 5, 0)
        with pytest.raises(buildgraph.DiscoError, match=r"error -4:"):
            g.format_par_simple(e1, p1)                         # before any contraction: DISCO_E_STATE
    G = _graph("errors", 45)
    g = G.g
    etext, eoff = g.format_edges(2, g.fetch_edge_files(2))
    ctext, coff = g.format_contained(2)
    edges, pieces = G.round_one(2)
    off = g.format_par_simple(edges, pieces, 2)
    text = g.fetch_par_simple_text(int(off[-1]))

    def refused(e, p, n_files=2):
        with pytest.raises(buildgraph.DiscoError, match=r"error -1:"):
            g.format_par_simple(e, p, n_files)

    bad = pieces.copy()
    bad[int(np.nonzero(pieces["kind"] == 1)[0][0])]["a"] = len(G.comp)
    refused(edges, bad)                                         # a composite id >= n_composite
    bad = edges.copy()
    bad[-1]["n_pieces"] = 2
    refused(bad, pieces)                                        # a piece range beyond n_pieces
    bad = edges.copy()
    bad["file"] = bad["file"][::-1]
    refused(bad, pieces)                                        # descending files
    bad = pieces.copy()
    bad[int(np.nonzero(pieces["kind"] == 0)[0][0])]["a"] = G.n
    refused(edges, bad)                                         # a read id >= n
    refused(edges, pieces, n_files=1)                           # a file beyond n_files
    # still usable, and the three texts are kept apart
    off2 = g.format_par_simple(edges, pieces, 2)
    assert np.array_equal(off, off2) and g.fetch_par_simple_text(int(off2[-1])) == text
    etext2, eoff2 = g.format_edges(2, g.fetch_edge_files(2))
    ctext2, coff2 = g.format_contained(2)
    assert sorted(etext2.split(b"\n")) == sorted(etext.split(b"\n")) and ctext2 == ctext and np.array_equal(coff, coff2)
    assert g.fetch_par_simple_text(int(off2[-1])) == text
