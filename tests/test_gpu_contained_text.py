"""-m gpu : disco_format_contained through the C-ABI — the lines of <prefix>_<t>_containedReads.txt (BG/OverlapGraph.cpp:438-447) grouped by
containing read, sorted and formatted on the GPU, against the same lines formatted here from disco_fetch_contained and from the oracle."""
import os

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from oracle import pyoracle

pytestmark = pytest.mark.gpu

SPEC = readgen.GenSpec.coverage(seed=43, n_reads=200_000, read_len=100, cov=25.0, n_contigs=7, len_max=250)
LDS_TIER = 4096  # CGRP_LDS_MAX of disco_amd/csrc/disco_text.h: groups beyond it are sorted through global memory


def _lines(rows, fidx):
    """the rows' lines in the files' order: ascending (containing read, j, contained read)"""
    rows = rows[np.lexsort((rows["contained"], rows["j"], rows["super"]))]
    out = []
    for r in rows:
        l2, l1, st = int(r["len2"]), int(r["len1"]), int(r["start"])
        out.append(f"{fidx[int(r['contained'])]}\t{fidx[int(r['super'])]}\t{int(r['orient'])},{l2},0,0,{l2},0,{l2},{l1},{st},{st + l2}\n")
    return rows, out


def _per_file(rows, lines, n_files, n):
    """text of every file: the rows whose containing read s has s * n_files // n == t"""
    owner = (rows["super"].astype(np.int64) * n_files) // n
    first = np.searchsorted(owner, np.arange(n_files + 1))
    return ["".join(lines[first[t]:first[t + 1]]).encode() for t in range(n_files)]


def _check(text, off, want_files):
    n_files = len(want_files)
    assert len(off) == n_files + 1 and off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off.astype(np.int64)) >= 0)
    for t in range(n_files):
        assert text[int(off[t]):int(off[t + 1])] == want_files[t], t


@pytest.fixture(scope="module")
def graph():
    """one pass over the 200 k set, shared: the context (graph built) and its rows"""
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(SPEC)
        g.run_graph()
        rows = g.fetch_contained()
        assert len(rows) > 1000
        yield g, rows


def _fidx(mapped):
    # file indices as the input stage assigns them when records are filtered: increasing, with gaps, up to 11 digits
    return np.arange(SPEC.n_reads, dtype=np.uint64) * np.uint64(3 if mapped else 1) + np.uint64(9_999_999_990 if mapped else 1)


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("n_files", [1, 7, 200, 5000])
def test_contained_text_equals_lines_formatted_from_the_records(graph, n_files, mapped):
    g, rows = graph
    fidx = _fidx(mapped)
    srows, lines = _lines(rows, fidx)
    text, off = g.format_contained(n_files, fidx if mapped else None)
    _check(text, off, _per_file(srows, lines, n_files, SPEC.n_reads))
    assert text.count(b"\n") == len(rows)   # (with 5000 files some own no containing read: equal offsets, checked above)


def test_contained_text_knows_no_row_limit(graph, monkeypatch):
    """DISCO_EAGER_ROWS_MAX gates the rows staged for the host, not this path: the same text"""
    g, rows = graph
    want, off0 = g.format_contained(7)
    monkeypatch.setenv("DISCO_EAGER_ROWS_MAX", "100")
    with buildgraph.BuildGraph(min_overlap=40) as h:
        h.generate_reads(SPEC)
        h.run_graph()
        text, off = h.format_contained(7)
    assert text == want and np.array_equal(off, off0) and len(text) > 20 * len(rows)


def big_group_reads(L, l, sizes, seed=5):
    """containing reads of L bases first (ids 0..: each the smallest container of its substrings); container i gets sizes[i] - sizes[i] // 4
    substrings of l bases at random offsets, half of them reverse-complemented, and sizes[i] // 4 exact duplicates of the first ones (ties on
    (containing read, j)); 500 unrelated reads of l + 20 bases; everything behind the containers shuffled"""
    rng = np.random.default_rng(seed)
    comp = str.maketrans("ACGT", "TGCA")
    rnd = lambda m: "".join("ACGT"[x] for x in rng.integers(0, 4, m))
    cont = [rnd(L) for _ in sizes]
    rest = []
    for c, s in zip(cont, sizes):
        sub = []
        for i in range(s - s // 4):
            o = int(rng.integers(0, L - l + 1))
            r = c[o:o + l]
            sub.append(r.translate(comp)[::-1] if i & 1 else r)
        rest += sub + sub[:s // 4]
    rest += [rnd(l + 20) for _ in range(500)]
    rng.shuffle(rest)
    return cont + rest


BIG_CASES = {
    "one_class": dict(L=250, l=60, min_overlap=20, sizes=[2, 255, 256, 257, 1025, 4097, 9000], n_reads=15_399, n_rows=14_892),
    "two_classes": dict(L=3000, l=100, min_overlap=40, sizes=[2, 255, 256, 257, 1025, 4097, 9000, 40000], n_reads=55_400, n_rows=54_892),
}


@pytest.mark.parametrize("case", list(BIG_CASES))
def test_groups_of_every_tier_against_the_oracle(case):
    """groups for the insertion sort (2, 255, 256), the LDS tier (257, 1025) and the tier through global memory (4097, 9000, 40 000 rows —
    more than a CU's LDS holds), with up to 32 rows sharing one (containing read, j): the text of three files, byte for byte, from the
    ORACLE's rows — no group is left out, and disco_fetch_contained_grouped still declines such sets"""
    c = BIG_CASES[case]
    reads = big_group_reads(c["L"], c["l"], c["sizes"])
    codes, off = pyoracle.encode_reads(reads)
    orows, oedges, ocnt = pyoracle.build_graph(codes, off, c["min_overlap"])
    assert len(reads) == c["n_reads"] and len(orows) == c["n_rows"] and len(oedges) == 0 and ocnt["cap_bind_sites"] == ocnt["asymmetric_pairs"] == 0
    sizes = np.bincount(orows["super"].astype(np.int64), minlength=len(c["sizes"]))
    assert list(sizes[:len(c["sizes"])]) == c["sizes"] and sizes[len(c["sizes"]):].sum() == 0
    assert max(c["sizes"]) > 2 * LDS_TIER and sum(s > LDS_TIER for s in c["sizes"]) >= 2 and any(256 < s <= LDS_TIER for s in c["sizes"])
    fidx = np.arange(len(reads), dtype=np.uint64) + np.uint64(1)
    srows, lines = _lines(orows, fidx)
    with buildgraph.BuildGraph(min_overlap=c["min_overlap"]) as g:
        g.upload_ascii(reads)
        g.run_graph()
        two = g.long_rows > 0
        text, toff = g.format_contained(3)
        grouped = g.fetch_contained_grouped()
    print(case, "long rows:", two, "text bytes:", len(text))
    _check(text, toff, _per_file(srows, lines, 3, len(reads)))
    assert text.count(b"\n") == c["n_rows"]
    assert grouped is None
    assert two == (case == "two_classes")


@pytest.mark.parametrize("text_first", ["contained", "edges"])
def test_contained_text_streamed_into_files_equals_the_fetched_text(graph, tmp_path, text_first):
    """disco_write_contained_text through the pinned ring, into 1 and 7 open files, interleaved with the edge text in both orders: neither
    text disturbs the other"""
    g, rows = graph

    def stream(write, text, off, tag):
        n_files = len(off) - 1
        paths = [str(tmp_path / f"{tag}{n_files}_{t}.txt") for t in range(n_files)]
        fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths]
        write(fds, threads=5)
        for fd in fds:
            os.close(fd)
        for t, p in enumerate(paths):
            assert open(p, "rb").read() == text[int(off[t]):int(off[t + 1])], (tag, n_files, t)
        assert sum(os.path.getsize(p) for p in paths) == len(text) > 0

    for n_files in (1, 7):
        files = g.fetch_edge_files(n_files)
        if text_first == "contained":
            ctext, coff = g.format_contained(n_files)
            etext, eoff = g.format_edges(n_files, files if n_files > 1 else None, None)
        else:
            etext, eoff = g.format_edges(n_files, files if n_files > 1 else None, None)
            ctext, coff = g.format_contained(n_files)
        assert ctext.count(b"\n") == len(rows)
        if text_first == "contained":
            stream(g.write_edge_text, etext, eoff, "e")
            stream(g.write_contained_text, ctext, coff, "c")
        else:
            stream(g.write_contained_text, ctext, coff, "c")
            stream(g.write_edge_text, etext, eoff, "e")
        stream(g.write_contained_text, ctext, coff, "c")   # once more, after the other text went through the ring


def test_contained_text_limits():
    spec = readgen.GenSpec.coverage(seed=42, n_reads=3000, read_len=100, cov=20.0)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.build_index()
        g.probe()
        with pytest.raises(buildgraph.DiscoError):
            g.format_contained(1)                       # no contained flags yet
        n_cont = g.mark_contained()
        text, off = g.format_contained(2)               # from disco_mark_contained on: no edges needed
        assert text.count(b"\n") == n_cont and off[-1] == len(text)
        g.build_edges()
        g.transitive_reduce()
        rows = g.fetch_contained()
    srows, lines = _lines(rows, np.arange(spec.n_reads, dtype=np.uint64) + np.uint64(1))
    _check(text, off, _per_file(srows, lines, 2, spec.n_reads))


def test_nothing_contained_gives_empty_files(tmp_path):
    rng = np.random.default_rng(7)
    reads = ["".join("ACGT"[x] for x in rng.integers(0, 4, 100)) for _ in range(50)]
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        g.run_graph()
        text, off = g.format_contained(3)
        assert text == b"" and list(off) == [0, 0, 0, 0]
        paths = [str(tmp_path / f"c{t}.txt") for t in range(3)]
        fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths]
        g.write_contained_text(fds)
        for fd in fds:
            os.close(fd)
        assert [os.path.getsize(p) for p in paths] == [0, 0, 0]


def test_contained_text_is_refused_under_a_communicator():
    gs = [buildgraph.BuildGraph(min_overlap=40) for _ in range(2)]
    try:
        buildgraph.BuildGraph.comm_init_local(gs)
        with pytest.raises(buildgraph.DiscoError):
            gs[0].format_contained(1)
    finally:
        for g in gs:
            g.close()


def test_contained_text_with_inexact_overlaps():
    """max_substitutions = 2: the line has no substitutions column, so the path works and equals the lines from the rows"""
    spec = readgen.GenSpec.coverage(seed=42, n_reads=3000, read_len=100, cov=20.0, len_max=180)
    with buildgraph.BuildGraph(min_overlap=40, max_substitutions=2) as g:
        g.generate_reads(spec)
        g.run_graph()
        rows = g.fetch_contained()
        text, off = g.format_contained(4)
    assert len(rows) > 100
    srows, lines = _lines(rows, np.arange(spec.n_reads, dtype=np.uint64) + np.uint64(1))
    _check(text, off, _per_file(srows, lines, 4, spec.n_reads))
