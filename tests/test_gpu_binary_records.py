"""-m gpu : the records of the binary side output formed on the GPU (disco_prepare_edge_records / disco_prepare_contained_records and their
fetch / write calls, disco_amd/csrc/disco_binrec.h) through the ctypes mirror — record for record what numpy builds from disco_fetch_edges,
disco_fetch_edge_files and disco_fetch_contained, which the other suites hold to the oracle. Every comparison is exact."""
import os

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from disco_amd.edgefile import CONTAINED, EDGE
from oracle import pyoracle
from tests.test_gpu_contained_text import BIG_CASES, big_group_reads
from tests.test_gpu_inexact import _mutated
from tests.test_gpu_two_class import mixed_reads

pytestmark = pytest.mark.gpu

SENTINEL = bytes(range(0xA0, 0xC0))  # 32 bytes where the header goes: the write calls must leave them alone


def edge_records(edges, files, n_files, fidx, subs=None):
    """the host writer's edge records (disco_amd/host/writer.cpp write_binary_edges) from the fetched arrays, in fetch order"""
    r = np.zeros(len(edges), dtype=EDGE)
    r["src"], r["dst"] = fidx[edges["src"].astype(np.int64)], fidx[edges["dst"].astype(np.int64)]
    for f in ("orient", "offset", "len_src", "len_dst"):
        r[f] = edges[f]
    r["file"] = np.minimum(files.astype(np.int64), n_files - 1) if n_files > 1 else 0
    r["flag"] = 2
    r["substitutions"] = 0 if subs is None else subs
    return r


def contained_records(rows, n_files, n, fidx):
    """... and its contained records: ascending (containing read, j, contained read), file = super * n_files // n"""
    rows = rows[np.lexsort((rows["contained"], rows["j"], rows["super"]))]
    r = np.zeros(len(rows), dtype=CONTAINED)
    r["contained"], r["super"] = fidx[rows["contained"].astype(np.int64)], fidx[rows["super"].astype(np.int64)]
    for f in ("orient", "len2", "len1", "start"):
        r[f] = rows[f]
    r["file"] = rows["super"].astype(np.int64) * n_files // max(n, 1)
    return r


def identity(n):
    return np.arange(n, dtype=np.uint64) + np.uint64(1)


def take(g, n_files, n, fidx=None, subs=False):
    """(edge records, contained records) from the device beside the same records built here from the fetched arrays"""
    edges, rows = g.fetch_edges(), g.fetch_contained()
    files = g.fetch_edge_files(n_files)
    ne = g.prepare_edge_records(n_files, files if n_files > 1 else None, fidx)
    nc = g.prepare_contained_records(n_files, fidx)
    assert (ne, nc) == (len(edges), len(rows))
    fi = identity(n) if fidx is None else fidx
    want_e = edge_records(edges, files, n_files, fi, g.fetch_edge_substitutions() if subs else None)
    want_c = contained_records(rows, n_files, n, fi)
    return g.fetch_edge_records(ne), g.fetch_contained_records(nc), want_e, want_c


def same(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()  # every byte, the pads included


# ---- wave and piece boundaries on tiled reads --------------------------------------------------------------------------------------
def tiled_reads(n, m, seed=5):
    """n reads of 100 bases cut at step 30 from a random contig, and the bases [20, 80) of the first m of them"""
    rng = np.random.default_rng(seed)
    contig = "".join("ACGT"[x] for x in rng.integers(0, 4, 30 * (n - 1) + 100))
    reads = [contig[30 * i:30 * i + 100] for i in range(n)]
    return reads + [r[20:80] for r in reads[:m]]


def unrelated_reads():
    rng = np.random.default_rng(6)
    return ["".join("ACGT"[x] for x in rng.integers(0, 4, 100)) for _ in range(2)]


TILED = [(2, 0), (2, 1), (64, 0), (65, 63), (66, 64), (67, 65), (130, 1)]


def _written(write, count, piece, path, g):
    with open(path, "wb") as f:
        f.write(SENTINEL)
    g.set_record_piece(piece)
    fd = os.open(path, os.O_WRONLY)
    try:
        write(fd, 32, threads=3)
    finally:
        os.close(fd)
        g.set_record_piece(0)
    data = open(path, "rb").read()
    assert len(data) == 32 + 40 * count, (piece, len(data))
    assert data[:32] == SENTINEL, piece
    return data[32:]


@pytest.mark.parametrize("shape", TILED + ["unrelated"], ids=lambda s: s if isinstance(s, str) else f"{s[0]}+{s[1]}")
def test_records_of_tiled_reads_across_wave_and_piece_boundaries(shape, tmp_path):
    reads = unrelated_reads() if shape == "unrelated" else tiled_reads(*shape)
    want_counts = (0, 0) if shape == "unrelated" else (shape[0] - 1, shape[1])
    codes, off = pyoracle.encode_reads(reads)
    orows, oedges, ocnt = pyoracle.build_graph(codes, off, 40)
    assert (len(oedges), len(orows)) == want_counts and ocnt["cap_bind_sites"] == ocnt["asymmetric_pairs"] == 0
    n_files = 3
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        g.run_graph()
        got_e, got_c, want_e, want_c = take(g, n_files, len(reads))
        assert (len(got_e), len(got_c)) == want_counts
        assert same(got_e, want_e) and same(got_c, want_c)
        for kind, count, fetch, write, want in (("e", len(got_e), g.fetch_edge_records, g.write_edge_records, want_e),
                                                ("c", len(got_c), g.fetch_contained_records, g.write_contained_records, want_c)):
            for piece in sorted({1, 7, 64, count - 1, count, 0} - {-1}):  # (0: the default — a half of the ring; count - 1 of one record is that too)
                assert _written(write, count, piece, str(tmp_path / f"{kind}{piece}.bin"), g) == want.tobytes(), (kind, piece)
                g.set_record_piece(piece)
                assert same(fetch(count), want), (kind, piece)
                g.set_record_piece(0)


# ---- field widths and files: the 30 000 reads of tests/test_gpu_text.py ------------------------------------------------------------
SPEC = readgen.GenSpec.coverage(seed=41, n_reads=30_000, read_len=90, cov=25.0, n_contigs=9, len_max=300)


@pytest.fixture(scope="module")
def graph():
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(SPEC)
        g.run_graph()
        yield g


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("n_files", [1, 5, 300])
def test_records_with_wide_ids_and_many_files(graph, n_files, mapped, tmp_path):
    g = graph
    # file indices as the input stage assigns them when records are filtered: increasing, with gaps, beyond 2^32 — the 64-bit fields
    fidx = np.arange(SPEC.n_reads, dtype=np.uint64) * np.uint64(3) + np.uint64(9_999_999_990) if mapped else None
    got_e, got_c, want_e, want_c = take(g, n_files, SPEC.n_reads, fidx)
    assert len(got_e) > 4099 and len(got_c) > 0   # (more edges than the piece used below)
    assert same(got_e, want_e) and same(got_c, want_c)
    if mapped:
        assert int(got_e["src"].min()) > 1 << 32 and int(got_c["super"].min()) > 1 << 32
    if n_files > 1:
        assert len(np.unique(got_e["file"])) > 1 and len(np.unique(got_c["file"])) > 1 and int(got_e["file"].max()) < n_files
    # several pieces of an odd size, each split among the writer threads
    assert _written(g.write_edge_records, len(got_e), 4099, str(tmp_path / "e.bin"), g) == want_e.tobytes()
    assert _written(g.write_contained_records, len(got_c), 4099, str(tmp_path / "c.bin"), g) == want_c.tobytes()


def test_record_calls_out_of_place(graph):
    with pytest.raises(buildgraph.DiscoError):
        graph.prepare_edge_records(4)                     # several files need the file of every edge
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(readgen.GenSpec.coverage(seed=42, n_reads=3000, read_len=100, cov=20.0))
        with pytest.raises(buildgraph.DiscoError):
            g.prepare_edge_records(1)                     # no graph yet
        with pytest.raises(buildgraph.DiscoError):
            g.prepare_contained_records(1)
        g.build_index()
        g.probe()
        n_cont = g.mark_contained()
        assert g.prepare_contained_records(2) == n_cont   # from disco_mark_contained on: no edges needed
        with pytest.raises(buildgraph.DiscoError):
            g.prepare_edge_records(1)
        with pytest.raises(buildgraph.DiscoError):
            g.fetch_edge_records(0)                       # nothing prepared
    gs = [buildgraph.BuildGraph(min_overlap=40) for _ in range(2)]
    try:
        buildgraph.BuildGraph.comm_init_local(gs)
        for call in (gs[0].prepare_edge_records, gs[0].prepare_contained_records):
            with pytest.raises(buildgraph.DiscoError):
                call(1)                                   # single GPU only
    finally:
        for g in gs:
            g.close()


def test_records_of_an_emission_with_unused_tails(monkeypatch):
    """DISCO_NO_HALF=1: the emission leaves chunks with unused tails (out_valid / out_pos): the records go through the compaction of
    disco_fetch_edges, so that slot i is edge i"""
    monkeypatch.setenv("DISCO_NO_HALF", "1")
    spec = readgen.GenSpec.coverage(seed=77, n_reads=20_000, read_len=150, cov=30.0, n_contigs=5)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        _lens, dense, used = g.fetch_survivor_layout(lengths=False)
        got_e, got_c, want_e, want_c = take(g, 4, spec.n_reads)
    assert not dense and used > len(got_e) > 10_000
    assert same(got_e, want_e) and same(got_c, want_c)


# ---- inexact overlaps: the substitutions field -------------------------------------------------------------------------------------
def test_records_carry_the_substitutions_of_inexact_overlaps():
    codes, off = _mutated(103, 3000, 100, 250, 30.0, 0.006)
    reads = readgen.codes_to_reads(codes, off)
    with buildgraph.BuildGraph(min_overlap=40, max_substitutions=2) as g:
        g.upload_ascii(reads)
        g.run_graph()
        subs = g.fetch_edge_substitutions()
        got_e, got_c, want_e, want_c = take(g, 3, len(reads), subs=True)
    assert np.array_equal(got_e["substitutions"], subs) and subs.max() > 0 and int(subs.max()) <= 2
    assert same(got_e, want_e) and same(got_c, want_c)


# ---- two classes of rows: lengths above 256 ----------------------------------------------------------------------------------------
def test_records_of_a_table_with_two_classes_of_rows():
    reads = mixed_reads(2, 6000, 100, 250, 30.0, 0.05, 257, 1000)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        g.run_graph()
        assert g.long_rows == sum(len(r) > 256 for r in reads) > 0
        got_e, got_c, want_e, want_c = take(g, 2, len(reads))
    assert same(got_e, want_e) and same(got_c, want_c)
    assert (got_e["len_src"] > 256).any() and (got_e["len_dst"] > 256).any() and (got_c["len1"] > 256).any()


# ---- every sort tier ----------------------------------------------------------------------------------------------------------------
def test_contained_records_of_groups_of_every_tier_equal_the_text():
    """groups of 2 ... 9000 rows with ties on (containing read, j): the records are the lines disco_format_contained gives for the same
    context (tests/test_gpu_contained_text.py holds that text to the oracle), parsed back"""
    c = BIG_CASES["one_class"]
    reads = big_group_reads(c["L"], c["l"], c["sizes"])
    with buildgraph.BuildGraph(min_overlap=c["min_overlap"]) as g:
        g.upload_ascii(reads)
        g.run_graph()
        text, off = g.format_contained(3)
        got = g.fetch_contained_records(g.prepare_contained_records(3))
    assert len(got) == c["n_rows"]
    want = np.zeros(c["n_rows"], dtype=CONTAINED)
    i = 0
    for t in range(3):
        for line in text[int(off[t]):int(off[t + 1])].decode().splitlines():
            a, b, info = line.split("\t")
            p = [int(x) for x in info.split(",")]  # orient, len2, 0, 0, len2, 0, len2, len1, start, start + len2
            want[i] = (int(a), int(b), p[0], p[1], p[7], p[8], t, 0, 0)
            i += 1
    assert i == c["n_rows"] and same(got, want)


# ---- reuse --------------------------------------------------------------------------------------------------------------------------
def test_a_second_pass_on_the_context_invalidates_and_replaces_the_records():
    first, second = tiled_reads(66, 64), tiled_reads(130, 1, seed=9)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(first)
        g.run_graph()
        got_e1, got_c1, want_e1, want_c1 = take(g, 2, len(first))
        g.upload_ascii(second)
        g.run_graph()
        with pytest.raises(buildgraph.DiscoError):
            g.fetch_edge_records(len(got_e1))             # what was prepared belonged to the first graph
        with pytest.raises(buildgraph.DiscoError):
            g.fetch_contained_records(len(got_c1))
        got_e2, got_c2, want_e2, want_c2 = take(g, 2, len(second))
    assert same(got_e1, want_e1) and same(got_c1, want_c1) and (len(got_e1), len(got_c1)) == (65, 64)
    assert same(got_e2, want_e2) and same(got_c2, want_c2) and (len(got_e2), len(got_c2)) == (129, 1)
