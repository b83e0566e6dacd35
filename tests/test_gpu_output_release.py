"""-m gpu : every output entry point gives back the device memory it took for itself. Called twice, a call leaves hbm_bytes where the
first call left it and produces the same bytes; a call that fails on the host in the middle (a descriptor opened read-only: pwrite
fails, "write error") leaves hbm_bytes where the call before it did, and the call after it writes the first call's file. Two ranks over
the in-process transport: the collective formatters called twice, and the passes after them still allocate nothing from the runtime."""
import os

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.test_gpu_dist_text import COV, COV_MO, Ranks

pytestmark = pytest.mark.gpu

N_FILES = 3
PIECE_BYTES = 65536


def _hbm(g):
    return g.counters()["hbm_bytes"]


def _fidx(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(9_999_999_990)


def _graph(max_substitutions):
    """the 3 000-read set of tests/test_gpu_gfa.py (edges and contained rows), one pass; about 1 000 records a piece"""
    spec = readgen.GenSpec.coverage(seed=71, n_reads=3000, read_len=100, cov=20.0)
    g = buildgraph.BuildGraph(min_overlap=40, max_substitutions=max_substitutions)
    g.generate_reads(spec)
    if max_substitutions:
        g.substitute_bases(9, 5000)
    g.run_graph()
    g.set_record_piece(1000)
    return g


@pytest.fixture(scope="module")
def exact():
    g = _graph(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def inexact():
    g = _graph(2)
    yield g
    g.close()


def _into_files(tmp_path, name, n, write, flags=os.O_WRONLY):
    """write(fds) into n fresh files opened with `flags`; their bytes"""
    paths = [str(tmp_path / f"{name}{t}") for t in range(n)]
    for p in paths:
        open(p, "wb").close()
    fds = [os.open(p, flags) for p in paths]
    try:
        write(fds)
    finally:
        for fd in fds:
            os.close(fd)
    return [open(p, "rb").read() for p in paths]


def _description(g, n_files):
    """a ParSimpleEdges description of the contraction as it stands: every composite edge one forward piece, every residue edge inline"""
    comp, _links, _absorbed = g.contract_chains(0)
    res_index, res_edges = g.chain_residue()
    first_edge = g.chain_first_edges(len(comp))
    g.chain_end_links(len(comp))
    ef = g.fetch_edge_files(n_files).astype(np.int64)
    recs = [(int(ef[int(first_edge[k])]), int(c["a"]), int(c["b"]), int(c["offset"]), int(c["orient"]), (1, k, 0, 0)) for k, c in enumerate(comp)]
    recs += [(int(ef[int(i)]), int(e["src"]), int(e["dst"]), int(e["offset"]), int(e["orient"]), (0, int(e["dst"]), int(e["offset"]), int(e["orient"])))
             for i, e in zip(res_index, res_edges)]
    recs.sort(key=lambda r: r[:5])
    edges = np.zeros(len(recs), dtype=buildgraph.PS_EDGE_DTYPE)
    pieces = np.zeros(len(recs), dtype=buildgraph.PS_PIECE_DTYPE)
    for i, (f, s, d, off, o, p) in enumerate(recs):
        edges[i] = (s, d, off, o, f, i, 1, 0)
        pieces[i] = p
    assert len(comp) > 0
    return edges, pieces


# ---- the entry points: name -> fn(g, tmp_path) -> what it produced, as something == compares ---------------------------------------------
def _edge_text(g, tmp_path):
    files = g.fetch_edge_files(N_FILES)
    text, off = g.format_edges(N_FILES, files, _fidx(g.num_reads))
    assert len(text) > 0
    return text, off.tolist(), _into_files(tmp_path, "e", N_FILES, g.write_edge_text)


def _contained_text(g, tmp_path):
    text, off = g.format_contained(N_FILES, _fidx(g.num_reads))
    assert len(text) > 0
    return text, off.tolist(), _into_files(tmp_path, "c", N_FILES, g.write_contained_text)


def _par_simple_text(g, tmp_path):
    edges, pieces = _description(g, N_FILES)
    off = g.format_par_simple(edges, pieces, N_FILES, _fidx(g.num_reads))
    text = g.fetch_par_simple_text(int(off[-1]))
    assert len(text) > 0
    return text, off.tolist(), _into_files(tmp_path, "p", N_FILES, g.write_par_simple_text)


def _edge_records(g, tmp_path):
    n = g.prepare_edge_records(N_FILES, g.fetch_edge_files(N_FILES), _fidx(g.num_reads))
    assert n > 2000   # three pieces of 1 000 records
    rec = g.fetch_edge_records(n)
    return rec.tobytes(), _into_files(tmp_path, "er", 1, lambda fds: g.write_edge_records(fds[0]))


def _contained_records(g, tmp_path):
    n = g.prepare_contained_records(N_FILES, _fidx(g.num_reads))
    assert n > 0
    rec = g.fetch_contained_records(n)
    return rec.tobytes(), _into_files(tmp_path, "cr", 1, lambda fds: g.write_contained_records(fds[0]))


def _edge_files(g, tmp_path):
    return g.fetch_edge_files(N_FILES).tobytes()


def _partition(g, tmp_path):
    return g.partition_edges(g.fetch_edges(), g.num_reads, N_FILES).tobytes()


def _substitutions(g, tmp_path):
    return g.fetch_edge_substitutions().tobytes()


def _contained_grouped(g, tmp_path):
    rows = g.fetch_contained_grouped()
    return None if rows is None else rows.tobytes()


def _gfa(g, tmp_path):
    out = _into_files(tmp_path, "g", 1, lambda fds: g.write_gfa(fds[0], file_index=_fidx(g.num_reads), piece_bytes=PIECE_BYTES, threads=3))
    assert len(out[0]) > 4 * PIECE_BYTES   # several pieces
    return out


def _chains(g, tmp_path):
    comp, links, absorbed = g.contract_chains(0)
    idx, rec = g.chain_residue()
    first = g.chain_first_edges(len(comp))
    end_first, end_last = g.chain_end_links(len(comp))
    assert len(comp) > 0
    return [x.tobytes() for x in (comp, links, absorbed, idx, rec, first, end_first, end_last)]


def _gfa_chains(g, tmp_path):
    g.contract_chains(0)
    out = _into_files(tmp_path, "u", 1, lambda fds: g.write_gfa_chains(fds[0], file_index=_fidx(g.num_reads), piece_bytes=PIECE_BYTES, threads=3))
    assert out[0].count(b"\nS\tc") > 0 and out[0].count(b"\nL\t") > 0   # (one contig: a small file, a piece for each of its sections)
    return out


EXACT = {"edge_text": _edge_text, "contained_text": _contained_text, "par_simple_text": _par_simple_text, "edge_records": _edge_records,
         "contained_records": _contained_records, "edge_files": _edge_files, "partition_edges": _partition, "edge_substitutions": _substitutions,
         "contained_grouped": _contained_grouped, "gfa": _gfa, "chains": _chains, "gfa_chains": _gfa_chains}
# max_substitutions = 2: the substitution counts exist as buffers (the edge text and the chains' GFA are the host writer's then)
INEXACT = {k: EXACT[k] for k in ("edge_substitutions", "edge_records", "gfa", "contained_text", "edge_files")}


def _twice(g, fn, tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    first = fn(g, tmp_path / "a")
    h1 = _hbm(g)
    second = fn(g, tmp_path / "b")
    h2 = _hbm(g)
    print(f"hbm_bytes after the first call {h1}, after the second {h2}")
    assert h2 == h1
    assert second == first


@pytest.mark.parametrize("name", list(EXACT))
def test_second_call_leaves_hbm_bytes_and_the_output_alone(exact, tmp_path, name):
    _twice(exact, EXACT[name], tmp_path)


@pytest.mark.parametrize("name", list(INEXACT))
def test_second_call_leaves_hbm_bytes_and_the_output_alone_with_substitutions(inexact, tmp_path, name):
    if name == "edge_substitutions":
        assert 0 < int(inexact.fetch_edge_substitutions().max()) <= 2
    _twice(inexact, INEXACT[name], tmp_path)


# ---- succeed, fail on the host, succeed --------------------------------------------------------------------------------------------------
def _w_gfa(g):
    return 1, lambda fds: g.write_gfa(fds[0], piece_bytes=PIECE_BYTES, threads=3)


def _w_gfa_chains(g):
    g.contract_chains(0)
    return 1, lambda fds: g.write_gfa_chains(fds[0], piece_bytes=PIECE_BYTES, threads=3)


def _w_edge_records(g):
    g.prepare_edge_records(N_FILES, g.fetch_edge_files(N_FILES), None)
    return 1, lambda fds: g.write_edge_records(fds[0])


def _w_edge_text(g):
    g.format_edges(N_FILES, g.fetch_edge_files(N_FILES), None)
    return N_FILES, g.write_edge_text


def _w_contained_text(g):
    g.format_contained(N_FILES)
    return N_FILES, g.write_contained_text


def _w_par_simple_text(g):
    edges, pieces = _description(g, N_FILES)
    g.format_par_simple(edges, pieces, N_FILES)
    return N_FILES, g.write_par_simple_text


WRITERS = {"write_gfa": _w_gfa, "write_gfa_chains": _w_gfa_chains, "write_edge_records": _w_edge_records, "write_edge_text": _w_edge_text,
           "write_contained_text": _w_contained_text, "write_par_simple_text": _w_par_simple_text}


@pytest.mark.parametrize("name", list(WRITERS))
def test_a_write_error_in_the_middle_leaks_nothing(exact, tmp_path, name):
    g = exact
    n, write = WRITERS[name](g)
    first = _into_files(tmp_path, "first", n, write)
    h1 = _hbm(g)
    with pytest.raises(buildgraph.DiscoError, match="write error"):
        _into_files(tmp_path, "refused", n, write, flags=os.O_RDONLY)
    h2 = _hbm(g)
    third = _into_files(tmp_path, "third", n, write)
    h3 = _hbm(g)
    print(f"hbm_bytes after the first call {h1}, after the failed one {h2}, after the third {h3}")
    assert h3 == h1
    assert third == first and sum(len(x) for x in first) > 0


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------------
def test_collective_formatters_twice_and_the_passes_after_them_allocate_nothing():
    rk = Ranks(2, COV_MO, lambda g: g.dist_generate_reads(COV))
    try:
        def work(r, g):
            e1 = g.dist_format_edges(N_FILES)
            he1 = _hbm(g)
            e2 = g.dist_format_edges(N_FILES)
            he2 = _hbm(g)
            c1 = g.dist_format_contained(N_FILES)
            hc1 = _hbm(g)
            c2 = g.dist_format_contained(N_FILES)
            hc2 = _hbm(g)
            g.dist_run_graph()
            g.dist_run_graph()   # the third pass of the context: warm, as tests/test_gpu_dist.py asserts it
            return (e1[0], e1[1].tolist()), (e2[0], e2[1].tolist()), (c1[0], c1[1].tolist()), (c2[0], c2[1].tolist()), (he1, he2, hc1, hc2), g.dist_info()

        res = rk.each(work)
    finally:
        rk.close()
    for e1, e2, c1, c2, (he1, he2, hc1, hc2), info in res:
        print(f"hbm_bytes: edges {he1} {he2}, contained {hc1} {hc2}; device_allocs {info['device_allocs']}, device_frees {info['device_frees']}")
        assert e2 == e1 and c2 == c1
        assert he2 == he1 and hc2 == hc1
        assert info["device_allocs"] == 0 and info["device_frees"] == 0, info
    assert sum(len(x[0][0]) for x in res) > 0 and sum(len(x[2][0]) for x in res) > 0
