"""-m gpu : disco_dist_format_contained / disco_dist_format_edges through the C-ABI — every rank of a multi-GPU job formats the text of the
files it owns (file f of F belongs to rank f * G // F) on its own device. G ranks = G host threads of this process over the in-process
communicator, as tests/dist_util.py runs them; the contexts stay open here, because the text is read off them after the pass."""
import os
import threading

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from oracle import pyoracle
from tests.test_gpu_contained_text import BIG_CASES, _lines, _per_file, big_group_reads

pytestmark = pytest.mark.gpu

COV = readgen.GenSpec.coverage(seed=42, n_reads=3000, read_len=100, cov=20.0)
COV_MO = 40


class Ranks:
    """G contexts that have run one pass over the reads setup(g) gave them; each(fn) runs fn(rank, context) on a thread per rank
    (collective calls allowed) and returns the results by rank"""

    def __init__(self, G, min_overlap, setup):
        self.G = G
        self.gs = [buildgraph.BuildGraph(min_overlap=min_overlap) for _ in range(G)]
        try:
            buildgraph.BuildGraph.comm_init_local(self.gs)

            def first(r, g):
                setup(g)
                g.dist_run_graph()
                return g.fetch_edges(), g.fetch_contained(), g.dist_info()

            self.first = self.each(first)
        except BaseException:
            self.close()
            raise
        self.e_out = self.first[0][2]["e_out"]
        self.n_contained = self.first[0][2]["n_contained"]

    def each(self, fn):
        out, errors = [None] * self.G, []

        def work(r):
            try:
                out[r] = fn(r, self.gs[r])
            except Exception as e:  # pragma: no cover
                errors.append((r, repr(e)))

        th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(self.G)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errors, errors
        assert not any(t.is_alive() for t in th), "a rank did not finish"
        return out

    def close(self):
        for g in self.gs:
            g.close()


def owner(t, G, F):
    return t * G // F


def union_per_file(per_rank, G, F):
    """per_rank[r] = (text, offsets) of rank r. Every file has text on its owner only and equal offsets elsewhere; returns the files' texts"""
    files = []
    for t in range(F):
        for r, (text, off) in enumerate(per_rank):
            assert len(off) == F + 1 and off[0] == 0 and int(off[-1]) == len(text) and np.all(np.diff(off.astype(np.int64)) >= 0)
            if r != owner(t, G, F):
                assert off[t] == off[t + 1], (t, r)
        text, off = per_rank[owner(t, G, F)]
        files.append(text[int(off[t]):int(off[t + 1])])
    return files


def _mapped(n):
    # file indices as the input stage assigns them when records are filtered: increasing, with gaps, up to 11 digits
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(9_999_999_990)


# ---- 1. contained lines against the oracle, every sort tier ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """the read set with groups of 2 ... 9000 rows and ties on (containing read, j), and the oracle's lines for it: computed once"""
    c = BIG_CASES["one_class"]
    reads = big_group_reads(c["L"], c["l"], c["sizes"])
    codes, off = pyoracle.encode_reads(reads)
    orows, oedges, _ = pyoracle.build_graph(codes, off, c["min_overlap"])
    assert len(reads) == c["n_reads"] and len(orows) == c["n_rows"] and len(oedges) == 0
    srows, lines = _lines(orows, np.arange(len(reads), dtype=np.uint64) + np.uint64(1))
    return reads, c["min_overlap"], srows, lines


@pytest.fixture(scope="module", params=[1, 2, 3, 4])
def big_ranks(request, big):
    reads, mo = big[0], big[1]
    rk = Ranks(request.param, mo, lambda g: g.dist_upload_ascii(reads))
    yield rk
    rk.close()


@pytest.mark.parametrize("n_files", [3, 5])
def test_contained_lines_of_every_tier_equal_the_oracles(big, big_ranks, n_files):
    """groups for the insertion sort, the LDS tier and the tier through global memory, contained reads that arrived on every rank: the
    union of the ranks' texts is the oracle's files byte for byte, order included, and a file has text on its owner only"""
    reads, _, srows, lines = big
    rk = big_ranks
    assert rk.n_contained == BIG_CASES["one_class"]["n_rows"]
    per_rank = rk.each(lambda r, g: g.dist_format_contained(n_files))
    files = union_per_file(per_rank, rk.G, n_files)
    want = _per_file(srows, lines, n_files, len(reads))
    assert files == want
    assert sum(f.count(b"\n") for f in files) == BIG_CASES["one_class"]["n_rows"] and len(files[0]) > 0


# ---- 2. edge lines ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single():
    """the coverage set on one context without a communicator: the reference for the edge lines and for the contained lines"""
    with buildgraph.BuildGraph(min_overlap=COV_MO) as g:
        g.generate_reads(COV)
        g.run_graph()
        cache = {}

        def edge_lines(n_files, mapped):
            if (n_files, mapped) not in cache:
                files = g.fetch_edge_files(n_files)
                text, off = g.format_edges(n_files, files if n_files > 1 else None, _mapped(COV.n_reads) if mapped else None)
                cache[(n_files, mapped)] = [sorted(text[int(off[t]):int(off[t + 1])].splitlines()) for t in range(n_files)]
            return cache[(n_files, mapped)]

        def contained(n_files, mapped=False):
            text, off = g.format_contained(n_files, _mapped(COV.n_reads) if mapped else None)
            return [text[int(off[t]):int(off[t + 1])] for t in range(n_files)]

        n_edges = len(g.fetch_edges())
        assert n_edges > 1000
        yield edge_lines, contained, n_edges


@pytest.fixture(scope="module", params=[2, 3, 4])
def cov_ranks(request):
    rk = Ranks(request.param, COV_MO, lambda g: g.dist_generate_reads(COV))
    yield rk
    rk.close()


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("n_files", [1, 2, 7])
def test_edge_lines_equal_the_single_context_files(single, cov_ranks, n_files, mapped):
    """every rank cuts the same files out of the gathered edges: file by file the lines of the single-context partition (sorted: the
    order inside a file follows the emission), every edge in exactly one file; with fewer files than ranks some ranks own nothing"""
    edge_lines, _, n_edges = single
    rk = cov_ranks
    assert rk.e_out == n_edges
    fidx = _mapped(COV.n_reads) if mapped else None
    per_rank = rk.each(lambda r, g: g.dist_format_edges(n_files, fidx))
    files = union_per_file(per_rank, rk.G, n_files)
    got = [sorted(f.splitlines()) for f in files]
    assert got == edge_lines(n_files, mapped)
    every = [l for f in got for l in f]
    assert len(every) == rk.e_out == len(set(every))
    if n_files < rk.G:
        assert any(len(text) == 0 for text, _ in per_rank)


# ---- 3. edge cases ---------------------------------------------------------------------------------------------------------------------
def _single_files(reads, mo, n_files):
    with buildgraph.BuildGraph(min_overlap=mo) as g:
        g.upload_ascii(reads)
        g.run_graph()
        ctext, coff = g.format_contained(n_files)
        files = g.fetch_edge_files(n_files)
        etext, eoff = g.format_edges(n_files, files if n_files > 1 else None, None)
    return ([ctext[int(coff[t]):int(coff[t + 1])] for t in range(n_files)], [sorted(etext[int(eoff[t]):int(eoff[t + 1])].splitlines()) for t in range(n_files)])


def _dist_files(reads, mo, G, n_files):
    rk = Ranks(G, mo, lambda g: g.dist_upload_ascii(reads))
    try:
        c = rk.each(lambda r, g: g.dist_format_contained(n_files))
        e = rk.each(lambda r, g: g.dist_format_edges(n_files))
        homes = [i["own_hi"] - i["own_lo"] for _, _, i in rk.first]
    finally:
        rk.close()
    return union_per_file(c, G, n_files), [sorted(f.splitlines()) for f in union_per_file(e, G, n_files)], c, e, homes


def test_nothing_contained_and_no_edges_give_empty_files(tmp_path):
    rng = np.random.default_rng(7)
    reads = ["".join("ACGT"[x] for x in rng.integers(0, 4, 100)) for _ in range(50)]
    rk = Ranks(3, 40, lambda g: g.dist_upload_ascii(reads))
    try:
        assert rk.e_out == 0 and rk.n_contained == 0

        def work(r, g):
            ctext, coff = g.dist_format_contained(3)
            etext, eoff = g.dist_format_edges(3)
            paths = [str(tmp_path / f"{k}{r}_{t}.txt") for k in "ce" for t in range(3)]
            fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in paths]
            g.write_contained_text(fds[:3])
            g.write_edge_text(fds[3:])
            for fd in fds:
                os.close(fd)
            return ctext, list(coff), etext, list(eoff), [os.path.getsize(p) for p in paths]

        for ctext, coff, etext, eoff, sizes in rk.each(work):
            assert ctext == b"" and etext == b"" and coff == [0] * 4 and eoff == [0] * 4 and sizes == [0] * 6
    finally:
        rk.close()


def test_ranks_with_an_empty_home_range():
    """100 reads on 4 ranks: the ranges are cut at multiples of 64 reads, so two ranks hold no read — and still own files"""
    reads = readgen.generate_reads(readgen.GenSpec.coverage(seed=11, n_reads=100, read_len=100, cov=20.0, len_max=160))
    want_c, want_e = _single_files(reads, 40, 4)
    got_c, got_e, _, _, homes = _dist_files(reads, 40, 4, 4)
    assert homes.count(0) >= 1
    assert got_c == want_c and got_e == want_e
    assert sum(len(f) for f in want_c) > 0 and sum(len(f) for f in want_e) > 0


def test_containers_and_their_substrings_on_different_ranks():
    """384 reads on 3 ranks of 128: the containing reads arrive in the first home range, their substrings in the last — every key
    crossed ranks in the pass's reduction, and the rank that writes a container's file received none of its contained reads itself"""
    rng = np.random.default_rng(23)
    comp = str.maketrans("ACGT", "TGCA")
    rnd = lambda m: "".join("ACGT"[x] for x in rng.integers(0, 4, m))
    cont = [rnd(220) for _ in range(40)]
    first = cont + [rnd(120) for _ in range(128 - len(cont))]
    rng.shuffle(first)
    middle = [rnd(120) for _ in range(128)]
    last = []
    for i in range(128):
        c = cont[i % len(cont)]
        o = int(rng.integers(0, 220 - 70 + 1))
        s = c[o:o + 70]
        last.append(s.translate(comp)[::-1] if i & 1 else s)
    reads = first + middle + last
    want_c, want_e = _single_files(reads, 30, 5)
    got_c, got_e, per_rank, _, homes = _dist_files(reads, 30, 3, 5)
    assert homes == [128, 128, 128]
    assert got_c == want_c and got_e == want_e
    assert sum(f.count(b"\n") for f in got_c) == 128
    assert len(per_rank[0][0]) > 0 and len(per_rank[2][0]) == 0   # the containers' files: ranks 0 and 1 (files 0-1 and 2-3); none in the last range


@pytest.mark.parametrize("G", [2, 3])
def test_more_components_by_size_than_64_per_file_under_ranks(G):
    """300 disjoint pairs of reads that overlap by 60 bases into 3 files: 300 components of one edge, thr = 1, all of them dealt out by
    size — more than 64 * 3 + 64. Every rank cuts the gathered edges on its own device and writes its files only: the ranks must agree, with
    each other, with a single context, and with the rule (tests/partition_model.py)"""
    from tests.partition_model import SHARE, partition_model

    rng = np.random.default_rng(300)
    reads = []
    for _ in range(300):
        x = "".join("ACGT"[b] for b in rng.integers(0, 4, 140))
        reads += [x[0:100], x[40:140]]
    n_files = 3
    want_c, want_e = _single_files(reads, 40, n_files)
    got_c, got_e, _, _, _ = _dist_files(reads, 40, G, n_files)
    assert all(len(f) == 0 for f in want_c)                  # nothing contained
    every = [l for f in got_e for l in f]
    assert len(every) == 300 == len(set(every))              # every edge line exactly once
    assert got_e == want_e and got_c == want_c
    ends = [np.array([[int(x) - 1 for x in l.split(b"\t")[:2]] for l in f], dtype=np.int64).reshape(-1, 2) for f in want_e]
    src, dst = np.concatenate([a[:, 0] for a in ends]), np.concatenate([a[:, 1] for a in ends])
    assert sorted(zip(np.minimum(src, dst).tolist(), np.maximum(src, dst).tolist())) == [(2 * k, 2 * k + 1) for k in range(300)]
    model, info = partition_model(src, dst, len(reads), n_files)
    assert info["thr"] == 1 and SHARE * n_files + SHARE < info["n_big"] == 300 < 2 * SHARE * n_files
    assert np.array_equal(model, np.repeat(np.arange(n_files), [len(a) for a in ends]))   # the single-context files are the model's


# ---- 4. streaming, 5. a second pass ----------------------------------------------------------------------------------------------------
def test_texts_streamed_into_files_and_a_second_pass(single, cov_ranks, tmp_path):
    """every rank writes its files through the pinned ring: rank after rank they are the fetched texts, and the single-context files. The
    in-place gather of the keys and the gathered edges disturbed nothing: a second pass on the same contexts gives the same edges and rows"""
    edge_lines, contained, _ = single
    rk = cov_ranks
    FC, FE = 5, 7

    def work(r, g):
        ctext, coff = g.dist_format_contained(FC)
        etext, eoff = g.dist_format_edges(FE)
        cp = [str(tmp_path / f"c{r}_{t}.txt") for t in range(FC)]
        ep = [str(tmp_path / f"e{r}_{t}.txt") for t in range(FE)]
        cf = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in cp]
        ef = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in ep]
        g.write_edge_text(ef, threads=3)
        g.write_contained_text(cf, threads=3)
        for fd in cf + ef:
            os.close(fd)
        g.dist_run_graph()
        return (ctext, coff), (etext, eoff), [open(p, "rb").read() for p in cp], [open(p, "rb").read() for p in ep], g.fetch_edges(), g.fetch_contained()

    res = rk.each(work)
    cfiles = union_per_file([x[0] for x in res], rk.G, FC)
    efiles = union_per_file([x[1] for x in res], rk.G, FE)
    assert cfiles == contained(FC) and sum(len(f) for f in cfiles) > 1000
    assert [sorted(f.splitlines()) for f in efiles] == edge_lines(FE, False)
    for t in range(FC):
        assert b"".join(x[2][t] for x in res) == cfiles[t], t
    for t in range(FE):
        assert b"".join(x[3][t] for x in res) == efiles[t], t
    for r in range(rk.G):   # the second pass: this rank's edges (as a set: the emission's order varies) and its rows
        e1, c1, _ = rk.first[r]
        e2, c2 = res[r][4], res[r][5]
        assert sorted(e1.tolist()) == sorted(e2.tolist()) and len(e1) > 0
        assert c1.tolist() == c2.tolist()


def test_contained_lines_with_mapped_file_indices(single, cov_ranks):
    _, contained, _ = single
    rk = cov_ranks
    fidx = _mapped(COV.n_reads)
    files = union_per_file(rk.each(lambda r, g: g.dist_format_contained(7, fidx)), rk.G, 7)
    assert files == contained(7, True)
    assert sum(1 for f in files if f) >= 5   # containing reads all over the id range: ranks other than the first write text too


# ---- 6. the transport without host waits -----------------------------------------------------------------------------------------------
def test_both_texts_over_the_transport_without_host_waits(single, big, monkeypatch):
    """DISCO_LOOP_ASYNC=1: an exchange only orders streams, as RCCL does — whoever reads a gathered buffer without a stream dependency reads
    garbage here"""
    monkeypatch.setenv("DISCO_LOOP_ASYNC", "1")
    edge_lines, contained, _ = single
    rk = Ranks(3, COV_MO, lambda g: g.dist_generate_reads(COV))
    try:
        c = rk.each(lambda r, g: g.dist_format_contained(5))
        e = rk.each(lambda r, g: g.dist_format_edges(7))
    finally:
        rk.close()
    assert union_per_file(c, 3, 5) == contained(5)
    assert [sorted(f.splitlines()) for f in union_per_file(e, 3, 7)] == edge_lines(7, False)
    reads, mo, srows, lines = big
    rk = Ranks(3, mo, lambda g: g.dist_upload_ascii(reads))
    try:
        c = rk.each(lambda r, g: g.dist_format_contained(3))
    finally:
        rk.close()
    assert union_per_file(c, 3, 3) == _per_file(srows, lines, 3, len(reads))


def test_the_collective_entry_points_need_a_communicator_and_a_pass():
    with buildgraph.BuildGraph(min_overlap=COV_MO) as g:
        g.generate_reads(COV)
        g.run_graph()
        with pytest.raises(buildgraph.DiscoError):
            g.dist_format_contained(2)
        with pytest.raises(buildgraph.DiscoError):
            g.dist_format_edges(2)
