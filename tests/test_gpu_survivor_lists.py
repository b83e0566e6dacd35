"""-m gpu : the self-delimiting survivor lists of the marking and the dense output of the emission (the whole-table pass of one GPU;
disco_amd/csrc/disco_survivor.h, emit_half_lists_kernel). Yardsticks: the oracle, and the row path (DISCO_NO_HALF=1: no lists, chunked
output, validity pass and scan) in the same process. The layout is looked at through disco_fetch_survivor_layout."""
import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.util import assert_parity, canon_hip, run_oracle_reads

pytestmark = pytest.mark.gpu
_COMP = str.maketrans("ACGT", "TGCA")
WIDE = 5


def _rc(s):
    return s.translate(_COMP)[::-1]


def _seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def sampled_reads(seed, n, read_len=150, cov=30.0):
    """n reads of read_len bases at cov-fold coverage of one random genome, either strand"""
    rng = np.random.default_rng(seed)
    genome = _seq(rng, max(read_len, int(n * read_len / cov)))
    out = []
    for _ in range(n):
        p = int(rng.integers(0, len(genome) - read_len + 1))
        s = genome[p:p + read_len]
        out.append(_rc(s) if rng.random() < 0.5 else s)
    return out


def branching_reads(seed, fans=(2, 3, 4, 6), read_len=150, shared=140, arm=200):
    """per fan C: C contigs prefix_i + SHARED + suffix_i (SHARED shorter than a read, so every read belongs to one contig), reads tiled at
    every offset on both strands. The read that ends where SHARED ends keeps its own continuation, the first read inside SHARED of every
    other contig, and its predecessor: C + 1 survivors of its own marking (and so does, mirrored, the first read inside SHARED). Reads at
    a contig's end keep one, reads in between two."""
    rng = np.random.default_rng(seed)
    reads = []
    for c in fans:
        mid = _seq(rng, shared)
        for _ in range(c):
            contig = _seq(rng, arm) + mid + _seq(rng, arm)
            for p in range(len(contig) - read_len + 1):
                s = contig[p:p + read_len]
                reads += [s, _rc(s)]
    order = rng.permutation(len(reads))  # (ids carry no structure)
    return [reads[int(i)] for i in order]


def _parity_on(g, reads, min_overlap, label):
    """assert_parity on a context that has seen other reads before"""
    g.upload_ascii(reads)
    g.run_graph()
    he, hr, hc = g.fetch_edges(), g.fetch_contained(), g.counters()
    oe, orows, oc = run_oracle_reads(reads, min_overlap)
    ce, cc = canon_hip(he, hr)
    oce, occ = canon_hip(oe, orows)
    assert np.array_equal(cc, occ), f"{label}: contained rows differ ({len(cc)} vs {len(occ)})"
    assert np.array_equal(ce, oce), f"{label}: edge list differs ({len(ce)} vs {len(oce)})"
    for key in ("probes", "kmer_hits", "n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs"):
        assert hc[key] == oc[key], f"{label}: counter {key}: hip {hc[key]} oracle {oc[key]}"
    return hc


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_sizes_around_the_work_item_of_64_nodes(n):
    assert_parity(sampled_reads(300 + n, n), 40, f"{n} reads")


def test_every_list_length():
    reads = branching_reads(7)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        hc = _parity_on(g, reads, 40, "branching contigs")
        lens, dense, used = g.fetch_survivor_layout()
    assert dense and used == hc["e_out"] > 0
    hist = {int(k): int(v) for k, v in zip(*np.unique(lens, return_counts=True))}
    print(f"survivor list lengths (5 = wide, 255 = no row): {hist}; a node with rows and no survivor occurred: {0 in hist}")
    for want in (1, 2, 3, 4, WIDE):
        assert hist.get(want, 0) > 0, (want, hist)
    assert set(hist) <= {0, 1, 2, 3, 4, WIDE, 255}


def test_stale_lists_of_an_earlier_pass_are_not_read():
    """the lists persist across passes: the second read set is smaller, and half of its reads overlap nothing — nodes without a row, whose
    slots still hold the linked lists of the first pass's nodes of the same ids"""
    first = branching_reads(8, fans=(2, 3))
    rng = np.random.default_rng(9)
    linked = sampled_reads(10, 150)
    second = [r for pair in zip(linked, (_seq(rng, 150) for _ in linked)) for r in pair]  # overlapping, lonely, overlapping, ...
    with buildgraph.BuildGraph(min_overlap=40) as g:
        c1 = _parity_on(g, first, 40, "first pass")
        assert len(second) < len(first) and c1["e_out"] > 0
        c2 = _parity_on(g, second, 40, "second pass on the same context")
        lens, dense, used = g.fetch_survivor_layout()
    assert dense and used == c2["e_out"] > 0
    assert int((lens == 255).sum()) >= len(linked)  # the lonely reads: no row, no list of this pass


# ---- dense output against the row path -------------------------------------------------------------------------------------------
def _edge_keys(e):
    return np.stack([e["src"].astype(np.int64), e["dst"].astype(np.int64), e["orient"].astype(np.int64), e["offset"].astype(np.int64)], axis=1)


def _outputs(spec, n_files, min_ovl_simplify):
    """everything that reads the emission's slots, in forms that do not depend on the order the edges were emitted in"""
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        _lens, dense, used = g.fetch_survivor_layout(lengths=False)
        edges = g.fetch_edges()
        files = g.fetch_edge_files(n_files)
        text, off = g.format_edges(n_files, files, None)
        comp, links, absorbed = g.contract_chains(min_ovl_simplify)
        comp2, links2, absorbed2 = g.contract_chains(min_ovl_simplify, edges=edges)  # the same slots handed back by the host: explicit identity
        e_out = g.counters()["e_out"]
    assert np.array_equal(comp, comp2) and np.array_equal(links, links2) and np.array_equal(absorbed, absorbed2)
    keys = _edge_keys(edges)
    order = np.lexsort(keys.T[::-1])
    lines = [sorted(text[int(off[t]):int(off[t + 1])].decode().splitlines()) for t in range(n_files)]
    return dict(dense=dense, used=used, e_out=e_out, edges=edges[order], files=files[order], lines=lines, n_comp=len(comp), n_links=len(links),
                absorbed=keys[order][absorbed[order] != 0])


def test_dense_output_and_its_consumers_equal_the_row_path(monkeypatch):
    spec = readgen.GenSpec.coverage(seed=77, n_reads=20_000, read_len=150, cov=30.0, n_contigs=5)
    monkeypatch.setenv("DISCO_EMIT_WAVES", "1")  # 20 k nodes are five grabs of the queue: a wavefront stages some 4000 edges, sixteen flushes
    new = _outputs(spec, 3, 50)
    monkeypatch.setenv("DISCO_NO_HALF", "1")
    old = _outputs(spec, 3, 50)
    assert new["dense"] and new["used"] == new["e_out"] > 10_000
    assert not old["dense"] and old["used"] > old["e_out"] == new["e_out"]  # the row path: chunks with unused tails
    oe, orows, _oc = run_oracle_reads(list(readgen.generate_reads(spec)), 40)
    assert np.array_equal(canon_hip(new["edges"], orows)[0], canon_hip(oe, orows)[0])
    assert np.array_equal(new["edges"], old["edges"])
    assert np.array_equal(new["files"], old["files"])
    assert new["lines"] == old["lines"] and sum(len(l) for l in new["lines"]) == new["e_out"]
    assert (new["n_comp"], new["n_links"]) == (old["n_comp"], old["n_links"]) and new["n_links"] > 0
    assert np.array_equal(new["absorbed"], old["absorbed"])
