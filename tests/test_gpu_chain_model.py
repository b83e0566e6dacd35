"""-m gpu : the chain contraction (disco_contract_chains / disco_contract_chains_of, disco_amd/csrc/disco_chains.h) held to
tests/chain_model.py, which walks the chains the kernels rank — every output array, whole and exact: the composite edges, their
links, the absorbed flags, the residue, the first edge of every composite edge and its two end links. The files made from these
records cannot show an incomplete contraction (the host pass contracts what is left); these comparisons can.

Constructed arrays go through contract_chains(min_ovl, edges=...) on a context that holds reads of the lengths the arrays were made
for (no graph is run); the emission's slot layout through contract_chains(min_ovl) after run_graph, with the model on fetch_edges()."""
import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests import chain_cases as cc
from tests.chain_model import chain_model, tile_edges, tiled

pytestmark = pytest.mark.gpu

FIELDS = ("comp", "links", "absorbed", "residue", "first_edges", "end_first", "end_last_rev")


def reads_of(lengths, seed=1):
    """random reads of the given lengths"""
    lengths = np.asarray(lengths).astype(np.int64)
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, int(off[-1]))].tobytes().decode()
    return [text[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def contracted(g, min_ovl, edges=None):
    """everything the device hands back after one contraction, under the model's names"""
    comp, links, absorbed = g.contract_chains(min_ovl, edges=edges)
    residue, records = g.chain_residue(records=edges is None)
    end_first, end_last_rev = g.chain_end_links(len(comp))
    return dict(comp=comp, links=links, absorbed=absorbed, residue=residue, first_edges=g.chain_first_edges(len(comp)), end_first=end_first,
                end_last_rev=end_last_rev, records=records)


def hold(got, want, label=""):
    for f in FIELDS:
        a, b = got[f], getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (label, f, len(a), len(b))


def check(g, edges, min_ovl, lengths=cc.LENGTHS, label=""):
    want = chain_model(edges, lengths, min_ovl)
    hold(contracted(g, min_ovl, edges), want, label)
    return want


@pytest.fixture(scope="module")
def ctx():
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads_of(cc.LENGTHS))
        yield g


# ---- ranking rounds -----------------------------------------------------------------------------------------------------------------
SMALL = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("lengths_of_paths", [SMALL, (65_535,), (65_536,), (65_537,)], ids=["1-1025", "65535", "65536", "65537"])
def test_disjoint_paths_are_ranked_to_their_ends(ctx, lengths_of_paths, order):
    rng = np.random.default_rng(len(order) + lengths_of_paths[-1])
    e, n_nodes = cc.paths(cc.LENGTHS, lengths_of_paths, rng)
    assert n_nodes <= cc.N_READS
    want = check(ctx, cc.ordered(e, order, rng), cc.MIN_OVL, label=order)
    assert sorted(want.comp["n_links"].tolist()) == sorted(L for L in lengths_of_paths if L > 1) and not want.rings   # one whole chain per path
    assert len(want.residue) == (1 if 1 in lengths_of_paths else 0)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("n_edges", [2, 3, 4097])
def test_one_path_that_is_the_whole_array(ctx, n_edges, order):
    """the bound of the rounds comes from the array's size: here the chain has every half-edge of one direction. A chain of L links
    needs ceil(log2 L) jumps and the bound 2^rounds >= 2 L grants one more: a ranking one round short still passes, one two rounds
    short leaves the ends of every such chain looking like a ring, and composite edges, links and absorbed flags all differ"""
    rng = np.random.default_rng(n_edges)
    e, _ = cc.paths(cc.LENGTHS, (n_edges,), rng, first_node=int(rng.integers(0, 50_000)))
    want = check(ctx, cc.ordered(e, order, rng), cc.MIN_OVL, label=order)
    assert want.comp["n_links"].tolist() == [n_edges] and want.absorbed.all()


# ---- rings --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_rings_between_chains_are_left_alone_and_the_chains_come_out_whole(ctx, order):
    rng = np.random.default_rng(11)
    parts, at, ring_sizes = [], 0, (2, 3, 4, 64, 1000)
    for k, size in enumerate(ring_sizes):
        p, at = cc.paths(cc.LENGTHS, (5 + 300 * k,), rng, first_node=at)
        parts += [p, cc.walk(cc.LENGTHS, np.arange(at, at + size), rng, closed=True)]
        at += size
    # a ring with one tail: its attachment node has three edge ends, so it is a chain from that node to itself
    parts += [cc.walk(cc.LENGTHS, np.arange(at, at + 9), rng, closed=True), cc.walk(cc.LENGTHS, [at, at + 9, at + 10], rng)]
    p, _ = cc.paths(cc.LENGTHS, (700,), rng, first_node=at + 11)
    want = check(ctx, cc.ordered(np.concatenate(parts + [p]), order, rng), cc.MIN_OVL, label=order)
    assert sorted(len(r) for r in want.rings) == list(ring_sizes)
    assert sorted(want.comp["n_links"].tolist()) == [2, 5, 9, 305, 605, 700, 905, 1205]
    loop = want.comp[want.comp["n_links"] == 9][0]
    assert loop["a"] == loop["b"] == at


# ---- special nodes ------------------------------------------------------------------------------------------------------------------
def test_self_loops_parallel_edges_same_side_nodes_and_a_star(ctx):
    rng = np.random.default_rng(12)
    L = cc.LENGTHS
    parts = [cc.walk(L, [0, 0], rng),                                    # a node with nothing but a self-loop
             cc.walk(L, [1, 1, 2, 3], rng),                              # a self-loop and one edge: three edge ends; 2 is absorbable
             cc.walk(L, [5, 4, 5, 6], rng),                              # parallel edges 4 = 5 and a third edge at 5: the chain 5 -> 4 -> 5
             cc.walk(L, [7, 8], rng, closed=True),                       # the same without the third edge: a two-ring
             cc.walk(L, [9, 10], rng, closed=True, same_side_at=(0,)),   # parallel edges that leave 9 on the same side: 10 absorbable, 9 not
             cc.walk(L, range(11, 18), rng, same_side_at=(3,)),          # a path whose middle node has both edges on one side: two chains
             cc.make_edges(L, [100] * 1000, range(101, 1101), rng.integers(0, 2, 1000), rng.integers(0, 2, 1000), rng),   # a star
             cc.make_edges(L, range(101, 601), range(1101, 1601), np.ones(500, dtype=np.int64), rng.integers(0, 2, 500), rng)]  # half its rays go on
    e = np.concatenate(parts)
    for order in ("ascending", "shuffled"):
        arr = cc.ordered(e, order, rng)
        want = check(ctx, arr, cc.MIN_OVL, label=order)
        assert not want.internal[[0, 1, 3, 5, 9, 14, 100]].any() and want.internal[[2, 4, 7, 8, 10, 12, 16]].all()
        assert sorted(len(r) for r in want.rings) == [2]
        by_end = {tuple(sorted((int(c["a"]), int(c["b"])))): int(c["n_links"]) for c in want.comp if c["a"] < 100}   # (either direction)
        assert by_end == {(1, 3): 2, (5, 5): 2, (9, 9): 2, (11, 14): 3, (14, 17): 3}
        rays = want.comp[(want.comp["a"] >= 100) | (want.comp["b"] >= 100)]
        assert len(rays) == int(want.internal[101:601].sum()) > 100 and (rays["n_links"] == 2).all()


# ---- the filter ---------------------------------------------------------------------------------------------------------------------
def test_the_overlap_filter_decides_which_nodes_are_absorbable(ctx):
    """three paths 0 - 1 - v - 3 - 4 with a third edge at v that overlaps by min_ovl - 1, min_ovl and min_ovl + 1: v is absorbable
    exactly where that edge is not loaded"""
    rng = np.random.default_rng(13)
    L, min_ovl = cc.LENGTHS, 60
    parts, vs = [], []
    for k, d in enumerate((-1, 0, 1)):
        base = 200 + 10 * k
        vs.append(base + 2)
        parts += [cc.walk(L, np.arange(base, base + 5), rng, ov_lo=min_ovl + 1), cc.make_edges(L, [base + 2], [base + 5], [rng.integers(0, 2)], [0], rng, overlap=min_ovl + d)]
    e = cc.ordered(np.concatenate(parts), "shuffled", rng)
    want = check(ctx, e, min_ovl)
    assert want.internal[vs].tolist() == [True, False, False] and sorted(want.comp["n_links"].tolist()) == [2, 2, 2, 2, 4]
    want = check(ctx, e, min_ovl + 1)
    assert want.internal[vs].tolist() == [True, True, False] and sorted(want.comp["n_links"].tolist()) == [2, 2, 4, 4]
    want = check(ctx, e, 0)
    assert not want.internal[vs].any() and want.kept.all()
    want = check(ctx, e, 10_000)                                          # nothing passes
    assert not want.kept.any() and len(want.comp) == 0 and len(want.residue) == 0


# ---- more half-edges than one trip of the grid --------------------------------------------------------------------------------------
def test_an_array_larger_than_one_trip_of_the_grid():
    import torch

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    one_trip = 16 * 256 * n_cu                                            # flat_grid: at most 16 blocks of 256 threads per CU
    n_tiles = one_trip // cc.TILE_EDGES + 3
    lengths = cc.LENGTHS[:cc.TILE_NODES]
    t = cc.tile(lengths)
    one = chain_model(t, lengths, cc.MIN_OVL)
    assert len(one.comp) >= 8 and sorted(len(r) for r in one.rings) == [2, 5]
    e = tile_edges(t, n_tiles, cc.TILE_NODES)
    assert len(e) > one_trip                                              # slots; the half-edges are twice as many
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads_of(np.tile(lengths, n_tiles)))
        hold(contracted(g, cc.MIN_OVL, e), tiled(one, n_tiles, cc.TILE_NODES, cc.TILE_EDGES))


# ---- random multigraphs -------------------------------------------------------------------------------------------------------------
def test_random_multigraphs(ctx):
    assert len(cc.RANDOM_SEEDS) >= 300
    for seed in cc.RANDOM_SEEDS:
        e, min_ovl = cc.random_multigraph(seed)
        check(ctx, e, min_ovl, label=seed)


# ---- reuse --------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_three_times_then_another_graph(ctx):
    rng = np.random.default_rng(14)
    e, at = cc.paths(cc.LENGTHS, (1, 2, 33, 1025, 3000), rng)
    e = cc.ordered(np.concatenate([e, cc.walk(cc.LENGTHS, np.arange(at, at + 17), rng, closed=True)]), "shuffled", rng)
    want = chain_model(e, cc.LENGTHS, cc.MIN_OVL)
    for k in range(3):
        hold(contracted(ctx, cc.MIN_OVL, e), want, label=k)
    other, _ = cc.paths(cc.LENGTHS, (4, 600, 2), rng, first_node=20_000)
    check(ctx, cc.ordered(other, "descending", rng), cc.MIN_OVL, label="other")
    hold(contracted(ctx, cc.MIN_OVL, e), want, label="back")


# ---- resident edges: the emission's slots with valid / pos --------------------------------------------------------------------------
def _errors(g, seed=22):
    spec = readgen.GenSpec.coverage(seed=seed, n_reads=60_000, read_len=100, cov=25.0, n_contigs=12, len_max=220, skew=0)
    g.generate_reads(spec)
    g.substitute_bases(5, 2000)


def _upload(reads):
    return lambda g: g.upload_ascii(reads)


def _resident(load, min_ovls, second_pass=False, before=None):
    """run the graph on the reads `load` puts into a context (second_pass: after a pass over other reads), contract the resident
    edges at every min_ovl (a function of the edges gives them) and hold them to the model on fetch_edges(): (edges, the models, dense)"""
    with buildgraph.BuildGraph(min_overlap=40) as g:
        if second_pass:
            before(g)
            g.run_graph()
            g.contract_chains(0)
        load(g)
        g.run_graph()
        edges = g.fetch_edges()
        _, lens = g.download_reads()
        _lens, dense, _used = g.fetch_survivor_layout(lengths=False)
        models = []
        for min_ovl in min_ovls(edges):
            want = chain_model(edges, lens, min_ovl)
            got = contracted(g, min_ovl)
            hold(got, want, label=min_ovl)
            assert np.array_equal(got["records"], edges[got["residue"].astype(np.int64)])
            hold(contracted(g, min_ovl, edges), want, label=("of", min_ovl))   # the same records from the array handed back by the host
            models.append(want)
    return edges, models, dense


VARIANTS = ["plain", "unused_tails", "second_pass"]


def _variant(variant, monkeypatch):
    if variant == "unused_tails":
        monkeypatch.setenv("DISCO_NO_HALF", "1")   # the emission leaves chunks with unused tails: valid / pos are in use
    return dict(second_pass=variant == "second_pass")


@pytest.mark.parametrize("variant", VARIANTS)
def test_resident_edges_of_reads_with_errors(variant, monkeypatch):
    kw = _variant(variant, monkeypatch)
    median = lambda e: (0, int(np.median(e["len_src"].astype(np.int64) - e["offset"])))   # at the median overlap half the edges fall to the filter
    edges, (at0, at_median), dense = _resident(_errors, median, before=lambda g: _errors(g, seed=29), **kw)
    assert variant != "unused_tails" or not dense
    assert 10_000 < len(edges) <= 120_000 and len(at0.comp) > 100 and len(at_median.comp) > 100
    assert 0.3 < at_median.kept.mean() < 0.7 and not np.array_equal(at0.absorbed, at_median.absorbed)


@pytest.mark.parametrize("variant", VARIANTS)
def test_resident_edges_of_a_circular_genome_hold_a_ring(variant, monkeypatch):
    kw = _variant(variant, monkeypatch)
    edges, (m,), dense = _resident(_upload(cc.circular_reads()), lambda e: (0,), before=_upload(cc.tandem_reads()), **kw)
    assert variant != "unused_tails" or not dense
    assert len(m.rings) >= 1 and max(len(r) for r in m.rings) > 100 and len(m.comp) >= 1


@pytest.mark.parametrize("variant", VARIANTS)
def test_resident_edges_of_a_tandem_repeat_hold_parallel_edges(variant, monkeypatch):
    kw = _variant(variant, monkeypatch)
    edges, (m, _m50), dense = _resident(_upload(cc.tandem_reads()), lambda e: (0, 50), before=_upload(cc.circular_reads()), **kw)
    loops, pairs = cc.self_loops_and_parallel_pairs(edges)
    assert variant != "unused_tails" or not dense
    assert loops + pairs >= 1 and len(m.comp) >= 1
