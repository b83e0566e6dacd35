"""-m gpu : the partition of the edges into files (partition_edges and the uf_* kernels: a concurrent union-find, a table in LDS per block
for the component sizes, a list of the components dealt out by size, a hash for the rest) held EXACTLY to the rule as
tests/partition_model.py restates it, on graphs built to hurt it. disco_partition_edges takes any host edge array, so every case is one
call and one array comparison; the resident path (disco_fetch_edge_files) is held to the same model at the end."""
import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.partition_model import SHARE, components, partition_model

pytestmark = pytest.mark.gpu

N = 200_003   # nodes of the shapes below: odd, a few hundred blocks of 256


@pytest.fixture(scope="module")
def ctx():
    """any context will do, and the call leaves it as it was: one for the module"""
    with buildgraph.BuildGraph(min_overlap=40) as g:
        yield g


def edge_array(src, dst):
    e = np.zeros(len(src), dtype=buildgraph.EDGE_DTYPE)
    e["src"], e["dst"] = src, dst
    return e


def check(g, src, dst, n_nodes, n_files, root_of_node=None):
    want, info = partition_model(src, dst, n_nodes, n_files, root_of_node)
    got = g.partition_edges(edge_array(src, dst), n_nodes, n_files)
    assert got.dtype == np.uint16 and np.array_equal(got, want), (n_files, info["thr"], info["n_big"], int((got != want).sum()))
    return got, info


# ---- shapes that stress the concurrent union-find ------------------------------------------------------------------------------------
def _path_ascending(rng):
    s = np.arange(N - 1)
    return s, s + 1, N


def _path_descending(rng):
    s = np.arange(N - 1, 0, -1)
    return s, s - 1, N


def _path_shuffled(rng):
    p = rng.permutation(N)
    return p[:-1], p[1:], N


def _star_centre_largest(rng):
    s = np.arange(N - 1)
    return s, np.full(N - 1, N - 1), N


def _star_centre_smallest(rng):
    return np.zeros(N - 1, dtype=np.int64), np.arange(1, N), N


def _binary_tree(rng):
    s = np.arange(1, N)
    return s, (s - 1) // 2, N


def _random(rng):
    return rng.integers(0, N, 2 * N), rng.integers(0, N, 2 * N), N


def _two_paths_joined_last(rng):
    h = N // 2
    a, b = np.arange(h - 1), np.arange(h, N - 1)
    return np.concatenate([a, b, [h - 1]]), np.concatenate([a + 1, b + 1, [N - 1]]), N


def _tree_shuffled_and_swapped(rng):
    s, d, n = _binary_tree(rng)
    p = rng.permutation(len(s))
    s, d = s[p], d[p]
    odd = np.arange(len(s)) & 1 == 1
    return np.where(odd, d, s), np.where(odd, s, d), n


def _random_with_duplicates(rng):
    s, d, n = _random(rng)
    pick = rng.integers(0, len(s), len(s) // 100)
    swap = rng.random(len(pick)) < 0.5
    s2, d2 = np.concatenate([s, np.where(swap, d[pick], s[pick])]), np.concatenate([d, np.where(swap, s[pick], d[pick])])
    p = rng.permutation(len(s2))
    return s2[p], d2[p], n


def _self_loops_and_isolated(rng):
    """paths of 1 ... 2000 edges over the lower half of the ids; the upper half is isolated, but for 50 nodes with a loop on themselves
    (components of one edge and one node); 50 more loops sit on nodes inside the paths"""
    h = N // 2
    cut = np.sort(rng.choice(np.arange(1, h), 600, replace=False))
    s = np.setdiff1d(np.arange(h - 1), cut - 1)   # a path over 0 .. h - 1, cut in 600 places
    alone = rng.choice(np.arange(h, N), 50, replace=False)
    inside = rng.choice(np.arange(h), 50, replace=False)
    src, dst = np.concatenate([s, alone, inside]), np.concatenate([s + 1, alone, inside])
    p = rng.permutation(len(src))
    return src[p], dst[p], N


def _sparse_ids_up_to_the_last(rng):
    """n_nodes is five times the ids in use, the last one among them"""
    n = 5 * N
    ids = np.concatenate([rng.choice(n - 1, N - 1, replace=False), [n - 1]])
    s, d = ids[rng.integers(0, N, N)], ids[rng.integers(0, N, N)]
    return np.concatenate([s, [n - 1]]), np.concatenate([d, ids[:1]]), n


SHAPES = {f.__name__[1:]: f for f in (_path_ascending, _path_descending, _path_shuffled, _star_centre_largest, _star_centre_smallest, _binary_tree,
                                      _random, _two_paths_joined_last, _tree_shuffled_and_swapped, _random_with_duplicates,
                                      _self_loops_and_isolated, _sparse_ids_up_to_the_last)}
ONE_COMPONENT = ("path_ascending", "path_descending", "path_shuffled", "star_centre_largest", "star_centre_smallest", "binary_tree",
                 "two_paths_joined_last", "tree_shuffled_and_swapped")


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_that_stress_the_union_find(ctx, name):
    """about 2 * 10^5 nodes each: long chains of hooks, one contended root, hooks against the id order, and a giant component among dust"""
    src, dst, n = SHAPES[name](np.random.default_rng(len(name)))
    root = np.zeros(n, dtype=np.int64) if name in ONE_COMPONENT else components(src, dst, n)
    for nf in (1, 2, 7, 256):
        f, info = check(ctx, src, dst, n, nf, root)
        cnt = info["cnt"]
        if name in ONE_COMPONENT:
            assert info["n_components"] == info["n_big"] == 1 and cnt[0] == N - 1 and np.all(f == 0)
        elif name in ("random", "random_with_duplicates"):
            assert cnt.max() > len(src) // 2 and info["n_components"] > 10 and info["n_big"] == 1   # a giant component and dust
            assert (src == dst).any() and (src > dst).any()
            if name == "random_with_duplicates":
                assert len(src) - len(np.unique(np.minimum(src, dst) * n + np.maximum(src, dst))) >= len(src) // 101
        elif name == "self_loops_and_isolated":
            loops = src == dst
            size_at_loop = cnt[info["root_of_node"][src[loops]]]
            assert loops.sum() == 100 and (size_at_loop == 1).sum() >= 50 and (size_at_loop > 1).sum() >= 40 and info["n_components"] > 600
            assert np.count_nonzero(np.bincount(np.concatenate([src, dst]), minlength=n) == 0) > N // 3   # isolated nodes
        else:
            assert n == 5 * N and max(src.max(), dst.max()) == n - 1 and len(np.unique(np.concatenate([src, dst]))) < n // 4
            assert info["n_components"] > 10


# ---- the threshold and the ties ------------------------------------------------------------------------------------------------------
def _paths_of(sizes, rng, spare=0):
    """disjoint paths of the given numbers of edges, over shuffled ids (so that the root order is not the order of construction)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int((sizes + 1).sum()) + spare
    first = np.concatenate([[0], np.cumsum(sizes + 1)[:-1]])
    s = np.repeat(first, sizes) + (np.arange(sizes.sum()) - np.repeat(np.cumsum(sizes) - sizes, sizes))
    ids = rng.permutation(n)
    p = rng.permutation(len(s))
    return ids[s][p], ids[s + 1][p], n


@pytest.mark.parametrize("n_files,mult", [(1, 40), (3, 5), (3, 2), (7, 3), (256, 3)])
@pytest.mark.parametrize("one_less", [0, 1])
def test_components_on_both_sides_of_the_threshold(ctx, n_files, mult, one_less):
    """ne an exact multiple of 64 * n_files, and one less (which lowers the threshold by one): components of thr - 1, thr and thr + 1 edges,
    many of each, so that equal sizes are ordered by their roots; what is left over goes into single edges"""
    rng = np.random.default_rng(n_files * 100 + mult)
    ne = mult * SHARE * n_files - one_less
    thr = max(ne // (SHARE * n_files), 1)
    assert thr == mult - one_less
    trip = ne // (3 * thr)
    sizes = [s for s in [thr - 1, thr, thr + 1] * trip if s > 0]
    sizes += [1] * (ne - sum(sizes))
    src, dst, n = _paths_of(sizes, rng, spare=17)
    assert len(src) == ne
    f, info = check(ctx, src, dst, n, n_files)
    cnt = info["cnt"][info["cnt"] > 0]
    assert info["thr"] == thr and min((cnt == thr).sum(), (cnt == thr + 1).sum()) >= 20 and (cnt < thr).sum() >= (20 if thr > 1 else 0)
    assert thr == 1 or 0 < info["n_big"] < info["n_components"]


# ---- the band in which a list of 64 * n_files + 64 entries overflowed ------------------------------------------------------------------
def _band(size, n_files):
    ne = (size + 1) * SHARE * n_files - size
    src, dst, n = _paths_of([size] * (ne // size), np.random.default_rng(size * 1000 + n_files), spare=31)
    assert len(src) == ne
    return src, dst, n


BAND = [(1, 2), (1, 3), (1, 7), (1, 200), (2, 3), (2, 7)]


@pytest.mark.parametrize("size,n_files", BAND)
def test_more_components_by_size_than_64_per_file(ctx, size, n_files):
    """disjoint single edges with ne = 128 * n_files - 1, pairs of edges with ne = 3 * 64 * n_files - 2: every component has thr edges
    and is dealt out by size — all of them, in root order, not the first 64 * n_files + 64 that an atomic counter let in"""
    src, dst, n = _band(size, n_files)
    f, info = check(ctx, src, dst, n, n_files)
    assert info["thr"] == size and info["n_big"] == info["n_components"] == len(src) // size
    assert info["n_big"] > SHARE * n_files + SHARE
    load = np.bincount(f, minlength=n_files)
    assert load.max() - load.min() <= size   # equal sizes, dealt round robin


@pytest.mark.parametrize("n_files,ne", [(256, 100), (256, 255), (65534, 1000)])
def test_fewer_edges_than_files(ctx, n_files, ne):
    """thr = 1, every component goes by size and meets an empty file: files 0 .. n_big - 1 are in use"""
    rng = np.random.default_rng(ne)
    sizes = []
    while sum(sizes) < ne:
        sizes.append(min(int(rng.integers(1, 6)), ne - sum(sizes)))
    src, dst, n = _paths_of(sizes, rng, spare=5)
    f, info = check(ctx, src, dst, n, n_files)
    assert info["thr"] == 1 and info["n_big"] == info["n_components"] == len(sizes) < n_files
    assert np.array_equal(np.unique(f), np.arange(info["n_big"]))


# ---- more roots in one block than the table in LDS holds -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_roots():
    """6 * 256 edges for each of the 16 * CUs blocks of uf_count_kernel (6.3 * 10^6 edges on the 256 CUs of an MI355X; nothing was
    reduced), into 256 files. Nine in ten are disjoint single edges, every one a root of its own; 21 large components — paths, of
    thr - 1, thr, thr + 1 edges, a few sizes around 8 thr that step by one, and around 100, 300 and 800 thr — are shuffled into the
    array, ids shuffled as well. A block meets about 1380 distinct roots for its 1024 slots, and the large components' roots
    in every block; one edge miscounted moves a component across the threshold or past a neighbour in the order."""
    import torch

    grid = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    n_files, ne = 256, 6 * 256 * grid
    rng = np.random.default_rng(2024)
    thr = ne // (SHARE * n_files)
    large = [thr - 1, thr, thr + 1, thr - 1, thr, thr + 1] + [8 * thr + k for k in range(-3, 4)] + [100 * thr, 100 * thr + 1, 100 * thr + 2,
                                                                                                   300 * thr, 300 * thr + 1, 800 * thr, 800 * thr - 1, 50 * thr]
    sizes = np.concatenate([np.asarray(large, dtype=np.int64), np.ones(ne - sum(large), dtype=np.int64)])
    n = int((sizes + 1).sum()) + 1000
    first = np.concatenate([[0], np.cumsum(sizes + 1)[:-1]])
    s = np.repeat(first, sizes) + (np.arange(ne) - np.repeat(np.cumsum(sizes) - sizes, sizes))
    ids = rng.permutation(n)
    comp_root = np.minimum.reduceat(ids[:first[-1] + 2], first)   # a path's nodes lie side by side before the ids are shuffled
    root_of_node = np.arange(n, dtype=np.int64)
    root_of_node[ids[:first[-1] + 2]] = np.repeat(comp_root, sizes + 1)
    single = np.repeat(sizes == 1, sizes)
    p = rng.permutation(ne)
    src, dst, single = ids[s][p], ids[s + 1][p], single[p]
    block = (np.arange(ne) // 256) % grid
    assert np.bincount(block[single], minlength=grid).min() > 1024          # distinct roots per block: more than the table's slots
    assert np.bincount(block[~single], minlength=grid).min() >= len(large)  # and edges of the large components in every block
    want, info = partition_model(src, dst, n, n_files, root_of_node)
    assert info["thr"] == thr and info["n_big"] == len(large) - 2 and info["n_components"] == len(sizes)
    assert sorted(info["cnt"][info["big_roots"]].tolist()) == sorted(x for x in large if x >= thr)
    return edge_array(src, dst), n, n_files, want


def test_more_roots_in_a_block_than_its_table_holds(ctx, many_roots):
    e, n, n_files, want = many_roots
    assert np.array_equal(ctx.partition_edges(e, n, n_files), want)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_files(ctx, many_roots):
    e, n, n_files, want = many_roots
    for _ in range(3):
        assert np.array_equal(ctx.partition_edges(e, n, n_files), want)
    src, dst, n = _band(1, 7)
    e = edge_array(src, dst)
    first = ctx.partition_edges(e, n, 7)
    for _ in range(2):
        assert np.array_equal(ctx.partition_edges(e, n, 7), first)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    e = edge_array(np.arange(10), np.arange(10) + 1)
    for n_files in (0, 0xFFFF):
        with pytest.raises(buildgraph.DiscoError, match="error -1"):
            ctx.partition_edges(e, 11, n_files)
    assert np.array_equal(ctx.partition_edges(e, 11, 0xFFFE), partition_model(e["src"], e["dst"], 11, 0xFFFE)[0])
    empty = ctx.partition_edges(e[:0], 11, 3)
    assert empty.dtype == np.uint16 and len(empty) == 0


# ---- the resident path against the host-array path -----------------------------------------------------------------------------------
CONTIGS12 = dict(seed=41, n_reads=30000, read_len=150, cov=30.0, n_contigs=12)                          # tests/test_gpu_parity.py
ERRORS = dict(seed=22, n_reads=60_000, read_len=100, cov=25.0, n_contigs=12, len_max=220)               # tests/test_gpu_par_simple_text.py


def _pairs_and_triples(rng):
    """2000 components of one edge and 500 of two: reads of 100 bases cut 40 apart from random stretches, nothing contained"""
    reads = []
    for k in range(2500):
        x = "".join("ACGT"[b] for b in rng.integers(0, 4, 180))
        reads += [x[0:100], x[40:140]] + ([x[80:180]] if k % 5 == 0 else [])
    return reads


@pytest.mark.parametrize("name", ["contigs12", "errors", "errors_unused_tails", "errors_second_pass", "pairs_and_triples"])
def test_resident_edges_are_cut_like_host_edges(name, monkeypatch):
    """disco_fetch_edge_files partitions the emission where it lies (with DISCO_NO_HALF=1: chunks with unused tails, so valid / pos are
    in use), disco_partition_edges the same edges from a host array: both are the model's files. The generated sets have 12 and 16
    components (all dealt out by size at 200 files); the pairs and triples 2500, hashed at 4 and 7 files, by size at 1 and 200"""
    if name == "errors_unused_tails":
        monkeypatch.setenv("DISCO_NO_HALF", "1")
    spec = readgen.GenSpec.coverage(**(CONTIGS12 if name == "contigs12" else ERRORS))
    with buildgraph.BuildGraph(min_overlap=40) as g:
        if name == "pairs_and_triples":
            reads = _pairs_and_triples(np.random.default_rng(77))
            g.upload_ascii(reads)
            n = len(reads)
        else:
            g.generate_reads(spec)
            n = spec.n_reads
        if name.startswith("errors"):
            g.substitute_bases(5, 2000)
        g.run_graph()
        if name == "errors_second_pass":
            g.run_graph()
        _, dense, used = g.fetch_survivor_layout(lengths=False)
        e = g.fetch_edges()
        if name == "errors_unused_tails":
            assert not dense and used > len(e)
        assert len(e) == 3000 if name == "pairs_and_triples" else len(e) > 10_000
        root = components(e["src"], e["dst"], n)
        for nf in (1, 4, 7, 200):
            want, info = partition_model(e["src"], e["dst"], n, nf, root)
            assert np.array_equal(g.fetch_edge_files(nf), want), (nf, "resident")
            assert np.array_equal(g.partition_edges(e, n, nf), want), (nf, "host array")
            assert np.array_equal(g.fetch_edges(), e)   # and the graph state is as it was
        assert info["n_components"] == info["n_big"] == 2500 if name == "pairs_and_triples" else info["n_components"] >= 12
