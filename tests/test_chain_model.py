"""CPU: tests/chain_model.py — the model the device's chain contraction is held to (tests/test_gpu_chain_model.py) — held to
something else itself: to cases written out by hand, which pin the conventions independently of model and kernel (the reverse edge,
SG/EdgeSimple.cpp:119-120; is_mergeable and the merged orientation, :254-272; the twin orientation, :277), to a second statement of
which edges form a chain or a ring (union-find over kept edges joined through absorbable nodes: no walk, no order) on 320 random
multigraphs, and to the invariants of a contraction (maximal, complete, every absorbed edge used once) on the same graphs."""
from collections import Counter, defaultdict

import numpy as np
import pytest

from disco_amd.buildgraph import CHAIN_EDGE_DTYPE, CHAIN_LINK_DTYPE, EDGE_DTYPE
from tests import chain_cases
from tests.chain_model import chain_model, tile_edges, tiled, twin


def _edges(lengths, rows):
    e = np.zeros(len(rows), dtype=EDGE_DTYPE)
    for i, (s, d, o, off) in enumerate(rows):
        e[i] = (s, d, o, off, lengths[s], lengths[d])
    return e


def _same(m, comp, links, absorbed, residue, first_edges, end_first, end_last_rev):
    assert m.comp.tolist() == comp                                  # (a, b, offset, orient, n_links, first_link)
    assert m.links.tolist() == links                                # (to, offset, orient)
    assert m.absorbed.tolist() == absorbed and m.residue.tolist() == residue and m.first_edges.tolist() == first_edges
    assert m.end_first.tolist() == end_first and m.end_last_rev.tolist() == end_last_rev
    assert (m.comp.dtype, m.links.dtype, m.end_first.dtype, m.end_last_rev.dtype) == (CHAIN_EDGE_DTYPE, CHAIN_LINK_DTYPE, CHAIN_LINK_DTYPE, CHAIN_LINK_DTYPE)
    assert (m.absorbed.dtype, m.residue.dtype, m.first_edges.dtype) == (np.uint8, np.uint64, np.uint64)


# ---- written out by hand ------------------------------------------------------------------------------------------------------------
# orientation: bit 1 = the source read is read forward, bit 0 = the target read is. twin(3) = 0, twin(0) = 3, twin(2) = 2, twin(1) = 1.
LEN4 = [100, 120, 110, 130]


def test_twin_orientation():
    assert [twin(o) for o in range(4)] == [3, 1, 2, 0]


def test_a_path_of_three_edges_stored_forward():
    """0 -> 1 -> 2 -> 3. At node 1 the reverse of edge 0 leaves with twin(3) = 0 and edge 1 with 3: bit 1 differs, absorbable; at node 2
    twin(3) = 0 against 2. Built from node 0 (first half-edge 2 * 0 + 0 = 0; from node 3 it would be 2 * 2 + 1 = 5)."""
    m = chain_model(_edges(LEN4, [(0, 1, 3, 30), (1, 2, 3, 40), (2, 3, 2, 50)]), LEN4, 0)
    _same(m, comp=[(0, 3, 120, (3 & 2) | (2 & 1), 3, 0)], links=[(1, 30, 3), (2, 40, 3), (3, 50, 2)], absorbed=[1, 1, 1], residue=[],
          first_edges=[0], end_first=[(1, 30, 3)],
          end_last_rev=[(2, 130 + 50 - 110, 2)])                    # edge 2 turned round: len(dst) + offset - len(src), twin(2) = 2
    assert m.internal.tolist() == [False, True, True, False] and m.rings == [] and m.comp_edges == [[0, 1, 2]]


def test_the_same_path_with_its_middle_edge_stored_the_other_way_round():
    """edge 1 as 2 -> 1: orientation twin(3) = 0, offset len(2) + 40 - len(1) = 30. Walked 1 -> 2 it is the record of the forward case again:
    twin(0) = 3, len(1) + 30 - len(2) = 40 — the composite edge and its links are the same"""
    m = chain_model(_edges(LEN4, [(0, 1, 3, 30), (2, 1, 0, 30), (2, 3, 2, 50)]), LEN4, 0)
    _same(m, comp=[(0, 3, 120, 2, 3, 0)], links=[(1, 30, 3), (2, 40, 3), (3, 50, 2)], absorbed=[1, 1, 1], residue=[], first_edges=[0],
          end_first=[(1, 30, 3)], end_last_rev=[(2, 70, 2)])


def test_the_same_path_in_the_opposite_array_order_is_built_from_its_other_end():
    """array = [2 -> 3, 2 -> 1, 0 -> 1]: from node 0 the first half-edge is 2 * 2 + 0 = 4, from node 3 it is 2 * 0 + 1 = 1: built 3 -> 2 -> 1 -> 0.
    Links: edge 0 reversed (into 2, 130 + 50 - 110 = 70, twin(2) = 2), edge 1 as stored (into 1, 30, 0), edge 2 reversed (into 0,
    120 + 30 - 100 = 50, twin(3) = 0); merged orientation (2 & 2) | (0 & 1) = 2"""
    m = chain_model(_edges(LEN4, [(2, 3, 2, 50), (2, 1, 0, 30), (0, 1, 3, 30)]), LEN4, 0)
    _same(m, comp=[(3, 0, 150, 2, 3, 0)], links=[(2, 70, 2), (1, 30, 0), (0, 50, 0)], absorbed=[1, 1, 1], residue=[], first_edges=[0],
          end_first=[(2, 70, 2)], end_last_rev=[(1, 30, 3)])        # the last link turned round is edge 2 as stored


def test_a_triangle_of_absorbable_nodes_is_left_alone():
    lengths = [100, 120, 110]
    m = chain_model(_edges(lengths, [(0, 1, 3, 30), (1, 2, 3, 40), (2, 0, 3, 50)]), lengths, 0)
    _same(m, comp=[], links=[], absorbed=[0, 0, 0], residue=[0, 1, 2], first_edges=[], end_first=[], end_last_rev=[])
    assert m.internal.tolist() == [True, True, True] and m.rings == [[0, 1, 2]]


def test_a_branch_node_with_a_loop_of_two_edges_back_to_itself():
    """0 -> 1 -> 0 and 0 -> 2: node 0 has three edge ends, node 1 is absorbable: one chain with a == b == 0, built along edge 0
    (first half-edge 0; the other way round it is 2 * 1 + 1 = 3). The filter: at 56 the edge 0 -> 2 (overlap 100 - 45 = 55) is not
    loaded, nodes 0 and 1 are both absorbable and the pair is a ring"""
    lengths = [100, 120, 110]
    e = _edges(lengths, [(0, 1, 3, 30), (1, 0, 3, 40), (0, 2, 3, 45)])
    for min_ovl in (0, 55):
        m = chain_model(e, lengths, min_ovl)
        _same(m, comp=[(0, 0, 70, 3, 2, 0)], links=[(1, 30, 3), (0, 40, 3)], absorbed=[1, 1, 0], residue=[2], first_edges=[0],
              end_first=[(1, 30, 3)], end_last_rev=[(1, 100 + 40 - 120, 0)])
    m = chain_model(e, lengths, 56)
    _same(m, comp=[], links=[], absorbed=[0, 0, 0], residue=[0, 1], first_edges=[], end_first=[], end_last_rev=[])
    assert m.rings == [[0, 1]] and m.kept.tolist() == [True, True, False]


# ---- a second statement: union-find over edges, on random multigraphs --------------------------------------------------------------
def _absorbable(e, min_ovl):
    """node -> absorbable, from a list of edge ends per node (no sorting, no half-edge numbers)"""
    ends = defaultdict(list)
    kept = []
    for i, r in enumerate(e.tolist()):
        s, d, o, off, ls, ld = r
        kept.append(ls - off >= min_ovl)
        if kept[-1]:
            ends[s].append((i, s == d, (o >> 1) & 1))               # leaves s with the edge's orientation
            ends[d].append((i, s == d, (twin(o) >> 1) & 1))         # leaves d with the twin's
    ok = {v: len(x) == 2 and x[0][0] != x[1][0] and not x[0][1] and not x[1][1] and x[0][2] != x[1][2] for v, x in ends.items()}
    return ok, ends, kept


def _classes(e, min_ovl):
    """(chains, rings): the kept edges joined through absorbable nodes; a class with such a node is a chain, or a ring when it touches
    no other node. Each as a sorted tuple of edge indices"""
    ok, ends, kept = _absorbable(e, min_ovl)
    parent = list(range(len(e)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for v, x in ends.items():
        if ok[v]:
            parent[find(x[0][0])] = find(x[1][0])
    members = defaultdict(list)
    for i in range(len(e)):
        if kept[i]:
            members[find(i)].append(i)
    chains, rings = [], []
    for m in members.values():
        nodes = [int(e[f][i]) for i in m for f in ("src", "dst")]
        if any(ok[v] for v in nodes):
            (rings if all(ok[v] for v in nodes) else chains).append(tuple(sorted(m)))
    return sorted(chains), sorted(rings), ok, kept


def test_the_random_multigraphs_are_what_they_are_meant_to_be():
    n_nodes, n_loops, n_parallel, n_dropped, n_rings, n_chains, longest = 0, 0, 0, 0, 0, 0, 0
    for seed in chain_cases.RANDOM_SEEDS:
        e, min_ovl = chain_cases.random_multigraph(seed)
        deg = Counter(e["src"].tolist() + e["dst"].tolist())
        assert max(deg.values()) <= 4 and len(deg) <= 40
        assert ((e["offset"] > 0) & (e["offset"] < e["len_src"])).all()
        assert (e["len_dst"].astype(np.int64) + e["offset"] - e["len_src"] > 0).all()
        pairs = Counter((min(s, d), max(s, d)) for s, d in zip(e["src"].tolist(), e["dst"].tolist()))
        m = chain_model(e, chain_cases.LENGTHS, min_ovl)
        n_nodes = max(n_nodes, len(deg))
        n_loops += int((e["src"] == e["dst"]).sum())
        n_parallel += sum(c > 1 for c in pairs.values())
        n_dropped += int((~m.kept).sum())
        n_rings += len(m.rings)
        n_chains += len(m.comp)
        longest = max(longest, int(m.comp["n_links"].max()) if len(m.comp) else 0)
    assert len(chain_cases.RANDOM_SEEDS) >= 300 and 35 <= n_nodes <= 40
    assert n_loops > 100 and n_parallel > 100 and n_dropped > 500 and n_rings > 20 and n_chains > 300 and longest >= 4


@pytest.mark.parametrize("block", range(8))
def test_model_against_union_find_and_the_invariants_of_a_contraction(block):
    for seed in chain_cases.RANDOM_SEEDS[block::8]:
        e, min_ovl = chain_cases.random_multigraph(seed)
        lengths = chain_cases.LENGTHS
        m = chain_model(e, lengths, min_ovl)
        chains, rings, ok, kept = _classes(e, min_ovl)
        # the second statement
        assert m.kept.tolist() == kept, seed
        assert {v for v, x in ok.items() if x} == set(np.flatnonzero(m.internal).tolist()), seed
        assert sorted(i for c in chains for i in c) == np.flatnonzero(m.absorbed).tolist(), seed
        assert len(m.comp) == len(chains), seed
        assert sorted(tuple(sorted(c)) for c in m.comp_edges) == chains, seed
        assert sorted(tuple(sorted(r)) for r in m.rings) == rings, seed
        # every absorbed edge lies in exactly one composite edge, once
        used = Counter(i for c in m.comp_edges for i in c)
        assert set(used.values()) <= {1} and sorted(used) == np.flatnonzero(m.absorbed).tolist(), seed
        assert not m.absorbed[~m.kept].any(), seed
        ring_edges = {i for r in m.rings for i in r}
        src, dst = e["src"].astype(np.int64), e["dst"].astype(np.int64)
        for i in np.flatnonzero(m.kept).tolist():                    # complete: what touches an absorbable node went somewhere
            if m.internal[src[i]] or m.internal[dst[i]]:
                assert (m.absorbed[i] == 1) != (i in ring_edges), (seed, i)
            else:
                assert not m.absorbed[i] and i not in ring_edges, (seed, i)
        assert m.residue.tolist() == [i for i in range(len(e)) if kept[i] and not m.absorbed[i]], seed
        at = 0
        for k, c in enumerate(m.comp):
            ls = m.links[int(c["first_link"]):int(c["first_link"]) + int(c["n_links"])]
            assert int(c["first_link"]) == at and int(c["n_links"]) == len(m.comp_edges[k]) >= 2, seed
            at += len(ls)
            assert not m.internal[int(c["a"])] and not m.internal[int(c["b"])], seed          # maximal
            assert m.internal[ls["to"][:-1].astype(np.int64)].all() and int(ls["to"][-1]) == int(c["b"]), seed
            assert int(ls["offset"].astype(np.int64).sum()) == int(c["offset"]), seed
            assert int(c["orient"]) == (int(ls["orient"][0]) & 2) | (int(ls["orient"][-1]) & 1), seed
            node = int(c["a"])
            for l, i in zip(ls.tolist(), m.comp_edges[k]):            # every link is its edge, read in the direction of the walk
                s, d, o, off, ls_, ld = e[i].tolist()
                as_stored = (d, off, o) if s == node else None
                turned = (s, ld + off - ls_, twin(o)) if d == node else None
                assert l in (as_stored, turned), (seed, k, i)
                node = l[0]
            assert int(m.first_edges[k]) == m.comp_edges[k][0], seed
            assert m.end_first[k] == ls[0], seed
            before = int(ls["to"][-2])
            assert m.end_last_rev[k].tolist() == (before, int(lengths[int(c["b"])]) + int(ls["offset"][-1]) - int(lengths[before]), twin(int(ls["orient"][-1]))), seed
        assert at == len(m.links) and (np.diff(m.first_edges.astype(np.int64)) > 0).all(), seed
        # the direction: the walk the other way round starts with the last edge, and 2 * first + dir < 2 * last + dir' iff first < last
        assert all(c[0] < c[-1] for c in m.comp_edges), seed


# ---- the tiling the device test uses for an array larger than one trip of the grid ---------------------------------------------------
def test_the_tiled_model_is_the_model_of_the_tiled_graph():
    lengths = chain_cases.LENGTHS[:chain_cases.TILE_NODES]
    t = chain_cases.tile(lengths)
    assert len(t) == chain_cases.TILE_EDGES and int(max(t["src"].max(), t["dst"].max())) == chain_cases.TILE_NODES - 1
    one = chain_model(t, lengths, chain_cases.MIN_OVL)
    # what the tile is made of: paths, a ring, a branch, a ring with a tail (a == b), a two-ring, a self-loop, dropped edges
    assert sorted(len(r) for r in one.rings) == [2, 5] and len(one.comp) >= 8 and (one.comp["a"] == one.comp["b"]).sum() == 1
    assert (~one.kept).sum() > 20 and (t["src"] == t["dst"])[one.kept].sum() == 1
    for n in (1, 3):
        want = chain_model(tile_edges(t, n, chain_cases.TILE_NODES), np.tile(lengths, n), chain_cases.MIN_OVL)
        got = tiled(one, n, chain_cases.TILE_NODES, chain_cases.TILE_EDGES)
        for f in ("comp", "links", "absorbed", "residue", "first_edges", "end_first", "end_last_rev"):
            assert np.array_equal(getattr(got, f), getattr(want, f)) and getattr(got, f).dtype == getattr(want, f).dtype, (n, f)


# ---- the read sets of the device test hold what they are named for, in the oracle's reduced graph ------------------------------------
def test_the_circular_and_the_tandem_read_sets_hold_a_ring_and_parallel_edges():
    from tests.util import run_oracle_reads

    reads = chain_cases.circular_reads()
    e, _rows, _cnt = run_oracle_reads(reads, 40)
    m = chain_model(e, [len(r) for r in reads], 0)
    print("circular:", len(e), "edges, rings", [len(r) for r in m.rings], "composite edges", len(m.comp))
    assert len(m.rings) >= 1 and max(len(r) for r in m.rings) > 100 and len(m.comp) >= 1
    reads = chain_cases.tandem_reads()
    e, _rows, _cnt = run_oracle_reads(reads, 40)
    m = chain_model(e, [len(r) for r in reads], 0)
    loops, pairs = chain_cases.self_loops_and_parallel_pairs(e)
    print("tandem:", len(e), "edges, self-loops", loops, "parallel pairs", pairs, "rings", [len(r) for r in m.rings], "composite edges", len(m.comp))
    assert loops + pairs >= 1 and len(m.comp) >= 1
