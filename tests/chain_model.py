"""The chain contraction, restated in plain Python/numpy from what include/disco_hip.h (disco_contract_chains) and the header comment
of disco_amd/csrc/disco_chains.h promise. The kernels RANK the chains by pointer jumping; this WALKS them, one link after the other,
as the reference does (contractParCompositeEdges, SG/OverlapGraphSimple.cpp; the conventions: SG/EdgeSimple.cpp:119-120 the reverse
edge, 254-272 is_mergeable and the merged orientation, 277 the twin orientation).

  1. an edge is kept iff len(src) - offset >= min_overlap_simplify
  2. half-edge (i, 0) is src -> dst with the edge's orient and offset; (i, 1) is dst -> src with twin(orient) and the offset
     len(dst) + offset - len(src)
  3. a node is internal iff exactly two kept edge ends meet it, of two different edges, neither a self-loop, and the two half-edges
     that leave it differ in bit 1 of their orientation
  4. a chain is a maximal walk whose inner nodes are all internal, with at least one inner node
  5. a closed walk over internal nodes only (a ring) is left alone: its edges stay in the residue
  6. of a chain's two directions the one is built whose first half-edge has the smaller 2 * (array index of its edge) + dir
  7. composite edge: a = source of the first half-edge, b = target of the last, offset = sum of the links' offsets,
     orient = (first.orient & 2) | (last.orient & 1), n_links; links (to, offset, orient) in walk order
  8. composite edges are numbered by the array position of the edge behind their first link; first_link is the running sum of n_links
"""
from types import SimpleNamespace

import numpy as np

from disco_amd.buildgraph import CHAIN_EDGE_DTYPE, CHAIN_LINK_DTYPE


def twin(o):
    return ((o >> 1) ^ 1) | (((o & 1) ^ 1) << 1)


def internal_nodes(src, dst, orient, kept, n_nodes):
    """(internal flag per node, out[v] = the one or two half-edges 2 * i + dir that leave an internal node v) — rule 3"""
    idx = np.flatnonzero(kept)
    node = np.concatenate([src[idx], dst[idx]])
    half = np.concatenate([2 * idx, 2 * idx + 1])
    bit1 = np.concatenate([(orient[idx] >> 1) & 1, (orient[idx] & 1) ^ 1])   # bit 1 of orient, and of twin(orient)
    loop = np.concatenate([src[idx] == dst[idx]] * 2)
    order = np.argsort(node, kind="stable")
    node, half, bit1, loop = node[order], half[order], bit1[order], loop[order]
    deg = np.bincount(node, minlength=n_nodes)
    first = np.cumsum(deg) - deg
    two = np.flatnonzero(deg == 2)
    p = first[two]
    ok = (half[p] >> 1 != half[p + 1] >> 1) & ~loop[p] & ~loop[p + 1] & (bit1[p] != bit1[p + 1])
    internal = np.zeros(n_nodes, dtype=bool)
    internal[two[ok]] = True
    out = np.full((n_nodes, 2), -1, dtype=np.int64)
    out[two[ok], 0], out[two[ok], 1] = half[p[ok]], half[p[ok] + 1]
    return internal, out


def chain_model(edges, lengths, min_overlap_simplify):
    """everything the C-ABI returns after disco_contract_chains[_of] on `edges` (buildgraph.EDGE_DTYPE), as a namespace:
    comp, links, absorbed, residue (chain_residue's indices), first_edges (chain_first_edges), end_first / end_last_rev
    (chain_end_links); beside them what the tests ask about: internal (flag per node), comp_edges (per composite the array
    indices of its links' edges, in walk order), rings (per ring the array indices of its edges, in walk order from its smallest)"""
    all_lengths = np.asarray(lengths).astype(np.int64)
    ne = len(edges)
    assert ne == 0 or max(edges["src"].max(), edges["dst"].max()) < len(all_lengths)
    # the nodes that have edges, renumbered in order of their ids: a graph of forty nodes somewhere in a large table costs forty
    ids = np.unique(np.concatenate([edges["src"], edges["dst"]])).astype(np.int64)
    src, dst = np.searchsorted(ids, edges["src"].astype(np.int64)), np.searchsorted(ids, edges["dst"].astype(np.int64))
    orient, offset = edges["orient"].astype(np.int64), edges["offset"].astype(np.int64)
    lengths, n_nodes = all_lengths[ids], len(ids)
    assert np.array_equal(lengths[src], edges["len_src"]) and np.array_equal(lengths[dst], edges["len_dst"])
    kept = lengths[src] - offset >= min_overlap_simplify
    internal, out = internal_nodes(src, dst, orient, kept, n_nodes)

    # the four attributes of every half-edge 2 * i + dir (rule 2), as lists: the walk below is plain Python
    h_from = np.stack([src, dst], axis=1).reshape(-1).tolist()
    h_to = np.stack([dst, src], axis=1).reshape(-1).tolist()
    h_ori = np.stack([orient, twin(orient)], axis=1).reshape(-1).tolist()
    h_off = np.stack([offset, lengths[dst] + offset - lengths[src]], axis=1).reshape(-1).tolist()
    is_int, out_l = internal.tolist(), out.tolist()

    def walk(h):
        """the half-edges from h on while the node reached is internal; stops when it comes back to h (a ring)"""
        path = [h]
        while True:
            v = h_to[path[-1]]
            if not is_int[v]:
                return path, False
            a, b = out_l[v]
            nxt = b if a == (path[-1] ^ 1) else a          # not the way back
            if nxt == h:
                return path, True
            path.append(nxt)

    absorbed = np.zeros(ne, dtype=np.uint8)
    in_ring = np.zeros(ne, dtype=bool)
    chains, rings = [], []
    touches = np.flatnonzero(kept & (internal[src] | internal[dst])).tolist()
    for i in touches:                                       # ascending: a chain is met first at the smaller of its two end half-edges (rule 6)
        starts = [2 * i + d for d in (0, 1) if not is_int[h_from[2 * i + d]]]
        if absorbed[i] or not starts:                       # (both ends internal: an inner edge of a chain, or of a ring)
            continue
        path, closed = walk(starts[0])
        assert not closed and len(path) >= 2 and len(starts) == 1
        assert starts[0] < (path[-1] ^ 1)                   # rule 6: the other direction starts with the reverse of the last half-edge
        assert not absorbed[[h >> 1 for h in path]].any()
        absorbed[[h >> 1 for h in path]] = 1
        chains.append(path)
    for i in touches:                                       # what no walk from a chain's end reached lies on a ring (rule 5)
        if absorbed[i] or in_ring[i]:
            continue
        path, closed = walk(2 * i)
        assert closed
        rings.append([h >> 1 for h in path])
        in_ring[rings[-1]] = True
    chains.sort(key=lambda p: p[0] >> 1)                    # rule 8 (the order they were met in already)

    comp = np.zeros(len(chains), dtype=CHAIN_EDGE_DTYPE)
    links = np.zeros(sum(len(p) for p in chains), dtype=CHAIN_LINK_DTYPE)
    end_first = np.zeros(len(chains), dtype=CHAIN_LINK_DTYPE)
    end_last_rev = np.zeros(len(chains), dtype=CHAIN_LINK_DTYPE)
    first_edges = np.zeros(len(chains), dtype=np.uint64)
    at = 0
    for k, p in enumerate(chains):
        ls = [(h_to[h], h_off[h], h_ori[h]) for h in p]
        links[at:at + len(p)] = ls
        comp[k] = (h_from[p[0]], h_to[p[-1]], sum(l[1] for l in ls), (ls[0][2] & 2) | (ls[-1][2] & 1), len(p), at)
        first_edges[k] = p[0] >> 1
        end_first[k] = ls[0]
        r = p[-1] ^ 1                                       # the last link turned round: into the node before the last
        end_last_rev[k] = (h_to[r], h_off[r], h_ori[r])
        at += len(p)
    for a, fields in ((comp, ("a", "b")), (links, ("to",)), (end_first, ("to",)), (end_last_rev, ("to",))):
        for f in fields:                                    # back to the ids of the table
            a[f] = ids[a[f].astype(np.int64)]
    full = np.zeros(len(all_lengths), dtype=bool)
    full[ids] = internal
    internal = full
    residue = np.flatnonzero(kept & (absorbed == 0)).astype(np.uint64)
    return SimpleNamespace(comp=comp, links=links, absorbed=absorbed, residue=residue, first_edges=first_edges, end_first=end_first,
                           end_last_rev=end_last_rev, internal=internal, kept=kept, comp_edges=[[h >> 1 for h in p] for p in chains], rings=rings)


def tiled(model, n_tiles, nodes_per_tile, edges_per_tile):
    """the model of a graph repeated n_tiles times with node ids shifted by nodes_per_tile and array positions by edges_per_tile,
    from the model of one tile — built in numpy, so that no Python loop sees the large array"""
    t = np.arange(n_tiles, dtype=np.uint64)
    nc, nl = len(model.comp), len(model.links)

    def rep(a, field, step, per):
        a = np.tile(a, n_tiles)
        shift = np.repeat(t * np.uint64(step), per)
        if field is None:
            return a + shift.astype(a.dtype)
        for f in field:
            a[f] = a[f] + shift.astype(a[f].dtype)
        return a

    comp = rep(model.comp, ("a", "b"), nodes_per_tile, nc)
    comp["first_link"] += np.repeat(t * np.uint64(nl), nc)
    return SimpleNamespace(comp=comp, links=rep(model.links, ("to",), nodes_per_tile, nl), absorbed=np.tile(model.absorbed, n_tiles),
                           residue=rep(model.residue, None, edges_per_tile, len(model.residue)), first_edges=rep(model.first_edges, None, edges_per_tile, nc),
                           end_first=rep(model.end_first, ("to",), nodes_per_tile, nc), end_last_rev=rep(model.end_last_rev, ("to",), nodes_per_tile, nc))


def tile_edges(edges, n_tiles, nodes_per_tile):
    out = np.tile(edges, n_tiles)
    shift = np.repeat(np.arange(n_tiles, dtype=np.uint64) * np.uint64(nodes_per_tile), len(edges))
    out["src"] += shift
    out["dst"] += shift
    return out
