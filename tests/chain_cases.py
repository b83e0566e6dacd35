"""Edge arrays for the chain contraction's tests (tests/test_chain_model.py on the CPU, tests/test_gpu_chain_model.py on the device):
graphs written down as walks over node ids, turned into buildgraph.EDGE_DTYPE records that are consistent with a table of read
lengths — 0 < offset < len(src), and 0 < the reverse offset < len(dst).

An edge end has a SIDE: bit 1 of the orientation of the half-edge that leaves the node through it. For an edge stored src -> dst with
orientation o that is (o >> 1) & 1 at src and (o & 1) ^ 1 at dst (the twin's bit 1). A node of two edges is absorbable iff the sides differ."""
import numpy as np

from disco_amd.buildgraph import EDGE_DTYPE

N_READS = 66_000        # the reads of the device tests' context: ids 0 .. N_READS - 1 with these lengths
LENGTHS = np.random.default_rng(20).integers(100, 251, N_READS).astype(np.int64)
MIN_OVL = 50            # min_overlap_simplify of the constructed cases; their edges overlap by at least that unless a case says otherwise


def make_edges(lengths, u, v, su, sv, rng, flip=None, ov_lo=MIN_OVL, ov_hi=None, overlap=None):
    """one edge per entry between the nodes u and v, meeting u on side su and v on side sv; stored v -> u where flip (default: a coin).
    Overlap: `overlap` where given (>= 0), else uniform in [ov_lo, min(ov_hi, both lengths - 1)]"""
    u, v, su, sv = (np.asarray(x).astype(np.int64).reshape(-1) for x in (u, v, su, sv))
    n = len(u)
    flip = rng.integers(0, 2, n).astype(bool) if flip is None else np.broadcast_to(np.asarray(flip, dtype=bool), n)
    src, dst = np.where(flip, v, u), np.where(flip, u, v)
    s_src, s_dst = np.where(flip, sv, su), np.where(flip, su, sv)
    top = np.minimum(lengths[src], lengths[dst]) - 1
    if ov_hi is not None:
        top = np.minimum(top, ov_hi)
    ov = rng.integers(np.minimum(ov_lo, top), top + 1)
    if overlap is not None:
        given = np.broadcast_to(np.asarray(overlap).astype(np.int64), n)
        ov = np.where(given >= 0, given, ov)
    assert (ov >= 1).all() and (ov <= np.minimum(lengths[src], lengths[dst]) - 1).all()
    e = np.zeros(n, dtype=EDGE_DTYPE)
    e["src"], e["dst"] = src, dst
    e["orient"] = (s_src << 1) | (s_dst ^ 1)
    e["offset"] = lengths[src] - ov
    e["len_src"], e["len_dst"] = lengths[src], lengths[dst]
    return e


def walk(lengths, nodes, rng, closed=False, same_side_at=(), **kw):
    """the edges of the walk nodes[0] - nodes[1] - ... (closed: and back to nodes[0]); every inner node gets its two edges on opposite
    sides, except the positions in same_side_at, where both meet the same side"""
    nodes = np.asarray(nodes).astype(np.int64)
    t = rng.integers(0, 2, len(nodes))
    u, tu = nodes[:-1], t[:-1]
    v, tv = nodes[1:], t[1:]
    if closed:
        u, tu, v, tv = nodes, t, np.roll(nodes, -1), np.roll(t, -1)
    su = 1 - tu
    for k in same_side_at:          # the edge that leaves position k takes the side the one before it came in on
        su[k] = t[k]
    return make_edges(lengths, u, v, su, tv, rng, **kw)


def ordered(edges, order, rng):
    if order == "descending":
        return edges[::-1].copy()
    if order == "shuffled":
        return edges[rng.permutation(len(edges))]
    assert order == "ascending"
    return edges


def paths(lengths, n_edges_each, rng, first_node=0):
    """disjoint paths of the given numbers of edges over consecutive node ids: (edges, next free node)"""
    out, at = [], first_node
    for L in n_edges_each:
        out.append(walk(lengths, np.arange(at, at + L + 1), rng))
        at += L + 1
    return np.concatenate(out), at


def random_multigraph(seed, lengths=LENGTHS):
    """(edges, min_overlap_simplify): up to 40 nodes of degree <= 4 anywhere in the table, with self-loops and parallel edges, stored
    either way round, sides at random, and a filter that bites"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 41))
    ids = rng.choice(len(lengths), n, replace=False)
    deg = np.zeros(n, dtype=np.int64)
    us, vs = [], []
    for _ in range(int(rng.integers(1, 2 * n + 1))):
        a, b, r = int(rng.integers(0, n)), int(rng.integers(0, n)), rng.random()
        if r < 0.08:
            b = a                                   # a self-loop
        elif r < 0.2 and us:
            k = int(rng.integers(0, len(us)))       # beside an edge that is there already
            a, b = vs[k], us[k]
        elif r < 0.55 and us:
            a = vs[-1]                              # on from where the last edge ended: paths grow
        if (deg[a] + 2 > 4) if a == b else (deg[a] + 1 > 4 or deg[b] + 1 > 4):
            continue
        deg[a] += 1
        deg[b] += 1
        us.append(a)
        vs.append(b)
    if not us:
        us, vs = [0], [1]
    # two in three of the nodes take their edge ends on alternating sides, so that chains of some length form; the rest at random
    alternate = rng.random(n) < 0.67
    free = np.flatnonzero(deg == 0)
    if len(free) >= 2 and rng.random() < 0.4:       # a cycle over nodes nothing else touches: a ring where they all alternate
        cyc = free[:int(rng.integers(2, 7))].tolist()
        us += cyc
        vs += cyc[1:] + cyc[:1]
        alternate[cyc] = rng.random() < 0.8
    seen = np.zeros(n, dtype=np.int64)
    base = rng.integers(0, 2, n)
    su, sv = [], []
    for a, b in zip(us, vs):
        for x, s in ((a, su), (b, sv)):
            s.append(int((base[x] + seen[x]) & 1) if alternate[x] else int(rng.integers(0, 2)))
            seen[x] += 1
    min_ovl = int(rng.choice([0, 40, 70, 99, 130]))
    return make_edges(lengths, ids[us], ids[vs], su, sv, rng, ov_lo=1), min_ovl


RANDOM_SEEDS = range(1000, 1320)   # 320 multigraphs


TILE_NODES, TILE_EDGES = 48, 128


def tile(lengths):
    """a small pattern over the node ids 0 .. 47 in 128 array positions: paths, a ring, a branch node with three arms, a ring with a
    tail, a pair of parallel edges, a self-loop, forty parallel edges between two hubs, and edges the filter drops laid across all of
    them — in shuffled order. lengths: of those 48 nodes"""
    rng = np.random.default_rng(7)
    parts = [walk(lengths, range(0, 9), rng), walk(lengths, range(9, 12), rng), walk(lengths, range(12, 17), rng, closed=True),
             walk(lengths, [19, 18, 17, 20, 21], rng), walk(lengths, [17, 22, 23, 24], rng),
             walk(lengths, range(25, 29), rng, closed=True), walk(lengths, [25, 29], rng),
             walk(lengths, [30, 31], rng, closed=True), walk(lengths, [32, 32, 33], rng),
             make_edges(lengths, [34] * 40, [35] * 40, rng.integers(0, 2, 40), rng.integers(0, 2, 40), rng),
             walk(lengths, range(36, 48), rng, same_side_at=(5,))]
    real = np.concatenate(parts)
    n_drop = TILE_EDGES - len(real)
    assert n_drop > 20
    dropped = make_edges(lengths, rng.integers(0, TILE_NODES, n_drop), rng.integers(0, TILE_NODES, n_drop), rng.integers(0, 2, n_drop),
                         rng.integers(0, 2, n_drop), rng, ov_lo=1, ov_hi=MIN_OVL - 1)
    return ordered(np.concatenate([real, dropped]), "shuffled", rng)


# ---- read sets whose reduced graph holds what the constructed arrays hold, for the edges that stay on the device --------------------
_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def _sample(genomes, n, lmin, lmax, rng):
    """n reads of lmin .. lmax bases from (sequence, circular) genomes, either strand (as tools/fuzz_chains.py cuts them)"""
    out = []
    for _ in range(n):
        g, circular = genomes[int(rng.integers(0, len(genomes)))]
        L = int(rng.integers(lmin, lmax + 1))
        p = int(rng.integers(0, len(g) if circular else len(g) - L + 1))
        s = (g + g)[p:p + L] if circular else g[p:p + L]
        out.append(s.translate(_COMPLEMENT)[::-1] if rng.random() < 0.5 else s)
    return out


def _random_sequence(rng, k):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, k))


def circular_reads(seed=3):
    """~25x of a circular genome of 12 000 bases and of a linear one of 8 000: a ring of absorbable nodes beside chains"""
    rng = np.random.default_rng(seed)
    genomes = [(_random_sequence(rng, 12_000), True), (_random_sequence(rng, 8_000), False)]
    return _sample(genomes, 20_000 * 25 // 125, 100, 150, rng)


def tandem_reads(seed=4):
    """~25x of linear genomes with a tandem repeat longer than a read in them (units of 37 and 61 bases, 450 - 500 bases in all): reads
    inside the repeat overlap one another at several shifts — parallel edges, and two-rings of them"""
    rng = np.random.default_rng(seed)
    genomes = [(_random_sequence(rng, 4_000) + _random_sequence(rng, unit) * copies + _random_sequence(rng, 4_000), False) for unit, copies in ((37, 13), (61, 8))]
    return _sample(genomes, sum(len(g) for g, _ in genomes) * 25 // 125, 100, 150, rng)


def self_loops_and_parallel_pairs(edges):
    """(self-loops, pairs of nodes joined by more than one edge) of an edge array"""
    a, b = np.minimum(edges["src"], edges["dst"]).astype(np.int64), np.maximum(edges["src"], edges["dst"]).astype(np.int64)
    _, count = np.unique(np.stack([a, b], axis=1), axis=0, return_counts=True) if len(edges) else (None, np.zeros(0, dtype=np.int64))
    return int((a == b).sum()), int((count > 1).sum())
