"""tests/partition_model.py against a brute force, and the facts about the rule that the GPU cases of tests/test_gpu_edge_partition.py
are built on (no GPU here)."""
import numpy as np
import pytest

from tests.partition_model import HASH, SHARE, components, hash_file, partition_model


def _random_graph(rng):
    n = int(rng.integers(1, 41))
    ne = int(rng.integers(0, 3 * n + 1))
    src, dst = rng.integers(0, n, ne), rng.integers(0, n, ne)   # self-loops and src > dst as they fall
    if ne > 2:   # duplicates, in both directions
        k = int(rng.integers(0, ne // 2 + 1))
        pick = rng.integers(0, ne, k)
        swap = rng.random(k) < 0.5
        src = np.concatenate([src, np.where(swap, dst[pick], src[pick])])
        dst = np.concatenate([dst, np.where(swap, src[pick], dst[pick])])
    return n, src.astype(np.int64), dst.astype(np.int64)


def _bfs_roots(n, src, dst):
    adj = [set() for _ in range(n)]
    for a, b in zip(src.tolist(), dst.tolist()):
        adj[a].add(b)
        adj[b].add(a)
    root = [-1] * n
    for s in range(n):   # ascending: the first node that reaches a component is its smallest
        if root[s] >= 0:
            continue
        root[s], todo = s, [s]
        while todo:
            nxt = []
            for v in todo:
                for w in adj[v]:
                    if root[w] < 0:
                        root[w] = s
                        nxt.append(w)
            todo = nxt
    return np.asarray(root, dtype=np.int64)


GRAPHS = [_random_graph(np.random.default_rng(1000 + i)) for i in range(300)]


def test_components_equal_a_breadth_first_search():
    seen_loop = seen_dup = seen_down = 0
    for n, src, dst in GRAPHS:
        want = _bfs_roots(n, src, dst)
        assert np.array_equal(components(src, dst, n), want)
        _, info = partition_model(src, dst, n, 3)
        assert np.array_equal(info["root_of_node"], want)
        assert np.array_equal(info["cnt"], np.bincount(want[src], minlength=n)) and info["cnt"].sum() == len(src)
        assert info["n_components"] == len(np.unique(want[src]))
        seen_loop += int((src == dst).any())
        seen_down += int((src > dst).any())
        seen_dup += int(len(set(zip(src.tolist(), dst.tolist()))) < len(src))
    assert min(seen_loop, seen_dup, seen_down) > 100   # the inputs really hold what they are meant to


@pytest.mark.parametrize("n_files", [1, 2, 7, 256])
def test_invariants_of_the_rule(n_files):
    rng = np.random.default_rng(n_files)
    for n, src, dst in GRAPHS:
        ne = len(src)
        f, info = partition_model(src, dst, n, n_files)
        assert f.dtype == np.uint16 and len(f) == ne and (ne == 0 or f.max() < n_files)
        root, cnt = info["root_of_node"], info["cnt"]
        assert info["thr"] == max(ne // (SHARE * n_files), 1)
        assert info["n_big"] == int((cnt >= info["thr"]).sum())
        # the file is a function of the root
        assert np.array_equal(f, info["file_of_root"][root[src]]) and np.array_equal(f, info["file_of_root"][root[dst]])
        # of the SET of edges: any order, either direction
        p = rng.permutation(ne)
        assert np.array_equal(partition_model(src[p], dst[p], n, n_files)[0], f[p])
        sw = rng.random(ne) < 0.5
        assert np.array_equal(partition_model(np.where(sw, dst, src), np.where(sw, src, dst), n, n_files)[0], f)
        # the deal: sizes never grow, equal sizes by root, each to the lightest file (lowest index on ties) — replayed the slow way
        big, sizes = info["big_roots"], cnt[info["big_roots"]]
        assert np.all(np.diff(sizes) <= 0) and np.all((np.diff(sizes) < 0) | (np.diff(big) > 0))
        load = np.zeros(n_files, dtype=np.int64)
        for r, c, t, met in zip(big.tolist(), sizes.tolist(), info["big_files"].tolist(), info["loads_met"].tolist()):
            assert t == int(np.argmin(load)) and met == load[t]
            load[t] += c
        assert np.all(np.diff(info["loads_met"]) >= 0)   # the lightest file only ever gets heavier
        assert np.array_equal(load, np.bincount(f[cnt[root[src]] >= info["thr"]], minlength=n_files))
        # everything else by the hash of its root
        small = cnt[root[src]] < info["thr"]
        want = ((root[src][small] * HASH) % 2**32 * n_files) >> 32
        assert np.array_equal(f[small], want.astype(np.uint16))


def test_root_of_node_argument_replaces_the_union_find():
    for n, src, dst in GRAPHS[:50]:
        f, info = partition_model(src, dst, n, 5)
        g, _ = partition_model(src, dst, n, 5, root_of_node=info["root_of_node"])
        assert np.array_equal(f, g)


def test_hash_spreads_over_every_file():
    for nf in (1, 2, 7, 200, 65534):
        f = hash_file(np.arange(1 << 18), nf)
        assert f.max() == nf - 1 and f.min() == 0 and len(np.unique(f)) == min(nf, 1 << 18)


@pytest.mark.parametrize("size,n_files,n_comp,old_list", [(1, 2, 255, 192), (2, 3, 287, 256)])
def test_more_big_components_than_64_per_file(size, n_files, n_comp, old_list):
    """the regime in which a list of 64 * n_files + 64 entries cannot hold the components that the rule deals out by size: disjoint paths
    of `size` edges, one edge short of the next threshold"""
    ne = n_comp * size
    assert ne == (size + 1) * SHARE * n_files - size and old_list == SHARE * n_files + SHARE
    first = np.arange(n_comp, dtype=np.int64) * (size + 1)
    src = (first[:, None] + np.arange(size)).ravel()
    f, info = partition_model(src, src + 1, n_comp * (size + 1), n_files)
    assert info["thr"] == size and info["n_components"] == n_comp
    assert info["n_big"] == n_comp > old_list
    # equal sizes, so dealt out round robin in root order
    assert np.array_equal(f.reshape(n_comp, size)[:, 0], np.arange(n_comp) % n_files)
