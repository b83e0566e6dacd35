"""The rule that cuts the edge files, restated in a few lines of numpy from the comment above partition_edges
(disco_amd/csrc/disco_hip.hip) — what disco_fetch_edge_files, disco_partition_edges and disco_dist_format_edges promise: the file of
an edge depends on the SET of edges only.

  1. a component's root is its smallest read id
  2. its size cnt[root] is its number of edges (duplicates and self-loops count)
  3. thr = max(ne // (SHARE * n_files), 1)
  4. the components with cnt >= thr, in (size descending, root ascending) order,
  5. each go to the file with the smallest load so far (lowest index on ties), and add their size to it
  6. every other edge goes to file (((root * HASH) mod 2^32) * n_files) >> 32
"""
import heapq

import numpy as np

SHARE = 64           # a component of at least 1 / (SHARE * n_files) of the edges is dealt out by size
HASH = 0x9E3779B1    # multiplier of the hash that spreads the smaller components


def components(src, dst, n_nodes):
    """root_of_node[v] = smallest id of v's component: a plain union-find (fine up to a few 10^5 edges)"""
    parent = list(range(n_nodes))
    for a, b in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    root = np.asarray(parent, dtype=np.int64).reshape(n_nodes)
    while True:   # the smaller root always wins, so parents only point downwards: pointer jumping ends at the smallest id
        nxt = root[root]
        if np.array_equal(nxt, root):
            return root
        root = nxt


def hash_file(root, n_files):
    r = np.asarray(root).astype(np.uint64)
    return ((((r * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)) * np.uint64(n_files)) >> np.uint64(32)).astype(np.uint16)


def partition_model(src, dst, n_nodes, n_files, root_of_node=None):
    """(file_of_edge: uint16[ne], info). root_of_node: the smallest id of every node's component, for constructed graphs whose
    components are known (a node without edges is its own root)"""
    src = np.asarray(src).astype(np.int64)
    dst = np.asarray(dst).astype(np.int64)
    ne = len(src)
    assert len(dst) == ne and 0 < n_files < 0xFFFF
    assert ne == 0 or (min(src.min(), dst.min()) >= 0 and max(src.max(), dst.max()) < n_nodes)
    root = components(src, dst, n_nodes) if root_of_node is None else np.asarray(root_of_node).astype(np.int64)
    assert len(root) == n_nodes
    edge_root = root[src]
    cnt = np.bincount(edge_root, minlength=n_nodes).astype(np.int64)
    thr = max(ne // (SHARE * n_files), 1)
    big = np.flatnonzero(cnt >= thr)
    big = big[np.lexsort((big, -cnt[big]))]
    file_of_root = hash_file(np.arange(n_nodes), n_files)
    heap = [(0, f) for f in range(n_files)]   # sorted, so a heap already
    big_files = np.zeros(len(big), dtype=np.uint16)
    loads_met = np.zeros(len(big), dtype=np.int64)
    for k, (r, c) in enumerate(zip(big.tolist(), cnt[big].tolist())):
        load, f = heap[0]
        heapq.heapreplace(heap, (load + c, f))
        big_files[k], loads_met[k] = f, load
    file_of_root[big] = big_files
    info = dict(thr=thr, n_big=len(big), n_components=int(np.count_nonzero(cnt)), cnt=cnt, root_of_node=root,
                big_roots=big, big_files=big_files, loads_met=loads_met, file_of_root=file_of_root)
    return file_of_root[edge_root].astype(np.uint16), info
