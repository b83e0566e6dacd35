"""CPU: what bench.py --dump-outputs writes — the edge rows in the oracle's canonical form, a read sample that does not depend on
the order a build emits its rows in, float64 files within the size limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from disco_amd.buildgraph import CONTAINED_DTYPE, EDGE_DTYPE  # noqa: E402
from oracle import pyoracle  # noqa: E402


def _edges(rng, n_reads, m):
    e = np.zeros(m, dtype=EDGE_DTYPE)
    e["src"], e["dst"] = rng.integers(0, n_reads, m), rng.integers(0, n_reads, m)
    e["orient"], e["offset"] = rng.integers(0, 4, m), rng.integers(1, 100, m)
    e["len_src"], e["len_dst"] = 150, rng.integers(100, 200, m)
    return e


class _Graph:
    def __init__(self, edges, rows):
        self.edges, self.rows = edges, rows

    def fetch_edges(self):
        return self.edges

    def fetch_contained(self):
        return self.rows


def test_edge_rows_are_the_oracles_canonical_edges():
    e = _edges(np.random.default_rng(1), 5000, 20000)
    ref = pyoracle.canonical_edges(e["src"], e["dst"], e["orient"], e["offset"], e["len_src"], e["len_dst"])
    assert np.array_equal(bench.canonical_edge_rows(e), ref)
    assert np.array_equal(bench.canonical_edge_rows(e[::-1]), ref)
    assert bench.canonical_edge_rows(e[:0]).shape == (0, 7)


def test_read_sample_is_fixed_and_order_free():
    rng = np.random.default_rng(2)
    n = 64 * bench.DUMP_SAMPLE_READS
    ids = rng.integers(0, n, 400_000)
    m = bench.sampled_reads(ids, n, 42)
    assert 0.5 / 64 < m.mean() < 2.0 / 64
    perm = rng.permutation(len(ids))
    assert np.array_equal(bench.sampled_reads(ids[perm], n, 42), m[perm])
    assert np.array_equal(bench.sampled_reads(ids, n, 42), m) and not np.array_equal(bench.sampled_reads(ids, n, 43), m)
    assert bench.sampled_reads(np.arange(1000), bench.DUMP_SAMPLE_READS, 42).all()  # a small run keeps every read


def test_dump_files(tmp_path):
    rng = np.random.default_rng(3)
    n = 4 * bench.DUMP_SAMPLE_READS
    rows = np.zeros(3000, dtype=CONTAINED_DTYPE)
    rows["contained"], rows["super"], rows["len2"], rows["len1"] = rng.integers(0, n, 3000), rng.integers(0, n, 3000), 90, 150
    e = _edges(rng, n, 200_000)
    # two ranks holding halves of the results write what one rank holding all of them writes
    bench.dump_outputs(tmp_path / "one", [7, 5, 3, 0, 0], [bench.dump_sample(_Graph(e, rows), n, 42)])
    bench.dump_outputs(tmp_path / "two", [7, 5, 3, 0, 0], [bench.dump_sample(_Graph(e[1::2], rows[:1000]), n, 42),
                                                           bench.dump_sample(_Graph(e[::2], rows[1000:]), n, 42)])
    total = 0
    for f in ("counts", "edges", "contained"):
        a, b = np.load(tmp_path / "one" / (f + ".npy")), np.load(tmp_path / "two" / (f + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, b), f
        total += os.path.getsize(tmp_path / "one" / (f + ".npy"))
    assert total <= 64 << 20
    edges = np.load(tmp_path / "one" / "edges.npy")
    assert edges.shape[1] == 7 and 0 < len(edges) < len(e) and (edges[:, 0] <= edges[:, 1]).all()
    assert np.load(tmp_path / "one" / "counts.npy").tolist() == [7, 5, 3, 0, 0]
    assert np.load(tmp_path / "one" / "contained.npy").shape[1] == 6
