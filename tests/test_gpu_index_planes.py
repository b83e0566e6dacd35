"""-m gpu : the binned index build over record PLANES (disco_kernels.h, "binned index build") — on the single-GPU path the count pass
leaves a 4-byte key plane and an 8-byte payload plane instead of 16-byte records, and the partition levels and the build kernel work on
the two. The index has no entry point of its own: kmer_hits equals the oracle's only if every record is found in its bucket. Two
yardsticks, as in test_gpu_binned_index.py: the oracle, and the old path (DISCO_NO_BINNED_INDEX=1, 16-byte records with a slot) in the
same process. The shapes are the smallest at which a plane layout can go wrong: every alignment of a segment or tile start in either
plane, an upload counted in many chunks, the second class of rows behind the first, a payload plane whose base moves with
the number of reads, and a bucket that spans tiles."""
import functools

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.test_gpu_binned_index import BINX_TILE, _outputs, _rc, _same, sampled_reads
from tests.util import canon_hip, run_hip_reads, run_oracle_reads

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reads(seed, n):
    return tuple(sampled_reads(seed, n))


@functools.lru_cache(maxsize=None)
def _oracle(key):
    """the oracle's canonical outputs and counters for a read set, computed once per set"""
    reads = _SETS[key]()
    oe, orows, oc = run_oracle_reads(list(reads), 40)
    return canon_hip(oe, orows), oc


def _skewed():
    """copies of one read and of its reverse complement among 1500 others: two buckets with more records than a tile each. 3053 copies,
    an odd number, 2051 of them forward: more than a tile of either strand"""
    base = list(_reads(7, 1500))
    reads = base + [base[0]] * 2051 + [_rc(base[0])] * 1002
    order = np.random.default_rng(8).permutation(len(reads))
    return tuple(reads[i] for i in order)


_SETS = {("sizes", n): (lambda n=n: _reads(100 + n, n)) for n in range(1500, 1508)}
_SETS[("skew",)] = _skewed


def _parity(key, label):
    """assert_parity's comparison (tests/util.py), with the oracle's side shared between the cases of a set"""
    reads = list(_SETS[key]())
    he, hr, hc = run_hip_reads(reads, 40)
    (oce, occ), oc = _oracle(key)
    ce, cc = canon_hip(he, hr)
    assert np.array_equal(cc, occ), f"{label}: contained rows differ ({len(cc)} vs {len(occ)})"
    assert np.array_equal(ce, oce), f"{label}: edge list differs ({len(ce)} vs {len(oce)})"
    for k in ("probes", "kmer_hits", "n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs"):
        assert hc[k] == oc[k], f"{label}: counter {k}: hip {hc[k]} oracle {oc[k]}"
    return hc


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["65536", "524288", "1048576"])
@pytest.mark.parametrize("n", range(1500, 1508))
def test_eight_consecutive_sizes(n, scale, monkeypatch):
    """2n = 3000 .. 3014 takes every even residue mod 16, and the segments of the second and third level start wherever the records
    fall: every alignment of a run in the 4-byte and in the 8-byte plane. Buckets per read: 65536 -> 2^27 buckets, two levels (7 + 6
    bits); 524288 -> 2^30, two levels of 8; 1048576 -> 2^31, three levels (6 + 6 + 5)"""
    monkeypatch.setenv("DISCO_BUCKET_SCALE", scale)
    c = _parity(("sizes", n), f"planes n = {n}, {scale} buckets per read")
    assert c["e_out"] > 0


def test_one_bucket_with_an_odd_number_of_records_above_a_tile(monkeypatch):
    monkeypatch.setenv("DISCO_BUCKET_SCALE", "65536")  # 4553 reads: 2^29 buckets, two levels
    assert 2051 > BINX_TILE
    _parity(("skew",), "planes skew")


# ---- against the old path -------------------------------------------------------------------------------------------------------
def _old_path(load, monkeypatch):
    monkeypatch.setenv("DISCO_NO_BINNED_INDEX", "1")
    old = _outputs(load)
    monkeypatch.delenv("DISCO_NO_BINNED_INDEX")
    return old


def test_odd_upload_chunks(monkeypatch):
    """the eager count of an upload writes the planes chunk by chunk, at record offsets 2 lo (IndexRecOut::from_read). The upload rounds
    DISCO_UPLOAD_CHUNK up to a multiple of 256 reads, so 255 runs as 256 (47 chunks) and 257 as 512 (24 chunks): every chunk starts at a
    read that is a multiple of 256 and both planes stay 16-byte aligned there. A record offset = 2 mod 4 therefore cannot be produced
    through the library (index_put_pair's stores are 8- and 16-byte aligned at any read all the same); what this holds is many chunks of
    two sizes against one chunk and against the old path"""
    reads = list(_reads(21, 12000))

    def load(g):
        g.upload_ascii(reads)

    one = _outputs(load)
    assert one[1]["e_out"] > 0
    _same(one, _old_path(load, monkeypatch), "one chunk against the old path")
    for chunk in ("255", "257"):
        monkeypatch.setenv("DISCO_UPLOAD_CHUNK", chunk)
        _same(_outputs(load), one, f"chunks of {chunk} against one chunk")
        monkeypatch.delenv("DISCO_UPLOAD_CHUNK")


def test_long_class_writes_planes_behind_the_short_class(monkeypatch):
    spec = readgen.GenSpec.coverage(seed=77, n_reads=20_000, read_len=150, cov=30.0, long_len=600, long_share=1300)

    def load(g):
        g.generate_reads(spec)

    new = _outputs(load)
    assert new[1]["e_out"] > 0
    _same(new, _old_path(load, monkeypatch), "two classes")
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        assert g.long_rows > 100


def test_serial_count_kernel_writes_planes(monkeypatch):
    """DISCO_NO_RUNS=1: index_count_kernel instead of index_runs_kernel, for every read"""
    reads = list(_reads(1, 5000))

    def load(g):
        g.upload_ascii(reads)

    monkeypatch.setenv("DISCO_NO_RUNS", "1")
    new = _outputs(load)
    assert new[1]["e_out"] > 0
    _same(new, _old_path(load, monkeypatch), "no runs")
    monkeypatch.delenv("DISCO_NO_RUNS")
    _same(new, _outputs(load), "no runs against runs")


def test_context_reuse_across_sizes():
    """the planes are cut from the scratch by the number of reads: 40 000 reads, 9 000, 300 uploaded, 40 000 again in ONE context, each
    pass equal to a fresh context's"""
    big = readgen.GenSpec.coverage(seed=31, n_reads=40_000, read_len=150, cov=30.0)
    small = readgen.GenSpec.coverage(seed=32, n_reads=9_000, read_len=150, cov=30.0)
    tiny = list(_reads(33, 300))
    want = [_outputs(lambda g: g.generate_reads(big)), _outputs(lambda g: g.generate_reads(small)), _outputs(lambda g: g.upload_ascii(tiny))]
    assert all(w[1]["e_out"] > 0 for w in want)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        for load, w in ((lambda: g.generate_reads(big), want[0]), (lambda: g.generate_reads(small), want[1]), (lambda: g.upload_ascii(tiny), want[2]),
                        (lambda: g.generate_reads(big), want[0])):
            load()
            g.run_graph()
            c = g.counters()
            c.pop("hbm_bytes")
            _same((canon_hip(g.fetch_edges(), g.fetch_contained()), c), w, "reused context")
