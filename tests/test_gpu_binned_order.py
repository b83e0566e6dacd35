"""-m gpu : the binned grouping (disco_hip.hip, binned_build_order) — the processing order as a radix partition of one item per read by
order bucket and one workgroup per partition, instead of a counting atomic per read, a memset and a scan of the counter table and a
scattered write. Results do not depend on the order, so parity alone cannot show a grouping that stopped grouping: the order itself is
looked at through disco_fetch_order. Yardsticks: the oracle, and the old path (DISCO_NO_BINNED_ORDER=1) in the same process."""
import functools

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.util import assert_parity, canon_hip

pytestmark = pytest.mark.gpu
_COMP = str.maketrans("ACGT", "TGCA")

# mirrored from disco_kernels.h
BINX_BUILD_BLOCK = 1024  # items per step of the build kernel's sweeps (its tile)
BINX_TILE = 2048         # items per tile of a partition level
ORDER_MULT = 0x9E3779B1  # ORDER_BUCKET(key, shift) = (key * ORDER_MULT mod 2^32) >> shift


@pytest.fixture(autouse=True)
def _binned_at_every_size(monkeypatch):
    """the library takes the binned grouping from 2^21 reads up (a size policy: below, its launches cost what it saves); the sets here are
    smaller"""
    monkeypatch.setenv("DISCO_BINNED_ORDER_MIN_READS", "1")


def _rc(s):
    return s.translate(_COMP)[::-1]


@functools.lru_cache(maxsize=None)
def sampled_reads(seed, n, read_len=150, cov=30.0, len_lo=0, lens=None):
    """n reads off a random genome, either strand; lengths: read_len, or uniform in [len_lo, read_len], or drawn from `lens`"""
    rng = np.random.default_rng(seed)
    G = max(int(n * read_len / cov), read_len + 1)
    genome = "".join(rng.choice(list("ACGT"), G))
    starts = rng.integers(0, G - read_len + 1, n)
    flips = rng.random(n) < 0.5
    if lens is not None:
        ls = rng.choice(np.asarray(lens), n)
    elif len_lo:
        ls = rng.integers(len_lo, read_len + 1, n)
    else:
        ls = np.full(n, read_len)
    return tuple(_rc(genome[p:p + l]) if f else genome[p:p + l] for p, l, f in zip(starts, ls, flips))


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _unenv(monkeypatch, env):
    for k in env:
        monkeypatch.delenv(k, raising=False)


# ---- the order itself -----------------------------------------------------------------------------------------------------------
def _order(reads, monkeypatch, env):
    _env(monkeypatch, env)
    try:
        with buildgraph.BuildGraph(min_overlap=40) as g:
            g.upload_ascii(list(reads))
            g.build_index()
            return g.fetch_order()
    finally:
        _unenv(monkeypatch, env)


def _buckets(keys, bits):
    return ((keys.astype(np.uint64) * np.uint64(ORDER_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def _check_order(reads, monkeypatch, env, want_bits=None):
    n = len(reads)
    order, keys, bits = _order(reads, monkeypatch, env)
    old_order, old_keys, old_bits = _order(reads, monkeypatch, dict(env, DISCO_NO_BINNED_ORDER="1"))
    assert bits == old_bits and (want_bits is None or bits == want_bits), (bits, old_bits, want_bits)
    assert len(order) == len(keys) == n and np.array_equal(keys, old_keys)
    ids = (order & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(n)), "the order is no permutation of the reads"
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    assert np.array_equal((order >> np.uint64(32)).astype(np.int64), lens[ids]), "a length field is not its read's length"
    b = _buckets(keys, bits)[ids]  # the buckets in processing order
    starts = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
    assert len(starts) == len(np.unique(b)), "reads of one bucket are not contiguous"
    # the same reads per bucket as the old path: both orders sorted by (bucket, id) are one list (inside a bucket the order is free)
    old_ids = (old_order & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ob = _buckets(keys, bits)[old_ids]
    assert np.array_equal(ids[np.lexsort((ids, b))], old_ids[np.lexsort((old_ids, ob))])
    # ... and the old path walks the buckets in ascending order: so does the partition
    assert np.all(np.diff(b[starts].astype(np.int64)) > 0)


@pytest.mark.parametrize("n", [300, 5000])
def test_the_order_groups(n, monkeypatch):
    _check_order(sampled_reads(n, n), monkeypatch, {"DISCO_ORDER_MIN_READS": "1"}, 16)


@pytest.mark.parametrize("bits", [16, 22, 23, 26])
def test_the_order_groups_through_one_and_two_levels(bits, monkeypatch):
    """20 000 reads: a level of 2 bits (2^16 buckets), one of 8 (2^22), two levels (2^23: 5 + 4 bits, 2^26: 6 + 6)"""
    _check_order(sampled_reads(20, 20_000), monkeypatch, {"DISCO_ORDER_BITS": str(bits)}, bits)


def test_no_order_is_a_state_error(monkeypatch):
    monkeypatch.setenv("DISCO_NO_ORDER", "1")
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(list(sampled_reads(5000, 5000)))
        g.build_index()
        with pytest.raises(Exception):
            g.fetch_order()


@pytest.mark.parametrize("tile", [BINX_TILE, BINX_BUILD_BLOCK])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_edges(tile, delta, monkeypatch):
    n = tile + delta
    env = {"DISCO_ORDER_BITS": "23", "DISCO_ORDER_MIN_READS": "1"}
    reads = sampled_reads(100 + n, n)
    _check_order(reads, monkeypatch, env, 23)
    _env(monkeypatch, env)
    assert_parity(list(reads), 40, f"binned grouping, {n} reads")


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
def test_one_bucket_with_more_items_than_a_tile(monkeypatch):
    """copies of one read and of its reverse complement: one order bucket holds more items than a tile of a level and of the build kernel,
    every other partition is nearly empty"""
    base = list(sampled_reads(7, 1500))
    reads = base + [base[0]] * 2000 + [_rc(base[0])] * 1000
    assert 3000 > BINX_TILE > BINX_BUILD_BLOCK
    perm = np.random.default_rng(8).permutation(len(reads))
    reads = [reads[i] for i in perm]
    assert_parity(reads, 40, "binned grouping, skew")
    _check_order(tuple(reads), monkeypatch, {"DISCO_ORDER_BITS": "23"}, 23)


def test_mixed_lengths_inside_a_wavefront():
    """lengths uniform in 41..256: a read must be longer than min-overlap (validate_len_kernel, as in the reference), so 41 = k + 2 is the
    shortest there is"""
    c = assert_parity(list(sampled_reads(61, 2000, read_len=256, len_lo=41)), 40, "lengths 41..256")
    assert c["e_out"] > 0


def test_lengths_at_the_block_edges_of_the_count_pass():
    """min-overlap 40: k = 39, windows of nf = 17 m-mers; lengths k + 2 (the shortest a read may be: no read has 0 windows ahead of its
    suffix k-mer's), k + nf - 1, k + nf, k + 2 nf: 2, 16, 17 and 34 windows — the rolling pass ends inside its first block, one short of a
    block, on a block, two blocks on"""
    k, nf = 39, 17
    c = assert_parity(list(sampled_reads(62, 2000, read_len=k + 2 * nf, cov=60.0, lens=(k + 2, k + nf - 1, k + nf, k + 2 * nf))), 40, "pinned lengths")
    assert c["kmer_hits"] > 0


@pytest.mark.parametrize("min_overlap", [33, 66])
def test_run_time_windows(min_overlap):
    c = assert_parity(list(sampled_reads(min_overlap, 2000, read_len=256, len_lo=min_overlap + 1)), min_overlap, f"min-overlap {min_overlap}, mixed lengths")
    assert c["e_out"] > 0


def test_two_classes_of_rows_keep_the_counting_form():
    spec = readgen.GenSpec.coverage(seed=77, n_reads=6000, read_len=150, cov=30.0, long_len=600, long_share=1300)
    reads = readgen.generate_reads(spec)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        g.run_graph()
        assert g.long_rows > 50
    assert_parity(reads, 40, "two classes")


# ---- against the old path -------------------------------------------------------------------------------------------------------
def _outputs(load, passes=1):
    with buildgraph.BuildGraph(min_overlap=40) as g:
        load(g)
        for _ in range(passes):
            g.run_graph()
        c = g.counters()
        c.pop("hbm_bytes")  # (the old path's counter table and slots)
        return canon_hip(g.fetch_edges(), g.fetch_contained()), c


def _same(a, b, label=""):
    assert np.array_equal(a[0][0], b[0][0]), f"{label}: edges differ"
    assert np.array_equal(a[0][1], b[0][1]), f"{label}: contained rows differ"
    assert a[1] == b[1], f"{label}: counters differ"


def _both_paths(load, monkeypatch, label=""):
    new = _outputs(load)
    monkeypatch.setenv("DISCO_NO_BINNED_ORDER", "1")
    old = _outputs(load)
    monkeypatch.delenv("DISCO_NO_BINNED_ORDER")
    _same(new, old, label)
    assert new[1]["e_out"] > 0
    return new


def test_device_generator(monkeypatch):
    spec = readgen.GenSpec.coverage(seed=5, n_reads=200_000, read_len=150, cov=30.0)
    _both_paths(lambda g: g.generate_reads(spec), monkeypatch, label="generated")


def test_chunked_upload_writes_its_items_behind_the_copies(monkeypatch):
    reads = list(sampled_reads(21, 12000))
    monkeypatch.setenv("DISCO_UPLOAD_CHUNK", "256")
    chunked = _both_paths(lambda g: g.upload_ascii(reads), monkeypatch, label="chunked upload")
    _check_order(tuple(reads), monkeypatch, {}, 16)
    monkeypatch.delenv("DISCO_UPLOAD_CHUNK")
    _same(chunked, _outputs(lambda g: g.upload_ascii(reads)), "chunked against one chunk")


def test_context_reuse(monkeypatch):
    """big, small, tiny, big again in one context, two passes each: no stale segment table, item buffer or order leaks in"""
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    big = readgen.GenSpec.coverage(seed=31, n_reads=40_000, read_len=150, cov=30.0)
    small = readgen.GenSpec.coverage(seed=32, n_reads=9_000, read_len=150, cov=30.0)
    tiny = list(sampled_reads(33, 300))
    want = [_outputs(lambda g: g.generate_reads(big)), _outputs(lambda g: g.generate_reads(small)), _outputs(lambda g: g.upload_ascii(tiny))]
    with buildgraph.BuildGraph(min_overlap=40) as g:
        for load, w in ((lambda: g.generate_reads(big), want[0]), (lambda: g.generate_reads(small), want[1]), (lambda: g.upload_ascii(tiny), want[2]),
                        (lambda: g.generate_reads(big), want[0])):
            load()
            for _ in range(2):
                g.run_graph()
                c = g.counters()
                c.pop("hbm_bytes")
                _same((canon_hip(g.fetch_edges(), g.fetch_contained()), c), w, "reused context")
                order, _keys, _bits = g.fetch_order()
                assert np.array_equal(np.sort(order & np.uint64(0xFFFFFFFF)), np.arange(len(order), dtype=np.uint64))
    monkeypatch.setenv("DISCO_NO_BINNED_ORDER", "1")
    _same(_outputs(lambda g: g.generate_reads(small)), want[1], "old path")


# ---- a clock --------------------------------------------------------------------------------------------------------------------
def _index_order_ms(n, env, monkeypatch):
    _env(monkeypatch, env)
    try:
        spec = readgen.GenSpec.coverage(42, n, 150, 30.0)
        with buildgraph.BuildGraph(min_overlap=40, device=0) as g:
            g.generate_reads(spec)
            g.run_graph()  # allocations
            g.run_graph()
            g.synchronize()
            ph = g.phase_ms()
            return ph["index"] + ph["order"], g.counters()
    finally:
        _unenv(monkeypatch, env)


def test_the_binned_grouping_keeps_its_factor_to_the_old_path(monkeypatch):
    """3 M reads, second pass of each context, same process: index + order with the binned grouping against the same phases on the old
    path. It catches a serialisation (a partition walked by one lane, a contended counter: a factor of several); it does not certify a gain"""
    new, cn = _index_order_ms(3_000_000, {}, monkeypatch)
    old, co = _index_order_ms(3_000_000, {"DISCO_NO_BINNED_ORDER": "1"}, monkeypatch)
    print(f"index + order at 3 M reads: binned grouping {new:.3f} ms, old path {old:.3f} ms, ratio {new / old:.3f}")
    assert cn["e_out"] == co["e_out"] and cn["kmer_hits"] == co["kmer_hits"]
    # the factor of the binned-index guard: the two paths are level at this size, 1.8 is the head-room the other guards give a small or busy box
    assert new < 1.8 * old, (new, old)
