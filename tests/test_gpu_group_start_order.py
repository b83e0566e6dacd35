"""-m gpu : the sub-key of the binned grouping (disco_kernels.h, ORDER_SUBKEY) — inside an order bucket the reads lie in the order of
their start against the minimizer their group shares, so that neighbours in the processing order overlap most. No result depends on the
order: the order itself is looked at through disco_fetch_order and held to a numpy statement of the sub-key (include/disco_hip_inspect.h,
disco_set_order_sub_bits) and to the old path (DISCO_NO_BINNED_ORDER=1); results to the oracle."""
import functools

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.util import assert_parity, canon_hip, low_complexity

pytestmark = pytest.mark.gpu

ORDER_MULT = 0x9E3779B1  # ORDER_BUCKET(key, shift) = (key * ORDER_MULT mod 2^32) >> shift   (disco_kernels.h)
ORDER_SUB_MAX = 3        # at most three bits of sub-key
M = 23                   # the minimizer length of every k from 23 to 86 (disco_minimizer_len)
_U = np.uint64
_COMP = str.maketrans("ACGT", "TGCA")


@pytest.fixture(autouse=True)
def _binned_at_every_size(monkeypatch):
    """the library takes the binned grouping from 2^21 reads up (a size policy); the sets here are smaller"""
    monkeypatch.setenv("DISCO_BINNED_ORDER_MIN_READS", "1")
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")


# ---- the sub-key in numpy ---------------------------------------------------------------------------------------------------------
def _umul24(a, b):
    return ((a & _U(0xFFFFFF)) * _U(b)) & _U(0xFFFFFFFF)


def order_hash23(c):
    """order_hash32(canonical m-mer) >> 9 (disco_device.h; m <= 23: two 24-bit products fold the m-mer, two more mix the fold)"""
    h = (_umul24(c, 0x9E3779) + _umul24(c >> _U(24), 0x85EBCB) + _U(0x7F4A7C15)) & _U(0xFFFFFFFF)
    return ((_umul24(h, 0xC1B3C7) + _umul24(h >> _U(8), 0x9E3779)) & _U(0xFFFFFFFF)) >> _U(9)


def mmers(x, lsb_first):
    """x[:, p] = a base in 2 bits -> y[:, p] = the M bases from p on as one number, the first base on top (lsb_first: at the bottom); by
    doubling: 1, 2, 4, 8, 16 bases, then 23 = 16 + 4 + 2 + 1"""
    def cat(a, na, b, nb):  # na bases from p on, then nb bases from p + na on
        w = x.shape[1] - (na + nb) + 1
        a, b = a[:, :w], b[:, na:na + w]
        return (a | (b << _U(2 * na))) if lsb_first else ((a << _U(2 * nb)) | b)

    w = {1: x}
    for n in (1, 2, 4, 8):
        w[2 * n] = cat(w[n], n, w[n], n)
    out, have = w[16], 16
    for n in (4, 2, 1):
        out, have = cat(out, have, w[n], n), have + n
    assert have == M
    return out


def read_sub_keys(codes, off, qbits, longest):
    """(sub-key, smallest order hash >> 9) of every read, as include/disco_hip_inspect.h states them"""
    lens = (off[1:] - off[:-1]).astype(np.int64)
    n, lmax = len(lens), int(lens.max())
    x = np.zeros((n, lmax), dtype=np.uint64)
    rid = np.repeat(np.arange(n), lens)
    x[rid, np.arange(len(codes)) - off[:-1].astype(np.int64)[rid]] = codes
    f = mmers(x, False)
    r = mmers(_U(3) - x, True)  # the reverse complement: the complement of the LAST base on top
    rev = r < f
    h = order_hash23(np.where(rev, r, f))
    nmm = lens - M + 1
    h[np.arange(h.shape[1])[None, :] >= nmm[:, None]] = _U(1 << 40)  # (behind the read)
    pos = np.argmin(h, axis=1)  # the leftmost of equal ones
    rows = np.arange(n)
    start_rel = np.where(rev[rows, pos], nmm - 1 - pos, pos)
    mul = (1 << (qbits + 16)) // (longest - M + 1)
    return np.minimum((start_rel * mul) >> 16, (1 << qbits) - 1), h[rows, pos]


def expected_sub_bits(n, longest, bits):
    idb, lenb = 1, 1
    while (1 << idb) < n:
        idb += 1
    while (1 << lenb) <= longest:
        lenb += 1
    return max(0, min(64 - (bits + lenb + idb), ORDER_SUB_MAX))


# ---- the order ------------------------------------------------------------------------------------------------------------------------
def _order(spec, monkeypatch, env, sub_limit=-1):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        with buildgraph.BuildGraph(min_overlap=40) as g:
            g.generate_reads(spec)
            g.order_sub_bits(sub_limit)
            g.build_index()
            order, keys, bits = g.fetch_order()
            return (order & _U(0xFFFFFFFF)).astype(np.int64), keys, bits, g.order_sub_bits()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def _buckets(keys, bits):
    return (((keys.astype(np.uint64) * _U(ORDER_MULT)) & _U(0xFFFFFFFF)) >> _U(32 - bits)).astype(np.int64)


def _check_shape(spec, monkeypatch, env, sub_limit=-1):
    """permutation, the old path's reads per bucket, buckets ascending, sub-keys not decreasing inside a bucket; returns what the callers
    go on with"""
    n = spec.n_reads
    ids, keys, bits, qbits = _order(spec, monkeypatch, env, sub_limit)
    old_ids, old_keys, old_bits, old_q = _order(spec, monkeypatch, dict(env, DISCO_NO_BINNED_ORDER="1"))
    assert bits == old_bits and old_q == 0 and np.array_equal(keys, old_keys)
    assert np.array_equal(np.sort(ids), np.arange(n)), "the order is no permutation of the reads"
    bucket = _buckets(keys, bits)
    b, ob = bucket[ids], bucket[old_ids]
    assert np.all(np.diff(b) >= 0), "the buckets do not ascend"
    assert np.array_equal(ids[np.lexsort((ids, b))], old_ids[np.lexsort((old_ids, ob))]), "a bucket holds other reads than on the old path"
    codes, off = readgen.generate_codes(spec)
    longest = int((off[1:] - off[:-1]).max())
    want_q = expected_sub_bits(n, longest, bits) if sub_limit < 0 else min(sub_limit, expected_sub_bits(n, longest, bits))
    assert qbits == want_q, (qbits, want_q)
    sub, hmin = read_sub_keys(codes, off, qbits, longest)
    assert np.array_equal(hmin, (keys >> np.uint32(9)).astype(np.uint64)), "the numpy statement of the order hash is not the kernels'"
    s = sub[ids]
    inside = b[1:] == b[:-1]
    if qbits:
        assert np.all(np.diff(s)[inside] >= 0), "inside a bucket a sub-key decreases"
        assert len(np.unique(sub)) == 1 << qbits, "the sub-key does not use its bits"
    return ids, old_ids, b, ob


def _neighbour_gap(spec, ids, b):
    """median distance between the true starts of neighbours inside buckets of at least 8 reads"""
    gpos, _, _ = readgen.read_locations(spec)
    starts = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
    size = np.diff(np.r_[starts, len(b)])
    big = np.repeat(size >= 8, size)
    same = (b[1:] == b[:-1]) & big[1:]
    assert same.sum() > 1000
    return float(np.median(np.abs(np.diff(gpos.astype(np.int64)[ids]))[same]))


def test_order_shape(monkeypatch):
    """100 000 reads of 150 bases at 30x in 2^12 buckets: dozens of reads, a few groups, per bucket"""
    spec = readgen.GenSpec.coverage(seed=11, n_reads=100_000, read_len=150, cov=30.0)
    ids, old_ids, b, ob = _check_shape(spec, monkeypatch, {"DISCO_ORDER_BITS": "12"})
    new, old = _neighbour_gap(spec, ids, b), _neighbour_gap(spec, old_ids, ob)
    print(f"median start distance of neighbours inside buckets of >= 8 reads: {new:.1f} bases, old path {old:.1f}")
    assert new < old


def test_natural_bucket_count_and_two_levels(monkeypatch):
    """the bucket count the library picks for the size (2^17: one level over bucket and sub-key), and 2^26 (two levels, 8 and 7 bits)"""
    spec = readgen.GenSpec.coverage(seed=12, n_reads=100_000, read_len=150, cov=30.0)
    ids, old_ids, b, ob = _check_shape(spec, monkeypatch, {})
    assert _neighbour_gap(spec, ids, b) < _neighbour_gap(spec, old_ids, ob)
    _check_shape(readgen.GenSpec.coverage(seed=13, n_reads=20_000, read_len=150, cov=30.0), monkeypatch, {"DISCO_ORDER_BITS": "26"})


def test_mixed_lengths(monkeypatch):
    """100 .. 250 bases: up to 228 m-mer positions, the quantization by the table's longest read; parity with the oracle"""
    spec = readgen.GenSpec.coverage(seed=14, n_reads=20_000, read_len=100, cov=30.0, len_max=250)
    _check_shape(spec, monkeypatch, {"DISCO_ORDER_BITS": "16"})
    c = assert_parity(readgen.generate_reads(spec), 40, "mixed lengths")
    assert c["e_out"] > 0


def _outputs(spec, sub_limit=-1):
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.order_sub_bits(sub_limit)
        g.run_graph()
        c = g.counters()
        c.pop("hbm_bytes")  # (the old path's counter table and slots)
        return canon_hip(g.fetch_edges(), g.fetch_contained()), c


def test_no_spare_bit(monkeypatch):
    """an item whose bucket, length and id leave no bit (a table of this size cannot fill the word: the limit of the inspect header
    stands for it) is the item as it was: the old path's reads per bucket, the old path's results"""
    spec = readgen.GenSpec.coverage(seed=15, n_reads=20_000, read_len=150, cov=30.0)
    _check_shape(spec, monkeypatch, {"DISCO_ORDER_BITS": "26"}, sub_limit=0)
    new, with_key = _outputs(spec, 0), _outputs(spec)
    monkeypatch.setenv("DISCO_NO_BINNED_ORDER", "1")
    old = _outputs(spec)
    for got, label in ((new, "no sub-key"), (with_key, "sub-key")):
        assert np.array_equal(got[0][0], old[0][0]) and np.array_equal(got[0][1], old[0][1]), f"{label}: results differ from the old path"
        assert got[1] == old[1], f"{label}: counters differ from the old path"
    assert old[1]["e_out"] > 0


@functools.lru_cache(maxsize=None)
def _parity_reads():
    """20 000 reads: both strands (the generator's), every twentieth read a second time — as it is or reverse complemented — and a
    low-complexity contig: the middle of one read in ten a repetition of a short unit (tied windows: the slow list)"""
    spec = readgen.GenSpec.coverage(seed=16, n_reads=19_000, read_len=150, cov=30.0)
    reads = readgen.generate_reads(spec)
    rng = np.random.default_rng(17)
    reads = low_complexity(reads, rng, share=0.1)
    dup = [reads[i] if i % 40 else reads[i].translate(_COMP)[::-1] for i in range(0, len(reads), 19)][:1000]
    reads = reads + dup
    return tuple(reads[i] for i in rng.permutation(len(reads)))


@pytest.mark.parametrize("min_overlap", [40, 33, 58])
def test_parity(min_overlap):
    """graph, contained rows and counters against the oracle; 33 and 58: the index pass with a run-time window length"""
    reads = list(_parity_reads())
    assert len(reads) == 20_000
    c = assert_parity(reads, min_overlap, f"start order, min-overlap {min_overlap}")
    assert c["e_out"] > 0 and c["n_contained"] >= 1000
    with buildgraph.BuildGraph(min_overlap=min_overlap) as g:
        g.upload_ascii(reads)
        g.build_index()
        assert g.order_sub_bits() == ORDER_SUB_MAX, "the pass took no sub-key: this parity run did not see it"
