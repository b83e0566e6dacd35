"""-m gpu : min-overlaps above 95 (DISCO_FLAG_SEEDED_KMER) against the CPU oracle. The index then holds a SEED of ks = 94 bases at each
read end and a seed hit at window w of read A stands for the reference's window j = w (prefix-aligned record, kept if w < len(A) - k) or
j = w - (k - ks) (suffix-aligned, kept if w >= k - ks); everything from verify on goes by the true k = min-overlap - 1 and by j.
The cases: d = k - ks of 1, 2, 3 and d, k at both sides of every 32-base word edge; reads that share an end with a longer read (the two
range tests at their limits); prefix- and suffix-type finds that meet at one reference window (the cap of four counts them together,
d seed windows apart); rows of 16 / 24 words and two classes of rows; three ranks with both index placements; inexact overlaps.
Every case: canonical edges, contained rows and the seven counters. Sets of at most 1500 reads (the oracle: 0.1 - 0.3 s each)."""
import functools

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from disco_amd.buildgraph import DiscoError
from oracle import pyoracle
from tests.dist_util import run_ranks_reads
from tests.util import canon_hip, run_hip_reads, run_oracle_reads, subs_by_edge

pytestmark = pytest.mark.gpu
SEEDED = buildgraph.FLAG_SEEDED_KMER
_COMP = str.maketrans("ACGT", "TGCA")
_COUNTERS = ("probes", "kmer_hits", "n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs")


def _rc(s):
    return s.translate(_COMP)[::-1]


def _rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _oracle(reads, mo):
    oe, orows, oc = run_oracle_reads(reads, mo)
    return canon_hip(oe, orows), oc, orows


def _assert_same(hip, oracle, label, counters=_COUNTERS):
    """what tests/test_gpu_min_overlap_sweep.py::_assert_same asserts: canonical edges, contained rows, the counters"""
    (ce, cc), hc = hip
    (oce, occ), oc = oracle[:2]
    assert np.array_equal(cc, occ), f"{label}: contained rows differ ({len(cc)} vs {len(occ)})"
    assert np.array_equal(ce, oce), f"{label}: edge list differs ({len(ce)} vs {len(oce)})"
    for key in counters:
        assert hc[key] == oc[key], f"{label}: counter {key}: hip {hc[key]} oracle {oc[key]}"


def _hip(reads, mo, flags=SEEDED, **kw):
    he, hr, hc = run_hip_reads(reads, mo, flags=flags, **kw)
    return canon_hip(he, hr), hc


def _check(reads, mo, label, oracle=None):
    oracle = oracle or _oracle(reads, mo)
    hip = _hip(reads, mo)
    _assert_same(hip, oracle, label)
    return hip[1], oracle


# ---- 1. the sweep -----------------------------------------------------------------------------------------------------------------
_SWEEP_MO = (96, 97, 98, 127, 128, 129, 130, 159, 160, 161, 200, 240)
_SWEEP_LENGTHS = {"short": lambda mo: (mo + 1, min(256, mo + 60)), "uniform": lambda mo: (250, 250)}


def _sweep_reads(kind, mo):
    lmin, lmax = _SWEEP_LENGTHS[kind](mo)
    return readgen.generate_reads(readgen.GenSpec.coverage(seed=5000 + mo, n_reads=1500, read_len=lmin, cov=30.0, len_max=lmax))


@functools.lru_cache(maxsize=None)
def _sweep_oracle(kind, mo):
    return _oracle(_sweep_reads(kind, mo), mo)


@pytest.mark.parametrize("mo", _SWEEP_MO)
def test_sweep(mo):
    """the shortest legal read (mo + 1 bases: two seed windows per base of d, one reference window) up to mo + 60, and 250 uniform"""
    for kind in _SWEEP_LENGTHS:
        reads = _sweep_reads(kind, mo)
        if kind == "short":
            assert min(len(r) for r in reads) == mo + 1
        hc, _ = _check(reads, mo, f"mo{mo} {kind}", _sweep_oracle(kind, mo))
        assert hc["e_out"] > 0, (mo, kind)


@pytest.mark.parametrize("mo", [96, 130])
@pytest.mark.parametrize("how", ["two_pass", "DISCO_ORDER_MIN_READS", "DISCO_NO_BINNED_INDEX"])
def test_sweep_other_paths(mo, how, monkeypatch):
    """the two-pass verify (its kmer_hits counts the compared candidates only, include/disco_hip.h: at most the oracle's), the grouped
    processing order and the index built with counting atomics"""
    for kind in _SWEEP_LENGTHS:
        reads, oracle = _sweep_reads(kind, mo), _sweep_oracle(kind, mo)
        if how == "two_pass":
            hip = _hip(reads, mo, flags=SEEDED | buildgraph.FLAG_TWO_PASS_VERIFY)
            _assert_same(hip, oracle, f"mo{mo} {kind} two passes", [c for c in _COUNTERS if c != "kmer_hits"])
            assert hip[1]["kmer_hits"] <= oracle[1]["kmer_hits"]
        else:
            monkeypatch.setenv(how, "1")
            _assert_same(_hip(reads, mo), oracle, f"mo{mo} {kind} {how}=1")


# ---- 2. shared ends: the range tests at w = d and w = L_A - k - 1 ------------------------------------------------------------------
def _shared_end_reads(mo):
    rng = np.random.default_rng(6000 + mo)
    genome = _rnd(rng, 5000)
    reads = []
    while len(reads) < 1200:
        L = int(rng.integers(mo + 2, 257))
        p = int(rng.integers(0, len(genome) - L + 1))
        L2 = int(rng.integers(mo + 1, L))  # in (mo, L)
        for q, n in ((p, L), (p, L2), (p + L - L2, L2)):  # the read, one with its left end, one with its right end
            s = genome[q:q + n]
            reads.append(_rc(s) if rng.random() < 0.5 else s)
    return reads[:1200]


@pytest.mark.parametrize("mo", [96, 97, 120, 160, 200])
def test_shared_ends(mo):
    """a contained read that starts where its container starts has the reference window 0 (a suffix-aligned seed hit at w = d exactly),
    one that ends where it ends the last window the reference looks up — shown from the oracle's rows alone"""
    reads = _shared_end_reads(mo)
    oracle = _oracle(reads, mo)
    rows = oracle[2]
    orients = np.unique(rows["orient"])
    assert len(orients) == 2, orients  # (a contained read lies on its container's strand or on the other one)
    for at_end, name in ((False, "start == 0"), (True, "start == len1 - len2")):
        sel = rows["start"] == (rows["len1"] - rows["len2"] if at_end else 0)
        for o in orients:
            assert int(np.sum(sel & (rows["orient"] == o))) >= 50, (mo, name, int(o), int(np.sum(sel & (rows["orient"] == o))))
    _check(reads, mo, f"shared ends mo{mo}", oracle)


# ---- 3. the cap across hit kinds --------------------------------------------------------------------------------------------------
def _cap_reads(mo, both_kinds):
    """20 groups: A = P + U[:mo + 2] has the reference window 30 = len(P) in common with three reads that begin with U (prefix-type
    finds) and three that end in P + U[:k] (suffix-type finds); with the seed the two kinds are found d windows apart, and the cap of
    four binds only if they are counted at the same window. Prefix-only form: eight readers of U"""
    rng = np.random.default_rng(7000 + mo + (0 if both_kinds else 1))
    k = mo - 1
    reads = []
    for _ in range(20):
        U, P = _rnd(rng, mo + 5), _rnd(rng, 30)
        group = [P + U[:mo + 2]]
        group += [U + _rnd(rng, 250 - len(U)) for _ in range(3 if both_kinds else 8)]
        if both_kinds:
            group += [_rnd(rng, 250 - 30 - k) + P + U[:k] for _ in range(3)]
        reads += group
    reads = [_rc(s) if rng.random() < 0.5 else s for s in reads]
    return [reads[i] for i in rng.permutation(len(reads))]


@pytest.mark.parametrize("mo", [96, 97, 130, 200])
@pytest.mark.parametrize("both_kinds", [True, False])
def test_cap_across_hit_kinds(mo, both_kinds):
    reads = _cap_reads(mo, both_kinds)
    oracle = _oracle(reads, mo)
    oc = oracle[1]
    want = (20, 40, 120) if both_kinds else (20, 80, None)
    assert oc["cap_bind_sites"] == want[0] and oc["asymmetric_pairs"] == want[1], (mo, oc)
    if want[2] is not None:
        assert oc["e_pre"] == want[2], (mo, oc)
    _check(reads, mo, f"cap mo{mo} both kinds {both_kinds}", oracle)


# ---- 4. long rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [512, 513])
def test_rows_of_16_and_24_words(L):
    """mo = 300 (d = 205: more than six words of k-mer beyond the seed) on reads that fill their last word or spill one base into a new one"""
    reads = readgen.generate_reads(readgen.GenSpec.coverage(seed=8000 + L, n_reads=1000, read_len=L, cov=25.0))
    hc, _ = _check(reads, 300, f"uniform {L} mo300")
    assert hc["e_out"] > 0


def test_two_classes_of_rows(monkeypatch):
    """mo = 130 on reads of 140 .. 250 bases with a tail of 600-base reads"""
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    reads = readgen.generate_reads(readgen.GenSpec.coverage(seed=8130, n_reads=1500, read_len=140, cov=30.0, len_max=250, long_len=600, long_share=1300))
    n_long = sum(len(r) > 256 for r in reads)
    assert n_long > 0
    oracle = _oracle(reads, 130)
    seen = {}
    he, hr, hc = run_hip_reads(reads, 130, seen, flags=SEEDED)
    assert seen["long_rows"] == n_long, (seen, n_long)  # (the two classes are what the case is for)
    _assert_same((canon_hip(he, hr), hc), oracle, "two classes mo130")
    assert hc["e_out"] > 0


# ---- 5. flows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mo", [96, 130])
@pytest.mark.parametrize("partitioned_index", [False, True])
def test_three_ranks(mo, partitioned_index, monkeypatch):
    """three ranks in one process, the index replicated and partitioned (the owner of a bucket maps and range-tests the seed hits)"""
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    for kind in _SWEEP_LENGTHS:
        (oce, occ), oc, _ = _sweep_oracle(kind, mo)
        edges, rows, info, _ = run_ranks_reads(_sweep_reads(kind, mo), mo, 3, flags=SEEDED, partitioned_index=partitioned_index)
        _assert_same((canon_hip(edges, rows), info), ((oce, occ), oc), f"three ranks mo{mo} {kind} partitioned {partitioned_index}")


@pytest.mark.parametrize("mo", [96, 130])
def test_inexact_overlaps(mo):
    """0.3 % substitutions and up to two of them inside an overlap, as tests/test_gpu_min_overlap_sweep.py builds them: the oracle's
    statement of the rule (the true k-mer exact, substitutions per edge included)"""
    rng = np.random.default_rng(99)
    reads = []
    for s in _sweep_reads("uniform", mo):
        b = np.frombuffer(s.encode(), dtype=np.uint8).copy()
        hit = rng.random(len(b)) < 0.003
        b[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        reads.append(b.tobytes().decode())
    with buildgraph.BuildGraph(min_overlap=mo, max_substitutions=2, flags=SEEDED) as g:
        g.upload_ascii(reads)
        g.run_graph()
        he, hr, hc, hs = g.fetch_edges(), g.fetch_contained(), g.counters(), g.fetch_edge_substitutions()
    codes, off = pyoracle.encode_reads(reads)
    orows, oe, oc, osubs = pyoracle.build_graph_inexact(codes, off, mo, 2)
    _assert_same((canon_hip(he, hr), hc), (canon_hip(oe, orows), oc), f"inexact mo{mo}", [c for c in _COUNTERS if c != "kmer_hits"])  # (tests.util.assert_parity_inexact's six)
    assert np.array_equal(subs_by_edge(he, hs), subs_by_edge(oe, osubs)), f"inexact mo{mo}: substitutions per edge differ"
    assert hc["e_out"] > 0 and int(np.asarray(hs).max()) > 0


# ---- 6. the flag ------------------------------------------------------------------------------------------------------------------
def test_refused_without_the_flag():
    with pytest.raises(DiscoError, match="unsupported"):
        buildgraph.BuildGraph(min_overlap=96)
    with pytest.raises(DiscoError, match="unsupported"):
        buildgraph.BuildGraph(min_overlap=1, flags=SEEDED)


@pytest.mark.parametrize("mo", [40, 95])
def test_no_effect_up_to_95(mo):
    reads = readgen.generate_reads(readgen.GenSpec.coverage(seed=9000 + mo, n_reads=1500, read_len=100, cov=30.0, len_max=250))
    (ce0, cc0), c0 = _hip(reads, mo, flags=0)
    (ce1, cc1), c1 = _hip(reads, mo, flags=SEEDED)
    assert np.array_equal(ce0, ce1) and np.array_equal(cc0, cc1) and len(ce0) > 0
    for key in _COUNTERS + ("raw_hits",):
        assert c0[key] == c1[key], key
