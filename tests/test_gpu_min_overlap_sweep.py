"""-m gpu : every legal min-overlap (18 .. 95, k = 17 .. 94) against the CPU oracle, on the shapes at which the minimizer run lists of the
index pass (index_runs_kernel -> probe_runs_kernel) change their instantiation: every window length nf = k - m + 1 from 1 to 64, every
NFMAX class of index_count_pick and both sides of every class edge, minimizers of 17 .. 31 bases, tied window minima (the 0xFFFE marker:
reads handed to the list pass), read ends at the edges of index_runs_kernel's blocks, and the stride selectors of the row kernels.
Small sets (1500 reads or fewer): a case costs the oracle about 0.1 s per set."""
import functools

import numpy as np
import pytest

from disco_amd import readgen
from tests.dist_util import run_ranks_reads
from tests.util import assert_parity, canon_hip, low_complexity, run_hip_reads, run_oracle_reads

pytestmark = pytest.mark.gpu
_COMP = str.maketrans("ACGT", "TGCA")
_COUNTERS = ("probes", "kmer_hits", "n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs")


def _shape(mo):
    """(k, m, nf) of a min-overlap: k-mer length, minimizer length (disco_minimizer_len) and m-mers per window"""
    k = mo - 1
    m = min(k, 23)
    if m % 2 == 0:
        m -= 1
    if k - m > 63:
        m = (k - 63) | 1
    return k, m, k - m + 1


_LENGTHS = {"short": lambda mo: (mo + 21, mo + 61), "uniform": lambda mo: (150, 150), "mixed": lambda mo: (100, 250)}

# 32-bit words of minimizer runs per read, by hand from the rule stated at runs_lpr_for (disco_hip.hip): with W = longest - k windows and
# about 2 W / (nf + 1) runs expected, 16 words where W <= 128 and that is at most 20, 32 where W <= 256 and it is at most 44, none
# otherwise, and none for windows of one m-mer. Literals on purpose: a library that answers differently is a finding.
_RUN_WORDS = {
    "short": {0: {18, 20, 22, 24}, 32: {19, 21, 23, 25, 26, 27}, 16: set(range(28, 96))},
    "uniform": {0: set(range(18, 28)), 32: set(range(28, 34)), 16: set(range(34, 96))},
    "mixed": {0: set(range(18, 32)), 32: set(range(32, 96)), 16: set()},
}


def _run_words(kind, mo):
    (w,) = [w for w, mos in _RUN_WORDS[kind].items() if mo in mos]
    return w


def _sweep_reads(kind, mo, **kw):
    lmin, lmax = _LENGTHS[kind](mo)
    reads = readgen.generate_reads(readgen.GenSpec.coverage(seed=1000 + mo, n_reads=1500, read_len=lmin, cov=30.0, len_max=lmax, **kw))
    assert max(len(r) for r in reads if len(r) <= 256) == lmax  # (the table above goes by the longest read)
    return reads


@functools.lru_cache(maxsize=None)
def _sweep_oracle(kind, mo):
    """the oracle's canonical output and counters for a set of (a) — computed once, shared by the flows of (e)"""
    oe, orows, oc = run_oracle_reads(_sweep_reads(kind, mo), mo)
    return canon_hip(oe, orows), oc


def _hip(reads, mo):
    """one pass through the entry points, one context: the results and the path that ran"""
    seen = {}
    he, hr, hc = run_hip_reads(reads, mo, seen)
    return canon_hip(he, hr), hc, seen["probe_run_words"], seen["long_rows"]


def _assert_same(hip, oracle, label):
    """what tests.util.assert_parity asserts: canonical edges, contained rows, all seven counters"""
    (ce, cc), hc = hip
    (oce, occ), oc = oracle
    assert np.array_equal(cc, occ), f"{label}: contained rows differ ({len(cc)} vs {len(occ)})"
    assert np.array_equal(ce, oce), f"{label}: edge list differs ({len(ce)} vs {len(oce)})"
    for key in _COUNTERS:
        assert hc[key] == oc[key], f"{label}: counter {key}: hip {hc[key]} oracle {oc[key]}"


@pytest.mark.parametrize("mo", range(18, 96))
def test_every_min_overlap(mo, monkeypatch):
    """three length shapes per min-overlap — short reads (the only ones windows of 2 .. 4 m-mers get run lists for), uniform 150 and
    mixed 100 .. 250 with the grouping's counting pass riding in the index pass — and the uniform one again with the counting atomics of
    the bucket table in the same kernels (COUNT = true): the oracle's graph, and the run words the documented rule gives"""
    for kind, env in (("short", None), ("uniform", None), ("uniform", "DISCO_NO_BINNED_INDEX"), ("mixed", "DISCO_ORDER_MIN_READS")):
        label = f"mo{mo} {kind}" + (f" {env}=1" if env else "")
        reads = _sweep_reads(kind, mo)
        oracle = _sweep_oracle(kind, mo)
        with monkeypatch.context() as mp:
            if env:
                mp.setenv(env, "1")
            canon, hc, words, _ = _hip(reads, mo)
        assert words == _run_words(kind, mo), f"{label}: {words} run words per read, the rule gives {_run_words(kind, mo)}"
        _assert_same((canon, hc), oracle, label)
        assert hc["e_out"] > 0, label


def _reads_with_a_tied_window(reads, mo):
    """reads in which the same canonical m-mer occurs twice less than nf positions apart: both inside one window, whose minimum can tie"""
    _, m, nf = _shape(mo)
    pw = np.uint64(4) ** np.arange(m, dtype=np.uint64)
    n = 0
    for s in reads:
        c = (np.frombuffer(s.encode(), dtype=np.uint8) >> 1 & 3).astype(np.uint64)  # A 0, C 1, T 2, G 3: the complement is c ^ 2
        win = np.lib.stride_tricks.sliding_window_view(c, m)
        fwd = (win * pw[::-1]).sum(axis=1, dtype=np.uint64)
        rev = ((win ^ np.uint64(2)) * pw).sum(axis=1, dtype=np.uint64)
        canon = np.minimum(fwd, rev)
        o = np.argsort(canon, kind="stable")  # (equal m-mers stay in position order: neighbours are the closest pair)
        same = canon[o][1:] == canon[o][:-1]
        n += bool(np.any(same & (np.diff(o) < nf)))
    return n


_EDGE_MO = (19, 21, 23, 25, 30, 31, 32, 35, 36, 39, 40, 41, 47, 48, 55, 56, 65, 66, 71, 72, 87, 88, 90, 92, 94, 95)


@pytest.mark.parametrize("mo", _EDGE_MO)
def test_tied_windows_at_every_class_edge(mo):
    """low-complexity stretches at both sides of every NFMAX class edge and at every minimizer length: tied window minima take the tie
    rule, the run list carries the marker and the read goes to the list pass. That the inputs tie is shown from the inputs alone"""
    for lmin, lmax in ((max(150, mo + 2), max(150, mo + 2)), (max(100, mo + 1), 250)):
        spec = readgen.GenSpec.coverage(seed=2000 + mo, n_reads=1500, read_len=lmin, cov=30.0, len_max=lmax)
        reads = low_complexity(readgen.generate_reads(spec), np.random.default_rng(2000 + mo + 2))
        tied = _reads_with_a_tied_window(reads, mo)
        assert tied >= 0.05 * len(reads), f"mo{mo} {lmin}-{lmax}: only {tied} of {len(reads)} reads can tie"
        assert_parity(reads, mo, f"ties mo{mo} {lmin}-{lmax}")


@pytest.mark.parametrize("mo", [19, 31, 40, 47, 55, 72, 87, 95])
def test_read_ends_at_block_edges(mo, monkeypatch):
    """reads that end at, one before and one behind the edges of index_runs_kernel's blocks of nf windows, the shortest legal read, the
    5-word / 8-word boundary of the compare and a full 64-byte row, mixed inside every wavefront; 1351 reads: a last block that is
    neither a full workgroup nor a full wavefront"""
    k, _, nf = _shape(mo)
    lengths = sorted({L for L in (mo + 1, mo + 2, k + nf, k + nf + 1, k + 2 * nf - 1, k + 2 * nf, 160, 161, 255, 256) if mo < L <= 256})
    rng = np.random.default_rng(3000 + mo)
    genome = "".join(rng.choice(list("ACGT"), 6000))
    reads = []
    for _ in range(1351):
        L = int(rng.choice(lengths))
        p = int(rng.integers(0, len(genome) - L + 1))
        s = genome[p:p + L]
        reads.append(s.translate(_COMP)[::-1] if rng.random() < 0.5 else s)
    assert_parity(reads, mo, f"block edges mo{mo}")
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    assert_parity(reads, mo, f"block edges mo{mo}, grouped order")


@pytest.mark.parametrize("mo", [40, 80])
@pytest.mark.parametrize("L", [160, 161, 256, 257, 512, 513, 768, 769, 1024, 1025])
def test_uniform_lengths_at_stride_edges(L, mo):
    """both sides of every selector boundary of the row kernels (160 bases, strides of 8 / 16 / 24 / 32 words, the generic variant beyond):
    every read fills its last word, or spills one base into a new one"""
    reads = readgen.generate_reads(readgen.GenSpec.coverage(seed=4000 + L, n_reads=1000, read_len=L, cov=25.0))
    c = assert_parity(reads, mo, f"uniform {L} mo{mo}")
    assert c["e_out"] > 0


_FLOW_MO = (19, 31, 39, 47, 55, 71, 72, 87, 95)


@pytest.mark.parametrize("mo", _FLOW_MO)
def test_three_ranks_at_the_ladder_edges(mo, monkeypatch):
    """the list form of the index pass (ranks own loci: run lists by position, runs_by_pos): three ranks, one process"""
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    (oce, occ), oc = _sweep_oracle("mixed", mo)
    seen = {}
    edges, rows, info, _ = run_ranks_reads(_sweep_reads("mixed", mo), mo, 3, inspect=seen)
    assert all(seen[r]["probe_run_words"] == _run_words("mixed", mo) for r in range(3)), (mo, seen)  # (the run lists are what the case is for)
    ce, cc = canon_hip(edges, rows)
    assert np.array_equal(cc, occ) and np.array_equal(ce, oce), f"mo{mo}: {len(ce)} edges, {len(cc)} rows; oracle {len(oce)}, {len(occ)}"
    for key in ("e_out", "n_contained", "e_pre"):
        assert info[key] == oc[key], (mo, key, info[key], oc[key])


@pytest.mark.parametrize("mo", _FLOW_MO)
def test_two_classes_of_rows_at_the_ladder_edges(mo, monkeypatch):
    """the mixed set with a tail of 600-base reads: two classes of rows exactly where a longest short read of 250 bases has run lists"""
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    reads = _sweep_reads("mixed", mo, long_len=600, long_share=1300)
    n_long = sum(len(r) > 256 for r in reads)
    assert n_long > 0
    oe, orows, oc = run_oracle_reads(reads, mo)
    canon, hc, _, long_rows = _hip(reads, mo)
    assert long_rows == (n_long if _run_words("mixed", mo) else 0), (mo, long_rows, n_long)
    _assert_same((canon, hc), (canon_hip(oe, orows), oc), f"two classes mo{mo}")


@pytest.mark.parametrize("mo", _FLOW_MO)
def test_inexact_overlaps_at_the_ladder_edges(mo):
    """0.3 % substitutions and up to two of them inside an overlap: the oracle's statement of the same rule, substitutions per edge included"""
    rng = np.random.default_rng(99)
    out = []
    for s in _sweep_reads("uniform", mo):
        b = np.frombuffer(s.encode(), dtype=np.uint8).copy()
        hit = rng.random(len(b)) < 0.003
        b[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        out.append(b.tobytes().decode())
    assert_parity(out, mo, f"inexact mo{mo}", max_substitutions=2)
