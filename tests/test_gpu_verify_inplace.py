"""-m gpu : verify_flat_kernel's in-place compaction. A verified hit whose rank is the slot it was loaded from is not stored onto itself, and
a read's count is rewritten only where it changed. Every read set here is built so that
one of the places where that can go wrong carries the result: rows that shift and rows that do not, drops at the front, in the middle and
at the end of a row, rows that cross batch boundaries behind a drop, tail rows whose id is rewritten where they lie, partial chunks.

Each case: edges and contained rows against the oracle, with the pair window and with DISCO_VERIFY_CACHE=0; the counters against a run
of the same reads under DISCO_NO_FLAT_VERIFY=1 (the wave-per-read verify_kernel, which this compaction is no part of). The precondition
that makes a case mean something is asserted on that run's counters."""
import os
import subprocess
import sys

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.util import canon_hip, run_hip_reads, run_oracle_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("kmer_hits", "raw_hits", "n_contained", "e_pre", "e_out")
_COMP = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s.translate(_COMP)[::-1]


def _distinct_starts(seed, n, cov=30.0):
    """150-base reads of the generator, one per start position (a second read at a start is a duplicate, whatever its strand), and no two
    starts 150 - k = 111 bases apart: such a pair shares exactly the k-mer (min-overlap 40: k = 39), a k-mer hit that is no overlap"""
    spec = readgen.GenSpec.coverage(seed, n, 150, cov)
    gpos, _len, _strand = readgen.read_locations(spec)
    reads = readgen.generate_reads(spec)
    seen, keep = set(), []
    for i, g in enumerate(int(x) for x in gpos):
        if g in seen or g - 111 in seen or g + 111 in seen:
            continue
        seen.add(g)
        keep.append(i)
    return [reads[i] for i in keep]


def _with_copies(reads, every):
    """an exact copy or (alternating) a reverse-complement copy of every `every`-th read, appended"""
    return reads + [reads[i] if (i // every) % 2 == 0 else _rc(reads[i]) for i in range(0, len(reads), every)]


def _mixed_lengths(seed=7, n=3000):
    return readgen.generate_reads(readgen.GenSpec.coverage(seed, n, 100, 30.0, len_max=250))


def _with_contained(reads):
    """shorter reads planted inside every fourth read of 170 bases or more: one from its middle, one that ends with it, one that begins
    with it, every other one as its reverse complement"""
    planted = []
    for t, s in enumerate(reads[::4]):
        if len(s) < 170:
            continue
        for u, p in enumerate((s[35:35 + 100 + t % 30], s[-(100 + t % 50):], s[:100 + t % 40])):
            planted.append(_rc(p) if (t + u) % 2 else p)
    return reads + planted


def _hold(reads, monkeypatch, label, precondition=None, flags=0, min_overlap=40):
    """the oracle's graph with the pair window on and off; the counters of the wave-per-read kernel's run"""
    kw = {"flags": flags} if flags else {}
    oe, orows, oc = run_oracle_reads(reads, min_overlap)
    oce, occ = canon_hip(oe, orows)
    monkeypatch.setenv("DISCO_NO_FLAT_VERIFY", "1")
    _e, _r, ref = run_hip_reads(reads, min_overlap, **kw)
    monkeypatch.delenv("DISCO_NO_FLAT_VERIFY")
    print(label, "n_reads", len(reads), {k: ref[k] for k in COUNTERS})
    if precondition is not None:
        assert precondition(ref, len(reads)), f"{label}: the read set does not do what the case is about: {ref}"
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("DISCO_VERIFY_CACHE", env)
        try:
            inspect = {}
            he, hr, hc = run_hip_reads(reads, min_overlap, inspect, **kw)
            inspect["edges"] = he
        finally:
            monkeypatch.delenv("DISCO_VERIFY_CACHE", raising=False)
        lab = f"{label} DISCO_VERIFY_CACHE={env}"
        ce, cc = canon_hip(he, hr)
        assert np.array_equal(cc, occ), f"{lab}: contained rows differ ({len(cc)} vs {len(occ)})"
        assert np.array_equal(ce, oce), f"{lab}: edge list differs ({len(ce)} vs {len(oce)})"
        for key in COUNTERS:
            assert hc[key] == ref[key], f"{lab}: counter {key}: flat {hc[key]} wave-per-read {ref[key]}"
        for key in ("probes", "n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs") + (() if flags else ("kmer_hits",)):
            assert hc[key] == oc[key], f"{lab}: counter {key}: hip {hc[key]} oracle {oc[key]}"
    return ref, inspect


def test_nothing_dropped_anywhere(monkeypatch):
    """reads of one length at pairwise distinct starts: every candidate verifies as an overlap, no hit moves, nothing is stored"""
    reads = _distinct_starts(201, 3900)
    assert 2700 <= len(reads) <= 3300  # about 3 000 of the 3 900 generated
    _hold(reads, monkeypatch, "distinct", lambda c, n: c["raw_hits"] == c["kmer_hits"] and c["n_contained"] == 0 and c["raw_hits"] > 20 * n)


def test_drops_at_the_front_of_rows(monkeypatch):
    """copies and reverse-complement copies of every fifth read: their rows lose the candidate of window 0 and shift by one"""
    reads = _with_copies(_distinct_starts(201, 3900), 5)
    _hold(reads, monkeypatch, "front", lambda c, n: c["n_contained"] > 0 and c["raw_hits"] < c["kmer_hits"])


def test_drops_in_the_middle_and_at_the_end_of_rows(monkeypatch):
    """mixed lengths with shorter reads planted in the middle and at both ends of longer ones: containment-type candidates anywhere in a
    row. A read planted as its host's suffix is a dropped candidate of the host's last window, so that rows end on a dropped lane (`last`,
    the carry) wherever no kept candidate shares that window; the counters cannot tell how many rows do, and nothing here asserts it"""
    base = _mixed_lengths()
    reads = _with_contained(base)
    assert len(reads) - len(base) >= 900  # three planted reads in each of some hundred hosts
    _hold(reads, monkeypatch, "contained", lambda c, n: c["n_contained"] > n // 8 and c["raw_hits"] < c["kmer_hits"])


def test_rows_that_cross_batch_boundaries_after_a_drop(monkeypatch):
    """75x on a small genome and every third read twice (100x): rows of more than 64 candidates that lose one at the front; their later
    batches drop nothing and must still move every hit (carry < 64 b - Pseg); the rows' counts go to row_cnt"""
    base = readgen.generate_reads(readgen.GenSpec.coverage(211, 1500, 150, 75.0))
    reads = _with_copies(base, 3)
    _hold(reads, monkeypatch, "wide", lambda c, n: c["kmer_hits"] > 64 * n and c["n_contained"] > 0 and c["raw_hits"] < c["kmer_hits"])


def test_substitution_errors(monkeypatch):
    """1 % substituted bases: candidates fail at arbitrary lanes, nearly every kept hit moves"""
    spec = readgen.GenSpec.coverage(223, 3000, 150, 30.0)
    codes, off = readgen.generate_codes(spec)
    reads = readgen.codes_to_reads(readgen.substitute(codes, off, 9, 10000), off)
    _hold(reads, monkeypatch, "errors", lambda c, n: 0 < c["raw_hits"] < 0.9 * c["kmer_hits"])


def test_two_classes_of_rows(monkeypatch):
    """a 0.1 % tail of 600-base reads among 150-base reads at distinct starts: a verified hit on a tail row gets the long read's id back
    although it stays where it lies (hw != h). With two classes of rows DISCO_NO_FLAT_VERIFY is not honoured (the short class always takes
    the flat kernel), so the counters' cross-check is no independent source here: the oracle carries this case"""
    spec = readgen.GenSpec.coverage(227, 8000, 150, 30.0, long_len=600, long_share=66)
    gpos, length, _strand = readgen.read_locations(spec)
    all_reads = readgen.generate_reads(spec)
    seen, reads = set(), []
    for i, s in enumerate(all_reads):  # the long reads all stay; of the short ones the first at every start
        if length[i] <= 256:
            if int(gpos[i]) in seen:
                continue
            seen.add(int(gpos[i]))
        reads.append(s)
    n_long = sum(len(s) > 256 for s in reads)
    assert n_long >= 3, n_long
    _ref, inspect = _hold(reads, monkeypatch, "two-class", lambda c, n: c["raw_hits"] > 20 * n)
    assert inspect["long_rows"] == n_long
    # edges whose short read lies beyond the long read's head row: they exist only through verified hits that named a tail row
    he = inspect["edges"]
    assert int(((he["len_src"] == 600) & (he["len_dst"] <= 256) & (he["offset"] > 256)).sum()) >= 3


def test_the_two_pass_form(monkeypatch):
    """MODE 2 (DISCO_FLAG_TWO_PASS_VERIFY): the candidates of the other pass are valid lanes that are never kept, so nearly every row shifts"""
    reads = _with_contained(_mixed_lengths())
    _hold(reads, monkeypatch, "two-pass", lambda c, n: c["n_contained"] > n // 8 and c["raw_hits"] < c["kmer_hits"], flags=buildgraph.FLAG_TWO_PASS_VERIFY)


@pytest.mark.parametrize("n", [1, 31, 33, 65])
def test_chunk_tails(monkeypatch, n):
    """read counts around the chunk sizes (32 with the pair window, 64 without): the last chunk and its last batch are partial"""
    reads = readgen.generate_reads(readgen.GenSpec.coverage(229 + n, n, 150, 12.0))
    _hold(reads, monkeypatch, f"tail-{n}", lambda c, m: c["kmer_hits"] > 0 if m > 1 else c["kmer_hits"] == 0)


_AB_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests.test_gpu_verify_inplace import _distinct_starts, _with_copies, COUNTERS
from tests.util import canon_hip, run_hip_reads
reads = _with_copies(_distinct_starts(201, 3900), 5)
he, hr, hc = run_hip_reads(reads, 40)
ce, cc = canon_hip(he, hr)
np.savez(sys.argv[2], ce=ce, cc=cc)
print(json.dumps({k: hc[k] for k in COUNTERS}))
"""


def test_the_ab_build_gives_the_same_graph(tmp_path):
    """-DVERIFY_ALWAYS_COMPACT (every kept hit is stored, every count rewritten: the form this kernel had) is a build for timing whose
    results are right: the same rows and counters as the shipped build on the set with drops at the front of rows"""
    import json
    import re

    from disco_amd import build

    # a build of tools/ab_build.py made beforehand is taken while no source is newer than it; otherwise the library is compiled here (minutes)
    lib = os.environ.get("DISCO_AB_ALWAYS_COMPACT_LIB", "")
    if not (lib and os.path.exists(lib) and all(os.path.getmtime(d) <= os.path.getmtime(lib) for d in build.HIP_DEPS)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_build.py"), "always_compact", "-DVERIFY_ALWAYS_COMPACT"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200)
        m = re.search(r"^(\S+lib_always_compact\.so) spills: (\{.*\})\s*$", r.stdout, flags=re.M)
        assert r.returncode == 0 and m, (r.stdout, r.stderr[-2000:])
        assert m.group(2) == "{}", f"the A/B build spills vector registers: {m.group(2)}"
        lib = m.group(1)
    assert os.path.exists(lib), lib
    got = {}
    for arm, path in (("shipped", ""), ("always_compact", lib)):
        env = dict(os.environ)
        env.pop("DISCO_LIB", None)
        if path:
            env["DISCO_LIB"] = path
        out = tmp_path / f"{arm}.npz"
        r = subprocess.run([sys.executable, "-c", _AB_SCRIPT, ROOT, str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, (arm, r.stderr[-2000:])
        z = np.load(out)
        got[arm] = (json.loads(r.stdout.strip().splitlines()[-1]), z["ce"], z["cc"])
    a, b = got["shipped"], got["always_compact"]
    assert a[0] == b[0], (a[0], b[0])
    assert a[0]["n_contained"] > 0 and a[0]["raw_hits"] < a[0]["kmer_hits"]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
