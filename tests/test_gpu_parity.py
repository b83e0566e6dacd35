"""-m gpu : the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs — bit-exact."""
import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests.util import assert_parity, canon_hip, run_oracle_reads

pytestmark = pytest.mark.gpu

def _gen(seed, n, lmin, cov, lmax=None, contigs=1):
    spec = readgen.GenSpec.coverage(seed, n, lmin, cov, n_contigs=contigs, len_max=lmax)
    return readgen.generate_reads(spec)


@pytest.mark.parametrize("seed,n,lmin,lmax,cov,minovl", [
    (42, 5000, 150, 150, 30.0, 40),     # BASELINE shape (uniform 150 bp, k = 39)
    (61, 5000, 100, 200, 30.0, 30),     # the reference's default min-overlap (disco.cfg): windows of 7 m-mers, 64 run entries per read
    (62, 4000, 150, 150, 30.0, 35),     # windows of 12
    (63, 4000, 120, 250, 40.0, 45),     # windows of 22, two reads per group
    (64, 4000, 150, 150, 30.0, 50),     # windows of 27
    (7, 4000, 100, 250, 30.0, 40),      # mixed lengths: heavy containment
    (11, 6000, 60, 90, 20.0, 31),       # k = 30 (even: palindromic k-mers possible), k <= 32 single word
    (13, 3000, 80, 120, 25.0, 66),      # k = 65 is rejected; see test_k_limits — here k = 64 via min_overlap 65
    (5, 2000, 300, 600, 20.0, 40),      # long reads, many words per row
    (43, 3000, 257, 512, 25.0, 40),     # 16-word rows: the staged verify variant for reads of 257..512 bases
    (47, 3000, 260, 500, 40.0, 65),     # the same at k = 64
    (71, 3000, 250, 500, 30.0, 80),     # round 4: k = 79 (three-word k-mers; windows of 57 m-mers of 23)
    (73, 3000, 150, 150, 60.0, 80),     # ... on 64-byte rows (the flat verify / selection kernels)
    (79, 3000, 250, 500, 30.0, 88),     # k = 87: minimizers of 25 bases (k - m <= 63)
    (83, 2500, 250, 500, 30.0, 95),     # k = 94, the widest supported: minimizers of 31
    (89, 3000, 130, 250, 40.0, 95),     # ... on 64-byte rows
    (53, 1500, 520, 760, 25.0, 40),     # 24-word rows
    (59, 1500, 800, 1024, 25.0, 50),    # 32-word rows (the widest staged variant; longer reads: generic variant)
    (17, 6000, 150, 150, 100.0, 40),    # 100x coverage: rows of 65..256 hits (wide-row paths of edge selection / marking)
    (19, 5000, 100, 250, 120.0, 40),    # the same with mixed lengths (containment inside wide rows)
    (29, 4000, 150, 150, 300.0, 40),    # 300x: rows of 257..1024 hits (edge_select_mid_kernel), big-node marking
    (31, 6000, 150, 150, 900.0, 40),    # 900x: rows beyond every LDS capacity (global-scratch passes), cap / duplicates bind
])
def test_generated(seed, n, lmin, lmax, cov, minovl):
    if minovl == 66:
        minovl = 65
    reads = _gen(seed, n, lmin, cov, lmax)
    c = assert_parity(reads, minovl, f"seed{seed}")
    assert c["e_out"] > 0


@pytest.mark.parametrize("seed,n,lmin,lmax,cov,minovl,words", [
    (42, 3000, 150, 150, 30.0, 40, 16),    # BASELINE: the instantiation for windows of 17
    (101, 3000, 150, 150, 30.0, 33, 32),   # round 6: windows of 10 (64 run entries per read) — no instantiation of their own: the window length as a run-time value
    (102, 3000, 150, 150, 30.0, 58, 16),   # windows of 35 (arrays for 64)
    (103, 3000, 100, 250, 30.0, 37, 32),   # windows of 14, reads of up to 256 bases: 64 run entries
    (104, 3000, 150, 150, 40.0, 66, 16),   # k = 65: three-word k-mers
    (73, 3000, 150, 150, 60.0, 80, 16),    # k = 79
    (89, 3000, 130, 250, 40.0, 95, 32),    # k = 94, minimizers of 31 bases
    (105, 2000, 300, 600, 20.0, 33, 0),    # reads beyond 256 bases: no run lists (round 2's probe), whatever the window
])
def test_which_shapes_get_minimizer_runs(seed, n, lmin, lmax, cov, minovl, words):
    """VERDICT r5 missing #3: the fast probe (run lists out of the index pass) existed for min-overlap 30 / 35 / 40 / 45 / 50 only; every
    window of up to 64 m-mers over 64-byte rows has it now — parity against the oracle AND the path that ran"""
    reads = _gen(seed, n, lmin, cov, lmax)
    with buildgraph.BuildGraph(min_overlap=minovl) as g:
        g.upload_ascii(reads)
        g.run_graph()
        assert g.probe_run_words() == words, (minovl, g.probe_run_words())
        he, hr, hc = g.fetch_edges(), g.fetch_contained(), g.counters()
    oe, orows, oc = run_oracle_reads(reads, minovl)
    ce, cc = canon_hip(he, hr)
    oce, occ = canon_hip(oe, orows)
    assert np.array_equal(cc, occ) and np.array_equal(ce, oce)
    for key in ("probes", "kmer_hits", "n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs"):
        assert hc[key] == oc[key], (key, hc[key], oc[key])


def test_duplicates_and_revcomp_duplicates():
    reads = _gen(3, 1500, 120, 20.0)
    comp = str.maketrans("ACGT", "TGCA")
    extra = [r for r in reads[:200]] + [r.translate(comp)[::-1] for r in reads[200:400]]
    assert_parity(reads + extra, 40, "dups")


def test_repeats_order_dependent_regime():
    # 30 copies of a 500 bp repeat inside random flanks: cap of 4 edges per k-mer binds, asymmetric pairs appear
    rng = np.random.default_rng(99)
    rep = "".join(rng.choice(list("ACGT"), 500))
    genome = ""
    for _ in range(30):
        genome += "".join(rng.choice(list("ACGT"), 300)) + rep
    reads = []
    for _ in range(8000):
        L = int(rng.integers(100, 201))
        p = int(rng.integers(0, len(genome) - L))
        s = genome[p:p + L]
        if rng.random() < 0.5:
            s = s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
        reads.append(s)
    c = assert_parity(reads, 40, "repeats")
    assert c["cap_bind_sites"] > 0 or c["asymmetric_pairs"] > 0


def test_tiny_and_empty_graphs():
    reads = _gen(21, 50, 100, 2.0)       # 2x coverage: few overlaps
    assert_parity(reads, 40, "sparse")
    assert_parity(reads[:1], 40, "single read")


def test_twin_check_shortcut_is_sound(monkeypatch):
    """edge selection that drops nothing implies symmetric lists (proof in disco_hip.hip:twin_check); force the search anyway
    and require the same answer, on data where nothing is dropped and on data where hits are dropped"""
    from tests import golden_util as gu
    from tests.util import run_hip_reads

    for name in ("mixed_4k", "repeats_8k"):
        reads, fidx, mo = gu.case_inputs(name)
        monkeypatch.delenv("DISCO_FORCE_TWIN_CHECK", raising=False)
        e1, r1, c1 = run_hip_reads(reads, mo)
        monkeypatch.setenv("DISCO_FORCE_TWIN_CHECK", "1")
        e2, r2, c2 = run_hip_reads(reads, mo)
        from tests.util import canon_hip
        (ce1, cc1), (ce2, cc2) = canon_hip(e1, r1), canon_hip(e2, r2)  # the emission order is not defined
        assert np.array_equal(ce1, ce2) and np.array_equal(cc1, cc2)
        assert c1["asymmetric_pairs"] == c2["asymmetric_pairs"] and c1["e_pre"] == c2["e_pre"]
        # the third way to the same answer: without the list of dropped hits the search goes by the bitmap of the reads that dropped
        # something (what the multi-GPU flow and selections with more than 2^20 drops use)
        monkeypatch.delenv("DISCO_FORCE_TWIN_CHECK")
        monkeypatch.setenv("DISCO_NO_DROP_LIST", "1")
        e3, r3, c3 = run_hip_reads(reads, mo)
        monkeypatch.delenv("DISCO_NO_DROP_LIST")
        ce3, cc3 = canon_hip(e3, r3)
        assert np.array_equal(ce1, ce3) and np.array_equal(cc1, cc3)
        assert c1["asymmetric_pairs"] == c3["asymmetric_pairs"] and c1["e_pre"] == c3["e_pre"]
        # ... and a list that is too short for what was dropped must be noticed and left unused
        monkeypatch.setenv("DISCO_DROP_LIST_CAP", "3")
        e4, r4, c4 = run_hip_reads(reads, mo)
        monkeypatch.delenv("DISCO_DROP_LIST_CAP")
        ce4, cc4 = canon_hip(e4, r4)
        assert np.array_equal(ce1, ce4) and np.array_equal(cc1, cc4)
        assert c1["asymmetric_pairs"] == c4["asymmetric_pairs"] and c1["e_pre"] == c4["e_pre"]


def test_long_reads_generic_stride_paths():
    """reads of 1.2-3 kbp: rows wider than the LDS staging limits (probe_kernel<.,false>, verify_kernel<false>) and more than one
    probe segment of PROBE_SEGW windows per read"""
    reads = _gen(31, 400, 1200, 12.0, 3000)
    c = assert_parity(reads, 40, "long")
    assert c["e_pre"] > 0


def test_high_multiplicity_rows_take_the_big_paths():
    """deep coverage of a 50-copy repeat: hundreds of candidates per read -> rows beyond the LDS capacities
    (probe big-row pass, edge-selection global-scratch pass, big-node transitive marking)"""
    rng = np.random.default_rng(5)
    rep = "".join(rng.choice(list("ACGT"), 260))
    genome = "".join("".join(rng.choice(list("ACGT"), 90)) + rep for _ in range(50))
    reads = []
    comp = str.maketrans("ACGT", "TGCA")
    for _ in range(9000):
        L = int(rng.integers(110, 160))
        p = int(rng.integers(0, len(genome) - L))
        s = genome[p:p + L]
        reads.append(s.translate(comp)[::-1] if rng.random() < 0.5 else s)
    c = assert_parity(reads, 40, "multiplicity")
    assert c["big_rows"] > 0


def test_bandwidth_probes_report_sane_numbers():
    """disco_measure_hbm / disco_measure_gather (the measured ceilings bench.py prints beside the nominal 8 TB/s)"""
    from disco_amd import buildgraph

    with buildgraph.BuildGraph(min_overlap=40) as g:
        copy = g.measure_hbm(256 << 20, 2)
        gather = g.measure_gather(256 << 20, 2)
    assert 500.0 < copy < 8000.0, copy      # GB/s, read + write bytes of a streaming copy
    assert 200.0 < gather < 8000.0, gather  # GB/s of random 64-byte rows


@pytest.mark.parametrize("rate,lmin,lmax", [(0.01, 150, 150), (0.004, 100, 250)])
def test_reads_with_substitution_errors(rate, lmin, lmax):
    """sequencing errors: many candidates whose end k-mer matches exactly but whose overlap region does not (the k-mer-only
    branch of verify_kernel; `kmer_hits` must still equal the oracle's count) and k-mers broken by an error"""
    reads = _gen(23, 6000, lmin, 40.0, lmax)
    rng = np.random.default_rng(99)
    out = []
    for s in reads:
        b = np.frombuffer(s.encode(), dtype=np.uint8).copy()
        hit = rng.random(len(b)) < rate
        b[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        out.append(b.tobytes().decode())
    c = assert_parity(out, 40, f"errors{rate}")
    assert c["kmer_hits"] > 2 * c["e_pre"] > 0


def test_metagenome_like_abundances():
    """contig abundances spread over two orders of magnitude (generator skew = 1): narrow, wide and big rows in one data set"""
    spec = readgen.GenSpec.coverage(37, 12000, 100, 30.0, n_contigs=40, len_max=250, skew=1)
    c = assert_parity(readgen.generate_reads(spec), 40, "skew")
    assert c["e_out"] > 0 and c["n_contained"] > 0


def test_edge_files_follow_connected_components():
    """disco_fetch_edge_files: all edges of a node in ONE file (what the consumer's per-file pre-simplification needs), large
    components dealt out by size"""
    from disco_amd import buildgraph
    from tests.partition_model import components, partition_model

    spec = readgen.GenSpec.coverage(41, 30000, 150, 30.0, n_contigs=12)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        e = g.fetch_edges()
        root = components(e["src"], e["dst"], spec.n_reads)
        for nf in (1, 4, 7):
            f = g.fetch_edge_files(nf)
            assert len(f) == len(e) and f.max() < nf
            assert np.array_equal(f, partition_model(e["src"], e["dst"], spec.n_reads, nf, root)[0])   # exactly the rule's files
            node_file = {}
            for a, b, t in zip(e["src"].tolist(), e["dst"].tolist(), f.tolist()):
                assert node_file.setdefault(a, t) == t and node_file.setdefault(b, t) == t
            if nf > 1:
                load = np.bincount(f, minlength=nf)
                assert load.min() > 0 and load.max() < 2.5 * load.mean()  # 12 contigs over 4 / 7 files


def test_grouped_verify_order_on_small_inputs(monkeypatch):
    """the processing order of the verify pass (reads grouped by read-level minimizer) is normally used from 4096 reads on;
    forced here on small, ragged and multi-segment inputs — results must not depend on it"""
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    for seed, n, lmin, lmax, cov in ((61, 700, 150, 150, 30.0), (67, 1500, 100, 250, 60.0), (71, 300, 400, 900, 20.0), (73, 65, 150, 150, 10.0)):
        assert_parity(_gen(seed, n, lmin, cov, lmax), 40, f"order{seed}")


def test_processing_order_is_a_grouped_permutation():
    """disco_get_query_order: the order the probe / verify passes walk is a permutation of the query range, and it keeps reads
    from the same genome locus together (generator coordinates: most neighbours in the order overlap on the genome)"""
    import torch
    n = 60_000
    spec = readgen.GenSpec.coverage(97, n, 150, 30.0, n_contigs=3)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        ptr = g.get_query_order()
        assert ptr, "grouping is on from 4096 reads"
        t = torch.empty(n, dtype=torch.int64, device="cuda")
        g.memcpy_d2d(t.data_ptr(), ptr, n * 8)
        g.synchronize()
        packed = t.cpu().numpy()
    order = packed & 0xFFFFFFFF  # entries carry the read's length in bits 47..32
    assert np.array_equal(packed >> 32, np.full(n, 150))
    assert np.array_equal(np.sort(order), np.arange(n))
    gpos, _, _ = readgen.read_locations(spec)
    d = np.abs(np.diff(gpos[order].astype(np.int64)))
    assert (d < 150).mean() > 0.8  # ~13 reads per group: 1 boundary in 13 neighbours (file order: 0.0002)


def test_probe_window_minimum_variants_agree(monkeypatch):
    """min-overlap 40 makes a window 17 m-mers and selects the DPP row-scan variant of probe_kernel; DISCO_NO_ROW17=1 forces the
    LDS range-minimum tables on the same data. Both must match the oracle (single- and multi-segment reads, > 128 windows)."""
    monkeypatch.setenv("DISCO_ORDER_MIN_READS", "1")
    cases = ((101, 900, 150, 150, 30.0), (103, 500, 100, 400, 40.0), (107, 200, 600, 1100, 15.0))
    for seed, n, lmin, lmax, cov in cases:
        assert_parity(_gen(seed, n, lmin, cov, lmax), 40, f"row17-{seed}")
    monkeypatch.setenv("DISCO_NO_ROW17", "1")
    for seed, n, lmin, lmax, cov in cases:
        assert_parity(_gen(seed, n, lmin, cov, lmax), 40, f"lds-{seed}")


def test_fall_back_kernel_choices_agree(monkeypatch):
    """every fall-back knob is parity-tested in both positions. These knobs pick another instantiation of the
    verify / selection / probe / index kernels (the host's kernel selectors own exactly these branches); each must give the oracle's graph
    on rows of at most 160 bases (the NW = 5 kernels) and on mixed lengths with heavy containment (NW = 8). The oracle runs once per
    read set; every run is held to what assert_parity holds it to."""
    from tests.util import run_hip_reads

    def check(reads, want, label, **kw):
        oe, orows, oc = want
        he, hr, hc = run_hip_reads(reads, 40, **kw)
        (ce, cc), (oce, occ) = canon_hip(he, hr), canon_hip(oe, orows)
        assert np.array_equal(cc, occ), f"{label}: contained rows differ ({len(cc)} vs {len(occ)})"
        assert np.array_equal(ce, oce), f"{label}: edge list differs ({len(ce)} vs {len(oce)})"
        for key in ("probes", "n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs"):
            assert hc[key] == oc[key], f"{label}: counter {key}: hip {hc[key]} oracle {oc[key]}"
        if kw:  # two passes: contained query reads are skipped by the second one, the counter counts what was compared
            assert 0 < hc["kmer_hits"] <= oc["kmer_hits"], label
        else:
            assert hc["kmer_hits"] == oc["kmer_hits"], f"{label}: counter kmer_hits: hip {hc['kmer_hits']} oracle {oc['kmer_hits']}"

    knobs = (("DISCO_NO_FLAT_VERIFY", "1"), ("DISCO_VERIFY_CACHE", "0"), ("DISCO_NO_FLAT_SELECT", "1"), ("DISCO_NO_RUNS", "1"))
    for name, reads in (("short", _gen(42, 5000, 150, 30.0, 150)), ("mixed", _gen(7, 4000, 100, 30.0, 250))):
        want = run_oracle_reads(reads, 40)
        for var, val in knobs:
            monkeypatch.setenv(var, val)
            check(reads, want, f"{name} {var}={val}")
            monkeypatch.delenv(var)
        if name == "mixed":  # verify_kernel<8, 1> and <8, 2>
            monkeypatch.setenv("DISCO_NO_FLAT_VERIFY", "1")
            check(reads, want, "mixed DISCO_NO_FLAT_VERIFY=1, two passes", flags=buildgraph.FLAG_TWO_PASS_VERIFY)
            monkeypatch.delenv("DISCO_NO_FLAT_VERIFY")


def test_caller_supplied_order_changes_nothing():
    """disco_set_query_order: any permutation of the query range (plain read ids) gives the same graph"""
    import torch
    n = 20_000
    spec = readgen.GenSpec.coverage(131, n, 100, 30.0, n_contigs=2, len_max=220)
    res = []
    for mode in ("own", "random", "reversed"):
        with buildgraph.BuildGraph(min_overlap=40) as g:
            g.generate_reads(spec)
            if mode == "random":
                perm = torch.randperm(n, dtype=torch.int64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
            elif mode == "reversed":
                perm = torch.arange(n - 1, -1, -1, dtype=torch.int64, device="cuda")
            if mode != "own":
                torch.cuda.synchronize()
                g.set_query_order(perm.data_ptr())
            g.run_graph()
            cnt = g.counters()
            e = np.sort(g.fetch_edges(), order=("src", "dst", "orient", "offset"))
            r = np.sort(g.fetch_contained(), order=("contained",))
            res.append((cnt["e_pre"], cnt["e_out"], cnt["n_contained"], cnt["kmer_hits"], e, r))
    for x in res[1:]:
        assert x[:4] == res[0][:4]
        assert np.array_equal(x[4], res[0][4]) and np.array_equal(x[5], res[0][5])


@pytest.mark.parametrize("name", ["mixed_4k", "long_2k", "k30_6k", "contigs_20k"])
def test_two_pass_verify_changes_no_result(name):
    """DISCO_FLAG_TWO_PASS_VERIFY (containment-type candidates first, then overlap-type candidates of non-contained reads):
    the same canonical output as the REAL reference's files; only the kmer_hits counter may count fewer compares"""
    from disco_amd import buildgraph
    from tests import golden_util as gu
    from tests.util import canon_hip

    reads, fidx, mo = gu.case_inputs(name)
    out = {}
    for flags in (0, buildgraph.FLAG_TWO_PASS_VERIFY):
        with buildgraph.BuildGraph(min_overlap=mo, flags=flags) as g:
            g.upload_ascii(reads)
            g.run_graph()
            out[flags] = (g.fetch_edges(), g.fetch_contained(), g.counters())
    ce, cc = canon_hip(out[1][0], out[1][1], fidx)
    gu.check_against_golden(name, ce, cc)
    c0, c1 = out[0][2], out[1][2]
    for k in ("n_contained", "e_pre", "e_out", "cap_bind_sites", "asymmetric_pairs"):
        assert c0[k] == c1[k], k
    # the diagnostic counters count what was compared: contained query reads are skipped by the second pass
    assert c1["kmer_hits"] <= c0["kmer_hits"] and c1["raw_hits"] <= c0["raw_hits"]


def test_two_pass_verify_on_repeats_equals_oracle():
    """order-dependent regime, mixed lengths: the two-pass form must still equal the oracle bit for bit"""
    from disco_amd import buildgraph
    from oracle import pyoracle
    from tests import golden_util as gu
    from tests.util import canon_hip

    reads, fidx, mo = gu.case_inputs("repeats_8k")
    with buildgraph.BuildGraph(min_overlap=mo, flags=buildgraph.FLAG_TWO_PASS_VERIFY) as g:
        g.upload_ascii(reads)
        g.run_graph()
        e, r, c = g.fetch_edges(), g.fetch_contained(), g.counters()
    ce, cc = canon_hip(e, r, fidx)
    oce, occ, ocnt = pyoracle.oracle_canonical(reads, fidx, mo)
    assert np.array_equal(cc, occ) and np.array_equal(ce, oce)
    assert c["e_pre"] == ocnt["e_pre"] and c["asymmetric_pairs"] == ocnt["asymmetric_pairs"]


def test_read_sets_of_the_same_shape_reuse_the_buffers():
    """a context that gets another read set of the same (n, stride) keeps every buffer (disco_upload_reads / disco_generate_reads:
    nothing freed, nothing re-allocated) — the results must be those of a fresh context, also when the new set needs MORE room
    (ten times the coverage: the hit buffer overflows and is regrown) and when it comes from the other entry point"""
    from tests.util import canon_hip

    n = 20_000
    specs = [readgen.GenSpec.coverage(61, n, 150, 20.0), readgen.GenSpec.coverage(62, n, 150, 200.0), readgen.GenSpec.coverage(63, n, 100, 30.0, len_max=250),
             readgen.GenSpec.coverage(64, n, 150, 30.0, n_contigs=3)]
    with buildgraph.BuildGraph(min_overlap=40) as g:
        for i, spec in enumerate(specs):
            if i % 2 == 0:
                g.generate_reads(spec)
            else:
                g.upload_ascii(readgen.generate_reads(spec))
            g.run_graph()
            got = canon_hip(g.fetch_edges(), g.fetch_contained())
            cnt = g.counters()
            with buildgraph.BuildGraph(min_overlap=40) as f:
                f.generate_reads(spec)
                f.run_graph()
                want = canon_hip(f.fetch_edges(), f.fetch_contained())
                wcnt = f.counters()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), i
            for k in ("e_pre", "e_out", "n_contained", "kmer_hits", "probes"):
                assert cnt[k] == wcnt[k], (i, k)


def test_hbm_bytes_do_not_drift_across_read_sets():
    """every device buffer is given back with the size it was allocated with: a context that ran A, B, A ends where one that ran B, A
    ends — the same edges and contained rows, and the same hbm_bytes (the buffers kept across read sets have seen the same sizes in both,
    so a free that accounts other bytes than its allocation shows as the difference of one extra cycle)"""
    a = readgen.GenSpec.coverage(71, 6000, 150, 30.0)
    b = readgen.GenSpec.coverage(72, 9000, 150, 30.0, long_len=600, long_share=1300)  # a tail of long reads: two classes of rows

    def run(specs):
        with buildgraph.BuildGraph(min_overlap=40) as g:
            for spec in specs:
                g.upload_ascii(readgen.generate_reads(spec))
                assert (g.long_rows > 0) == (spec is b), "B must take the two-class path (its long class is accounted too), A one stride"
                g.run_graph()
                res = canon_hip(g.fetch_edges(), g.fetch_contained())
            return res, g.counters()["hbm_bytes"]

    (e1, c1), hbm1 = run([a, b, a])
    (e2, c2), hbm2 = run([b, a])
    assert np.array_equal(e1, e2) and np.array_equal(c1, c2)
    assert hbm1 == hbm2 > 0, (hbm1, hbm2)


def test_cap_binds_in_short_rows():
    """rows of a handful of hits in which ONE window collects eight acceptable hits: read A ends 42 bases into a 45-base unit U,
    eight reads B_i start with U and continue into flanks of their own — A's suffix overlaps every B_i's prefix at the same window, the
    cap of four binds inside a register-sized row, which then takes the sequential accept scan with the row found through the header by
    position (the per-read arrays only serve rows of more than 64 entries: a kernel that looked there computed garbage or crashed —
    tools/ab_build.py -DES_EXP_STALE_ROWSTART rebuilds that defect). Twice on one context, behind a read set of another shape."""
    from disco_amd import buildgraph

    rng = np.random.default_rng(5)
    rnd = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    comp = str.maketrans("ACGT", "TGCA")
    reads = []
    for _ in range(12):
        u = rnd(45)
        reads.append(rnd(70) + u[:42])
        reads += [u + rnd(70) for _ in range(8)]
    genome = rnd(12000)
    for _ in range(1200):  # an ordinary 10x background around them
        L = int(rng.integers(90, 111))
        p = int(rng.integers(0, len(genome) - L))
        reads.append(genome[p:p + L])
    reads = [r.translate(comp)[::-1] if rng.random() < 0.5 else r for r in reads]
    perm = rng.permutation(len(reads))
    reads = [reads[i] for i in perm]
    c = assert_parity(reads, 40, "cap in short rows")
    assert c["cap_bind_sites"] >= 12 and c["asymmetric_pairs"] > 0
    oe, orows, oc = run_oracle_reads(reads, 40)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii([r[::-1] for r in reads[:700]])  # a different read set first: stale rows of another shape in every per-read array
        g.run_graph()
        g.upload_ascii(reads)
        g.run_graph()
        he, hr, hc = g.fetch_edges(), g.fetch_contained(), g.counters()
    ce, cc = canon_hip(he, hr)
    oce, occ = canon_hip(oe, orows)
    assert np.array_equal(ce, oce) and np.array_equal(cc, occ) and hc["cap_bind_sites"] == oc["cap_bind_sites"]


def test_contained_rows_grouped_on_the_device_are_the_sorted_rows():
    """disco_fetch_contained_grouped: the rows in the order of the contained-read files — (containing read, j, contained read) — sorted on the
    device during the pass; equal to the host sort of disco_fetch_contained's rows. A containing read with more than 256 rows makes it
    decline (the caller sorts)."""
    spec = readgen.GenSpec.coverage(seed=3, n_reads=60000, read_len=60, cov=40.0, len_max=250)  # mixed lengths: most reads contained
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        rows = g.fetch_contained()
        grouped = g.fetch_contained_grouped()
    assert grouped is not None and len(grouped) == len(rows) > 20000
    order = np.lexsort((rows["contained"], rows["j"], rows["super"]))
    assert np.array_equal(grouped, rows[order])
    assert len(np.unique(rows["super"])) < len(rows)  # groups of several rows exist
    # one long read that contains hundreds of short ones
    rng = np.random.default_rng(1)
    long_read = "".join(rng.choice(list("ACGT"), 3000))
    reads = [long_read] + [long_read[p:p + 80] for p in rng.integers(0, 2900, 400)]
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        g.run_graph()
        rows = g.fetch_contained()
        assert g.fetch_contained_grouped() is None and len(rows) >= 300


@pytest.mark.parametrize("sel_small,tr_small", [("0", "0"), ("1", "1"), ("1", "0"), ("0", "1")])
@pytest.mark.parametrize("seed,n,lmin,lmax,cov", [
    (42, 5000, 150, 150, 30.0),    # rows of more than 64 hits rare: the variants the defaults pick
    (17, 6000, 150, 150, 100.0),   # rows of 65..256 hits everywhere: forced small, every row goes through the big-row list and its 256-entry pass
    (29, 4000, 150, 150, 300.0),   # rows of 257..1024 hits, nodes of more than 128 / 256 neighbours: both passes over the list, big-node marking
    (19, 5000, 100, 250, 120.0),   # mixed lengths (containment inside wide rows)
])
def test_variants_of_selection_and_marking_agree(monkeypatch, sel_small, tr_small, seed, n, lmin, lmax, cov):
    """round 5: edge_select_flat_kernel<3, 2, true> (five waves per SIMD, sequential path in arrays of 64, longer rows listed) and
    transitive_mark_kernel<., ., 128> (eight waves, nodes beyond 128 neighbours listed) are picked by counts the kernels before them leave;
    forced either way they must give the oracle's graph on every coverage"""
    monkeypatch.setenv("DISCO_SELECT_SMALL", sel_small)
    monkeypatch.setenv("DISCO_TR_SMALL", tr_small)
    reads = _gen(seed, n, lmin, cov, lmax)
    c = assert_parity(reads, 40, f"variants{seed}")
    assert c["e_out"] > 0


def test_repeats_with_forced_small_variants(monkeypatch):
    """the order-dependent regime (cap binds, duplicates: rows fail the flat kernel's tests and take its sequential path in arrays of 64)"""
    monkeypatch.setenv("DISCO_SELECT_SMALL", "1")
    monkeypatch.setenv("DISCO_TR_SMALL", "1")
    test_repeats_order_dependent_regime()
    test_high_multiplicity_rows_take_the_big_paths()
