"""-m gpu : disco_write_gfa_chains through the C-ABI and buildG --gfa-unitigs — the compacted graph as GFA 1.0, every chain of the
contraction one segment whose bases are spelled on the GPU — against tests/gfa_chains_model.py: every byte against the model built from
disco_download_reads, disco_fetch_contained, disco_fetch_edges and what disco_contract_chains(0) returns on the same context (arrays that
are themselves held to tests/chain_model.py); hand-built sets at the word, class and piece boundaries with the counts a CPU run of the
oracle and the chain model gave; and, from the file alone, what its L lines claim about its segments and that every chain with its two
end reads spells a stretch of the genome the reads were cut from."""
import glob
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build, buildgraph, readgen
from tests import chain_model
from tests import gfa_chains_model as gcm
from tests import gfa_model
from tests.test_gpu_gfa import _SETS, _assert_same_lines, _tiling

pytestmark = pytest.mark.gpu

BIN = os.path.join(build.HERE, "bin")
_COMP = str.maketrans("ACGT", "TGCA")
E_STATE, E_UNSUPPORTED = -4, -6   # DISCO_E_STATE, DISCO_E_UNSUPPORTED (include/disco_hip.h)


def _rc(s):
    return s.translate(_COMP)[::-1]


def _tiling_genome(seed, lengths, step):
    """the genome _tiling(seed, lengths, step) cuts its reads from"""
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list("ACGT"), step * len(lengths) + max(lengths) + 1))


def _random(seed, n):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), n))


def _write(g, path, **kw):
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        size = g.write_gfa_chains(fd, **kw)
    finally:
        os.close(fd)
    text = open(path, "rb").read()
    assert size == len(text)
    return text


def _pass(g):
    """one pass and its contraction with every overlap counted: everything the model is built from, the contraction held to the chain model"""
    g.run_graph()
    packed, lens = g.download_reads()
    rows, edges = g.fetch_contained(), g.fetch_edges()
    comp, links, absorbed = g.contract_chains(0)
    cm = chain_model.chain_model(edges, lens, 0)
    assert np.array_equal(comp, cm.comp) and np.array_equal(links, cm.links) and np.array_equal(absorbed, cm.absorbed)
    contained = np.zeros(len(lens), dtype=np.uint8)
    contained[rows["contained"].astype(np.int64)] = 1
    return {"seqs": gfa_model.unpack(packed, lens), "lens": lens, "contained": contained, "edges": edges, "comp": comp, "links": links, "absorbed": absorbed,
            "rings": cm.rings, "interior": sorted(int(c["n_links"]) - 1 for c in comp)}


def _model(s, names=None, no_seq=False):
    names = np.arange(1, len(s["lens"]) + 1, dtype=np.uint64) if names is None else names
    return gcm.model(None if no_seq else s["seqs"], s["lens"], names, s["contained"], s["edges"], s["absorbed"], s["comp"], s["links"])


def _spells_a_genome(text, genomes):
    merged = gcm.merged_chains(text)
    for m in merged:
        m = m.decode()
        assert any(m in g or _rc(m) in g for g in genomes), (len(m), m[:60])
    return len(merged)


# ---- one long line ------------------------------------------------------------------------------------------------------------------
def test_a_chain_line_longer_than_a_piece(tmp_path):
    lengths, step = [100] * 2200, 40
    reads, genome = _tiling(2200, lengths, step), _tiling_genome(2200, lengths, step)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        s = _pass(g)
        whole = _write(g, tmp_path / "whole.gfa")
        pieces = _write(g, tmp_path / "pieces.gfa", piece_bytes=65536, threads=3)
    assert s["interior"] == [2198] and s["contained"].sum() == 0
    S, L = gcm.parse(whole)
    # LN = s_{m-1} + len[r_{m-1}]: 2198 interior reads 40 bases apart, 2197 * 40 + 100 — the 88 060 bases all 2200 reads cover less the
    # 40 bases each end read has to itself
    assert S[b"c0"][1] == 2197 * step + 100 == 87980 and S[b"c0"][2] == 2198 and len(S) == 3 and len(L) == 2
    line_at = whole.index(b"S\tc0\t")
    assert line_at < 65536 < line_at + 87980   # the line straddles the first two pieces of its section, which begins where it does
    _assert_same_lines(whole, _model(s))
    assert pieces == whole
    assert gcm.semantic_check(whole) == (2, 1, 2)
    merged = gcm.merged_chains(whole)[0].decode()
    assert len(merged) == 2199 * step + 100 == 88060 and merged in (genome[:88060], _rc(genome[:88060]))


# ---- the word and class boundaries of the read table, and reads that own one base or more than two words ------------------------------
def _no_flips(seed, lengths, step):
    genome = _random(seed, step * len(lengths) + max(lengths) + 1)
    return [genome[i * step:i * step + L] for i, L in enumerate(lengths)], genome


# name: (reads, genome, min-overlap, long rows expected, what the CPU run gave: contained reads, edges, interior reads per chain — or None)
def _boundary_sets():
    out = {}
    for name, key, minovl, classes, counts in (("words", "words", 20, False, (12, 17, [16])), ("classes", "classes-at-40", 40, True, (None, None, [15])),
                                               ("wide-stride", "classes-at-40", 20, False, None)):
        lengths = _SETS[key][0]
        out[name] = (_tiling(len(key), lengths, 9), _tiling_genome(len(key), lengths, 9), minovl, classes, counts)
    out["step1"] = (_tiling(70, [50] * 70, 1), _tiling_genome(70, [50] * 70, 1), 20, False, (0, None, [68]))
    reads, genome = _no_flips(5, [100] * 5, 70)
    out["step70"] = (reads, genome, 20, False, (0, 4, [3]))
    return out


_BSETS = _boundary_sets()


@pytest.mark.parametrize("name", list(_BSETS))
def test_chains_at_word_and_class_boundaries_spell_the_genome(tmp_path, name):
    reads, genome, minovl, classes, counts = _BSETS[name]
    with buildgraph.BuildGraph(min_overlap=minovl) as g:
        g.upload_ascii(reads)
        s = _pass(g)
        long_rows = g.long_rows
        text = _write(g, tmp_path / "b.gfa")
    assert (long_rows > 0) == classes
    if counts:
        n_contained, n_edges, interior = counts
        assert n_contained is None or s["contained"].sum() == n_contained
        assert n_edges is None or len(s["edges"]) == n_edges
        assert s["interior"] == interior
    assert len(s["comp"]) > 0
    offsets = np.concatenate([s["links"]["offset"][int(c["first_link"]) + 1:int(c["first_link"]) + int(c["n_links"])] for c in s["comp"]])
    if name == "words":
        assert offsets.min() == 9 and offsets.max() == 63
    if name == "classes":
        assert offsets.max() == 279 and any(s["lens"][int(l["to"])] > 256 for l in s["links"][gcm.interior(s["comp"], s["links"])])
    if name == "step1":
        assert (s["links"]["offset"][1:-1] == 1).all()
    if name == "step70":
        assert (s["links"]["offset"][1:-1] == 70).all()
    _assert_same_lines(text, _model(s))
    gcm.semantic_check(text)
    assert _spells_a_genome(text, [genome]) == len(s["comp"])


# ---- every kind of chain in one graph --------------------------------------------------------------------------------------------------
def _mixed():
    """(reads, the genomes they were cut from — the circular one doubled)"""
    reads, genomes = [], []

    def part(seed, lengths, step):
        reads.extend(_tiling(seed, lengths, step))
        genomes.append(_tiling_genome(seed, lengths, step))

    part(8, [100] * 2, 30)    # one edge, no chain
    part(9, [100] * 3, 45)    # a chain of one interior read
    ring = _random(60, 60 * 30)
    genomes.append(ring + ring)
    reads.extend((ring + ring)[30 * i:30 * i + 100] for i in range(60))   # a ring of absorbable nodes: left alone
    for n in (65, 66, 67):
        part(n, [100] * n, 7)
    repeat = _random(150, 150)   # two genomes that share a repeat: junction reads, chains between them
    for k, strand in ((1, False), (2, True)):
        genome = _random(950 + k, 400) + repeat + _random(960 + k, 400)
        genomes.append(genome)
        for i in range(0, 851, 10):
            reads.append(_rc(genome[i:i + 100]) if strand else genome[i:i + 100])
    return reads, genomes


@pytest.fixture(scope="module")
def mixed():
    reads, genomes = _mixed()
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        s = _pass(g)
        s.update(g=g, genomes=genomes, reads=reads, fidx=np.arange(len(reads), dtype=np.uint64) * np.uint64(3) + np.uint64(9_999_999_990))
        yield s


def test_the_mixed_set_is_what_the_cpu_run_gave(mixed):
    s = mixed
    assert len(s["lens"]) == 435 and s["contained"].sum() == 6 and len(s["edges"]) == 423
    assert s["interior"] == [1, 4, 39, 39, 39, 39, 63, 64, 65] and len(s["links"]) == 362
    assert len(s["rings"]) == 1 and int((s["absorbed"] == 0).sum()) == 61


@pytest.mark.parametrize("no_seq", [False, True], ids=["bases", "no-seq"])
@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "id+1"])
def test_mixed_bytes_equal_the_model(mixed, tmp_path, mapped, no_seq):
    s = mixed
    text = _write(s["g"], tmp_path / "m.gfa", file_index=s["fidx"] if mapped else None, no_seq=no_seq)
    _assert_same_lines(text, _model(s, s["fidx"] if mapped else None, no_seq))
    assert len(str(int(s["fidx"][-1]))) == 11
    n_reads, n_chains, n_l = gcm.semantic_check(text)
    inside = int(sum(s["interior"]))
    assert (n_reads, n_chains, n_l) == (435 - 6 - inside, 9, 61 + 2 * 9)
    if not no_seq:
        assert _spells_a_genome(text, s["genomes"]) == 9


# ---- a general read set ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("errors_ppm", [0, 1000], ids=["as-generated", "with-substitution-errors"])
def test_general_set_bytes_equal_the_model_pass_after_pass(tmp_path, errors_ppm):
    """tests/test_gpu_gfa.py's graph3k set. As generated it is ONE contig of error-free reads — one chain of 2711 interior reads, 287
    contained reads and no edge left over (CPU run of the oracle and the chain model) — so the set is run a second time with
    substitution errors in the reads (exact overlaps all the same: an error ends the overlaps across it), which leaves 270 chains, 328
    edges that went into none and 230 contained reads"""
    spec = readgen.GenSpec.coverage(seed=71, n_reads=3000, read_len=100, cov=20.0)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        if errors_ppm:
            g.substitute_bases(9, errors_ppm)
        s = _pass(g)
        text = _write(g, tmp_path / "g.gfa")
        _assert_same_lines(text, _model(s))
        n_reads, n_chains, n_l = gcm.semantic_check(text)
        inside, left_over = int(sum(s["interior"])), int((s["absorbed"] == 0).sum())
        assert n_chains == len(s["comp"]) > 0 and s["contained"].sum() > 0 and inside > 0 and n_l == left_over + 2 * n_chains
        assert left_over > 0 if errors_ppm else s["interior"] == [2711]
        assert n_reads + n_chains == 3000 - int(s["contained"].sum()) - inside + len(s["comp"])
        s2 = _pass(g)   # the same context once more: a new pass, a new contraction
        _assert_same_lines(_write(g, tmp_path / "g2.gfa"), _model(s2))


# ---- nothing to merge ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "apart"])
def test_nothing_to_merge(tmp_path, name):
    reads = _tiling(8, [100] * 2, 30) if name == "two" else [_random(900 + i, 100) for i in range(5)]
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        s = _pass(g)
        text = _write(g, tmp_path / "n.gfa")
    assert len(s["comp"]) == 0 and len(s["edges"]) == (1 if name == "two" else 0)
    assert text == _model(s)
    assert gcm.semantic_check(text) == (len(reads), 0, len(s["edges"]))


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def _code(g, path):
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        return int(g.L.disco_write_gfa_chains(g._h, fd, None, 0, 0, 1))
    finally:
        os.close(fd)


def test_limits(tmp_path):
    reads, _ = _mixed()
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        g.run_graph()
        assert _code(g, tmp_path / "early.gfa") == E_STATE          # no contraction yet
        g.contract_chains(0, edges=g.fetch_edges())
        assert _code(g, tmp_path / "host.gfa") == E_STATE           # the host holds the edges of that one
        assert os.path.getsize(tmp_path / "early.gfa") == 0 and os.path.getsize(tmp_path / "host.gfa") == 0
        s = _pass(g)
        assert _write(g, tmp_path / "late.gfa") == _model(s)        # the context is usable afterwards
    with buildgraph.BuildGraph(min_overlap=40, max_substitutions=2) as g:
        g.upload_ascii(reads)
        g.run_graph()
        g.contract_chains(0)
        assert _code(g, tmp_path / "subs.gfa") == E_UNSUPPORTED
        assert len(g.fetch_edges()) > 0


# ---- buildG --gfa-unitigs ----------------------------------------------------------------------------------------------------------------
def _buildg(tmp_path, sub, flags, cfg_extra=""):
    d = tmp_path / sub
    d.mkdir()
    fa = tmp_path / "mixed.fa"
    if not fa.exists():
        fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(_mixed()[0])))
    cfg = tmp_path / (sub + ".cfg")
    cfg.write_text("MinOverlap4BuildGraph = 40\n" + cfg_extra)
    cmd = [os.path.join(BIN, "buildG"), "-se", str(fa), "-f", str(d / "g"), "-p", str(cfg), "-t", "3"] + flags
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    return p, str(d / "g")


def _other_files(prefix):
    """every file of a run but the two GFAs; an edge file is its sorted lines (two runs write its lines in two orders), everything else bytes"""
    out = {}
    for p in sorted(glob.glob(prefix + "*")):
        key = p[len(prefix):]
        data = open(p, "rb").read()
        if key not in (".gfa", ".unitigs.gfa"):
            out[key] = sorted(data.splitlines(keepends=True)) if key.endswith("_parGraph.txt") else data
    return out


def test_buildg_gfa_unitigs(tmp_path, mixed):
    build.build_host()
    p0, plain = _buildg(tmp_path, "plain", [])
    p1, with_u = _buildg(tmp_path, "unitigs", ["--gfa-unitigs"])
    p2, both = _buildg(tmp_path, "both", ["--gfa", "--gfa-unitigs"])
    assert p0.returncode == 0 and p1.returncode == 0 and p2.returncode == 0, p0.stdout + p1.stdout + p2.stdout
    assert not os.path.exists(plain + ".unitigs.gfa") and not os.path.exists(with_u + ".gfa")
    a, b = _other_files(plain), _other_files(with_u)
    assert sorted(a) == sorted(b) and len(a) >= 8
    for key in a:
        assert a[key] == b[key], key
    text = open(with_u + ".unitigs.gfa", "rb").read()
    want = gcm.semantic_check(_model(mixed))   # (two runs number their edges, and so their chains, in two orders: the counts, not the bytes)
    assert gcm.semantic_check(text) == want == (435 - 6 - sum(mixed["interior"]), 9, 61 + 18)
    assert _spells_a_genome(text, mixed["genomes"]) == 9
    assert gcm.semantic_check(open(both + ".unitigs.gfa", "rb").read()) == want
    assert gfa_model.semantic_check(open(both + ".gfa", "rb").read()) == (435, 423, 6)


@pytest.mark.parametrize("how", ["gpus", "cli-substitutions", "file-substitutions"])
def test_buildg_gfa_unitigs_refusals(tmp_path, how):
    build.build_host()
    flags = {"gpus": ["--gpus", "2", "--same-device"], "cli-substitutions": ["--max-substitutions", "1"], "file-substitutions": []}[how]
    p, prefix = _buildg(tmp_path, "refused", ["--gfa-unitigs"] + flags, "MaxSubstitutions4BuildGraph = 1\n" if how == "file-substitutions" else "")
    assert p.returncode != 0 and "--gfa-unitigs" in p.stdout, p.stdout
    assert not glob.glob(prefix + "*")
