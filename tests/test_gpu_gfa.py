"""-m gpu : disco_write_gfa through the C-ABI and buildG --gfa — the reduced graph as GFA 1.0, formatted on the GPU piece by piece and sent
through the pinned ring into one file — against tests/gfa_model.py: every byte against the model built from disco_download_reads,
disco_fetch_edges, disco_fetch_contained and the index map; the S lines of hand-built sets at the word and class boundaries of the read
table against the strings that went in; and, from the file alone, what its L and C lines claim about its S lines."""
import glob
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build, buildgraph, readgen
from tests import gfa_model
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

BIN = os.path.join(build.HERE, "bin")
_COMP = str.maketrans("ACGT", "TGCA")


def _gfa(g, path, **kw):
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        size = g.write_gfa(fd, **kw)
    finally:
        os.close(fd)
    text = open(path, "rb").read()
    assert size == len(text)
    return text


def _assert_same_lines(got: bytes, want: bytes):
    g, w = got.split(b"\n"), want.split(b"\n")
    assert len(g) == len(w), (len(g), len(w))
    for i, (a, b) in enumerate(zip(g, w)):   # every line; the first one that differs is the one reported
        assert a == b, (i, a[:200], b[:200])
    assert got == want


@pytest.fixture(scope="module")
def graph3k():
    """test 1's set, one pass, shared: the context with its graph and the three arrays the model is built from"""
    spec = readgen.GenSpec.coverage(seed=71, n_reads=3000, read_len=100, cov=20.0)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        packed, lens = g.download_reads()
        yield {"g": g, "seqs": gfa_model.unpack(packed, lens), "lens": lens, "edges": g.fetch_edges(), "rows": g.fetch_contained(),
               # file indices as the input stage assigns them when records are filtered: increasing, with gaps, up to 11 digits
               "fidx": np.arange(spec.n_reads, dtype=np.uint64) * np.uint64(3) + np.uint64(9_999_999_990)}


@pytest.mark.parametrize("no_seq", [False, True], ids=["bases", "no-seq"])
@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "id+1"])
def test_gfa_bytes_equal_the_model(graph3k, tmp_path, mapped, no_seq):
    s = graph3k
    names = s["fidx"] if mapped else np.arange(1, len(s["lens"]) + 1, dtype=np.uint64)
    text = _gfa(s["g"], tmp_path / "g.gfa", file_index=s["fidx"] if mapped else None, no_seq=no_seq)
    want = gfa_model.model(None if no_seq else s["seqs"], s["lens"], names, s["edges"], None, s["rows"])
    assert len(s["edges"]) > 0 and len(s["rows"]) > 0 and len(str(int(s["fidx"][-1]))) == 11
    _assert_same_lines(text, want)


def _tiling(seed, lengths, step):
    """reads of the given lengths laid along one random genome, `step` bases apart, every third one from the other strand"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), step * len(lengths) + max(lengths) + 1))
    reads = []
    for i, L in enumerate(lengths):
        s = genome[i * step:i * step + L]
        reads.append(s.translate(_COMP)[::-1] if i % 3 == 2 else s)
    return reads


_BOUNDARY = [31, 32, 33, 63, 64, 65, 127, 128, 129, 160]
_LONG = [257, 300, 450, 1000, 999, 640, 641]
_CLASSES = [255, 256, 200, 120, 180, 256, 96, 224, 225, 255] * 6
# name: (lengths, min-overlap, two classes of rows expected)
_SETS = {
    "words": (_BOUNDARY * 3, 20, False),
    # A table goes to two classes of rows only where the short class can take the minimizer runs (two_class_ok, disco_hip.hip): with reads
    # of up to 256 bases that needs a window of at least 10 m-mers of 23 bases, min-overlap 33 or more — at min-overlap 20 (k = 19, m = 19:
    # one m-mer a window) the same set is one stride of 32 words. Both are run: the set at 20, and at 40 with the classes asserted.
    "classes-at-40": (_CLASSES[:30] + _LONG[:4] + _CLASSES[30:] + _LONG[4:], 40, True),
    "classes-set-at-20": (_CLASSES[:30] + _LONG[:4] + _CLASSES[30:] + _LONG[4:], 20, False),
    "wide-stride": ([300, 600, 301, 352, 353, 383, 384, 385, 599, 415, 416, 417, 447, 448, 449, 480, 511, 512, 513, 575, 576, 577, 330, 600], 20, False),
}


@pytest.mark.parametrize("name", list(_SETS))
def test_gfa_s_lines_at_word_and_class_boundaries_are_the_input(tmp_path, name):
    lengths, minovl, classes = _SETS[name]
    reads = _tiling(len(name), lengths, 9)
    with buildgraph.BuildGraph(min_overlap=minovl) as g:
        g.upload_ascii(reads)
        g.run_graph()
        long_rows = g.long_rows
        text = _gfa(g, tmp_path / "b.gfa")
    if classes:
        assert long_rows == sum(L > 256 for L in lengths) > 0 and long_rows * 5 <= len(reads)
    else:
        assert long_rows == 0
    S, L, C = gfa_model.parse(text)
    assert [S[i + 1] for i in range(len(reads))] == [(r.encode(), len(r)) for r in reads]
    assert len(S) == len(reads) and len(L) > 0   # (the reads overlap: every decode path under L and C lines that read it back)
    gfa_model.semantic_check(text)


def test_gfa_lines_say_what_the_sequences_show(graph3k, tmp_path):
    """the file alone, exact overlaps: no model, no fetch"""
    s = graph3k
    n_s, n_l, n_c = gfa_model.semantic_check(_gfa(s["g"], tmp_path / "s.gfa", file_index=s["fidx"]))
    assert n_s == len(s["lens"]) and n_l == len(s["edges"]) > 0 and n_c == len(s["rows"]) > 0


def test_gfa_lines_say_what_the_sequences_show_with_substitutions(tmp_path):
    """max_substitutions = 2 over reads with substitution errors: every L line's mismatches are its NM tag, at most 2; every C line's at most 2"""
    spec = readgen.GenSpec.coverage(seed=73, n_reads=3000, read_len=100, cov=25.0, len_max=170)
    with buildgraph.BuildGraph(min_overlap=40, max_substitutions=2) as g:
        g.generate_reads(spec)
        g.substitute_bases(9, 5000)
        g.run_graph()
        subs = g.fetch_edge_substitutions()
        n_rows = len(g.fetch_contained())
        text = _gfa(g, tmp_path / "x.gfa")
    S, L, C = gfa_model.parse(text)
    assert [nm for *_, nm in L] == [int(x) for x in subs]   # (the order of disco_fetch_edges)
    assert len(L) == len(subs) > 0 and len(C) == n_rows > 0 and 0 < max(subs) <= 2
    gfa_model.semantic_check(text, max_subs=2)


def test_gfa_in_small_pieces_is_the_same_file(tmp_path):
    spec = readgen.GenSpec.coverage(seed=71, n_reads=6000, read_len=150, cov=20.0)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        g.run_graph()
        whole = _gfa(g, tmp_path / "whole.gfa")
        small = _gfa(g, tmp_path / "small.gfa", piece_bytes=65536, threads=3)
        tiny = _gfa(g, tmp_path / "tiny.gfa", piece_bytes=1)   # (below 64 KiB: raised to it)
    assert len(small) >= 10 * 65536   # a piece holds at most 65 536 bytes: at least 10 of them
    _assert_same_lines(small, whole)
    assert tiny == whole
    assert gfa_model.semantic_check(whole)[0] == 6000


def test_gfa_limits(tmp_path):
    spec = readgen.GenSpec.coverage(seed=42, n_reads=3000, read_len=100, cov=20.0)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.generate_reads(spec)
        with pytest.raises(buildgraph.DiscoError, match="disco_transitive_reduce"):
            _gfa(g, tmp_path / "early.gfa")   # no graph yet
        g.run_graph()
        fd = os.open(str(tmp_path / "flags.gfa"), os.O_WRONLY | os.O_CREAT, 0o644)
        with pytest.raises(buildgraph.DiscoError, match="unknown flags"):
            g._chk(g.L.disco_write_gfa(g._h, fd, None, 6, 0, 1))
        os.close(fd)
        assert os.path.getsize(tmp_path / "flags.gfa") == 0
        assert _gfa(g, tmp_path / "late.gfa").startswith(gfa_model.HEADER)
    ranks = [buildgraph.BuildGraph(min_overlap=40) for _ in range(2)]
    try:
        buildgraph.BuildGraph.comm_init_local(ranks)
        with pytest.raises(buildgraph.DiscoError, match="error -6"):   # DISCO_E_UNSUPPORTED
            _gfa(ranks[0], tmp_path / "rank.gfa")
    finally:
        for r in ranks:
            r.close()


# ---- buildG --gfa ------------------------------------------------------------------------------------------------------------------
def _inputs(name, tmp_path):
    c = gu.CASES[name]
    if c["kind"] == "generated":
        reads, _, _ = gu.case_inputs(name)
        fa = tmp_path / (name + ".fa")
        fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
        return ["-se", str(fa)]
    return ["-pe", ",".join(os.path.join(gu.GOLD, f) for f in c["pe"]), "-se", ",".join(os.path.join(gu.GOLD, f) for f in c["se"])]


def _buildg(tmp_path, name, sub, flags):
    d = tmp_path / sub
    d.mkdir()
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {gu.CASES[name]['min_overlap']}\n")
    cmd = [os.path.join(BIN, "buildG")] + _inputs(name, tmp_path) + ["-f", str(d / "g"), "-p", str(cfg), "-t", "3"] + flags
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    return p, str(d / "g")


def _other_files(prefix):
    """every file of a run but the GFA. The edges leave the reduction through one counting atomic, so two runs write the lines of an edge
    file in two orders (tests/test_host_output_matrix.py compares them the same way): an edge file is its sorted lines, everything else bytes"""
    out = {}
    for p in sorted(glob.glob(prefix + "*")):
        key = p[len(prefix):]
        data = open(p, "rb").read()
        if key != ".gfa":
            out[key] = sorted(data.splitlines(keepends=True)) if key.endswith("_parGraph.txt") else data
    return out


@pytest.mark.parametrize("name", ["u150_5k", "multifile"])
def test_buildg_gfa_is_the_cases_graph_and_changes_no_other_file(tmp_path, name):
    build.build_host()
    p0, plain = _buildg(tmp_path, name, "plain", [])
    p1, with_gfa = _buildg(tmp_path, name, "gfa", ["--gfa"])
    assert p0.returncode == 0 and p1.returncode == 0, p0.stdout + p1.stdout
    assert not os.path.exists(plain + ".gfa")
    a, b = _other_files(plain), _other_files(with_gfa)
    assert sorted(a) == sorted(b) and len(a) >= 8
    for key in a:
        assert a[key] == b[key], key
    text = open(with_gfa + ".gfa", "rb").read()
    S, L, C = gfa_model.parse(text)
    gfa_model.semantic_check(text)
    # S names: the file indices of the good reads, inside the ranges <prefix>_ReadIDMap.txt gives the files
    reads, fidx, _ = gu.case_inputs(name)
    assert list(S) == [int(x) for x in fidx] and [S[int(x)][0].decode() for x in fidx] == list(reads)
    ranges = [tuple(int(v) for v in l[len("ReadID Range: ("):-1].split(",")) for l in open(with_gfa + "_ReadIDMap.txt").read().splitlines() if l.startswith("ReadID Range")]
    assert ranges and all(any(lo <= x <= hi for lo, hi in ranges) for x in S)
    if "good_reads_per_file" in gu.CASES[name]:
        assert [sum(lo <= x <= hi for x in S) for lo, hi in ranges] == gu.CASES[name]["good_reads_per_file"]
    # L lines back to (src, dst, orient, offset): the canonical edge set of the reference-made fixture
    want_e = set()
    for l in open(os.path.join(gu.GOLD, name + ".edges.txt")):
        s_, d_, info = l.rstrip("\n").split("\t")
        f = info.split(",")
        want_e.add((int(s_), int(d_), int(f[0]), int(f[5])))
    got_e = [(src, dst, (2 if so == "+" else 0) | (1 if do == "+" else 0), S[src][1] - ovl) for src, so, dst, do, ovl, _ in L]
    assert len(got_e) == len(want_e) == gu.CASES[name]["n_edges"] and set(got_e) == want_e
    # C lines: the fixture's contained rows, in count and pairs
    want_c = sorted(tuple(int(x) for x in l.split("\t")[:2]) for l in open(os.path.join(gu.GOLD, name + ".contained.txt")))
    assert sorted((con, sup) for sup, con, _, _, _ in C) == want_c and len(C) == gu.CASES[name]["n_contained"]
    # and without the bases
    p2, no_seq = _buildg(tmp_path, name, "noseq", ["--gfa-no-seq"])
    assert p2.returncode == 0, p2.stdout
    assert open(no_seq + ".gfa", "rb").read().splitlines()[1:len(S) + 1] == [b"S\t%d\t*\tLN:i:%d" % (k, v[1]) for k, v in S.items()]


def test_buildg_gfa_refuses_several_gpus(tmp_path):
    build.build_host()
    p, prefix = _buildg(tmp_path, "multifile", "ranks", ["--gfa", "--gpus", "2", "--same-device"])
    assert p.returncode != 0 and "--gfa writes the graph of one GPU" in p.stdout
    assert not glob.glob(prefix + "*")
