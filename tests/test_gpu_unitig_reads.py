"""-m gpu : disco_write_unitig_reads through the C-ABI and buildG --unitig-reads / --unitig-depth — every read placed on its segment of
the compacted graph, roots found by pointer doubling on the GPU — against tests/unitig_reads_model.py: every byte against the model
built from disco_fetch_contained, disco_fetch_edges, disco_contract_chains(0) and disco_download_reads on the same context; from the
files alone, that bases [start, start + len) of the segment <prefix>.unitigs.gfa of the same context spells are the read; and the counts
a CPU run of the oracle and the chain model gave for every set."""
import glob
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build, buildgraph, readgen
from tests import gfa_model
from tests import unitig_reads_model as urm
from tests.test_gpu_gfa_chains import _buildg, _mixed
from tests.test_unitig_reads_host import nest_reads

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_UNSUPPORTED = -1, -4, -6   # DISCO_E_ARG, DISCO_E_STATE, DISCO_E_UNSUPPORTED (include/disco_hip.h)


def _to_file(write, path, **kw):
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        size = write(fd, **kw)
    finally:
        os.close(fd)
    text = open(path, "rb").read()
    assert size == len(text)
    return text


def _pass(g):
    """one pass and its contraction with every overlap counted: everything the model is built from"""
    g.run_graph()
    packed, lens = g.download_reads()
    rows, edges = g.fetch_contained(), g.fetch_edges()
    comp, links, absorbed = g.contract_chains(0)
    return {"seqs": gfa_model.unpack(packed, lens), "lens": lens, "rows": rows, "edges": edges, "comp": comp, "links": links, "absorbed": absorbed}


def _model(s, names=None, depth_only=False):
    names = np.arange(1, len(s["lens"]) + 1, dtype=np.uint64) if names is None else names
    return urm.model(s["lens"], names, s["rows"], s["comp"], s["links"], depth_only)


def _assert_same_lines(got: bytes, want: bytes):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):   # the first line that differs is the one reported
        assert a == b, (i, a[:200], b[:200])
    assert got == want


def _figures(s, text):
    """what the sets are pinned by, read off the file and the arrays of the same context"""
    U, R = urm.parse(text)
    contained = set(s["rows"]["contained"].astype(np.int64).tolist())
    names = [r[0] for r in R]
    hist = np.bincount([r[6] for r in R]).tolist()
    return {"contained": len(s["rows"]), "edges": len(s["edges"]), "chains": len(s["comp"]), "links": len(s["links"]), "left_over": int((s["absorbed"] == 0).sum()),
            "hops": hist, "on_chains": sum(r[1].startswith(b"c") for r in R), "minus": sum(r[2] == "-" for r in R),
            "contained_on_chains": sum(r[1].startswith(b"c") for i, r in enumerate(R) if i in contained),
            "contained_on_reads": sum(not r[1].startswith(b"c") for i, r in enumerate(R) if i in contained),
            "largest_reads": max(u[2] for u in U), "on_c0": sum(r[1] == b"c0" for r in R), "n": len(names)}


_MIXED_4K = dict(seed=7, n_reads=4000, read_len=100, cov=30.0, len_max=250)
_GRAPH3K = dict(seed=71, n_reads=3000, read_len=100, cov=20.0)
# name: (reads or generator settings, substitution errors per million, the figures a CPU run of the oracle and the chain model gave)
_SETS = {
    "nest": (nest_reads, 0, {"n": 143, "contained": 69, "edges": 73, "chains": 1, "links": 73, "left_over": 0, "on_c0": 141, "hops": [74] + [1] * 69}),
    "mixed_4k": (_MIXED_4K, 0, {"contained": 3049, "edges": 950, "chains": 1, "links": 950, "hops": [951, 1930, 912, 193, 14], "on_c0": 3996, "minus": 2023}),
    "mixed_4k-errors": (_MIXED_4K, 1000, {"contained": 2535, "edges": 2034, "chains": 231, "links": 613, "left_over": 1421, "hops": [1465, 1702, 693, 134, 6],
                                          "contained_on_chains": 830, "contained_on_reads": 1705, "largest_reads": 29}),
    "graph3k": (_GRAPH3K, 0, {"contained": 287, "chains": 1, "links": 2712, "on_c0": 2998}),
    "graph3k-errors": (_GRAPH3K, 1000, {"contained": 230, "chains": 270, "left_over": 328, "contained_on_reads": 35, "largest_reads": 57}),
}


@pytest.mark.parametrize("name", list(_SETS))
def test_set_bytes_equal_the_model_and_hold_against_the_bases(tmp_path, name):
    what, errors_ppm, want = _SETS[name]
    with buildgraph.BuildGraph(min_overlap=40) as g:
        if callable(what):
            g.upload_ascii(what())
        else:
            g.generate_reads(readgen.GenSpec.coverage(**what))
            if errors_ppm:
                g.substitute_bases(9, errors_ppm)
        s = _pass(g)
        cnt = g.counters()
        gfa = _to_file(g.write_gfa_chains, tmp_path / "u.gfa")
        text = _to_file(g.write_unitig_reads, tmp_path / "u.reads")
        pieces = _to_file(g.write_unitig_reads, tmp_path / "p.reads", piece_bytes=65536, threads=3)
        depth = _to_file(g.write_unitig_reads, tmp_path / "d.reads", depth_only=True)
        if name == "graph3k-errors":   # the same context once more: a new pass, a new contraction
            s2 = _pass(g)
            _assert_same_lines(_to_file(g.write_unitig_reads, tmp_path / "u2.reads"), _model(s2))
    assert cnt["cap_bind_sites"] == 0 and cnt["asymmetric_pairs"] == 0
    _assert_same_lines(text, _model(s))
    assert pieces == text and depth == _model(s, depth_only=True)
    n_u, n_r, on_chains, minus, hops = urm.semantic_check(text, gfa, s["seqs"])
    assert n_r == len(s["lens"]) and urm.depth_only_is_prefix(depth, text) == n_u
    got = _figures(s, text)
    assert (got["on_chains"], got["minus"], got["hops"]) == (on_chains, minus, hops)
    print(name, got)
    assert {k: got[k] for k in want} == want
    if name == "nest":
        R = urm.parse(text)[1]
        assert R[0][5:] == (b"70", 69) and R[0][1] == b"c0"                 # read 0: 69 hops to read id 69
        r69, r0 = R[69], R[0]
        assert r0[2] == r69[2] and abs(r0[3] - r69[3]) in (34, len(s["seqs"][69]) - 34 - len(s["seqs"][0]))   # base 34 of its root, on its strand
        assert sorted(r[1] for r in R if not r[1].startswith(b"c")) == sorted(b"%d" % (int(v) + 1) for v in (s["comp"][0]["a"], s["comp"][0]["b"]))
    if name == "mixed_4k":
        assert len(text) > 3 * (65536 - 32832)   # the pieces above were several: one takes the lines that start in 65536 - GFA_MAX_LINE bytes


# ---- every kind of chain in one graph: names, a ring's reads as segments ------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    reads, _ = _mixed()
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        s = _pass(g)
        s.update(g=g, fidx=np.arange(len(reads), dtype=np.uint64) * np.uint64(3) + np.uint64(10_000_000_011))
        yield s


@pytest.mark.parametrize("depth_only", [False, True], ids=["reads", "depth-only"])
@pytest.mark.parametrize("mapped", [True, False], ids=["mapped", "id+1"])
def test_mixed_bytes_equal_the_model(mixed, tmp_path, mapped, depth_only):
    s = mixed
    fidx = s["fidx"] if mapped else None
    assert len(s["lens"]) == 435 and len(s["rows"]) == 6 and len(s["comp"]) == 9 and all(len(str(int(v))) == 11 for v in s["fidx"])
    text = _to_file(s["g"].write_unitig_reads, tmp_path / "m.reads", file_index=fidx, depth_only=depth_only)
    _assert_same_lines(text, _model(s, fidx, depth_only))
    U, R = urm.parse(text)
    inside = sum(int(c["n_links"]) - 1 for c in s["comp"])
    assert len(U) == 435 - 6 - inside + 9 and len(R) == (0 if depth_only else 435)
    if not depth_only:
        gfa = _to_file(s["g"].write_gfa_chains, tmp_path / "m.gfa", file_index=fidx)
        urm.semantic_check(text, gfa, s["seqs"], fidx)
        # the ring's sixty reads (ids 5 .. 64) are segments of their own
        ring = {b"%d" % (int(fidx[i]) if mapped else i + 1) for i in range(5, 65)}
        assert ring <= {u[0] for u in U} and all(r[1] == r[0] for r in R if r[0] in ring)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def _code(g, path, flags=0):
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        return int(g.L.disco_write_unitig_reads(g._h, fd, None, flags, 0, 1))
    finally:
        os.close(fd)


def test_limits(tmp_path):
    reads, _ = _mixed()
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(reads)
        g.run_graph()
        assert _code(g, tmp_path / "early.reads") == E_STATE          # no contraction yet
        g.contract_chains(0, edges=g.fetch_edges())
        assert _code(g, tmp_path / "host.reads") == E_STATE           # the host holds the edges of that one
        g.contract_chains(0)
        assert _code(g, tmp_path / "flags.reads", 2) == E_ARG         # an unknown flag
        assert all(os.path.getsize(tmp_path / f) == 0 for f in ("early.reads", "host.reads", "flags.reads"))
        s = _pass(g)
        assert _to_file(g.write_unitig_reads, tmp_path / "late.reads") == _model(s)   # the context is usable afterwards
    with buildgraph.BuildGraph(min_overlap=40, max_substitutions=2) as g:
        g.upload_ascii(reads)
        g.run_graph()
        g.contract_chains(0)
        assert _code(g, tmp_path / "subs.reads") == E_UNSUPPORTED
        assert os.path.getsize(tmp_path / "subs.reads") == 0
        assert len(g.fetch_edges()) > 0


# ---- buildG --unitig-reads, --unitig-depth ----------------------------------------------------------------------------------------------
def _files(prefix, but=()):
    """every file of a run but the named ones; an edge file is its sorted lines (two runs write its lines in two orders), everything else bytes"""
    out = {}
    for p in sorted(glob.glob(prefix + "*")):
        key = p[len(prefix):]
        data = open(p, "rb").read()
        if key not in but:
            out[key] = sorted(data.splitlines(keepends=True)) if key.endswith("_parGraph.txt") else data
    return out


def test_buildg_unitig_reads(tmp_path):
    build.build_host()
    reads = [r.encode() for r in _mixed()[0]]
    runs = {"plain": [], "reads": ["--unitig-reads"], "depth": ["--unitig-depth"], "both-flags": ["--unitig-depth", "--unitig-reads"],
            "with-gfa": ["--gfa-unitigs", "--unitig-reads"], "depth-with-gfa": ["--gfa-unitigs", "--unitig-depth"]}
    prefix = {}
    for sub, flags in runs.items():
        p, prefix[sub] = _buildg(tmp_path, sub, flags)
        assert p.returncode == 0, p.stdout
    plain = _files(prefix["plain"])
    assert len(plain) >= 8 and not any(k.startswith(".unitigs") for k in plain)      # no new file without a flag
    for sub, flags in runs.items():
        new = {".unitigs.reads"} if sub != "plain" else set()
        if "--gfa-unitigs" in flags:
            new.add(".unitigs.gfa")
        got = _files(prefix[sub])
        assert set(got) == set(plain) | new, sub
        for key in plain:
            assert got[key] == plain[key], (sub, key)
    # two runs number their edges, and so their chains, in two orders: each pair is held by what it says, and the counts agree
    full = open(prefix["with-gfa"] + ".unitigs.reads", "rb").read()
    want = urm.semantic_check(full, open(prefix["with-gfa"] + ".unitigs.gfa", "rb").read(), reads)
    assert want[:2] == (435 - 6 - 353 + 9, 435) and want[4][0] == 429 and sum(want[4]) == 435
    depth = open(prefix["depth-with-gfa"] + ".unitigs.reads", "rb").read()
    U, R = urm.parse(depth)
    assert not R and len(U) == want[0] and sorted(u[1:] for u in U) == sorted(u[1:] for u in urm.parse(full)[0])
    for sub in ("reads", "both-flags"):
        U1, R1 = urm.parse(open(prefix[sub] + ".unitigs.reads", "rb").read())
        assert len(R1) == 435 and len(U1) == want[0]
    alone = open(prefix["depth"] + ".unitigs.reads", "rb").read()
    assert urm.depth_only_is_prefix(alone, alone) == want[0]


@pytest.mark.parametrize("flag", ["--unitig-reads", "--unitig-depth"])
@pytest.mark.parametrize("how", ["gpus", "cli-substitutions", "file-substitutions"])
def test_buildg_unitig_reads_refusals(tmp_path, how, flag):
    build.build_host()
    flags = {"gpus": ["--gpus", "2", "--same-device"], "cli-substitutions": ["--max-substitutions", "1"], "file-substitutions": []}[how]
    p, prefix = _buildg(tmp_path, "refused", [flag] + flags, "MaxSubstitutions4BuildGraph = 1\n" if how == "file-substitutions" else "")
    assert p.returncode != 0 and flag in p.stdout, p.stdout
    assert not glob.glob(prefix + "*")
