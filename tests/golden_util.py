"""load the committed golden cases (tests/golden/cases.json, made by tests/golden/make_golden.py with the REAL reference)"""
from __future__ import annotations

import json
import os

import numpy as np

from disco_amd import readgen
from oracle import pyoracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = json.load(open(os.path.join(GOLD, "cases.json")))
COMP = str.maketrans("ACGT", "TGCA")


def repeat_reads(seed, n_reads, copies, rep_len, flank, lmin, lmax):
    """same construction as tests/golden/make_golden.py:repeat_reads"""
    rng = np.random.default_rng(seed)
    rep = "".join(rng.choice(list("ACGT"), rep_len))
    genome = "".join("".join(rng.choice(list("ACGT"), flank)) + rep for _ in range(copies))
    reads = []
    for _ in range(n_reads):
        L = int(rng.integers(lmin, lmax + 1))
        p = int(rng.integers(0, len(genome) - L))
        s = genome[p:p + L]
        reads.append(s.translate(COMP)[::-1] if rng.random() < 0.5 else s)
    return reads


def case_inputs(name):
    """returns (good reads, file index array (1-based over all records), min_overlap)"""
    c = CASES[name]
    mo = c["min_overlap"]
    if c["kind"] == "generated":
        reads = readgen.generate_reads(readgen.GenSpec.coverage(**c["spec"]))
        return reads, np.arange(1, len(reads) + 1, dtype=np.uint64), mo
    if c["kind"] == "repeats":
        reads = repeat_reads(*c["args"])
        return reads, np.arange(1, len(reads) + 1, dtype=np.uint64), mo
    if c["kind"] == "file":
        paths = [os.path.join(GOLD, f) for f in c["files"]]
    else:
        paths = [os.path.join(GOLD, f) for f in c["pe"] + c["se"]]
    reads, fidx, _total = pyoracle.load_good_reads(paths, mo)
    return reads, fidx, mo


def check_against_golden(name, edges_canon, contained_canon):
    c = CASES[name]
    et, ct = pyoracle.edges_text(edges_canon), pyoracle.contained_text(contained_canon)
    if c["full_text"]:
        assert et == open(os.path.join(GOLD, name + ".edges.txt")).read(), f"{name}: edge list differs from the reference"
        assert ct == open(os.path.join(GOLD, name + ".contained.txt")).read(), f"{name}: contained rows differ from the reference"
    assert len(edges_canon) == c["n_edges"] and len(contained_canon) == c["n_contained"], (name, len(edges_canon), c["n_edges"])
    assert pyoracle.digest(et) == c["edges_sha256"], f"{name}: edge digest differs from the reference"
    assert pyoracle.digest(ct) == c["contained_sha256"], f"{name}: contained digest differs from the reference"


BIT_EXACT_CASES = [n for n, c in CASES.items() if c["kind"] != "repeats"]


# recorded.json: the reference's output where the tests cannot always run it (tests/golden/make_golden.py --parsimplify / --live-small),
# as SHA-256 and size like the larger cases of cases.json: "parsimplify" = the reference parsimplify with its uninitialised-length
# defect repaired on partial_edge_file(<case>, <whole|split>), the lines as par_lines returns them
RECORDED = json.load(open(os.path.join(GOLD, "recorded.json")))
PS_CASES = ["u150_5k", "mixed_4k", "k30_6k", "k64_3k", "long_2k", "multifile"]


def partial_edge_file(name, split, path):
    """the edge file of a golden case as one parsimplify input: every edge flagged 2 (both ends owned), or — split — a file that owns
    only the lower half of the nodes, edges to the other half carrying flags 0 / 1. Returns the number of edges in the case."""
    lines = [l.rstrip("\n") for l in open(os.path.join(GOLD, name + ".edges.txt")) if l.strip()]
    ids = sorted({int(x) for l in lines for x in l.split("\t")[:2]})
    cut = ids[len(ids) // 2]
    with open(path, "w") as f:
        for l in lines:
            a, b = (int(x) for x in l.split("\t")[:2])
            if not split:
                f.write(l + ",2\n")
            elif a < cut or b < cut:
                f.write(l + ("," + ("2" if (a < cut and b < cut) else "0" if a < cut else "1")) + "\n")
    return len(lines)


def par_lines(path, drop_length=False):
    """sorted lines of a ParSimpleEdges file; drop_length: without the edge-length column (offset + length of the destination),
    which the STOCK reference fills from uninitialised members on some composite edges (SG/EdgeSimple.cpp:50-71); fullsimplify never
    reads that column (SG/OverlapGraph.cpp:2028-2094 takes fields 0, 1 and 5)"""
    out = []
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        info = f[2].split(",")
        out.append("\t".join(f[:2] + [",".join(info[:2] + info[3:]) if drop_length else f[2]] + f[3:]))
    return sorted(out)


def check_recorded_par_lines(name, split, lines):
    r = RECORDED["parsimplify"][f"{name}.{'split' if split else 'whole'}"]
    assert len(lines) == r["n_lines"], (name, split, len(lines), r["n_lines"])
    assert pyoracle.digest("".join(l + "\n" for l in lines)) == r["sha256"], f"{name} split={split}: lines differ from the reference parsimplify"
