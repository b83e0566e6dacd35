"""The line and item functions behind <prefix>.gfa (disco_amd/csrc/disco_gfa.h) without a GPU: disco_amd/bin/gfa_check builds the header
the kernels include as plain C++ and writes a described case the way disco_write_gfa does — the S lines word by word, in the kernels'
two passes over the three layouts of the read table; the text must be tests/gfa_model.py's. Once more under AddressSanitizer and
UBSan: every store of every item inside the bytes its line measured."""
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build
from disco_amd.buildgraph import CONTAINED_DTYPE, EDGE_DTYPE
from tests import gfa_model

BIN = os.path.join(build.HERE, "bin")
BOUNDARY = [31, 32, 33, 63, 64, 65, 127, 128, 129, 160]
# name: (lengths, layout, stride words, 11-digit file indices)
SETS = {
    "five-word-rows": (BOUNDARY, 0, 5, False),
    "five-word-rows-mapped": (BOUNDARY, 0, 5, True),
    "two-classes": ([255, 256, 257, 40, 300, 1000, 288, 289, 96, 1, 320, 321, 250, 8, 9, 512, 513] + [100] * 8, 1, 32, True),
    "one-wide-stride": ([300, 600, 301, 352, 353, 383, 384, 385, 599, 97, 32], 0, 19, False),
}


def _case(name, no_seq, has_nm):
    lens, layout, stride, mapped = SETS[name]
    rng = np.random.default_rng(len(name) * 7 + stride)
    n = len(lens)
    seqs = ["".join(rng.choice(list("ACGT"), L)).encode() for L in lens]
    names = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(9_999_999_993) if mapped else np.arange(1, n + 1, dtype=np.uint64)
    edges = np.zeros(4 * (n - 1), dtype=EDGE_DTYPE)   # every orientation between neighbours; offsets from 0 to the last base
    for x in range(len(edges)):
        s = x // 4
        edges[x] = (s, s + 1, x % 4, int(rng.integers(0, lens[s])), lens[s], lens[s + 1])
    subs = rng.integers(0, 12, len(edges)).astype(np.uint16)   # one and two digits
    rows = []   # every orientation — both position branches, both signs — wherever a read fits into another one
    for a in range(n):
        for b in range(n):
            if a != b and lens[b] <= lens[a] and len(rows) < 40:
                start = int(rng.integers(0, lens[a] - lens[b] + 1))
                rows.append((b, a, len(rows) % 4, lens[b], lens[a], start, len(rows) % 7, 0))
    rows = np.array(rows, dtype=CONTAINED_DTYPE)
    rows = rows[np.lexsort((rows["contained"], rows["j"], rows["super"]))]   # (the order of the files: the model sorts, gfa_check takes it)
    assert {int(r["orient"]) for r in rows} == {0, 1, 2, 3}
    text = [f"{n} {int(mapped)} {layout} {stride} {int(no_seq)} {int(has_nm)}"]
    for i in range(n):
        text.append(seqs[i].decode() + (f" {int(names[i])}" if mapped else ""))
    text.append(str(len(edges)))
    text += [f"{int(e['src'])} {int(e['dst'])} {int(e['orient'])} {int(e['offset'])} {int(subs[x])}" for x, e in enumerate(edges)]
    text.append(str(len(rows)))
    text += [f"{int(r['super'])} {int(r['contained'])} {int(r['orient'])} {int(r['start'])}" for r in rows]
    want = gfa_model.model(None if no_seq else seqs, lens, names, edges, subs if has_nm else None, rows)
    return "\n".join(text) + "\n", want


VARIANTS = [(name, no_seq, has_nm) for name in SETS for no_seq, has_nm in ((False, False), (False, True), (True, False))]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("gfa_cases")
    out = {}
    for v in VARIANTS:
        text, want = _case(*v)
        p = d / ("%s-%d-%d.txt" % v)
        p.write_text(text)
        out[v] = (str(p), want)
    return out


@pytest.mark.parametrize("variant", VARIANTS, ids=["%s-noseq%d-nm%d" % v for v in VARIANTS])
def test_gfa_check_writes_the_models_text(cases, variant):
    build.build_host()
    path, want = cases[variant]
    p = subprocess.run([os.path.join(BIN, "gfa_check"), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.splitlines() == want.splitlines()
    assert p.stdout == want
    S, L, C = gfa_model.parse(p.stdout)
    assert len(S) == len(SETS[variant[0]][0]) and len(L) == 4 * (len(S) - 1) and 4 <= len(C) <= 40
    assert {(so, do) for _, so, _, do, _, _ in L} == {("+", "+"), ("+", "-"), ("-", "+"), ("-", "-")}
    assert {o for _, _, o, _, _ in C} == {"+", "-"}


def test_the_model_places_a_contained_read_as_the_reference_orients_it():
    """BG/OverlapGraph.cpp:428-434 by hand: container ACGTTGCAAC (10), contained of 4 bases"""
    assert gfa_model.c_fields(3, 10, 4, 2) == ("+", 2)   # prefix k-mer hit, same strand: begins at start
    assert gfa_model.c_fields(0, 10, 4, 2) == ("+", 4)   # suffix hit, same strand: ends at len1 - start = 8
    assert gfa_model.c_fields(2, 10, 4, 2) == ("-", 2)
    assert gfa_model.c_fields(1, 10, 4, 2) == ("-", 4)


def test_gfa_check_under_address_and_undefined_sanitizers(cases, tmp_path):
    """the program as it is — its own main, nothing preloaded — built with -fsanitize=address,undefined, once over every case"""
    exe = str(tmp_path / "gfa_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(build.HERE, "host", "gfa_check.cpp")])
    for v in VARIANTS:
        path, want = cases[v]
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, (v, p.stderr.decode()[-3000:])
        assert p.stdout == want, v
