"""The item functions behind <prefix>.unitigs.gfa (disco_amd/csrc/disco_gfa_chains.h) without a GPU: disco_amd/bin/gfa_chains_check
builds the header the kernels include as plain C++ and writes a described case the way disco_write_gfa_chains does — the chain S section
item by item, piece by piece, over the three layouts of the read table; the text must be tests/gfa_chains_model.py's. Once more under
AddressSanitizer and UBSan: every store of every item inside the piece it was given."""
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build
from disco_amd.buildgraph import CHAIN_EDGE_DTYPE, CHAIN_LINK_DTYPE, EDGE_DTYPE
from tests import gfa_chains_model as gcm

BIN = os.path.join(build.HERE, "bin")
LENGTHS = [31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
OFFSETS = [1, 31, 32, 33, 64, 65, 300]
# name: (interior lengths of the long chain, layout, stride words, 11-digit file indices)
SETS = {
    "five-word-rows": ([L for L in LENGTHS if L <= 160], 0, 5, True),
    "two-classes": (LENGTHS, 1, 32, True),
    "one-wide-stride": (LENGTHS, 0, 32, False),
}
PIECES = [1, 7, 64, 0]   # 0: the chain S section in one piece


def _graph(name):
    """reads, contained flags, edges with their absorbed flags, composite edges and links — described by hand, not made by a pass: the
    rule says who is read where, so the reads need not agree where they overlap and every base is told apart from its neighbours'"""
    interior_lens, layout, stride, mapped = SETS[name]
    rng = np.random.default_rng(len(name) * 11 + stride)
    lens = [100, 100, 90, 77, 50]            # reads 0..4: chain ends (0, 1), a read with edges only (2), a contained read (3), the end of a loop (4)
    comp, links = [], []

    def chain(a, b, inner, orient_of, offset_of):
        first = len(links)
        prev = a
        for j, L in enumerate(inner + [None]):
            off = min(offset_of(j), lens[prev] - 1)
            if L is None:
                links.append((b, off, orient_of(j)))
            else:
                lens.append(L)
                links.append((len(lens) - 1, off, orient_of(j)))
                prev = len(lens) - 1
        comp.append((a, b, sum(l[1] for l in links[first:]), (links[first][2] & 2) | (links[-1][2] & 1), len(inner) + 1, first))

    # every length on both strands; the offset INTO a read cycles through OFFSETS (cut to the read before it), 300 comes behind a read of 1000
    both = [L for L in interior_lens for _ in (0, 1)]
    chain(0, 1, both, lambda j: (j % 2) | (2 if j % 3 else 0), lambda j: OFFSETS[(j + 2) % len(OFFSETS)] if j else 60)
    chain(4, 4, [interior_lens[-1]], lambda j: 3 - j, lambda j: 20 + j)           # one interior read, a == b
    chain(0, 1, [40, 41], lambda j: 1 + 2 * (j % 2), lambda j: 7)                 # a second chain between the same ends
    n = len(lens)
    comp = np.array(comp, dtype=CHAIN_EDGE_DTYPE)
    links = np.array(links, dtype=CHAIN_LINK_DTYPE)
    seqs = ["".join(rng.choice(list("ACGT"), L)).encode() for L in lens]
    names = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(9_999_999_993) if mapped else np.arange(1, n + 1, dtype=np.uint64)
    contained = np.zeros(n, dtype=np.uint8)
    contained[3] = 1
    edges = np.zeros(8, dtype=EDGE_DTYPE)    # every orientation, absorbed or not
    for x in range(len(edges)):
        s, d = (2, x % 2) if x < 4 else (x % 2, 4)
        edges[x] = (s, d, x % 4, int(rng.integers(0, lens[s])), lens[s], lens[d])
    absorbed = (np.arange(len(edges)) % 3 == 1).astype(np.uint8)
    return seqs, lens, names, contained, edges, absorbed, comp, links


def _case(name, no_seq, piece):
    seqs, lens, names, contained, edges, absorbed, comp, links = _graph(name)
    _, layout, stride, mapped = SETS[name]
    skip = contained.astype(bool).copy()
    skip[links["to"][gcm.interior(comp, links)].astype(int)] = True
    text = [f"{len(lens)} {int(mapped)} {layout} {stride} {int(no_seq)} {piece}"]
    for i in range(len(lens)):
        text.append(seqs[i].decode() + (f" {int(names[i])}" if mapped else "") + f" {int(skip[i])}")
    text.append(str(len(comp)))
    for c in comp:
        text.append(f"{int(c['a'])} {int(c['b'])} {int(c['n_links'])}")
        text += [f"{int(l['to'])} {int(l['offset'])} {int(l['orient'])}" for l in links[int(c["first_link"]):int(c["first_link"]) + int(c["n_links"])]]
    kept = edges[absorbed == 0]
    text.append(str(len(kept)))
    text += [f"{int(e['src'])} {int(e['dst'])} {int(e['orient'])} {int(e['offset'])}" for e in kept]
    want = gcm.model(None if no_seq else seqs, lens, names, contained, edges, absorbed, comp, links)
    return "\n".join(text) + "\n", want


VARIANTS = [(name, no_seq, piece) for name in SETS for no_seq, piece in [(False, p) for p in PIECES] + [(True, 7), (True, 0)]]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("gfa_chains_cases")
    out = {}
    for v in VARIANTS:
        text, want = _case(*v)
        p = d / ("%s-%d-%d.txt" % v)
        p.write_text(text)
        out[v] = (str(p), want)
    return out


def test_the_cases_cover_what_they_are_there_for():
    for name, (interior_lens, _, _, _) in SETS.items():
        _, lens, _, contained, _, absorbed, comp, links = _graph(name)
        c = comp[0]
        ls = links[int(c["first_link"]):int(c["first_link"]) + int(c["n_links"])]
        inner = ls[:-1]
        assert {(int(lens[int(l["to"])]), int(l["orient"]) & 1) for l in inner} == {(L, s) for L in interior_lens for s in (0, 1)}
        want_offsets = {o for o in OFFSETS if o < max(interior_lens)}
        assert want_offsets <= {int(l["offset"]) for l in ls[1:]}, name
        assert int(comp[1]["n_links"]) == 2 and comp[1]["a"] == comp[1]["b"] and (comp[2]["a"], comp[2]["b"]) == (c["a"], c["b"])
        assert contained.sum() == 1 and 0 < absorbed.sum() < len(absorbed)
    assert set(LENGTHS) == set(SETS["two-classes"][0]) == set(SETS["one-wide-stride"][0]) and set(OFFSETS) <= {1, 31, 32, 33, 64, 65, 300}


@pytest.mark.parametrize("variant", VARIANTS, ids=["%s-noseq%d-piece%d" % v for v in VARIANTS])
def test_gfa_chains_check_writes_the_models_text(cases, variant):
    build.build_host()
    path, want = cases[variant]
    p = subprocess.run([os.path.join(BIN, "gfa_chains_check"), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.splitlines() == want.splitlines()
    assert p.stdout == want
    S, L = gcm.parse(p.stdout)
    names = [k for k in S if not k.startswith(b"c")]
    assert len(names) == 4 and [k for k in S if k.startswith(b"c")] == [b"c0", b"c1", b"c2"] and len(L) == 5 + 6
    assert any(len(k) == 11 for k in names) == SETS[variant[0]][3]
    assert S[b"c1"][2] == 1 and S[b"c0"][2] == 2 * len(SETS[variant[0]][0])
    assert {(so, do) for _, so, _, do, _ in L} == {("+", "+"), ("+", "-"), ("-", "+"), ("-", "-")}


def test_gfa_chains_check_under_address_and_undefined_sanitizers(cases, tmp_path):
    """the program as it is — its own main, nothing preloaded — built with -fsanitize=address,undefined, once over every case"""
    exe = str(tmp_path / "gfa_chains_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(build.HERE, "host", "gfa_chains_check.cpp")])
    for v in VARIANTS:
        path, want = cases[v]
        p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, (v, p.stderr.decode()[-3000:])
        assert p.stdout == want, v


def test_the_model_lays_every_read_over_the_one_before_it():
    """by hand: ACGTACGT, then TTTT read backwards (AAAA) from base 3, then GG from base 5 — the last read ends the segment"""
    links = np.array([(1, 2, 3), (2, 3, 0), (3, 2, 1), (4, 1, 1)], dtype=CHAIN_LINK_DTYPE)
    comp = np.array([(0, 4, 8, 3, 4, 0)], dtype=CHAIN_EDGE_DTYPE)
    seqs = [b"CCCCC", b"ACGTACGT", b"TTTT", b"GG", b"CCCCC"]
    seg, ln, m = gcm.chain_segment(seqs, [len(s) for s in seqs], comp[0], links)
    assert (seg, ln, m) == (b"ACGAAGG", 7, 3)
    text = gcm.model(seqs, [len(s) for s in seqs], [1, 2, 3, 4, 5], [0] * 5, np.zeros(0, dtype=EDGE_DTYPE), [], comp, links)
    assert text == b"H\tVN:Z:1.0\nS\t1\tCCCCC\tLN:i:5\nS\t5\tCCCCC\tLN:i:5\nS\tc0\tACGAAGG\tLN:i:7\tRC:i:3\nL\t1\t+\tc0\t+\t3M\nL\tc0\t+\t5\t+\t1M\n"
