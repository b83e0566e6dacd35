"""The states, rounds and lines behind <prefix>.unitigs.reads (disco_amd/csrc/disco_unitig_reads.h) without a GPU:
disco_amd/bin/unitig_reads_check builds the header the kernels include as plain C++ and runs a described case the way
disco_write_unitig_reads does — initial states, rounds of doubling, the links' places, the counts and their scan, every section piece
by piece; the text must be tests/unitig_reads_model.py's, which walks hop by hop. The nest set (70 reads inside each other: seven
rounds) comes from the oracle's rows and the chain model; the forests are described by hand. Once more under AddressSanitizer and
UBSan: the program as it is, its own main, nothing preloaded."""
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build
from disco_amd.buildgraph import CHAIN_EDGE_DTYPE, CHAIN_LINK_DTYPE, CONTAINED_DTYPE
from oracle import pyoracle
from tests import chain_model
from tests import gfa_chains_model as gcm
from tests import unitig_reads_model as urm

BIN = os.path.join(build.HERE, "bin")
_COMP = str.maketrans("ACGT", "TGCA")
PIECES = [1, 7, 64, 0]   # lines per piece; 0: every section in one


def _rc(s):
    return s.translate(_COMP)[::-1]


def nest_reads():
    """70 reads around one place of a genome, each one base longer than the one before it and inside it, every third one on the other
    strand; then tiles of 100 bases every 40 over the genome, every fourth one on the other strand"""
    G = "".join(np.random.default_rng(7).choice(list("ACGT"), 3000))
    reads = []
    for i in range(70):
        s = G[1000 - (i + 1) // 2:1060 + i // 2]
        reads.append(_rc(s) if i % 3 == 0 else s)
    for a in range(0, 2900, 40):
        s = G[a:a + 100]
        reads.append(_rc(s) if (a // 40) % 4 == 1 else s)
    return reads


def _nest():
    reads = nest_reads()
    codes, off = pyoracle.encode_reads(reads)
    rows, edges, cnt = pyoracle.build_graph(codes, off, 40)
    lens = [len(r) for r in reads]
    cm = chain_model.chain_model(edges, lens, 0)
    assert cnt["cap_bind_sites"] == 0 and cnt["asymmetric_pairs"] == 0
    return {"seqs": [r.encode() for r in reads], "lens": lens, "rows": rows, "edges": edges, "absorbed": cm.absorbed, "comp": cm.comp, "links": cm.links,
            "rings": cm.rings, "names": np.arange(1, len(reads) + 1, dtype=np.uint64)}


def _forest():
    """described by hand: two chains — c0 with six interior reads on both strands, c1 with one, reversed — their four ends, an isolated
    read, and under five roots (an interior read of either strand of c0, the one of c1, a chain end, the isolated read) a tree three
    hops deep in which every read has a contained read of every orientation: all sixteen pairs at either pair of hops. Reads under a
    read are cut from it, the interior reads from one genome, so that the files can be checked against the bases too"""
    rng = np.random.default_rng(20)
    rnd = lambda n: "".join(rng.choice(list("ACGT"), n))   # noqa: E731
    G = rnd(600)
    seqs = [rnd(100), rnd(100), rnd(90), rnd(95), rnd(77)]   # 0, 1: ends of c0; 2, 3: ends of c1; 4: isolated
    comp, links = [], []

    def chain(a, b, inner, g0):
        """inner: (start in the segment, length, forward); the segment is G[g0:]"""
        first, prev, at = len(links), a, 0
        for j, (s, L, fwd) in enumerate(inner):
            piece = G[g0 + s:g0 + s + L]
            seqs.append(piece if fwd else _rc(piece))
            off = (s - at) if j else 17
            assert off < len(seqs[prev])
            links.append((len(seqs) - 1, off, (2 if j % 3 else 0) | int(fwd)))
            prev, at = len(seqs) - 1, s
        links.append((b, 33, 1))
        comp.append((a, b, sum(l[1] for l in links[first:]), (links[first][2] & 2) | 1, len(inner) + 1, first))

    chain(0, 1, [(0, 100, True), (30, 110, False), (60, 105, False), (95, 120, True), (140, 101, True), (170, 99, False)], 0)
    chain(2, 3, [(0, 88, False)], 400)
    roots = [5, 6, 11, 1, 4]   # c0's first interior read (forward), its second (reversed), c1's (reversed), an end of c0, the isolated read
    rows, level = [], roots
    for child_len in (64, 50, 41):
        nxt = []
        for y in level:
            for orient in range(4):
                Ly = len(seqs[y])
                p = int(rng.integers(0, Ly - child_len + 1))
                oriented = seqs[y][p:p + child_len]
                seqs.append(oriented if orient in (0, 3) else _rc(oriented))
                start = p if orient in (3, 2) else Ly - p - child_len
                rows.append((len(seqs) - 1, y, orient, child_len, Ly, start, 0, 0))
                nxt.append(len(seqs) - 1)
        level = nxt
    n = len(seqs)
    order = rng.permutation(n)   # ids in no order of depth: a container may have the larger id
    new_of = np.empty(n, dtype=np.int64)
    new_of[order] = np.arange(n)
    seqs = [seqs[int(i)] for i in order]
    rows = np.array(sorted((int(new_of[c]), int(new_of[y]), o, l2, l1, st, 0, 0) for c, y, o, l2, l1, st, _, _ in rows), dtype=CONTAINED_DTYPE)
    links = np.array([(int(new_of[t]), off, o) for t, off, o in links], dtype=CHAIN_LINK_DTYPE)
    comp = np.array([(int(new_of[a]), int(new_of[b]), off, o, nl, f) for a, b, off, o, nl, f in comp], dtype=CHAIN_EDGE_DTYPE)
    return {"seqs": [s.encode() for s in seqs], "lens": [len(s) for s in seqs], "rows": rows, "comp": comp, "links": links,
            "names": np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(10_000_000_019), "roots": [int(new_of[r]) for r in roots]}


SETS = {"nest": _nest, "forest": _forest}


def _case_text(s, mapped, depth_only, piece, rows=None):
    rows = s["rows"] if rows is None else rows
    by_read = {int(r["contained"]): r for r in rows}
    text = [f"{len(s['lens'])} {int(mapped)} {int(depth_only)} {piece}"]
    for i, L in enumerate(s["lens"]):
        r = by_read.get(i)
        text.append(f"{L}" + (f" {int(s['names'][i])}" if mapped else "") + (f" 1 {int(r['super'])} {int(r['orient'])} {int(r['start'])}" if r is not None else " 0 0 0 0"))
    text.append(str(len(s["comp"])))
    for c in s["comp"]:
        text.append(f"{int(c['a'])} {int(c['b'])} {int(c['n_links'])}")
        text += [f"{int(l['to'])} {int(l['offset'])} {int(l['orient'])}" for l in s["links"][int(c["first_link"]):int(c["first_link"]) + int(c["n_links"])]]
    return "\n".join(text) + "\n"


VARIANTS = [(name, False, p) for name in SETS for p in PIECES] + [(name, True, p) for name in SETS for p in (7, 0)]


@pytest.fixture(scope="module")
def sets():
    return {name: make() for name, make in SETS.items()}


@pytest.fixture(scope="module")
def cases(sets, tmp_path_factory):
    d = tmp_path_factory.mktemp("unitig_reads_cases")
    out = {}
    for v in VARIANTS:
        name, depth_only, piece = v
        s = sets[name]
        mapped = name == "forest"
        names = s["names"] if mapped else np.arange(1, len(s["lens"]) + 1)
        p = d / ("%s-%d-%d.txt" % v)
        p.write_text(_case_text(s, mapped, depth_only, piece))
        out[v] = (str(p), urm.model(s["lens"], names, s["rows"], s["comp"], s["links"], depth_only))
    return out


def _run(exe, path):
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout, p.stderr.decode()


def test_the_nest_is_what_the_cpu_run_gave(sets):
    s = sets["nest"]
    assert len(s["lens"]) == 143 and len(s["rows"]) == 69 and len(s["edges"]) == 73
    assert len(s["comp"]) == 1 and int(s["comp"][0]["n_links"]) == 73 and not s["rings"] and int((s["absorbed"] == 0).sum()) == 0
    place = urm.placements(s["lens"], s["rows"], s["comp"], s["links"])
    seg, plus, start, root, hops = place[0]
    assert (hops, root) == (69, 69)
    r, pos, same, _ = urm.root_of(0, s["lens"], urm.direct(s["rows"]))
    assert (r, pos, same) == (69, 34, True)                                         # at base 34 of its root, on the root's strand
    assert sum(p[0] == ("c", 0) for p in place) == 141
    assert sorted(p[0] for p in place if p[0][0] == "r") == [("r", int(s["comp"][0]["a"])), ("r", int(s["comp"][0]["b"]))]
    assert max(p[4] for p in place) == 69 > 64                                      # deeper than a wavefront is wide


def test_the_forest_covers_what_it_is_there_for(sets):
    s = sets["forest"]
    step = urm.direct(s["rows"])
    on_chain = urm.chain_places(s["comp"], s["links"])
    pairs = {1: set(), 2: set()}
    by_read = {int(r["contained"]): int(r["orient"]) for r in s["rows"]}
    for x in by_read:
        y = step[x][0]
        if y in by_read:
            z = step[y][0]
            pairs[2 if z in by_read else 1].add((by_read[x], by_read[y]))
    assert pairs[1] == pairs[2] == {(a, b) for a in range(4) for b in range(4)}   # every orientation pair at either pair of hops
    roots = {urm.root_of(x, s["lens"], step)[0] for x in by_read}
    assert roots == set(s["roots"])
    assert sorted(on_chain[r][2] for r in roots if r in on_chain) == [False, False, True] and sum(r not in on_chain for r in roots) == 2
    assert {on_chain[r][0] for r in roots if r in on_chain} == {0, 1}
    assert any(step[x][0] > x for x in step) and any(step[x][0] < x for x in step)
    assert all(len(str(int(v))) == 11 for v in s["names"])
    place = urm.placements(s["lens"], s["rows"], s["comp"], s["links"])
    assert max(p[4] for p in place) == 3 and {p[1] for p in place if p[0][0] == "c"} == {True, False}


@pytest.mark.parametrize("variant", VARIANTS, ids=["%s-depth%d-piece%d" % v for v in VARIANTS])
def test_unitig_reads_check_writes_the_models_text(sets, cases, variant):
    build.build_host()
    path, want = cases[variant]
    rc, out, err = _run(os.path.join(BIN, "unitig_reads_check"), path)
    assert rc == 0, err
    assert out.splitlines() == want.splitlines()
    assert out == want
    name, depth_only, _ = variant
    s = sets[name]
    assert err.strip() == "rounds %d" % (7 if name == "nest" else 2)              # 69 hops: 2^6 < 69 <= 2^7; 3 hops: two rounds
    U, R = urm.parse(out)
    n_inside = int(gcm.interior(s["comp"], s["links"]).sum())
    assert len(U) == len(s["lens"]) - len(s["rows"]) - n_inside + len(s["comp"])
    assert len(R) == (0 if depth_only else len(s["lens"]))


@pytest.mark.parametrize("name", list(SETS))
def test_the_text_holds_against_the_bases(sets, cases, name):
    """the model's text, which the program's equals, against <prefix>.unitigs.gfa as its model writes it and the reads themselves"""
    s = sets[name]
    mapped = name == "forest"
    names = s["names"] if mapped else np.arange(1, len(s["lens"]) + 1)
    contained = np.zeros(len(s["lens"]), dtype=np.uint8)
    contained[s["rows"]["contained"].astype(np.int64)] = 1
    gfa = gcm.model(s["seqs"], s["lens"], names, contained, np.zeros(0, dtype=pyoracle.EDGE_DTYPE), [], s["comp"], s["links"])
    full, depth = cases[(name, False, 0)][1], cases[(name, True, 0)][1]
    n_u, n_r, on_chains, minus, hops = urm.semantic_check(full, gfa, s["seqs"], names)
    assert n_r == len(s["lens"]) and urm.depth_only_is_prefix(depth, full) == n_u
    if name == "nest":
        assert (n_u, on_chains) == (3, 141) and hops == [74] + [1] * 69
    else:
        assert hops == [len(s["lens"]) - len(s["rows"]), 20, 80, 320] and 0 < minus < n_r


@pytest.mark.parametrize("how", ["no-read", "cycle-of-two", "cycle-of-three"])
def test_rows_that_cannot_be_placed_are_refused_with_a_message(sets, tmp_path, how):
    build.build_host()
    s = sets["forest"]
    rows = s["rows"].copy()
    free = [i for i in range(len(s["lens"])) if i not in set(rows["contained"].astype(int).tolist())]
    if how == "no-read":
        rows["super"][5] = len(s["lens"])
        want = "1 contained reads have a key that names no containing read"
    else:
        ring = free[:2] if how == "cycle-of-two" else free[:3]   # reads that were roots, now each inside the next
        extra = np.array([(x, ring[(i + 1) % len(ring)], 3, s["lens"][x], s["lens"][ring[(i + 1) % len(ring)]], 0, 0, 0) for i, x in enumerate(ring)], dtype=CONTAINED_DTYPE)
        rows = np.concatenate([rows, extra])
        want = "do not settle in 17 rounds of doubling: they hold a cycle"
        with pytest.raises(ValueError, match="cycle"):
            urm.model(s["lens"], s["names"], rows, s["comp"], s["links"])
    p = tmp_path / "bad.txt"
    p.write_text(_case_text(s, True, False, 0, rows))
    rc, out, err = _run(os.path.join(BIN, "unitig_reads_check"), str(p))
    assert rc == 1 and out == b"" and want in err, err


def test_unitig_reads_check_under_address_and_undefined_sanitizers(cases, tmp_path):
    """the program as it is — its own main, nothing preloaded — built with -fsanitize=address,undefined, once over every case"""
    exe = str(tmp_path / "unitig_reads_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(build.HERE, "host", "unitig_reads_check.cpp")])
    for v in VARIANTS:
        path, want = cases[v]
        rc, out, err = _run(exe, path)
        assert rc == 0, (v, err[-3000:])
        assert out == want, v


def test_the_model_composes_two_hops_by_hand():
    """z = ACGTACGTAA; y = its bases [2, 9) reversed (orient 1: start = len1 - p - len2 = 1); x = bases [1, 4) of oriented... of y as stored,
    forward (orient 3: start = p = 1). y stored = rc(GTACGTA) = TACGTAC, x = ACG. In z: y is minus at 2, so x lies at 2 + 7 - 1 - 3 = 5 on
    the other strand: z[5:8] = CGT = rc(ACG)"""
    z, y, x = b"ACGTACGTAA", b"TACGTAC", b"ACG"
    rows = np.array([(1, 0, 1, 7, 10, 1, 0, 0), (2, 1, 3, 3, 7, 1, 0, 0)], dtype=CONTAINED_DTYPE)
    none_c, none_l = np.zeros(0, dtype=CHAIN_EDGE_DTYPE), np.zeros(0, dtype=CHAIN_LINK_DTYPE)
    text = urm.model([10, 7, 3], [1, 2, 3], rows, none_c, none_l)
    assert text == b"H\tunitig-reads\t1\nU\t1\t10\t3\t20\nR\t1\t1\t+\t0\t10\t1\t0\nR\t2\t1\t-\t2\t7\t1\t1\nR\t3\t1\t-\t5\t3\t1\t2\n"
    assert z[2:9] == gcm.oriented(y, False) and z[5:8] == gcm.oriented(x, False)
