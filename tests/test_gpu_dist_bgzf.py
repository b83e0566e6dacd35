"""-m gpu : BGZF files through the device input stage on every rank (disco_dist_ingest_fasta with DISCO_DIST_BGZF=1: every rank walks the
member chain, the shares are cut over TEXT bytes, and a rank's piece is decoded on its GPU from the members that hold it, the first and
the last one clipped) — per rank exactly what the same text in plain files gives through the same number of ranks, the oracle's graph,
collective declines, and buildG --gpus N end to end. Ranks are threads over the in-process communicator (tests/test_gpu_dist_ingest.py)."""
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import bgzf_util as bz
from tests.test_gpu_dist_ingest import (BIN, JOIN_S, _check_graph, _check_homes, _fasta, _fastq, _graph, _home, _ingest_and_pass, _pool, _ranks, _want)
from tests.test_gpu_ingest import _decode, _wrapped
from tests.util import canon_hip, run_oracle_reads

pytestmark = pytest.mark.gpu
GS = (2, 3)
MO = 33
DI_TAIL = 1 << 21  # bytes of text behind a piece that travel with it (disco_hip.hip)


@pytest.fixture(autouse=True)
def knob(monkeypatch):
    monkeypatch.setenv("DISCO_DIST_BGZF", "1")


def _same_ranks(got, want):
    """per rank: info (shares, counts, home ranges), files[] and the reads held at home"""
    assert len(got) == len(want)
    for r, (a, b) in enumerate(zip(got, want)):
        for k in a["info"]:
            if k not in ("read_s", "device_s"):
                assert a["info"][k] == b["info"][k], (r, k, a["info"][k], b["info"][k])
        assert a["files"] == b["files"], r
        (alo, ahi, areads, afi), (blo, bhi, breads, bfi) = a["home"], b["home"]
        assert (alo, ahi) == (blo, bhi) and areads == breads and np.array_equal(afi, bfi), r


def _check(bgzf_paths, plain_paths, G, graph=True):
    want, wfidx, wtotal, _ = _want(plain_paths, MO)
    plain = _ingest_and_pass(plain_paths, MO, G, graph=False)
    res = _ingest_and_pass(bgzf_paths, MO, G, graph=graph)
    _same_ranks(res, plain)
    infos = _check_homes(res, want, wfidx)
    T = sum(os.path.getsize(p) for p in plain_paths)
    assert [(i["share_lo"], i["share_hi"]) for i in infos] == [(T * r // G, T * (r + 1) // G) for r in range(G)], "shares are cut over text bytes"
    assert infos[0]["total_records"] == wtotal and len(want) > 100
    if graph:
        _check_graph(res, want, wfidx)
    return res


# ---- 1. FASTA in small members ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
def test_fasta_in_small_members_is_the_plain_file(tmp_path, G):
    reads, _ = _pool(71 + G, 300, 100)
    text = _fasta(reads).encode()
    plain, gz = tmp_path / "a.fasta", tmp_path / "a.fasta.gz"
    plain.write_bytes(text)
    gz.write_bytes(bz.bgzf_bytes(text, 700))
    assert sum(text[b - 1] != 10 for b in range(700, len(text), 700)) > 20  # records straddle the members
    res = _check([str(gz)], [str(plain)], G)
    assert res[0]["graph"][2]["e_out"] > 50


# ---- 2. plain and BGZF files in one job ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
def test_a_mixed_job_is_the_all_plain_job(tmp_path, G):
    reads, rng = _pool(81 + G, 420, 120)
    n = len(reads)
    texts = {"q.fastq": _fastq(reads[:n // 3], rng), "p.fasta": _fasta(reads[n // 3:2 * n // 3]),
             "w.fasta": "".join(f">w{i}\n{_wrapped(rng, s, 'w60')}\n" for i, s in enumerate(reads[2 * n // 3:]))}
    plain, mixed = [], []
    for k, (name, t) in enumerate(texts.items()):
        p = tmp_path / name
        p.write_bytes(t.encode())
        plain.append(str(p))
        if name == "p.fasta":
            mixed.append(str(p))
        else:
            z = tmp_path / (name + ".gz")
            z.write_bytes(bz.bgzf_bytes(t.encode(), 4096 if k else 700, eof=bool(k), **bz.SETTINGS[2 if k else 0]))
            mixed.append(str(z))
    _check(mixed, plain, G)


# ---- 3. member edges on share edges ---------------------------------------------------------------------------------------------------------
def _cut_at(text, cuts, between=b""):
    """BGZF of `text` made of whole BGZF files of its parts: a member boundary exactly at every cut (`between`: what stands on it)"""
    at, out = 0, []
    for c in sorted(cuts) + [len(text)]:
        out.append(bz.bgzf_bytes(text[at:c], 4096, eof=False))
        at = c
    return between.join(out)


@pytest.mark.parametrize("G", GS)
def test_member_boundaries_on_share_boundaries(tmp_path, G):
    reads, _ = _pool(91 + G, 300, 100)
    text = _fasta(reads).encode()
    T = len(text)
    plain = tmp_path / "e.fasta"
    plain.write_bytes(text)
    edges = [T * r // G for r in range(1, G)]
    variants = {"on": (0, b""), "before": (-1, b""), "after": (1, b""), "empty_member_on": (0, bz.EOF_MEMBER)}
    paths = {}
    for name, (d, between) in variants.items():
        data = _cut_at(text, [e + d for e in edges], between)
        assert gzip.decompress(data) == text
        p = tmp_path / f"{name}.fasta.gz"
        p.write_bytes(data)
        paths[name] = str(p)
    want, wfidx, wtotal, _ = _want([str(plain)], MO)
    ref = _ingest_and_pass([str(plain)], MO, G, graph=False)

    def work(g, r):  # the same contexts take one file after the other, each with its graph pass: the checks of case 1
        out = {}
        for name, p in paths.items():
            got = g.dist_ingest_fasta([p], threads=2)
            assert got is not None, (name, g.last_error())
            out[name] = {"info": got[0], "files": got[1], "home": _home(g), "mo": MO, "graph": _graph(g)}
            if r == 0:
                packed, lens = g.download_reads()
                out[name]["table"] = _decode(packed, lens)
        return out

    res = _ranks(G, MO, work)
    for name in variants:
        per_rank = [o[name] for o in res]
        _same_ranks(per_rank, ref)
        infos = _check_homes(per_rank, want, wfidx)
        assert [(i["share_lo"], i["share_hi"]) for i in infos] == [(T * r // G, T * (r + 1) // G) for r in range(G)], name
        assert infos[0]["total_records"] == wtotal and len(want) > 100
        _check_graph(per_rank, want, wfidx)


# ---- 4. one member, three windows -----------------------------------------------------------------------------------------------------------
def test_one_member_holds_the_whole_file(tmp_path):
    reads, _ = _pool(101, 200, 60)
    text = _fasta(reads).encode()
    assert len(text) <= 65280
    plain, gz = tmp_path / "one.fasta", tmp_path / "one.fasta.gz"
    plain.write_bytes(text)
    data = bz.bgzf_bytes(text)
    assert len(bz.bgzf_members(text)) == 1  # every rank decodes the same member, each with its own window
    gz.write_bytes(data)
    _check([str(gz)], [str(plain)], 3)


# ---- 5. declines with the knob set ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_member(tmp_path_factory):
    """a FASTA text of 9 MB (450 records of 20 000 bases) as BGZF with the CRC32 of its last member but two flipped: farther than DI_TAIL
    behind every share edge, so only the last rank's piece holds it (and not the member that every rank decodes for the file's last byte)"""
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = b"".join(b">L%d\n" % i + acgt[rng.integers(0, 4, 20000)].tobytes() + b"\n" for i in range(450))
    mem = bz.bgzf_members(text, 65280, level=1)
    k = len(mem) - 3
    m = bytearray(mem[k])
    m[-6] ^= 0x40
    p = tmp_path_factory.mktemp("far") / "far.fasta.gz"
    p.write_bytes(b"".join(mem[:k]) + bytes(m) + b"".join(mem[k + 1:]) + bz.EOF_MEMBER)
    return str(p), len(text), k * 65280


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("what", ["plain_gzip", "bsize_beyond_the_file", "crc_in_the_last_ranks_piece"])
def test_declines_are_collective_and_the_contexts_go_on(tmp_path, G, what, far_member):
    reads, _ = _pool(31, 300, 60)
    text = _fasta(reads).encode()
    ok = tmp_path / "ok.fasta"
    ok.write_bytes(text)
    words = None
    if what == "plain_gzip":
        bad = tmp_path / "plain.fasta.gz"
        bad.write_bytes(gzip.compress(text))
        paths, named, words = [str(ok), str(bad)], str(bad), "gzip input"
    elif what == "bsize_beyond_the_file":
        bad = tmp_path / "short.fasta.gz"
        bad.write_bytes(bz.bgzf_bytes(text, 4096, eof=False)[:-9])
        paths, named, words = [str(bad), str(ok)], str(bad), "gzip input, a member chain that does not hold"
    else:
        named, T, at = far_member
        paths = [named]
        # from the input alone: the pieces of all ranks but the last end in front of the member
        assert all(min(T, T * (r + 1) // G + DI_TAIL) <= at for r in range(G - 1)) and T * (G - 1) // G < at
        words = f"seen by rank {G - 1}"
    want, wfidx, _, _ = _want([str(ok)], MO)

    def work(g, r):
        got = g.dist_ingest_fasta(paths, threads=2)
        msg = g.last_error()
        g.dist_upload_ascii(want)  # the same contexts take the host stage's reads
        return {"got": got, "msg": msg, "graph": _graph(g), "mo": MO}

    res = _ranks(G, MO, work)
    assert all(o["got"] is None for o in res), "every rank gets DISCO_E_UNSUPPORTED"
    assert all(named in o["msg"] and "the host input stage takes this job" in o["msg"] and words in o["msg"] for o in res), [o["msg"] for o in res]
    assert len({o["msg"] for o in res}) == 1
    if what == "crc_in_the_last_ranks_piece":
        assert "BGZF" in res[0]["msg"] and "CRC32" in res[0]["msg"]
    oe, orows, ocnt = run_oracle_reads(want, MO, count_hits=False)
    ce, cc = canon_hip(np.concatenate([o["graph"][0] for o in res]), np.concatenate([o["graph"][1] for o in res]), wfidx)
    oce, occ = canon_hip(oe, orows, wfidx)
    assert np.array_equal(ce, oce) and np.array_equal(cc, occ) and res[0]["graph"][2]["e_out"] == ocnt["e_out"] > 0


# ---- 6. the drop-in -------------------------------------------------------------------------------------------------------------------------
def test_buildg_decodes_a_bgzf_file_on_every_rank(tmp_path):
    from disco_amd import build

    build.build_host()
    reads, _ = _pool(51, 500, 150)
    se, gz = tmp_path / "s.fasta", tmp_path / "s.fasta.gz"
    se.write_text(_fasta(reads))
    gz.write_bytes(bz.bgzf_bytes(se.read_bytes(), 4096))
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {MO}\n")
    G, out = 3, {}
    for how, src in (("plain", se), ("bgzf", gz)):
        prefix = str(tmp_path / how)
        env = dict(os.environ, DISCO_VERBOSE="1", DISCO_DIST_DEVICE_INPUT="1", DISCO_DIST_BGZF="1")
        cmd = [os.path.join(BIN, "buildG"), "-se", str(src), "-f", prefix, "-p", str(cfg), "--gpus", str(G), "--same-device", "-t", "4"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=JOIN_S)
        assert p.returncode == 0, p.stdout[-2000:]
        assert all(f"input stage on rank {r} of {G}" in p.stdout for r in range(G)), p.stdout[-2000:]
        assert "the host input stage takes this job" not in p.stdout, p.stdout[-2000:]
        assert ("member chains walked" in p.stdout) == (how == "bgzf")
        # (the LINES of an edge file as a sorted list: their order inside a file follows the emission's atomics in any two runs)
        out[how] = {os.path.basename(f)[len(how):]: sorted(open(f, "rb").read().splitlines()) if f.endswith("parGraph.txt") else open(f, "rb").read()
                    for f in sorted(glob.glob(prefix + "_*"))}
        # (_ReadIDMap.txt names the input files: the BGZF file's name read as the plain one's)
        out[how]["_ReadIDMap.txt"] = out[how]["_ReadIDMap.txt"].replace(os.fsencode(str(gz)), os.fsencode(str(se)))
    assert out["bgzf"].keys() == out["plain"].keys() and len(out["plain"]) >= 4
    for k in out["plain"]:
        assert out["bgzf"][k] == out["plain"][k], k
    assert out["plain"]["_ReadIDMap.txt"].count(b"\n") >= 1
