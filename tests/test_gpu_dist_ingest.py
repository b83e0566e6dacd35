"""-m gpu : the device input stage on every rank of a multi-GPU job (disco_dist_ingest_fasta: every rank reads its share of the bytes of
the files laid end to end, finds / cleans / filters / packs the records that START there, and sends what belongs to other ranks' home
ranges to its owners) against the CPU restatement of the reference's parser (oracle/pyoracle.load_good_reads) and the oracle's graph.
Ranks are threads of this process over the in-process communicator, G in {2, 3, 5}; a rank thread that does not come back within
JOIN_S seconds is a failure (a collective somebody never entered), not a wait."""
import glob
import gzip
import os
import subprocess
import threading

import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from oracle import pyoracle
from tests.ingest_edges import EDGE_DECLINED, edge_files, edge_want
from tests.test_gpu_ingest import _adversarial, _decode, _wrapped
from tests.util import canon_hip, run_oracle_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disco_amd", "bin")
JOIN_S = 120
GS = (2, 3, 5)


def _ranks(G, min_overlap, work):
    """work(g, r) on G rank threads over contexts that share one in-process communicator; returns the ranks' results"""
    gs = [buildgraph.BuildGraph(min_overlap=min_overlap) for _ in range(G)]
    buildgraph.BuildGraph.comm_init_local(gs)
    out, errors = [None] * G, []

    def run(r):
        try:
            out[r] = work(gs[r], r)
        except Exception as e:  # pragma: no cover
            errors.append((r, repr(e)))

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=JOIN_S)
    stuck = [r for r, t in enumerate(th) if t.is_alive()]
    assert not stuck, f"ranks {stuck} are still inside a call: a collective somebody did not enter"
    try:
        assert not errors, errors
        return out
    finally:
        for g in gs:
            g.close()


def _home(g):
    """what the stage left in the rank's home range: (lo, hi, reads, lengths, file indices)"""
    ln, fi = g.dist_ingest_fetch()
    lo, hi = g.dist_range(g.num_reads)
    packed, lens = g.download_reads()
    assert np.array_equal(lens[lo:hi], ln)
    return lo, hi, _decode(packed[lo:hi], ln), fi


def _graph(g):
    g.dist_run_graph(True, False)
    return g.fetch_edges(), g.fetch_contained(), g.dist_info()


def _want(paths, mo):
    want, wfidx, wtotal = pyoracle.load_good_reads(paths, mo)
    keep = [i for i, s in enumerate(want) if len(s) <= 32767]
    return [want[i] for i in keep], np.asarray(wfidx, dtype=np.int64)[keep], wtotal, len(want) - len(keep)


def _check_homes(res, want, wfidx):
    """every rank's home range is the parser's slice; the ranges tile the job"""
    at = 0
    for r, o in enumerate(res):
        lo, hi, reads, fi = o["home"]
        assert lo == min(at, len(want)) or lo == hi, (r, lo, hi)
        assert reads == want[lo:hi], f"rank {r}: rows of the home range differ from the parser's"
        assert np.array_equal(fi.astype(np.int64), wfidx[lo:hi]), f"rank {r}: file indices"
        at = hi
    assert at == len(want)
    infos = [o["info"] for o in res]
    for k in ("n_reads", "total_records", "too_long", "stride_words", "shortest", "longest"):
        assert len({i[k] for i in infos}) == 1, k
    assert all(o["files"] == res[0]["files"] for o in res)
    assert sum(i["share_reads"] for i in infos) == len(want) == infos[0]["n_reads"]
    return infos


def _check_graph(res, want, wfidx):
    oe, orows, ocnt = run_oracle_reads(want, res[0]["mo"], count_hits=False)
    edges = np.concatenate([o["graph"][0] for o in res])
    rows = np.concatenate([o["graph"][1] for o in res])
    info = res[0]["graph"][2]
    ce, cc = canon_hip(edges, rows, wfidx)
    oce, occ = canon_hip(oe, orows, wfidx)
    assert np.array_equal(ce, oce) and np.array_equal(cc, occ)
    for k in ("e_pre", "e_out", "n_contained"):
        assert info[k] == ocnt[k], k
    assert res[0]["table"] == want, "rank 0's table after the pass differs from the parser's reads"


def _ingest_and_pass(paths, mo, G, graph=True):
    def work(g, r):
        got = g.dist_ingest_fasta(paths, threads=2)
        assert got is not None, g.last_error()
        o = {"info": got[0], "files": got[1], "home": _home(g), "mo": mo, "long_rows_before": g.long_rows}
        if graph:
            o["graph"] = _graph(g)
            o["long_rows"] = g.long_rows
            if r == 0:
                packed, lens = g.download_reads()
                o["table"] = _decode(packed, lens)
        return o

    return _ranks(G, mo, work)


def _pool(seed, n_genome, n_adv, read_len=100, len_max=180):
    """overlapping reads of one genome (edges, contained reads) shuffled among adversarial ones around every filter threshold"""
    rng = np.random.default_rng(seed)
    reads = list(readgen.generate_reads(readgen.GenSpec.coverage(seed=seed, n_reads=n_genome, read_len=read_len, cov=12.0, len_max=len_max)))
    reads += [s for s in _adversarial(rng, n_adv) if len(s) < 1000]
    return [reads[i] for i in rng.permutation(len(reads))], rng


def _fasta(reads, eol="\n", final_newline=True, tag="r"):
    text = "".join(f">{tag}{i} some description{eol}{s}{eol}" for i, s in enumerate(reads))
    return text if final_newline else text[:-len(eol)]


def _fastq(reads, rng, tail="full"):
    recs = []
    for i, s in enumerate(reads):
        q = "".join(rng.choice(list("@>IF#+"), len(s)))
        q = ("@" if i % 2 == 0 else ">") + q[1:]
        recs.append(f"@r{i} x\n{s}\n+\n{q}\n")
    text = "".join(recs)
    if tail == "no_final_newline":
        text = text[:-1]
    elif tail == "header_only":
        text += "@last"
    elif tail == "three_lines":
        text += "@last\n" + "ACGT" * 20 + "\n+"
    return text


# ---- 1. parity with the parser ----------------------------------------------------------------------------------------------------------
PARITY = [("fasta", "\n", True), ("fasta", "\n", False), ("fasta", "\r\n", True), ("fasta", "\r\n", False), ("fastq", "full", None), ("fastq", "no_final_newline", None),
          ("fastq", "header_only", None), ("fastq", "three_lines", None), ("wrapped", True, None), ("wrapped", False, None)]


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("kind,a,b", PARITY)
def test_every_rank_keeps_what_the_parser_keeps(tmp_path, G, kind, a, b):
    reads, rng = _pool(11 + G, 260, 140)
    if kind == "fasta":
        text = _fasta(reads, a, b)
    elif kind == "fastq":
        text = _fastq(reads, rng, a)
    else:
        hows = ["w60", "w70", "w7", "w1", "irregular", "blank", "trail", "one", "w150", "w29"]
        text = "".join(f">r{i} d\n{_wrapped(rng, s, hows[i % len(hows)])}\n" for i, s in enumerate(reads))
        text = text if a else text.rstrip("\n")
    p = tmp_path / ("in." + ("fastq" if kind == "fastq" else "fasta"))
    p.write_bytes(text.encode())
    mo = 33
    want, wfidx, wtotal, n_long = _want([str(p)], mo)
    if want == []:  # "\r\n" with a final newline: a CR is not ACGT, no good read — the job is the host stage's (for its message), on every rank
        assert kind == "fasta" and a == "\r\n" and b

        def declined(g, r):
            return g.dist_ingest_fasta([str(p)]), g.last_error()

        res = _ranks(G, mo, declined)
        assert want == [] and all(o[0] is None and "no good read" in o[1] for o in res), res
        return
    res = _ingest_and_pass([str(p)], mo, G)
    infos = _check_homes(res, want, wfidx)
    assert infos[0]["total_records"] == wtotal and infos[0]["too_long"] == n_long
    assert res[0]["files"][0]["good"] == len(want) and res[0]["files"][0]["good"] + res[0]["files"][0]["bad"] == wtotal
    _check_graph(res, want, wfidx)
    if a == "\r\n":  # without a final newline the last record has no CR behind it: the one read the parser keeps
        assert len(want) == 1
    else:
        assert len(want) > 200 and res[0]["graph"][2]["e_out"] > 50


# ---- 2. cuts --------------------------------------------------------------------------------------------------------------------------
def _where(text, fastq, pos):
    """what byte `pos` of the text is: the kinds of cut the issue names"""
    lines, at = [], 0
    for ln in text.split("\n"):
        lines.append((at, at + len(ln)))  # [start, newline position)
        at += len(ln) + 1
    rec_lines = [i for i in range(len(lines)) if (i % 4 == 0 if fastq else text[lines[i][0]:lines[i][0] + 1] == ">") and lines[i][0] < len(text)]
    starts = {lines[i][0] for i in rec_lines}
    if pos in starts:
        return "first_byte"
    if pos + 1 in starts:
        return "newline_in_front"
    for i, (s, e) in enumerate(lines):
        if s < pos < e:
            if i in rec_lines:
                return "header"
            if fastq:
                return {1: "sequence", 3: "quality_at" if text[s] == "@" else "quality"}.get(i % 4, "plus")
            return "sequence"
    return "other"


def _cut_input(G, fastq, kind, seed):
    """records whose first header is padded until some share boundary of G ranks falls on a byte of the given kind"""
    reads, rng = _pool(seed, 90, 40)
    body = _fastq(reads, rng) if fastq else _fasta(reads)
    for pad in range(400):
        text = ("@" if fastq else ">") + "p" * pad + body[1:]
        T = len(text)
        if any(_where(text, fastq, T * r // G) == kind for r in range(1, G)):
            return text
    raise AssertionError(f"no padding puts a boundary of {G} shares on {kind}")


CUTS = [(True, k) for k in ("header", "sequence", "quality_at", "first_byte", "newline_in_front")] + [(False, k) for k in ("header", "sequence", "first_byte", "newline_in_front")]


@pytest.mark.parametrize("G", GS)
def test_share_boundaries_inside_lines_and_on_record_starts(tmp_path, G):
    mo, paths, wants = 33, [], []
    for n, (fastq, kind) in enumerate(CUTS):
        text = _cut_input(G, fastq, kind, 100 + n)
        # from the input alone, before anything runs on the GPU: some boundary of the G shares is of this kind
        assert kind in {_where(text, fastq, len(text) * r // G) for r in range(1, G)}
        p = tmp_path / f"cut{n}.{'fastq' if fastq else 'fasta'}"
        p.write_text(text)
        paths.append(str(p))
        wants.append(_want([str(p)], mo))

    def work(g, r):  # the same contexts take one input after the other
        out = []
        for p in paths:
            got = g.dist_ingest_fasta([p], threads=2)
            assert got is not None, g.last_error()
            out.append({"info": got[0], "files": got[1], "home": _home(g)})
        return out

    res = _ranks(G, mo, work)
    for n, (want, wfidx, wtotal, _) in enumerate(wants):
        infos = _check_homes([o[n] for o in res], want, wfidx)
        assert infos[0]["total_records"] == wtotal and len(want) > 60, CUTS[n]


# ---- 3. several files -------------------------------------------------------------------------------------------------------------------
def test_shares_across_files_of_very_different_sizes(tmp_path):
    reads, rng = _pool(5, 700, 200)
    big = tmp_path / "big.fasta"           # ~100 KB
    big.write_text(_fasta(reads[:600]))
    mid = tmp_path / "mid.fastq"           # ~10 KB
    mid.write_text(_fastq(reads[600:640], rng))
    tiny = tmp_path / "tiny.fasta"         # two records: most of five ranks' pieces of it are empty
    tiny.write_text(_fasta(reads[640:642], tag="t"))
    small = tmp_path / "small_wrapped.fasta"  # ~1 KB, wrapped
    small.write_text("".join(f">w{i}\n{_wrapped(rng, s, 'w60')}\n" for i, s in enumerate(reads[642:650])))
    mo = 33
    for G, paths in ((5, [str(tiny), str(big), str(mid), str(small)]), (3, [str(big), str(small), str(mid), str(tiny)]), (2, [str(mid), str(tiny), str(big)])):
        sizes = [os.path.getsize(p) for p in paths]
        T, cum = sum(sizes), np.concatenate([[0], np.cumsum([os.path.getsize(p) for p in paths])])
        cuts = [T * r // G for r in range(G + 1)]
        spans = [[f for f in range(len(paths)) if max(cuts[r], cum[f]) < min(cuts[r + 1], cum[f + 1])] for r in range(G)]
        assert any(len(s) >= 2 for s in spans), "one share spans two files"
        assert any(sum(f in s for s in spans) == 1 for f in range(len(paths))), "one file lies inside a single share"
        want, wfidx, wtotal, _ = _want(paths, mo)
        res = _ingest_and_pass(paths, mo, G)
        infos = _check_homes(res, want, wfidx)
        assert infos[0]["total_records"] == wtotal
        first = 1
        for f, p in zip(res[0]["files"], paths):  # the record counter runs through all files
            n_rec = pyoracle.load_good_reads([p], mo)[2]
            assert f["first_index"] == first and f["last_index"] == first + n_rec - 1
            first += n_rec
        _check_graph(res, want, wfidx)
    # the two-record file alone through five ranks: pieces without a record start
    want, wfidx, wtotal, _ = _want([str(tiny)], mo)
    res = _ingest_and_pass([str(tiny)], mo, 5, graph=False)
    infos = _check_homes(res, want, wfidx)
    assert wtotal == 2 and sum(1 for i in infos if i["share_reads"] == 0) >= 3


# ---- 4. imbalance -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
def test_a_first_file_without_a_good_read_moves_whole_shares(tmp_path, G):
    # the first file, which the filter empties (one base all over), is half of the bytes: with three or five ranks the first rank that has
    # good reads holds ids from 0 on — all inside rank 0's home range. Two ranks: the second has ALL the good reads, and keeps none only
    # when they fit one home range (64 ids: the ranges are multiples of 64)
    reads, rng = _pool(21 + G, 60 if G == 2 else 400, 0)
    good = tmp_path / "good.fasta"
    good.write_text(_fasta(reads))
    junk_reads, size = [], 0
    while size < os.path.getsize(good) + 200:
        junk_reads.append("A" * int(rng.integers(80, 160)))
        size = len(_fasta(junk_reads, tag="j"))
    junk = tmp_path / "junk.fasta"
    junk.write_text(_fasta(junk_reads, tag="j"))
    paths, mo = [str(junk), str(good)], 33
    want, wfidx, wtotal, _ = _want(paths, mo)
    assert pyoracle.load_good_reads([str(junk)], mo)[0] == []
    res = _ingest_and_pass(paths, mo, G)
    infos = _check_homes(res, want, wfidx)
    # from the counts: some rank made rows and kept none of them (its ids all lie in other ranks' home ranges)
    assert any(i["share_reads"] > 0 and i["kept_reads"] == 0 for i in infos), [(i["share_reads"], i["kept_reads"]) for i in infos]
    assert res[0]["files"][0]["good"] == 0 and res[0]["files"][0]["bad"] == len(junk_reads)
    _check_graph(res, want, wfidx)


# ---- 5. collective decline --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("what", ["gt_inside_a_line", "irregular_beyond_walking", "bgzf", "missing"])
def test_a_decline_anywhere_is_a_decline_everywhere(tmp_path, G, what):
    from tests import bgzf_util

    reads, rng = _pool(31, 300, 60)
    text = _fasta(reads)
    ok = tmp_path / "ok.fasta"
    ok.write_text(text)
    if what == "gt_inside_a_line":  # in the last header: only the last rank's share holds it
        at = text.rindex(">r")
        bad = tmp_path / "bad.fasta"
        bad.write_text(text[:at + 3] + ">" + text[at + 3:])
        assert at > len(text) * (G - 1) // G
        paths, named = [str(bad)], str(bad)
    elif what == "irregular_beyond_walking":  # in a middle share
        long_read = "".join(rng.choice(list("ACGT"), 6000))
        mid = text.index("\n>", len(text) // 2) + 1
        bad = tmp_path / "bad.fasta"
        bad.write_text(text[:mid] + ">irr\n" + _wrapped(rng, long_read, "irregular") + "\n" + text[mid:])
        paths, named = [str(bad)], str(bad)
        assert G == 2 or len(text) // G < mid < len(text) * (G - 1) // G  # (two ranks have no middle share: the second one's)
    elif what == "bgzf":
        gz = tmp_path / "ok.fasta.gz"
        gz.write_bytes(bgzf_util.bgzf_bytes(text.encode()))
        paths, named = [str(ok), str(gz)], str(gz)
    else:
        paths, named = [str(ok), str(tmp_path / "nobody.fasta")], str(tmp_path / "nobody.fasta")
    mo = 33
    want, wfidx, _, _ = _want([str(ok)], mo)

    def work(g, r):
        got = g.dist_ingest_fasta(paths, threads=2)
        msg = g.last_error()
        g.dist_upload_ascii(want)  # the same contexts take the host stage's reads
        return {"got": got, "msg": msg, "graph": _graph(g), "mo": mo}

    res = _ranks(G, mo, work)
    assert all(o["got"] is None for o in res), "every rank gets DISCO_E_UNSUPPORTED"
    assert all(named in o["msg"] and "the host input stage takes this job" in o["msg"] for o in res), [o["msg"] for o in res]
    assert len({o["msg"] for o in res}) == 1
    oe, orows, ocnt = run_oracle_reads(want, mo, count_hits=False)
    ce, cc = canon_hip(np.concatenate([o["graph"][0] for o in res]), np.concatenate([o["graph"][1] for o in res]), wfidx)
    oce, occ = canon_hip(oe, orows, wfidx)
    assert np.array_equal(ce, oce) and np.array_equal(cc, occ) and res[0]["graph"][2]["e_out"] == ocnt["e_out"] > 0


# ---- 6. long reads ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (2, 3))
def test_a_tail_of_long_reads_gets_the_rows_an_upload_gets(tmp_path, G):
    from tests.test_gpu_two_class import mixed_reads

    reads = mixed_reads(41 + G, 900, 100, 200, 20.0, 0.01, 600, 600)
    assert 2 <= sum(len(s) == 600 for s in reads) <= 40
    p = tmp_path / "long.fasta"
    p.write_text(_fasta(reads))
    mo = 40
    want, wfidx, _, _ = _want([str(p)], mo)
    res = _ingest_and_pass([str(p)], mo, G)
    _check_homes(res, want, wfidx)

    def uploaded(g, r):
        g.dist_upload_ascii(want)
        _graph(g)
        return g.long_rows

    up = _ranks(G, mo, uploaded)
    assert [o["long_rows"] for o in res] == up
    oe, orows, ocnt = run_oracle_reads(want, mo, count_hits=False)
    ce, cc = canon_hip(np.concatenate([o["graph"][0] for o in res]), np.concatenate([o["graph"][1] for o in res]), wfidx)
    oce, occ = canon_hip(oe, orows, wfidx)
    assert np.array_equal(ce, oce) and np.array_equal(cc, occ) and res[0]["graph"][2]["e_out"] == ocnt["e_out"] > 0


# ---- 7. the drop-in ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--gpus", "3", "--same-device", "-t", "4"], ["--gpus", "2", "--same-device", "--mpi-names"]])
def test_buildg_reads_its_files_on_every_rank(tmp_path, args):
    reads, rng = _pool(51, 500, 150)
    pe1, pe2, se = tmp_path / "a_1.fasta", tmp_path / "a_2.fastq", tmp_path / "s.fasta"
    pe1.write_text(_fasta(reads[:250]))
    pe2.write_text(_fastq(reads[250:450], rng))
    se.write_text("".join(f">w{i}\n{_wrapped(rng, s, 'w60')}\n" for i, s in enumerate(reads[450:])))
    gz = tmp_path / "s.fasta.gz"
    gz.write_bytes(gzip.compress(se.read_bytes()))
    cfg = tmp_path / "disco.cfg"
    cfg.write_text("MinOverlap4BuildGraph = 33\n")
    G = int(args[1])
    out = {}
    for how in ("device", "host", "gz"):
        prefix = str(tmp_path / how)
        # (the device stage under --gpus N is asked for: on ranks that share one device it is not faster than the host stage)
        env = dict(os.environ, DISCO_VERBOSE="1", DISCO_DIST_DEVICE_INPUT="1", **({"DISCO_HOST_INPUT": "1"} if how == "host" else {}))
        cmd = [os.path.join(BIN, "buildG"), "-pe", f"{pe1},{pe2}", "-se", str(gz if how == "gz" else se), "-f", prefix, "-p", str(cfg)] + args
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=JOIN_S)
        assert p.returncode == 0, p.stdout[-2000:]
        on_ranks = sum(f"input stage on rank {r} of {G}" in p.stdout for r in range(G))
        assert on_ranks == (G if how == "device" else 0), p.stdout[-2000:]
        assert ("the host input stage takes this job" in p.stdout) == (how == "gz"), p.stdout[-2000:]
        # (byte for byte; the LINES of an edge file as a sorted list: their order inside a file follows the emission's atomics in any two runs)
        out[how] = {os.path.basename(f)[len(how):]: sorted(open(f, "rb").read().splitlines()) if f.endswith("parGraph.txt") else open(f, "rb").read()
                    for f in sorted(glob.glob(prefix + "_*"))}
        # (_ReadIDMap.txt and the per-file lines name the input files: the gzipped file's name read as the plain one's)
        out[how]["_ReadIDMap.txt"] = out[how]["_ReadIDMap.txt"].replace(os.fsencode(str(gz)), os.fsencode(str(se)))
        out[how + "_log"] = [l.replace(str(gz), str(se)) for l in p.stdout.splitlines()
                             if "reads in current dataset" in l or "read length in all datasets" in l or l.startswith("File name:")]
    for how in ("host", "gz"):
        assert out["device"].keys() == out[how].keys() and len(out["device"]) >= 4
        for k in out["device"]:
            assert out["device"][k] == out[how][k], (how, k)
        assert out["device_log"] == out[how + "_log"] and len(out["device_log"]) == 4 * 3 + 2
    assert out["device"]["_ReadIDMap.txt"].count(b"\n") >= 3


# ---- 8. the seams of the record-finding kernels, and one rank against one GPU -------------------------------------------------------------
@pytest.mark.parametrize("G", (2, 3))
def test_block_and_lane_edges_under_a_communicator(tmp_path, G):
    """the files of tests/test_gpu_ingest.py::test_record_starts_on_block_and_lane_edges through G ranks: the top piece of a file begins
    its buffer as a whole file does; the other pieces see the same seams one byte further on"""
    mo = 33
    files = edge_files(tmp_path)
    names = list(files)

    def work(g, r):  # the same contexts take one input after the other
        out = {}
        for name in names:
            got = g.dist_ingest_fasta([files[name][0]], threads=2)
            if name == EDGE_DECLINED:
                out[name] = (got, g.last_error())
                continue
            assert got is not None, (name, g.last_error())
            out[name] = {"info": got[0], "files": got[1], "home": _home(g)}
        return out

    res = _ranks(G, mo, work)
    for name in names:
        want, wfidx, wtotal = edge_want(files[name][0], mo)
        if name == EDGE_DECLINED:
            assert want == [] and all(o[name][0] is None and "no good read (or more than 2^31)" in o[name][1] for o in res), name
            continue
        infos = _check_homes([o[name] for o in res], want, wfidx)
        assert infos[0]["total_records"] == wtotal and len(want) > 10, name


def test_a_communicator_of_one_rank_makes_the_table_one_gpu_makes(tmp_path):
    reads, rng = _pool(61, 1500, 500)
    fa, fq = tmp_path / "one.fasta", tmp_path / "one.fastq"
    fa.write_text(_fasta(reads))
    fq.write_text(_fastq(reads, rng))
    mo = 33
    for p in (str(fa), str(fq)):
        def work(g, r):
            got = g.dist_ingest_fasta([p], threads=2)
            assert got is not None, g.last_error()
            ln, fi = g.dist_ingest_fetch()
            packed, lens = g.download_reads()
            return got[0], got[1], ln, fi, packed, lens

        (dinfo, dfiles, dln, dfi, dpacked, dlens), = _ranks(1, mo, work)
        with buildgraph.BuildGraph(min_overlap=mo) as g:
            info, files = g.ingest_fasta([p], threads=2)
            ln, fi = g.ingest_fetch()
            packed, lens = g.download_reads()
        assert len(ln) > 1500
        for k in ("n_reads", "total_records", "too_long"):
            assert dinfo[k] == info[k], k
        assert dfiles == files
        assert np.array_equal(dln, ln) and np.array_equal(dlens, lens) and np.array_equal(dfi, fi)
        m = min(dpacked.shape[1], packed.shape[1])  # (the row strides may differ: words behind a read are zero in both)
        assert np.array_equal(dpacked[:, :m], packed[:, :m]) and not dpacked[:, m:].any() and not packed[:, m:].any()
