"""-m gpu : BGZF-compressed FASTA / FASTQ through the device input stage (disco_ingest_fasta: the file travels compressed, one wavefront
per member decodes it in front of the record kernels) — the same reads, counts and file indices as the plain file gives, whatever
the deflate settings and wherever the member boundaries fall; damaged members decline the call; buildG end to end."""
import glob
import os
import subprocess
import zlib

import numpy as np
import pytest

from disco_amd import build, buildgraph
from oracle import pyoracle
from tests import bgzf_util as bz
from tests import golden_util as gu
from tests.test_gpu_ingest import _adversarial, _decode, _ingest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disco_amd", "bin")
VARIANTS = [(dict(level=0), 65280), (dict(level=0), 4096), (dict(level=6), 65280), (dict(level=6), 4096), (dict(strategy=zlib.Z_FIXED), 65280),
            (dict(strategy=zlib.Z_FIXED), 4096)]


def _reads(seed=3):
    from disco_amd import readgen

    rng = np.random.default_rng(seed)
    reads = list(readgen.generate_reads(readgen.GenSpec.coverage(seed=seed, n_reads=3000, read_len=100, cov=20.0, len_max=180))) + _adversarial(rng, 400)
    return [reads[j] for j in rng.permutation(len(reads))], rng


def _text(kind):
    reads, rng = _reads()
    if kind == "fasta":
        return "".join(f">r{i} d\n{s}\n" for i, s in enumerate(reads)).encode()
    if kind == "wrapped":
        return "".join(f">r{i}\n" + "\n".join(s[q:q + 60] for q in range(0, len(s), 60)) + "\n" for i, s in enumerate(reads)).encode()
    reads = [s for s in reads if len(s) <= 32767]
    return "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads)).encode()


def _same(a, b):
    (ia, fa, ra, xa), (ib, fb, rb, xb) = a, b
    keys = ("n_reads", "total_records", "too_long", "stride_words", "shortest", "longest")
    assert {k: ia[k] for k in keys} == {k: ib[k] for k in keys}
    assert fa == fb and ra == rb and np.array_equal(xa, xb)


@pytest.mark.parametrize("kind", ["fasta", "fastq", "wrapped"])
def test_bgzf_ingest_equals_the_plain_files(tmp_path, kind):
    text = _text(kind)
    plain = tmp_path / ("r." + kind)
    plain.write_bytes(text)
    want = _ingest([str(plain)], 35)
    oreads, ofidx, ototal = pyoracle.load_good_reads([str(plain)], 35)
    keep = [i for i, s in enumerate(oreads) if len(s) <= 32767]
    assert want[2] == [oreads[i] for i in keep] and np.array_equal(want[3].astype(np.int64), np.asarray(ofidx, dtype=np.int64)[keep])
    assert want[0]["total_records"] == ototal and len(want[2]) > 2000
    # records straddle the members: a boundary inside a sequence line
    inside = [b for b in range(4096, len(text), 4096) if text[b - 1] != 10 and text[b] != 10 and text[text.rfind(b"\n", 0, b) + 1] not in b">@+"]
    assert inside
    for n, (settings, member) in enumerate(VARIANTS):
        gz = tmp_path / f"v{n}.{kind}.gz"
        gz.write_bytes(bz.bgzf_bytes(text, member, eof=n % 2 == 0, **settings))
        got = _ingest([str(gz)], 35)
        assert got is not None, (settings, member)
        _same(got, want)


def test_plain_and_bgzf_files_in_one_call(tmp_path):
    a, b = _text("fasta"), _text("fastq")
    pa, pb, gb = tmp_path / "a.fasta", tmp_path / "b.fastq", tmp_path / "b.fastq.gz"
    pa.write_bytes(a)
    pb.write_bytes(b)
    gb.write_bytes(bz.bgzf_bytes(b, 4096))
    want, got = _ingest([str(pa), str(pb)], 35), _ingest([str(pa), str(gb)], 35)
    _same(got, want)
    _same(_ingest([str(gb), str(pa)], 35), _ingest([str(pb), str(pa)], 35))


def test_a_tail_of_long_reads_from_bgzf(tmp_path):
    from tests.test_gpu_two_class import mixed_reads

    reads = mixed_reads(33, 6000, 100, 250, 30.0, 0.01, 257, 3000)
    text = "".join(f">t{i}\n{s}\n" for i, s in enumerate(reads)).encode()
    plain, gz = tmp_path / "t.fa", tmp_path / "t.fa.gz"
    plain.write_bytes(text)
    gz.write_bytes(bz.bgzf_bytes(text))
    res = []
    for p in (plain, gz):
        with buildgraph.BuildGraph(min_overlap=40) as g:
            info, files = g.ingest_fasta([str(p)], threads=4)
            ln, fi = g.ingest_fetch()
            packed, lens = g.download_reads()
            res.append((g.long_rows, info["n_reads"], files, fi, packed, lens))
    assert res[0][0] == res[1][0] > 30 and res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert np.array_equal(res[0][3], res[1][3]) and np.array_equal(res[0][5], res[1][5]) and np.array_equal(res[0][4], res[1][4])
    assert _decode(res[1][4][:50], res[1][5][:50]) == reads[:50]


def test_a_damaged_member_declines_the_file_and_the_context_goes_on(tmp_path):
    text = _text("fasta")
    mem = bz.bgzf_members(text, 65280)
    good, bad = tmp_path / "good.fa.gz", tmp_path / "bad.fa.gz"
    good.write_bytes(b"".join(mem) + bz.EOF_MEMBER)
    m = bytearray(mem[2])
    m[-6] ^= 0x40  # the trailer's CRC32
    bad.write_bytes(b"".join(mem[:2]) + bytes(m) + b"".join(mem[3:]) + bz.EOF_MEMBER)
    plain = tmp_path / "p.fa"
    plain.write_bytes(text)
    with buildgraph.BuildGraph(min_overlap=35) as g:
        assert g.ingest_fasta([str(bad)], threads=4) is None
        assert "member 2" in g.last_error() and "CRC32" in g.last_error() and "the host input stage takes this job" in g.last_error()
        info, files = g.ingest_fasta([str(good)], threads=4)
        packed, lens = g.download_reads()
        got = _decode(packed, lens)
    assert got == _ingest([str(plain)], 35)[2] and info["n_reads"] == len(got)


def _buildg(args, env=None):
    p = subprocess.run([os.path.join(BIN, "buildG")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, DISCO_VERBOSE="1", **(env or {})))
    assert p.returncode == 0, p.stdout[-1500:]
    return p.stdout


def test_buildg_reads_the_multifile_fixture_with_its_plain_fasta_as_bgzf(tmp_path):
    from oracle import refrun

    build.build_host()
    c = gu.CASES["multifile"]
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {c['min_overlap']}\n")
    gz = tmp_path / "plain.fasta.gz"
    gz.write_bytes(bz.bgzf_bytes(open(os.path.join(gu.GOLD, c["se"][0]), "rb").read(), 4096))
    prefix = str(tmp_path / "m")
    log = _buildg(["-pe", ",".join(os.path.join(gu.GOLD, f) for f in c["pe"]), "-se", str(gz), "-f", prefix, "-p", str(cfg), "-t", "2"])
    assert "input stage on the GPU" in log and "the host input stage takes this job" not in log, log[-1500:]
    gu.check_against_golden("multifile", refrun.parse_pargraph(sorted(glob.glob(prefix + "_*_parGraph.txt"))), refrun.parse_contained(sorted(glob.glob(prefix + "_*_containedReads.txt"))))


def test_buildg_on_bgzf_writes_the_host_stages_files(tmp_path):
    """the 20 000-read FASTA of tests/test_gpu_ingest.py's CLI test as BGZF: the device stage against DISCO_HOST_INPUT=1 (zlib) on the same .gz"""
    from disco_amd import readgen

    build.build_host()
    rng = np.random.default_rng(11)
    spec = readgen.GenSpec.coverage(seed=21, n_reads=20000, read_len=100, cov=20.0, n_contigs=3, len_max=180)
    reads = list(readgen.generate_reads(spec)) + _adversarial(rng, 2000)
    order = rng.permutation(len(reads))
    gz = tmp_path / "r.fasta.gz"
    gz.write_bytes(bz.bgzf_bytes("".join(f">q{i}\n{reads[j]}\n" for i, j in enumerate(order)).encode()))
    cfg = tmp_path / "disco.cfg"
    cfg.write_text("MinOverlap4BuildGraph = 40\n")
    out = {}
    for how in ("device", "host"):
        prefix = str(tmp_path / how)
        log = _buildg(["-se", str(gz), "-f", prefix, "-p", str(cfg), "-t", "3"], {"DISCO_HOST_INPUT": "1"} if how == "host" else None)
        assert ("input stage on the GPU" in log) == (how == "device"), log[-1500:]
        out[how] = {os.path.basename(f)[len(how):]: sorted(open(f, "rb").read().splitlines()) for f in sorted(glob.glob(prefix + "_*"))}
    assert out["device"].keys() == out["host"].keys() and len(out["device"]) >= 3 * 3 + 2
    for k in out["device"]:
        assert out["device"][k] == out["host"][k], k
