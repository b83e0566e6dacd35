"""-m gpu : buildG --par-simple writes its files from the GPU (DISCO_PAR_SIMPLE_GPU_TEXT=1: the residue of the chain contraction and the
composite edges' headers to the host pass, its description of the final lines to disco_format_par_simple, the text through the pinned
ring into the files) — byte for byte, order included, what the flow through the host writes (DISCO_PAR_SIMPLE_HOST_TEXT=1: edges, links
and text fetched) and what the host walk writes (DISCO_PAR_SIMPLE_HOST=1: no contraction on the GPU at all)."""
import os
import re
import subprocess

import pytest

from disco_amd import build, readgen

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")
FLOWS = {"gpu": {"DISCO_PAR_SIMPLE_GPU_TEXT": "1"}, "host_text": {"DISCO_PAR_SIMPLE_HOST_TEXT": "1"}, "host": {"DISCO_PAR_SIMPLE_HOST": "1"}}
GPU_LINE = "partial simplification on the GPU:"


def _run(tmp_path, how, fa, threads, simplify=45, extra=("--no-text",), env_extra=None, par_simple=True):
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = 40\nMinOverlap4SimplifyGraph = {simplify}\n")
    prefix = str(tmp_path / f"g_{how}")
    cmd = [os.path.join(BIN, "buildG"), "-se", fa, "-f", prefix, "-p", str(cfg), "-t", str(threads)] + list(extra)
    if par_simple:
        cmd += ["--par-simple", str(tmp_path / f"s_{how}")]
    env = dict(os.environ, DISCO_VERBOSE="1", **FLOWS.get(how, {}), **(env_extra or {}))
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert p.returncode == 0, p.stdout
    files = [open(str(tmp_path / f"s_{how}_{t}_ParSimpleEdges.txt"), "rb").read() for t in range(threads)] if par_simple else None
    return p.stdout, files, prefix


def _assert_same_bytes(a, b):
    """NOT sorted first: the order of the lines is part of the contract (the message names the first line that differs)"""
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        if x != y:
            lx, ly = x.splitlines(), y.splitlines()
            i = next((i for i, (p, q) in enumerate(zip(lx, ly)) if p != q), min(len(lx), len(ly)))
            raise AssertionError(f"file {t}: {len(lx)} / {len(ly)} lines, the same set: {sorted(lx) == sorted(ly)}; line {i}: {lx[i:i + 2]!r} / {ly[i:i + 2]!r}"[:3000])


def _stats(out):
    line = [l for l in out.splitlines() if l.startswith("Partial simplification")][0]
    return re.sub(r"\d+ rounds", "R rounds", line.split("files")[0])


@pytest.mark.parametrize("shape", ["uniform", "metagenome", "errors"])
def test_the_three_flows_write_the_same_bytes(tmp_path, shape):
    build.build_host()
    if shape == "uniform":
        spec = readgen.GenSpec.coverage(seed=15, n_reads=400_000, read_len=150, cov=30.0, n_contigs=4)
    else:
        spec = readgen.GenSpec.coverage(seed=16, n_reads=400_000, read_len=100, cov=25.0, n_contigs=40, len_max=250, skew=1 if shape == "metagenome" else 0)
    codes, off = readgen.generate_codes(spec)
    if shape == "errors":
        codes = readgen.substitute(codes, off, 3, 2000)
    fa = str(tmp_path / "r.fasta")
    readgen.write_fasta(fa, readgen.codes_to_reads(codes, off))
    out, files = {}, {}
    for how in FLOWS:
        out[how], files[how], _ = _run(tmp_path, how, fa, 4)
    _assert_same_bytes(files["gpu"], files["host_text"])
    _assert_same_bytes(files["gpu"], files["host"])
    assert sum(x.count(b"\n") for x in files["gpu"]) > 0
    assert _stats(out["gpu"]) == _stats(out["host_text"]) == _stats(out["host"])
    assert GPU_LINE in out["gpu"] and GPU_LINE not in out["host_text"] and GPU_LINE not in out["host"]
    assert "contract chains on the GPU" in out["gpu"] and "contract chains on the GPU" in out["host_text"] and "contract chains on the GPU" not in out["host"]
    assert "fetch edges" in out["host_text"]   # the fallback is alive (--no-text asks for the binary side output, which fetches the edges in every flow)
    if shape == "errors":   # the only place later rounds meet device link arrays: edges composed of several pieces, some turned round
        m = re.search(r"in (\d+) pieces \((\d+) reversed, at most (\d+) in one edge\)", out["gpu"])
        assert m, out["gpu"]
        print(m.group(0))
        assert int(m.group(3)) >= 2 and int(m.group(2)) >= 1


N_RECORDS = []   # 1-based record numbers of the filtered records of the last _small_fasta(with_n=True)


def _small_fasta(tmp_path, with_n=False):
    reads = readgen.generate_reads(readgen.GenSpec.coverage(seed=5, n_reads=30000, read_len=110, cov=20.0, n_contigs=6, len_max=190))
    fa = str(tmp_path / "r.fasta")
    del N_RECORDS[:]
    if with_n:   # every 37th record is filtered (a read with N): file index != read id + 1 from there on
        out = []
        for i, r in enumerate(reads):
            if i % 37 == 5:
                out.append(r[:20] + "N" + r[21:])
                N_RECORDS.append(len(out))
            out.append(r)
        reads = out
    readgen.write_fasta(fa, reads)
    return fa


def test_with_text_the_edge_lines_stream_and_no_edge_reaches_the_host(tmp_path):
    build.build_host()
    fa = _small_fasta(tmp_path)
    out_gpu, ps_gpu, pre_gpu = _run(tmp_path, "gpu", fa, 3, simplify=40, extra=())
    out_host, ps_host, _ = _run(tmp_path, "host_text", fa, 3, simplify=40, extra=())
    out_plain, _, pre_plain = _run(tmp_path, "plain", fa, 3, simplify=40, extra=(), par_simple=False)
    _assert_same_bytes(ps_gpu, ps_host)
    assert sum(x.count(b"\n") for x in ps_gpu) > 0
    assert "edge lines into the files" in out_gpu and "fetch edges" not in out_gpu and "fetch edge lines" not in out_gpu
    assert "fetch edges" in out_host
    for t in range(3):
        for kind in ("parGraph", "containedReads"):
            a, b = open(f"{pre_gpu}_{t}_{kind}.txt", "rb").read(), open(f"{pre_plain}_{t}_{kind}.txt", "rb").read()
            # (the order of the edges inside a file is the order of the emission, which differs from run to run)
            assert sorted(a.split(b"\n")) == sorted(b.split(b"\n")) and (kind == "parGraph" or a == b)


def test_filtered_records_print_file_indices(tmp_path):
    build.build_host()
    fa = _small_fasta(tmp_path, with_n=True)
    out_gpu, ps_gpu, _ = _run(tmp_path, "gpu", fa, 2, simplify=40)
    out_host, ps_host, _ = _run(tmp_path, "host", fa, 2, simplify=40)
    assert GPU_LINE in out_gpu
    _assert_same_bytes(ps_gpu, ps_host)
    ids = {int(x) for f in ps_gpu for line in f.splitlines() for x in line.split(b"\t")[:2] + re.findall(rb"\((\d+),", line)}
    assert max(ids) > 30000 and not ids & set(N_RECORDS)   # numbers of the file's records, not read ids (30 000 reads), and never a filtered one


def test_disco_par_simple_env_with_the_pipeline_layout(tmp_path):
    build.build_host()
    fa = _small_fasta(tmp_path)
    cfg = tmp_path / "disco.cfg"
    cfg.write_text("MinOverlap4BuildGraph = 40\nMinOverlap4SimplifyGraph = 40\n")
    got = {}
    for how in ("gpu", "host"):
        os.makedirs(tmp_path / how / "graph")
        p = subprocess.run([os.path.join(BIN, "buildG"), "-se", fa, "-f", str(tmp_path / how / "graph" / "asm"), "-p", str(cfg), "-t", "3"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, env=dict(os.environ, DISCO_PAR_SIMPLE="1", DISCO_VERBOSE="1", **FLOWS[how]))
        assert p.returncode == 0 and "Partial simplification" in p.stdout, p.stdout
        assert (GPU_LINE in p.stdout) == (how == "gpu")
        got[how] = [open(tmp_path / how / "assembly" / f"asm_{t}_ParSimpleEdges.txt", "rb").read() for t in range(3)]
    assert got["gpu"] == got["host"] and sum(len(x) for x in got["gpu"]) > 0
