"""-m gpu : buildG writes the binary side output from the GPU (DISCO_GPU_BINARY=1: disco_write_edge_records / disco_write_contained_records
behind a header the host writes) — the files the host writer produces (DISCO_GPU_BINARY=0), and the text files of a run without the flag."""
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build, edgefile, readgen
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")
GPU_LAPS = ("binary contained records on the GPU", "binary edge records on the GPU")
HOST_LAP = "write binary side output"
CONTAINED_TEXT_LAP = "format contained lines on the GPU"


def _multifile():
    c = gu.CASES["multifile"]  # its records are filtered: file index != read id + 1
    return ["-pe", ",".join(os.path.join(gu.GOLD, f) for f in c["pe"]), "-se", ",".join(os.path.join(gu.GOLD, f) for f in c["se"])], c["min_overlap"], 3


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """200 000 reads of 100 .. 260 bases as FASTA: as generated, and with substitutions at 0.4 % per base (for --max-substitutions)"""
    d = tmp_path_factory.mktemp("binreads")
    spec = readgen.GenSpec.coverage(seed=31, n_reads=200_000, read_len=100, cov=30.0, n_contigs=7, len_max=260)
    codes, off = readgen.generate_codes(spec)
    exact, mutated = str(d / "r.fasta"), str(d / "m.fasta")
    readgen.write_fasta(exact, readgen.codes_to_reads(codes, off))
    rng = np.random.default_rng(1031)
    m = rng.random(len(codes)) < 0.004
    codes = codes.copy()
    codes[m] = (codes[m] + rng.integers(1, 4, int(m.sum())).astype(np.uint8)) % 4
    readgen.write_fasta(mutated, readgen.codes_to_reads(codes, off))
    return {"exact": exact, "mutated": mutated}


def _run(tmp_path, how, inputs, mo, threads, extra=(), knob=None):
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {mo}\n")
    prefix = str(tmp_path / how)
    env = dict(os.environ, DISCO_VERBOSE="1")
    env.pop("DISCO_GPU_BINARY", None)
    if knob is not None:
        env["DISCO_GPU_BINARY"] = knob
    extra = [str(tmp_path / (how + "_ps")) if x == "PS" else x for x in extra]
    p = subprocess.run([os.path.join(BIN, "buildG")] + inputs + ["-f", prefix, "-p", str(cfg), "-t", str(threads)] + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=env)
    assert p.returncode == 0, p.stdout
    return p.stdout, prefix


def _text(prefix, threads):
    """the text files of a run, by kind and file: edge lines sorted (their order is the emission's, which differs from run to run), contained
    files as they are"""
    return ([sorted(open(f"{prefix}_{t}_parGraph.txt").read().splitlines()) for t in range(threads)],
            [open(f"{prefix}_{t}_containedReads.txt").read() for t in range(threads)])


def _text_of_binary(prefix, threads):
    texts = edgefile.text_files(prefix)
    assert len(texts) == 2 * threads
    return ([sorted(texts[f"{prefix}_{t}_parGraph.txt"].splitlines()) for t in range(threads)], [texts[f"{prefix}_{t}_containedReads.txt"] for t in range(threads)])


FLAGS = {
    "no-text": ["--no-text"],
    "binary-out": ["--binary-out"],
    "no-text+par-simple": ["--no-text", "--par-simple", "PS"],
    "binary-out+subs": ["--binary-out", "--max-substitutions", "2"],
}


def test_defaults_without_the_variable(tmp_path):
    """--no-text takes the device path by default (profiles/binary_records.txt), --binary-out the host writer"""
    build.build_host()
    inputs, mo, threads = _multifile()
    out_nt, _ = _run(tmp_path, "nt", inputs, mo, threads, ["--no-text"])
    out_bo, _ = _run(tmp_path, "bo", inputs, mo, threads, ["--binary-out"])
    assert all(lap in out_nt for lap in GPU_LAPS) and HOST_LAP not in out_nt and "fetch edges" not in out_nt
    assert not any(lap in out_bo for lap in GPU_LAPS) and HOST_LAP in out_bo


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("fixture", ["multifile", "generated"])
def test_binary_files_from_the_gpu_are_the_host_writers(tmp_path, generated, fixture, flags):
    build.build_host()
    extra = FLAGS[flags]
    subs = ["--max-substitutions", "2"] if "subs" in flags else []
    if fixture == "multifile":
        inputs, mo, threads = _multifile()
    else:
        inputs, mo, threads = ["-se", generated["mutated" if subs else "exact"]], 40, 16
    out_on, on = _run(tmp_path, "on", inputs, mo, threads, extra, knob="1")
    out_off, off = _run(tmp_path, "off", inputs, mo, threads, extra, knob="0")
    out_plain, plain = _run(tmp_path, "plain", inputs, mo, threads, subs)
    # the laps: the device path prints its two and not the host writer's; the host path the reverse
    assert all(lap in out_on for lap in GPU_LAPS) and HOST_LAP not in out_on, out_on
    assert not any(lap in out_off for lap in GPU_LAPS) and HOST_LAP in out_off, out_off
    if "--no-text" in extra and "--par-simple" not in extra:  # nothing is fetched for the binary files (the verbose laps of the fetches)
        assert "fetch edges" not in out_on and "fetch edges" in out_off
    # <prefix>_contained.bin: byte for byte (the order of the rows is part of the contract)
    c_on, c_off = open(on + "_contained.bin", "rb").read(), open(off + "_contained.bin", "rb").read()
    assert c_on == c_off and len(c_on) > 32 + 40 * (50 if fixture == "multifile" else 1000)
    # <prefix>_edges.bin: the header, and the records as sorted arrays (the emission's order differs from run to run)
    e_on, e_off = open(on + "_edges.bin", "rb").read(), open(off + "_edges.bin", "rb").read()
    assert e_on[:32] == e_off[:32] and len(e_on) == len(e_off)
    r_on, nf_on = edgefile.read_edges(on + "_edges.bin")
    r_off, nf_off = edgefile.read_edges(off + "_edges.bin")
    assert nf_on == nf_off == threads and len(r_on) > (0 if fixture == "multifile" else 1000)
    names = list(edgefile.EDGE.names)
    assert np.array_equal(np.sort(r_on, order=names), np.sort(r_off, order=names))
    assert set(np.unique(r_on["flag"])) == {2}
    if subs and fixture == "generated":
        assert r_on["substitutions"].max() > 0
    # the binary pair stands for the text files of a run without the flag
    plain_text = _text(plain, threads)
    assert _text_of_binary(on, threads) == plain_text
    if "--binary-out" in extra:   # ... which that run's own text files are too, written the way the plain run writes them
        assert _text(on, threads) == plain_text
        assert (CONTAINED_TEXT_LAP in out_on) == (CONTAINED_TEXT_LAP in out_plain) and CONTAINED_TEXT_LAP in out_on
        assert CONTAINED_TEXT_LAP not in out_off
    else:                         # --no-text: the file lists exist, empty
        assert all(os.path.getsize(f"{on}_{t}_parGraph.txt") == 0 and os.path.getsize(f"{on}_{t}_containedReads.txt") == 0 for t in range(threads))
    if "--par-simple" in extra:   # the partial simplification beside it: the same files either way
        for t in range(threads):
            a = sorted(open(f"{tmp_path / 'on_ps'}_{t}_ParSimpleEdges.txt").read().splitlines())
            b = sorted(open(f"{tmp_path / 'off_ps'}_{t}_ParSimpleEdges.txt").read().splitlines())
            assert a == b, t
