"""-m gpu : buildG writes the contained-read files from the GPU (disco_format_contained + disco_write_contained_text) — byte for byte, order
included, what the host writer produces (DISCO_HOST_CONTAINED_TEXT=1)."""
import os
import subprocess

import pytest

from disco_amd import build, readgen
from tests import golden_util as gu
from tests.test_gpu_contained_text import BIG_CASES, big_group_reads

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")
GPU_LAP = "format contained lines on the GPU"
HOST_LAP = "write_contained sort"


def _multifile():
    c = gu.CASES["multifile"]
    return ["-pe", ",".join(os.path.join(gu.GOLD, f) for f in c["pe"]), "-se", ",".join(os.path.join(gu.GOLD, f) for f in c["se"])], c["min_overlap"]


def _run(tmp_path, how, inputs, mo, threads, extra=(), env_extra=None):
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {mo}\n")
    prefix = str(tmp_path / how)
    env = dict(os.environ, DISCO_VERBOSE="1", **(env_extra or {}))
    p = subprocess.run([os.path.join(BIN, "buildG")] + inputs + ["-f", prefix, "-p", str(cfg), "-t", str(threads)] + list(extra), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=env)
    assert p.returncode == 0, p.stdout
    contained = [open(f"{prefix}_{t}_containedReads.txt", "rb").read() for t in range(threads)]
    # (the order of the edges inside a file is the order of the emission, which differs from run to run: lines compared sorted)
    edges = [sorted(open(f"{prefix}_{t}_parGraph.txt", "rb").read().split(b"\n")) for t in range(threads)]
    return p.stdout, contained, edges


@pytest.mark.parametrize("case,threads", [("multifile", 1), ("multifile", 4), ("generated", 16), ("generated", 3), ("big_groups", 3)])
def test_contained_files_from_the_gpu_are_the_host_writers_bytes(tmp_path, case, threads):
    build.build_host()
    if case == "multifile":   # its records are filtered: file index != read id + 1
        inputs, mo = _multifile()
    elif case == "generated":
        fa = str(tmp_path / "r.fasta")
        readgen.write_fasta(fa, readgen.generate_reads(readgen.GenSpec.coverage(seed=31, n_reads=200_000, read_len=100, cov=30.0, n_contigs=7, len_max=260)))
        inputs, mo = ["-se", fa], 40
    else:                     # groups of up to 40 000 rows: the host run sorts on the host
        c = BIG_CASES["two_classes"]
        fa = str(tmp_path / "big.fasta")
        with open(fa, "w") as f:
            f.write("".join(f">r{i}\n{r}\n" for i, r in enumerate(big_group_reads(c["L"], c["l"], c["sizes"]))))
        inputs, mo = ["-se", fa], c["min_overlap"]
    out_gpu, cont_gpu, edges_gpu = _run(tmp_path, "gpu", inputs, mo, threads)
    out_host, cont_host, edges_host = _run(tmp_path, "host", inputs, mo, threads, env_extra={"DISCO_HOST_CONTAINED_TEXT": "1"})
    assert GPU_LAP in out_gpu and "contained lines into the files" in out_gpu and HOST_LAP not in out_gpu
    assert GPU_LAP not in out_host and HOST_LAP in out_host
    assert cont_gpu == cont_host            # NOT sorted first: the order of the rows is part of the contract
    assert sum(x.count(b"\n") for x in cont_gpu) > (50 if case == "multifile" else 1000)
    assert edges_gpu == edges_host
    if case == "big_groups":
        assert sum(x.count(b"\n") for x in cont_gpu) == BIG_CASES["two_classes"]["n_rows"]


def test_binary_out_keeps_the_host_path_and_writes_the_same_text(tmp_path):
    """--binary-out needs the rows on the host: the old path, the same text files"""
    build.build_host()
    inputs, mo = _multifile()
    out_plain, cont_plain, edges_plain = _run(tmp_path, "plain", inputs, mo, 3)
    out_bin, cont_bin, edges_bin = _run(tmp_path, "bin", inputs, mo, 3, extra=["--binary-out"])
    assert GPU_LAP in out_plain and GPU_LAP not in out_bin and HOST_LAP in out_bin
    assert cont_bin == cont_plain and edges_bin == edges_plain
    assert os.path.getsize(str(tmp_path / "bin") + "_contained.bin") > 0
