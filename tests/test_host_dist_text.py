"""-m gpu : buildG --gpus N writes its edge and contained-read files from the ranks' GPUs (disco_dist_format_contained /
disco_dist_format_edges, every rank its own files) — the files of the host writer (DISCO_HOST_TEXT=1) and of the real reference."""
import glob
import os
import subprocess

import pytest

from disco_amd import build, readgen
from oracle import refrun
from tests import golden_util as gu
from tests.test_host import _file_tags

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")
RANK_LAPS = ("format contained lines on the GPU", "contained lines into the files", "partition + format edge lines on the GPU", "edge lines into the files")


def _inputs(case, tmp_path):
    if case == "multifile":   # its records are filtered: file index != read id + 1
        c = gu.CASES["multifile"]
        return ["-pe", ",".join(os.path.join(gu.GOLD, f) for f in c["pe"]), "-se", ",".join(os.path.join(gu.GOLD, f) for f in c["se"])], c["min_overlap"]
    reads, _, mo = gu.case_inputs(case)
    fa = str(tmp_path / (case + ".fasta"))
    if not os.path.exists(fa):
        readgen.write_fasta(fa, reads)
    return ["-se", fa], mo


def _run(tmp_path, how, inputs, mo, threads, gpus, mpi_names, extra=(), env_extra=None):
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {mo}\n")
    prefix = str(tmp_path / how)
    env = dict(os.environ, DISCO_VERBOSE="1", DISCO_DIST_GPU_TEXT="1", **(env_extra or {}))
    cmd = [os.path.join(BIN, "buildG")] + inputs + ["-f", prefix, "-p", str(cfg), "-t", str(threads), "--gpus", str(gpus), "--same-device"]
    p = subprocess.run(cmd + (["--mpi-names"] if mpi_names else []) + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout
    etags, ctags = _file_tags(threads, gpus, mpi_names)
    assert len(glob.glob(prefix + "_*_parGraph.txt")) == len(etags) and len(glob.glob(prefix + "_*_containedReads.txt")) == len(ctags)
    contained = [open(f"{prefix}_{t}_containedReads.txt", "rb").read() for t in ctags]   # (every file must exist, empty or not)
    edges = [sorted(open(f"{prefix}_{t}_parGraph.txt", "rb").read().splitlines()) for t in etags]
    assert open(prefix + "_CheckpointInfo.txt").read() == "CCR=Complete\nGC=Complete\n"
    return p.stdout, contained, edges, prefix


def _canonical(prefix):
    return refrun.parse_pargraph(sorted(glob.glob(prefix + "_*_parGraph.txt"))), refrun.parse_contained(sorted(glob.glob(prefix + "_*_containedReads.txt")))


@pytest.mark.parametrize("mpi_names", [False, True])
@pytest.mark.parametrize("threads", [2, 3])
@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("case", ["multifile", "tail_20k"])
def test_files_written_by_the_ranks_are_the_host_writers_and_the_references(tmp_path, case, gpus, threads, mpi_names):
    build.build_host()
    inputs, mo = _inputs(case, tmp_path)
    out_dev, cont_dev, edges_dev, prefix = _run(tmp_path, "dev", inputs, mo, threads, gpus, mpi_names)
    out_host, cont_host, edges_host, _ = _run(tmp_path, "host", inputs, mo, threads, gpus, mpi_names, env_extra={"DISCO_HOST_TEXT": "1"})
    # the device path was taken: every rank reports its four steps — and none of them under DISCO_HOST_TEXT=1
    for what in RANK_LAPS:
        for r in range(gpus):
            assert f"rank {r}: {what}" in out_dev, (what, r, out_dev)
        assert what not in out_host
    assert "partition edges into files" not in out_dev and "partition edges into files" in out_host   # no host partition, nothing gathered
    assert cont_dev == cont_host              # NOT sorted first: the order of the rows is part of the contract
    assert edges_dev == edges_host            # file by file, as sorted lines
    assert sum(x.count(b"\n") for x in cont_dev) > 50 and sum(len(x) for x in edges_dev) > 50
    gu.check_against_golden(case, *_canonical(prefix))


@pytest.mark.parametrize("extra", [["--binary-out"], ["--par-simple", "PS"], ["--max-substitutions", "1"]], ids=["binary-out", "par-simple", "max-substitutions"])
def test_declining_cases_take_the_host_path_and_deliver_the_reference(tmp_path, extra):
    """what needs the records on the host, or a column the device does not write, keeps the host writer — inside the same run"""
    build.build_host()
    inputs, mo = _inputs("multifile", tmp_path)
    extra = [str(tmp_path / "ps") if x == "PS" else x for x in extra]
    out, _, _, prefix = _run(tmp_path, "g", inputs, mo, 3, 2, False, extra=extra)
    for what in RANK_LAPS:
        assert what not in out, out
    assert "partition edges into files" in out
    gu.check_against_golden("multifile", *_canonical(prefix))
