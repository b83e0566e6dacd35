"""-m gpu : the rows of buildG's output-route matrix ("Who writes which file") that no other test runs — every case against
the same flags with every route forced to the host (DISCO_HOST_TEXT=1 DISCO_GPU_BINARY=0 DISCO_PAR_SIMPLE_HOST=1): the same files, and the
verbose laps that prove the intended route was the one taken."""
import glob
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build, edgefile
from tests import golden_util as gu
from tests.test_host import _file_tags

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")
ALL_HOST = {"DISCO_HOST_TEXT": "1", "DISCO_GPU_BINARY": "0", "DISCO_PAR_SIMPLE_HOST": "1"}
KNOBS = ("DISCO_HOST_TEXT", "DISCO_HOST_CONTAINED_TEXT", "DISCO_TEXT_VIA_HOST", "DISCO_LATE_ROWS", "DISCO_HOST_ROW_SORT", "DISCO_PAR_SIMPLE_HOST",
         "DISCO_PAR_SIMPLE_HOST_TEXT", "DISCO_PAR_SIMPLE_GPU_TEXT", "DISCO_GPU_BINARY", "DISCO_DIST_GPU_TEXT", "DISCO_PAR_SIMPLE")

C_FMT, C_WRITE = "format contained lines on the GPU", "contained lines into the files"
E_FMT, E_WRITE, E_FETCH = "format edge lines on the GPU", "edge lines into the files", "fetch edge lines"
BIN_GPU = ("binary contained records on the GPU", "binary edge records on the GPU")
BIN_HOST, FETCH_EDGES, CHAINS, PS_GPU = "write binary side output", "fetch edges", "contract chains on the GPU", "partial simplification: host rounds"
RANK_E = ("partition + format edge lines on the GPU", E_WRITE)
RANKS = ["--gpus", "2", "--same-device"]

# name: (flags, environment, threads, ranks, laps that must be there, laps that must not)
CASES = {
    "text-via-host": ([], {"DISCO_TEXT_VIA_HOST": "1"}, 3, 1, [C_FMT, E_FMT, E_FETCH], [E_WRITE, FETCH_EDGES]),
    "late-rows": ([], {"DISCO_LATE_ROWS": "1", "DISCO_HOST_CONTAINED_TEXT": "1"}, 3, 1, [E_FMT, E_WRITE], [C_FMT, C_WRITE]),
    "host-row-sort": ([], {"DISCO_HOST_ROW_SORT": "1", "DISCO_HOST_CONTAINED_TEXT": "1"}, 3, 1, [E_FMT, E_WRITE], [C_FMT, C_WRITE]),
    "binary-out+host-contained": (["--binary-out"], {"DISCO_HOST_CONTAINED_TEXT": "1"}, 3, 1, [BIN_HOST, E_FMT, E_FETCH, FETCH_EDGES], [C_FMT, E_WRITE, *BIN_GPU]),
    "binary-out+par-simple+gpu-binary": (["--binary-out", "--par-simple", "PS"], {"DISCO_GPU_BINARY": "1"}, 3, 1, [*BIN_GPU, C_FMT, E_FMT, E_WRITE, CHAINS, PS_GPU],
                                         [BIN_HOST, E_FETCH, FETCH_EDGES]),
    "binary-out+par-simple": (["--binary-out", "--par-simple", "PS"], {}, 3, 1, [BIN_HOST, E_FMT, E_FETCH, FETCH_EDGES, CHAINS, PS_GPU], [C_FMT, E_WRITE, *BIN_GPU]),
    "par-simple+mpi-names": (["--par-simple", "PS", "--mpi-names"], {}, 3, 1, [C_FMT, E_FMT, E_FETCH, FETCH_EDGES], [E_WRITE, CHAINS, PS_GPU, "partial simplification"]),
    "t300": ([], {}, 300, 1, [C_FMT, C_WRITE, FETCH_EDGES], [E_FMT, E_WRITE, E_FETCH]),
    "par-simple+gpu-text-0": (["--par-simple", "PS"], {"DISCO_PAR_SIMPLE_GPU_TEXT": "0"}, 3, 1, [C_FMT, E_FMT, E_FETCH, FETCH_EDGES, CHAINS], [E_WRITE, PS_GPU]),
    "ranks+host-contained": (RANKS, {"DISCO_DIST_GPU_TEXT": "1", "DISCO_HOST_CONTAINED_TEXT": "1"}, 3, 2, [f"rank {r}: {w}" for r in (0, 1) for w in RANK_E],
                             [C_FMT, C_WRITE, "partition edges into files"]),
    "ranks+t300": (RANKS, {"DISCO_DIST_GPU_TEXT": "1"}, 300, 2, [f"rank {r}: {w}" for r in (0, 1) for w in (C_FMT, C_WRITE)] + ["partition edges into files"], list(RANK_E)),
    "host-text-0": ([], {"DISCO_HOST_TEXT": "0"}, 3, 1, [FETCH_EDGES], [C_FMT, C_WRITE, E_FMT, E_WRITE, E_FETCH]),
}


def _run(tmp_path, how, flags, env_extra, threads):
    c = gu.CASES["multifile"]  # its records are filtered: file index != read id + 1
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {c['min_overlap']}\n")
    prefix, ps = str(tmp_path / how), str(tmp_path / (how + "_ps"))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(DISCO_VERBOSE="1", **env_extra)
    cmd = [os.path.join(BIN, "buildG"), "-pe", ",".join(os.path.join(gu.GOLD, f) for f in c["pe"]), "-se", ",".join(os.path.join(gu.GOLD, f) for f in c["se"]),
           "-f", prefix, "-p", str(cfg), "-t", str(threads)] + [ps if x == "PS" else x for x in flags]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout
    assert open(prefix + "_CheckpointInfo.txt").read() == "CCR=Complete\nGC=Complete\n"
    return p.stdout, prefix, ps


def _files(prefix, ps, flags, threads, gpus):
    """what a run left behind, in the form two runs are compared in: contained files and _contained.bin as bytes, edge and ParSimpleEdges files
    as sorted lines, _edges.bin as its header and its sorted records"""
    etags, ctags = _file_tags(threads, gpus, "--mpi-names" in flags)
    assert len(glob.glob(prefix + "_*_parGraph.txt")) == len(etags) and len(glob.glob(prefix + "_*_containedReads.txt")) == len(ctags)
    out = {"contained": [open(f"{prefix}_{t}_containedReads.txt", "rb").read() for t in ctags],
           "edges": [sorted(open(f"{prefix}_{t}_parGraph.txt", "rb").read().splitlines()) for t in etags]}
    assert os.path.exists(prefix + "_contained.bin") == os.path.exists(prefix + "_edges.bin") == ("--binary-out" in flags)
    if "--binary-out" in flags:
        out["contained.bin"] = open(prefix + "_contained.bin", "rb").read()
        rec, n_files = edgefile.read_edges(prefix + "_edges.bin")
        out["edges.bin"] = (open(prefix + "_edges.bin", "rb").read(32), n_files, np.sort(rec, order=list(edgefile.EDGE.names)).tobytes())
    ps_files = sorted(glob.glob(ps + "_*_ParSimpleEdges.txt"))
    if "--par-simple" in flags and "--mpi-names" not in flags:
        assert ps_files == sorted(f"{ps}_{t}_ParSimpleEdges.txt" for t in range(threads))
    else:
        assert not ps_files   # (--par-simple with --mpi-names on one GPU writes none)
    out["par-simple"] = [sorted(open(f, "rb").read().splitlines()) for f in ps_files]
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_a_route_of_the_matrix_writes_the_files_of_the_host_routes(tmp_path, case):
    build.build_host()
    flags, env, threads, gpus, laps_in, laps_out = CASES[case]
    out, prefix, ps = _run(tmp_path, "case", flags, env, threads)
    out_ref, prefix_ref, ps_ref = _run(tmp_path, "ref", flags, {**env, **ALL_HOST}, threads)
    for lap in laps_in:
        assert lap in out, (lap, out)
    for lap in laps_out:
        assert lap not in out, (lap, out)
    for lap in (C_FMT, E_FMT, *BIN_GPU, CHAINS, PS_GPU):   # the reference run went through the host, every file of it
        assert lap not in out_ref, (lap, out_ref)
    got, want = _files(prefix, ps, flags, threads, gpus), _files(prefix_ref, ps_ref, flags, threads, gpus)
    for kind in want:
        assert got[kind] == want[kind], kind
    assert sum(x.count(b"\n") for x in want["contained"]) > 50 and sum(len(x) for x in want["edges"]) > 50
    if "--par-simple" in flags and "--mpi-names" not in flags:
        assert sum(len(x) for x in want["par-simple"]) > 0
