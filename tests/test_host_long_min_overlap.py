"""-m gpu : buildG with MinOverlap4BuildGraph = 120 in its parameter file (every context it creates carries DISCO_FLAG_SEEDED_KMER): 1560
records of 100 .. 250 bases, 60 of them of at most 120 — the files of the oracle and of the real reference (tests/golden/long_min_overlap.json)
through the device input stage, the host's, the binary side output and two ranks."""
import glob
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build, edgefile
from oracle import pyoracle, refrun
from tests import long_min_overlap_sets as sets

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(build.HERE), "disco_amd", "bin")
WAYS = {
    "device input": ([], {}),
    "host input": ([], {"DISCO_HOST_INPUT": "1"}),
    "no-text": (["--no-text"], {}),
    "two ranks": (["--gpus", "2", "--same-device"], {}),
}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("mo120")
    fa = str(d / "r.fasta")
    mo = sets.write_fasta("mo120", fa)
    reads, fidx, total = pyoracle.load_good_reads([fa], mo)
    ce, cc, _ = pyoracle.oracle_canonical(reads, fidx, mo)
    return dict(fasta=fa, mo=mo, total=total, good=len(reads), edges=ce, contained=cc)


@pytest.mark.parametrize("way", list(WAYS))
def test_min_overlap_120(tmp_path, case, way):
    build.build_host()
    extra, env_extra = WAYS[way]
    r = sets.recorded()["mo120"]
    cfg = tmp_path / "disco.cfg"
    cfg.write_text(f"MinOverlap4BuildGraph = {case['mo']}\n")
    prefix = str(tmp_path / "g")
    env = dict(os.environ, **env_extra)
    if not env_extra:
        env.pop("DISCO_HOST_INPUT", None)
    p = subprocess.run([os.path.join(BIN, "buildG"), "-se", case["fasta"], "-f", prefix, "-p", str(cfg), "-t", "4"] + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "MinOverlap4BuildGraph = 120" in p.stdout
    if "--no-text" in extra:  # the file lists exist, empty: the binary pair stands for them
        assert all(os.path.getsize(f) == 0 for f in glob.glob(prefix + "_*_parGraph.txt") + glob.glob(prefix + "_*_containedReads.txt"))
        for name, text in edgefile.text_files(prefix).items():
            with open(name, "w") as f:
                f.write(text)
    ce = refrun.parse_pargraph(sorted(glob.glob(prefix + "_*_parGraph.txt")))
    cc = refrun.parse_contained(sorted(glob.glob(prefix + "_*_containedReads.txt")))
    assert np.array_equal(cc, case["contained"]), f"{way}: contained rows differ ({len(cc)} vs {len(case['contained'])})"
    assert np.array_equal(ce, case["edges"]), f"{way}: edge list differs ({len(ce)} vs {len(case['edges'])})"
    assert (len(ce), len(cc)) == (r["n_edges"], r["n_contained"])
    assert pyoracle.digest(pyoracle.edges_text(ce)) == r["edges_sha256"] and pyoracle.digest(pyoracle.contained_text(cc)) == r["contained_sha256"]
    # the records of at most 120 bases are gone, as the reference drops them: ids are file indices, and the counts are the reference's
    assert (case["total"], case["good"]) == (r["n_records"], r["n_good"]) == (1560, 1500)
    assert f"{r['n_good']} good reads" in p.stdout.replace(",", ""), p.stdout
