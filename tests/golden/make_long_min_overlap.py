#!/usr/bin/env python3
"""Record what the REAL reference buildG (oracle/_ref/buildG_ref, `make -C oracle ref`) writes for the three read sets of
tests/long_min_overlap_sets.py — min-overlap 96, 120 and 200, above what the index of disco_amd holds as one k-mer — into
tests/golden/long_min_overlap.json: counts and sha256 of the canonical edge and contained texts (oracle/pyoracle.digest), and the good
reads the reference kept. -t 1: the reference's output is a function of the input there.

usage: make_long_min_overlap.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import pyoracle, refrun  # noqa: E402
from tests import long_min_overlap_sets as sets  # noqa: E402


def main():
    assert refrun.available(), "build the reference first: make -C oracle ref"
    out = {}
    for name in sets.SETS:
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "r.fasta")
            mo = sets.write_fasta(name, fa)
            ref = refrun.run_reference([fa], mo, threads=1, workdir=d)
            assert ref["returncode"] == 0, ref["log"]
            (good,) = [int(line.split()[0]) for line in ref["log"].splitlines() if "good reads in all datasets" in line]
            out[name] = dict(min_overlap=mo, n_records=len(sets.records(name)), n_edges=int(len(ref["edges"])), n_contained=int(len(ref["contained"])),
                             edges_sha256=pyoracle.digest(pyoracle.edges_text(ref["edges"])),
                             contained_sha256=pyoracle.digest(pyoracle.contained_text(ref["contained"])),
                             n_good=good, reference="oracle/_ref/buildG_ref -se <generated fasta> -t 1")
            print(name, out[name])
    with open(sets.GOLD, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
