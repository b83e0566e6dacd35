"""CPU: the C restatement (oracle/) is a valid yardstick above min-overlap 95 — it reproduces what the REAL reference wrote for three
generated sets (min-overlap 96, 120, 200; tests/golden/long_min_overlap.json, recorded by tests/golden/make_long_min_overlap.py), and a
live run of the reference where its binary is built. The reference hashes k-mers of any length (BG/HashTable.cpp:396-416)."""
import numpy as np
import pytest

from oracle import pyoracle, refrun
from tests import long_min_overlap_sets as sets


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_oracle_reproduces_the_reference(name, tmp_path):
    r = sets.recorded()[name]
    fa = str(tmp_path / "r.fasta")
    mo = sets.write_fasta(name, fa)
    assert mo == r["min_overlap"]
    reads, fidx, total = pyoracle.load_good_reads([fa], mo)
    assert (total, len(reads)) == (r["n_records"], r["n_good"])
    assert all(len(s) > mo for s in reads)
    if name == "mo120":  # the records of at most 120 bases, one of exactly 120 among them, are what the filter dropped
        rec = sets.records(name)
        assert sum(len(s) <= mo for s in rec) == total - len(reads) == sets.N_SHORT_120 and any(len(s) == mo for s in rec)
    ce, cc, cnt = pyoracle.oracle_canonical(reads, fidx, mo)
    assert (len(ce), len(cc)) == (r["n_edges"], r["n_contained"]) and len(ce) > 100 and len(cc) > 50
    assert pyoracle.digest(pyoracle.edges_text(ce)) == r["edges_sha256"]
    assert pyoracle.digest(pyoracle.contained_text(cc)) == r["contained_sha256"]
    assert cnt["asymmetric_pairs"] == 0 and cnt["cap_bind_sites"] == 0  # inside the order-independent parity domain
    if refrun.available():
        ref = refrun.run_reference([fa], mo, threads=1, workdir=str(tmp_path))
        assert np.array_equal(ce, ref["edges"]) and np.array_equal(cc, ref["contained"])
