"""the three generated read sets behind tests/golden/long_min_overlap.json (min-overlap 96, 120, 200): what the real reference wrote for
them is recorded there (tests/golden/make_long_min_overlap.py); the tests rebuild the reads from the parameters below."""
import json
import os

import numpy as np

from disco_amd import readgen

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_min_overlap.json")

# name -> (min-overlap, generator parameters). mo120 also carries 60 reads of 100 .. 120 bases (the last one of exactly 120), every 25th
# record of the file: the reference drops reads of at most min-overlap bases (BG/Dataset.cpp:305), so file index != read id + 1 there
SETS = {
    "mo96": (96, dict(seed=9601, n_reads=1500, read_len=150, cov=30.0)),
    "mo120": (120, dict(seed=12001, n_reads=1500, read_len=150, cov=30.0, len_max=250)),
    "mo200": (200, dict(seed=20001, n_reads=1500, read_len=250, cov=30.0)),
}
N_SHORT_120 = 60


def records(name):
    """the records of the set's FASTA file, in file order"""
    mo, kw = SETS[name]
    reads = readgen.generate_reads(readgen.GenSpec.coverage(**kw))
    if name != "mo120":
        return reads
    rng = np.random.default_rng(120)
    out = []
    for i, s in enumerate(reads):
        if i % 25 == 0:
            n = len(out) // 26
            L = 120 if n == N_SHORT_120 - 1 else int(rng.integers(100, 121))
            out.append(reads[int(rng.integers(0, len(reads)))][:L])
        out.append(s)
    return out


def write_fasta(name, path):
    readgen.write_fasta(path, records(name))
    return SETS[name][0]


def recorded():
    with open(GOLD) as f:
        return json.load(f)
