#!/usr/bin/env python3
"""upper bound of what ordering the reads INSIDE a locus group by their start could buy, with no kernel change: take the processing order
a pass made (disco_fetch_order), re-order the reads of every order bucket on the host from the generator's true genome positions, and hand
the order back as a caller's order (disco_set_query_order -> order_pack_kernel). Every arm goes through the caller's-order path, so the
arms differ in the order alone:
   parent : the order as the pass made it (inside a bucket: whatever the LDS cursors gave)
   sorted : every bucket sorted by the true start of the read's span on the genome (either strand)
   q4     : every bucket sorted by start >> 3 only, ties as in `parent` — what a 4-bit sub-key (16 bins over the ~127 positions the reads
            of one group spread over) can give
   own    : the library's own grouping, once per round, for the level of the pass
usage: group_start_order_probe.py [--rounds 5] [--steps 5] [--out FILE] N_READS ...     (one line per arm and round, then medians)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from disco_amd import buildgraph, readgen  # noqa: E402

ORDER_MULT = 0x9E3779B1
args = sys.argv[1:]
rounds, steps, out_path = 5, 5, None
while args and args[0].startswith("--"):
    k = args.pop(0)
    if k == "--rounds":
        rounds = int(args.pop(0))
    elif k == "--steps":
        steps = int(args.pop(0))
    elif k == "--out":
        out_path = args.pop(0)
sizes = [int(a) for a in args] or [20_000_000]
out = open(out_path, "a") if out_path else None


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def neighbour_gap(ids, bucket_sorted, gpos):
    """median |start difference| of neighbours in processing order inside buckets of at least 8 reads"""
    b = bucket_sorted
    starts = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
    size = np.diff(np.r_[starts, len(b)])
    big = np.repeat(size >= 8, size)
    same = (b[1:] == b[:-1]) & big[1:]
    p = gpos[ids].astype(np.int64)
    return float(np.median(np.abs(np.diff(p))[same]))


torch.zeros(1, device="cuda")
for n in sizes:
    genome = int(n * 150 / 30)
    spec = readgen.GenSpec.coverage(42, n, 150, 30.0, n_contigs=max(1, genome // 5_000_000))
    g = buildgraph.BuildGraph(min_overlap=40)
    g.generate_reads(spec)
    g.run_graph()
    g.synchronize()
    order, keys, bits = g.fetch_order()
    ids = (order & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(n))
    bucket = (((keys.astype(np.uint64) * np.uint64(ORDER_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)).astype(np.int64)
    gpos = np.empty(n, dtype=np.int64)
    for a in range(0, n, 10_000_000):
        p, _, _ = readgen.read_locations(spec, a, min(a + 10_000_000, n))
        gpos[a:a + len(p)] = p.astype(np.int64)
    b_par = bucket[ids]
    assert np.all(np.diff(b_par) >= 0), "the buckets of the pass's order do not ascend"
    pos_in_parent = np.empty(n, dtype=np.int64)
    pos_in_parent[ids] = np.arange(n)
    all_ids = np.arange(n, dtype=np.int64)
    arms = {"parent": ids,
            "sorted": all_ids[np.lexsort((gpos, bucket))],
            "q4": all_ids[np.lexsort((pos_in_parent, gpos >> 3, bucket))]}
    say(f"== reads {n} rounds {rounds} steps {steps}  order bits {bits}  buckets in use {len(np.unique(bucket))}")
    for name, a in arms.items():
        assert np.array_equal(bucket[a], b_par) and np.array_equal(np.sort(a), all_ids)
        say(f"{name:8s} median start distance of neighbours inside buckets of >= 8 reads: {neighbour_gap(a, b_par, gpos):.1f} bases")
    dev = {name: torch.from_numpy(a).cuda() for name, a in arms.items()}
    dev["own"] = None
    torch.cuda.synchronize()
    rec = {name: [] for name in dev}
    for rnd in range(rounds):
        for name, t in dev.items():
            g.set_query_order(t.data_ptr() if t is not None else 0)
            g.run_graph()  # (warm-up: the first pass on an order)
            g.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                g.run_graph()
            g.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            ph, c = g.phase_ms(), g.counters()
            rec[name].append(dict(ph, **{"pass": ms}))
            say(f"{name:8s} pass {ms:7.2f}  " + " ".join(f"{k} {v:6.2f}" for k, v in ph.items() if v > 0.05) +
                f"  | e_pre {c['e_pre']} e_out {c['e_out']} contained {c['n_contained']} kmer_hits {c['kmer_hits']}")
    say(f"median (range) per arm, {n} reads")
    for name, rows in rec.items():
        def mr(k):
            v = sorted(r.get(k, 0.0) for r in rows)
            return f"{v[len(v) // 2]:.2f} ({v[0]:.2f}-{v[-1]:.2f})"
        say(f"{name:8s} pass {mr('pass')} | probe_kernel {mr('probe_kernel')} | verify {mr('verify')} | select {mr('select')} | trmark {mr('trmark')} | emit {mr('emit')}")
    g.set_query_order(0)
    g.close()
    del dev
    torch.cuda.empty_cache()
