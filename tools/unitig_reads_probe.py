#!/usr/bin/env python3
"""wall and GB/s of the --unitig-reads / --unitig-depth stage (disco_write_unitig_reads) beside the --gfa-unitigs stage — the
contraction with every overlap counted (disco_contract_chains(0)) and disco_write_gfa_chains — of the same pass; the library's own line
(DISCO_VERBOSE) gives the rounds of doubling that moved a read and the time of the kernels that resolve, place and count apart from
the writes — the figures of profiles/unitig_reads.txt:
   python tools/unitig_reads_probe.py config3|metagenome|<n_reads> [--once] [DIR]
--once: one contraction and one disco_write_unitig_reads with the R lines, nothing else (the run to put under rocprofv3 --kernel-trace
--stats for the kernels' own times: utr_round_kernel, utr_count_kernel, the scans and utr_r_write_kernel, and cgrp_count_kernel beside
them — the run groups the contained rows once, unwritten, for that comparison); DIR: where the files go (removed afterwards); default:
a temporary one"""
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disco_amd import buildgraph  # noqa: E402
from tools.gfa_probe import spec_of  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if a != "--once"]
    once = "--once" in sys.argv[1:]
    shape = args[0]
    d = tempfile.mkdtemp(prefix="unitig_reads_probe_", dir=args[1] if len(args) > 1 else None)
    path = os.path.join(d, "g.out")

    def timed_write(write, **kw):
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        t = time.perf_counter()
        nb = write(fd, threads=16, **kw)
        dt = time.perf_counter() - t
        os.close(fd)
        assert os.path.getsize(path) == nb
        os.unlink(path)
        return nb, dt

    try:
        with buildgraph.BuildGraph(min_overlap=40) as g:
            g.generate_reads(spec_of(shape))
            t = time.perf_counter()
            g.run_graph()
            g.synchronize()
            c = g.counters()
            print(f"{shape}: {c['n_reads']} reads, {c['e_out']} edges, {c['n_contained']} contained; graph {time.perf_counter() - t:.3f} s", flush=True)
            if once and c["n_contained"]:   # cgrp_count_kernel into the same trace: one atomic per contained read to its container
                g._chk(g.L.disco_prepare_contained_records(g._h, 1, None))
            for rep in range(1 if once else 3):
                line = []
                nc, nl = C.c_uint64(), C.c_uint64()
                t = time.perf_counter()
                g._chk(g.L.disco_contract_chains(g._h, 0, C.byref(nc), C.byref(nl)))
                line.append(f"contract {nc.value} chains of {nl.value} links: {time.perf_counter() - t:.3f} s")
                if not once:
                    nb, dt = timed_write(g.write_gfa_chains)
                    line.append(f"unitigs gfa {nb} B: {dt:.3f} s ({nb / dt * 1e-9:.2f} GB/s)")
                print(f"  run {rep}: " + "; ".join(line), flush=True)
                os.environ["DISCO_VERBOSE"] = "1"   # the library's line: rounds, and the kernels before the first write
                for depth_only in (False,) if once else (False, True):
                    nb, dt = timed_write(g.write_unitig_reads, depth_only=depth_only)
                    print(f"  run {rep}: unitig {'depth' if depth_only else 'reads'} {nb} B: {dt:.3f} s ({nb / dt * 1e-9:.2f} GB/s)", flush=True)
                del os.environ["DISCO_VERBOSE"]
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
