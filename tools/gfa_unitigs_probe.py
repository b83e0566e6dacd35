#!/usr/bin/env python3
"""wall and GB/s of the --gfa-unitigs stage — the contraction with every overlap counted (disco_contract_chains(0)) and the write
(disco_write_gfa_chains) — beside the --gfa step (disco_write_gfa) of the same pass, and the bytes the spelling kernel stores (the S lines
of the composite edges) — the figures of profiles/gfa_unitigs.txt:
   python tools/gfa_unitigs_probe.py config3|metagenome|<n_reads> [--once|--once-gfa] [DIR]
--once: one contraction and one write with the bases, nothing else; --once-gfa: one disco_write_gfa, nothing else (the two runs to put
under rocprofv3 --kernel-trace --stats for the kernels' own times: gfu_spell_kernel there, gfa_s_write_kernel here, and the bytes each
stores); DIR: where the files go (removed afterwards); default: a temporary one"""
import ctypes as C
import mmap
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disco_amd import buildgraph  # noqa: E402
from tools.gfa_probe import spec_of  # noqa: E402


def section_bytes(path, first=b"\nS\tc"):
    """the bytes of the file's S lines of composite edges (first = b"\\nS\\t": of all its S lines): from the first of them to the first L line"""
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        a = m.find(first)
        if a < 0:
            return 0
        b = m.find(b"\nL\t", a)
        return (len(m) - 1 if b < 0 else b) - a


SLINE = b"\nS\t"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--once")]
    once, once_gfa = "--once" in sys.argv[1:], "--once-gfa" in sys.argv[1:]
    shape = args[0]
    d = tempfile.mkdtemp(prefix="gfa_unitigs_probe_", dir=args[1] if len(args) > 1 else None)
    path = os.path.join(d, "g.gfa")

    def timed_write(write, **kw):
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        t = time.perf_counter()
        nb = write(fd, threads=16, **kw)
        dt = time.perf_counter() - t
        os.close(fd)
        assert os.path.getsize(path) == nb
        return nb, dt

    try:
        with buildgraph.BuildGraph(min_overlap=40) as g:
            g.generate_reads(spec_of(shape))
            t = time.perf_counter()
            g.run_graph()
            g.synchronize()
            c = g.counters()
            print(f"{shape}: {c['n_reads']} reads, {c['e_out']} edges, {c['n_contained']} contained; graph {time.perf_counter() - t:.3f} s", flush=True)
            for rep in range(1 if once or once_gfa else 3):
                line = []
                if not once:
                    nb, dt = timed_write(g.write_gfa)
                    line.append(f"gfa {nb} B{f', S lines {section_bytes(path, SLINE)} B' if once_gfa else ''}: {dt:.3f} s ({nb / dt * 1e-9:.2f} GB/s)")
                if once_gfa:
                    print(f"  run {rep}: " + "; ".join(line), flush=True)
                    break
                nc, nl = C.c_uint64(), C.c_uint64()
                t = time.perf_counter()
                g._chk(g.L.disco_contract_chains(g._h, 0, C.byref(nc), C.byref(nl)))
                line.append(f"contract {nc.value} chains of {nl.value} links: {time.perf_counter() - t:.3f} s")
                for no_seq in (False,) if once else (False, True):
                    nb, dt = timed_write(g.write_gfa_chains, no_seq=no_seq)
                    line.append(f"unitigs gfa{' no-seq' if no_seq else ''} {nb} B, chain S lines {section_bytes(path)} B: {dt:.3f} s ({nb / dt * 1e-9:.2f} GB/s)")
                    os.unlink(path)
                print(f"  run {rep}: " + "; ".join(line), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
