#!/usr/bin/env python3
"""wall and GB/s of the GFA step (disco_write_gfa) beside the edge-text step of the same pass (disco_format_edges + disco_write_edge_text
into 16 files), with and without sequences — the figures of profiles/gfa.txt:
   python tools/gfa_probe.py config3|metagenome|<n_reads> [DIR]        DIR: where the files go (removed afterwards); default: a temporary one"""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disco_amd import buildgraph, readgen  # noqa: E402

BIG = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cases_big.json")))


def spec_of(shape):
    c = BIG["u150_50m" if shape == "config3" else "s100_250_10m"] if shape in ("config3", "metagenome") else dict(BIG["u150_50m"], reads=int(shape), n_contigs=max(int(shape) // 10 ** 6, 1))
    return readgen.GenSpec.coverage(c["seed"], c["reads"], c["read_len"], c["coverage"], n_contigs=c["n_contigs"], len_max=c.get("len_max", c["read_len"]), skew=c.get("skew", 0))


def main():
    shape = sys.argv[1]
    d = tempfile.mkdtemp(prefix="gfa_probe_", dir=sys.argv[2] if len(sys.argv) > 2 else None)
    try:
        with buildgraph.BuildGraph(min_overlap=40) as g:
            g.generate_reads(spec_of(shape))
            t = time.perf_counter()
            g.run_graph()
            g.synchronize()
            c = g.counters()
            print(f"{shape}: {c['n_reads']} reads, {c['e_out']} edges, {c['n_contained']} contained; graph {time.perf_counter() - t:.3f} s", flush=True)
            for rep in range(3):
                line = []
                files = g.fetch_edge_files(16)
                fds = [os.open(os.path.join(d, f"e{t_}.txt"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for t_ in range(16)]
                t = time.perf_counter()
                off = buildgraph.np.zeros(17, dtype=buildgraph.np.uint64)
                nb = g._chk(g.L.disco_format_edges(g._h, 16, files.ctypes.data, None, off.ctypes.data))
                t_fmt = time.perf_counter() - t
                g.write_edge_text(fds, threads=16)
                t_all = time.perf_counter() - t
                for fd in fds:
                    os.close(fd)
                line.append(f"edge text {nb} B: format {t_fmt:.3f} s, format + write {t_all:.3f} s ({nb / t_all * 1e-9:.2f} GB/s)")
                for no_seq in (False, True):
                    path = os.path.join(d, "g.gfa")
                    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                    t = time.perf_counter()
                    nb = g.write_gfa(fd, no_seq=no_seq, threads=16)
                    dt = time.perf_counter() - t
                    os.close(fd)
                    assert os.path.getsize(path) == nb
                    os.unlink(path)
                    line.append(f"gfa{' no-seq' if no_seq else ''} {nb} B: {dt:.3f} s ({nb / dt * 1e-9:.2f} GB/s)")
                print(f"  run {rep}: " + "; ".join(line), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
