"""what BGZF costs the input stage: buildG on one read set three ways — (a) plain FASTA through the device stage, (b) the same file as
BGZF through the device stage (bgzf_inflate_kernel), (c) the BGZF file through the host stage (DISCO_HOST_INPUT=1: one zlib stream) —
three runs each, interleaved, every run a child process under its own time limit; the first run that fails or runs out of time ends
the probe. A last run of (b) under `rocprofv3 --kernel-trace --stats` gives the inflate kernel's own time.

   python tools/bgzf_probe.py [N_READS=5000000] [OUT=profiles/bgzf_ingest.txt] [WORKDIR=/tmp/bgzf_probe]

The read set is disco_amd/bin/readgen's (150 bp, 30x); it is compressed at level 6 into members of 65280 bytes by at most 16 worker
processes, none of which opens the GPU."""
import glob
import os
import re
import shutil
import statistics
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "disco_amd", "bin")
MEMBER = 65280
GROUP = 256  # members per task of a worker


def _compress(args):
    from tests import bgzf_util as bz

    path, off, n = args
    with open(path, "rb") as f:
        f.seek(off)
        data = f.read(n)
    return b"".join(bz.bgzf_block(data[i:i + MEMBER], level=6) for i in range(0, len(data), MEMBER))


def write_bgzf(src, dst):
    from tests import bgzf_util as bz

    size = os.path.getsize(src)
    tasks = [(src, off, min(MEMBER * GROUP, size - off)) for off in range(0, size, MEMBER * GROUP)]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex, open(dst, "wb") as out:
        for piece in ex.map(_compress, tasks):
            out.write(piece)
        out.write(bz.EOF_MEMBER)


def run(cmd, env, limit):
    t0 = time.time()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=limit)
    return p.returncode, time.time() - t0, p.stdout


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bgzf_ingest.txt")
    work = sys.argv[3] if len(sys.argv) > 3 else "/tmp/bgzf_probe"
    os.makedirs(work, exist_ok=True)
    fa, gz, cfg = os.path.join(work, "r.fasta"), os.path.join(work, "r.fasta.gz"), os.path.join(work, "disco.cfg")
    open(cfg, "w").write("MinOverlap4BuildGraph = 40\n")
    subprocess.check_call([os.path.join(BIN, "readgen"), fa, str(n_reads), "150", "30"])
    t0 = time.time()
    write_bgzf(fa, gz)
    lines = [f"bgzf_probe: {n_reads} reads of 150 bp; FASTA {os.path.getsize(fa) / 1e6:.1f} MB, BGZF level 6 {os.path.getsize(gz) / 1e6:.1f} MB "
             f"(written in {time.time() - t0:.1f} s by the Python writer)"]
    ways = {"a plain, device stage": (fa, {}), "b BGZF, device stage": (gz, {}), "c BGZF, host stage": (gz, {"DISCO_HOST_INPUT": "1"})}
    walls = {k: [] for k in ways}
    laps = {k: [] for k in ways}
    ok = True
    for rep in range(3):
        for k, (path, extra) in ways.items():
            for f in glob.glob(os.path.join(work, "out_*")):
                os.remove(f)
            env = dict(os.environ, DISCO_VERBOSE="1", **extra)
            try:
                rc, wall, log = run([os.path.join(BIN, "buildG"), "-se", path, "-f", os.path.join(work, "out"), "-p", cfg, "-t", "16"], env, 300)
            except subprocess.TimeoutExpired:
                rc, wall, log = 124, 300.0, "time limit"
            if rc != 0:
                lines.append(f"run {rep} of ({k}) ended with status {rc}: the probe stops here\n{log[-2000:]}")
                ok = False
                break
            if ("input stage on the GPU" in log) != (not extra):
                lines.append(f"run {rep} of ({k}) took the other input stage\n{log[-2000:]}")
                ok = False
                break
            walls[k].append(wall)
            laps[k].append([l.strip() for l in log.splitlines() if re.search(r"input stage|BGZF|file reader|reads loaded|input:", l)])
        if not ok:
            break
    for k in ways:
        if walls[k]:
            lines.append(f"({k}) buildG wall s: {' '.join(f'{w:.2f}' for w in walls[k])}  median {statistics.median(walls[k]):.2f}")
            lines += ["      " + l for l in laps[k][-1]]
    if ok:
        ma, mb, mc = (statistics.median(walls[k]) for k in ways)
        lines.append(f"median (c) / median (b) = {mc / mb:.2f}; (b) - (a) = {mb - ma:+.2f} s")
        prof = os.path.join(work, "prof")
        shutil.rmtree(prof, ignore_errors=True)
        try:
            rc, wall, log = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "bgzf", "--", os.path.join(BIN, "buildG"), "-se", gz, "-f", os.path.join(work, "out"),
                                 "-p", cfg, "-t", "16"], dict(os.environ, DISCO_ORDERLY_EXIT="1"), 400)  # (buildG's _exit would take the profiler's output with it)
        except subprocess.TimeoutExpired:
            rc = 124
        stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
        if rc == 0 and stats:
            import csv

            for cols in csv.reader(open(stats[0])):
                if cols and "bgzf_inflate_kernel" in cols[0]:
                    row = ",".join(cols)
                    ns = float(cols[2])
                    lines.append(f"rocprofv3 --kernel-trace --stats: bgzf_inflate_kernel {ns / 1e6:.1f} ms for {os.path.getsize(fa) / 1e6:.1f} MB of text = "
                                 f"{os.path.getsize(fa) / ns:.2f} GB/s out")
                    lines.append("      " + row.strip())
        else:
            lines.append(f"the rocprofv3 run ended with status {rc}; no kernel statistics")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
