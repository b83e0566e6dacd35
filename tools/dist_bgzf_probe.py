"""what BGZF costs the input stage of a multi-GPU job: buildG --gpus 4 --same-device on one read set three ways — (a) plain FASTA through
the ranks' device stage (DISCO_DIST_DEVICE_INPUT=1), (b) the same file as BGZF with DISCO_DIST_BGZF=1: every rank decodes its share of
the members on the GPU, (c) the BGZF file without that knob: the ranks decline and the host stage reads one zlib stream — three runs
each, interleaved, every run a child process under its own time limit; the first run that fails or runs out of time ends the probe.

   python tools/dist_bgzf_probe.py [N_READS=5000000] [OUT=profiles/dist_bgzf.txt] [WORKDIR=/tmp/dist_bgzf_probe]

The expectation the result is held to: the median of (b) lies below the median of (c) by more than the spread (max - min) of (c)'s
three runs. Four ranks on ONE device share one decoder, one link and one host: what (b) gains with a GPU per rank is not measured here.
The read set and the BGZF writer are those of tools/bgzf_probe.py."""
import glob
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bgzf_probe import BIN, run, write_bgzf  # noqa: E402

GPUS = 4


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "dist_bgzf.txt")
    work = sys.argv[3] if len(sys.argv) > 3 else "/tmp/dist_bgzf_probe"
    os.makedirs(work, exist_ok=True)
    fa, gz, cfg = os.path.join(work, "r.fasta"), os.path.join(work, "r.fasta.gz"), os.path.join(work, "disco.cfg")
    open(cfg, "w").write("MinOverlap4BuildGraph = 40\n")
    subprocess.check_call([os.path.join(BIN, "readgen"), fa, str(n_reads), "150", "30"])
    t0 = time.time()
    write_bgzf(fa, gz)
    lines = [f"dist_bgzf_probe: buildG --gpus {GPUS} --same-device, {n_reads} reads of 150 bp; FASTA {os.path.getsize(fa) / 1e6:.1f} MB, BGZF level 6 "
             f"{os.path.getsize(gz) / 1e6:.1f} MB (written in {time.time() - t0:.1f} s by the Python writer)"]
    dev = {"DISCO_DIST_DEVICE_INPUT": "1"}
    ways = {"a plain, device stage on the ranks": (fa, dev, True), "b BGZF, device stage on the ranks (DISCO_DIST_BGZF=1)": (gz, dict(dev, DISCO_DIST_BGZF="1"), True),
            "c BGZF without the knob: host stage": (gz, dev, False)}
    walls = {k: [] for k in ways}
    laps = {k: [] for k in ways}
    ok = True
    for rep in range(3):
        for k, (path, extra, on_ranks) in ways.items():
            for f in glob.glob(os.path.join(work, "out_*")):
                os.remove(f)
            env = {name: v for name, v in os.environ.items() if name != "DISCO_DIST_BGZF"}  # (the knob only where the way sets it)
            env.update(DISCO_VERBOSE="1", **extra)
            cmd = [os.path.join(BIN, "buildG"), "-se", path, "-f", os.path.join(work, "out"), "-p", cfg, "-t", "16", "--gpus", str(GPUS), "--same-device"]
            try:
                rc, wall, log = run(cmd, env, 300)
            except subprocess.TimeoutExpired:
                rc, wall, log = 124, 300.0, "time limit"
            if rc != 0:
                lines.append(f"run {rep} of ({k}) ended with status {rc}: the probe stops here\n{log[-2000:]}")
                ok = False
                break
            got = sum(f"input stage on rank {r} of {GPUS}" in log for r in range(GPUS))
            if got != (GPUS if on_ranks else 0) or ("the host input stage takes this job" in log) == on_ranks:
                lines.append(f"run {rep} of ({k}) took the other input stage\n{log[-2000:]}")
                ok = False
                break
            walls[k].append(wall)
            laps[k].append([l.strip() for l in log.splitlines() if re.search(r"input stage|BGZF|reads loaded|input:", l)])
        if not ok:
            break
    for k in ways:
        if walls[k]:
            lines.append(f"({k}) buildG wall s: {' '.join(f'{w:.2f}' for w in walls[k])}  median {statistics.median(walls[k]):.2f}")
            lines += ["      " + l for l in laps[k][-1]]
    if ok:
        ma, mb, mc = (statistics.median(walls[k]) for k in ways)
        spread = max(walls[list(ways)[2]]) - min(walls[list(ways)[2]])
        held = mc - mb > spread
        lines.append(f"median (c) - median (b) = {mc - mb:+.2f} s, spread of (c) = {spread:.2f} s: the expectation (b below c by more than c's spread) "
                     f"{'holds' if held else 'DOES NOT hold'}; (b) - (a) = {mb - ma:+.2f} s")
        lines.append(f"({GPUS} ranks on one device share one decoder, one link and one host: this says nothing about a GPU per rank)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
