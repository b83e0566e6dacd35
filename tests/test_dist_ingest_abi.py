"""CPU: include/disco_hip.h declares the collective input stage — disco_dist_ingest_fasta and disco_dist_ingest_fetch — with the
prototypes its comment documents, in plain C99 (a host written in C binds the header as it is)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNIT = r"""
#include "disco_hip.h"

typedef int (*ingest_fn)(disco_ctx *, const char *const *, int, uint32_t, disco_dist_ingest_info *, disco_ingest_file *);
typedef int (*fetch_fn)(disco_ctx *, uint16_t *, uint64_t *);

ingest_fn the_ingest = disco_dist_ingest_fasta;
fetch_fn the_fetch = disco_dist_ingest_fetch;

/* what a caller reads off the info struct */
uint64_t kept(const disco_dist_ingest_info *i) { return i->kept_reads + i->share_reads + i->home_hi - i->home_lo + i->n_reads + i->world; }
"""


def test_the_collective_input_stage_is_declared_for_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "unit.c"
    src.write_text(UNIT)
    p = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "#define DISCO_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "disco_hip.h")).read()  # a new struct, no existing one changed
