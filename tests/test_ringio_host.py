"""CPU: the host's end of the output ring (disco_amd/csrc/disco_ringio.h, the header the library delivers every piece with) built for the
host as disco_amd/bin/ringio_check — a segment split among writers lands at its offset of a sentinel-filled file and changes nothing around
it, at 0, 1, 65 535, 65 536, 65 537, 3 * 4096 + 1 and 5 MB + 3 bytes with 1, 2, 16, 64 and 100 threads; the same into memory; a piece of
several segments, some empty, with a writer each; a descriptor opened read-only is reported and nothing crashes."""
import os
import subprocess

from disco_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "disco_amd", "bin", "ringio_check")


def test_segments_land_where_they_belong(tmp_path):
    build.build_host()
    assert os.path.exists(TOOL)
    r = subprocess.run([TOOL, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(b"ok ") and int(r.stdout.split()[1]) > 10_000_000
    assert os.listdir(tmp_path) == []  # the program removes what it made
