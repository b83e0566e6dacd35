"""CPU: the self-delimiting survivor lists of the marking (disco_amd/csrc/disco_survivor.h, the header the kernels include) built for
the host as disco_amd/bin/survivor_check — every length 0..4 and wide round trips, the sentinel is no entry, and whatever an earlier pass
left behind the mark is never read."""
import os
import subprocess

from disco_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "disco_amd", "bin", "survivor_check")


def test_encode_and_decode_round_trip():
    build.build_host()
    assert os.path.exists(TOOL)
    r = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(b"ok ") and int(r.stdout.split()[1]) > 1_000_000
