"""CPU: a window of a BGZF file's text through disco_amd/bin/inflate_check --window LO N — the member choice (bgzf_window_members), the
rebased table (bgzf_rebase) and the clip that disco_inflate_bgzf_window and the ranks of disco_dist_ingest_fasta run, with the serial
byte sink: the output is text[lo:lo + n] for every window of tests/bgzf_windows.py, in every deflate setting, stored and compressed."""
import os
import subprocess

import pytest

from disco_amd import build
from tests import bgzf_util as bz
from tests import bgzf_windows as bw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "disco_amd", "bin", "inflate_check")


@pytest.fixture(scope="module")
def tool():
    build.build_host()
    assert os.path.exists(TOOL)
    return TOOL


def _window(tool, path, lo, n):
    return subprocess.run([tool, "--window", str(lo), str(n), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def check_windows(tool, path, text, bounds):
    wins = bw.windows(bounds, len(text))
    assert len(wins) > 60
    for lo, n in wins:
        r = _window(tool, path, lo, n)
        assert r.returncode == 0, (lo, n, r.stderr)
        assert r.stdout == text[lo:lo + n], (lo, n)
    return wins


@pytest.mark.parametrize("member,si", bw.FILES)
def test_every_window_is_the_slice_of_the_text(tool, tmp_path, member, si):
    data, text, bounds = bw.plain_file(member, si)
    assert len(bounds) >= 4 and (si != 0 or (data[18] & 6) == 0)  # level 0: stored members
    p = tmp_path / "w.gz"
    p.write_bytes(data)
    wins = check_windows(tool, p, text, bounds)
    B1 = bounds[bw.middle(bounds)]
    # from the list alone: the cases the clip must get right are in it
    assert any(B1 < lo and lo + n < B1 + member for lo, n in wins), "a window inside one member"
    assert {(B1 - 1, 1), (B1, 1), (0, 1), (len(text) - 1, 1)} <= set(wins), "windows of one byte"
    assert all(any(lo == B1 + d and n % 16 == e % 16 for lo, n in wins) for d in (-1, 0, 1) for e in (15, 0, 1)), "16-byte multiples and their neighbours"


def test_empty_members_inside_the_window_and_on_its_edges(tool, tmp_path):
    data, text, bounds = bw.file_with_empty_members()
    p = tmp_path / "e.gz"
    p.write_bytes(data)
    wins = check_windows(tool, p, text, bounds)
    # the empty members stand on B1 and B2 of the list: on a window's first byte, behind its last one, and inside it
    B1 = bounds[bw.middle(bounds)]
    assert {(B1, 700), (B1 - 1, 2), (B1, 1), (B1 + 699, 1), (B1 - 5, 1409)} <= set(wins)


def test_a_corrupt_member_counts_only_inside_the_window(tool, tmp_path):
    data, text, bounds = bw.plain_file(700, 2)
    off = bw.member_offsets(data)
    p = tmp_path / "c.gz"
    p.write_bytes(bw.corrupt_crc(data, off, 3))  # text bytes [2100, 2800)
    for lo, n, bad in ((2100, 700, True), (2799, 1, True), (2050, 100, True), (0, 2100, False), (2800, 900, False), (2099, 1, False), (2800, 1, False)):
        r = _window(tool, p, lo, n)
        if bad:
            assert r.returncode == 3 and r.stderr.startswith(b"block 3: CRC32"), (lo, n, r.stderr)
        else:
            assert r.returncode == 0 and r.stdout == text[lo:lo + n], (lo, n, r.stderr)
    assert subprocess.run([tool, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 3


def test_the_whole_file_mode_is_what_it_was(tool, tmp_path):
    data, text, _ = bw.plain_file(4096, 2)
    p = tmp_path / "f.gz"
    p.write_bytes(data)
    r = subprocess.run([tool, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == text
    assert subprocess.run([tool, "--window", "x", "1", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 2
    p.write_bytes(data[:-40])  # a chain that does not end with the file
    r = _window(tool, p, 0, 10)
    assert r.returncode == 3 and r.stderr.startswith(b"block "), r.stderr
