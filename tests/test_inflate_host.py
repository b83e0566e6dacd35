"""CPU: the BGZF decode core of the device input stage (disco_amd/csrc/disco_inflate.h) built for the host as disco_amd/bin/inflate_check
— every deflate block type and member shape round trips, and damaged files are refused (exit 3) or read exactly as Python's gzip
reads them, never anything else."""
import gzip
import os
import subprocess
import zlib

import pytest

from disco_amd import build
from tests import bgzf_util as bz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "disco_amd", "bin", "inflate_check")


@pytest.fixture(scope="module")
def tool():
    build.build_host()
    assert os.path.exists(TOOL)
    return TOOL


@pytest.fixture(scope="module")
def text():
    return bz.fasta_text(5, 1600)  # about 280 KB: five members of 65280 bytes, the last one short


def _run(tool, tmp_path, data):
    p = tmp_path / "case.gz"
    p.write_bytes(data)
    return subprocess.run([tool, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def first_block_type(member):
    """BTYPE of a member's first deflate block (the writer's fixed 18-byte header)"""
    return (member[18] >> 1) & 3


def test_the_writer_writes_gzip_and_every_block_type(text):
    assert bz.bgzf_block(b"") == bz.EOF_MEMBER
    types = {}
    for si, s in enumerate(bz.SETTINGS):
        mem = bz.bgzf_members(text, 4096, **s)
        assert gzip.decompress(b"".join(mem) + bz.EOF_MEMBER) == text
        types[si] = {first_block_type(m) for m in mem[:-1]}
    assert types[0] == {0} and types[4] == {1} and all(types[i] == {2} for i in (1, 2, 3, 5, 6, 7)), types


@pytest.mark.parametrize("member", bz.MEMBER_SIZES)
@pytest.mark.parametrize("si", range(len(bz.SETTINGS)))
def test_round_trip(tool, tmp_path, text, si, member):
    r = _run(tool, tmp_path, bz.bgzf_bytes(text, member, **bz.SETTINGS[si]))
    assert r.returncode == 0, r.stderr
    assert r.stdout == text


def test_round_trip_of_odd_files(tool, tmp_path, text):
    cases = {
        "one byte per member": bz.bgzf_bytes(text[:300], 1),
        "one long run": bz.bgzf_bytes(b">x\n" + b"A" * 60000 + b"\n"),
        "no end-of-file member": bz.bgzf_bytes(text, 4096, eof=False),
    }
    mem = bz.bgzf_members(text, 4096)
    cases["empty members in the middle"] = b"".join(mem[:3]) + bz.EOF_MEMBER + mem[3] + bz.EOF_MEMBER * 2 + b"".join(mem[4:]) + bz.EOF_MEMBER
    want = {"one byte per member": text[:300], "one long run": b">x\n" + b"A" * 60000 + b"\n"}
    for name, data in cases.items():
        r = _run(tool, tmp_path, data)
        assert r.returncode == 0, (name, r.stderr)
        assert r.stdout == want.get(name, text), name
    # a member of 65280 bytes at level 6 holds more symbols than one block of zlib's: several deflate blocks without any help
    d = zlib.decompressobj(-15)
    payload = bz.bgzf_block(text[:65280])[18:-8]
    assert d.decompress(payload) == text[:65280] and len(payload) > 12000


def test_what_is_not_bgzf_is_refused(tool, tmp_path, text):
    for name, data in {"plain gzip": gzip.compress(text[:5000]), "empty": b"", "text": text[:3000]}.items():
        r = _run(tool, tmp_path, data)
        assert r.returncode == 3 and r.stderr.startswith(b"block 0: "), (name, r.returncode, r.stderr)


def test_damaged_files_are_refused_or_read_as_gzip_reads_them(tool, tmp_path):
    """400 damaged files (tests/bgzf_util.mutated_files) against Python's gzip on the same bytes: exit 0 only with the judge's bytes,
    otherwise exit 3; damage no BGZF reader looks at must be accepted; refusing what the judge accepts is held to 2 % of the other cases"""
    cases = bz.mutated_files()
    assert len(cases) == 400 and {k for k, _ in cases} == set(bz.MUTATIONS)
    stricter, others = [], 0
    for i, (kind, data) in enumerate(cases):
        try:
            judge = gzip.decompress(data)
        except (OSError, EOFError, zlib.error):
            judge = None
        r = _run(tool, tmp_path, data)
        assert r.returncode in (0, 3), (i, kind, r.returncode, r.stderr)
        if r.returncode == 0:
            assert judge is not None and r.stdout == judge, (i, kind)
        else:
            assert r.stderr.startswith(b"block "), (i, kind, r.stderr)
        if kind in bz.MUST_ACCEPT:
            assert r.returncode == 0, (i, kind, r.stderr)
        else:
            others += 1
            if r.returncode == 3 and judge is not None:
                stricter.append((i, kind, r.stderr.decode().strip()))
    print(f"refused although gzip reads it: {len(stricter)} of {others} cases {stricter}")
    assert len(stricter) <= 0.02 * others
