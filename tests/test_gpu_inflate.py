"""-m gpu : BGZF decoded on the device (disco_inflate_bgzf -> bgzf_inflate_kernel, one wavefront per member) against the bytes that
went in: every deflate block type and member shape of tests/test_inflate_host.py, arbitrary bytes, grids smaller and larger than
the device, and damaged files the host build of the same decoder has already classified."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from disco_amd import build, buildgraph
from tests import bgzf_util as bz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "disco_amd", "bin", "inflate_check")


@pytest.fixture(scope="module")
def g():
    with buildgraph.BuildGraph(min_overlap=40) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def text():
    return bz.fasta_text(5, 1600)  # about 280 KB


@pytest.mark.parametrize("member", bz.MEMBER_SIZES)
@pytest.mark.parametrize("si", range(len(bz.SETTINGS)))
def test_round_trip(g, text, si, member):
    assert g.inflate_bgzf(bz.bgzf_bytes(text, member, **bz.SETTINGS[si])) == text


def test_round_trip_of_odd_files(g, text):
    assert g.inflate_bgzf(bz.bgzf_bytes(text[:300], 1)) == text[:300]
    run = b">x\n" + b"A" * 60000 + b"\n"  # matches whose distance is below their length
    assert g.inflate_bgzf(bz.bgzf_bytes(run)) == run
    assert g.inflate_bgzf(bz.bgzf_bytes(text, 4096, eof=False)) == text
    mem = bz.bgzf_members(text, 4096)
    assert g.inflate_bgzf(b"".join(mem[:3]) + bz.EOF_MEMBER + mem[3] + bz.EOF_MEMBER * 2 + b"".join(mem[4:]) + bz.EOF_MEMBER) == text
    assert g.inflate_bgzf(bz.EOF_MEMBER) == b""


@pytest.mark.parametrize("level", [0, 6])
def test_arbitrary_bytes(g, level):
    raw = np.random.default_rng(41).integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    # (incompressible: 65280 bytes and deflate's framing would not fit a member's 16-bit size)
    assert g.inflate_bgzf(bz.bgzf_bytes(raw, 60000, level=level)) == raw
    # periods of every short length, and long matches far back
    rep = b"".join(bytes([65 + k % 7]) * k + raw[:k] for k in range(1, 300)) + raw[:20000] * 3
    assert g.inflate_bgzf(bz.bgzf_bytes(rep, 65280, level=level)) == rep


def test_size_only_few_members_and_many_members(g, text):
    data = bz.bgzf_bytes(text[:150_000], 65280)  # 3 members: most of the device idle
    L = buildgraph.load()
    assert L.disco_inflate_bgzf(g._h, data, len(data), None, 0) == 150_000
    out = bytes(10)
    assert L.disco_inflate_bgzf(g._h, data, len(data), out, 10) == -5  # DISCO_E_CAPACITY
    assert g.inflate_bgzf(data) == text[:150_000]
    many = bz.bgzf_bytes(text[:200_000], 100)  # 2000 members: more than the device holds waves of this kernel
    assert many.count(b"\x1f\x8b\x08\x04") >= 2001 and g.inflate_bgzf(many) == text[:200_000]


def test_what_is_not_bgzf_returns_none(g, text):
    assert g.inflate_bgzf(gzip.compress(text[:5000])) is None and "member 0" in g.last_error()
    assert g.inflate_bgzf(text[:5000]) is None
    assert g.inflate_bgzf(bz.bgzf_bytes(text[:5000])) == text[:5000]


def test_damaged_files_the_host_build_has_classified(g, text):
    """twenty of tests/bgzf_util.mutated_files (the 400 of tests/test_inflate_host.py, same generator and seed): ten the host build of
    the decoder refuses inside a member — damaged payload, CRC32 or ISIZE — and ten it accepts. The device must decide the same way,
    name the member, and decode a good file on the same context after every refusal. Error paths of bounds-checked code that has
    run on the host build; nothing here is meant to fault."""
    build.build_host()
    cases = bz.mutated_files()
    good = bz.bgzf_bytes(text[:70_000], 4096)
    refused, accepted = [], []
    for i, (kind, data) in enumerate(cases):
        if kind in ("payload", "crc", "isize") and len(refused) < 10:
            refused.append((i, kind, data))
        elif kind in bz.MUST_ACCEPT and len(accepted) < 10:
            accepted.append((i, kind, data))
    assert len(refused) == 10 and len(accepted) == 10

    def host(data):
        p = subprocess.run([TOOL, "/dev/stdin"], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        return p.returncode, p.stdout, p.stderr.decode()

    for i, kind, data in refused:
        rc, _out, err = host(data)
        assert rc == 3 and err.startswith("block "), (i, kind, rc, err)
        assert g.inflate_bgzf(data) is None, (i, kind)
        assert "member " + err.split()[1].rstrip(":") in g.last_error(), (i, kind, err, g.last_error())
        assert g.inflate_bgzf(good) == text[:70_000], (i, kind)
    for i, kind, data in accepted:
        rc, out, err = host(data)
        assert rc == 0 and out == gzip.decompress(data), (i, kind, err)
        assert g.inflate_bgzf(data) == out, (i, kind)
