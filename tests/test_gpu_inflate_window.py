"""-m gpu : a window of a BGZF buffer's text decoded on the device (disco_inflate_bgzf_window -> bgzf_inflate_kernel with a text window:
the members that hold the window are decoded whole, the first and the last one stored from / up to the window's edge) — every window
of tests/bgzf_windows.py, the list the host tool is held to (tests/test_inflate_window_host.py), equals the slice of the text, and
nothing is written around the region handed to the library."""
import numpy as np
import pytest

from disco_amd import buildgraph
from tests import bgzf_windows as bw

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, 0xA5
E_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def g():
    with buildgraph.BuildGraph(min_overlap=40) as ctx:
        yield ctx


def _window(g, data, lo, n):
    """(return value, the region handed to the library, guards intact) over a sentinel-filled buffer with GUARD bytes on either side"""
    buf = np.full(n + 2 * GUARD, SENTINEL, dtype=np.uint8)
    got = g.L.disco_inflate_bgzf_window(g._h, data, len(data), lo, n, buf.ctypes.data + GUARD)
    return got, buf[GUARD:GUARD + n].tobytes(), bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all())


def check_windows(g, data, text, bounds):
    wins = bw.windows(bounds, len(text))
    assert len(wins) > 60
    for i, (lo, n) in enumerate(wins):
        got, region, guards = _window(g, data, lo, n)
        want = text[lo:lo + n]
        assert got == len(want), (lo, n, got, g.last_error())
        assert region[:got] == want, (lo, n)
        assert guards and region[got:] == bytes([SENTINEL]) * (n - got), (lo, n, "written outside the window")
        if i % 8 == 0:  # the mirror, on a part of the list
            assert g.inflate_bgzf_window(data, lo, n) == want, (lo, n)


@pytest.mark.parametrize("member,si", bw.FILES)
def test_every_window_is_the_slice_of_the_text(g, member, si):
    data, text, bounds = bw.plain_file(member, si)
    check_windows(g, data, text, bounds)
    assert g.inflate_bgzf(data) == text


def test_empty_members_inside_the_window_and_on_its_edges(g):
    data, text, bounds = bw.file_with_empty_members()
    check_windows(g, data, text, bounds)
    assert g.inflate_bgzf(data) == text


def test_a_corrupt_member_is_named_by_its_number_in_the_file_and_only_inside_the_window(g):
    data, text, _ = bw.plain_file(700, 2)
    bad = bw.corrupt_crc(data, bw.member_offsets(data), 3)  # member 3: text bytes [2100, 2800)
    for lo, n in ((2100, 700), (2799, 1), (2050, 100), (2500, 3000), (0, len(text))):
        got, region, guards = _window(g, bad, lo, n)
        assert got == E_UNSUPPORTED and guards and region == bytes([SENTINEL]) * n, (lo, n, got)
        assert "member 3:" in g.last_error() and "CRC32" in g.last_error(), g.last_error()
        assert g.inflate_bgzf_window(bad, lo, n) is None
    for lo, n in ((0, 2100), (2800, 900), (2099, 1), (2800, 1), (2800, len(text))):
        got, region, guards = _window(g, bad, lo, n)
        want = text[lo:lo + n]
        assert got == len(want) and region[:got] == want and guards, (lo, n, got, g.last_error())
    assert g.inflate_bgzf(bad) is None and "member 3" in g.last_error()
    assert g.inflate_bgzf(data) == text


def test_what_is_not_bgzf_and_the_size_query(g):
    import gzip

    data, text, _ = bw.plain_file(4096, 4)
    assert g.inflate_bgzf_window(gzip.compress(text[:5000]), 0, 10) is None and "member 0" in g.last_error()
    assert g.inflate_bgzf_window(data[:-40], 0, 10) is None and "BSIZE" in g.last_error()
    L = g.L
    assert L.disco_inflate_bgzf_window(g._h, data, len(data), 100, 50, None) == 50
    assert L.disco_inflate_bgzf_window(g._h, data, len(data), len(text) - 7, 50, None) == 7
    assert L.disco_inflate_bgzf_window(g._h, data, len(data), len(text), 50, None) == 0
    assert g.inflate_bgzf_window(data, 100, 50) == text[100:150]
