"""-m gpu : where a read table begins and how the input stage gives up (disco_amd/csrc/disco_hip.hip: begin_read_table, IngestJob) —
a declined disco_ingest_fasta gives back what it took and the context goes on; a refused upload between two layouts leaves no reads
and no long class behind; the generator's spec is checked by one check, whichever call hands it over."""
import numpy as np
import pytest

from disco_amd import buildgraph, readgen
from tests import bgzf_util as bz
from tests.test_gpu_two_class import mixed_reads
from tests.util import canon_hip

pytestmark = pytest.mark.gpu
DECLINED = "the host input stage takes this job"
POINTS = ["first_byte", "gt_inside_a_line", "bgzf_crc", "second_of_two_files", "text_beyond_the_arena"]


def _fasta(reads):
    return "".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)).encode()


def _graph(g):
    g.run_graph()
    return canon_hip(g.fetch_edges(), g.fetch_contained()), g.long_rows


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """the tail set as a FASTA, the five declining inputs, a fresh context's pass over the FASTA, and THE context the tests share"""
    d = tmp_path_factory.mktemp("read_table")
    tail = mixed_reads(61, 3000, 150, 150, 30.0, 0.03, 300, 900)
    assert 60 < sum(len(r) > 256 for r in tail) < 130
    text = _fasta(tail)
    good = d / "tail.fa"
    good.write_bytes(text)
    files = {}
    (d / "first.fa").write_bytes(b"X" + text[1:])  # (a) neither '>' nor '@': declined before any device memory is taken
    files["first_byte"] = [str(d / "first.fa")]
    lines = text.split(b"\n")
    lines[2001] = lines[2001][:70] + b">" + lines[2001][71:]  # (b) a '>' inside the sequence of record 1000: declined after the filter
    (d / "gt.fa").write_bytes(b"\n".join(lines))
    files["gt_inside_a_line"] = [str(d / "gt.fa")]
    mem = bz.bgzf_members(text, 65280)  # (c) the third member's CRC32: declined inside the inflate step
    assert len(mem) > 3
    m = bytearray(mem[2])
    m[-6] ^= 0x40
    (d / "crc.fa.gz").write_bytes(b"".join(mem[:2]) + bytes(m) + b"".join(mem[3:]) + bz.EOF_MEMBER)
    files["bgzf_crc"] = [str(d / "crc.fa.gz")]
    files["second_of_two_files"] = [str(good), str(d / "gt.fa")]  # (d) the first file's pieces are held when the second gives up
    # (e) a BGZF file whose text — 80 MB, one record over and over, a '>' inside the last sequence — is 90 times the file: the arena is
    # sized for five times the file plus 64 MB, so the text and its record arrays are pieces of their own, which the job has to free
    rec = b">r\n" + tail[0][:150].encode() + b"\n"
    big = rec * (80_000_000 // len(rec))
    big = big[:-80] + b">" + big[-79:]
    (d / "big.fa.gz").write_bytes(bz.bgzf_bytes(big, 65280, level=1))
    assert (d / "big.fa.gz").stat().st_size * 5 + (64 << 20) < len(big)
    files["text_beyond_the_arena"] = [str(d / "big.fa.gz")]
    with buildgraph.BuildGraph(min_overlap=40) as f:
        assert f.ingest_fasta([str(good)], threads=4) is not None
        want = _graph(f)
    assert want[1] == sum(len(r) > 256 for r in tail) > 0
    with buildgraph.BuildGraph(min_overlap=40) as g:
        yield {"g": g, "good": str(good), "files": files, "want": want}


@pytest.mark.parametrize("point", POINTS)
def test_a_declined_input_stage_gives_back_what_it_took(stage, point):
    """hbm_bytes after the second of two declines equals hbm_bytes after the first, whatever the context held before: the first call may
    grow the stage's arena and ask for a larger hit buffer (counted by the call that asks, ingest_choose_arena), the second adds nothing —
    the pieces a job took beyond the arena included (text_beyond_the_arena)."""
    g = stage["g"]
    hbm = []
    for _ in range(2):
        assert g.ingest_fasta(stage["files"][point], threads=4) is None
        assert g.last_error().endswith(DECLINED), g.last_error()
        hbm.append(g.counters()["hbm_bytes"])
    print(f"{point}: hbm_bytes after the first decline {hbm[0]}, after the second {hbm[1]}")
    # (the first call may create the stage's arena, which the context keeps on purpose: the second adds nothing)
    assert hbm[1] == hbm[0]


@pytest.mark.parametrize("point", POINTS)
def test_the_context_goes_on_after_a_decline(stage, point):
    g = stage["g"]
    assert g.ingest_fasta(stage["files"][point], threads=4) is None
    assert g.ingest_fasta([stage["good"]], threads=4) is not None
    (edges, rows), long_rows = _graph(g)
    (wedges, wrows), wlong = stage["want"]
    assert np.array_equal(edges, wedges) and np.array_equal(rows, wrows)
    assert long_rows == wlong > 0


@pytest.mark.parametrize("ragged", [False, True], ids=["strided", "back_to_back"])
def test_a_refused_upload_between_two_layouts(monkeypatch, ragged):
    monkeypatch.setenv("DISCO_UPLOAD_CHUNK", "256")  # twelve chunks: the ring of three staging buffers goes round
    tail = mixed_reads(61, 3000, 150, 150, 30.0, 0.03, 300, 900)
    pure = mixed_reads(62, 3000, 150, 150, 30.0, 0.0, 300, 300)
    with buildgraph.BuildGraph(min_overlap=40) as f:
        f.upload_ascii(pure, ragged=ragged)
        want = _graph(f)
    with buildgraph.BuildGraph(min_overlap=40) as g:
        g.upload_ascii(tail, ragged=ragged)
        assert g.long_rows > 0  # two classes of rows
        with pytest.raises(buildgraph.DiscoError, match="length outside"):
            g.upload_ascii(["ACGT" * 10], ragged=ragged)  # one read of min_overlap bases
        assert g.num_reads == 0 and g.long_rows == 0
        g.upload_ascii(pure, ragged=ragged)
        got = _graph(g)
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1])
    assert got[1] == want[1] == 0


def test_the_generator_spec_check_is_one_check():
    bad = [readgen.GenSpec(seed=1, n_reads=10, contig_len=100, n_contigs=1, len_min=150, len_max=150),
           readgen.GenSpec(seed=1, n_reads=10, contig_len=1000, n_contigs=0, len_min=150, len_max=150)]
    ranks = [buildgraph.BuildGraph(min_overlap=40) for _ in range(2)]
    try:
        buildgraph.BuildGraph.comm_init_local(ranks)
        with buildgraph.BuildGraph(min_overlap=40) as g:
            for spec in bad:
                with pytest.raises(buildgraph.DiscoError, match="bad spec") as single:
                    g.generate_reads(spec)
                for r in ranks:  # (the check comes before anything collective)
                    with pytest.raises(buildgraph.DiscoError, match="bad spec") as dist:
                        r.dist_generate_reads(spec)
                    assert str(dist.value) == str(single.value).replace("disco_generate_reads", "disco_dist_generate_reads")
                    assert "error -1:" in str(dist.value)  # DISCO_E_ARG
    finally:
        for r in ranks:
            r.close()
