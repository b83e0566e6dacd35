"""files that put record starts and newlines on the seams of the record-finding kernels of the device input stage (4096 bytes of text per
block, 16 per lane), for tests/test_gpu_ingest.py (one GPU) and tests/test_gpu_dist_ingest.py (the same files under a communicator)"""
import numpy as np

from oracle import pyoracle

EDGE_OFFSETS = (4095, 4096, 4097, 4111, 4112, 8192)
EDGE_DECLINED = "tiny"


def _edge_reads(rng, n):
    """reads of about 100 bases that the filter keeps, every seventh too short to be one"""
    return ["".join(rng.choice(list("ACGT"), 20 if i % 7 == 3 else int(rng.integers(95, 106)))) for i in range(n)]


def _padded(records, target, ends):
    """the records as one text whose first header line is padded until some value of ends(text) — positions that grow by one with
    every padding byte — equals target"""
    text = "".join(records)
    pad = min(target - e for e in ends(text) if e <= target)
    text = records[0][:1] + "p" * pad + "".join(records)[1:]
    assert target in ends(text)
    return text


def _record_starts(text, fastq):
    lines = text.split("\n")
    at, out = 0, []
    for i, ln in enumerate(lines):
        if at < len(text) and (i % 4 == 0 if fastq else ln.startswith(">")):
            out.append(at)
        at += len(ln) + 1
    return out[1:]  # (the first record is where the padding goes)


def edge_files(tmp_path):
    """name -> (path, fastq): a record's first byte at each of EDGE_OFFSETS, FASTQ newlines inside a record at 4095 and 4096, each with
    and without a final newline; FASTA files of exactly 4096 and 4097 bytes; a FASTA that ends in a lone '>'; EDGE_DECLINED: one record
    of fewer than 16 bytes. What each file is meant to hold is asserted here, from its bytes."""
    rng = np.random.default_rng(4096)
    reads = _edge_reads(rng, 100)
    fa = [f">r{i} d\n{s}\n" for i, s in enumerate(reads)]
    fq = []
    for i, s in enumerate(reads[:50]):
        q = "".join(rng.choice(list("@>IF#+"), len(s)))
        fq.append(f"@r{i} x\n{s}\n+\n{'@' if i % 2 else '>'}{q[1:]}\n")
    texts = {}
    for off in EDGE_OFFSETS:
        t = _padded(fa, off, lambda x: _record_starts(x, False))
        assert t[off] == ">" and t[off - 1] == "\n"
        texts[f"fasta_{off}"] = (t, False)
        t = _padded(fq, off, lambda x: _record_starts(x, True))
        assert t[off] == "@" and t[off - 1] == "\n" and t[:off].count("\n") % 4 == 0
        texts[f"fastq_{off}"] = (t, True)
    for off in (4095, 4096):  # a newline inside a record: behind its header, sequence or '+' line
        t = _padded(fq, off, lambda x: [i for i, ch in enumerate(x) if ch == "\n" and x[:i].count("\n") % 4 != 3])
        assert t[off] == "\n" and t[:off].count("\n") % 4 != 3
        texts[f"fastq_newline_{off}"] = (t, True)
    for name, (t, fastq) in list(texts.items()):
        assert t.endswith("\n")
        texts[name + "_no_final_newline"] = (t[:-1], fastq)
    for size in (4096, 4097):
        k = max(k for k in range(1, len(fa)) if len("".join(fa[:k])) <= size)
        t = _padded(fa[:k], size, lambda x: [len(x)])
        assert len(t) == size and t.endswith("\n") and t[:1] == ">"
        texts[f"fasta_size_{size}"] = (t, False)
    texts["fasta_lone_gt"] = ("".join(fa[:45]) + ">", False)
    texts[EDGE_DECLINED] = (">a\nACGTACGT\n", False)
    assert len(texts[EDGE_DECLINED][0]) < 16
    out = {}
    for name, (t, fastq) in texts.items():
        p = tmp_path / (name + (".fastq" if fastq else ".fasta"))
        p.write_bytes(t.encode())
        out[name] = (str(p), fastq)
    return out


def edge_want(path, min_overlap):
    want, wfidx, wtotal = pyoracle.load_good_reads([path], min_overlap)
    return want, np.asarray(wfidx, dtype=np.int64), wtotal
